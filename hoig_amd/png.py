"""PNG files encoded on the device (hoig_png_encode_u8; docs/png_encode.md).

``encode_u8(batch)`` takes a uint8 [B, H, W, C] device tensor (C = 3 or 1) and returns one ``bytes`` per image: ordinary PNG that
Pillow and libpng read back to exactly the input.  The three kernels run on the current stream; the host then copies ``sizes`` (the
one synchronising copy) and the used prefix of each image's slot into pinned memory -- the compressed bytes, not the raw pixels.
``encode_u8_host`` gives the same bytes from a host array through the CPU twin.  A missing kernel is an error, nothing falls back."""
import numpy as np

from . import _lib as L

SEGMENT_BYTES = L.PNG_SEGMENT_BYTES


def _sizes(h, w, c, segment_bytes, b):
    stride = L.lib.hoig_png_encode_bound(h, w, c, segment_bytes)
    L.check(min(stride, 0), 'hoig_png_encode_bound')
    ws = L.lib.hoig_png_encode_workspace_bytes(b, h, w, c, segment_bytes)
    L.check(min(ws, 0), 'hoig_png_encode_workspace_bytes')
    return stride, ws


def encode_u8(batch, segment_bytes=0):
    """The PNG files of a uint8 [B, H, W, C] CUDA tensor, in batch order."""
    import torch
    if not (torch.is_tensor(batch) and batch.is_cuda and batch.dtype == torch.uint8 and batch.dim() == 4):
        raise ValueError('encode_u8: a uint8 [B,H,W,C] CUDA tensor expected')
    batch = batch.contiguous()
    b, h, w, c = batch.shape
    if b == 0:
        return []
    stride, ws_bytes = _sizes(h, w, c, segment_bytes, b)
    with torch.cuda.device(batch.device):
        out = torch.empty(b * stride, dtype=torch.uint8, device=batch.device)
        sizes = torch.empty(b, dtype=torch.int32, device=batch.device)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=batch.device)
        L.call('hoig_png_encode_u8', batch.data_ptr(), b, h, w, c, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), ws_bytes,
               segment_bytes, torch.cuda.current_stream().cuda_stream)
        n = sizes.cpu().tolist()
        host = torch.empty(sum(n), dtype=torch.uint8).pin_memory()
        at = 0
        for i, k in enumerate(n):
            host[at:at + k].copy_(out[i * stride:i * stride + k], non_blocking=True)
            at += k
        torch.cuda.current_stream().synchronize()
    data = host.numpy().tobytes()
    ends = np.cumsum(n).tolist()
    return [data[e - k:e] for e, k in zip(ends, n)]


def encode_u8_host(batch, segment_bytes=0):
    """The same files from a uint8 [B, H, W, C] host array through the CPU twin (hoig_png_encode_host)."""
    a = np.ascontiguousarray(batch)
    if a.dtype != np.uint8 or a.ndim != 4:
        raise ValueError('encode_u8_host: a uint8 [B,H,W,C] array expected')
    b, h, w, c = a.shape
    if b == 0:
        return []
    stride, _ = _sizes(h, w, c, segment_bytes, b)
    out = np.empty(b * stride, np.uint8)
    sizes = np.zeros(b, np.int32)
    L.call('hoig_png_encode_host', a.ctypes.data, b, h, w, c, out.ctypes.data, stride, sizes.ctypes.data, segment_bytes)
    return [out[i * stride:i * stride + int(k)].tobytes() for i, k in enumerate(sizes)]
