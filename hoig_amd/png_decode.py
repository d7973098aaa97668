"""PNG files decoded on the device (hoig_png_decode_u8; docs/png_decode.md).

``parse(data)`` walks the chunks of one file on the host and returns ``(plan, None)``, or ``(None, reason)`` for a file outside the
supported set (the caller decodes that one with Pillow); it never raises on a foreign file.  ``decode_u8(files, device)`` takes the
bytes of B files of one size and returns the uint8 [B, H, W, 3] device tensor that ``np.asarray(Image.open(f).convert('RGB'))`` gives
for each, byte for byte (``bgr=True``: the channels reversed): the compressed bytes are what crosses to the device, two kernels run on
the current stream, and the one synchronising copy is that of the status words.  ``decode_u8_host`` gives the same array through the
CPU twin.  A missing kernel is an error, nothing falls back."""
import ctypes
import struct

import numpy as np

from . import _lib as L

SIGNATURE = b'\x89PNG\r\n\x1a\n'
STATUS_BITS = ((L.PNG_ECODE, 'invalid or over-subscribed code'), (L.PNG_EBTYPE, 'reserved block type'),
               (L.PNG_ESTORED, 'stored block LEN / NLEN mismatch'), (L.PNG_EDIST, 'distance in front of the stream'),
               (L.PNG_EEARLY, 'data ends early'), (L.PNG_EMORE, 'more output than the image holds'),
               (L.PNG_ELESS, 'less output than the image holds'), (L.PNG_EFILTER, 'filter type above 4'),
               (L.PNG_EADLER, 'Adler-32 mismatch'))
_DEPTHS = {0: (1, 2, 4, 8), 2: (8,), 3: (1, 2, 4, 8), 4: (8,), 6: (8,)}
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def status_text(status):
    """The names of the HOIG_PNG_E* bits of one status word."""
    return ', '.join(t for b, t in STATUS_BITS if status & b) or 'ok'


class Plan(object):
    """One parsed file: the header fields, the concatenated IDAT payloads (one zlib stream) and the PLTE payload."""
    __slots__ = ('width', 'height', 'color_type', 'bit_depth', 'stream', 'palette')

    def __init__(self, width, height, color_type, bit_depth, stream, palette):
        self.width, self.height, self.color_type, self.bit_depth = width, height, color_type, bit_depth
        self.stream, self.palette = stream, palette

    @property
    def filtered_bytes(self):
        return self.height * (1 + (self.width * _CHANNELS[self.color_type] * self.bit_depth + 7) // 8)


def parse(data):
    """(Plan, None) of a file the device decodes, or (None, reason).  Chunk CRC-32s are not checked on this path."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        return None, 'not a PNG file'
    at, ihdr, palette, idat, ended, after_idat = 8, None, None, [], False, False
    while at < len(data):
        if at + 8 > len(data):
            return None, 'truncated file'
        n, kind = struct.unpack('>I4s', data[at:at + 8])
        if at + 12 + n > len(data):
            return None, 'truncated file'
        body = data[at + 8:at + 8 + n]
        at += 12 + n
        if ihdr is None:
            if kind != b'IHDR' or n != 13:
                return None, 'no IHDR chunk in front'
            ihdr = struct.unpack('>IIBBBBB', body)
            continue
        if kind == b'IHDR':
            return None, 'a second IHDR chunk'
        if kind == b'IDAT':
            if after_idat:
                return None, 'IDAT chunks are not consecutive'
            idat.append(body)
        elif kind == b'IEND':
            ended = True
            break
        else:
            if idat:
                after_idat = True
            if kind == b'PLTE':
                if palette is not None or idat:
                    return None, 'a misplaced PLTE chunk'
                palette = body
            elif kind == b'tRNS':
                return None, 'a tRNS chunk'
            elif kind in (b'acTL', b'fcTL', b'fdAT'):
                return None, 'an animated file (APNG)'
            elif not kind[0:1].islower():
                return None, 'an unknown critical chunk'
    if ihdr is None or not ended or not idat:
        return None, 'truncated file'
    width, height, depth, ctype, compression, filt, interlace = ihdr
    if width < 1 or height < 1 or compression != 0 or filt != 0:
        return None, 'an invalid IHDR chunk'
    if interlace != 0:
        return None, 'an interlaced file'
    if depth == 16:
        return None, 'a 16-bit file'
    if ctype not in _DEPTHS or depth not in _DEPTHS[ctype]:
        return None, 'colour type %d at %d bits' % (ctype, depth)
    if ctype == 3:
        if palette is None:
            return None, 'no PLTE chunk'
        if len(palette) % 3 or not 3 <= len(palette) <= 768:
            return None, 'a short or invalid PLTE chunk'
    else:
        palette = None
    stream = idat[0] if len(idat) == 1 else b''.join(idat)
    if len(stream) < 2 or stream[0] & 15 != 8 or stream[0] >> 4 > 7 or (stream[0] * 256 + stream[1]) % 31 or stream[1] & 32:
        return None, 'an invalid zlib header'
    plan = Plan(width, height, ctype, depth, stream, palette)
    if plan.filtered_bytes >= 1 << 31 or len(stream) >= 1 << 31:
        return None, 'a filtered stream of 2^31 bytes or more'
    return plan, None


class PlanStruct(ctypes.Structure):
    """hoig_png_decode_plan"""
    _fields_ = [('data_off', ctypes.c_int64), ('out_off', ctypes.c_int64), ('pal_off', ctypes.c_int64), ('filt_off', ctypes.c_int64),
                ('data_len', ctypes.c_int32), ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('color_type', ctypes.c_int32),
                ('bit_depth', ctypes.c_int32), ('pal_entries', ctypes.c_int32), ('reserved', ctypes.c_int32 * 2)]


def _pad16(n):
    return (n + 15) // 16 * 16


def pack(items):
    """(bytes uint8 array, PlanStruct array, output bytes, workspace bytes) of a list of Plans: every stream and palette at a
    16-byte-aligned offset of one buffer, the results back to back in batch order, the workspace laid out by the library."""
    plans = (PlanStruct * len(items))()
    at = out = 0
    for p, it in zip(plans, items):
        p.data_off, p.data_len, at = at, len(it.stream), at + _pad16(len(it.stream))
        p.pal_off, p.pal_entries = (at, len(it.palette) // 3) if it.palette is not None else (0, 0)
        at += _pad16(len(it.palette)) if it.palette is not None else 0
        p.width, p.height, p.color_type, p.bit_depth = it.width, it.height, it.color_type, it.bit_depth
        p.out_off, out = out, out + it.width * it.height * 3
    buf = np.zeros(max(at, 16), np.uint8)
    for p, it in zip(plans, items):
        buf[p.data_off:p.data_off + p.data_len] = np.frombuffer(it.stream, np.uint8)
        if it.palette is not None:
            buf[p.pal_off:p.pal_off + len(it.palette)] = np.frombuffer(it.palette, np.uint8)
    ws = L.lib.hoig_png_decode_workspace_bytes(plans, len(items))
    L.check(min(ws, 0), 'hoig_png_decode_workspace_bytes')
    return buf, plans, out, max(ws, 16)


def _plans_of(files_bytes):
    items = []
    for i, data in enumerate(files_bytes):
        plan, reason = parse(data)
        if plan is None:
            raise ValueError('decode_u8: file %d is outside the supported set: %s' % (i, reason))
        items.append(plan)
    sizes = {(p.height, p.width) for p in items}
    if len(sizes) > 1:
        raise ValueError('decode_u8: images of one call differ in size: %s' % ', '.join('%dx%d' % (w, h) for h, w in sorted(sizes)))
    return items


def _raise_on_status(status):
    bad = [(i, int(s)) for i, s in enumerate(status) if s]
    if bad:
        raise ValueError('decode_u8: bad stream in ' + '; '.join('file %d (%s)' % (i, status_text(s)) for i, s in bad))


def decode_plans_u8(items, device, bgr=False, statuses=None):
    """decode_u8 on Plans already parsed (one size).  With a list for `statuses` a bad stream does not raise: the status words are
    appended to it, and an image with a status has an unspecified slot."""
    import torch
    device = torch.device(device)
    buf, plans, out_bytes, ws_bytes = pack(items)
    n = len(items)
    with torch.cuda.device(device):
        host = torch.from_numpy(buf).pin_memory()
        dev_bytes = host.to(device, non_blocking=True)
        plans_host = torch.from_numpy(np.frombuffer(bytes(plans), np.uint8).copy()).pin_memory()
        plans_dev = plans_host.to(device, non_blocking=True)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=device)
        status = torch.empty(n, dtype=torch.int32, device=device)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        L.call('hoig_png_decode_u8', dev_bytes.data_ptr(), dev_bytes.numel(), plans, plans_dev.data_ptr(), n, out.data_ptr(), out_bytes,
               status.data_ptr(), ws.data_ptr(), ws_bytes, int(bool(bgr)), torch.cuda.current_stream().cuda_stream)
        if statuses is None:
            _raise_on_status(status.cpu().tolist())
        else:
            statuses.extend(status.cpu().tolist())
    return out.view(n, items[0].height, items[0].width, 3)


def decode_u8(files_bytes, device, bgr=False):
    """uint8 [B, H, W, 3] on `device` of the bytes of B PNG files of one size (ValueError otherwise, or for a file outside the supported
    set, or -- with status_text of its status -- for a bad stream)."""
    import torch
    if len(files_bytes) == 0:
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device)
    return decode_plans_u8(_plans_of(files_bytes), device, bgr)


def decode_u8_host(files_bytes, bgr=False):
    """The same array on the host through the CPU twin (hoig_png_decode_host)."""
    if len(files_bytes) == 0:
        return np.empty((0, 0, 0, 3), np.uint8)
    items = _plans_of(files_bytes)
    buf, plans, out_bytes, ws_bytes = pack(items)
    out = np.empty(out_bytes, np.uint8)
    status = np.zeros(len(items), np.int32)
    ws = np.empty(ws_bytes, np.uint8)
    L.call('hoig_png_decode_host', buf.ctypes.data, buf.size, plans, len(items), out.ctypes.data, out_bytes, status.ctypes.data,
           ws.ctypes.data, ws_bytes, int(bool(bgr)))
    _raise_on_status(status.tolist())
    return out.reshape(len(items), items[0].height, items[0].width, 3)
