"""One dispatcher for the entry points that have a CPU twin (`<name>_host`, same arguments without workspace and stream): the
metric modules call the device kernel on a device tensor and the twin on a CPU tensor through it."""
import ctypes

import torch

from . import _lib as L


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run(name, ref, args, workspace_bytes=None, tail=()):
    """The device entry on `ref`'s device and current stream -- `args`, then `tail`, then (workspace, workspace_bytes) of a buffer
    made here when a size is given, then the stream -- or the host twin with `args` alone for a CPU tensor."""
    if not ref.is_cuda:
        L.call(name + '_host', *args)
        return
    with torch.cuda.device(ref.device):
        ws = ()
        if workspace_bytes is not None:
            if workspace_bytes < 0:
                raise ValueError('%s: no workspace for these sizes' % name)
            buf = torch.empty((workspace_bytes + 7) // 8 + 1, dtype=torch.float64, device=ref.device)
            ws = (ptr(buf), workspace_bytes)
        L.call(name, *(tuple(args) + tuple(tail) + ws + (torch.cuda.current_stream().cuda_stream,)))
