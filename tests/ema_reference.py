"""Shared by tests/test_ema_cpu.py and tests/test_ema_gpu.py (docs/ema.md): the CPU twins of the EMA entry points behind numpy /
torch-CPU arguments, the same arithmetic restated operation by operation in numpy and Python doubles, and the replay of a run of
weight snapshots through the twins that the device results are compared with."""
import ctypes

import numpy as np
import torch

SIZES = (1, 3, 4, 5, 255, 256, 1023, 1025, 4099)        # float4 body and scalar tail; one block and several
DECAYS = (0.5, 0.999, 0.9999)


def aligned_f32(n, fill=None):
    """A float32 array of n elements whose first byte is 16-byte aligned (the entry points refuse anything else)."""
    raw = np.zeros(n + 4, dtype=np.float32)
    skip = (-raw.ctypes.data % 16) // 4
    out = raw[skip:skip + n]
    assert out.ctypes.data % 16 == 0
    if fill is not None:
        out[:] = fill
    return out


def values(rng, n):
    """Magnitudes 1e-3 .. 1, both signs: normal fp32 numbers whose differences and products stay normal or are exactly zero."""
    mag = np.exp(rng.uniform(np.log(1e-3), 0.0, size=n))
    return (mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


def _ptr(a):
    if a is None:
        return None
    return a.data_ptr() if torch.is_tensor(a) else a.ctypes.data


def tick_host(state, derived, guard=None):
    from hoig_amd import _lib as L
    return L.lib.hoig_ema_tick_host(_ptr(state), _ptr(derived), _ptr(guard))


def update_host(ema, param, n, derived, guard=None):
    from hoig_amd import _lib as L
    return L.lib.hoig_ema_update_host(_ptr(ema), _ptr(param), n, _ptr(derived), _ptr(guard))


def py_tick(decay, warmup, t):
    """(the fp32 weight 1 - beta of update number t, the count afterwards) in Python doubles"""
    beta = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return np.float32(1.0 - beta), t + 1.0


def numpy_update(ema, param, w):
    """e + (p - e) * w, every operation rounded to fp32 on its own"""
    assert ema.dtype == param.dtype == np.float32 and type(w) is np.float32
    diff = param - ema
    prod = diff * w
    return ema + prod


def replay(ema0, snapshots, decay, warmup, updates=0, skipped=()):
    """The twins over a run of weight snapshots (CPU float32 tensors): -> (average, update count).  `skipped`: indices of steps a
    guard skipped (the twins are called with skip = 1 there)."""
    n = ema0.numel()
    ema = ema0.clone()                       # (torch's CPU blocks are 64-byte aligned)
    assert ema.data_ptr() % 16 == 0 and ema.dtype == torch.float32
    state = np.array([decay, 1.0 if warmup else 0.0, float(updates)], dtype=np.float64)
    derived = np.zeros(1, dtype=np.float32)
    for i, p in enumerate(snapshots):
        guard = np.array([1.0, 1.0 if i in skipped else 0.0], dtype=np.float32)
        assert p.data_ptr() % 16 == 0 and p.dtype == torch.float32 and p.numel() == n and p.is_contiguous()
        assert tick_host(state, derived, guard) == 0
        assert update_host(ema, p, n, derived, guard) == 0
    return ema, int(state[2])
