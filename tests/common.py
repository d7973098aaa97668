"""Shared builders for the parity tests (test infrastructure)."""
import os
import numpy as np
import torch

from oracle import hogan_oracle as O
from hoig_amd import synthetic
from hoig_amd.options import opt_namespace  # noqa: F401  (re-exported for the tests)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEEDS = dict(G=8, D=9, VGG=10, inputs=8)
OUT_NAMES = ['fake_src_bg', 'fake_tsf_bg', 'fake_src_imgs', 'fake_tsf_imgs', 'fake_masks_bg', 'fake_masks_hand']


def seeded_state(gen_name, dataset='hov3'):
    cfg = O.make_cfg(gen_name, dataset)
    sdG = O.make_weights(O.gen_param_shapes(cfg), seed=SEEDS['G'], mode='random')
    sdD = O.make_weights(O.disc_param_shapes(cfg), seed=SEEDS['D'], mode='random')
    sdV = O.make_weights(O.vgg_param_shapes(), seed=SEEDS['VGG'], kind='vgg')
    return cfg, sdG, sdD, sdV


def oracle_trainer(gen_name, batch, side, dataset='hov3'):
    cfg, sdG, sdD, sdV = seeded_state(gen_name, dataset)
    ot = O.OracleTrainer(cfg, sdG, sdD, sdV)
    ot.set_prepared_input(synthetic.make_inputs(batch, side, seed=SEEDS['inputs'], dataset=dataset))
    return ot


def product_trainer(gen_name, batch, side, dataset='hov3', use_ddp=False, inputs=None, **over):
    from hoig_amd.models import ModelsFactory
    cfg, sdG, sdD, sdV = seeded_state(gen_name, dataset)
    opt = opt_namespace(gen_name=gen_name, dataset_mode=dataset, **over)
    m = ModelsFactory.get_by_name('trainer', opt, use_ddp=use_ddp)
    m._G.load_state_dict(sdG)
    m._D.load_state_dict(sdD)
    m._crt_tsf.vgg.load_state_dict(sdV)
    m.set_input(inputs if inputs is not None else synthetic.make_inputs(batch, side, seed=SEEDS['inputs'], dataset=dataset))
    return m


class _GoldenParts(dict):
    """The arrays of a fixture stored as <name>.part<i>.npz pieces (every committed file stays under 1 MiB), read as one."""

    @property
    def files(self):
        return list(self)


def load_golden(name):
    path = os.path.join(GOLDEN_DIR, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    import glob
    parts = sorted(glob.glob(path[:-len('.npz')] + '.part*.npz'))
    if not parts:
        raise FileNotFoundError(path)
    out = _GoldenParts()
    for p in parts:
        with np.load(p, allow_pickle=False) as z:
            out.update((k, z[k]) for k in z.files)
    return out


def line_digests(path):
    """64-bit digests (uint64, in file order) of the non-trivial lines of a Python file: stripped, 12 characters or more, not a
    comment or an import (test_data_cpu.py compares the package's loader files with the reference's through these)."""
    import hashlib
    out = []
    for line in open(path):
        line = line.strip()
        if len(line) >= 12 and not line.startswith(('#', 'import ', 'from ')):
            out.append(int.from_bytes(hashlib.sha1(line.encode()).digest()[:8], 'little'))
    return np.array(out, dtype=np.uint64)


# ---- rasteriser test helpers (oracle/raster.c through ctypes; test infrastructure) ----
def oracle_rasterize(faces, image_size=256, near=0.1, far=100.0):
    """faces (B,F,3,3) CPU tensor -> (fim int32 (B,S,S), wim (B,S,S,3)) by the plain-C oracle."""
    import ctypes
    import numpy as np
    import torch
    lib = ctypes.CDLL(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, 'oracle', '_build', 'libhoig_oracle_c.so'))
    f = np.ascontiguousarray(faces.numpy(), dtype=np.float32)
    B, F = f.shape[0], f.shape[1]
    S = image_size
    fim = np.empty((B, S, S), np.int32)
    wim = np.empty((B, S, S, 3), np.float32)
    inv = np.empty((B, F, 9), np.float32)
    vp = ctypes.c_void_p
    lib.oracle_rasterize_fim_wim.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, vp,
                                             vp, vp]
    lib.oracle_rasterize_fim_wim(f.ctypes.data, B, F, S, near, far, fim.ctypes.data, wim.ctypes.data, inv.ctypes.data)
    return torch.from_numpy(fim), torch.from_numpy(wim)


def synthetic_mesh_faces(batch, n_random=1500, seed=5):
    """(B,F,3,3) face tensors in the rasteriser's input convention (x, y in [-1,1], y up, z = depth): a rotated, lumpy UV
    sphere (closed surface: back faces, depth order, shared edges) plus random triangles of all sizes, some partly or fully
    outside the image, some beyond near / far, some degenerate."""
    import numpy as np
    import torch
    out = []
    for b in range(batch):
        g = np.random.default_rng([seed, b])
        nu, nv = 48, 24
        u = np.linspace(0, 2 * np.pi, nu, endpoint=False)
        v = np.linspace(0.05, np.pi - 0.05, nv)
        uu, vv = np.meshgrid(u, v)
        r = 0.55 + 0.08 * np.sin(3 * uu) * np.sin(2 * vv)
        P = np.stack([r * np.sin(vv) * np.cos(uu), r * np.cos(vv), r * np.sin(vv) * np.sin(uu)], -1).reshape(-1, 3)
        a = g.uniform(0, 2 * np.pi, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        P = P @ Rx.T @ Ry.T + np.array([g.uniform(-0.3, 0.3), g.uniform(-0.3, 0.3), 2.7])
        idx = []
        for j in range(nv - 1):
            for i in range(nu):
                p00, p01 = j * nu + i, j * nu + (i + 1) % nu
                p10, p11 = (j + 1) * nu + i, (j + 1) * nu + (i + 1) % nu
                idx += [(p00, p10, p01), (p01, p10, p11)]
        sphere = P[np.array(idx)]
        c = g.uniform(-1.3, 1.3, size=(n_random, 1, 2))
        size = g.choice([0.01, 0.05, 0.2, 0.8], size=(n_random, 1, 1))
        xy = c + g.uniform(-1, 1, size=(n_random, 3, 2)) * size
        z = g.uniform(0.05, 5.0, size=(n_random, 3, 1)) * g.choice([1.0, 1.0, 1.0, 40.0], size=(n_random, 1, 1))
        rnd = np.concatenate([xy, z], -1)
        if n_random >= 20:
            rnd[:10, 1] = rnd[:10, 0]                               # degenerate (two equal vertices)
            rnd[10:20, :, 2] = 1.5                                  # coplanar depth ties among overlapping faces
            rnd[10:20, :, :2] = g.uniform(-0.2, 0.2, size=(1, 3, 2)) + g.uniform(-0.01, 0.01, size=(10, 3, 2))
        out.append(np.concatenate([sphere, rnd], 0).astype(np.float32))
    return torch.from_numpy(np.stack(out))


def raster_boxes_host(faces, image_size):
    """faces (..., 3, 3) float32 array or tensor -> the packed tile boxes (uint32, one per face) of the rasteriser's setup stage by
    its CPU twin (hoig_raster_face_boxes_host: hoig_amd/csrc/raster_box.h, the function raster_setup_kernel calls)."""
    from hoig_amd import _lib as L
    f = np.ascontiguousarray(faces.numpy() if torch.is_tensor(faces) else faces, dtype=np.float32).reshape(-1, 9)
    out = np.empty(f.shape[0], np.uint32)
    if not len(out):
        return out
    L.call('hoig_raster_face_boxes_host', f.ctypes.data, f.shape[0], int(image_size), out.ctypes.data)
    return out


def pixel_centre(i, S):
    """The rasteriser's own coordinate of pixel i (rasterize_cuda_kernel.cu:112-113): (2 i + 1 - S) / S in double, rounded to fp32."""
    return ((2.0 * np.asarray(i, np.float64) + 1 - S) / S).astype(np.float32)


def sliver_faces(S, n, seed, on_centres=True):
    """(n,3,3) float32 slivers: faces whose two long edges differ in direction by a few ulps, so that both edge tests round to 'not
    outside' along the line through the face (docs/raster_parity.md).  Two vertices on pixel centres, a step of {-2..2}^2 times 2..9 pixels apart
    (or, on_centres=False, at arbitrary points of such a line through one pixel centre), one end sometimes outside the image; the third on the
    segment at a fraction in [0.05, 0.5], nudged by -2..+2 ulps on one coordinate; vertex order permuted; depths in [1, 3]."""
    g = np.random.default_rng([seed, S, int(on_centres)])
    step = g.integers(-2, 3, size=(n, 2))
    step[(step == 0).all(1)] = (1, 2)
    step = step * g.integers(2, 10, size=(n, 1))
    i0 = g.integers(-3, S + 3, size=(n, 2))
    if on_centres:
        v0, v1 = pixel_centre(i0, S), pixel_centre(i0 + step, S)
    else:                       # on the lattice line through pixel i0, at real multiples of the step: off it by their own rounding
        c = (2.0 * i0 + 1 - S) / S
        v0 = (c + g.uniform(-0.9, -0.1, size=(n, 1)) * step * (2.0 / S)).astype(np.float32)
        v1 = (c + g.uniform(0.1, 0.9, size=(n, 1)) * step * (2.0 / S)).astype(np.float32)
    t = g.uniform(0.05, 0.5, size=(n, 1)).astype(np.float32)
    v2 = (v0 + t * (v1 - v0)).astype(np.float32)
    axis, ulps = g.integers(0, 2, size=n), g.integers(-2, 3, size=n)
    for k in (1, 2):                                                  # |ulps| steps of nextafter on the chosen coordinate
        sel = np.abs(ulps) >= k
        v2[sel, axis[sel]] = np.nextafter(v2[sel, axis[sel]], np.where(ulps[sel] > 0, np.float32(np.inf), np.float32(-np.inf)))
    xy = np.stack([v0, v1, v2], 1)
    order = np.argsort(g.uniform(size=(n, 3)), axis=1)
    xy = np.take_along_axis(xy, order[:, :, None], axis=1)
    z = g.uniform(1.0, 3.0, size=(n, 3, 1)).astype(np.float32)
    return np.concatenate([xy, z], -1).astype(np.float32)
