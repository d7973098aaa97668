"""CPU: the plain-C rasteriser oracle (oracle/raster.c, a restatement of neural_renderer's forward_face_index_map kernels,
rasterize_cuda_kernel.cu:40-186, PARITY UNPINNED against the CUDA original) checked against geometric ground truth: coverage of
known triangles, barycentric weights that reproduce the pixel, depth order and its index-order tie-break, back-face and
near/far culling, the wrapper's vertical flip and -1 / 0 fill."""
import numpy as np
import torch

from common import oracle_rasterize, synthetic_mesh_faces

S = 64


def tri(x0, y0, x1, y1, x2, y2, z=2.0):
    return [[x0, y0, z], [x1, y1, z], [x2, y2, z]]


def test_coverage_weights_and_flip():
    # counter-clockwise (x right, y up) = front side (rasterize_cuda_kernel.cu:55); upper-left quadrant
    f = torch.tensor([[tri(-0.9, 0.1, -0.1, 0.1, -0.9, 0.9)]], dtype=torch.float32)
    fim, wim = oracle_rasterize(f, S)
    rows, cols = np.nonzero(fim[0].numpy() == 0)
    assert len(rows) > 200
    assert rows.max() < S // 2 and cols.max() < S // 2          # y up -> top rows after the wrapper's vertical flip
    assert (fim[0][S // 2:] == -1).all() and (wim[0][fim[0] == -1] == 0).all()
    # the weights are the pixel's barycentric coordinates: sum_k w_k * vertex_k = pixel centre (normalised coordinates)
    w = wim[0][rows, cols].numpy()
    np.testing.assert_allclose(w.sum(1), 1.0, atol=1e-6)
    verts = f[0, 0, :, :2].numpy()
    xy = w @ verts
    xp = (2.0 * cols + 1 - S) / S
    yp = (2.0 * (S - 1 - rows) + 1 - S) / S                      # undo the flip
    np.testing.assert_allclose(xy[:, 0], xp, atol=2e-5)
    np.testing.assert_allclose(xy[:, 1], yp, atol=2e-5)
    # pixel count ~ triangle area (0.8 * 0.8 / 2 of a 2 x 2 square)
    assert abs(len(rows) - 0.32 / 4 * S * S) < 0.1 * 0.32 / 4 * S * S


def test_depth_order_ties_and_culling():
    big = tri(-0.8, -0.8, 0.8, -0.8, 0.0, 0.8)
    near_f = [[v[0], v[1], 1.0] for v in big]
    far_f = [[v[0], v[1], 3.0] for v in big]
    back = [big[0], big[2], big[1]]                              # clockwise: back side
    fim, _ = oracle_rasterize(torch.tensor([[far_f, near_f]], dtype=torch.float32), S)
    assert set(np.unique(fim.numpy())) == {-1, 1}                # the nearer face wins wherever both cover
    fim, _ = oracle_rasterize(torch.tensor([[near_f, far_f]], dtype=torch.float32), S)
    assert set(np.unique(fim.numpy())) == {-1, 0}
    fim, _ = oracle_rasterize(torch.tensor([[far_f, far_f]], dtype=torch.float32), S)
    assert set(np.unique(fim.numpy())) == {-1, 0}                # equal depth: the first face in index order (strict <)
    fim, _ = oracle_rasterize(torch.tensor([[back]], dtype=torch.float32), S)
    assert (fim == -1).all()                                     # back side culled
    behind = [[v[0], v[1], 0.05] for v in big]                   # z <= near
    beyond = [[v[0], v[1], 150.0] for v in big]                  # z >= far
    fim, _ = oracle_rasterize(torch.tensor([[behind, beyond]], dtype=torch.float32), S)
    assert (fim == -1).all()
    fim, _ = oracle_rasterize(torch.tensor([[beyond]], dtype=torch.float32), S, far=200.0)
    assert (fim == 0).any()


def test_mesh_is_watertight_and_consistent():
    f = synthetic_mesh_faces(1, n_random=0)
    fim, wim = oracle_rasterize(f, 128)
    cov = (fim[0] >= 0)
    assert 0.05 < cov.float().mean() < 0.5
    # a closed surface: the silhouette has no pin holes (every covered pixel's 4-neighbourhood is mostly covered)
    c = cov.float()
    inner = c[1:-1, 1:-1] * c[:-2, 1:-1] * c[2:, 1:-1] * c[1:-1, :-2] * c[1:-1, 2:]
    assert inner.sum() > 0.8 * c.sum()
    # every winning face is front-facing and its interpolated depth is the smallest among the faces covering the pixel:
    # spot-check 50 pixels by brute force in float64
    ys, xs = np.nonzero(cov.numpy())
    g = np.random.default_rng(0)
    F = f[0].double().numpy()
    for k in g.choice(len(ys), 50, replace=False):
        y, x = ys[k], xs[k]
        xp, yp = (2.0 * x + 1 - 128) / 128, (2.0 * (127 - y) + 1 - 128) / 128
        w = wim[0, y, x].double().numpy()
        fa = F[int(fim[0, y, x])]
        np.testing.assert_allclose(w @ fa[:, :2], [xp, yp], atol=1e-4)


def test_vertex_stage_matches_reference_fixture():
    """hoig_amd.raster.project_to_faces (pure torch, runs on CPU tensors too) against the fixture made by the reference's own
    projection / look_at / vertices_to_faces (tests/golden/make_golden_raster_vertex.py)."""
    import os
    from hoig_amd import raster
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'raster_vertex_stage.npz'))
    faces = raster.project_to_faces(torch.from_numpy(g['cam']), torch.from_numpy(g['vertices']), torch.from_numpy(g['faces_idx']))
    np.testing.assert_allclose(faces.numpy(), g['faces'], rtol=0, atol=1e-6)


def test_vertex_stage_matches_reference_fixture_dexycb():
    """The HOIG_DexYCB copy's projection (cam = [fx, fy, cx, cy | crop transform], its utils/nmr.py:38-48,146-163) against the fixture
    made by that copy's own code, one sample at a time as it runs there (tests/golden/make_golden_raster_vertex.py dexycb)."""
    import os
    from hoig_amd import raster
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'raster_vertex_stage_dexycb.npz'))
    faces = raster.project_to_faces(torch.from_numpy(g['cam']), torch.from_numpy(g['vertices']), torch.from_numpy(g['faces_idx']))
    np.testing.assert_allclose(faces.numpy(), g['faces'], rtol=0, atol=1e-6)
    assert np.abs(g['faces'][..., :2]).max() < 1.5                 # (the fixture's geometry lands in and around the image)


def test_wrapper_conventions_match_reference_python():
    """The reference's OWN Python wrapper (neural_renderer/rasterize.py: fill, call sequence, vertical flips) run over the oracle's
    restatement of the two CUDA kernels (tests/golden/make_golden_live_pins.py wrapper) gives exactly what oracle_rasterize_fim_wim
    returns."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'raster_wrapper_64.npz'))
    rf, rw = torch.from_numpy(g['fim']), torch.from_numpy(g['wim'])
    f = synthetic_mesh_faces(2, 300)
    of, ow = oracle_rasterize(f, 64)
    assert rf.dtype == torch.int32 and torch.equal(rf, of) and torch.equal(rw, ow)


def test_vertex_stage_matches_reference_live():
    """hoig_amd.raster.project_to_faces against the reference's own vertex stage on a second seed (tests/golden/
    make_golden_live_pins.py vertex): bit for bit."""
    import sys, os
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'golden'))
    from make_golden_raster_vertex import inputs
    from hoig_amd import raster
    cam, verts, idx = inputs(seed=7, B=4, V=40, F=70)       # (not 3: nr.look_at calls torch.cross without dim, which then
    # picks the batch axis -- a quirk the reference never meets, render_fim_wim is called per sample)
    ref = torch.from_numpy(np.load(os.path.join(here, 'golden', 'raster_vertex_stage_seed7.npz'))['faces'])
    assert torch.equal(raster.project_to_faces(cam, verts, idx), ref)


def test_weight_clamp_drops_nan_like_the_reference():
    """rasterize_cuda_kernel.cu:146 clamps with min(max(w, 0.), 1.): the double literals pick fmax / fmin, which return the other
    operand for a NaN, so a NaN weight becomes 0 -- it does not stay NaN, as a chain of comparisons would leave it.  (The HIP kernel
    says fmin / fmax too.)  On exactly collinear faces through pixel centres, whose weights are 0 / 0 and x / 0, this shows in no
    output: they cover nothing."""
    import ctypes
    import os
    from common import GOLDEN_DIR, pixel_centre
    lib = ctypes.CDLL(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, 'oracle', '_build', 'libhoig_oracle_c.so'))
    lib.oracle_raster_clamp01.argtypes, lib.oracle_raster_clamp01.restype = [ctypes.c_float], ctypes.c_float
    c = lib.oracle_raster_clamp01
    assert c(float('nan')) == 0.0
    assert [c(v) for v in (-np.inf, -3.0, 0.0, 0.25, 1.0, 1.5, np.inf)] == [0.0, 0.0, 0.0, 0.25, 1.0, 1.0, 1.0]
    g = np.random.default_rng(6)
    n = 500
    i0, step = g.integers(0, S, size=(n, 2)), g.integers(-2, 3, size=(n, 2))
    k = np.sort(g.integers(-6, 7, size=(n, 3)), axis=1)                   # three points of one lattice line, two of them equal at times
    xy = pixel_centre(i0[:, None, :] + k[:, :, None] * step[:, None, :], S)
    f = np.concatenate([xy, g.uniform(1, 3, size=(n, 3, 1)).astype(np.float32)], -1)
    fim, wim = oracle_rasterize(torch.from_numpy(f[:, None]), S)
    assert (fim == -1).all() and not wim.any()
