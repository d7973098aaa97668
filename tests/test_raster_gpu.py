"""GPU: the tile-binned HIP rasteriser (hoig_rasterize_fim_wim through the C ABI) against the plain-C oracle of the
reference's brute-force kernels (oracle/raster.c): the face-index map must be IDENTICAL (integer output) and the weight map
bit-identical (same fp32 operations, no contraction on either side) on meshes with back faces, depth ties, degenerate,
clipped, huge and out-of-range triangles."""
import numpy as np
import pytest
import torch

from common import oracle_rasterize, synthetic_mesh_faces

pytestmark = pytest.mark.gpu


def check(faces, S, **kw):
    from hoig_amd import raster
    fim, wim = raster.rasterize_fim_wim(faces.cuda(), S, **kw)
    ofim, owim = oracle_rasterize(faces, S, **kw)
    fim, wim = fim.cpu(), wim.cpu()
    bad = (fim != ofim)
    assert not bad.any(), '%d of %d pixels differ' % (int(bad.sum()), fim.numel())
    assert torch.equal(wim, owim), float((wim - owim).abs().max())
    return fim


@pytest.mark.parametrize('batch,n_random,S', [(2, 1500, 256), (1, 0, 256), (3, 4000, 128), (1, 300, 64)])
def test_hip_matches_oracle_exactly(batch, n_random, S):
    fim = check(synthetic_mesh_faces(batch, n_random), S)
    assert (fim >= 0).float().mean() > 0.05


def test_non_multiple_of_tile_and_near_far():
    f = synthetic_mesh_faces(1, 800, seed=9)
    check(f, 100)                                  # image side not a multiple of the 16-pixel tile
    check(f, 256, near=1.0, far=3.0)


def test_many_faces_in_one_tile():
    """More faces over one tile than the LDS list holds (512): the list is consumed in several rounds."""
    g = np.random.default_rng(3)
    n = 3000
    xy = g.uniform(-0.05, 0.05, size=(n, 1, 2)) + g.uniform(-0.04, 0.04, size=(n, 3, 2))
    z = g.uniform(1.0, 4.0, size=(n, 3, 1))
    f = torch.from_numpy(np.concatenate([xy, z], -1).astype(np.float32))[None]
    fim = check(f, 256)
    assert len(np.unique(fim.numpy())) > 50


def test_empty_and_offscreen():
    f = torch.tensor([[[[2.0, 2.0, 2.0], [3.0, 2.0, 2.0], [2.0, 3.0, 2.0]]]])           # entirely off screen
    fim = check(f, 64)
    assert (fim == -1).all()
    f = torch.tensor([[[[-5.0, -5.0, 2.0], [5.0, -5.0, 2.0], [0.0, 5.0, 2.0]]]])         # covers the whole image
    fim = check(f, 64)
    assert (fim == 0).all()


def test_render_fim_wim_feeds_input_prep():
    """render_fim_wim (projection + look-at + rasterisation) produces maps the input-preparation stage accepts."""
    from hoig_amd import raster
    g = np.random.default_rng(1)
    V = 600
    verts = torch.from_numpy(np.concatenate([g.uniform(-0.1, 0.1, size=(1, V, 2)), g.uniform(-0.7, -0.5, size=(1, V, 1))],
                                            -1).astype(np.float32)).cuda()
    cam = torch.tensor([[600.0, 0, 128, 0, 600.0, 128, 0, 0, 1, 1, 0, 0, 0, 1, 0]], dtype=torch.float32).cuda()
    idx = torch.from_numpy(g.integers(0, V, size=(1200, 3)).astype(np.int32)).cuda()
    faces, fim, wim = raster.render_fim_wim(cam, verts, idx, 256)
    assert faces.shape == (1, 1200, 3, 3) and fim.shape == (1, 256, 256) and wim.shape == (1, 256, 256, 3)
    ofim, owim = oracle_rasterize(faces.cpu(), 256)
    assert torch.equal(fim.cpu(), ofim) and torch.equal(wim.cpu(), owim)
    assert (fim >= 0).any() and (fim == -1).any()
    covered = fim[0] >= 0
    assert torch.allclose(wim[0][covered].sum(-1), torch.ones_like(wim[0][covered].sum(-1)), atol=1e-5)


def test_vertex_stage_on_device_matches_reference_fixture():
    import os
    from hoig_amd import raster
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'raster_vertex_stage.npz'))
    faces = raster.project_to_faces(torch.from_numpy(g['cam']).cuda(), torch.from_numpy(g['vertices']).cuda(),
                                    torch.from_numpy(g['faces_idx']).cuda())
    np.testing.assert_allclose(faces.cpu().numpy(), g['faces'], rtol=0, atol=2e-5)


def test_vertex_stage_on_device_matches_reference_fixture_dexycb():
    import os
    from hoig_amd import raster
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'raster_vertex_stage_dexycb.npz'))
    faces = raster.project_to_faces(torch.from_numpy(g['cam']).cuda(), torch.from_numpy(g['vertices']).cuda(),
                                    torch.from_numpy(g['faces_idx']).cuda())
    np.testing.assert_allclose(faces.cpu().numpy(), g['faces'], rtol=0, atol=2e-5)


@pytest.mark.parametrize('fixture', ['raster_vertex_stage.npz', 'raster_vertex_stage_dexycb.npz'])
def test_one_launch_vertex_stage_matches_the_reference_fixture_and_the_torch_form(fixture):
    """hoig_project_faces (round 6: projection + flip + look-at + vertices_to_faces for a batch whose samples hold different objects, one
    launch) against the fixture made by the reference's own projection, and against raster.project_to_faces on a batch with two
    face lists of different lengths and a padded tail."""
    import os
    from hoig_amd import raster
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', fixture))
    cam, verts = torch.from_numpy(g['cam']).cuda(), torch.from_numpy(g['vertices']).cuda()
    idx = torch.from_numpy(g['faces_idx']).cuda().long().contiguous()
    B = cam.shape[0]
    lists = [idx if idx.dim() == 2 else idx[b].contiguous() for b in range(B)]
    faces = raster.project_faces_batched(cam, verts, lists, lists[0].shape[0])
    np.testing.assert_allclose(faces.cpu().numpy(), g['faces'], rtol=0, atol=2e-5)
    # two different lists in one batch: sample 0 keeps the full list, the others a prefix; rows beyond a list are the far-away point
    short = lists[0][: lists[0].shape[0] // 3].contiguous()
    mixed = [lists[0]] + [short] * (B - 1)
    got = raster.project_faces_batched(cam, verts, mixed, lists[0].shape[0], pad_value=-1.0e6)
    full = raster.project_to_faces(cam, verts, lists[0])
    np.testing.assert_allclose(got[0].cpu().numpy(), full[0].cpu().numpy(), rtol=0, atol=2e-5)
    for b in range(1, B):
        np.testing.assert_allclose(got[b, :short.shape[0]].cpu().numpy(), full[b, :short.shape[0]].cpu().numpy(), rtol=0, atol=2e-5)
        assert bool((got[b, short.shape[0]:] == -1.0e6).all())


def test_vertices_to_generator_inputs_end_to_end():
    """The whole HandRecoveryFlow.forward chain on the device -- render_fim_wim for the source and the reference pose, then
    the input preparation -- against the oracle chain (C rasteriser + torch restatement) on the same vertices."""
    from hoig_amd import raster, input_prep as IP, synthetic
    from oracle import input_prep_oracle as P
    tb = synthetic.make_object_tables(3, seed=21)
    F, NH = tb['n_faces'], synthetic.N_HAND_FACES
    g = np.random.default_rng(4)
    hand_v = np.concatenate([g.uniform(-0.06, 0.02, size=(300, 2)), g.uniform(-0.62, -0.56, size=(300, 1))], -1)
    obj_v = np.concatenate([g.uniform(0.0, 0.08, size=(200, 2)), g.uniform(-0.66, -0.58, size=(200, 1))], -1)
    verts = torch.from_numpy(np.concatenate([hand_v, obj_v])[None].astype(np.float32))
    near = lambda n, lo, hi: g.integers(lo, hi, size=(n, 3))
    idx = torch.from_numpy(np.concatenate([near(NH, 0, 300), near(F - NH, 300, 500)]).astype(np.int32))
    cams = [torch.tensor([[600.0, 0, 128, 0, 600.0, 128, 0, 0, 1, 1, 0, 0, 0, 1, 0]], dtype=torch.float32),
            torch.tensor([[560.0, 0, 120, 0, 580.0, 140, 0, 0, 1, 1, 0.02, 3, -0.02, 1, -2]], dtype=torch.float32)]
    src_img = torch.from_numpy(g.uniform(-1, 1, size=(1, 3, 256, 256)).astype(np.float32))
    ref_img = torch.from_numpy(g.uniform(-1, 1, size=(1, 3, 256, 256)).astype(np.float32))
    dev = torch.device('cuda', 0)
    s_faces, s_fim, s_wim = raster.render_fim_wim(cams[0].to(dev), verts.to(dev), idx.to(dev))
    _, r_fim, r_wim = raster.render_fim_wim(cams[1].to(dev), verts.to(dev), idx.to(dev))
    assert ((s_fim >= 0) & (s_fim < NH)).any() and (s_fim >= NH).any() and (s_fim == -1).any()
    out = IP.prepare_inputs(src_img.to(dev), ref_img.to(dev), s_faces, s_fim, s_wim, r_fim, r_wim, [IP.ObjectTables(tb, dev)])
    # oracle chain from the same face tensors (the vertex stage is pinned separately)
    of, ow = oracle_rasterize(s_faces.cpu(), 256)
    rf, rw = oracle_rasterize(raster.project_to_faces(cams[1].to(dev), verts.to(dev), idx.to(dev)).cpu(), 256)
    assert torch.equal(s_fim.cpu(), of) and torch.equal(r_fim.cpu(), rf)
    want = P.prepare_inputs(src_img, ref_img, s_faces.cpu(), of, ow, rf, rw, [tb])
    for a, b in zip(out, want):
        if a is not None:
            assert (a.cpu() - b).abs().max() <= 2e-6
    for i in (7, 8, 9, 10):
        assert torch.equal(out[i].cpu(), want[i])


# ---------------------------------------------------------------------------------------------------- slivers (docs/raster_parity.md)
def _tri(S, a, b, c, z):
    """One face with its vertices on the pixel centres a, b, c (pixel units; they may lie outside the image)."""
    from common import pixel_centre
    z = np.broadcast_to(np.asarray(z, np.float32), (3,))
    return np.concatenate([pixel_centre(np.array([a, b, c]), S), z[:, None]], -1).astype(np.float32)


def _ccw(f):
    """The face with its winding turned to the front side (counter-clockwise, y up), by swapping two vertices if need be."""
    e, d = f[1, :2].astype(np.float64) - f[0, :2], f[2, :2].astype(np.float64) - f[0, :2]
    return f if e[0] * d[1] - e[1] * d[0] > 0 else f[[0, 2, 1]]


@pytest.mark.parametrize('S,n', [(64, 400), (100, 300)])
def test_slivers_cover_pixels_far_outside_their_bounding_box(S, n):
    """Slivers, whose fp32 edge tests pass along the whole line through them, between ordinary faces behind and in front of them and
    beside their own copies (equal depth: the first in index order wins): the stray pixels compete on depth and on index ties."""
    from common import sliver_faces
    from test_raster_box_cpu import REGRESSION_FACE, in_box, old_boxes
    sl = np.concatenate([sliver_faces(S, n, seed=3), sliver_faces(S, n // 4, seed=4, on_centres=False)])
    g = np.random.default_rng(S)
    behind = synthetic_mesh_faces(1, 40, seed=S).numpy()[0][-40:].copy()
    behind[:, :, 2] = g.uniform(3.5, 5.0, size=(40, 3))
    front = synthetic_mesh_faces(1, 40, seed=S + 1).numpy()[0][-40:].copy()
    front[:, :, 2] = g.uniform(0.4, 0.9, size=(40, 3))
    back_wall = np.stack([_tri(S, (-4, -4), (2 * S, -4), (-4, 2 * S), 3.2)])               # behind every sliver, over the whole image
    faces = np.concatenate([behind[:20], back_wall, sl[:n // 2], front[:20], sl, REGRESSION_FACE[None], behind[20:], sl[::3], front[20:]])
    fim = check(torch.from_numpy(faces)[None], S).numpy()[0]
    # what the comparison covered: pixels that a sliver owns outside the bounding box that used to bin it
    row, xi = np.nonzero(fim >= 0)
    owner = fim[row, xi]
    stray = ~in_box(old_boxes(faces, S)[owner], xi // 16, (S - 1 - row) // 16)
    assert stray.sum() > 20, int(stray.sum())
    assert len(np.unique(owner[stray])) > 5


def test_the_regression_sliver_alone():
    """The face of docs/raster_parity.md at side 64: pixels x 7..16, y 13..31, and the reference gives it pixel (32, 63) as well."""
    from test_raster_box_cpu import REGRESSION_FACE
    fim = check(torch.from_numpy(REGRESSION_FACE)[None, None], 64)
    assert int(fim[0, 64 - 1 - 63, 32]) == 0


# ---------------------------------------------------------------------------------------------------- the tile kernel's list rounds
@pytest.mark.parametrize('pad', [0, 100])
@pytest.mark.parametrize('N', [256, 257, 511, 512, 513])
def test_list_rounds(N, pad):
    """Exactly N faces over the middle tile of a 48-pixel image, behind `pad` faces that touch no tile.  The kernel reads the faces 256
    at a time and consumes its list once it holds more than 256 records, so the rounds end at face indices that are multiples of 256.
    Pairs of small faces sit on both sides of each such index: two copies (a depth tie: the first wins, whichever round holds it), the
    nearer face before the index, and the nearer face after it."""
    S, F = 48, pad + N
    g = np.random.default_rng([N, pad])
    faces = np.empty((F, 3, 3), np.float32)
    faces[:pad] = _tri(S, (100, 100), (110, 100), (100, 110), 2.0)                          # off the image
    for i in range(pad, F):                                                                 # over the whole middle tile
        faces[i] = _tri(S, (14 - g.integers(0, 3), 14 - g.integers(0, 3)), (52 + g.integers(0, 3), 14), (14, 52 + g.integers(0, 3)),
                        g.uniform(2.0, 3.0, size=3))
    spots, want = iter([(17, 17), (22, 17), (27, 17), (17, 24), (22, 24), (27, 24)]), {}
    for b in (256, 512):
        for k, (z0, z1) in enumerate([(1.0, 1.0), (1.0, 1.5), (1.5, 1.0)]):
            i, j = (b - 1 - k, b + k) if b + k < F and b - 1 - k >= pad else (pad + 3 * (b // 256) + k, F - 1 - 3 * (b // 256) - k)
            x, y = next(spots)
            faces[i] = _tri(S, (x - 1, y - 1), (x + 3, y - 1), (x - 1, y + 3), z0)
            faces[j] = _tri(S, (x - 1, y - 1), (x + 3, y - 1), (x - 1, y + 3), z1)
            want[(x, y)] = i if z0 <= z1 else j
    fim = check(torch.from_numpy(faces)[None], S)[0]
    for (x, y), i in want.items():
        assert int(fim[S - 1 - y, x]) == i, ((x, y), i)
    assert (fim[16:32, 16:32] >= pad).all()


# ---------------------------------------------------------------------------------------------------- image sides
@pytest.mark.parametrize('S', [1, 15, 16, 17])
def test_small_image_sides(S):
    """One pixel, and partial tiles on both axes."""
    fim = check(synthetic_mesh_faces(2, 300), S)
    assert (fim >= 0).any()


def test_side_4096_reaches_tile_255():
    """The largest side: tile index 255 is the value the empty box borrows for its first column.  One face in the last tile column and
    row only, one in tile 0 only, one off the image."""
    S = 4096
    faces = np.stack([_tri(S, (4084, 4085), (4094, 4086), (4086, 4094), (2.0, 2.5, 3.0)),
                      _tri(S, (2, 3), (12, 4), (4, 13), (1.0, 2.0, 1.5)),
                      _tri(S, (5000, 5000), (5010, 5000), (5000, 5010), 2.0)])
    fim = check(torch.from_numpy(faces)[None], S)[0]
    assert (fim[S - 1 - 4094:S - 1 - 4084, 4084:4095] == 0).sum() > 20 and (fim[S - 1 - 13:S - 1 - 2, 2:13] == 1).sum() > 20
    assert int((fim >= 0).sum()) == int((fim[:16, -16:] == 0).sum() + (fim[-16:, :16] == 1).sum()) and not (fim == 2).any()


# ---------------------------------------------------------------------------------------------------- pixel-centre geometry
def test_pixel_centre_geometry_across_tile_boundaries():
    """Vertices and edges exactly on pixel centres at x, y in {15, 16}, the seam of the tiles; faces that touch the image at pixel 0 or
    S - 1 alone; faces whose extent ends exactly at -1 and at S in pixel units, where the early reject begins."""
    S, faces = 64, []
    q = [(15, 15), (16, 15), (16, 16), (15, 16)]
    for a in range(4):                                                 # the four half-squares of the seam's 2 x 2 pixels
        faces.append(_tri(S, q[a], q[(a + 1) % 4], q[(a + 2) % 4], 2.0))
    for (a, b, c) in [((15, 15), (40, 15), (15, 40)), ((16, 16), (16, 2), (2, 16)), ((15, 16), (15, 50), (3, 16)), ((16, 15), (60, 15), (16, 3)),
                      ((15, 0), (16, 31), (15, 63)), ((0, 16), (63, 15), (31, 16)), ((0, 15), (63, 15), (31, 16)), ((15, 0), (15, 63), (16, 31)),
                      ((8, 8), (24, 8), (16, 24)), ((15, 31), (31, 15), (31, 31)), ((16, 32), (32, 16), (16, 16))]:
        faces.append(_tri(S, a, b, c, (1.5, 2.5, 2.0)))
    for e in (0, S - 1):                                               # a vertex on the centre of an edge or corner pixel, the rest outside
        o = -6 if e == 0 else S + 5
        faces += [_tri(S, (e, 5), (o, 2), (o, 8), 1.2), _tri(S, (20, e), (17, o), (23, o), 1.2), _tri(S, (e, e), (o, e), (e, o), 1.2),
                  _tri(S, (e, S - 1 - e), (o, S - 1 - e), (e, S - 1 - o), 1.2)]
    for lim, o in ((-1, -9), (S, S + 8)):                              # the extent ends exactly at -1 / begins exactly at S
        faces += [_tri(S, (lim, 10), (o, 4), (o, 16), 1.1), _tri(S, (30, lim), (24, o), (36, o), 1.1), _tri(S, (lim, lim), (o, lim), (lim, o), 1.1),
                  _tri(S, (lim, 3), (lim, 40), (o, 20), 1.1), _tri(S, (3, lim), (40, lim), (20, o), 1.1)]
    faces = [_ccw(f) for f in faces]
    faces += [f[[0, 2, 1]] for f in faces[:8]]                          # and some from their back side
    faces.append(_tri(S, (-4, -4), (2 * S, -4), (-4, 2 * S), 3.0))      # a wall behind them all
    f = torch.from_numpy(np.stack(faces))[None]
    fim = check(f, S)[0]
    assert len(np.unique(fim.numpy())) > 15
    for y, x in ((5, 0), (S - 1, 20), (0, 0), (S - 1, S - 1), (5, S - 1)):   # the vertices on the border pixels' centres are inside
        assert int(fim[S - 1 - y, x]) != len(faces) - 1, (x, y)
    check(f, S - 1)                                                     # the same numbers off the centres, the seam inside a partial tile


# ---------------------------------------------------------------------------------------------------- non-finite vertices
def test_non_finite_vertices_among_ordinary_faces():
    S = 64
    base = synthetic_mesh_faces(1, 300).numpy()[0]
    tri = np.array([[-0.6, -0.5, 2.0], [0.7, -0.4, 1.5], [0.1, 0.8, 1.8]], np.float32)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for vert in range(3):
            for axis in range(3):
                t = np.roll(tri, vert, 0).copy()
                t[vert, axis] = v
                bad.append(t)
    bad = np.stack(bad)
    idx = np.linspace(0, len(base) - 1, len(bad)).astype(int)
    faces = np.insert(base, idx, bad, 0)                                # spread through the list
    check(torch.from_numpy(faces)[None], S)
    fim = check(torch.from_numpy(np.concatenate([bad, base[:50]]))[None], 100)
    assert (fim >= 0).any()


# ---------------------------------------------------------------------------------------------------- batches
def test_batch_of_three_with_one_face_list():
    """B = 3, one face list (F = 700: no multiple of 256) over three sets of vertices: blockIdx.y must address rec and box per sample."""
    g = np.random.default_rng(12)
    V, F, S = 150, 700, 64
    idx = g.integers(0, V, size=(F, 3))
    verts = np.concatenate([g.uniform(-1.1, 1.1, size=(3, V, 2)), g.uniform(1.0, 4.0, size=(3, V, 1))], -1).astype(np.float32)
    faces = torch.from_numpy(verts[:, idx])                             # (3, F, 3, 3)
    fim = check(faces, S)
    for b in range(3):
        assert torch.equal(fim[b], check(faces[b:b + 1], S)[0])
    assert not torch.equal(fim[0], fim[1]) and not torch.equal(fim[1], fim[2])


# ---------------------------------------------------------------------------------------------------- the vertex stage's edges
def _project_f64(cam, verts, lists, fmax, pad, viewing_angle=30.0):
    """hoig_project_faces restated in float64 (nmr.py:109-140 / the DexYCB copy's :146-163, the y flip :506, look_at, vertices_to_faces)."""
    import math
    cam, verts = cam.astype(np.float64), verts.astype(np.float64)
    eye_z = -(1.0 / math.tan(math.radians(viewing_angle)) + 1.0)
    out = np.full((len(lists), fmax, 3, 3), float(pad))
    with np.errstate(all='ignore'):
        for b, fl in enumerate(lists):
            c, v = cam[b], verts[b][fl.reshape(-1)]
            if len(c) == 15:
                p = v * np.array([1.0, -1.0, -1.0])
                q = [(p[:, 0] * c[3 * r] + p[:, 1] * c[3 * r + 1]) + p[:, 2] * c[3 * r + 2] for r in range(3)]
                x, y, z, tr = q[0] / q[2], q[1] / q[2], p[:, 2], c[9:]
            else:
                eps = np.float64(np.float32(1e-8))                      # (the fp32 constant of both implementations)
                x, y = v[:, 0] / (v[:, 2] + eps) * c[0] + c[2], v[:, 1] / (v[:, 2] + eps) * c[1] + c[3]
                z, tr = v[:, 2], c[4:]
            u, w = (tr[0] * x + tr[1] * y) + tr[2], (tr[3] * x + tr[4] * y) + tr[5]
            o = np.stack([u / 255.0 * 2 - 1, -(w / 255.0 * 2 - 1), z - eye_z], -1)
            out[b, :len(fl)] = o.reshape(-1, 3, 3)
    return out


def _vertex_case(B, V, F, cam_dim, seed):
    g = np.random.default_rng(seed)
    verts = np.concatenate([g.uniform(-0.1, 0.1, size=(B, V, 2)), g.uniform(-0.7, -0.5, size=(B, V, 1))], -1).astype(np.float32)
    if cam_dim == 15:
        cam = np.tile(np.array([600.0, 0, 128, 0, 600.0, 128, 0, 0, 1, 1, 0.02, 3, -0.02, 1, -2], np.float32), (B, 1))
    else:
        verts[:, :, 2] *= -1
        cam = np.tile(np.array([600.0, 610.0, 128, 120, 1, 0.02, 3, -0.02, 1, -2], np.float32), (B, 1))
    cam[:, :2] += g.uniform(-20, 20, size=(B, 2)).astype(np.float32)
    lists = [g.integers(0, V, size=(int(n), 3)) for n in g.integers(1, F + 1, size=B)]
    return cam, verts, lists


def _same(got, want):
    """finite values within the file's 2e-5; NaN where NaN is, and each infinity with its sign"""
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=2e-5)


@pytest.mark.parametrize('cam_dim', [15, 10])
def test_vertex_stage_with_a_sample_without_faces(cam_dim):
    from hoig_amd import raster
    cam, verts, lists = _vertex_case(3, 50, 40, cam_dim, seed=cam_dim)
    lists[1] = lists[1][:0]
    dev = [torch.from_numpy(fl).cuda().contiguous() for fl in lists]
    assert dev[1].numel() == 0
    got = raster.project_faces_batched(torch.from_numpy(cam).cuda(), torch.from_numpy(verts).cuda(), dev, 40, pad_value=-1.0e6)
    _same(got.cpu().numpy(), _project_f64(cam, verts, lists, 40, -1.0e6))
    assert bool((got[1] == -1.0e6).all())
    fim, _ = raster.rasterize_fim_wim(got, 64)
    assert bool((fim[1] == -1).all()) and bool((fim[0] >= 0).any())


def test_vertex_stage_at_the_largest_batch_and_one_above():
    import ctypes
    from hoig_amd import _lib as L, raster
    B = L.PREP_MAX_BATCH
    cam, verts, lists = _vertex_case(B + 1, 30, 20, 15, seed=2)
    dev = [torch.from_numpy(fl).cuda().contiguous() for fl in lists]
    dcam, dverts = torch.from_numpy(cam).cuda(), torch.from_numpy(verts).cuda()
    got = raster.project_faces_batched(dcam[:B], dverts[:B], dev[:B], 20)
    _same(got.cpu().numpy(), _project_f64(cam[:B], verts[:B], lists[:B], 20, -1.0e6))
    # one above: unsupported, and nothing is written
    out = torch.full((B + 1, 20, 3, 3), 7.0, device='cuda')
    ptrs = (ctypes.c_void_p * (B + 1))(*[t.data_ptr() for t in dev])
    nf = (ctypes.c_int * (B + 1))(*[int(t.shape[0]) for t in dev])
    rc = L.lib.hoig_project_faces(dcam.data_ptr(), 15, dverts.data_ptr(), 30, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nf, ctypes.c_void_p),
                                  B + 1, 20, -2.7, -1.0e6, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == L.EUNSUPPORTED and bool((out == 7.0).all())
    with pytest.raises(L.HoigKernelError):
        raster.project_faces_batched(dcam, dverts, dev, 20)


@pytest.mark.parametrize('cam_dim', [15, 10])
def test_vertex_with_zero_depth_goes_through_the_rasteriser(cam_dim):
    """A vertex in the camera's plane: the perspective divide gives infinities (and NaN where they meet a zero or each other); the
    faces that hold it take the rasteriser's whole-image path, the others are drawn as ever."""
    from hoig_amd import raster
    cam, verts, lists = _vertex_case(2, 60, 200, cam_dim, seed=5)
    verts[0, 7, 2] = 0.0
    verts[1, 9] = (0.0, 0.05, 0.0)
    if cam_dim == 10:
        verts[0, 7, 2] = verts[1, 9, 2] = -1e-8       # x / (z + 1e-8): the zero of the DexYCB form
    lists = [np.concatenate([fl, [[7, 1, 2], [3, 9, 4], [7, 9, 5]]]) for fl in lists]
    fmax = max(len(fl) for fl in lists)
    dev = [torch.from_numpy(fl).cuda().contiguous() for fl in lists]
    got = raster.project_faces_batched(torch.from_numpy(cam).cuda(), torch.from_numpy(verts).cuda(), dev, fmax).cpu()
    want = _project_f64(cam, verts, lists, fmax, -1.0e6)
    _same(got.numpy(), want)
    assert not np.isfinite(want[0]).all() and not np.isfinite(want[1]).all()
    fim = check(got, 64)
    assert (fim >= 0).any()
