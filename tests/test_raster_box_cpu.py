"""CPU: the rasteriser's tile boxes (hoig_amd/csrc/raster_box.h through its CPU twin hoig_raster_face_boxes_host, the function
raster_setup_kernel calls) against the brute-force oracle (oracle/raster.c), which tests every face at every pixel: for every pixel the
oracle gives to a face, the face's box holds the pixel's tile -- on slivers, whose fp32 edge tests pass far outside their bounding box,
and on ordinary triangles.  And the fix stays narrow: faces that are no slivers keep the box they had (docs/raster_parity.md)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from common import oracle_rasterize, raster_boxes_host, sliver_faces, synthetic_mesh_faces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16
EMPTY = 0x00ff00ff
SIDES = {16: 42000, 64: 40000, 100: 15000, 256: 5000}          # image side -> pixel-centre slivers: 102000 faces in all
# the issue's single face, at side 64: it spans pixels x 7..16, y 13..31, and the oracle gives it pixel (32, 63) too
REGRESSION_FACE = np.array([[-0.765625, -0.578125, 2.8835], [-0.69071561, -0.42830628, 1.9197], [-0.484375, -0.015625, 1.2467]],
                           np.float32)
MESHES = [((2, 1500), {}), ((3, 4000), {}), ((1, 300), {}), ((1, 800), dict(seed=9))]


def whole(S):
    last = (S - 1) // TILE
    return (last << 8) | (last << 24)


def old_boxes(faces, S):
    """The box formula before slivers were known: bounding box of the pixel-space vertices, one pixel of slack, in tiles; the whole
    image for non-finite vertices, EMPTY for back faces and off-screen faces.  fp32 step by step, as raster_setup_kernel had it."""
    f = np.ascontiguousarray(faces, np.float32).reshape(-1, 9)
    f32 = np.float32
    with np.errstate(all='ignore'):
        back = (f[:, 7] - f[:, 1]) * (f[:, 3] - f[:, 0]) < (f[:, 4] - f[:, 1]) * (f[:, 6] - f[:, 0])
        p = (f.reshape(-1, 3, 3)[:, :, :2] * f32(S) + f32(S) - f32(1)) * f32(0.5)
        finite = np.isfinite(p).all((1, 2))
        p = np.where(finite[:, None, None], p, f32(0))
        lo, hi = p.min(1), p.max(1)
        off = (hi < -1).any(1) | (lo > S).any(1)
        b0 = np.maximum(np.floor(np.maximum(lo, f32(-1))).astype(np.int64) - 1, 0) // TILE
        b1 = np.minimum(np.ceil(np.minimum(hi, f32(S))).astype(np.int64) + 1, S - 1) // TILE
    box = (b0[:, 0] | (b1[:, 0] << 8) | (b0[:, 1] << 16) | (b1[:, 1] << 24)).astype(np.uint32)
    box[off] = EMPTY
    box[~finite] = whole(S)
    box[back] = EMPTY
    return box


def min_sine(faces, S):
    """The smallest interior-angle sine of each face, in float64 from pixel coordinates (0 for a face with a zero-length edge)."""
    p = 0.5 * (np.asarray(faces, np.float64).reshape(-1, 3, 3)[:, :, :2] * S + S - 1)
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], 1)
    n = np.sqrt((e ** 2).sum(-1))
    area2 = np.abs(e[:, 0, 0] * e[:, 1, 1] - e[:, 0, 1] * e[:, 1, 0])
    with np.errstate(all='ignore'):
        s = np.stack([area2 / (n[:, 0] * n[:, 1]), area2 / (n[:, 1] * n[:, 2]), area2 / (n[:, 2] * n[:, 0])], 1).min(1)
    return np.where(np.isfinite(s), s, 0.0)


def in_box(box, tx, ty):
    box = box.astype(np.int64)
    return (tx >= (box & 255)) & (tx <= ((box >> 8) & 255)) & (ty >= ((box >> 16) & 255)) & (ty <= (box >> 24))


def covered_pixels(faces, S):
    """Every face alone in its own image through the oracle -> (face, xi, yi) of every pixel it is given (yi before the flip)."""
    faces = np.ascontiguousarray(faces, np.float32).reshape(-1, 3, 3)
    chunk = max(1, (1 << 22) // (S * S))
    out = []
    for a in range(0, len(faces), chunk):
        fim, _ = oracle_rasterize(torch.from_numpy(faces[a:a + chunk, None]), S)
        b, row, xi = np.nonzero(fim.numpy() >= 0)
        out.append(np.stack([b + a, xi, S - 1 - row], 1))
    return np.concatenate(out)


def escapes(faces, S, boxes):
    """-> (covered pixels, those among them whose tile the face's box does not hold)"""
    c = covered_pixels(faces, S)
    return len(c), int((~in_box(boxes[c[:, 0]], c[:, 1] // TILE, c[:, 2] // TILE)).sum())


@pytest.mark.parametrize('S', sorted(SIDES))
def test_the_box_holds_every_pixel_the_oracle_gives_a_sliver(S):
    faces = sliver_faces(S, SIDES[S], seed=1)
    c = covered_pixels(faces, S)
    tx, ty = c[:, 1] // TILE, c[:, 2] // TILE
    new, old = raster_boxes_host(faces, S), old_boxes(faces, S)
    out_old = int((~in_box(old[c[:, 0]], tx, ty)).sum())
    out_new = int((~in_box(new[c[:, 0]], tx, ty)).sum())
    print('side %d: %d faces, %d covered pixels, %d outside the old box, %d outside the box' % (S, len(faces), len(c), out_old, out_new))
    assert len(c) > len(faces) // 20
    assert out_new == 0
    if S > TILE:                                 # (one tile: every box of an on-screen face is the image)
        # non-vacuity: the recipe still makes pixels that leave the bounding box (the issue measured 21 %; 10 % asked)
        assert out_old >= 0.10 * len(c), (out_old, len(c))


@pytest.mark.parametrize('S', sorted(SIDES))
def test_the_box_holds_every_pixel_of_slivers_through_arbitrary_points(S):
    faces = sliver_faces(S, SIDES[S] // 4, seed=2, on_centres=False)
    n, out = escapes(faces, S, raster_boxes_host(faces, S))
    print('side %d: %d covered pixels' % (S, n))
    assert n > len(faces) // 2 and out == 0


@pytest.mark.parametrize('S', sorted(SIDES))
def test_the_box_holds_every_pixel_of_ordinary_triangles(S):
    faces = synthetic_mesh_faces(1, 800 if S < 256 else 300, seed=S).numpy()[0]
    n, out = escapes(faces, S, raster_boxes_host(faces, S))
    assert n > S * S // 2 and out == 0


def test_the_regression_face():
    S = 64
    fim, wim = oracle_rasterize(torch.from_numpy(REGRESSION_FACE[None, None]), S)
    assert int(fim[0, S - 1 - 63, 32]) == 0 and wim[0, S - 1 - 63, 32].tolist() == [0.0, 0.0, 1.0]
    old, new = old_boxes(REGRESSION_FACE, S), raster_boxes_host(REGRESSION_FACE, S)
    assert int(old[0]) == (0 | (1 << 8) | (0 << 16) | (2 << 24))           # tiles x 0..1, y 0..2: it ends at x = 31, y = 47
    assert not in_box(old, 32 // TILE, 63 // TILE)[0]
    assert int(new[0]) == whole(S)
    n, out = escapes(REGRESSION_FACE, S, new)
    assert n > 0 and out == 0


def _all_cases():
    for S in sorted(SIDES):
        yield S, sliver_faces(S, SIDES[S] // 10, seed=1)
        yield S, sliver_faces(S, SIDES[S] // 10, seed=2, on_centres=False)
    for (args, kw), S in zip(MESHES, (256, 128, 64, 100)):
        yield S, synthetic_mesh_faces(*args, **kw).numpy()


def test_faces_that_are_no_slivers_keep_their_box():
    """(a): every face whose smallest interior-angle sine is >= 1e-3 has exactly the box it had."""
    kept = 0
    for S, faces in _all_cases():
        faces = faces.reshape(-1, 3, 3)
        sel = min_sine(faces, S) >= 1e-3
        assert np.array_equal(raster_boxes_host(faces[sel], S), old_boxes(faces[sel], S)), S
        kept += int(sel.sum())
    assert kept > 20000


@pytest.mark.parametrize('mesh,S', list(zip(MESHES, (256, 128, 64, 100))), ids=str)
def test_few_faces_of_a_mesh_take_the_whole_image(mesh, S):
    """(b): at most 1 % of the faces of the synthetic meshes get another box than before -- the whole image."""
    (args, kw) = mesh
    faces = synthetic_mesh_faces(*args, **kw).numpy().reshape(-1, 3, 3)
    new, old = raster_boxes_host(faces, S), old_boxes(faces, S)
    changed = new != old
    assert (new[changed] == whole(S)).all()
    share = changed.mean()
    print('%s side %d: %d of %d faces take the whole image (%.3f %%); sine < 1e-3: %.3f %%'
          % (mesh, S, int(changed.sum()), len(faces), 100 * share, 100 * (min_sine(faces, S) < 1e-3).mean()))
    assert share <= 0.01


def test_point_faces_nonfinite_faces_and_refusals():
    from hoig_amd import _lib as L
    S = 64
    pt = np.array([[[0.1, 0.2, 2.0]] * 3, [[-1.0e6, -1.0e6, -1.0e6]] * 3], np.float32)      # a point in the image; the padding point
    assert raster_boxes_host(pt, S).tolist() == old_boxes(pt, S).tolist() and raster_boxes_host(pt, S)[1] == EMPTY
    n, _ = escapes(pt, S, raster_boxes_host(pt, S))
    assert n == 0                                                                            # a point covers nothing
    for bad in (np.nan, np.inf, -np.inf):
        f = np.array([[-0.5, -0.5, 2.0], [0.5, -0.5, 2.0], [0.0, 0.5, 2.0]], np.float32)
        f[2, 0] = bad
        b = raster_boxes_host(f, S)[0]
        assert b in (whole(S), EMPTY)                                 # (EMPTY: the back-face test, which comes first, said so)
    out = np.zeros(1, np.uint32)
    f = np.zeros(9, np.float32)
    fn = L.lib.hoig_raster_face_boxes_host
    assert fn(f.ctypes.data, 1, 64, out.ctypes.data) == L.OK
    for args in ((None, 1, 64, out.ctypes.data), (f.ctypes.data, 0, 64, out.ctypes.data), (f.ctypes.data, 1, 0, out.ctypes.data),
                 (f.ctypes.data, 1, 4097, out.ctypes.data), (f.ctypes.data, 1, 64, None)):
        assert fn(*args) == L.EINVAL


def test_the_twin_under_a_host_sanitizer_build(tmp_path):
    """raster_host.cpp built with -fsanitize=address,undefined into a program of its own (tests/raster_box_asan_driver.cpp), every buffer
    a heap block of exactly its size: no report, and the library twin's boxes."""
    # (the compiler, the flags and the reasons for them: tests/test_grad_guard_cpu.py)
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    assert cxx is not None, 'no host C++ compiler (c++, or $CXX) on PATH'
    flags = ['-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
             '-static-libasan']
    exe = str(tmp_path / 'raster_box_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'raster_host.cpp'), os.path.join(ROOT, 'tests', 'raster_box_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    for S, n in ((1, 7), (64, 500), (100, 333), (4096, 64)):
        run = subprocess.run([exe, str(n), str(S)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert run.returncode == 0 and 'Sanitizer' not in run.stdout and 'runtime error' not in run.stdout, run.stdout[-3000:]
        got = run.stdout.split()
        assert got[0] == '0' and len(got) == n + 1
        # the driver's faces (its function `coord`), through the library's twin
        k = np.arange(n * 9, dtype=np.int64)
        f = (((k * 37 + (k // 9) * 11) % 83 - 41).astype(np.float32) * np.float32(0.03125))
        f[k % 9 % 3 == 2] += np.float32(3.0)
        f[(k % 173) == 172] = np.inf
        assert [int(v, 16) for v in got[1:]] == raster_boxes_host(f, S).tolist()
