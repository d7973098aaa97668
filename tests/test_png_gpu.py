"""hoig_png_encode_u8 on the MI355X against its host twin, byte for byte (content, shapes and the twin's wrappers: tests/png_reference.py;
what the twin's files must be: tests/test_png_cpu.py)."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 4096
GROUPS = [(shape, seg, kinds) for shape, segs, kinds in R.SHAPES for seg in segs]
GROUP_IDS = ['%dx%dx%d-s%d' % (s + (seg,)) for s, seg, _ in GROUPS]


def device_encode(batch, segment_bytes=0):
    """The files of a uint8 [B, H, W, C] host batch through hoig_png_encode_u8, and sizes; everything in the slots past sizes[i] and a
    guard region behind the last slot must keep its 0x5A fill."""
    from hoig_amd import _lib as L
    b, h, w, c = batch.shape
    stride = L.lib.hoig_png_encode_bound(h, w, c, segment_bytes)
    ws_bytes = L.lib.hoig_png_encode_workspace_bytes(b, h, w, c, segment_bytes)
    assert stride > 0 and ws_bytes > 0
    src = torch.from_numpy(np.ascontiguousarray(batch)).to(DEV)
    out = torch.full((b * stride + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    sizes = torch.full((b,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    L.call('hoig_png_encode_u8', src.data_ptr(), b, h, w, c, out.data_ptr(), stride, sizes.data_ptr(), ws.data_ptr(), ws_bytes,
           segment_bytes, torch.cuda.current_stream().cuda_stream)
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    files = []
    for i in range(b):
        assert 0 < sizes[i] <= stride
        files.append(out[i * stride:i * stride + sizes[i]].tobytes())
        assert (out[i * stride + sizes[i]:(i + 1) * stride] == 0x5A).all(), i
    assert (out[b * stride:] == 0x5A).all()
    return files


@pytest.mark.parametrize('group', GROUPS, ids=GROUP_IDS)
def test_the_device_files_equal_the_twins_every_byte(group):
    shape, seg, kinds = group
    batch = np.stack([R.content(k, *shape) for k in kinds])
    got, want = device_encode(batch, seg), R.encode_host(batch, seg)
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w, k in zip(got, want, kinds):
        assert g == w, k


def test_the_mixed_batch_opens_in_pillow_to_the_input():
    batch = R.mixed_batch()
    got = device_encode(batch)
    assert got == R.encode_host(batch)
    for png, img in zip(got, batch):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), img)
        assert R.parse(png)[2] == R.filter_stream(img).tobytes()


def test_the_workloads_own_shape():
    from hoig_amd import png
    batch = R.workload_batch()
    got = png.encode_u8(torch.from_numpy(batch).to(DEV))
    assert got == R.encode_host(batch)
    assert got == device_encode(batch)
    for f, img in zip(got, batch):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), img)


def test_a_side_stream_with_its_input_made_on_that_stream():
    from hoig_amd import ops, png
    x = torch.from_numpy(np.random.RandomState(11).uniform(-1, 1, (3, 128, 128, 3)).astype(np.float32)).to(DEV)
    want = png.encode_u8(ops.tensor2im_nhwc_u8(x))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        u8 = ops.tensor2im_nhwc_u8(x)
        got = png.encode_u8(u8, 0)
    side.synchronize()
    assert got == want == R.encode_host(u8.cpu().numpy())


def test_eval_writer_writes_the_same_pixels_under_the_same_names(tmp_path):
    from hoig_amd import eval_output as E
    batch = R.mixed_batch()
    images = {k: torch.from_numpy(np.ascontiguousarray(batch[i:i + 3])).to(DEV) for i, k in enumerate(('source', 'imitators', 'gt'))}
    names_a, names_b = ['v1/0001.jpg', 'v2/0002.jpg'], ['v1/0005.jpg', 'v2/0009.jpg']       # (B = 3 >= the two names)
    trees = []
    for flag in (False, True):
        w = E.EvalWriter(str(tmp_path / ('png%d' % flag)), workers=2, device_png=flag)
        w.write_images(images, names_a, names_b)
        w.close()
        assert w.written == 6
        trees.append({os.path.relpath(os.path.join(d, f), w.out_dir): os.path.join(d, f) for d, _, fs in os.walk(w.out_dir) for f in fs})
    assert sorted(trees[0]) == sorted(trees[1]) and len(trees[0]) == 6
    for rel in trees[0]:
        a, b = np.asarray(Image.open(trees[0][rel])), np.asarray(Image.open(trees[1][rel]))
        assert a.shape == (128, 128, 3) and np.array_equal(a, b), rel
    # the device files are the encoder's own (segmented), not Pillow's
    with open(trees[1][os.path.join('gt', 'v1_0001_0005.png')], 'rb') as f:
        assert f.read() == R.encode_host(batch[2:3])[0]
