"""JPEG frames decoded on the device (hoig_amd/csrc/jpeg.hip): hoig_jpeg_decode_bgr_u8 against Pillow, every byte, over the grid of
tests/jpeg_reference.py; the reconstruction stages alone from the host twin's coefficients; and the loader with ``opt.device_jpeg``
against the loader without it, tensor for tensor."""
import ctypes
import os

import numpy as np
import pytest
import torch

import data_fixture as FX
import jpeg_reference as R
from test_jpeg_cpu import grid, host_entropy, host_status, jpeg_frames

pytestmark = pytest.mark.gpu
_p = lambda t: ctypes.c_void_p(t.data_ptr())
_np = lambda a: ctypes.c_void_p(a.ctypes.data)


def _st():
    return torch.cuda.current_stream().cuda_stream


def device_decode(datas):
    """files -> ([BGR uint8 [H][W][3]], status words), one hoig_jpeg_decode_bgr_u8 call for all of them"""
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    plans = [J.parse(d) for d in datas]
    assert all(p is not None for p in plans)
    buf, recs, ivs = J.pack(list(zip(datas, plans)))
    size = L.lib.hoig_jpeg_decode_workspace_bytes(_np(recs), len(datas))
    assert size > 0
    total = sum(p['width'] * p['height'] * 3 for p in plans)
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device='cuda')           # (64 guard bytes behind the last image)
    work = torch.empty(size, dtype=torch.uint8, device='cuda')
    status = torch.full((len(datas),), -1, dtype=torch.int32, device='cuda')
    b_dev, r_dev, i_dev = torch.from_numpy(buf).cuda(), torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(ivs).cuda()
    L.call('hoig_jpeg_decode_bgr_u8', _p(b_dev), b_dev.numel(), _np(recs), _p(r_dev), len(datas), _p(i_dev), i_dev.numel(), _p(out), total,
           _p(status), _p(work), size, _st())
    flat = out.cpu().numpy()
    assert (flat[total:] == 0xA5).all()
    images = [flat[int(r['out_off']):int(r['out_off']) + p['width'] * p['height'] * 3].reshape(p['height'], p['width'], 3)
              for r, p in zip(recs, plans)]
    return images, status.cpu().numpy()


@pytest.mark.parametrize('mode', R.MODES)
def test_device_decode_equals_pillow_every_byte(mode):
    """13 sizes x 4 qualities of one mode as ONE batch of images of different sizes (1 x 1 up to 640 x 480; odd sizes; chroma planes
    one and two samples wide; with 'restart' hundreds of intervals per image, with 'optimize' per-file Huffman tables)."""
    cases = grid(modes=[mode])
    datas = [R.encode(R.content(w, h, 1 + q % 7), m, q) for w, h, m, q in cases]
    images, status = device_decode(datas)
    assert not status.any(), status
    for c, data, got in zip(cases, datas, images):
        assert np.array_equal(got, R.pillow_bgr(data)), c


def test_reconstruction_alone_from_the_host_twins_coefficients():
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    picks = [(640, 480, '420', 95), (33, 50, '422', 75), (17, 23, '444', 100), (9, 3, '420', 30), (40, 31, 'grey', 75), (48, 64, 'restart', 75)]
    datas = [R.encode(R.content(w, h, 1 + q % 7), m, q) for w, h, m, q in picks]
    _, recs, _, work, status = host_entropy([(d, J.parse(d)) for d in datas])
    assert not status.any()
    total = int(sum(r['width'] * r['height'] * 3 for r in recs))
    out = torch.zeros(total, dtype=torch.uint8, device='cuda')
    w_dev, r_dev = torch.from_numpy(work).cuda(), torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
    L.call('hoig_jpeg_reconstruct_bgr_u8', _np(recs), _p(r_dev), len(datas), _p(out), total, _p(w_dev), w_dev.numel(), _st())
    flat = out.cpu().numpy()
    for c, r, data in zip(picks, recs, datas):
        h, w = int(r['height']), int(r['width'])
        assert np.array_equal(flat[int(r['out_off']):int(r['out_off']) + h * w * 3].reshape(h, w, 3), R.pillow_bgr(data)), c
    # the entry points refuse what their kernels would index with
    bad = recs.copy()
    bad[0]['out_off'] = total
    assert L.lib.hoig_jpeg_reconstruct_bgr_u8(_np(bad), _p(r_dev), len(datas), _p(out), total, _p(w_dev), w_dev.numel(), _st()) == L.EINVAL
    bad = recs.copy()
    bad[1]['plane_off'] = w_dev.numel()
    assert L.lib.hoig_jpeg_reconstruct_bgr_u8(_np(bad), _p(r_dev), len(datas), _p(out), total, _p(w_dev), w_dev.numel(), _st()) == L.EINVAL


def _batches(opt, on):
    from hoig_amd.data import CustomDatasetDataLoader
    opt.device_jpeg = on
    return list(CustomDatasetDataLoader(opt, is_for_train=True).load_data())


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif torch.is_tensor(a[k]):
            assert a[k].device == b[k].device and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_dexycb_loader_with_the_option_equals_the_loader_without(tmp_path, monkeypatch):
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = FX.build_ycb(str(tmp_path), seed=6)
    v0, v1 = '20200709-subject-01/20200709_141754/836212060125', '20200813-subject-02/20200813_145612/932122062010'
    FX.write_pairs(opt, [(v0 + '/1', v1 + '/2'), (v1 + '/0', v0 + '/2'), (v0 + '/0', v0 + '/1')])
    off, on = _batches(opt, False), _batches(opt, True)
    assert len(off) == len(on) == 2
    for a, b in zip(off, on):
        _same(a, b)


def test_hov3_loader_on_jpeg_frames_with_the_option_equals_the_loader_without(tmp_path, monkeypatch):
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = jpeg_frames(FX.build(str(tmp_path), seed=5))
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0003.jpg'), ('MC2_0/0000.jpg', 'ABF1_0/0002.jpg'), ('ABF1_0/0000.jpg', 'ABF1_0/0003.jpg')])
    off, on = _batches(opt, False), _batches(opt, True)
    assert len(off) == len(on) == 2 and 'maskA' in on[0]
    for a, b in zip(off, on):
        _same(a, b)


def test_a_progressive_file_among_baseline_ones_gives_the_same_batch(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = jpeg_frames(FX.build(str(tmp_path), seed=5))
    path = os.path.join(opt.data_dir, 'images', 'train', 'MC2', 'rgb', '0003.jpg')
    Image.open(path).save(path, quality=90, progressive=True)
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0003.jpg'), ('MC2_0/0003.jpg', 'ABF1_0/0002.jpg')])
    off, on = _batches(opt, False), _batches(opt, True)
    assert len(off) == len(on) == 1
    _same(off[0], on[0])


def test_a_truncated_frame_is_an_oserror_at_finish_and_the_stage_goes_on(tmp_path, monkeypatch):
    """The status path: the device reports the file through its status word, finish() of that batch raises OSError with the file's
    name, and the same stage decodes the next batch correctly.  The file goes through the host twin first: same status, on the CPU."""
    from hoig_amd.data import DatasetFactory, DeviceStage
    from hoig_amd.data import jpeg as J
    from hoig_amd.data.device_stage import collate_raw
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = jpeg_frames(FX.build(str(tmp_path), seed=5))
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0003.jpg'), ('MC2_0/0000.jpg', 'ABF1_0/0002.jpg'),
                         ('ABF1_0/0000.jpg', 'ABF1_0/0003.jpg'), ('MC2_0/0001.jpg', 'MC2_0/0002.jpg')])
    good = _batches(opt, False)
    path = os.path.join(opt.data_dir, 'images', 'train', 'MC2', 'rgb', '0003.jpg')
    data = open(path, 'rb').read()
    cut = data[:len(data) * 2 // 3]
    plan = J.parse(cut)
    assert plan is not None and host_status(cut, plan) & (J.EOVERRUN | J.ECODE)
    with open(path, 'wb') as f:
        f.write(cut)
    opt.device_jpeg = True
    ds = DatasetFactory.get_by_name('hov3', opt, True)
    stage = DeviceStage(ds)
    first, second = collate_raw([ds[0], ds[1]]), collate_raw([ds[2], ds[3]])
    pending = stage.submit(first)
    with pytest.raises(OSError, match='0003.jpg'):
        stage.finish(pending)
    _same(good[1], stage(second))
    torch.cuda.synchronize()
