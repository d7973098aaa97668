"""hoig_jpeg_decode_bgr_u8_par (hoig_amd/csrc/jpeg.hip: the entropy stage parallel inside a restart interval) against Pillow, every
byte, and against the serial entry point's status words; that two calls give the same bytes whatever the buffers held; the plan checks;
and the loader, which now decodes both views of a batch with one call."""
import ctypes
import os

import numpy as np
import pytest
import torch

import data_fixture as FX
import jpeg_reference as R
from test_jpeg_cpu import corrupt_streams, grid, jpeg_frames
from test_jpeg_gpu import _batches, _same, device_decode
from test_jpeg_par_cpu import encoded as case_bytes, noise_file, stuffing_at_a_boundary

pytestmark = pytest.mark.gpu
_p = lambda t: ctypes.c_void_p(t.data_ptr())
_np = lambda a: ctypes.c_void_p(a.ctypes.data)


def _st():
    return torch.cuda.current_stream().cuda_stream


class Batch(object):
    """files packed for the parallel entry point, with its workspace and an output that has 64 guard bytes behind the last image"""

    def __init__(self, datas, subseq=0, fill=0xA5):
        from hoig_amd import _lib as L
        from hoig_amd.data import jpeg as J
        self.plans = [J.parse(d) for d in datas]
        assert all(p is not None for p in self.plans)
        self.n, self.subseq = len(datas), subseq
        buf, self.recs, ivs = J.pack(list(zip(datas, self.plans)))
        self.size = L.lib.hoig_jpeg_decode_par_workspace_bytes(_np(self.recs), self.n, subseq)
        assert self.size > 0
        self.total = sum(p['width'] * p['height'] * 3 for p in self.plans)
        self.out = torch.full((self.total + 64,), fill, dtype=torch.uint8, device='cuda')
        self.work = torch.full((self.size,), fill, dtype=torch.uint8, device='cuda')
        self.status = torch.full((self.n,), -1, dtype=torch.int32, device='cuda')
        self.bytes, self.ivs = torch.from_numpy(buf).cuda(), torch.from_numpy(ivs).cuda()
        self.recs_dev = torch.from_numpy(self.recs.view(np.uint8).reshape(-1)).cuda()

    def args(self, recs=None, work_bytes=None, subseq=None):
        return (_p(self.bytes), self.bytes.numel(), _np(self.recs if recs is None else recs), _p(self.recs_dev), self.n, _p(self.ivs),
                self.ivs.numel(), _p(self.out), self.total, _p(self.status), _p(self.work), self.size if work_bytes is None else work_bytes,
                self.subseq if subseq is None else subseq, _st())

    def decode(self):
        """-> ([BGR uint8 [H][W][3]], status words); the guard bytes are checked"""
        from hoig_amd import _lib as L
        L.call('hoig_jpeg_decode_bgr_u8_par', *self.args())
        flat = self.out.cpu().numpy()
        assert (flat[self.total:] == flat[self.total]).all() and flat[self.total] in (0xA5, 0x3C)
        images = [flat[int(r['out_off']):int(r['out_off']) + p['width'] * p['height'] * 3].reshape(p['height'], p['width'], 3)
                  for r, p in zip(self.recs, self.plans)]
        return images, self.status.cpu().numpy()


@pytest.mark.parametrize('subseq', [0, 32])
@pytest.mark.parametrize('mode', R.MODES)
def test_parallel_device_decode_equals_pillow_every_byte(mode, subseq):
    """13 sizes x 4 qualities of one mode as ONE batch (1 x 1 up to 640 x 480 at quality 100: thousands of sub-sequences, many chunks)"""
    cases = grid(modes=[mode])
    datas = [case_bytes(*c) for c in cases]
    images, status = Batch(datas, subseq).decode()
    assert not status.any(), status
    for c, data, got in zip(cases, datas, images):
        assert np.array_equal(got, R.pillow_bgr(data)), c


@pytest.mark.parametrize('subseq', [0, 32, 64, 256])
def test_the_boundary_cases_on_the_device(subseq):
    """Files with FF | 00 across a sub-sequence boundary at this size, and the noise files whose blocks are longer than a sub-sequence
    and which need as many rounds as they have sub-sequences (tests/test_jpeg_par_cpu.py shows that the cases are reached)."""
    from hoig_amd import _lib as L
    picks = stuffing_at_a_boundary(subseq or L.JPEG_SUBSEQ_BYTES)[:12] if subseq != 32 else []
    assert picks or subseq == 32
    datas = [case_bytes(*c) for c in picks] + [noise_file(k) for k in ('444', '420', 'grey')]
    images, status = Batch(datas, subseq).decode()
    assert not status.any(), status
    for k, (data, got) in enumerate(zip(datas, images)):
        assert np.array_equal(got, R.pillow_bgr(data)), (picks + ['444', '420', 'grey'])[k]


def test_two_decodes_into_differently_filled_buffers_give_the_same_bytes():
    """A coefficient the decoder did not zero, or a state read while its owner wrote it, shows as a difference."""
    picks = [(640, 480, '420', 95), (33, 50, '422', 75), (17, 23, '444', 100), (48, 64, 'restart', 75), (640, 480, 'optimize', 30),
             (40, 31, 'grey', 75), (640, 480, 'restart', 95)]
    datas = [case_bytes(*c) for c in picks] + [noise_file('420')]
    a, b = Batch(datas, 0, fill=0xA5), Batch(datas, 0, fill=0x3C)
    ia, sa = a.decode()
    ib, sb = b.decode()
    assert not sa.any() and not sb.any()
    coef_bytes = int(a.recs[0]['plane_off'])
    assert torch.equal(a.out[:a.total], b.out[:b.total]) and torch.equal(a.work[:coef_bytes], b.work[:coef_bytes])
    for data, got in zip(datas, ia):
        assert np.array_equal(got, R.pillow_bgr(data))
    # and the coefficients are the host twins'
    from test_jpeg_cpu import host_entropy
    from hoig_amd.data import jpeg as J
    _, _, _, work, status = host_entropy([(d, J.parse(d)) for d in datas])
    assert not status.any() and np.array_equal(a.work[:coef_bytes].cpu().numpy(), work[:coef_bytes])


def test_corrupt_streams_give_the_serial_entry_points_status_words():
    """Truncations, injected and lost markers among intact files in one batch: ordinary decode errors, reported through the status
    words -- those of hoig_jpeg_decode_bgr_u8 on the same batch.  The intact files equal Pillow, and so does a following call."""
    from hoig_amd.data import jpeg as J
    bad = [d for _, d, must_fail in corrupt_streams() if must_fail and J.parse(d) is not None]
    good = [case_bytes(48, 64, m, 75) for m in ('420', 'restart', 'grey')] + [case_bytes(640, 480, '420', 75)]
    assert len(bad) >= 20
    datas = []
    for k, d in enumerate(bad):                                        # intact files between the corrupt ones
        datas.append(d)
        if k % 5 == 0:
            datas.append(good[(k // 5) % len(good)])
    intact = [k for k, d in enumerate(datas) if any(d is g for g in good)]
    _, serial = device_decode(datas)
    for subseq in (0, 32):
        images, status = Batch(datas, subseq).decode()
        assert np.array_equal(status, serial), (subseq, status, serial)
        assert all(status[k] == 0 for k in intact) and all(status[k] != 0 for k in range(len(datas)) if k not in intact)
        for k in intact:
            assert np.array_equal(images[k], R.pillow_bgr(datas[k])), k
    images, status = Batch(good).decode()
    assert not status.any()
    for d, got in zip(good, images):
        assert np.array_equal(got, R.pillow_bgr(d))


def test_the_parallel_entry_point_refuses_what_its_kernels_would_index_with():
    from hoig_amd import _lib as L
    b = Batch([case_bytes(48, 64, '420', 75), case_bytes(33, 50, '422', 75)])
    call = lambda **kw: L.lib.hoig_jpeg_decode_bgr_u8_par(*b.args(**kw))
    assert call() == 0
    for field, value in (('out_off', b.total), ('plane_off', b.size), ('coef_off', b.size), ('data_off', b.bytes.numel()),
                         ('interval_first', b.ivs.numel())):
        bad = b.recs.copy()
        bad[1][field] = value
        assert call(recs=bad) == L.EINVAL, field
    bad = b.recs.copy()
    bad[0]['plane_off'] = 0                                            # planes inside the coefficients, which are zeroed as one range
    assert call(recs=bad) == L.EINVAL
    bad = b.recs.copy()
    bad[0]['hs'] = 3
    assert call(recs=bad) == L.EUNSUPPORTED
    for subseq in (-1, 16, 48, 512):
        assert call(subseq=subseq) == L.EINVAL, subseq
    # the serial decoder's workspace is too small by the parallel decoder's table
    serial_size = L.lib.hoig_jpeg_decode_workspace_bytes(_np(b.recs.copy()), b.n)
    assert 0 < serial_size < b.size and call(work_bytes=serial_size) == L.EINVAL and call(work_bytes=b.size - 1) == L.EINVAL
    torch.cuda.synchronize()


# ---- the loader: both views of a batch in one call
def _count_decodes(monkeypatch):
    from hoig_amd import _lib as L
    calls = []
    real = L.call

    def counting(name, *args):
        if name.startswith('hoig_jpeg_'):
            calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, 'call', counting)
    return calls


def test_hov3_and_dexycb_batches_come_from_one_decode_call_each(tmp_path, monkeypatch):
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = jpeg_frames(FX.build(str(tmp_path / 'hov3'), seed=5))
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0003.jpg'), ('MC2_0/0000.jpg', 'ABF1_0/0002.jpg'), ('ABF1_0/0000.jpg', 'ABF1_0/0003.jpg')])
    ycb = FX.build_ycb(str(tmp_path / 'ycb'), seed=6)
    v0, v1 = '20200709-subject-01/20200709_141754/836212060125', '20200813-subject-02/20200813_145612/932122062010'
    FX.write_pairs(ycb, [(v0 + '/1', v1 + '/2'), (v1 + '/0', v0 + '/2'), (v0 + '/0', v0 + '/1')])
    for o in (opt, ycb):
        off = _batches(o, False)
        calls = _count_decodes(monkeypatch)
        on = _batches(o, True)
        assert len(off) == len(on) == 2
        assert calls == ['hoig_jpeg_decode_bgr_u8_par'] * len(on), calls       # ONE call per batch, not one per view
        for a, b in zip(off, on):
            _same(a, b)
        monkeypatch.undo()
        monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)


def test_the_serial_entry_point_stays_selectable_for_a_comparison(tmp_path, monkeypatch):
    from hoig_amd.data import DeviceStage
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    assert DeviceStage.JPEG_ENTRY == 'hoig_jpeg_decode_bgr_u8_par'
    opt = jpeg_frames(FX.build(str(tmp_path), seed=5))
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0003.jpg'), ('MC2_0/0000.jpg', 'ABF1_0/0002.jpg')])
    off = _batches(opt, False)
    monkeypatch.setattr(DeviceStage, 'JPEG_ENTRY', 'hoig_jpeg_decode_bgr_u8')
    calls = _count_decodes(monkeypatch)
    on = _batches(opt, True)
    assert calls == ['hoig_jpeg_decode_bgr_u8'] and len(on) == 1
    _same(off[0], on[0])


def test_a_truncated_frame_in_view_b_is_an_oserror_at_finish_and_the_stage_goes_on(tmp_path, monkeypatch):
    from hoig_amd.data import DatasetFactory, DeviceStage
    from hoig_amd.data.device_stage import collate_raw
    monkeypatch.delenv('HOIG_DEVICE_JPEG', raising=False)
    opt = jpeg_frames(FX.build(str(tmp_path), seed=5))
    FX.write_pairs(opt, [('ABF1_0/0001.jpg', 'MC2_0/0003.jpg'), ('MC2_0/0000.jpg', 'ABF1_0/0002.jpg'),
                         ('ABF1_0/0000.jpg', 'ABF1_0/0003.jpg'), ('MC2_0/0001.jpg', 'MC2_0/0002.jpg')])
    good = _batches(opt, False)
    path = os.path.join(opt.data_dir, 'images', 'train', 'MC2', 'rgb', '0003.jpg')      # view B of the first pair
    data = open(path, 'rb').read()
    with open(path, 'wb') as f:
        f.write(data[:len(data) * 2 // 3])
    opt.device_jpeg = True
    ds = DatasetFactory.get_by_name('hov3', opt, True)
    stage = DeviceStage(ds)
    first, second = collate_raw([ds[0], ds[1]]), collate_raw([ds[2], ds[3]])
    assert path in first['B']['jpeg']['paths'] and path not in first['A']['jpeg']['paths']
    calls = _count_decodes(monkeypatch)
    pending = stage.submit(first)
    with pytest.raises(OSError, match='0003.jpg') as err:
        stage.finish(pending)
    assert 'ABF1' not in str(err.value)                                # only the bad file is named
    _same(good[1], stage(second))
    assert calls == ['hoig_jpeg_decode_bgr_u8_par'] * 2
    torch.cuda.synchronize()
