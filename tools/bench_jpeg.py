"""What decoding the loader's JPEG frames on the device costs (hoig_amd/csrc/jpeg.hip, opt.device_jpeg) -> profiles/jpeg_decode.txt.

Batches of 16 frames (batch 8, two views), 640 x 480, 4:2:0, quality 90, of the test fixture's smooth-plus-noise content -- synthetic: no
real HO3D-v3 or DexYCB frame has been measured -- without restart markers and with one restart interval per MCU row.
  host    seconds per frame in this process: Pillow decode (imread_bgr), and file read + jpeg.parse (what a worker does with the option)
  device  one batch's decode alone, by events (20 repetitions after a warm-up), through the serial entry point (hoig_jpeg_decode_bgr_u8)
          and through the one that is parallel inside a restart interval (hoig_jpeg_decode_bgr_u8_par) at every sub-sequence size, with
          the decode rounds per frame that the host twin counts for the same workgroup; and its H2D bytes against 16 x 921,600
  step    the loader-fed training step (tools/bench_loader_step.py's last leg: workers + DeviceStage + raw stage one batch ahead +
          set_input + step) on a tree of JPEG frames: option off, on with the serial entry point, on with the parallel one (one call
          per batch either way), alternating, `rounds` rounds
usage: python tools/bench_jpeg.py [--out FILE] [--steps 24] [--workers 4] [--rounds 3] [--decode-only]
(--decode-only: just the device leg, for a `rocprofv3 --kernel-trace --stats -- python tools/bench_jpeg.py --decode-only` run)"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import jpeg_reference as R                                  # noqa: E402  (the fixture's content and the encoder settings)
from hoig_amd import _lib as L                              # noqa: E402
from hoig_amd.data import jpeg as J                         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=None)
ap.add_argument('--steps', type=int, default=24)
ap.add_argument('--workers', type=int, default=4)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--decode-only', action='store_true')
args = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def encode(img, restart):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=90, subsampling=2, **({'restart_marker_rows': 1} if restart else {}))
    return buf.getvalue()


def host_rounds(buf, recs, ivs, n, subseq):
    """decode rounds per frame, from the host twin walking the device's workgroup (512 / 256 / 128 lanes for 32, 64 / 128 / 256 bytes)"""
    q = lambda a: ctypes.c_void_p(a.ctypes.data)
    work = np.zeros(int(recs[0]['plane_off']), np.uint8)
    status, rounds = np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.call('hoig_jpeg_entropy_par_host', q(buf), buf.size, q(recs), n, q(ivs), ivs.size, subseq, min(512, 32768 // subseq), q(work),
           work.size, q(status), q(rounds), None, 0)
    assert not status.any()
    return rounds


def device_leg(datas, label, reps=20, subseq=None):
    """-> (ms per batch: median of reps, spread), the decode call alone: the files are already on the device.  subseq None: the serial
    entry point; else the parallel one with sub-sequences of that many bytes"""
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    plans = [J.parse(d) for d in datas]
    buf, recs, ivs = J.pack(list(zip(datas, plans)))
    if subseq is None:
        size = L.lib.hoig_jpeg_decode_workspace_bytes(ctypes.c_void_p(recs.ctypes.data), len(datas))
    else:
        size = L.lib.hoig_jpeg_decode_par_workspace_bytes(ctypes.c_void_p(recs.ctypes.data), len(datas), subseq)
    total = sum(q['width'] * q['height'] * 3 for q in plans)
    out = torch.empty(total, dtype=torch.uint8, device='cuda')
    work = torch.empty(size, dtype=torch.uint8, device='cuda')
    status = torch.empty(len(datas), dtype=torch.int32, device='cuda')
    b_dev, r_dev, i_dev = torch.from_numpy(buf).cuda(), torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(ivs).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def run():
        L.call('hoig_jpeg_decode_bgr_u8' if subseq is None else 'hoig_jpeg_decode_bgr_u8_par', p(b_dev), b_dev.numel(),
               ctypes.c_void_p(recs.ctypes.data), p(r_dev), len(datas), p(i_dev), i_dev.numel(), p(out), total, p(status), p(work), size,
               *(((subseq,) if subseq is not None else ()) + (st,)))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    want = np.concatenate([R.pillow_bgr(d).reshape(-1) for d in datas])
    assert np.array_equal(out.cpu().numpy(), want), 'the device decode differs from Pillow'
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    h2d = buf.size + recs.nbytes + ivs.nbytes
    how = 'serial entry' if subseq is None else 'parallel, %3d bytes' % subseq
    say('%-22s %-19s: decode of one batch alone %.3f ms (median of %d; min %.3f, max %.3f); %d restart intervals per frame; equal to Pillow, every byte'
        % (label, how, float(np.median(ms)), reps, min(ms), max(ms), len(plans[0]['intervals']) - 1))
    if subseq is None:
        say('%-22s  H2D per batch %d bytes (files %d + plans %d + interval offsets %d) against %d of decoded frames: %.1f%%'
            % ('', h2d, buf.size, recs.nbytes, ivs.nbytes, len(datas) * 921600, 100.0 * h2d / (len(datas) * 921600)))
    else:
        r = host_rounds(buf, recs, ivs, len(datas), subseq)
        say('%-22s  decode rounds per frame (the largest among its intervals): median %d, min %d, max %d; sub-sequences per frame: median %d'
            % ('', int(np.median(r)), r.min(), r.max(), int(np.median([-(-q['scan_length'] // subseq) for q in plans]))))
    return float(np.median(ms)), max(ms) - min(ms)


frames = [R.content(640, 480, k) for k in range(16)]
plain, restart = [encode(f, False) for f in frames], [encode(f, True) for f in frames]
say('frames: 16 x 640 x 480, 4:2:0, quality 90, synthetic smooth-plus-noise content (tests/data_fixture.py); NO real HO3D-v3 / DexYCB frame was measured')
say('bytes per frame: %.0f without restart markers, %.0f with one interval per MCU row (decoded: 921600)'
    % (np.mean([len(d) for d in plain]), np.mean([len(d) for d in restart])))
SUBSEQ = (32, 64, 128, 256)
ms_plain, sp_plain = device_leg(plain, 'no restart markers')
par_plain = {S: device_leg(plain, 'no restart markers', subseq=S) for S in SUBSEQ}
ms_restart, sp_restart = device_leg(restart, 'one interval per row')
par_restart = {S: device_leg(restart, 'one interval per row', subseq=S) for S in SUBSEQ}
S0 = L.JPEG_SUBSEQ_BYTES
say('conditions, at the default of %d bytes (HOIG_JPEG_SUBSEQ_BYTES):' % S0)
say('  no restart markers  : parallel %.3f ms < serial %.3f ms by more than the two spreads (%.3f + %.3f): %s'
    % (par_plain[S0][0], ms_plain, par_plain[S0][1], sp_plain,
       'MET' if ms_plain - par_plain[S0][0] > par_plain[S0][1] + sp_plain else 'NOT MET'))
say('  one interval per row: parallel %.3f ms not above serial %.3f ms by more than the two spreads (%.3f + %.3f): %s'
    % (par_restart[S0][0], ms_restart, par_restart[S0][1], sp_restart,
       'MET' if par_restart[S0][0] - ms_restart <= par_restart[S0][1] + sp_restart else 'NOT MET'))
if args.decode_only:
    sys.exit(0)

# ---- host side, this process
from hoig_amd.data.hov3_dataset import imread_bgr          # noqa: E402
with tempfile.TemporaryDirectory() as d:
    paths = []
    for k, data in enumerate(plain):
        paths.append(os.path.join(d, '%04d.jpg' % k))
        with open(paths[-1], 'wb') as f:
            f.write(data)

    def per_frame(fn, reps=5):
        for q in paths:
            fn(q)
        t = time.perf_counter()
        for _ in range(reps):
            for q in paths:
                fn(q)
        return (time.perf_counter() - t) / (reps * len(paths))
    s_pil = per_frame(imread_bgr)
    s_parse = per_frame(lambda q: J.parse(open(q, 'rb').read()))
say('host, one process: Pillow decode (imread_bgr) %.3f ms per frame; read + jpeg.parse %.3f ms per frame' % (s_pil * 1e3, s_parse * 1e3))

# ---- the loader-fed step, option off / on
import data_fixture as FX                                  # noqa: E402
from test_hand_recovery_gpu import _assets                 # noqa: E402
from test_jpeg_cpu import jpeg_frames                      # noqa: E402
from common import opt_namespace                           # noqa: E402
from hoig_amd import ops                                   # noqa: E402
from hoig_amd.data import CustomDatasetDataLoader, DeviceStage   # noqa: E402
from hoig_amd.mano import ManoModel                        # noqa: E402
from hoig_amd.models import ModelsFactory                  # noqa: E402
from oracle import mano_oracle as M                        # noqa: E402

B, steps = 8, args.steps
ops.set_precision('bf16x3:f16x2')
assets, nv = _assets([2, 5], 21)
with tempfile.TemporaryDirectory() as root:
    opt_d = jpeg_frames(FX.build(root, seed=8, frames=B, n_obj_verts=nv), quality=90)
    opt_d.batch_size, opt_d.n_threads_train = B, args.workers
    vid = lambda k: ('ABF1_0', 'MC2_0')[k % 2]
    FX.write_pairs(opt_d, [('%s/%04d.jpg' % (vid(k), k % B), '%s/%04d.jpg' % (vid(k), (k + 3) % B)) for k in range(B * (steps + 4))])
    opt = opt_namespace(gen_name='generator_spade_attn', local_rank=0, image_size=256)
    opt.mano_model = opt_d.mano_model = ManoModel.from_dict(M.synthetic_model(4))
    opt.object_assets = opt_d.object_assets = assets
    opt_d.image_size, opt_d.loader_prepares = 256, True
    torch.manual_seed(3)
    model = ModelsFactory.get_by_name('trainer', opt, use_ddp=False)
    model.set_train()

    def leg(on, entry='hoig_jpeg_decode_bgr_u8_par'):
        opt_d.device_jpeg = on
        DeviceStage.JPEG_ENTRY = entry
        k, t = 0, None
        for b in CustomDatasetDataLoader(opt_d, is_for_train=True).load_data():
            if k == 4:                                      # (the first batches pay the worker start-up)
                torch.cuda.synchronize()
                t = time.perf_counter()
            model.set_input(b)
            model.optimize_parameters()
            k += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / (k - 4) * 1e3
    leg(False)                                              # warm-up of everything the timed legs use
    leg(True, 'hoig_jpeg_decode_bgr_u8')
    leg(True)
    off, ser, on = [], [], []
    for _ in range(args.rounds):
        off.append(leg(False))
        ser.append(leg(True, 'hoig_jpeg_decode_bgr_u8'))
        on.append(leg(True))
say('loader-fed step (batch 8 = 16 frames per step, %d workers, %d timed steps per leg, %d rounds alternating):' % (args.workers, steps, args.rounds))
say('  option off: %s ms   (mean %.2f, spread %.2f)' % (' / '.join('%.2f' % v for v in off), np.mean(off), max(off) - min(off)))
say('  option on, serial entry, one call per batch  : %s ms   (mean %.2f, spread %.2f)'
    % (' / '.join('%.2f' % v for v in ser), np.mean(ser), max(ser) - min(ser)))
say('  option on, parallel entry, one call per batch: %s ms   (mean %.2f, spread %.2f)'
    % (' / '.join('%.2f' % v for v in on), np.mean(on), max(on) - min(on)))
gap = float(np.mean(on) - np.mean(off))
say('the step with the option on (parallel) against off: %+.2f ms (%s)'
    % (gap, 'within the spreads' if abs(gap) <= (max(on) - min(on)) + (max(off) - min(off)) else ('SLOWER' if gap > 0 else 'faster')))
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
