"""The entropy decode that is parallel inside a restart interval (hoig_amd/csrc/jpeg_parallel.h) through its CPU twin
hoig_jpeg_entropy_par_host, against the serial twin hoig_jpeg_entropy_host, which tests/test_jpeg_cpu.py pins to Pillow: the same
coefficient bytes and status words over the grid, at every sub-sequence size and with fewer and more lanes than sub-sequences; the
boundary cases, each shown to be reached before it is compared; and every corrupt stream, at the end of an allocation and under a host
AddressSanitizer build."""
import ctypes
import functools
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_reference as R
from test_jpeg_cpu import ROOT, at_the_end_of_an_allocation, case, corrupt_streams, grid, host_entropy, host_status

_p = lambda a: ctypes.c_void_p(a.ctypes.data)
SUBSEQ = (32, 64, 128, 256)


def interval_table(rec, ivs, S):
    """plan record, interval offsets -> [(begin, end, sub-sequences, blocks)] per restart interval, as jpeg_parallel.h counts them"""
    hs, vs = (int(rec['hs']), int(rec['vs'])) if rec['ncomp'] == 3 else (1, 1)
    mcus = -(-int(rec['width']) // (8 * hs)) * -(-int(rec['height']) // (8 * vs))
    bpm = hs * vs + 2 if rec['ncomp'] == 3 else 1
    n, first, ri = int(rec['n_intervals']), int(rec['interval_first']), int(rec['restart_interval'])
    out = []
    for iv in range(n):
        begin, stop = int(ivs[first + iv]), int(ivs[first + iv + 1])
        end = stop if iv + 1 == n else stop - 2
        m0 = iv * ri if ri else 0
        m1 = min(m0 + ri, mcus) if ri else mcus
        out.append((begin, end, -(-(end - begin) // S) if end > begin else 0, (m1 - m0) * bpm))
    return out


def par_entropy(files, S, lanes):
    """[(bytes, plan)] -> (plan records, workspace uint8, status, rounds, states [n][4], [[(begin, end, nsub, blocks)] per image]) after
    hoig_jpeg_entropy_par_host"""
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    buf, plans, ivs = J.pack(files)
    size = L.lib.hoig_jpeg_decode_par_workspace_bytes(_p(plans), len(files), S)
    assert size > 0, size
    tables = [interval_table(r, ivs, S or L.JPEG_SUBSEQ_BYTES) for r in plans]
    n_states = sum(t[2] for tab in tables for t in tab)
    work = np.full(size, 0x5A, np.uint8)
    status, rounds = np.full(len(files), -1, np.int32), np.full(len(files), -1, np.int32)
    states = np.full((n_states, 4), -1, np.int32)
    rc = L.lib.hoig_jpeg_entropy_par_host(_p(buf), buf.size, _p(plans), len(files), _p(ivs), ivs.size, S, lanes, _p(work), work.size,
                                          _p(status), _p(rounds), _p(states), n_states)
    assert rc == 0, rc
    return plans, work, status, rounds, states, tables


def check_against_the_serial_twin(files, S, lanes, what):
    """-> (rounds, states, tables); asserts the coefficient bytes and status words of the serial twin, a consistent state table and
    rounds <= sub-sequences"""
    from hoig_amd import _lib as L
    _, splans, _, swork, sstatus = serial(tuple(d for d, _ in files))
    size = S or L.JPEG_SUBSEQ_BYTES
    plans, work, status, rounds, states, tables = par_entropy(files, S, lanes)
    assert np.array_equal(status, sstatus) and not status.any(), (what, S, lanes, status, sstatus)
    coef_bytes = int(splans[0]['plane_off'])
    assert all(int(a['coef_off']) == int(b['coef_off']) and int(a['plane_off']) == int(b['plane_off']) for a, b in zip(plans, splans))
    assert np.array_equal(work[:coef_bytes], swork[:coef_bytes]), (what, S, lanes)
    assert (work[coef_bytes:] == 0x5A).all()                            # the twin writes coefficients only
    at = 0
    for i, tab in enumerate(tables):
        most = 0
        for begin, end, nsub, blocks in tab:
            rows = states[at:at + nsub]
            at += nsub
            assert nsub >= 1 and rows[:, 3].sum() == blocks, (what, S, lanes, i, rows[:, 3].sum(), blocks)
            assert tuple(rows[0, :3]) == (0, 0, 0) and (rows[:, 0] >= 0).all() and (rows[:, 0] < 8 * size).all(), (what, S, lanes)
            most = max(most, nsub)
        assert 1 <= rounds[i] <= most, (what, S, lanes, int(rounds[i]), most)
    return rounds, states, tables


@functools.lru_cache(maxsize=None)
def serial(datas):
    from hoig_amd.data import jpeg as J
    return host_entropy([(d, J.parse(d)) for d in datas])


def _files(datas):
    from hoig_amd.data import jpeg as J
    return [(d, J.parse(d)) for d in datas]


@pytest.mark.parametrize('mode', R.MODES)
def test_the_parallel_twin_gives_the_serial_twins_coefficients_over_the_grid(mode):
    for w, h, m, q in grid(modes=[mode]):
        data = case(w, h, m, q)[0]
        for S in SUBSEQ:
            for lanes in (64, 1024):
                check_against_the_serial_twin(_files([data]), S, lanes, (w, h, m, q))


def test_the_parallel_twin_takes_a_batch_of_different_sizes_and_the_default_size():
    from hoig_amd import _lib as L
    datas = [case(17, 23, '420', 75)[0], case(48, 64, 'restart', 95)[0], case(9, 3, 'grey', 30)[0], case(33, 50, '422', 100)[0],
             case(640, 480, 'optimize', 30)[0]]
    for S in SUBSEQ + (0,):
        check_against_the_serial_twin(_files(datas), S, 64, 'batch')
    # 0 is the library's default, which the header exports
    header = open(os.path.join(ROOT, 'include', 'hoig_kernels.h')).read()
    assert '#define HOIG_JPEG_SUBSEQ_BYTES %d\n' % L.JPEG_SUBSEQ_BYTES in header and L.JPEG_SUBSEQ_BYTES in SUBSEQ
    a, b = par_entropy(_files(datas), 0, 64), par_entropy(_files(datas), L.JPEG_SUBSEQ_BYTES, 64)
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[3], b[3])


def test_the_entry_points_refuse_other_sub_sequence_sizes_and_short_buffers():
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    data = case(48, 64, '420', 75)[0]
    buf, plans, ivs = J.pack([(data, J.parse(data))])
    for S in (-1, 1, 16, 48, 100, 512):
        assert L.lib.hoig_jpeg_decode_par_workspace_bytes(_p(plans), 1, S) == L.EINVAL, S
    serial_size = L.lib.hoig_jpeg_decode_workspace_bytes(_p(plans), 1)
    size = L.lib.hoig_jpeg_decode_par_workspace_bytes(_p(plans), 1, 64)
    assert size > serial_size                                           # the planes, then the parallel decoder's table
    work, status, rounds = np.zeros(size, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32)
    states = np.zeros((64, 4), np.int32)
    call = lambda S, lanes, n_states, coef_bytes=size: L.lib.hoig_jpeg_entropy_par_host(
        _p(buf), buf.size, _p(plans), 1, _p(ivs), ivs.size, S, lanes, _p(work), coef_bytes, _p(status), _p(rounds), _p(states), n_states)
    assert call(64, 64, 64) == 0 and status[0] == 0
    assert call(48, 64, 64) == L.EINVAL and call(64, 0, 64) == L.EINVAL
    assert call(64, 64, 1) == L.EINVAL                                  # fewer state rows than sub-sequences
    assert call(64, 64, 64, int(plans[0]['plane_off']) - 1) == L.EINVAL
    bad = plans.copy()
    bad[0]['width'] = 70000
    assert L.lib.hoig_jpeg_decode_par_workspace_bytes(_p(bad), 1, 64) == L.EUNSUPPORTED
    # states and rounds are optional
    assert L.lib.hoig_jpeg_entropy_par_host(_p(buf), buf.size, _p(plans), 1, _p(ivs), ivs.size, 64, 64, _p(work), size, _p(status), None,
                                            None, 0) == 0


# ---- boundary cases: each is shown to be reached, then compared
def scan_of(data):
    from hoig_amd.data import jpeg as J
    plan = J.parse(data)
    return data[plan['scan_offset']:plan['scan_offset'] + plan['scan_length']], plan


@functools.lru_cache(maxsize=None)
def encoded(w, h, mode, quality):
    """case(...)[0] without the restatement's decode"""
    return R.encode(R.content(w, h, 1 + quality % 7), mode, quality)


@functools.lru_cache(maxsize=None)
def stuffing_at_a_boundary(S):
    """grid files without restart markers whose scan has the FF of an FF 00 pair as the last byte of a sub-sequence"""
    out = []
    for w, h, m, q in grid(modes=['444', '422', '420', 'grey', 'optimize']):
        scan, _ = scan_of(encoded(w, h, m, q))
        a = np.frombuffer(scan, np.uint8)
        k = np.arange(S, a.size, S)
        if k.size and ((a[k - 1] == 0xFF) & (a[k] == 0)).any():
            out.append((w, h, m, q))
    return out


@pytest.mark.parametrize('S', [64, 128, 256])
def test_a_sub_sequence_that_begins_with_the_stuffed_zero(S):
    cases = stuffing_at_a_boundary(S)
    assert cases, 'no file of the grid has FF | 00 across a boundary at S = %d' % S
    for c in cases:
        data = case(*c)[0]
        _, states, _ = check_against_the_serial_twin(_files([data]), S, 1024, c)
        a = np.frombuffer(scan_of(data)[0], np.uint8)
        for k in range(S, a.size, S):
            if a[k - 1] == 0xFF and a[k] == 0:
                assert states[k // S, 0] >= 8, (c, k)                   # no symbol starts in the stuffed byte


@functools.lru_cache(maxsize=None)
def noise_file(kind):
    """16 x 16 noise with all-ones quantisation tables: blocks of about 90 bytes, a stream that never synchronises early"""
    from PIL import Image
    g = np.random.Generator(np.random.Philox(key=[23, len(kind)]))
    buf = io.BytesIO()
    if kind == 'grey':
        Image.fromarray(g.integers(0, 256, (16, 16), dtype=np.uint8)).save(buf, 'JPEG', qtables=[[1] * 64])
    else:
        Image.fromarray(g.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(buf, 'JPEG', qtables=[[1] * 64, [1] * 64],
                                                                              subsampling={'444': 0, '420': 2}[kind])
    return buf.getvalue()


@pytest.mark.parametrize('kind', ['444', '420', 'grey'])
def test_noise_files_blocks_longer_than_a_sub_sequence_and_as_many_rounds_as_sub_sequences(kind):
    data = noise_file(kind)
    assert np.array_equal(R.decode_bgr(data), R.pillow_bgr(data))
    for S in (32, 64):
        rounds, states, tables = check_against_the_serial_twin(_files([data]), S, 1024, kind)
        nsub = tables[0][0][2]
        inside = (states[:, 3] == 0) & (states[:, 2] > 0)              # starts inside a block and completes none
        assert inside.any(), (kind, S)
        # The worst case: a block is about three (S = 32) or one and a half (S = 64) sub-sequences long and every coefficient is
        # present, so a lane that guessed "a block starts here" rarely falls into step, and the true state has to walk the stream one
        # sub-sequence per round.  Ordinary files need far fewer rounds than sub-sequences (usually a few per cent, at most about
        # half).  "As many rounds as sub-sequences, or nearly" is taken as: at least three quarters of them -- the last lanes may be
        # right by chance or fall into the padding --, and never more than all of them.
        assert nsub - nsub // 4 <= rounds[0] <= nsub, (kind, S, int(rounds[0]), nsub)
    # the same with fewer lanes than sub-sequences
    check_against_the_serial_twin(_files([data]), 32, 4, kind)


def test_more_sub_sequences_than_lanes():
    data = case(640, 480, '444', 100)[0]
    for S in (128, 32):
        _, _, tables = check_against_the_serial_twin(_files([data]), S, 64, 'large')
        assert tables[0][0][2] > 64 * 64                                # many chunks of 64 lanes
    scan, _ = scan_of(data)
    assert len(scan) > 700000


def test_the_dc_predictor_wraps_as_the_serial_codes_does():
    """DC differences of +2047 in every block of a grey image: the predictor passes 32767 after 17 blocks, and both twins narrow it at
    the store.  The stream is written here (standard tables of a Pillow file, new scan data)."""
    from hoig_amd.data import jpeg as J
    base = case(48, 64, 'grey', 75)[0]
    plan = J.parse(base)
    counts, vals = plan['dc_counts'][0], plan['dc_vals'][0]
    codes, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(int(counts[length - 1])):
            codes[int(vals[p])] = (code, length)
            code, p = code + 1, p + 1
        code <<= 1
    acc, ap = {}, 0
    code = 0
    for length in range(1, 17):
        for _ in range(int(plan['ac_counts'][0][length - 1])):
            acc[int(plan['ac_vals'][0][ap])] = (code, length)
            code, ap = code + 1, ap + 1
        code <<= 1
    bits = ''
    for _ in range(48):                                                # 6 x 8 blocks
        c, n = codes[11]
        bits += format(c, '0%db' % n) + format(2047, '011b')
        c, n = acc[0]
        bits += format(c, '0%db' % n)                                  # EOB
    bits += '1' * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b'\xff', b'\xff\x00')
    data = base[:plan['scan_offset']] + raw + b'\xff\xd9'
    _, _, _, work, status = host_entropy([(data, J.parse(data))])
    dcs = work[:48 * 128].view(np.int16).reshape(48, 64)[:, 0]
    assert status[0] == 0 and dcs[15] == 32752 and dcs[16] < 0       # wrapped
    for S in (32, 64):
        check_against_the_serial_twin(_files([data]), S, 64, 'dc wrap')


# ---- corrupt streams
def par_status(data, plan, S, lanes=64):
    """hoig_jpeg_entropy_par_host on one file that sits at the end of an allocation -> its status word"""
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    _, plans, ivs = J.pack([(data, plan)])
    size = L.lib.hoig_jpeg_decode_par_workspace_bytes(_p(plans), 1, S)
    assert size > 0
    work, status = np.zeros(size, np.uint8), np.full(1, -1, np.int32)
    with at_the_end_of_an_allocation(data) as addr:
        rc = L.lib.hoig_jpeg_entropy_par_host(ctypes.c_void_p(addr), len(data), _p(plans), 1, _p(ivs), ivs.size, S, lanes, _p(work),
                                              work.size, _p(status), None, None, 0)
    assert rc == 0, rc
    return int(status[0])


def test_corrupt_streams_give_the_serial_twins_status_inside_the_buffer():
    from hoig_amd.data import jpeg as J
    seen = 0
    for what, data, must_fail in corrupt_streams():
        plan = J.parse(data)
        if plan is None:
            continue
        want = host_status(data, plan)
        assert want != 0 or not must_fail, what
        seen += 1
        for S in SUBSEQ:
            assert par_status(data, plan, S) == want, (what, S)
        assert par_status(data, plan, 32, lanes=3) == want, what
    assert seen > 80
    data = case(48, 64, 'restart', 75)[0]
    assert par_status(data, J.parse(data), 64) == 0


def test_a_table_that_is_no_prefix_code_is_the_serial_twins_status():
    from hoig_amd.data import jpeg as J
    data = case(16, 16, '420', 75)[0]
    plan = J.parse(data)
    plan['ac_counts'] = plan['ac_counts'].copy()
    plan['ac_counts'][0, 0] = 3
    assert par_status(data, plan, 64) == host_status(data, plan) == J.ECODE


def test_corrupt_streams_under_a_host_address_sanitizer_build_of_the_parallel_twin(tmp_path):
    """The corrupt streams (and the intact ones) through jpeg_host.cpp built with -fsanitize=address, each buffer a heap block of
    exactly its size (tests/jpeg_par_asan_driver.cpp), at every sub-sequence size: no report, and the statuses of the serial twin."""
    from hoig_amd import _lib as L
    from hoig_amd.data import jpeg as J
    cxx = shutil.which(os.environ.get('CXX', 'c++'))
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address', '-static-libasan']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if cxx is None or subprocess.run([cxx] + flags + [str(probe), '-o', str(tmp_path / 'probe')], stdout=subprocess.DEVNULL,
                                     stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip('no host C++ compiler that links an AddressSanitizer runtime (an empty program does not build with %s)' % ' '.join(flags))
    exe = str(tmp_path / 'jpeg_par_asan_driver')
    src = [os.path.join(ROOT, 'hoig_amd', 'csrc', 'jpeg_host.cpp'), os.path.join(ROOT, 'tests', 'jpeg_par_asan_driver.cpp')]
    build = subprocess.run([cxx] + flags + ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'hoig_amd', 'csrc')] + src +
                           ['-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    streams = [(w, d) for w, d, _ in corrupt_streams()] + [('intact ' + m, case(48, 64, m, 75)[0]) for m in R.MODES]
    blob, want = [], []
    for what, data in streams:
        plan = J.parse(data)
        if plan is None:
            continue
        _, plans, ivs = J.pack([(data, plan)])
        expect = host_status(data, plan)
        for S, lanes in ((32, 7), (64, 64), (128, 64), (256, 64)):
            size = L.lib.hoig_jpeg_decode_par_workspace_bytes(_p(plans), 1, S)
            coef_bytes = int(plans[0]['plane_off'])
            assert 0 < coef_bytes < size
            n_states = sum(t[2] for t in interval_table(plans[0], ivs, S))
            blob.append(struct.pack('<qqqqqq', len(data), ivs.size, coef_bytes, S, lanes, n_states) + plans.tobytes() + data + ivs.tobytes())
            want.append('0 %d' % expect)
    case_file = tmp_path / 'cases.bin'
    case_file.write_bytes(struct.pack('<i', len(blob)) + b''.join(blob))
    run = subprocess.run([exe, str(case_file)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and 'AddressSanitizer' not in run.stdout, run.stdout[-3000:]
    assert run.stdout.split('\n')[:len(want)] == want and len(want) > 320
