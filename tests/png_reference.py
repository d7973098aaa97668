"""What the PNG encoder's tests share: seeded content, the shapes, a numpy restatement of the row-filter rule, a chunk parser that
checks every CRC-32, and ctypes wrappers of the host twins (hoig_png_filter_host, hoig_png_deflate_host, hoig_png_encode_host)."""
import ctypes
import struct
import zlib

import numpy as np

SEGMENTS = (4096, 8192, 16384, 32768)
CLASSES = ('noise55', 'noise6', 'smooth', 'rect', 'zeros', 'uniform')


def content(kind, h, w, c, seed=0):
    """One uint8 [h, w, c] image.  'noise55' is metrics_reference.write_pngs' content (gradients + noise 0..55), 'noise6' the same with
    noise 0..6, 'smooth' the same without noise; 'rect' a flat rectangle on black; 'zeros'; 'uniform' noise."""
    rng = np.random.RandomState(1000 * CLASSES.index(kind) + seed)
    if kind == 'zeros':
        return np.zeros((h, w, c), np.uint8)
    if kind == 'uniform':
        return rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    if kind == 'rect':
        a = np.zeros((h, w, c), np.uint8)
        a[h // 4:h - h // 4, w // 3:w - w // 5] = np.array([200, 90, 31], np.uint8)[:c]
        return a
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 199 // max(w - 1, 1), yy * 199 // max(h - 1, 1), (xx + yy) * 199 // max(h + w - 2, 1)], -1)[..., :c]
    top = {'noise55': 56, 'noise6': 7, 'smooth': 1}[kind]
    return (base + rng.randint(0, top, (h, w, c))).astype(np.uint8)


# (H, W, C), the segment sizes it runs at (0: the default), the classes
ALL = CLASSES
SHAPES = [
    ((1, 1, 3), (0,), ALL),                  # a row shorter than any match, one segment, the degenerate codes
    ((1, 1, 1), (0,), ALL),
    ((2, 1, 3), (0,), ALL),                  # no previous pixel
    ((1, 5, 3), (0,), ALL),                  # no previous row
    ((5, 7, 3), (0,), ALL),                  # odd strides
    ((33, 17, 1), (0,), ALL),
    ((40, 70, 3), SEGMENTS, ALL),            # 8440 bytes: two segments at 8192, the cut inside a row
    ((64, 64, 1), SEGMENTS, ALL),            # 4160 bytes: a second segment of 64 bytes at 4096
    ((32, 128, 1), SEGMENTS, ALL),           # 4128 bytes
    ((64, 127, 1), (4096, 0), ALL),          # 8192 bytes: an exact multiple of the segment, no empty tail
    ((64, 64, 3), (4096, 0), ('zeros',)),    # runs of 258 at distance 1 across segment cuts
]
CASES = [(shape, seg, kind) for shape, segs, kinds in SHAPES for seg in segs for kind in kinds]
CASE_IDS = ['%dx%dx%d-s%d-%s' % (s + (seg, kind)) for s, seg, kind in CASES]
MIXED = (128, 128, 3)                        # a batch of 5, a different class per image
WORKLOAD = (256, 256, 3)                     # the workload's own shape, a batch of 3


def mixed_batch():
    return np.stack([content(k, *MIXED, seed=7) for k in CLASSES[:5]])


def workload_batch():
    return np.stack([content(k, *WORKLOAD, seed=3) for k in ('noise55', 'smooth', 'uniform')])


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_stream(img):
    """The rule restated: per row the filter (0..4) whose bytes, read as signed 8-bit, have the smallest sum of absolute values; the
    lowest type on a tie.  Returns the H (1 + W C) bytes."""
    h, w, c = img.shape
    raw = img.reshape(h, w * c).astype(np.int64)
    out = np.zeros((h, 1 + w * c), np.uint8)
    zero = np.zeros(w * c, np.int64)
    for y in range(h):
        x = raw[y]
        up = raw[y - 1] if y else zero
        left = np.concatenate([zero[:c], x[:-c]]) if w > 1 else zero
        upleft = np.concatenate([zero[:c], up[:-c]]) if w > 1 else zero
        cands = [x, x - left, x - up, x - (left + up) // 2, x - paeth(left, up, upleft)]
        cands = [(v & 255).astype(np.uint8) for v in cands]
        sums = [int(np.abs(v.view(np.int8).astype(np.int64)).sum()) for v in cands]
        t = sums.index(min(sums))
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out.reshape(-1)


def parse(png):
    """(ihdr fields, [the data of every IDAT], the inflated stream) of a PNG file; every chunk's CRC-32 is checked, the chunk order too."""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(png):
        n, kind = struct.unpack('>I4s', png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        crc, = struct.unpack('>I', png[at + 8 + n:at + 12 + n])
        assert len(data) == n and crc == zlib.crc32(kind + data), (kind, at)
        chunks.append((kind, data))
        at += 12 + n
    assert at == len(png)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and set(kinds[1:-1]) == {b'IDAT'}, kinds     # no ancillary chunk
    assert chunks[-1][1] == b''
    idat = [d for k, d in chunks if k == b'IDAT']
    return struct.unpack('>IIBBBBB', chunks[0][1]), idat, zlib.decompress(b''.join(idat))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def lib():
    from hoig_amd import _lib as L
    return L


def filter_host(img):
    h, w, c = img.shape
    img = np.ascontiguousarray(img)
    out = np.full(h * (1 + w * c), 0x5A, np.uint8)
    rc = lib().lib.hoig_png_filter_host(_p(img), h, w, c, _p(out))
    assert rc == 0, rc
    return out


def encode_host(batch, segment_bytes=0):
    """The files of a uint8 [B, H, W, C] batch through the twin; the slots' untouched tails are checked against their 0x5A fill."""
    L = lib()
    batch = np.ascontiguousarray(batch)
    b, h, w, c = batch.shape
    stride = L.lib.hoig_png_encode_bound(h, w, c, segment_bytes)
    assert stride > 0, stride
    out = np.full(b * stride + 64, 0x5A, np.uint8)
    sizes = np.zeros(b, np.int32)
    rc = L.lib.hoig_png_encode_host(_p(batch), b, h, w, c, _p(out), stride, _p(sizes), segment_bytes)
    assert rc == 0, rc
    files = []
    for i in range(b):
        assert 0 < sizes[i] <= stride
        assert (out[i * stride + sizes[i]:(i + 1) * stride] == 0x5A).all()
        files.append(out[i * stride:i * stride + sizes[i]].tobytes())
    assert (out[b * stride:] == 0x5A).all()
    return files


def deflate_host(stream, segment_bytes=0, dist_c=0, dist_row=0):
    """(the zlib stream, the bytes of each segment) of any byte string through the twin."""
    L = lib()
    s = np.frombuffer(bytes(stream), np.uint8) if len(stream) else np.zeros(0, np.uint8)
    seg = segment_bytes or 8192
    nseg = max(1, -(-len(s) // seg))
    cap = 2 + len(s) + 10 * nseg + 4
    out = np.full(cap + 16, 0x5A, np.uint8)
    size = ctypes.c_int64(0)
    segs = np.zeros(nseg, np.int32)
    hold = s if len(s) else np.zeros(1, np.uint8)
    rc = L.lib.hoig_png_deflate_host(_p(hold), len(s), segment_bytes, dist_c, dist_row, _p(out), cap, ctypes.byref(size), _p(segs))
    assert rc == 0, rc
    assert 0 < size.value <= cap and (out[size.value:] == 0x5A).all()
    return out[:size.value].tobytes(), segs


def first_block_code_lengths(z):
    """(literal/length code lengths, distance code lengths) that the header of a zlib stream's first block declares (BTYPE 2)."""
    bits = int.from_bytes(z[2:], 'little')
    at = [0]

    def take(n):
        v = (bits >> at[0]) & ((1 << n) - 1)
        at[0] += n
        return v

    assert take(1) in (0, 1) and take(2) == 2, 'not a dynamic block'
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    clen = [0] * 19
    for i in range(hclen):
        clen[order[i]] = take(3)
    code, table = 0, {}
    for n in range(1, 8):                                   # canonical codes, read MSB first
        for s in range(19):
            if clen[s] == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        n, code = 0, 0
        while (n, code) not in table:
            code, n = code << 1 | take(1), n + 1
            assert n <= 7
        s = table[(n, code)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        else:
            lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
    assert len(lens) == hlit + hdist
    return lens[:hlit], lens[hlit:]
