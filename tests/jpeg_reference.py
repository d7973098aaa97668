"""A numpy restatement of the baseline JPEG decode that Pillow (libjpeg-turbo) performs: the reference of tests/test_jpeg_cpu.py and
tests/test_jpeg_gpu.py.  It shares no code with hoig_amd/data/jpeg.py or the kernels: its own marker walk, a bit-serial Huffman decode
(T.81 F.2.2), then the four rules the device decoder is pinned to:

1. IDCT: jidctint (islow), CONST_BITS 13, PASS1_BITS 2, columns first (descale 11), then rows (descale 18), clamp(x + 128, 0, 255).
2. A component plane is cropped to ceil(W h / hmax) x ceil(H v / vmax) before upsampling: edges replicate the last REAL row / column.
3. Fancy upsampling: h2v1 (3a + left + 1) >> 2, (3a + right + 2) >> 2, end samples copied; h2v2 colsum = 3 near + far,
   (3c + cleft + 8) >> 4, (3c + cright + 7) >> 4, ends (4c + 8) >> 4 and (4c + 7) >> 4; a chroma plane of width <= 2 is replicated.
4. R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), clamped.
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def _headers(data):
    """-> dict(width, height, comps [(h, v, quant[64] row-major, dc table, ac table)], dri, scan (bytes of entropy-coded data))."""
    q, huff, dri, pos = {}, {}, 0, 2
    assert data[:2] == b'\xff\xd8'
    while True:
        assert data[pos] == 0xFF
        m, length = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + length]
        if m in (0xC0, 0xC1):
            assert seg[0] == 8
            height, width = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            frame = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                counts = list(seg[at + 1:at + 17])
                vals = list(seg[at + 17:at + 17 + sum(counts)])
                codes, code, k = {}, 0, 0
                for length_ in range(1, 17):
                    for _ in range(counts[length_ - 1]):
                        codes[(length_, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                huff[(seg[at] >> 4, seg[at] & 15)] = codes
                at += 17 + len(vals)
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                wide = seg[at] >> 4
                raw = seg[at + 1:at + 1 + (128 if wide else 64)]
                t = [(raw[2 * i] << 8) | raw[2 * i + 1] for i in range(64)] if wide else list(raw)
                nat = [0] * 64
                for i, v in enumerate(t):
                    nat[ZIGZAG[i]] = v
                q[seg[at] & 15] = np.array(nat, np.int64)
                at += 1 + len(raw)
        elif m == 0xDD:
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            comps = []
            for c, (cid, h, v, tq) in enumerate(frame):
                assert seg[1 + 2 * c] == cid
                comps.append((h, v, q[tq], huff[(0, seg[2 + 2 * c] >> 4)], huff[(1, seg[2 + 2 * c] & 15)]))
            if len(comps) == 1:
                comps = [(1, 1) + comps[0][2:]]
            return dict(width=width, height=height, comps=comps, dri=dri, scan=data[pos + 2 + length:])
        pos += 2 + length


class _Bits(object):
    def __init__(self, scan):
        self.d, self.p, self.acc, self.n = scan, 0, 0, 0

    def bit(self):
        if self.n == 0:
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                assert self.d[self.p] == 0, 'marker inside an interval'
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, codes):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = codes.get((length, code))
            if s is not None:
                return s
        raise ValueError('no Huffman code matches')

    def left(self):
        """whole bytes between the reader and the next marker (an encoder leaves none: it pads the last byte and writes the marker)"""
        p = self.p
        while not (self.d[p] == 0xFF and self.d[p + 1] != 0):
            p += 1
        return p - self.p

    def restart(self, k):
        assert self.left() == 0, 'bytes left in front of RST%d' % (k & 7)
        self.n = 0                                      # the padding bits
        assert self.d[self.p] == 0xFF and self.d[self.p + 1] == 0xD0 + (k & 7), 'RST%d expected' % (k & 7)
        self.p += 2


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def decode_coefficients(data):
    """-> (info, [per component int16 [block rows][block columns][64]]): quantised coefficients, row-major inside a block, of the
    PADDED planes (whole MCUs)."""
    info = _headers(bytes(data))
    W, H, comps = info['width'], info['height'], info['comps']
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coefs = [np.zeros((mcuy * v, mcux * h, 64), np.int16) for h, v, _, _, _ in comps]
    br, pred = _Bits(info['scan']), [0] * len(comps)
    for m in range(mcux * mcuy):
        if info['dri'] and m and m % info['dri'] == 0:
            br.restart(m // info['dri'] - 1)
            pred = [0] * len(comps)
        my, mx = divmod(m, mcux)
        for c, (h, v, _, dc, ac) in enumerate(comps):
            for y in range(v):
                for x in range(h):
                    blk = coefs[c][my * v + y, mx * h + x]
                    s = br.symbol(dc)
                    if s:
                        pred[c] += _extend(br.bits(s), s)
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = br.symbol(ac)
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                            k += 1
                        elif r == 15:
                            k += 16
                            if k > 64:
                                raise ValueError('a run of zeros leaves the block')
                        else:
                            break
    info['left'] = br.left()
    return info, coefs


def _idct8(d, shift):
    """jidctint's 1-D pass on d[..., 8] (int64), descaled by `shift`."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    tmp0, tmp1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct_plane(coef, quant):
    """[bh][bw][64] quantised coefficients -> uint8 [8 bh][8 bw]"""
    bh, bw, _ = coef.shape
    d = (coef.astype(np.int64) * quant).reshape(bh, bw, 8, 8)
    d = _idct8(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)            # columns
    d = _idct8(d, 18)                                              # rows
    return np.clip(d + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2v1(p):
    a = p.astype(np.int64)
    cw = a.shape[1]
    if cw <= 2:
        return np.repeat(a, 2, axis=1)
    left, right = np.concatenate([a[:, :1], a[:, :-1]], 1), np.concatenate([a[:, 1:], a[:, -1:]], 1)
    even, odd = (3 * a + left + 1) >> 2, (3 * a + right + 2) >> 2
    even[:, 0], odd[:, -1] = a[:, 0], a[:, -1]
    return np.stack([even, odd], -1).reshape(a.shape[0], 2 * cw)


def _h2v2(p):
    a = p.astype(np.int64)
    ch, cw = a.shape
    if cw <= 2:
        return np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)
    up, down = np.concatenate([a[:1], a[:-1]], 0), np.concatenate([a[1:], a[-1:]], 0)
    rows = []
    for far in (up, down):
        c = 3 * a + far
        left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
        even, odd = (3 * c + left + 8) >> 4, (3 * c + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * c[:, 0] + 8) >> 4, (4 * c[:, -1] + 7) >> 4
        rows.append(np.stack([even, odd], -1).reshape(ch, 2 * cw))
    return np.stack(rows, 1).reshape(2 * ch, 2 * cw)


def reconstruct(info, coefs):
    """Quantised coefficients -> BGR uint8 [H][W][3] (what cv2.imread / hoig_amd's imread_bgr return)."""
    W, H, comps = info['width'], info['height'], info['comps']
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    planes = []
    for (h, v, quant, _, _), coef in zip(comps, coefs):
        p = idct_plane(coef, quant)[:-(-H * v // vmax), :-(-W * h // hmax)]
        if (hmax // h, vmax // v) == (2, 1):
            p = _h2v1(p)
        elif (hmax // h, vmax // v) == (2, 2):
            p = _h2v2(p)
        else:
            assert (h, v) == (hmax, vmax)
        planes.append(p[:H, :W].astype(np.int64))
    if len(planes) == 1:
        return np.repeat(planes[0].astype(np.uint8)[:, :, None], 3, axis=2)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode_bgr(data):
    return reconstruct(*decode_coefficients(data))


def pillow_bgr(data):
    """What the package's host decoder gives for these bytes (hov3_dataset.imread_bgr without the file)."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


# ---- the grid of encodings both test files walk
SIZES = [(1, 1), (2, 2), (9, 3), (5, 4), (7, 5), (3, 9), (8, 6), (16, 16), (17, 23), (33, 50), (40, 31), (48, 64), (640, 480)]   # (W, H)
MODES = ['444', '422', '420', 'grey', 'restart', 'optimize']
QUALITIES = [30, 75, 95, 100]


def content(w, h, seed):
    """tests/data_fixture.py's frames: smooth ramps plus noise."""
    g = np.random.Generator(np.random.Philox(key=[seed, w * 1000 + h]))
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.stack([xx * 0.37 + yy * 0.11, yy * 0.41, (xx + yy) * 0.23], -1) + 40 * seed) % 256
    return np.clip(base + g.integers(-20, 20, base.shape), 0, 255).astype(np.uint8)


def encode(img, mode, quality):
    import io
    from PIL import Image
    kw = {'444': dict(subsampling=0), '422': dict(subsampling=1), '420': dict(subsampling=2), 'grey': {},
          'restart': dict(subsampling=2, restart_marker_blocks=2), 'optimize': dict(subsampling=2, optimize=True)}[mode]
    im = Image.fromarray(img[:, :, 0] if mode == 'grey' else img)
    buf = io.BytesIO()
    im.save(buf, 'JPEG', quality=quality, **kw)
    return buf.getvalue()
