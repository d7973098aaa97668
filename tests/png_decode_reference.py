"""What the PNG decoder's tests share: a chunk writer, a fixed-Huffman token writer for crafted streams, the corpus of good files (each
with Pillow's pixels) and of bad streams (each refused by zlib or Pillow, or of the wrong size), and a runner that puts a batch through
the twin or the device with a guard band of 64 bytes around every output slot and the workspace.  The references are Pillow and zlib."""
import ctypes
import io
import struct
import zlib

import numpy as np
from PIL import Image

import png_reference as R

GUARD = 64
FILL = 0x5A


def D():
    from hoig_amd import png_decode
    return png_decode


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def png_file(w, h, depth, ctype, stream, cuts=(), plte=None, before=(), after=(), interlace=0):
    """A file around a given zlib stream: IHDR, the `before` chunks, PLTE, IDAT chunks cut at the offsets `cuts` (a repeated offset
    gives a zero-length IDAT), the `after` chunks, IEND."""
    f = R_SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, interlace))
    for k, d in before:
        f += chunk(k, d)
    if plte is not None:
        f += chunk(b'PLTE', plte)
    edges = [0] + list(cuts) + [len(stream)]
    for a, b in zip(edges[:-1], edges[1:]):
        f += chunk(b'IDAT', stream[a:b])
    for k, d in after:
        f += chunk(k, d)
    return f + chunk(b'IEND', b'')


R_SIG = b'\x89PNG\r\n\x1a\n'


def pillow_rgb(f):
    return np.asarray(Image.open(io.BytesIO(f)).convert('RGB'))


class FixedTokens(object):
    """One final fixed-Huffman block written token by token; `expected` is what it must inflate to."""

    LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
    LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
    DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
    DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

    def __init__(self):
        self.bits, self.n, self.expected = 0, 0, bytearray()
        self.put(1, 1)
        self.put(1, 2)

    def put(self, v, n):                     # n bits, least significant first
        self.bits |= v << self.n
        self.n += n

    def code(self, v, n):                    # a Huffman code, most significant bit first
        for i in range(n - 1, -1, -1):
            self.put((v >> i) & 1, 1)

    def symbol(self, s):                     # literal / length symbol 0 .. 287
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def literal(self, b):
        self.symbol(b)
        self.expected.append(b)

    def literals(self, data):
        for b in data:
            self.literal(b)

    def match(self, length, dist, track=True):
        k = max(i for i in range(29) if self.LBASE[i] <= length and (i == 28 or length < 258))
        self.symbol(257 + k)
        self.put(length - self.LBASE[k], self.LEXT[k])
        j = max(i for i in range(30) if self.DBASE[i] <= dist)
        self.code(j, 5)
        self.put(dist - self.DBASE[j], self.DEXT[j])
        if track:
            for _ in range(length):
                self.expected.append(self.expected[-dist])

    def stream(self, end=True):
        """The zlib stream: header, the block (closed by the end-of-block symbol unless end=False), the Adler-32 of `expected`."""
        if end:
            self.symbol(256)
        body = self.bits.to_bytes((self.n + 7) // 8, 'little')
        return b'\x78\x01' + body + struct.pack('>I', zlib.adler32(bytes(self.expected)))


def text_like(n, seed=0):
    rng = np.random.RandomState(seed)
    return bytes(rng.choice(np.frombuffer(b'etaoin shrdlu,.\n', np.uint8), n).astype(np.uint8))


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def inflate_host(z, expect):
    """(bytes, status) of a zlib stream through hoig_png_inflate_host; the stream and the output are blocks of exactly their size
    inside guard bands, which must come back untouched."""
    L = R.lib()
    data = np.frombuffer(bytes(z), np.uint8).copy() if len(z) else np.zeros(1, np.uint8)
    out = np.full(expect + 2 * GUARD, FILL, np.uint8)
    st = np.full(1, -1, np.int32)
    rc = L.lib.hoig_png_inflate_host(_p(data), len(z), _p(out[GUARD:]), expect, _p(st))
    assert rc == 0, rc
    assert (out[:GUARD] == FILL).all() and (out[GUARD + expect:] == FILL).all(), 'guard band touched'
    return out[GUARD:GUARD + expect].tobytes(), int(st[0])


def pack_guarded(items):
    """png_decode.pack with a guard band in front of every output slot and behind the last"""
    buf, plans, out_bytes, ws_bytes = D().pack(items)
    for i, p in enumerate(plans):
        p.out_off += GUARD * (i + 1)
    return buf, plans, out_bytes + GUARD * (len(items) + 1), ws_bytes


def check_guards(out, plans, ws, ws_bytes):
    at = 0
    for p in plans:
        assert (out[at:p.out_off] == FILL).all(), 'guard band in front of a slot touched'
        at = p.out_off + p.width * p.height * 3
    assert (out[at:] == FILL).all(), 'guard band behind the last slot touched'
    assert (ws[:GUARD] == FILL).all() and (ws[GUARD + ws_bytes:] == FILL).all(), 'guard band of the workspace touched'


def slots(out, plans):
    return [out[p.out_off:p.out_off + p.width * p.height * 3].reshape(p.height, p.width, 3).copy() for p in plans]


def decode_host(items, bgr=False):
    """([H, W, 3] per image, status per image) of a list of Plans (any sizes) through hoig_png_decode_host, guard bands checked"""
    L = R.lib()
    buf, plans, out_bytes, ws_bytes = pack_guarded(items)
    out = np.full(out_bytes, FILL, np.uint8)
    ws = np.full(ws_bytes + 2 * GUARD, FILL, np.uint8)
    st = np.full(len(items), -1, np.int32)
    rc = L.lib.hoig_png_decode_host(_p(buf), buf.size, plans, len(items), _p(out), out_bytes, _p(st), _p(ws[GUARD:]), ws_bytes, int(bgr))
    assert rc == 0, rc
    check_guards(out, plans, ws, ws_bytes)
    return slots(out, plans), st.tolist()


def decode_device(items, bgr=False, stream=None):
    """decode_host on the device (hoig_png_decode_u8 on the current stream)"""
    import torch
    L = R.lib()
    buf, plans, out_bytes, ws_bytes = pack_guarded(items)
    dev = torch.device('cuda')
    dbuf = torch.from_numpy(buf).to(dev)
    dplans = torch.from_numpy(np.frombuffer(bytes(plans), np.uint8).copy()).to(dev)
    out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device=dev)
    ws = torch.full((ws_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    st = torch.full((len(items),), -1, dtype=torch.int32, device=dev)
    L.call('hoig_png_decode_u8', dbuf.data_ptr(), dbuf.numel(), plans, dplans.data_ptr(), len(items), out.data_ptr(), out_bytes,
           st.data_ptr(), ws.data_ptr() + GUARD, ws_bytes, int(bgr), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out, ws = out.cpu().numpy(), ws.cpu().numpy()
    check_guards(out, plans, ws, ws_bytes)
    return slots(out, plans), st.cpu().tolist()


def plan_of(f):
    plan, why = D().parse(f)
    assert plan is not None, why
    return plan


# ---- good files: (name, file bytes)

SIZES = ((1, 1), (1, 7), (7, 1), (3, 5), (17, 9), (64, 48), (255, 257), (256, 256))        # (W, H)
MODES = ('1', 'L', 'P', 'LA', 'RGBA', 'RGB')


def pillow_image(mode, w, h, seed=1):
    img = R.content('noise55', h, w, 3, seed=seed)
    im = Image.fromarray(img)
    if mode == 'RGBA':
        im = im.convert('RGBA')
        im.putalpha(Image.fromarray(np.ascontiguousarray(img[..., 1])))
    elif mode == 'P':
        im = im.quantize(200)
    elif mode == 'P16':
        im = im.quantize(16)
    elif mode == 'P1':
        im = im.quantize(2)
    else:
        im = im.convert(mode)
    return im


def save(im, **kw):
    b = io.BytesIO()
    im.save(b, 'PNG', **kw)
    return b.getvalue()


def pillow_files(sizes=SIZES, settings=None):
    settings = settings or [{'compress_level': 0}, {'compress_level': 1}, {'compress_level': 6}, {'compress_level': 9}, {'optimize': True}]
    out = []
    for w, h in sizes:
        for mode in MODES:
            for kw in settings:
                out.append(('%s-%dx%d-%s' % (mode, w, h, '-'.join('%s%s' % kv for kv in kw.items())), save(pillow_image(mode, w, h), **kw)))
        out.append(('P-bits1-%dx%d' % (w, h), save(pillow_image('P1', w, h), bits=1)))
        out.append(('P16-optimize-%dx%d' % (w, h), save(pillow_image('P16', w, h), optimize=True)))
    return out


def apply_filter(rows, bpp, types):
    """The filtered stream of raw rows (uint8 [H, rowbytes]) with row y filtered by types[y]"""
    h, n = rows.shape
    raw = rows.astype(np.int64)
    out = bytearray()
    zero = np.zeros(n, np.int64)
    for y in range(h):
        x, up = raw[y], raw[y - 1] if y else zero
        left = np.concatenate([zero[:bpp], x[:-bpp]])[:n]
        upleft = np.concatenate([zero[:bpp], up[:-bpp]])[:n]
        t = types[y]
        pred = [zero, left, up, (left + up) // 2, R.paeth(left, up, upleft)][t]
        out.append(t)
        out += bytes(((x - pred) & 255).astype(np.uint8))
    return bytes(out)


# (colour type, depth): every kind the decoder takes, with its filter unit in bytes
KINDS = ((0, 8, 1), (4, 8, 2), (2, 8, 3), (6, 8, 4), (3, 8, 1), (0, 1, 1), (0, 2, 1), (0, 4, 1), (3, 1, 1), (3, 2, 1), (3, 4, 1))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def hand_filtered_files(w=13, h=11):
    """Every colour type and depth with each of the five filter types forced on every row (and one file that cycles through them)"""
    out = []
    rng = np.random.RandomState(11)
    for ctype, depth, bpp in KINDS:
        rowbytes = (w * CHANNELS[ctype] * depth + 7) // 8
        rows = rng.randint(0, 256, (h, rowbytes)).astype(np.uint8)
        plte = bytes(rng.randint(0, 256, 3 * (1 << depth)).astype(np.uint8)) if ctype == 3 else None
        for t in (0, 1, 2, 3, 4, 'cycle'):
            types = [(y % 5) if t == 'cycle' else t for y in range(h)]
            z = zlib.compress(apply_filter(rows, bpp, types), 6)
            out.append(('hand-c%d-d%d-f%s' % (ctype, depth, t), png_file(w, h, depth, ctype, z, plte=plte)))
    return out


def own_files():
    """The device encoder's files (png_reference.encode_host): all five filter types, dynamic and stored blocks, matches across
    segments, 25 IDATs at 256 x 256 x 3"""
    out = []
    for kind in R.CLASSES:
        out.append(('own-%s-40x70x3-s4096' % kind, R.encode_host(R.content(kind, 40, 70, 3)[None], 4096)[0]))
        out.append(('own-%s-33x17x1' % kind, R.encode_host(R.content(kind, 33, 17, 1)[None])[0]))
    out.append(('own-noise55-256x256x3', R.encode_host(R.content('noise55', 256, 256, 3, seed=3)[None])[0]))
    out.append(('own-smooth-256x256x3', R.encode_host(R.content('smooth', 256, 256, 3, seed=3)[None])[0]))
    return out


def recut_files():
    f = save(pillow_image('RGB', 17, 9))
    plan = plan_of(f)
    z = plan.stream
    anc = [(b'gAMA', struct.pack('>I', 45455)), (b'pHYs', struct.pack('>IIB', 2835, 2835, 1)), (b'tEXt', b'Comment\x00hello')]
    return [('recut-1-byte', png_file(17, 9, 8, 2, z, cuts=range(1, len(z)))),
            ('recut-empty-idats', png_file(17, 9, 8, 2, z, cuts=[0, 0, 5, 5, 5, len(z) // 2, len(z), len(z)])),
            ('ancillary-before', png_file(17, 9, 8, 2, z, before=anc)),
            ('ancillary-after', png_file(17, 9, 8, 2, z, after=anc)),
            ('ancillary-both', png_file(17, 9, 8, 2, z, cuts=[7], before=anc[:2], after=anc[2:]))]


def unsupported_files():
    """(name, file bytes, a word of the reason)"""
    rgb = pillow_image('RGB', 17, 9)
    f = save(rgb)
    z = plan_of(f).stream
    i16 = Image.fromarray((np.arange(17 * 9, dtype=np.uint16) * 257).reshape(9, 17))
    p = pillow_image('P', 17, 9)
    pf = save(p)
    pz = plan_of(pf).stream
    trns = save(pillow_image('P', 17, 9), transparency=3)
    return [('interlaced', png_file(17, 9, 8, 2, z, interlace=1), 'interlaced'),
            ('16-bit', save(i16), '16-bit'),
            ('tRNS', trns, 'tRNS'),
            ('apng', png_file(17, 9, 8, 2, z, before=[(b'acTL', struct.pack('>II', 1, 0))]), 'APNG'),
            ('no-plte', png_file(17, 9, 8, 3, pz), 'PLTE'),
            ('truncated', f[:len(f) - 20], 'truncated'),
            ('truncated-in-header', f[:20], 'truncated'),
            ('not-a-png', b'\xff\xd8\xff\xe0' + bytes(64), 'not a PNG')]


# ---- bad streams: (name, zlib stream, expected size, the one status bit)

def bad_streams():
    L = R.lib()
    good = bytes(range(7)) * 6                       # 42 bytes
    out = []
    t = FixedTokens()
    t.literals(good[:10])
    t.symbol(286)                                    # a literal/length symbol that does not exist
    t.literals(good[10:])
    out.append(('code-symbol-286', t.stream(), 42, L.PNG_ECODE))
    t = FixedTokens()
    t.literals(good[:10])
    t.symbol(257)                                    # length 3 ...
    t.code(30, 5)                                    # ... at a distance code that does not exist
    t.literals(good[10:])
    out.append(('code-distance-30', t.stream(), 42, L.PNG_ECODE))
    # a dynamic block whose code-length code gives all 19 symbols one bit: over-subscribed
    bits, n = 0, 0
    for v, k in [(1, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(1, 3)] * 19:
        bits |= v << n
        n += k
    out.append(('code-over-subscribed', b'\x78\x01' + bits.to_bytes((n + 7) // 8, 'little') + bytes(8) + struct.pack('>I', 1), 42, L.PNG_ECODE))
    out.append(('reserved-block-type', b'\x78\x01' + b'\x07' + bytes(8) + struct.pack('>I', 1), 42, L.PNG_EBTYPE))
    out.append(('stored-len-nlen', b'\x78\x01' + b'\x01' + struct.pack('<HH', 42, 42) + good + struct.pack('>I', zlib.adler32(good)), 42,
                L.PNG_ESTORED))
    t = FixedTokens()
    t.literal(5)
    t.match(3, 2, track=False)                       # two bytes back with one byte written
    t.literals(good[:38])
    out.append(('distance-too-far', t.stream(), 42, L.PNG_EDIST))
    noise = np.random.RandomState(2).randint(0, 32, 3000).astype(np.uint8).tobytes()
    z = zlib.compress(noise, 6)
    out.append(('cut-in-a-dynamic-block', z[:len(z) // 2], 3000, L.PNG_EEARLY))
    z0 = zlib.compress(noise, 0)
    out.append(('cut-in-a-stored-block', z0[:1500], 3000, L.PNG_EEARLY))
    out.append(('cut-in-the-adler', z[:-2], 3000, L.PNG_EEARLY))
    zt = zlib.compress(text_like(3000), 9)
    out.append(('cut-in-a-match-heavy-block', zt[:len(zt) // 2], 3000, L.PNG_EEARLY))
    out.append(('one-byte-more', zlib.compress(noise + b'\x00', 6), 3000, L.PNG_EMORE))
    out.append(('a-match-over-the-end', zlib.compress(bytes(3001), 6), 3000, L.PNG_EMORE))
    out.append(('stored-over-the-end', zlib.compress(noise + b'\x00', 0), 3000, L.PNG_EMORE))
    out.append(('one-byte-less', zlib.compress(noise[:-1], 6), 3000, L.PNG_ELESS))
    out.append(('empty', zlib.compress(b'', 6), 3000, L.PNG_ELESS))
    out.append(('adler-off-by-one', z[:-1] + bytes([z[-1] ^ 1]), 3000, L.PNG_EADLER))
    return out


def refused(z, expect):
    """What makes a stream bad: zlib refuses it, or it does not hold the `expect` bytes a PNG of that size must hold"""
    try:
        return len(zlib.decompress(z)) != expect
    except zlib.error:
        return True


def bad_plans():
    """(name, Plan, the one status bit): the bad streams as images (3000 = 30 rows of 1 + 99 bytes, grey 8 bit; 42 = 2 rows of 1 + 20),
    plus rows whose filter type is above 4 (Pillow refuses those files)"""
    L = R.lib()
    P = D().Plan
    out = []
    for name, z, expect, bit in bad_streams():
        w, h = (99, 30) if expect == 3000 else (20, 2)
        out.append((name, P(w, h, 0, 8, z, None), bit))
    rows = np.random.RandomState(4).randint(0, 256, (6, 1 + 15)).astype(np.uint8)
    rows[:, 0] = (0, 1, 5, 2, 3, 4)
    out.append(('filter-type-5', P(5, 6, 2, 8, zlib.compress(rows.tobytes()), None), L.PNG_EFILTER))
    rows[:, 0] = (0, 1, 4, 2, 3, 255)
    out.append(('filter-type-255', P(5, 6, 2, 8, zlib.compress(rows.tobytes()), None), L.PNG_EFILTER))
    return out


def mixed_batch_files():
    """Every colour type and depth, the five filter types, Pillow's and the encoder's files, sizes up to 255 x 257, in one list"""
    files = [f for n, f in hand_filtered_files() if n.endswith('cycle')]
    files += [f for _, f in pillow_files(sizes=((3, 5), (64, 48)), settings=[{'compress_level': 6}])]
    files += [f for _, f in pillow_files(sizes=((255, 257),), settings=[{'compress_level': 0}, {'optimize': True}])]
    files += [f for _, f in own_files()[:4]] + [f for _, f in recut_files()]
    return files
