"""Host half of the device JPEG decoder (hoig_amd/csrc/jpeg.hip): header parsing and batch packing, pure Python + numpy -- this is what
a DataLoader worker runs when ``opt.device_jpeg`` is on, and nothing here touches HIP.

``parse(data)`` walks the markers of a JPEG file and returns a *plan* (a dict: size, sampling, per-component quantisation and Huffman
tables, DRI, where the scan's entropy-coded data lies and where its restart intervals start), or ``None`` for a file outside the
supported set -- the caller then decodes that file on the host as before.  Supported: baseline and extended-sequential Huffman (SOF0 /
SOF1), 8-bit, one interleaved scan, YCbCr 4:4:4 / 4:2:2 (2x1) / 4:2:0 (2x2) or a single component, EXIF orientation 1 or none.

``pack(items)`` lays a batch's files and plans out for ``hoig_jpeg_decode_bgr_u8`` / ``hoig_jpeg_decode_bgr_u8_par``: one byte buffer, the plan records
(``PLAN_DTYPE`` restates ``hoig_jpeg_plan`` of include/hoig_kernels.h) and the interval offsets."""
import struct

import numpy as np

PLAN_DTYPE = np.dtype([
    ('data_off', '<i8'), ('out_off', '<i8'), ('coef_off', '<i8'), ('plane_off', '<i8'),
    ('data_len', '<i4'), ('width', '<i4'), ('height', '<i4'), ('ncomp', '<i4'), ('hs', '<i4'), ('vs', '<i4'),
    ('restart_interval', '<i4'), ('n_intervals', '<i4'), ('interval_first', '<i4'), ('reserved', '<i4', (3,)),
    ('quant', '<u2', (3, 64)),
    ('dc_counts', 'u1', (3, 16)), ('dc_vals', 'u1', (3, 16)), ('ac_counts', 'u1', (3, 16)), ('ac_vals', 'u1', (3, 256))])
assert PLAN_DTYPE.itemsize == 1376

ECODE, EOVERRUN, EMARKER, ETRAILING = 1, 2, 4, 8
_STATUS = {ECODE: 'invalid Huffman code', EOVERRUN: 'data ends early', EMARKER: 'restart marker missing',
           ETRAILING: 'bytes left after the last block'}

# zigzag position -> row-major position in the block
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


def status_text(word):
    return ', '.join(t for bit, t in _STATUS.items() if word & bit) or 'ok'


def _exif_orientation(seg):
    """The Orientation tag (0x0112) of an APP1 Exif segment's IFD0, or 1."""
    if len(seg) < 14 or seg[:6] != b'Exif\x00\x00':
        return 1
    tiff = seg[6:]
    order = {b'II': '<', b'MM': '>'}.get(tiff[:2])
    if order is None:
        return 1
    try:
        ifd, = struct.unpack(order + 'I', tiff[4:8])
        count, = struct.unpack(order + 'H', tiff[ifd:ifd + 2])
        for k in range(count):
            tag, kind, n = struct.unpack(order + 'HHI', tiff[ifd + 2 + 12 * k:ifd + 10 + 12 * k])
            if tag == 0x0112:
                return struct.unpack(order + 'H', tiff[ifd + 10 + 12 * k:ifd + 12 + 12 * k])[0]
    except struct.error:
        return None                                   # a damaged Exif block: leave the file to the host decoder
    return 1


def parse(data):
    """bytes of a JPEG file -> plan dict, or None (not a JPEG this decoder takes)."""
    a = np.frombuffer(data, dtype=np.uint8)
    n = a.size
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        return None
    quant, huff = {}, {}
    frame = None
    dri, jfif, adobe = 0, False, None
    pos = 2
    while True:
        if pos + 4 > n or a[pos] != 0xFF:
            return None
        m = int(a[pos + 1])
        if m == 0xFF:                                  # fill byte
            pos += 1
            continue
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if m == 0xD9:
            return None                                # EOI before any scan
        length = (int(a[pos + 2]) << 8) | int(a[pos + 3])
        if length < 2 or pos + 2 + length > n:
            return None
        seg = data[pos + 4:pos + 2 + length]
        if m == 0xC0 or m == 0xC1:
            if frame is not None or len(seg) < 6:
                return None
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8 or nc not in (1, 3) or h == 0 or w == 0 or len(seg) != 6 + 3 * nc:
                return None
            frame = (w, h, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)])
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None                                # progressive, lossless, differential, arithmetic
        elif m == 0xCC:
            return None                                # arithmetic conditioning
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    return None
                tc, th = seg[at] >> 4, seg[at] & 15
                counts = np.frombuffer(seg[at + 1:at + 17], np.uint8)
                total = int(counts.sum())
                if tc > 1 or th > 3 or at + 17 + total > len(seg) or total > (256 if tc else 16):
                    return None
                huff[(tc, th)] = (counts.copy(), np.frombuffer(seg[at + 17:at + 17 + total], np.uint8).copy())
                at += 17 + total
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or at + 1 + size > len(seg):
                    return None
                t = np.frombuffer(seg[at + 1:at + 1 + size], '>u2' if pq else np.uint8).astype(np.uint16)
                nat = np.zeros(64, np.uint16)
                nat[ZIGZAG] = t
                quant[tq] = nat
                at += 1 + size
        elif m == 0xDD:
            if len(seg) != 2:
                return None
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            jfif = jfif or seg[:5] == b'JFIF\x00'
        elif m == 0xE1:
            if _exif_orientation(seg) != 1:
                return None
        elif m == 0xEE:
            if seg[:5] == b'Adobe' and len(seg) >= 12:
                adobe = seg[11]
        elif m == 0xDC:
            return None                                # DNL
        elif m == 0xDA:
            break
        pos += 2 + length
    if frame is None:
        return None
    w, h, comps = frame
    nc = len(comps)
    if len(seg) != 4 + 2 * nc or seg[0] != nc:         # every component in ONE scan
        return None
    if (seg[1 + 2 * nc], seg[2 + 2 * nc], seg[3 + 2 * nc]) != (0, 63, 0):
        return None
    if nc == 3:
        # libjpeg's colour-space guess (jdapimin.c default_decompress_parms): JFIF says YCbCr; else Adobe's transform flag; else the ids
        ids = tuple(c[0] for c in comps)
        if not jfif and (adobe not in (None, 1) or (adobe is None and ids == (82, 71, 66))):
            return None
        if (comps[1][1], comps[1][2], comps[2][1], comps[2][2]) != (1, 1, 1, 1) or (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)):
            return None
        hs, vs = comps[0][1], comps[0][2]
    else:
        hs = vs = 1                                    # a single-component scan is never interleaved: its sampling factors do not matter
    plan = {'width': w, 'height': h, 'ncomp': nc, 'hs': hs, 'vs': vs, 'restart_interval': dri,
            'quant': np.zeros((3, 64), np.uint16), 'dc_counts': np.zeros((3, 16), np.uint8), 'dc_vals': np.zeros((3, 16), np.uint8),
            'ac_counts': np.zeros((3, 16), np.uint8), 'ac_vals': np.zeros((3, 256), np.uint8)}
    for c, (cid, _, _, tq) in enumerate(comps):
        if seg[1 + 2 * c] != cid:                      # (scan order = frame order: what every encoder writes)
            return None
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if tq not in quant or (0, td) not in huff or (1, ta) not in huff:
            return None
        plan['quant'][c] = quant[tq]
        for kind, sel, cn, vn in ((0, td, 'dc_counts', 'dc_vals'), (1, ta, 'ac_counts', 'ac_vals')):
            counts, vals = huff[(kind, sel)]
            plan[cn][c] = counts
            plan[vn][c, :vals.size] = vals
    start = pos + 2 + length
    # the scan's data ends at the first marker that is neither a stuffed FF 00, a fill FF nor RSTn; the RSTn on the way are the interval ends
    ff = np.flatnonzero(a[start:n - 1] == 0xFF) + start
    nxt = a[ff + 1]
    other = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    end = int(other[0]) if other.size else n           # (no marker: a truncated file; the decoder will report the overrun)
    if other.size and a[end + 1] != 0xD9:
        return None                                    # another scan, or tables between scans
    if ((nxt == 0xFF) & (ff < end)).any():
        return None                                    # fill bytes (FF FF) in front of a marker: legal, rare, left to the host decoder
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7) & (ff < end)]
    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    n_int = -(-mcus // dri) if dri else 1
    # interval k runs from its start to the k-th RST marker; markers that are missing leave empty intervals (the decoder reports them)
    starts = np.full(n_int + 1, end - start, np.int32)
    starts[0] = 0
    k = min(n_int - 1, rst.size)
    starts[1:1 + k] = rst[:k] + 2 - start
    if rst.size > n_int - 1:
        starts[n_int] = rst[n_int - 1] + 2 - start      # more markers than intervals: the last interval ends at the next one, with bytes left over
    plan['scan_offset'], plan['scan_length'], plan['intervals'] = start, end - start, starts
    return plan


def pack(items, out_offsets=None):
    """items: [(file bytes or uint8 array, plan)] -> (bytes uint8 [N], N % 16 == 0; plans PLAN_DTYPE [n]; intervals int32 [m]).
    Each file starts at a multiple of 16.  out_offsets: where each image's [H][W][3] result starts in the output (default: back to back)."""
    chunks, at, out_at = [], 0, 0
    plans = np.zeros(len(items), PLAN_DTYPE)
    ivs, iv_at = [], 0
    for i, (data, plan) in enumerate(items):
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
        pad = -buf.size % 16
        chunks.append(buf)
        if pad:
            chunks.append(np.zeros(pad, np.uint8))
        r = plans[i]
        for k in ('width', 'height', 'ncomp', 'hs', 'vs', 'restart_interval', 'quant', 'dc_counts', 'dc_vals', 'ac_counts', 'ac_vals'):
            r[k] = plan[k]
        r['data_off'], r['data_len'] = at + plan['scan_offset'], plan['scan_length']
        r['n_intervals'], r['interval_first'] = len(plan['intervals']) - 1, iv_at
        r['out_off'] = out_at if out_offsets is None else out_offsets[i]
        ivs.append(np.asarray(plan['intervals'], np.int32))
        iv_at += len(plan['intervals'])
        at += buf.size + pad
        out_at += plan['width'] * plan['height'] * 3
    return np.concatenate(chunks), plans, np.concatenate(ivs)
