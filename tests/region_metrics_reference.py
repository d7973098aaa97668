"""Restatements of the region scores (docs/region_metrics.md) in numpy int64, Pillow and fp64: the label rule, the statistics rows, the
box rule, the crop and the scalar formulas -- what the kernels of hoig_amd/csrc/region_metrics.hip and their CPU twins are compared
with, for equality.  tests/test_region_metrics_cpu.py pins this file to a hand-written case first."""
import numpy as np
from PIL import Image

NAMES = ('hand', 'object')


def labels_from_masks(bg_mask, hand_mask):
    """1 where hand_mask < 0.5 (that mask is 1 outside the hand), else 2 where bg_mask < 0.5, else 0."""
    bg_mask, hand_mask = np.asarray(bg_mask), np.asarray(hand_mask)
    return np.where(hand_mask < 0.5, 1, np.where(bg_mask < 0.5, 2, 0)).astype(np.uint8)


def stats(gen, gt, labels, regions=2):
    """-> (int64 [N, regions + 1, 8], status): rows [count, sum |d|, sum d^2, x0, y0, x1, y1, 0]; status 0, or 1 | largest bad label << 8."""
    gen, gt, labels = np.asarray(gen), np.asarray(gt), np.asarray(labels)
    N, H, W = labels.shape
    d = gen.astype(np.int64) - gt.astype(np.int64)
    ad, sq = np.abs(d).sum(-1), (d * d).sum(-1)
    out = np.zeros((N, regions + 1, 8), np.int64)
    for n in range(N):
        for r in range(regions + 1):
            m = np.ones((H, W), bool) if r == 0 else labels[n] == r
            ys, xs = np.nonzero(m)
            box = (xs.min(), ys.min(), xs.max(), ys.max()) if xs.size else (W, H, -1, -1)
            out[n, r] = (m.sum(), ad[n][m].sum(), sq[n][m].sum()) + box + (0,)
    bad = int(labels.max()) if labels.size and labels.max() > regions else 0
    return out, (1 | bad << 8) if bad else 0


def box(row, H, W, min_pixels):
    """[left, top, side, valid] of one statistics row, in Python integers."""
    count, x0, y0, x1, y1 = int(row[0]), int(row[3]), int(row[4]), int(row[5]), int(row[6])
    if count < max(min_pixels, 1):
        return [0, 0, 0, 0]
    side0 = max(x1 - x0 + 1, y1 - y0 + 1)
    pad = (side0 + 3) // 4
    side = min(side0 + 2 * pad, H, W)
    left = min(max((x0 + x1 + 1 - side) // 2, 0), W - side)
    top = min(max((y0 + y1 + 1 - side) // 2, 0), H - side)
    return [left, top, side, 1]


def boxes(st, H, W, min_pixels):
    """int32 [N, regions, 4] from the rows 1 .. of stats [N, regions + 1, 8]."""
    return np.array([[box(row, H, W, min_pixels) for row in img[1:]] for img in st], np.int32).reshape(st.shape[0], st.shape[1] - 1, 4)


def crop(img, bx, size):
    """Image.crop(box).resize((size, size), BILINEAR) of one HWC uint8 image; zeros for an invalid box."""
    left, top, side, valid = (int(v) for v in bx)
    if not valid:
        return np.zeros((size, size, 3), np.uint8)
    pil = Image.fromarray(np.ascontiguousarray(img)).crop((left, top, left + side, top + side)).resize((size, size), Image.BILINEAR)
    return np.asarray(pil, dtype=np.uint8)


def crops(images, bxs, size):
    """uint8 [regions, N, size, size, 3] of images [N,H,W,3] and boxes [N, regions, 4]."""
    N, R = bxs.shape[:2]
    return np.stack([np.stack([crop(images[n], bxs[n, r], size) for n in range(N)]) for r in range(R)])


def psnr_mae(row):
    """(10 log10(255^2 * 3 count / sum d^2), sum |d| / (3 count)) of one statistics row in fp64; inf for equal pixels."""
    count, ad, sq = (np.float64(v) for v in row[:3])
    with np.errstate(divide='ignore'):
        return 10.0 * np.log10(np.float64(255.0) ** 2 * 3.0 * count / sq), ad / (3.0 * count)


def scalars(gen, gt, labels, min_pixels, names=NAMES):
    """The scorer's keys that need no network: n_<r>, psnr, mae, psnr_<r>, mae_<r>."""
    st, status = stats(gen, gt, labels, len(names))
    assert status == 0
    bx = boxes(st, labels.shape[1], labels.shape[2], min_pixels)
    whole = [psnr_mae(row) for row in st[:, 0]]
    out = {'psnr': float(np.mean([p for p, _ in whole])), 'mae': float(np.mean([m for _, m in whole]))}
    for r, name in enumerate(names):
        rows = [psnr_mae(st[n, r + 1]) for n in range(st.shape[0]) if bx[n, r, 3]]
        out['n_' + name] = len(rows)
        out['psnr_' + name] = float(np.mean([p for p, _ in rows]))
        out['mae_' + name] = float(np.mean([m for _, m in rows]))
    return out


# ------------------------------------------------------------------------------------------------ the cases of the tests
STATS_SHAPES = [(1, 1), (5, 7), (33, 65), (64, 64)]          # H x W, N = 3; 3 W is no multiple of 4 in the first three


def content(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def stats_case(h, w, seed=0):
    """(gen, gt, labels) of 3 images: image 0 has region 1 on all four borders, region 2 empty and one pixel labelled 3; image 1 has a
    single pixel of region 2 and region 1 empty; image 2 is random labels 0 .. 2 with some pixels of gen equal to gt."""
    gen, gt = content(3, h, w, seed), content(3, h, w, seed + 1)
    gt[2, : h // 2] = gen[2, : h // 2]
    lab = np.zeros((3, h, w), np.uint8)
    lab[0, 0, :] = lab[0, -1, :] = 1
    lab[0, :, 0] = lab[0, :, -1] = 1
    lab[0, h // 2, w // 2] = 3
    lab[1, h - 1, w // 3] = 2
    lab[2] = np.random.default_rng(seed + 2).integers(0, 3, size=(h, w), dtype=np.uint8)
    return gen, gt, lab


# (H, W), size, [(left, top, side)]: every (side -> size) pair with the box in the top-left and in the bottom-right corner
CROP_CASES = [
    ((40, 52), 8, [(0, 0, 1), (51, 39, 1), (0, 0, 3), (49, 37, 3), (0, 0, 8), (44, 32, 8), (0, 0, 37), (15, 3, 37)]),
    ((45, 41), 6, [(0, 0, 40), (1, 5, 40)]),
    ((100, 120), 64, [(0, 0, 100), (20, 0, 100)]),
    ((170, 150), 128, [(0, 0, 150), (0, 20, 150)]),
]


def crop_case(case, seed=3):
    """(images [N,H,W,3], boxes [N, 1, 4]) of a CROP_CASES entry: one image per box, and a last image with an invalid box."""
    (h, w), size, windows = case
    n = len(windows) + 1
    images = content(n, h, w, seed + h)
    bxs = np.zeros((n, 1, 4), np.int32)
    for i, (left, top, side) in enumerate(windows):
        bxs[i, 0] = (left, top, side, 1)
    return images, bxs
