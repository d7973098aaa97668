"""python -m hoig_amd.metrics {fid,lpips,ssim} PATH1 PATH2: what metrics/pytorch_fid, metrics/lpips.py and metrics/ssim.py print;
kid, prc: the Kernel Inception Distance and precision / recall / density of PATH1 (generated) against PATH2 (real) on the same
Inception features (docs/feature_metrics.md); swd: the Laplacian-pyramid sliced Wasserstein distance of PATH1 against PATH2, which
needs no weights (docs/swd.md); regions: PSNR, MAE and the crop metrics of the hand and the object region of PATH1 (generated) against
PATH2 (ground truth) with the label maps of --labels (docs/region_metrics.md): SSIM always, LPIPS, FID and KID when their weights are
given."""
import argparse
import os
import sys

DIMS = (64, 192, 768, 2048)


def parser():
    p = argparse.ArgumentParser(prog='python -m hoig_amd.metrics', description=__doc__)
    p.add_argument('metric', choices=('fid', 'lpips', 'ssim', 'kid', 'prc', 'swd', 'regions'))
    p.add_argument('path', nargs=2, help='two image directories (fid: or .npz statistics)')
    p.add_argument('--batch-size', type=int, default=None, help='fid / lpips / kid / prc / swd: 50, ssim: 1 (the reference defaults)')
    p.add_argument('--dims', type=int, default=2048, choices=DIMS, help='fid / kid / prc: Inception feature dimensionality')
    p.add_argument('--img-size', type=int, default=256, help='lpips / ssim: first resize of get_eval_loader')
    p.add_argument('--device', default=None)
    p.add_argument('--inception-weights', default=None, help='pt_inception-2015-12-05-6726825d.pth')
    p.add_argument('--alexnet-weights', default=None, help='alexnet-owt-7be5be79.pth')
    p.add_argument('--lpips-weights', default=None, help='lpips_weights.ckpt')
    p.add_argument('--precision', default=None, help="convolution arithmetic: 'bf16x3' (default) or 'f32'")
    p.add_argument('--device-resize', action='store_true',
                   help='lpips / ssim: run the two PIL resizes of get_eval_loader on the device (the same bytes; workers only decode)')
    p.add_argument('--device-png-decode', action='store_true', default=None,
                   help='decode the PNG files the device decoder supports on the device (the same bytes; the workers only read the '
                        'files); lpips / ssim: implies --device-resize.  HOIG_DEVICE_PNG_DECODE=1 does the same')
    p.add_argument('--device-fid', action='store_true', default=None,
                   help='fid: streaming fp64 moments and the Frechet distance on the device instead of np.cov and scipy sqrtm (close '
                        'to the default value, not equal: docs/fid_device.md).  HOIG_DEVICE_FID=1 does the same')
    p.add_argument('--kid-subsets', type=int, default=100, help='kid: the number of random subsets')
    p.add_argument('--kid-subset-size', type=int, default=1000, help='kid: rows per subset (at most the smaller directory)')
    p.add_argument('--kid-seed', type=int, default=0, help='kid: seed of the subset draws')
    p.add_argument('--prc-k', type=int, default=3, help='prc: the nearest neighbour that sets a ball\'s radius (1 .. 8)')
    p.add_argument('--swd-patches', type=int, default=128, help='swd: patches per image and level')
    p.add_argument('--swd-repeats', type=int, default=4, help='swd: sets of directions')
    p.add_argument('--swd-dirs', type=int, default=128, help='swd: directions per set')
    p.add_argument('--swd-levels', type=int, default=None, help='swd: at most this many pyramid levels (default: down to 16 pixels)')
    p.add_argument('--swd-seed', type=int, default=0, help='swd: seed of the patch positions and of the directions')
    p.add_argument('--labels', default=None, help='regions: the directory of label maps (8-bit greyscale: 0 background, 1 hand, 2 object)')
    p.add_argument('--region-size', type=int, default=128, help='regions: the side of the resized crops')
    p.add_argument('--region-min-pixels', type=int, default=64, help='regions: a region with fewer pixels does not count')
    return p


def _regions(a):
    """regions: the networks whose weights were given, then one line per value."""
    from .regions import calculate_region_metrics_given_paths
    if a.labels is None or not os.path.exists(a.labels):
        raise RuntimeError('regions needs --labels DIR, got %r' % (a.labels,))
    fid = lpips = None
    if a.inception_weights is not None:
        from .fid import InceptionFeatures
        fid = InceptionFeatures(a.inception_weights, a.dims, a.precision, a.device)
    if a.alexnet_weights is not None or a.lpips_weights is not None:
        from .lpips import LPIPS
        lpips = LPIPS(a.alexnet_weights, a.lpips_weights, a.precision, a.device)
    kid = dict(subsets=a.kid_subsets, subset_size=a.kid_subset_size, seed=a.kid_seed) if fid is not None else None
    v = calculate_region_metrics_given_paths(a.path, a.labels, a.region_size, a.region_min_pixels, a.batch_size or 50, fid, lpips, True,
                                             kid, a.device, fid_device=bool(a.device_fid))
    for key, value in v.items():
        print('%s:  %r' % (key, value))
    return v


def main(argv=None):
    a = parser().parse_args(argv)
    if a.batch_size is not None and a.batch_size < 1:
        raise ValueError('--batch-size must be >= 1')
    for p in a.path:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
    if a.metric == 'regions':
        return _regions(a)
    if a.metric == 'fid':
        from .fid import calculate_fid_given_paths
        v = calculate_fid_given_paths(a.path, a.batch_size or 50, a.device, a.dims, a.inception_weights, a.precision,
                                      device_png_decode=a.device_png_decode, device_stats=a.device_fid)
        print('FID: ', v)
    elif a.metric == 'kid':
        from .feature_metrics import calculate_kid_given_paths
        v = calculate_kid_given_paths(a.path, a.batch_size or 50, a.device, a.dims, a.inception_weights, a.precision,
                                      device_png_decode=a.device_png_decode, subsets=a.kid_subsets, subset_size=a.kid_subset_size,
                                      seed=a.kid_seed)
        print('KID: ', v[0], '', v[1])                    # (mean, then the standard deviation over the subsets)
    elif a.metric == 'prc':
        from .feature_metrics import calculate_prc_given_paths
        v = calculate_prc_given_paths(a.path, a.batch_size or 50, a.device, a.dims, a.inception_weights, a.precision,
                                      device_png_decode=a.device_png_decode, k=a.prc_k)
        print('Precision: ', v['precision'], ' Recall: ', v['recall'], ' Density: ', v['density'])
    elif a.metric == 'swd':
        from .swd import calculate_swd_given_paths
        v = calculate_swd_given_paths(a.path, a.batch_size or 50, a.device, device_png_decode=a.device_png_decode,
                                      patches=a.swd_patches, repeats=a.swd_repeats, dirs=a.swd_dirs, levels=a.swd_levels, seed=a.swd_seed)
        print('SWD: ', v['swd'], '', ' '.join(repr(x) for x in v['swd_levels']))    # (the mean, then the levels, finest first)
    elif a.metric == 'lpips':
        from .lpips import calculate_lpips_given_paths
        v = calculate_lpips_given_paths(a.path, a.img_size, a.batch_size or 50, a.alexnet_weights, a.lpips_weights, a.precision,
                                        a.device, device_resize=a.device_resize, device_png_decode=a.device_png_decode)
        print('LPIPS: ', v)
    else:
        from .ssim import calculate_ssim_given_paths
        v = calculate_ssim_given_paths(a.path, a.img_size, a.batch_size or 1, a.device, device_resize=a.device_resize,
                                       device_png_decode=a.device_png_decode)
        print('SSIM: ', v[0], ' MS-SSIM: ', v[1])
    return v


if __name__ == '__main__':
    sys.exit(0 if main() is not None else 1)
