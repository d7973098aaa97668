"""python -m hoig_amd.metrics {fid,lpips,ssim} PATH1 PATH2: what metrics/pytorch_fid, metrics/lpips.py and metrics/ssim.py print."""
import argparse
import os
import sys

DIMS = (64, 192, 768, 2048)


def parser():
    p = argparse.ArgumentParser(prog='python -m hoig_amd.metrics', description=__doc__)
    p.add_argument('metric', choices=('fid', 'lpips', 'ssim'))
    p.add_argument('path', nargs=2, help='two image directories (fid: or .npz statistics)')
    p.add_argument('--batch-size', type=int, default=None, help='fid / lpips: 50, ssim: 1 (the reference defaults)')
    p.add_argument('--dims', type=int, default=2048, choices=DIMS, help='fid: Inception feature dimensionality')
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
    return p


def main(argv=None):
    a = parser().parse_args(argv)
    if a.batch_size is not None and a.batch_size < 1:
        raise ValueError('--batch-size must be >= 1')
    for p in a.path:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
    if a.metric == 'fid':
        from .fid import calculate_fid_given_paths
        v = calculate_fid_given_paths(a.path, a.batch_size or 50, a.device, a.dims, a.inception_weights, a.precision,
                                      device_png_decode=a.device_png_decode, device_stats=a.device_fid)
        print('FID: ', v)
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
