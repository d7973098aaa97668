"""Evaluation metrics on the HIP path: FID (InceptionV3 pool features), LPIPS (AlexNet) and SSIM / MS-SSIM, scoring the PNG
directories that hoig_amd.eval_output writes.  ``python -m hoig_amd.metrics {fid,lpips,ssim} DIR1 DIR2``."""
