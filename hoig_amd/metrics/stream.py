"""Scoring eval output from device memory: FID, LPIPS and SSIM / MS-SSIM of a stream of generated / ground-truth uint8 batches, with
the values the path functions give on two directories that hold the same images as PNGs.

PNG is lossless and eval.py's bytes are made on the device (Trainer.eval_images_u8), so the only piece of the directory path without a
device form was get_eval_loader's resize chain, PIL's 8-bit BILINEAR twice: kernels.pil_resize_chain_u8 gives the same bytes.  The
values are then EQUAL, not close, as long as the same launches see the same bytes -- so the scorer re-groups whatever it is given into
exactly the batches the path functions form (LPIPS is the mean of per-batch means, and a kernel may pick its tiling by batch size),
keeps the remainder as uint8 and runs it as the short last batch when result() is asked.

Every network is one the caller built (weights.py: without weights nothing runs).
"""
import numpy as np
import torch

from . import kernels as K
from .fid import calculate_frechet_distance, compute_statistics_of_path
from .feature_metrics import FeatureBank, _options, kid_from_features, precision_recall_from_features
from .fid_device import Moments, fid_device_option, frechet_distance_device
from .regions import RegionScores, region_options
from .ssim import ssim_pairs_u8
from .swd import banks_for, swd_from_banks, swd_options


class _Batches(object):
    """Consecutive batches of exactly `size` images out of uint8 [N,H,W,3] pieces of any N; what is left over stays here."""

    def __init__(self, size):
        if size < 1:
            raise ValueError('batch size must be >= 1')
        self.size, self.rest = size, None

    def push(self, u8):
        """-> the full batches that `u8` completes, in order."""
        if self.rest is not None:
            if self.rest.shape[1:] != u8.shape[1:]:
                raise ValueError('images of one batch differ in size: %s after %s' % (tuple(u8.shape[1:]), tuple(self.rest.shape[1:])))
            u8 = torch.cat([self.rest, u8])
        full = u8.shape[0] // self.size * self.size
        self.rest = u8[full:].clone() if full < u8.shape[0] else None      # (a copy: the caller may reuse its tensor)
        return [u8[i:i + self.size] for i in range(0, full, self.size)]


class Scorer(object):
    """``s = Scorer(fid=InceptionFeatures(...), lpips=LPIPS(...), ssim=True); s.update(gen_u8, gt_u8) ...; s.result()``

    update(): device uint8 [N,H,W,3] of generated and ground-truth images, any N per call.  result(): {'n', 'fid', 'lpips', 'ssim',
    'ms_ssim'} (absent metrics omitted), equal to calculate_fid_given_paths([gen, gt], fid_batch, ..), calculate_lpips_given_paths(
    [gen, gt], img_size, lpips_batch, model=lpips) and calculate_ssim_given_paths([gen, gt], img_size, ssim_batch) on directories whose
    sorted file names are in update() order.  FID is between the two streams, or against `fid_reference`: (mu, sigma) or an .npz of
    them (then the ground truth's features are not taken).

    fid_device (HOIG_DEVICE_FID=1; off by default): the features go into streaming fp64 moments on the device (fid_device.Moments:
    update() makes no host copy and does not wait for the device) and result() takes the distance with
    fid_device.frechet_distance_device.  The values are then close to the directory functions', not equal (docs/fid_device.md).

    kid, prc (off by default; True, or a dict of the keyword arguments of feature_metrics.kid_from_features /
    precision_recall_from_features): the features of both streams are also kept on the device (feature_metrics.FeatureBank, 4 * dims
    bytes per image and stream) and result() gains 'kid', 'kid_std' and 'precision', 'recall', 'density', equal to
    calculate_kid_given_paths / calculate_prc_given_paths on the directories (docs/feature_metrics.md).  Both need the FID network and
    the ground truth's features, so neither goes with fid_reference.

    swd (off by default; True, or a dict of patches, repeats, dirs, levels, seed): the Laplacian-pyramid sliced Wasserstein distance
    between the two streams (swd.py, docs/swd.md).  It needs no network -- Scorer(fid=None, lpips=None, ssim=False, swd=True) runs
    without any weights.  update() keeps each image's patch descriptors on the device (swd.SWDBank, 4 * 147 * patches * levels bytes
    per image and stream) and result() gains 'swd' and 'swd_levels', equal to calculate_swd_given_paths on the directories whatever
    the sizes of the update() calls.

    regions (off by default; True, or a dict of size, min_pixels, batch): scores on the hand and the object region (regions.py,
    docs/region_metrics.md).  update() then takes a third argument, the ground truth's label map as device uint8 [N,H,W] (0 background,
    1 hand, 2 object: Trainer.eval_regions_u8), and result() gains 'psnr', 'mae' of the whole frame and per region r in ('hand',
    'object') 'n_<r>', 'psnr_<r>', 'mae_<r>' and -- from square crops around the region, for the metrics this scorer has --
    'lpips_<r>', 'ssim_<r>', 'fid_<r>', 'kid_<r>', 'kid_std_<r>'.  It takes no fid_reference, prc or swd per region."""

    def __init__(self, fid=None, lpips=None, ssim=True, img_size=256, fid_batch=50, lpips_batch=50, ssim_batch=50, fid_reference=None,
                 fid_device=None, kid=None, prc=None, swd=None, regions=None):
        self.fid, self.lpips, self.ssim, self.img_size = fid, lpips, bool(ssim), img_size
        self.n = 0
        if isinstance(fid_reference, str):
            if not fid_reference.endswith('.npz'):
                raise ValueError('fid_reference %r: (mu, sigma) or an .npz of them' % fid_reference)
            fid_reference = compute_statistics_of_path(fid_reference, None, None, None)
        self.fid_reference = fid_reference
        self.fid_device = False
        self.kid, self.prc = _options(kid, 'kid'), _options(prc, 'prc')
        self._bank_gen = self._bank_gt = None
        self.swd = swd_options(swd)
        self._swd_gen = self._swd_gt = None
        if self.kid is not None or self.prc is not None:
            if fid is None:
                raise ValueError('kid / prc need the FID network: Scorer(fid=InceptionFeatures(...), ...)')
            if fid_reference is not None:
                raise ValueError('kid / prc need the ground truth\'s features, which a fid_reference replaces')
            self._bank_gen, self._bank_gt = FeatureBank(fid.dims, fid.device), FeatureBank(fid.dims, fid.device)
        if fid is not None:
            self._fid_gen, self._fid_gt = _Batches(fid_batch), (_Batches(fid_batch) if fid_reference is None else None)
            self._feat_gen, self._feat_gt = [], []
            self.fid_device = fid_device_option(fid_device)
            if self.fid_device:
                self._feat_gen, self._feat_gt = Moments(fid.dims, fid.device), Moments(fid.dims, fid.device)
        # the pair metrics that share a batch size share the resized batch
        self._pairs = {}
        if lpips is not None:
            self._pairs.setdefault(lpips_batch, []).append('lpips')
        if self.ssim:
            self._pairs.setdefault(ssim_batch, []).append('ssim')
        self._pair_batches = {size: (_Batches(size), _Batches(size)) for size in self._pairs}
        self._lpips_means, self._ssim, self._ms_ssim = [], [], []
        self.regions = region_options(regions)
        self._regions = None
        if self.regions is not None:
            self._regions = RegionScores(self.regions, fid, lpips, self.ssim, self.kid, self.fid_device)

    # ---- one batch, as the path functions run it
    def _features_device(self, u8, bank=None):
        """fp32 [B, dims] on the device; with kid / prc on, a copy goes into the stream's bank."""
        f = self.fid.features_u8(u8.contiguous())
        if bank is not None:
            bank.append(f)
        return f

    def _features(self, u8, bank=None):
        return self._features_device(u8, bank).double().cpu().numpy()

    def _pair(self, metrics, gen, gt, into):
        u8 = K.pil_resize_chain_u8(torch.cat([gen, gt]), self.img_size)
        if 'lpips' in metrics:
            into[0].append(self.lpips.distance_u8(u8).mean())
        if 'ssim' in metrics:
            s, m = ssim_pairs_u8(u8)
            into[1].append(s)
            into[2].append(m)

    def update(self, gen_u8, gt_u8, regions_u8=None):
        if (regions_u8 is None) != (self._regions is None):
            raise ValueError('update(gen_u8, gt_u8, regions_u8): the label map goes with Scorer(regions=...), and only with it')
        for t in (gen_u8, gt_u8):
            if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 4 or t.shape[-1] != 3:
                raise ValueError('device uint8 [N,H,W,3] expected, got %s %s on %s' % (t.dtype, tuple(t.shape), t.device))
        if gen_u8.shape != gt_u8.shape:
            raise ValueError('generated %s and ground truth %s differ in shape' % (tuple(gen_u8.shape), tuple(gt_u8.shape)))
        if self._regions is not None:
            if regions_u8.dtype != torch.uint8 or not regions_u8.is_cuda or tuple(regions_u8.shape) != tuple(gen_u8.shape[:3]):
                raise ValueError('regions_u8: device uint8 %s expected, got %s %s on %s' % (tuple(gen_u8.shape[:3]), regions_u8.dtype,
                                                                                        tuple(regions_u8.shape), regions_u8.device))
            self._regions.update(gen_u8, gt_u8, regions_u8)
        if self.swd is not None and gen_u8.shape[0]:
            if self._swd_gen is None:
                self._swd_gen, self._swd_gt = banks_for(self.swd, gen_u8.device)
            self._swd_gen.append(gen_u8)
            self._swd_gt.append(gt_u8)
        self.n += gen_u8.shape[0]
        if self.fid is not None and self.fid_device:
            for b in self._fid_gen.push(gen_u8):
                self._feat_gen.update(self._features_device(b, self._bank_gen))
            if self._fid_gt is not None:
                for b in self._fid_gt.push(gt_u8):
                    self._feat_gt.update(self._features_device(b, self._bank_gt))
        elif self.fid is not None:
            self._feat_gen += [self._features(b, self._bank_gen) for b in self._fid_gen.push(gen_u8)]
            if self._fid_gt is not None:
                self._feat_gt += [self._features(b, self._bank_gt) for b in self._fid_gt.push(gt_u8)]
        into = (self._lpips_means, self._ssim, self._ms_ssim)
        for size, metrics in self._pairs.items():
            bg, bt = self._pair_batches[size]
            for gen, gt in zip(bg.push(gen_u8), bt.push(gt_u8)):
                self._pair(metrics, gen, gt, into)

    # ---- the totals: what was flushed plus the short last batch (the state is left as it is, so update() may go on)
    def _moments(self, moments, batches):
        """The device moments with the short last batch in: that batch goes into a COPY of the state."""
        if batches.rest is not None:
            moments = moments.copy().update(self.fid.features_u8(batches.rest.contiguous()))
        if moments.n == 0:
            raise ValueError('no images were given')
        return moments

    def _rows(self, bank, batches):
        """A stream's feature rows with the short last batch in: that batch goes into a COPY of the bank, as in _moments."""
        if batches.rest is not None:
            bank = bank.copy().append(self.fid.features_u8(batches.rest.contiguous()))
        return bank.rows()

    def _statistics(self, feats, batches):
        if self.fid_device:
            return self._moments(feats, batches).statistics_host()
        feats = list(feats)
        if batches.rest is not None:
            feats.append(self._features(batches.rest))
        if not feats:
            raise ValueError('no images were given')
        act = np.concatenate(feats)
        return np.mean(act, axis=0), np.cov(act, rowvar=False)

    def statistics(self):
        """(mu, sigma) of the generated set's Inception features (fid_score.py calculate_activation_statistics)."""
        if self.fid is None:
            raise ValueError('this scorer has no FID network')
        return self._statistics(self._feat_gen, self._fid_gen)

    def save_statistics(self, path):
        """The .npz that fid.compute_statistics_of_path reads: mu, sigma of the generated set."""
        mu, sigma = self.statistics()
        np.savez(path, mu=mu, sigma=sigma)

    def result(self):
        if self.n == 0:
            raise ValueError('no images were given')
        out = {'n': self.n}
        if self.fid is not None and self.fid_device:
            ref = self.fid_reference if self.fid_reference is not None else self._moments(self._feat_gt, self._fid_gt).statistics()
            out['fid'] = frechet_distance_device(*(self._moments(self._feat_gen, self._fid_gen).statistics() + tuple(ref)))
        elif self.fid is not None:
            ref = self.fid_reference if self.fid_reference is not None else self._statistics(self._feat_gt, self._fid_gt)
            out['fid'] = calculate_frechet_distance(*(self.statistics() + tuple(ref)))
        if self._bank_gen is not None:
            gen, gt = self._rows(self._bank_gen, self._fid_gen), self._rows(self._bank_gt, self._fid_gt)
            if self.kid is not None:
                out['kid'], out['kid_std'] = kid_from_features(gen, gt, **self.kid)
            if self.prc is not None:
                out.update(precision_recall_from_features(gt, gen, **self.prc))
        if self.swd is not None:
            value = swd_from_banks(self._swd_gen, self._swd_gt, self.swd['repeats'], self.swd['dirs'], self.swd['seed'])
            out['swd'], out['swd_levels'] = value['swd'], value['swd_levels']
        into = (list(self._lpips_means), list(self._ssim), list(self._ms_ssim))
        for size, metrics in self._pairs.items():
            bg, bt = self._pair_batches[size]
            if bg.rest is not None:
                self._pair(metrics, bg.rest, bt.rest, into)
        if self.lpips is not None:
            out['lpips'] = torch.stack(into[0]).double().mean().item()
        if self.ssim:
            out['ssim'] = torch.cat(into[1]).double().mean().item()
            out['ms_ssim'] = torch.cat(into[2]).double().mean().item()
        if self._regions is not None:
            out.update(self._regions.result())
        return out


def score_model(model, dataset, scorer, writer=None):
    """The evaluation loop without files: for every batch of `dataset` (dicts as eval.py's loader yields them) forward() under
    no_grad, the three images as device bytes, scorer.update(imitators, gt) and, with an EvalWriter, the PNGs of the same bytes.
    A scorer with regions also takes model.eval_regions_u8(), and a writer with sav_regions keeps those label maps as PNGs.
    Returns scorer.result()."""
    with_regions = getattr(scorer, 'regions', None) is not None
    for batch in dataset:
        model.set_input(batch)
        with torch.no_grad():
            outs = model.forward()
        images = model.eval_images_u8(outs)
        if with_regions:
            labels = model.eval_regions_u8()
            scorer.update(images['imitators'], images['gt'], labels)
            if writer is not None and getattr(writer, 'sav_regions', False):
                images = dict(images, regions=labels)
        else:
            scorer.update(images['imitators'], images['gt'])
        if writer is not None:
            writer.write_images(images, batch['nameA'], batch['nameB'])
    return scorer.result()
