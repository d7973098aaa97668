"""Opt-in region reconstruction term of G (docs/region_loss.md): the options, the raw head and the autograd function.

``region_l1_loss`` launches hoig_region_loss on the current stream and returns: the pixel counts of every (image, region) row, the
rows' validity and the gradient scales are made and consumed on the device inside the call, so it sits in a captured step and follows
the masks of whichever batch is in the static buffers.  It keeps no state.  On CPU tensors the same call runs the twin
(hoig_amd/_twin.py)."""
import ctypes
import os

import torch
from torch.autograd import Function

from . import _lib as L
from . import _twin

VIEWS = ('both', 'src', 'tsf')
NAMES = ('hand', 'obj')          # the regions of the trainer's label map: 1, 2 (hoig_amd.metrics.regions.labels_from_masks)


def _pick(opt, environ, name, env, default=None):
    v = getattr(opt, name, None)
    if v is None and env is not None:
        v = environ.get(env, None)
    return default if v is None or v == '' else v


def _weight(raw, name):
    if isinstance(raw, bool):
        raise ValueError('%s %r is not a number' % (name, raw))
    try:
        v = float(raw)
    except (TypeError, ValueError):
        raise ValueError('%s %r is not a number' % (name, raw))
    if not 0.0 <= v < float('inf'):
        raise ValueError('%s %r must be a finite weight >= 0 (0: off)' % (name, raw))
    return v


def parse_options(opt, environ=None):
    """dict(hand, obj, views, min_pixels) from ``opt.lambda_rec_hand`` / HOIG_LAMBDA_REC_HAND and ``opt.lambda_rec_obj`` /
    HOIG_LAMBDA_REC_OBJ (finite weights >= 0; 0, '' or unset: off), ``opt.region_loss_views`` ('both' (default) | 'src' | 'tsf') and
    ``opt.region_loss_min_pixels`` (an integer >= 1, 64).  An option of `opt` wins over the environment.  Anything else is a
    ValueError with the offending value -- raised where the model is built, not in the middle of a step."""
    environ = os.environ if environ is None else environ
    hand = _weight(_pick(opt, environ, 'lambda_rec_hand', 'HOIG_LAMBDA_REC_HAND', 0.0), 'lambda_rec_hand')
    obj = _weight(_pick(opt, environ, 'lambda_rec_obj', 'HOIG_LAMBDA_REC_OBJ', 0.0), 'lambda_rec_obj')
    raw = _pick(opt, environ, 'region_loss_views', None, 'both')
    views = raw.strip().lower() if isinstance(raw, str) else None
    if views not in VIEWS:
        raise ValueError("region_loss_views %r ('both' | 'src' | 'tsf')" % (raw,))
    raw = _pick(opt, environ, 'region_loss_min_pixels', None, 64)
    try:
        if isinstance(raw, bool) or (isinstance(raw, float) and raw != int(raw)):
            raise ValueError
        min_pixels = int(raw)
    except (TypeError, ValueError):
        raise ValueError('region_loss_min_pixels %r is not an integer' % (raw,))
    if not 1 <= min_pixels < 2 ** 31:
        raise ValueError('region_loss_min_pixels %r must be an integer >= 1' % (raw,))
    return dict(hand=hand, obj=obj, views=views, min_pixels=min_pixels)


def active(options):
    """Does anything of this module run?  (False: the trainer's whole-frame ops.l1_loss, launch for launch.)"""
    return options['hand'] > 0.0 or options['obj'] > 0.0


def head(pred, target, labels, lambdas, lambda_all, min_pixels, term, dpred=None, terms_r=None, term_all=None, counts=None, status=None):
    """hoig_region_loss (or its twin, on CPU tensors) on contiguous tensors: the raw call.  pred, target: fp32 [N,H,W,C]; labels: uint8
    [N,H,W]; lambdas: R + 1 weights, the background's first; `dpred`: a tensor the gradient is written to, or None; `term`, `term_all`
    (one element) and `terms_r` (R + 1 elements): fp32 tensors that are added to; `counts`: int32 [N, R + 1] or None; `status`: int32
    [1], made here when None.  Returns `status`."""
    if pred.dtype != torch.float32 or target.dtype != torch.float32 or labels.dtype != torch.uint8:
        raise TypeError('region loss: float32 images and uint8 labels expected, got %s, %s, %s' % (pred.dtype, target.dtype, labels.dtype))
    if pred.dim() != 4 or target.shape != pred.shape or tuple(labels.shape) != tuple(pred.shape[:3]):
        raise ValueError('region loss: pred %s, target %s, labels %s' % (tuple(pred.shape), tuple(target.shape), tuple(labels.shape)))
    for t in (target, labels, dpred, term, terms_r, term_all, counts, status):
        if t is not None and t.device != pred.device:
            raise ValueError('region loss: tensors on %s and %s' % (pred.device, t.device))
    assert pred.is_contiguous() and target.is_contiguous() and labels.is_contiguous()
    lam = [float(v) for v in lambdas]
    R = len(lam) - 1
    if terms_r is not None and terms_r.numel() < R + 1:
        raise ValueError('region loss: %d report slots for %d regions' % (terms_r.numel(), R + 1))
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != pred.shape[0] * (R + 1) or not counts.is_contiguous()):
        raise ValueError('region loss: counts must be int32 [%d, %d]' % (pred.shape[0], R + 1))
    if status is None:
        status = torch.empty(1, dtype=torch.int32, device=pred.device)       # (the head always writes it)
    N, H, W, C = pred.shape
    lam_c = (ctypes.c_double * (R + 1))(*lam)             # (read by the entry point before it returns)
    args = (_twin.ptr(pred), _twin.ptr(target), _twin.ptr(labels), N, H, W, C, R, ctypes.cast(lam_c, ctypes.c_void_p), float(lambda_all),
            int(min_pixels), _twin.ptr(dpred), _twin.ptr(term), _twin.ptr(terms_r), _twin.ptr(term_all), _twin.ptr(counts), _twin.ptr(status))
    ws = L.lib.hoig_region_loss_workspace_bytes(N, H, W, C, R) if pred.is_cuda else None
    _twin.run('hoig_region_loss', pred, args, workspace_bytes=ws)
    return status


def _slot(into):
    """LossSlots.term(name) -> (a view of the slot, for its address; the 0-dim view that is returned)"""
    slots, k = into
    return slots.buf[k:k + 1], slots.buf[k]


class _RegionL1(Function):
    """The region terms of `pred` against `target` as a term of a LossSlots (`into`): the kernel stores the gradient pre-scaled, and it
    is returned as it is -- like _MeanLoss with `into=`, the term is meant to be differentiated through LossSlots.total(), whose
    backward hands it the constant 1."""

    @staticmethod
    def forward(ctx, pred, target, labels, lambdas, lambda_all, min_pixels, into, into_regions, into_all):
        p = pred.contiguous()
        dpred = torch.empty_like(p) if pred.requires_grad else None
        ctx.save_for_backward(dpred)
        term, out = _slot(into)
        lam = [float(v) for v in lambdas]
        terms_r = None
        if into_regions is not None:       # R + 1 report slots side by side, the background's first
            slots, k = into_regions
            if k + len(lam) > slots.buf.numel():
                raise ValueError('region loss: into_regions needs %d consecutive slots' % len(lam))
            terms_r = slots.buf[k:k + len(lam)]
        all_ = None if into_all is None else _slot(into_all)[0]
        head(p, target.detach().contiguous(), labels.contiguous(), lam, lambda_all, min_pixels, term, dpred=dpred, terms_r=terms_r,
             term_all=all_)
        return out

    @staticmethod
    def backward(ctx, g):
        dpred, = ctx.saved_tensors
        return (dpred,) + (None,) * 8


def region_l1_loss(pred, target, labels, lambdas, lambda_all, min_pixels, into, into_regions=None, into_all=None):
    """sum_r lambdas[r] L_r of (pred, target, labels), added to the slot `into` = LossSlots.term(name); lambda_all L_all, the whole-frame
    L1 term, is added to the slot `into_all` when given, and to `into` otherwise; the unweighted L_0 .. L_R are added to the R + 1
    consecutive report slots that begin at `into_regions` = LossSlots.term(the background's) when given.  Returns the 0-dim view of the term's slot."""
    return _RegionL1.apply(pred, target, labels, lambdas, lambda_all, min_pixels, into, into_regions, into_all)
