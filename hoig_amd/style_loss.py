"""Opt-in style (Gram-matrix) term of G on the VGG features (docs/style_loss.md): the options, the raw calls and the autograd function.

``style_loss`` launches hoig_style_gram on the current stream and returns; its backward launches hoig_style_dfeat.  Nothing is read
back and nothing is kept between steps, so the term sits in a captured step as it sits in an eager one.  On CPU tensors the same calls
run the twins (hoig_amd/_twin.py)."""
import math
import os

import torch
from torch.autograd import Function

from . import _lib as L
from . import _twin

TILE, CHUNK = L.STYLE_TILE, L.STYLE_CHUNK
DEFAULT_LEVELS = (2, 3, 4, 5)          # relu{k}_1 of VGGLoss, 1-based; GFLA's four deeper taps (level 1 is the largest map)


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


def _items(raw):
    if isinstance(raw, str):
        return [s.strip() for s in raw.split(',')]
    if isinstance(raw, (list, tuple)):
        return list(raw)
    return [raw]


def parse_options(opt, environ=None):
    """dict(weight, levels, level_weights) from ``opt.lambda_style`` / HOIG_LAMBDA_STYLE (a finite weight >= 0; 0, '' or unset: off),
    ``opt.style_levels`` (a comma list out of 1 .. 5, '2,3,4,5') and ``opt.style_level_weights`` (a comma list of as many finite
    weights >= 0, all 1).  An option of `opt` wins over the environment.  Anything else is a ValueError with the offending value --
    raised where the model is built, not in the middle of a step."""
    environ = os.environ if environ is None else environ
    weight = _weight(_pick(opt, environ, 'lambda_style', 'HOIG_LAMBDA_STYLE', 0.0), 'lambda_style')
    raw = _pick(opt, environ, 'style_levels', None, None)
    levels = []
    for item in (DEFAULT_LEVELS if raw is None else _items(raw)):
        try:
            if isinstance(item, bool) or (isinstance(item, float) and item != int(item)):
                raise ValueError
            k = int(item)
        except (TypeError, ValueError):
            raise ValueError('style_levels %r: %r is not an integer' % (raw, item))
        if not 1 <= k <= 5 or k in levels:
            raise ValueError('style_levels %r: %r must be one of 1 .. 5, each at most once' % (raw, item))
        levels.append(k)
    if not levels:
        raise ValueError('style_levels %r names no level' % (raw,))
    raw = _pick(opt, environ, 'style_level_weights', None, None)
    ws = [1.0] * len(levels) if raw is None else [_weight(item, 'style_level_weights %r: weight' % (raw,)) for item in _items(raw)]
    if len(ws) != len(levels):
        raise ValueError('style_level_weights %r: %d weights for %d levels' % (raw, len(ws), len(levels)))
    return dict(weight=weight, levels=tuple(levels), level_weights=tuple(ws))


def active(options):
    """Does anything of this module run?  (False: VGGLoss's five L1 launches alone.)"""
    return options['weight'] > 0.0


def _chk(t, what):
    if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
        raise TypeError('style loss: %s must be a contiguous float32 [N,H,W,C] tensor, got %s %s' % (what, t.dtype, tuple(t.shape)))


def gram(fx, fy, scale, term=None, report=None, out_gram=None):
    """hoig_style_gram (or its twin, on CPU tensors): the raw call.  fx, fy: contiguous fp32 [N,H,W,C]; `term`, `report`: one-element fp32
    tensors that are added to, or None; `out_gram`: float64 [2N,C,C] or None.  Returns S, fp32 [N,C,C]."""
    _chk(fx, 'fx'), _chk(fy, 'fy')
    if fy.shape != fx.shape:
        raise ValueError('style loss: fx %s, fy %s' % (tuple(fx.shape), tuple(fy.shape)))
    N, H, W, C = fx.shape
    for t in (fy, term, report, out_gram):
        if t is not None and t.device != fx.device:
            raise ValueError('style loss: tensors on %s and %s' % (fx.device, t.device))
    if out_gram is not None and (out_gram.dtype != torch.float64 or tuple(out_gram.shape) != (2 * N, C, C) or not out_gram.is_contiguous()):
        raise ValueError('style loss: out_gram must be float64 [%d, %d, %d]' % (2 * N, C, C))
    S = torch.empty((N, C, C), dtype=torch.float32, device=fx.device)
    args = (_twin.ptr(fx), _twin.ptr(fy), N, H * W, C, float(scale), _twin.ptr(S), _twin.ptr(term), _twin.ptr(report), _twin.ptr(out_gram))
    ws = L.lib.hoig_style_workspace_bytes(N, H * W, C) if fx.is_cuda else None
    _twin.run('hoig_style_gram', fx, args, workspace_bytes=ws)
    return S


def dfeat(fx, S):
    """hoig_style_dfeat (or its twin): fx [N,H,W,C] times S [N,C,C] per image, a new tensor shaped like fx."""
    _chk(fx, 'fx')
    N, H, W, C = fx.shape
    if S.dtype != torch.float32 or tuple(S.shape) != (N, C, C) or not S.is_contiguous() or S.device != fx.device:
        raise ValueError('style loss: S must be a contiguous float32 [%d, %d, %d] tensor on %s' % (N, C, C, fx.device))
    out = torch.empty_like(fx)
    _twin.run('hoig_style_dfeat', fx, (_twin.ptr(fx), _twin.ptr(S), N, H * W, C, _twin.ptr(out)))
    return out


def _slot(into):
    """LossSlots.term(name) -> (a view of the slot, for its address; the 0-dim view that is returned)"""
    slots, k = into
    return slots.buf[k:k + 1], slots.buf[k]


class _StyleLoss(Function):
    """scale * L of one level as a term of a LossSlots (`into`): the backward's gradient is pre-scaled and returned as it is -- like
    _MeanLoss with `into=`, the term is meant to be differentiated through LossSlots.total(), whose backward hands it the constant 1."""

    @staticmethod
    def forward(ctx, fx, fy, scale, into, into_raw):
        x = fx.contiguous()
        term, out = _slot(into)
        report = None if into_raw is None else _slot(into_raw)[0]
        S = gram(x, fy.detach().contiguous(), scale, term=term, report=report)
        ctx.need = ctx.needs_input_grad[0]
        if ctx.need:
            ctx.save_for_backward(x, S)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.need:
            return (None,) * 5
        x, S = ctx.saved_tensors
        return (dfeat(x, S),) + (None,) * 4


def style_loss(fx, fy, scale, into, into_raw=None):
    """scale * L(fx, fy) added to the slot `into` = LossSlots.term(name), and the unscaled L to the slot `into_raw` when given.  Returns
    the 0-dim view of the term's slot."""
    if not math.isfinite(float(scale)) or float(scale) < 0.0:
        raise ValueError('style loss: scale %r must be a finite weight >= 0' % (scale,))
    return _StyleLoss.apply(fx, fy, float(scale), into, into_raw)
