"""The augment-and-concatenate operator in front of the discriminator (docs/d_augment.md; re-exported by hoig_amd/ops.py)."""
import torch
from torch.autograd import Function

from . import _lib as L
from .ops import _chk, _p, _st


def _daug_ws(x):
    return torch.empty(x.shape[0] * L.DAUG_MAX_PARTS, dtype=torch.float32, device=x.device)


def _daug_check(img, cond, params):
    _chk(img); _chk(cond)
    assert img.dim() == 4 and img.shape[-1] == 3 and cond.shape[:-1] == img.shape[:-1] and img.is_contiguous() and cond.is_contiguous()
    assert params.dtype == torch.int32 and tuple(params.shape) == (img.shape[0], 8) and params.is_contiguous() and params.is_cuda


def _daug_fwd(img, cond, params, out):
    b, h, w, _ = img.shape
    L.call('hoig_daug_fwd', _p(img), _p(cond), _p(params), _p(out), b, h, w, cond.shape[-1], _p(_daug_ws(img)), _st())
    return out


class _AugmentCat(Function):
    """[img | cond] along the channels under the records `params` (hoig_daug_draw); the gradient reaches `img` only."""

    @staticmethod
    def forward(ctx, img, cond, params):
        _daug_check(img, cond, params)
        out = torch.empty(img.shape[:-1] + (3 + cond.shape[-1],), dtype=img.dtype, device=img.device)
        _daug_fwd(img, cond, params, out)
        # the records of the forward: the buffer is the site's own and is drawn again next step, after this backward
        ctx.save_for_backward(params)
        ctx.k = cond.shape[-1]
        return out

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        params, = ctx.saved_tensors
        dy = dy.contiguous()
        b, h, w, _ = dy.shape
        dimg = torch.empty((b, h, w, 3), dtype=dy.dtype, device=dy.device)
        L.call('hoig_daug_bwd', _p(dy), _p(params), _p(dimg), b, h, w, ctx.k, _p(_daug_ws(dy)), _st())
        return dimg, None, None


def augment_cat(img, cond, params, out=None):
    """The augmented concatenation [B,H,W,3+k] of img [B,H,W,3] and cond [B,H,W,k] (NHWC fp32) under params [B,8] (int32 records).
    `out`: a contiguous [B,H,W,3+k] tensor to write into -- one half of the discriminator's stacked input, say; no gradient flows
    through that form."""
    if out is None:
        return _AugmentCat.apply(img, cond, params)
    if torch.is_grad_enabled() and (img.requires_grad or cond.requires_grad):
        raise RuntimeError('augment_cat(out=...) records no gradient: detach the inputs, or let it allocate its output')
    _daug_check(img, cond, params)
    _chk(out)
    assert out.is_contiguous() and tuple(out.shape) == tuple(img.shape[:-1]) + (3 + cond.shape[-1],)
    return _daug_fwd(img, cond, params, out)
