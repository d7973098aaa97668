"""Opt-in GAN objectives (hinge, logistic) and the LeCam regulariser (docs/gan_objectives.md): the options, the class that owns the
device state of the LeCam anchors, and the two loss heads as autograd functions.

``gan_d_loss`` / ``gan_g_loss`` launch hoig_gan_d_loss / hoig_gan_g_loss on the current stream and return; the anchors are read and
ticked on the device, so the calls sit in a captured step and the regulariser switches itself on during a replay.  Only
``LeCam.report()`` and ``LeCam.state_dict()`` copy to the host.  On CPU tensors the same calls run the twins (hoig_amd/_twin.py).
"""
import os
import struct

import torch
from torch.autograd import Function

from . import _lib as L
from . import _twin

MODES = (('lsgan', L.GAN_LSGAN), ('hinge', L.GAN_HINGE), ('logistic', L.GAN_LOGISTIC))
FORMS = (('paper', L.LECAM_PAPER), ('relu', L.LECAM_RELU))
# the words of the state (hoig_amd/csrc/gan_loss.h)
COUNT, ALPHA_R, ALPHA_F, GAMMA, START, BAD, LAST_R, LAST_F = range(8)


def _pick(opt, environ, name, env, default=None):
    v = getattr(opt, name, None)
    if v is None and env is not None:
        v = environ.get(env, None)
    return default if v is None or v == '' else v


def _number(raw, name, kind):
    if isinstance(raw, bool):
        raise ValueError('%s %r is not a number' % (name, raw))
    try:
        if kind is int and isinstance(raw, float) and raw != int(raw):
            raise ValueError
        return kind(raw)
    except (TypeError, ValueError):
        raise ValueError('%s %r is not %s' % (name, raw, 'an integer' if kind is int else 'a number'))


def parse_options(opt, environ=None):
    """dict(mode, lecam, decay, start, form) from ``opt.gan_mode`` / HOIG_GAN_MODE ('lsgan' (default) | 'hinge' | 'logistic'),
    ``opt.lecam`` / HOIG_LECAM (the regulariser's weight >= 0; 0 or unset: off), ``opt.lecam_decay`` (in (0, 1), 0.99),
    ``opt.lecam_start`` (an integer >= 1, 1000) and ``opt.lecam_form`` ('paper' (default) | 'relu'): ``mode`` and ``form`` are the
    library's constants.  Anything else is a ValueError -- raised where the model is built, not in the middle of a step."""
    environ = os.environ if environ is None else environ
    raw = _pick(opt, environ, 'gan_mode', 'HOIG_GAN_MODE', 'lsgan')
    mode = dict(MODES).get(raw.strip().lower() if isinstance(raw, str) else None)
    if mode is None:
        raise ValueError("gan_mode %r ('lsgan' | 'hinge' | 'logistic')" % (raw,))
    raw = _pick(opt, environ, 'lecam', 'HOIG_LECAM', 0.0)
    lecam = _number(raw, 'lecam', float)
    if not 0.0 <= lecam < float('inf'):
        raise ValueError('lecam %r must be a finite weight >= 0 (0: off)' % (raw,))
    raw = _pick(opt, environ, 'lecam_decay', None, 0.99)
    decay = _number(raw, 'lecam_decay', float)
    if not 0.0 < decay < 1.0:
        raise ValueError('lecam_decay %r must lie in (0, 1)' % (raw,))
    raw = _pick(opt, environ, 'lecam_start', None, 1000)
    start = _number(raw, 'lecam_start', int)
    if not 1 <= start < 2 ** 62:
        raise ValueError('lecam_start %r must be an integer >= 1' % (raw,))
    raw = _pick(opt, environ, 'lecam_form', None, 'paper')
    form = dict(FORMS).get(raw.strip().lower() if isinstance(raw, str) else None)
    if form is None:
        raise ValueError("lecam_form %r ('paper' | 'relu')" % (raw,))
    return dict(mode=mode, lecam=lecam, decay=decay, start=start, form=form)


def active(options):
    """Does anything of this module run?  (False: the trainer's least-squares path, launch for launch.)"""
    return options['mode'] != L.GAN_LSGAN or options['lecam'] > 0.0


def _f2w(x):
    """the bits of a double as a signed 64-bit integer (the state is an int64 tensor)"""
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


def _w2f(w):
    return struct.unpack('<d', struct.pack('<q', int(w)))[0]


class LeCam(object):
    """The device state of the LeCam regulariser: the tick count, the two anchors, the decay and the start, the count of refused
    ticks and the last two means."""

    def __init__(self, device, weight, decay=0.99, start=1000, form=L.LECAM_PAPER):
        if not weight > 0.0 or not 0.0 < decay < 1.0 or int(start) < 1 or form not in (L.LECAM_PAPER, L.LECAM_RELU):
            raise ValueError('LeCam: weight %r > 0, decay %r in (0, 1), start %r >= 1, form %r' % (weight, decay, start, form))
        self.device = torch.device(device)
        self.weight, self.decay, self.start, self.form = float(weight), float(decay), int(start), int(form)
        self.state = torch.zeros(L.LECAM_STATE_WORDS, dtype=torch.int64, device=self.device)
        self.reset()

    def _words(self, count=0, alpha_real=0.0, alpha_fake=0.0, bad=0, last_real=0.0, last_fake=0.0):
        w = [0] * L.LECAM_STATE_WORDS
        w[COUNT], w[ALPHA_R], w[ALPHA_F], w[GAMMA], w[START] = int(count), _f2w(alpha_real), _f2w(alpha_fake), _f2w(self.decay), self.start
        w[BAD], w[LAST_R], w[LAST_F] = int(bad), _f2w(last_real), _f2w(last_fake)
        return w

    def reset(self):
        """No tick taken, anchors 0."""
        self.state.copy_(torch.tensor(self._words(), dtype=torch.int64))

    def state_dict(self):
        """The words a run continues from (copies to the host: synchronises)."""
        w = self.state.cpu().tolist()
        return dict(count=w[COUNT], alpha_real=_w2f(w[ALPHA_R]), alpha_fake=_w2f(w[ALPHA_F]), bad=w[BAD], last_real=_w2f(w[LAST_R]),
                    last_fake=_w2f(w[LAST_F]), decay=self.decay, start=self.start, form=dict((v, k) for k, v in FORMS)[self.form])

    def load_state_dict(self, sd):
        """The count, the anchors, the refusal counter and the last means of `sd`; the decay, the start and the form stay the options'."""
        self.state.copy_(torch.tensor(self._words(count=sd['count'], alpha_real=sd['alpha_real'], alpha_fake=sd['alpha_fake'],
                                                  bad=sd.get('bad', 0), last_real=sd.get('last_real', 0.0),
                                                  last_fake=sd.get('last_fake', 0.0)), dtype=torch.int64))

    def report(self):
        """{'real', 'fake', 'count', 'bad'}: the anchors and the counters (a logging tick: copies to the host)."""
        sd = self.state_dict()
        return dict(real=sd['alpha_real'], fake=sd['alpha_fake'], count=sd['count'], bad=sd['bad'])


def _slot(into):
    """LossSlots.term(name) -> (a one-element view of the slot, for its address and its device; the 0-dim view that is returned)"""
    slots, k = into
    return slots.buf[k:k + 1], slots.buf[k]


def _check(t, ref=None):
    if t.dtype != torch.float32:
        raise TypeError('gan loss: the logits must be float32')
    if ref is not None and t.device != ref.device:
        raise ValueError('gan loss: tensors on %s and %s' % (t.device, ref.device))


def d_head(mode, a, b, scale, lecam=None, da=None, db=None, term=None, mean_a=None, mean_b=None, reg=None):
    """hoig_gan_d_loss (or its twin, on CPU tensors) on contiguous fp32 tensors: the raw call.  `lecam`: a LeCam or None; `da`, `db`:
    tensors the gradients are written to, or None; `term`, `mean_a`, `mean_b`, `reg`: one-element fp32 tensors that are added to."""
    _check(a); _check(b, a)
    assert a.is_contiguous() and b.is_contiguous() and a.numel() > 0 and b.numel() > 0
    state = None if lecam is None else lecam.state
    args = (int(mode), _twin.ptr(a), a.numel(), _twin.ptr(b), b.numel(), float(scale), 0.0 if lecam is None else lecam.weight,
            L.LECAM_PAPER if lecam is None else lecam.form, _twin.ptr(state), _twin.ptr(da), _twin.ptr(db), _twin.ptr(term),
            _twin.ptr(mean_a), _twin.ptr(mean_b), _twin.ptr(reg))
    ws = L.lib.hoig_gan_d_loss_workspace_bytes(a.numel(), b.numel()) if a.is_cuda else None
    _twin.run('hoig_gan_d_loss', a, args, workspace_bytes=ws)


def g_head(mode, b, scale, db=None, term=None):
    """hoig_gan_g_loss (or its twin): the raw call."""
    _check(b)
    assert b.is_contiguous() and b.numel() > 0
    args = (int(mode), _twin.ptr(b), b.numel(), float(scale), _twin.ptr(db), _twin.ptr(term))
    ws = L.lib.hoig_gan_g_loss_workspace_bytes(b.numel()) if b.is_cuda else None
    _twin.run('hoig_gan_g_loss', b, args, workspace_bytes=ws)


class _GanD(Function):
    """The D objective of `mode` on (d_real, d_fake), LeCam included, as a term of a LossSlots (`into`): the kernel stores both
    gradients pre-scaled, and they are returned as they are -- like _MeanLoss with `into=`, the term is meant to be differentiated
    through LossSlots.total(), whose backward hands it the constant 1."""

    @staticmethod
    def forward(ctx, d_real, d_fake, mode, scale, lecam, into, into_real, into_fake, into_reg):
        a, b = d_real.contiguous(), d_fake.contiguous()
        da = torch.empty_like(a) if d_real.requires_grad else None
        db = torch.empty_like(b) if d_fake.requires_grad else None
        ctx.save_for_backward(da, db)
        term, out = _slot(into)
        d_head(mode, a, b, scale, lecam, da, db, term, *[None if s is None else _slot(s)[0] for s in (into_real, into_fake, into_reg)])
        return out

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return (da, db) + (None,) * 7


class _GanG(Function):
    """The generator's adversarial term of `mode` on D(fake), as a term of a LossSlots."""

    @staticmethod
    def forward(ctx, d_fake, mode, scale, into):
        b = d_fake.contiguous()
        db = torch.empty_like(b) if d_fake.requires_grad else None
        ctx.save_for_backward(db)
        term, out = _slot(into)
        g_head(mode, b, scale, db, term)
        return out

    @staticmethod
    def backward(ctx, g):
        db, = ctx.saved_tensors
        return db, None, None, None


def gan_d_loss(d_real, d_fake, mode, scale, into, lecam=None, into_real=None, into_fake=None, into_reg=None):
    """scale * (mean f_real(d_real) + mean f_fake(d_fake)) + lecam.weight * w * R, added to the slot `into` = LossSlots.term(name);
    mean(d_real), mean(d_fake) and w * R are added to the report slots `into_real`, `into_fake`, `into_reg` when given, and `lecam`
    takes its tick.  Returns the 0-dim view of the term's slot."""
    return _GanD.apply(d_real, d_fake, mode, scale, lecam, into, into_real, into_fake, into_reg)


def gan_g_loss(d_fake, mode, scale, into):
    """scale * mean g(d_fake), the generator's term of `mode`, added to the slot `into`."""
    return _GanG.apply(d_fake, mode, scale, into)
