"""The exponential moving average of a network's weights (docs/ema.md): the average, its decay schedule and its update count, all in
device memory.

``update()`` launches hoig_ema_tick and hoig_ema_update on the current stream and returns; nothing comes back to the host there, so
the launches sit behind the optimiser's in a captured step, and under a gradient guard they obey the decision the optimiser obeyed.
``swapped()`` exchanges the average and the weights in place for an eval forward.  Only ``updates()`` copies to the host.
"""
import contextlib
import os

import torch

from . import _lib as L
from .ops import _p, _st


def _flag(v):
    if isinstance(v, str):
        return v.strip().lower() not in ('', '0', 'false', 'no', 'off')
    return bool(v)


def parse_options(opt, is_train, environ=None):
    """(ema_decay or None, ema_warmup, eval_ema) from ``opt.ema_decay`` / HOIG_EMA_DECAY, ``opt.ema_warmup`` and ``opt.eval_ema`` /
    HOIG_EVAL_EMA.  0, None or unset: no average.  Anything else outside (0, 1), and eval_ema on a training model without a decay,
    is a ValueError -- raised where the model is built, not in the middle of a step."""
    environ = os.environ if environ is None else environ
    raw = getattr(opt, 'ema_decay', None)
    if raw is None:
        raw = environ.get('HOIG_EMA_DECAY', None)
    decay = None
    if raw is not None and raw is not False and raw != '':
        try:
            decay = float(raw)
        except (TypeError, ValueError):
            raise ValueError('ema_decay %r is not a number (a float in (0, 1); 0 or unset: off)' % (raw,))
        if decay == 0.0:
            decay = None
        elif not 0.0 < decay < 1.0:
            raise ValueError('ema_decay %r must lie in (0, 1) (0 or unset: off)' % (raw,))
    warmup = _flag(getattr(opt, 'ema_warmup', True))
    ev = getattr(opt, 'eval_ema', None)
    eval_ema = _flag(environ.get('HOIG_EVAL_EMA', '') if ev is None else ev)
    if eval_ema and is_train and decay is None:
        raise ValueError('eval_ema needs ema_decay on a training model (an eval-only model loads the saved average instead)')
    return decay, warmup, eval_ema


class EmaWeights(object):
    """ema <- ema + (flat - ema) * (1 - beta) per ``update()``, beta = min(decay, (1 + t) / (10 + t)) after t updates with
    ``warmup`` (else decay).  The buffer has the tree's flat layout, so ``state_dict()`` is a state dict of the network."""

    def __init__(self, tree, decay, warmup=True):
        if not 0.0 < float(decay) < 1.0:
            raise ValueError('EmaWeights: decay %r must lie in (0, 1)' % (decay,))
        self.tree = tree
        self.decay = float(decay)
        self.warmup = bool(warmup)
        dev = tree.flat.device
        self.n = tree.flat.numel()
        self.ema = torch.zeros_like(tree.flat)
        self._state = torch.zeros(3, dtype=torch.float64, device=dev)       # {decay, warmup, updates}: hoig_ema_tick advances it
        self._derived = torch.zeros(1, dtype=torch.float32, device=dev)     # {1 - beta} of the current update
        self.active = False                                                 # inside swapped()
        self.reset()

    def _upload(self, updates):
        self._state.copy_(torch.tensor([self.decay, 1.0 if self.warmup else 0.0, float(updates)], dtype=torch.float64))

    def reset(self):
        """ema := the current weights, no updates behind it (construction; after weights were loaded without an average)."""
        self._no_swap('reset')
        self.tree.wait_pending()
        self.ema.copy_(self.tree.flat)
        self._upload(0)

    def _no_swap(self, what):
        if self.active:
            raise RuntimeError('EmaWeights.%s() inside swapped(): the buffers are exchanged' % what)

    def update(self, guard=None):
        """One update from the tree's current weights, on the current stream.  `guard` (hoig_amd.guard.GradGuard): a step the guard
        skipped leaves the average and its count as they are."""
        self._no_swap('update')
        gp = _p(guard.guard) if guard is not None else None
        L.call('hoig_ema_tick', _p(self._state), _p(self._derived), gp, _st())
        L.call('hoig_ema_update', _p(self.ema), _p(self.tree.flat), self.n, _p(self._derived), gp, _st())

    def updates(self):
        """The device's update count (copies to the host: synchronises)."""
        self.tree.wait_pending()                      # (the step may still be running on a side stream)
        return int(self._state[2].item())

    def state_dict(self, prefix=''):
        self._no_swap('state_dict')
        return self.tree.export_dict(self.ema, prefix)

    def load_state_dict(self, sd, updates):
        self._no_swap('load_state_dict')
        self.tree.import_dict(self.ema, sd)
        self._upload(int(updates))

    def _exchange(self):
        self.tree.wait_pending()
        L.call('hoig_swap_f32', _p(self.tree.flat), _p(self.ema), self.n, _st())
        self.tree.version += 1                        # planes, fp6 records and cached operands are re-made as after a step

    @contextlib.contextmanager
    def swapped(self):
        """Inside the scope the tree's weights ARE the average (and ``ema`` holds the weights): an eval forward, a state_dict() of
        the network.  Exchanged in place on the current stream, and exchanged back on exit, also when the body raises."""
        from . import ops
        if ops.capturing():
            raise RuntimeError('EmaWeights.swapped() while a hipGraph is being captured')
        if self.active:
            raise RuntimeError('EmaWeights.swapped() is already active (no nesting)')
        self._exchange()
        self.active = True
        try:
            yield self
        finally:
            self.active = False
            self._exchange()
