"""Differentiable augmentation of everything the discriminator sees (docs/d_augment.md): the options, and the class that owns the
device state -- the step index, the probability p, the adaptive controller's counters -- and the per-site records of the last draws.

``tick()``, ``draw()`` and ``adapt()`` launch hoig_daug_tick / hoig_daug_draw / hoig_daug_adapt on the current stream and return;
nothing comes back to the host there, so the launches sit in a captured step and the draws advance on every replay.  Only
``report()`` and ``state_dict()`` copy to the host.
"""
import os
import struct

import torch

from . import _lib as L
from .ops import _p, _st

FAMILIES = (('color', L.DAUG_COLOR), ('translation', L.DAUG_TRANSLATION), ('cutout', L.DAUG_CUTOUT))
SITE_G_FAKE, SITE_D_REAL, SITE_D_FAKE = 0, 1, 2
# the words of the state (hoig_amd/csrc/d_augment.h)
STEP, P, POS, NEG, TOTAL, STEPS, SEED, RANK, TARGET, INTERVAL, INCREMENT, POLICY, RT, ADJUSTS = range(14)
_DOUBLES = (P, TARGET, INCREMENT, RT)


def _pick(opt, environ, name, env, default=None):
    v = getattr(opt, name, None)
    if v is None and env is not None:
        v = environ.get(env, None)
    return default if v is None or v == '' else v


def parse_policy(raw):
    """'color,cutout' -> the policy word; '', None, False, 'off' -> 0; an unknown word: ValueError."""
    if raw is None or raw is False:
        return 0
    words = [w.strip().lower() for w in (raw.split(',') if isinstance(raw, str) else list(raw))]
    words = [w for w in words if w]
    if not words or words == ['off']:
        return 0
    known = dict(FAMILIES)
    mask = 0
    for w in words:
        if w not in known:
            raise ValueError("d_augment %r: unknown word %r (a comma list out of 'color', 'translation', 'cutout'; '' or 'off': off)" % (raw, w))
        mask |= known[w]
    return mask


def parse_options(opt, environ=None):
    """None with the option off, else dict(policy, p, adaptive, target, interval, kimg, seed) from ``opt.d_augment`` / HOIG_D_AUGMENT,
    ``opt.d_augment_p`` / HOIG_D_AUGMENT_P (a float in [0, 1], default 1.0, or 'adaptive'), ``opt.d_augment_target`` (0.6),
    ``opt.d_augment_interval`` (4), ``opt.d_augment_kimg`` (500) and ``opt.d_augment_seed`` (0).  Anything else is a ValueError --
    raised where the model is built, not in the middle of a step."""
    environ = os.environ if environ is None else environ
    policy = parse_policy(_pick(opt, environ, 'd_augment', 'HOIG_D_AUGMENT'))
    if not policy:
        return None
    raw = _pick(opt, environ, 'd_augment_p', 'HOIG_D_AUGMENT_P', 1.0)
    adaptive = isinstance(raw, str) and raw.strip().lower() == 'adaptive'
    p = 0.0
    if not adaptive:
        try:
            p = float(raw)
        except (TypeError, ValueError):
            raise ValueError("d_augment_p %r is not a number (a float in [0, 1], or 'adaptive')" % (raw,))
        if isinstance(raw, bool) or not 0.0 <= p <= 1.0:
            raise ValueError("d_augment_p %r must lie in [0, 1] (or be 'adaptive')" % (raw,))
    target = float(_pick(opt, environ, 'd_augment_target', None, 0.6))
    interval = int(_pick(opt, environ, 'd_augment_interval', None, 4))
    kimg = float(_pick(opt, environ, 'd_augment_kimg', None, 500))
    seed = int(_pick(opt, environ, 'd_augment_seed', None, 0))
    if adaptive and (not -1.0 <= target <= 1.0 or interval < 1 or not kimg > 0.0):
        raise ValueError('d_augment: adaptive p needs d_augment_target in [-1, 1], d_augment_interval >= 1 and d_augment_kimg > 0')
    if not 0 <= seed < 2 ** 64:
        raise ValueError('d_augment_seed %r must lie in [0, 2^64)' % (seed,))
    return dict(policy=policy, p=p, adaptive=adaptive, target=target, interval=interval, kimg=kimg, seed=seed)


def _f2w(x):
    """the bits of a double as a signed 64-bit integer (the state is an int64 tensor)"""
    return struct.unpack('<q', struct.pack('<d', float(x)))[0]


def _w2f(w):
    return struct.unpack('<d', struct.pack('<q', int(w)))[0]


def _signed(u):
    return u - 2 ** 64 if u >= 2 ** 63 else u


class DAugment(object):
    """The device state of the augmentation and one record buffer per site and batch size.  ``batch`` (samples per step, for the
    adaptive increment batch * interval / (kimg * 1000)) may be given later through ``set_batch``."""

    def __init__(self, device, policy, p=1.0, adaptive=False, target=0.6, interval=4, kimg=500.0, seed=0, rank=0, batch=None):
        if not 0 < int(policy) < 8:
            raise ValueError('DAugment: policy %r is not a set of families' % (policy,))
        self.device = torch.device(device)
        self.policy, self.adaptive = int(policy), bool(adaptive)
        self.p0 = 0.0 if self.adaptive else float(p)
        self.target, self.interval, self.kimg = float(target), int(interval), float(kimg)
        self.seed, self.rank = int(seed), int(rank)
        self.batch = None
        self.state = torch.zeros(L.DAUG_STATE_WORDS, dtype=torch.int64, device=self.device)
        self._params = {}                # (site, B) -> int32 [B, 8]: the records of the site's last draw
        self.reset()
        if batch is not None:
            self.set_batch(batch)

    def names(self):
        return [n for n, bit in FAMILIES if self.policy & bit]

    def _words(self, step=0, p=None, pos=0, neg=0, total=0, steps=0, rt=0.0, adjusts=0):
        w = [0] * L.DAUG_STATE_WORDS
        w[STEP], w[P], w[POS], w[NEG], w[TOTAL], w[STEPS] = _signed(int(step)), _f2w(self.p0 if p is None else p), pos, neg, total, steps
        w[SEED], w[RANK], w[TARGET], w[INTERVAL], w[POLICY] = _signed(self.seed), self.rank, _f2w(self.target), self.interval, self.policy
        w[INCREMENT] = _f2w(self._increment())
        w[RT], w[ADJUSTS] = _f2w(rt), adjusts
        return w

    def _increment(self):
        return 0.0 if self.batch is None else self.batch * self.interval / (self.kimg * 1000.0)

    def reset(self):
        """Step 0, the option's p, empty counters."""
        self.state.copy_(torch.tensor(self._words(), dtype=torch.int64))

    def set_batch(self, batch):
        """The samples of a step, once known: fixes the adaptive increment (not while a step is being captured)."""
        from . import ops
        if ops.capturing():
            raise RuntimeError('DAugment.set_batch() while a hipGraph is being captured')
        self.batch = int(batch)
        self.state[INCREMENT:INCREMENT + 1].copy_(torch.tensor([_f2w(self._increment())], dtype=torch.int64))

    def tick(self):
        L.call('hoig_daug_tick', _p(self.state), _st())

    def params(self, site, B):
        buf = self._params.get((site, B))
        if buf is None:
            buf = self._params[(site, B)] = torch.zeros((B, 8), dtype=torch.int32, device=self.device)
        return buf

    def draw(self, site, B, H, W):
        """The records of `site` for B samples of H x W, drawn at the state's step index: int32 [B, 8], the site's own buffer."""
        buf = self.params(site, B)
        L.call('hoig_daug_draw', _p(self.state), site, B, H, W, _p(buf), _st())
        return buf

    def adapt(self, d_real):
        """D's outputs on the (augmented) real batch join the interval's sign counts; every `interval` calls p moves."""
        assert d_real.is_contiguous() and d_real.dtype == torch.float32
        L.call('hoig_daug_adapt', _p(self.state), _p(d_real), d_real.numel(), _st())

    def state_dict(self):
        """The words a run continues from (copies to the host: synchronises)."""
        w = self.state.cpu().tolist()
        return dict(step=w[STEP] % 2 ** 64, p=_w2f(w[P]), pos=w[POS], neg=w[NEG], total=w[TOTAL], steps=w[STEPS], rt=_w2f(w[RT]),
                    adjusts=w[ADJUSTS], policy=self.names(), adaptive=self.adaptive, seed=self.seed)

    def load_state_dict(self, sd):
        self.state.copy_(torch.tensor(self._words(step=sd['step'], p=sd['p'], pos=sd.get('pos', 0), neg=sd.get('neg', 0),
                                                  total=sd.get('total', 0), steps=sd.get('steps', 0), rt=sd.get('rt', 0.0),
                                                  adjusts=sd.get('adjusts', 0)), dtype=torch.int64))

    def report(self):
        """{'p', 'rt', 'step'} (a logging tick: copies to the host)."""
        sd = self.state_dict()
        return dict(p=sd['p'], rt=sd['rt'], step=sd['step'])
