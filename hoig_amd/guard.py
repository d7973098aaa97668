"""The gradient guard of a network (docs/grad_guard.md): statistics of its flat gradient, the skip / clip decision and the
counters, all in device memory.

``observe()`` launches hoig_grad_stats and hoig_guard_decide on the current stream and returns; nothing comes back to the host
there, so the launches sit in a captured step like any other.  The guarded Adam entry points (FusedAdam.step(guard=...)) read the
decision from ``guard``.  Only ``report()`` and ``per_tensor()`` copy to the host -- call them where the run synchronises anyway.
"""
import weakref
from collections import OrderedDict

import torch

from . import _lib as L
from .ops import _p, _st

POLICIES = ('watch', 'skip')
RECORD_FIELDS = ('steps', 'skipped', 'clipped', 'norm', 'max', 'nonfinite', 'norm_peak')


class GradGuard(object):
    """policy 'watch': a non-finite gradient is counted and the update goes through as without a guard; 'skip': the update (and
    the optimiser's step count) is skipped.  max_norm > 0: gradients of a larger global 2-norm are scaled by
    torch.nn.utils.clip_grad_norm_'s coefficient.  per_tensor: also keep the statistics of every parameter (per_tensor())."""

    def __init__(self, tree, policy='skip', max_norm=0.0, per_tensor=False):
        if policy not in POLICIES:
            raise ValueError('GradGuard: policy %r is not one of %s' % (policy, POLICIES))
        if not float(max_norm) >= 0.0:
            raise ValueError('GradGuard: max_norm %r must be >= 0 (0: no clipping)' % (max_norm,))
        self.tree = tree
        self.policy = policy
        self.flags = L.GUARD_SKIP if policy == 'skip' else 0
        self.max_norm = float(max_norm)
        dev = tree.flat.device
        self.n = tree.flat_grad.numel()
        # the segment table: one row per stored parameter, in memory order (ParamTree pads each to 4 elements: gaps)
        self._rows = [(name, off, _numel(tree._internal[name][0])) for name, off in tree._offsets.items()] if per_tensor else []
        self._rows.sort(key=lambda r: r[1])
        self.nseg = len(self._rows)
        table = [[off, cnt] for _, off, cnt in self._rows] or [[0, 0]]
        self._segs_host = torch.tensor(table, dtype=torch.int64)             # read by every hoig_grad_stats call: kept alive here
        self._segs_dev = self._segs_host.to(dev)
        nbytes = L.lib.hoig_grad_stats_workspace_bytes(self.n, self.nseg)
        if nbytes < 0:
            raise ValueError('GradGuard: hoig_grad_stats_workspace_bytes(%d, %d) refused' % (self.n, self.nseg))
        self._workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        self._total = torch.zeros(3, dtype=torch.float64, device=dev)
        self._seg_out = torch.zeros(max(self.nseg, 1), 3, dtype=torch.float64, device=dev)
        self.guard = torch.tensor([1.0, 0.0], dtype=torch.float32, device=dev)    # {scale, skip}: hoig_guard_decide writes it
        self.record = torch.zeros(len(RECORD_FIELDS), dtype=torch.float64, device=dev)
        self._pre_scale = 1.0
        self._optimizers = weakref.WeakSet()

    def observe(self, pre_scale=1.0):
        """Statistics of the tree's gradient buffer and the decision, on the current stream.  pre_scale: the factor the optimiser
        applies to the gradient (1 / world under a summed exchange), so that the norm is the norm of what Adam reads."""
        self._pre_scale = float(pre_scale)
        L.call('hoig_grad_stats', _p(self.tree.flat_grad), self.n, self._segs_host.data_ptr(), _p(self._segs_dev), self.nseg,
               _p(self._seg_out), _p(self._total), _p(self._workspace), _st())
        L.call('hoig_guard_decide', _p(self._total), self._pre_scale, self.max_norm, self.flags, _p(self.guard), _p(self.record),
               _st())

    def attach(self, optimizer):
        """An optimiser that steps under this guard: report() brings its host step count in line with the device's."""
        self._optimizers.add(optimizer)

    def report(self):
        """The record as a dict (copies to the host: synchronises).  norm / max / nonfinite are the last observed step's."""
        self.tree.wait_pending()                      # (the step may still be running on a side stream)
        rec = self.record.cpu().tolist()
        for o in list(self._optimizers):
            o.reconcile_step()
        out = OrderedDict(zip(RECORD_FIELDS, rec))
        for k in ('steps', 'skipped', 'clipped', 'nonfinite'):
            out[k] = int(out[k])
        return out

    def per_tensor(self):
        """{reference parameter name: (norm, max |g|, non-finite count)} of the last observed gradient (copies to the host).  A
        weight the tree stores in two halves is reported as one."""
        if not self.nseg:
            raise RuntimeError('GradGuard.per_tensor(): built with per_tensor=False')
        self.tree.wait_pending()
        rows = self._seg_out[:self.nseg].cpu().tolist()
        acc = OrderedDict((name, [0.0, 0.0, 0]) for name in self.tree.ref_names())
        for (name, _, _), (ss, mx, nf) in zip(self._rows, rows):
            a = acc[name.split('#')[0]]
            a[0] += ss
            a[1] = max(a[1], mx)
            a[2] += int(nf)
        s = self._pre_scale
        return OrderedDict((k, (s * a[0] ** 0.5, s * a[1], a[2])) for k, a in acc.items())


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n
