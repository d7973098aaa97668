"""What the model feeds its instance norms (docs/norm_conditioning.md, first table): the CPU oracle runs the configurations of the
committed 64 x 64 fixtures and a synthetic batch whose first image has a flat background, and every F.instance_norm call records
the largest |mean| / sigma over (image, channel) of its input, in float64, and the share of (image, channel) pairs above 2.6 --
the ratio from which hoig_inorm_stats_from_sums recomputes a channel from the tensor instead of trusting the plain sums.

    python tools/norm_conditioning.py            # prints the markdown table (CPU only, about a minute)
"""
import os
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from common import SEEDS, seeded_state          # noqa: E402
from hoig_amd import synthetic                  # noqa: E402
from oracle import hogan_oracle as O            # noqa: E402

REDO = 2.6          # sqrt(SUMS_COND - 1) of hoig_amd/csrc/norm.hip


class Recorder:
    def __init__(self):
        self.rows = OrderedDict()
        self._orig = F.instance_norm

    def __enter__(self):
        def hook(x, *a, **k):
            f = sys._getframe(1)
            who = f.f_code.co_name
            if who == '_inorm':                   # the oracle's wrapper: name the layer by its caller
                who = f.f_back.f_code.co_name + ':' + str(f.f_locals.get('name') or f.f_back.f_locals.get('p') or 'param-free')
            x64 = x.detach().double()
            m = x64.mean(dim=(2, 3))
            s = x64.var(dim=(2, 3), unbiased=False).sqrt()
            ratio = m.abs() / s.clamp_min(1e-300)
            key = (who, tuple(x.shape[1:]))
            old = self.rows.get(key, (0.0, 0, 0, 0))
            self.rows[key] = (max(old[0], float(ratio.max())), old[1] + int((ratio > REDO).sum()), old[2] + ratio.numel(),
                              old[3] + int((s == 0).sum()))
            return self._orig(x, *a, **k)
        F.instance_norm = hook
        return self

    def __exit__(self, *exc):
        F.instance_norm = self._orig


def flat_background_inputs(batch, side):
    """synthetic.make_inputs with image 0 repainted: a flat 0.8 where the random texture was (background, hand and object alike)."""
    inp = synthetic.make_inputs(batch, side, seed=SEEDS['inputs'])
    inp['real_src'][0] = 0.8
    inp['real_tsf'][0] = 0.8
    inp['input_G_bg'][0, :3] = 0.8 * inp['input_G_bg'][0, 3]
    for k in ('input_G_src_hand', 'input_G_tsf_hand', 'input_G_src_obj', 'input_G_tsf_obj'):
        inp[k][0, :3] = 0.8 * (1.0 - inp[k][0, 5])
    return inp


def run(gen_name, batch, side, dataset='hov3', inputs=None, steps=2):
    cfg, sdG, sdD, sdV = seeded_state(gen_name, dataset)
    ot = O.OracleTrainer(cfg, sdG, sdD, sdV)
    ot.set_prepared_input(inputs if inputs is not None else synthetic.make_inputs(batch, side, seed=SEEDS['inputs'], dataset=dataset))
    with Recorder() as rec:
        for _ in range(steps):
            ot.optimize_parameters()
    return rec.rows


def layer_family(who, shape):
    fn, _, layer = who.partition(':')
    return '%s / %s, C = %d' % (layer.split('.')[0] if '.' in layer else 'discriminator', fn, shape[0])


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cases = [('A', 'generator_spade_attn, hov3, batch 2, 64x64, two steps (fixture hov3_spade_attn_64)', ('generator_spade_attn', 2, 64)),
             ('B', 'generator_base, hov3, batch 2, 64x64, two steps (fixture hov3_base_64)', ('generator_base', 2, 64)),
             ('C', 'generator_spade_attn, dexycb, batch 2, 64x64, two steps (fixture dexycb_spade_attn_64)', ('generator_spade_attn', 2, 64, 'dexycb')),
             ('D', 'as A, image 0 repainted with a FLAT 0.8 background', ('generator_spade_attn', 2, 64, 'hov3', flat_background_inputs(2, 64))),
             ('E', 'as D at batch 1, 128x128, one step', ('generator_spade_attn', 1, 128, 'hov3', flat_background_inputs(1, 128), 1))]
    table, tail = OrderedDict(), []
    for tag, title, args in cases:
        rows = run(*args)
        for (who, shape), (mx, hi, n, const) in rows.items():
            fam = table.setdefault(layer_family(who, shape), {})
            old = fam.get(tag, (0.0, 0, 0))
            fam[tag] = (max(old[0], mx), old[1] + hi, old[2] + n)
        worst = max(v[0] for v in rows.values())
        hi, n, const = (sum(v[k] for v in rows.values()) for k in (1, 2, 3))
        tail.append('- **%s**: %s -- largest ratio %.3g; %d of %d (image, channel) pairs above %.1f (%.2f %%); %d constant channels'
                    % (tag, title, worst, hi, n, REDO, 100.0 * hi / n, const))
    tags = [c[0] for c in cases]
    print('| norm inputs of (sub-network / oracle function, channels) | ' + ' | '.join(tags) + ' |')
    print('|---|' + '---|' * len(tags))
    for fam, cols in table.items():
        print('| %s | ' % fam + ' | '.join(('%.3g (%d)' % cols[t][:2]) if t in cols else '-' for t in tags) + ' |')
    print('\nEach cell: largest abs(mean)/sigma over (image, channel) of the inputs of those norms, in float64, and in brackets how many pairs exceed %.1f.\n' % REDO)
    print('\n'.join(tail))


if __name__ == '__main__':
    main()
