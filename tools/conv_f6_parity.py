"""The numbers of docs/conv_f6_parity.md, measured on the device:   python tools/conv_f6_parity.py [out.json]

Per row of tests/conv_f6_reference.ROWS:
  * the YARDSTICK of TOL_F6 -- the three-term kernel (ops.conv2d under 'bf16x3') on the row's operands against its own operand-rounded
    float64 emulation (conv_f6_reference.three_term_ref): what fp32 accumulation in MFMA order costs a kernel that is not under test;
  * the row itself through tests/test_conv_f6_gpu.check_row: route, kernel vs emulation, kernel vs float64, emulation vs float64.
TOL_F6 = 4 x the largest yardstick value, rounded up to one digit."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch

import conv_f6_reference as F6
import test_conv_f6_gpu as T
from hoig_amd import _lib as L, ops


def yardstick(rid):
    r, o = F6.ROW[rid], F6.operands(rid)
    x = F6.gathered_input(o['x'], None, o['in_scale'], o['in_shift'], r.relu_c0)
    ops.set_precision('bf16x3')
    try:
        with torch.no_grad():
            y = ops.conv2d(x.cuda(), ops.pack_weight(o['w'].cuda()), None, 1, 1)
        route = L.last_route(L.ROUTE_FWD)
        torch.cuda.synchronize()
    finally:
        ops.set_precision('f32')
    return route, F6.rel_err64(y, F6.three_term_ref(x, o['w']))


def main():
    out = {}
    print('| row | B, Ci->Co, HxW | three-term kernel vs its emulation (route) | route | kernel vs emulation | kernel vs float64 | emulation vs float64 |')
    print('|---|---|---|---|---|---|---|')
    for r in F6.ROWS:
        rep = {}
        rep['x3_route'], rep['x3_vs_emu'] = yardstick(r.id)
        try:
            T.check_row(r.id, rep)
            rep['passed'] = True
        except AssertionError as e:
            rep['passed'] = False
            rep['failure'] = str(e)[:300]
        out[r.id] = rep
        print('| `%s` | %d, %d->%d, %dx%d | %.1e (`%s`) | `%s` | %s | %s | %.1e |%s' % (
            r.id, r.B, r.Ci, r.Co, r.H, r.W, rep['x3_vs_emu'], rep['x3_route'], rep.get('route'),
            '%.1e' % rep['vs_emu'] if 'vs_emu' in rep else '-', '%.1e' % rep['vs_f64'] if 'vs_f64' in rep else '-', rep['emu_vs_f64'],
            '' if rep['passed'] else ' FAILED: ' + rep['failure']), flush=True)
    worst = max(v['x3_vs_emu'] for v in out.values())
    digit = 10.0 ** math.floor(math.log10(4 * worst))
    tol = math.ceil(4 * worst / digit - 1e-9) * digit
    print('\nlargest three-term kernel vs emulation %.2e -> TOL_F6 = 4 x that, rounded up to one digit = %.0e (the tests use %.0e)' % (
        worst, tol, F6.TOL_F6))
    print('largest fp6 kernel vs emulation (rows without tanh / sigmoid): %.2e' % max(
        v.get('vs_emu', 0.0) for k, v in out.items() if F6.ROW[k].act not in ('tanh', 'sigmoid')))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
