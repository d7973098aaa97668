"""Generates the fixtures of the comparisons that used to run the REFERENCE's own Python at test time (oracle/ref_harness.py),
so that those tests run on stored results wherever the suite runs.  Build container only, one reference copy per process:
    python tests/golden/make_golden_live_pins.py vertex       -> raster_vertex_stage_seed7.npz  (the (B,F,3,3) face tensor)
    python tests/golden/make_golden_live_pins.py wrapper      -> raster_wrapper_64.npz          (face index map, weight map)
    python tests/golden/make_golden_live_pins.py input_prep   -> input_prep_live.npz            (as input_prep_256.npz: CRC32,
                                                                                               sums, every 4th pixel)
    python tests/golden/make_golden_live_pins.py data_lines   -> reference_data_lines.npz       (64-bit digests of the
                                                                                               non-trivial lines of the
                                                                                               reference's data/*.py files)
Inputs are re-derived from seeds at test time; nothing of the reference's source travels (the line digests are one-way)."""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_harness as RH           # noqa: E402

INPUT_PREP_CASES = [(11, 3, False), (12, 1, True)]          # (seed, batch, bg_both)


def vertex():
    from make_golden_raster_vertex import inputs
    cam, verts, idx = inputs(seed=7, B=4, V=40, F=70)
    faces = RH.reference_vertex_stage(cam.clone(), verts.clone(), idx)
    return 'raster_vertex_stage_seed7.npz', dict(faces=faces.numpy())


def wrapper():
    from common import synthetic_mesh_faces
    rf, rw = RH.reference_rasterize_wrapper(synthetic_mesh_faces(2, 300), 64)
    return 'raster_wrapper_64.npz', dict(fim=rf.numpy(), wim=rw.numpy())


def input_prep():
    from hoig_amd import synthetic
    from make_golden_input_prep import NAMES, summarise
    out = {}
    for seed, batch, bg_both in INPUT_PREP_CASES:
        ref = RH.reference_input_prep(synthetic.make_raster(batch, seed), bg_both=bg_both)
        for name, v in zip(NAMES, ref):
            key = 'seed%d/%s' % (seed, name)
            out[key + '/present'] = np.bool_(v is not None)
            if v is not None:
                summarise(out, v.numpy(), key)
    return 'input_prep_live.npz', out


def data_lines():
    from common import line_digests
    refs = sorted(glob.glob(os.path.join(RH.REF_ROOT, '*', 'data', '*.py')))
    return 'reference_data_lines.npz', {'file%d' % i: line_digests(p) for i, p in enumerate(refs)}


if __name__ == '__main__':
    name, out = dict(vertex=vertex, wrapper=wrapper, input_prep=input_prep, data_lines=data_lines)[sys.argv[1]]()
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
