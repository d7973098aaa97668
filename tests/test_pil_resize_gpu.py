"""hoig_resize_pil_bilinear_u8 on the MI355X against Pillow, every byte (cases and restatement: tests/pil_resize_reference.py)."""
import numpy as np
import pytest
import torch
from PIL import Image

import pil_resize_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
IDS = ['%dx%d-%dx%d' % (c[0] + c[1]) for c in R.CASES]


@pytest.mark.parametrize('case', R.CASES, ids=IDS)
def test_the_device_resize_equals_pillow_every_byte(case):
    from hoig_amd.metrics import kernels as K
    (h, w), size = case
    for binary in (False, True):
        a = R.content(3, h, w, h * 13 + w, binary)
        got = K.pil_resize_u8(torch.from_numpy(a).to(DEV), size)
        assert got.shape == (3,) + size + (3,) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.pillow(a, size)), binary


def test_the_chain_equals_resize_chain_and_cached_tables_repeat_it():
    from hoig_amd.metrics import images as I
    from hoig_amd.metrics import kernels as K
    (h, w), mid, side = R.CHAIN
    assert (mid, side) == (256, I.EVAL_SIDE)
    a = R.content(2, h, w, 3)
    want = np.stack([np.asarray(I.resize_chain(Image.fromarray(im), mid)) for im in a])
    K._pil_tables.clear()
    u8 = torch.from_numpy(a).to(DEV)
    first = K.pil_resize_chain_u8(u8, mid)
    assert np.array_equal(first.cpu().numpy(), want)
    tables = dict(K._pil_tables)
    assert sorted(k[:2] for k in tables) == sorted([(h, mid), (w, mid), (mid, side)])
    second = K.pil_resize_chain_u8(u8, mid)
    assert all(K._pil_tables[k] is t for k, t in tables.items()) and len(K._pil_tables) == len(tables)    # (nothing rebuilt)
    assert torch.equal(first, second)
