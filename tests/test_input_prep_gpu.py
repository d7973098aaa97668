"""GPU: hoig_amd.input_prep (HIP, through the C ABI) against the oracle restatement of HandRecoveryFlow.forward
(trainer.py:46-145) and against the reference-made fixture.  Every discrete output -- the four crop masks, the eroded
background mask, one-hot segments, the -2 flow sentinel, which atlas texels are painted -- must match EXACTLY; the
interpolated values (two bilinear samplers, 3-tap barycentric sums) within 2e-6 absolute on data in [-2, 10]."""
import os

import numpy as np
import pytest
import torch

from hoig_amd import synthetic
from oracle import input_prep_oracle as P

pytestmark = pytest.mark.gpu
NAMES = ['input_G_src_bg', 'input_G_tsf_bg', 'input_G_src_obj', 'input_G_tsf_obj', 'input_G_src_hand', 'input_G_ref_hand',
         'T_hand', 'src_crop_mask_bg', 'ref_crop_mask_bg', 'src_crop_mask_hand', 'ref_crop_mask_hand']
ATOL = 2e-6


def run_hip(r, bg_both, dexycb=False):
    from hoig_amd import input_prep as IP
    dev = torch.device('cuda', 0)
    tabs = {k: IP.ObjectTables(tb, dev) for k, tb in r['tables'].items()}
    c = lambda k: r[k].to(dev)
    return IP.prepare_inputs(c('src_img'), c('ref_img'), c('src_faces'), c('src_fim'), c('src_wim'), c('ref_fim'),
                             c('ref_wim'), [tabs[k] for k in r['obj_ids']], bg_both, dexycb)


def run_oracle(r, bg_both, dexycb=False):
    tabs = [r['tables'][k] for k in r['obj_ids']]
    return P.prepare_inputs(r['src_img'], r['ref_img'], r['src_faces'], r['src_fim'], r['src_wim'], r['ref_fim'],
                            r['ref_wim'], tabs, bg_both, dexycb)


def compare(hip, ora):
    for name, a, b in zip(NAMES, hip, ora):
        assert (a is None) == (b is None), name
        if a is None:
            continue
        a = a.cpu()
        assert a.shape == b.shape, name
        if 'mask' in name:
            assert torch.equal(a, b), name
        else:
            bad = ((a - b).abs() > ATOL)
            assert not bad.any(), '%s: %d of %d values differ, max %g' % (name, int(bad.sum()), a.numel(),
                                                                        float((a - b).abs().max()))
    # discrete channels inside the float tensors: exact
    assert torch.equal(hip[0][:, 3].cpu(), ora[0][:, 3])                          # 15x15-eroded background mask
    for i in (2, 3):
        assert torch.equal(hip[i][:, 5:].cpu(), ora[i][:, 5:])                    # flag + one-hot object segments
    assert torch.equal((hip[6] == -2).cpu(), ora[6] == -2)                        # the flow sentinel


@pytest.mark.parametrize('seed,batch,bg_both', [(8, 2, False), (8, 2, True), (11, 3, False), (13, 8, False)])
def test_hip_matches_oracle(seed, batch, bg_both):
    r = synthetic.make_raster(batch, seed)
    compare(run_hip(r, bg_both), run_oracle(r, bg_both))


def test_hip_matches_oracle_dexycb_layout():
    r = synthetic.make_raster(2, 14)
    hip, ora = run_hip(r, True, dexycb=True), run_oracle(r, True, dexycb=True)
    assert hip[4].shape[1] == 12 and hip[5].shape[1] == 12
    compare(hip, ora)
    for i in (4, 5):
        assert torch.equal(hip[i][:, 5:].cpu(), ora[i][:, 5:])                    # flag + the six hand-part one-hots


def test_hip_matches_reference_fixture():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'input_prep_256.npz'))
    r = synthetic.make_raster(int(g['batch']), int(g['seed']))
    for bg_both in (False, True):
        out = run_hip(r, bg_both)
        for name, v in zip(NAMES, out):
            if v is None:
                continue
            a = v.cpu().numpy()
            sub = a[:, 1::4, 2::4, :] if name == 'T_hand' else a[:, :, 1::4, 2::4]
            want = g['bg_both%d/%s/sub' % (bg_both, name)]
            if 'mask' in name:
                np.testing.assert_array_equal(sub, want, err_msg=name)
            else:
                np.testing.assert_allclose(sub, want, rtol=0, atol=ATOL, err_msg=name)
            np.testing.assert_allclose(a.astype(np.float64).sum(), float(g['bg_both%d/%s/sum' % (bg_both, name)]),
                                       rtol=1e-6, atol=1e-2)


def test_batched_launches_equal_the_per_sample_launches(monkeypatch):
    """Round 6: prepare_inputs issues hoig_prep_texture_batched / hoig_prep_lookup_batched (five launches per batch) where it used to
    loop over the samples (three launches each): the same arithmetic on the same tables, so every output is bit-identical; the
    per-sample entry points stay the C ABI of one sample and the path of batches beyond HOIG_PREP_MAX_BATCH."""
    from hoig_amd import input_prep as IP, synthetic
    r = synthetic.make_raster(3, 12)
    dev = torch.device('cuda', 0)
    args = [r[k].to(dev) for k in ('src_img', 'ref_img', 'src_faces', 'src_fim', 'src_wim', 'ref_fim', 'ref_wim')]
    tabs = [IP.ObjectTables(r['tables'][k], dev) for k in r['obj_ids']]
    assert len({id(t) for t in tabs}) > 1 or len(tabs) == 1
    a = IP.prepare_inputs(*args, tabs, bg_both=True)
    monkeypatch.setattr(IP, 'MAX_BATCH', 0)
    b = IP.prepare_inputs(*args, tabs, bg_both=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x, y)


def test_edge_cases_empty_and_full():
    r = synthetic.make_raster(1, 8)
    r['src_fim'] = -torch.ones_like(r['src_fim'])
    r['ref_fim'] = -torch.ones_like(r['ref_fim'])
    r['src_wim'] = torch.zeros_like(r['src_wim'])
    r['ref_wim'] = torch.zeros_like(r['ref_wim'])
    out = run_hip(r, True)
    compare(out, run_oracle(r, True))
    assert (out[6] == -2).all() and (out[7] == 1).all() and (out[9] == 1).all()
    r['src_fim'] = torch.zeros_like(r['src_fim'])
    r['ref_fim'] = torch.zeros_like(r['ref_fim'])
    r['src_wim'] = torch.full_like(r['src_wim'], 1.0 / 3)
    r['ref_wim'] = torch.full_like(r['ref_wim'], 1.0 / 3)
    out = run_hip(r, False)
    compare(out, run_oracle(r, False))
    assert (out[9] == 0).all() and (out[6] != -2).all()


def test_rejects_cpu_tensors_and_wrong_size():
    from hoig_amd import input_prep as IP
    r = synthetic.make_raster(1, 8)
    tabs = [IP.ObjectTables(r['tables'][r['obj_ids'][0]], torch.device('cuda', 0))]
    with pytest.raises(NotImplementedError):
        IP.prepare_inputs(r['src_img'], r['ref_img'], r['src_faces'], r['src_fim'], r['src_wim'], r['ref_fim'], r['ref_wim'],
                          tabs)
    bad = r['src_fim'].clone()
    bad[0, 0, 0] = 10 ** 6
    with pytest.raises(IndexError):
        IP.prepare_inputs(r['src_img'].cuda(), r['ref_img'].cuda(), r['src_faces'].cuda(), bad.cuda(), r['src_wim'].cuda(),
                          r['ref_fim'].cuda(), r['ref_wim'].cuda(), tabs, validate=True)
    # 'deferred' (the training loop's mode): no host wait; the bad index is clamped for the kernels and reported afterwards
    IP.prepare_inputs(r['src_img'].cuda(), r['ref_img'].cuda(), r['src_faces'].cuda(), bad.cuda(), r['src_wim'].cuda(),
                      r['ref_fim'].cuda(), r['ref_wim'].cuda(), tabs, validate='deferred')
    with pytest.raises(IndexError):
        IP.flush_range_checks()
    IP.flush_range_checks()                                  # reported once
    with pytest.raises(ValueError):
        IP.prepare_inputs(r['src_img'][:, :, :128, :128].cuda(), r['ref_img'].cuda(), r['src_faces'].cuda(),
                          r['src_fim'].cuda(), r['src_wim'].cuda(), r['ref_fim'].cuda(), r['ref_wim'].cuda(), tabs)


def test_trainer_accepts_rasterised_batches():
    """Trainer.set_input on a raw batch (images + rasteriser outputs + tables): stages what the oracle's tuple implies
    (trainer.py:346-362) and one optimisation step runs on it."""
    from hoig_amd import ops
    from hoig_amd.models import ModelsFactory
    from common import opt_namespace
    ops.set_precision('bf16x3')
    r = synthetic.make_raster(1, 9)
    opt = opt_namespace(gen_name='generator_spade_attn', local_rank=0, image_size=256)
    torch.manual_seed(3)
    model = ModelsFactory.get_by_name('trainer', opt, use_ddp=False)
    model.set_train()
    arm = torch.zeros(1, 1, 256, 256)
    batch = dict(src_img=r['src_img'], ref_img=r['ref_img'], src_faces=r['src_faces'], src_fim=r['src_fim'],
                 src_wim=r['src_wim'], ref_fim=r['ref_fim'], ref_wim=r['ref_wim'],
                 tables=[r['tables'][k] for k in r['obj_ids']], maskA=arm, maskB=arm)
    model.set_input(batch)
    want = P.to_prepared(run_oracle(r, False), r['src_img'], r['ref_img'], arm, arm)
    assert torch.equal(model._bg_mask.cpu(), want['bg_mask']) and torch.equal(model._hand_mask.cpu(), want['hand_mask'])
    assert (model._input_G_src_obj.cpu() - want['input_G_src_obj']).abs().max() <= ATOL
    assert (model._input_G_tsf_hand.cpu() - want['input_G_tsf_hand']).abs().max() <= ATOL
    assert (model._T.cpu() - want['T']).abs().max() <= ATOL
    model.optimize_parameters()
    errs = model.get_current_errors()
    assert all(np.isfinite(v) for v in errs.values()), errs


def test_trainer_reports_a_bad_face_index_of_the_last_batch():
    """a batch staged with the deferred range check is reported by the next host-side read (get_current_errors / save /
    get_current_visuals), not only when another batch follows; an eval-mode batch is checked before it runs."""
    from hoig_amd import ops
    from hoig_amd.models import ModelsFactory
    from common import opt_namespace
    ops.set_precision('bf16x3')
    r = synthetic.make_raster(1, 9)
    opt = opt_namespace(gen_name='generator_spade_attn', local_rank=0, image_size=256)
    torch.manual_seed(3)
    model = ModelsFactory.get_by_name('trainer', opt, use_ddp=False)
    arm = torch.zeros(1, 1, 256, 256)
    bad = r['ref_fim'].clone()
    bad[0, 5, 5] = 10 ** 6
    batch = dict(src_img=r['src_img'], ref_img=r['ref_img'], src_faces=r['src_faces'], src_fim=r['src_fim'],
                 src_wim=r['src_wim'], ref_fim=bad, ref_wim=r['ref_wim'],
                 tables=[r['tables'][k] for k in r['obj_ids']], maskA=arm, maskB=arm)
    model.set_train()
    model.set_input(batch)                       # no host wait, indices clamped for the kernels
    model.optimize_parameters()
    with pytest.raises(IndexError):
        model.get_current_errors()
    model.get_current_errors()                   # reported once
    model.set_eval()
    with pytest.raises(IndexError):
        model.set_input(batch)
    model.set_train()


# ---------------------------------------------------------------------------------------------------- constructed maps
# make_raster scenes are smooth: the discrete decisions of this stage -- the truncation of the visibility test, the opening of the
# occlusion mask, the erosions, the hand / object thresholds, the samplers' borders -- are probed here at their thresholds, on maps
# built by hand at the fixed 256 x 256 image and 256 x 640 atlas.
NH = synthetic.N_HAND_FACES
f32 = np.float32


def blank_scene(seed=31, batch=1):
    """A make_raster scene with nothing in it: no face in either view, no face in the atlas.  The tests below write into it."""
    r = synthetic.make_raster(batch, seed)
    for k in ('src_fim', 'ref_fim'):
        r[k].fill_(-1)
    for k in ('src_wim', 'ref_wim'):
        r[k].zero_()
    for tb in r['tables'].values():
        tb['fim_uv'].fill_(-1)
        tb['wim_uv'].zero_()
    return r, r['tables'][r['obj_ids'][0]]


def to_px(x):
    """((T + 1) / 2.0 * 255.0) in fp32, step by step (nmr.py:1012)"""
    return (np.asarray(x, f32) + f32(1)) / f32(2) * f32(255)


def coords_around(k):
    """fp32 coordinates whose pixel value to_px is the largest below k, k itself (where a coordinate reaches it: not at k = 1), and the
    smallest above k: the values next to k that a coordinate can reach (at k >= 1 the rounding of T + 1 is coarser than one ulp of k)."""
    c = [f32(2.0 * k / 255 - 1)]
    for _ in range(60):                                  # neighbours of the coordinate, and of the coordinate + 1
        c += [np.nextafter(max(c), f32(4)), np.nextafter(min(c), f32(-4))]
    s = [c[0] + f32(1)]
    for _ in range(60):
        s += [np.nextafter(max(s), f32(4)), np.nextafter(min(s), f32(-4))]
    c = np.array(sorted(set(c) | set(np.array(s, f32) - f32(1))), f32)
    px = to_px(c)
    assert (px < k).any() and (px > k).any() and ((px == k).any() or k == 1)
    return [c[px < k][-1]] + list(c[px == k][:1]) + [c[px > k][0]]


def textures(r, tb):
    """-> the atlas (3,256,640) of sample 0 by the per-sample kernel, by the batched kernel, and by the oracle"""
    import ctypes
    from hoig_amd import _lib as L, input_prep as IP
    dev = torch.device('cuda', 0)
    t = IP.ObjectTables(tb, dev)
    img, faces, fim = r['src_img'][:1].to(dev).contiguous(), r['src_faces'][:1].to(dev).contiguous(), r['src_fim'][:1].to(dev).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for batched in (False, True):
        occ = torch.empty(256 * 640, dtype=torch.uint8, device=dev)
        tex = torch.empty(3, 256, 640, dtype=torch.float32, device=dev)
        if batched:
            vp = lambda x: ctypes.cast((ctypes.c_void_p * 1)(x.data_ptr()), ctypes.c_void_p)
            L.call('hoig_prep_texture_batched', 1, img.data_ptr(), faces.data_ptr(), int(faces.stride(0)), fim.data_ptr(), vp(t.fim_uv),
                   vp(t.wim_uv), vp(t.obj_tex_img), occ.data_ptr(), tex.data_ptr(), st)
        else:
            L.call('hoig_prep_texture', img.data_ptr(), faces.data_ptr(), fim.data_ptr(), t.fim_uv.data_ptr(), t.wim_uv.data_ptr(),
                   t.obj_tex_img.data_ptr(), occ.data_ptr(), tex.data_ptr(), st)
        out.append(tex.cpu())
    nf = tb['map_fn'].shape[0] - 1
    f2pts = r['src_faces'][0, :nf, :, 0:2].clone()
    f2pts[:, :, 1] *= -1
    out.append(P.texture_backward_warp(r['src_img'][:1], f2pts, r['src_fim'][0], tb)[0])
    return out


def compare_textures(r, tb):
    """-> the oracle's atlas, after both kernels' were compared with it: the painted texels (1.0: occluded after the opening) exactly,
    the sampled ones within ATOL"""
    one, many, want = textures(r, tb)
    for got in (one, many):
        assert torch.equal(got[:, :, :384] == 1.0, want[:, :, :384] == 1.0)
        assert (got - want).abs().max() <= ATOL
    return want


def show_texel(r, tb, face, ty, tx, ry, rx):
    """Reference pixel (ry, rx) shows `face` (a hand face), whose first atlas vertex is the centre of texel (ty, tx): the pipeline's
    input_G_ref_hand reads that texel there (align_corners=True, trainer.py:86)."""
    tb['faces_uv_coord'][0, face, 0] = torch.tensor([tx / 639.0 * 2 - 1, ty / 255.0 * 2 - 1])
    r['ref_fim'][0, ry, rx] = face
    r['ref_wim'][0, ry, rx] = torch.tensor([1.0, 0.0, 0.0])


def test_visibility_truncates_toward_zero_at_pixel_boundaries():
    """prep_occlusion_kernel: an atlas texel's face is visible when the source view shows it in the 3 x 3 window round
    ((T + 1) / 2 * 255).long().clamp(0, 255).  The coordinates give pixel values just below, at and just above k = 0, 1, 128, 254, 255,
    negative fractions (which truncate to 0, not to -1) and values beyond 255; the source view shows the face in one corner of the
    window only, or two pixels from its centre only."""
    r, tb = blank_scene()
    probes = [(float(k), c) for k in (0, 1, 128, 254, 255) for c in coords_around(k)]
    probes += [(None, f32(v)) for v in (-1.004, -1.0075, 1.002, 2.0 * 256 / 255 - 1, 1.4)]    # px -0.51, -0.96, 255.26, 256, 306
    face, want_occluded, blocks = 0, {}, []
    for axis in (0, 1):
        for _, c in probes:
            centre = min(max(int(to_px(c)), 0), 255)                       # int(): toward zero
            for d_along, d_across in ((1, 1), (-1, 1), (2, 0), (-2, 0)):   # two corners of the window; two pixels outside it
                q = centre + d_along
                if not 0 <= q <= 255:
                    continue
                other = 3 + 2 * (face % 120)
                by, bx = 4 + 6 * (face // 60), 4 + 6 * (face % 60)         # a 4 x 4 block of atlas texels for this probe
                assert bx + 4 < 384 and by + 4 < 256 and face < NH
                xy = [c, f32(2.0 * (other + 0.5) / 255 - 1)]
                x, y = xy if axis == 0 else xy[::-1]
                r['src_faces'][0, face] = torch.tensor([[x, -y, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
                px = (q, other + d_across) if axis == 0 else (other + d_across, q)
                assert int(r['src_fim'][0, px[1], px[0]]) == -1
                r['src_fim'][0, px[1], px[0]] = face
                tb['fim_uv'][0, by:by + 4, bx:bx + 4] = face
                tb['wim_uv'][0, by:by + 4, bx:bx + 4] = torch.tensor([1.0, 0.0, 0.0])
                show_texel(r, tb, face, by + 1, bx + 1, 2 + 3 * (face // 80), 2 + 3 * (face % 80))
                want_occluded[face] = abs(d_along) == 2
                blocks.append((face, by, bx))
                face += 1
    assert face >= 100 and 40 <= sum(want_occluded.values()) <= face - 40
    r['src_wim'][r['src_fim'] >= 0] = torch.tensor([0.2, 0.3, 0.5])
    tex = compare_textures(r, tb)
    for f, by, bx in blocks:                                               # the construction says what it means to
        assert bool((tex[:, by + 1:by + 3, bx + 1:bx + 3] == 1.0).all()) == want_occluded[f], f
    hip, ora = run_hip(r, True), run_oracle(r, True)
    compare(hip, ora)
    painted = (ora[5][0, :3] == 1.0).all(0)
    assert int(painted.sum()) == sum(want_occluded.values())


def test_opening_of_the_occlusion_mask():
    """The occlusion mask is eroded and dilated (3 x 3, nmr.py:1052-1054; the outside counts as occluded for the erosion): single texels
    and 2 x 2 islands go, 3 x 3 islands stay; at the atlas' borders and corners, where the outside stands in for a row or a column; and across the seam between
    column 383, the last painted one, and column 384, which the mask still covers."""
    r, tb = blank_scene(seed=32)
    hidden, shown = 5, 6                                # hand faces: `hidden` is in no source pixel, `shown` in all of them
    r['src_fim'].fill_(shown)
    r['src_wim'][:] = torch.tensor([0.2, 0.3, 0.5])
    for f in (hidden, shown):
        r['src_faces'][0, f] = torch.tensor([[-0.3, 0.2, 1.0], [0.4, 0.1, 1.0], [0.1, -0.5, 1.0]])
    g = np.random.default_rng(32)
    fim_uv = np.where(g.uniform(size=(256, 640)) < 0.5, shown, -1).astype(np.int32)       # free texels: a visible face, or none
    isl = []                                            # (y, x, h, w) of occluded islands, a free margin round each
    isl += [(0, 0, 1, 1), (0, 639, 2, 2), (254, 0, 2, 2), (255, 639, 1, 1)]               # corners (the right ones are painted over)
    isl += [(0, 20, 1, 3), (0, 30, 2, 3), (0, 40, 2, 2), (0, 50, 2, 1), (254, 20, 2, 3), (255, 30, 1, 3), (254, 40, 2, 2)]   # top, bottom
    isl += [(20, 0, 3, 1), (30, 0, 3, 2), (40, 0, 2, 2), (50, 0, 1, 2), (20, 638, 3, 2), (30, 639, 3, 1)]                   # left, right
    isl += [(60, 382, 3, 2), (70, 382, 3, 3), (80, 383, 3, 1), (90, 383, 3, 3), (100, 381, 3, 3), (110, 384, 3, 3), (120, 382, 2, 4)]   # seam
    isl += [(140, 100, 1, 1), (140, 110, 2, 2), (140, 120, 3, 3), (140, 130, 4, 4), (140, 140, 3, 2), (140, 150, 2, 3), (140, 160, 5, 3)]
    for y, x, h, w in isl:
        fim_uv[max(y - 2, 0):y + h + 2, max(x - 2, 0):x + w + 2] = shown
        fim_uv[y:y + h, x:x + w] = hidden
    fim_uv[150:153, 170:173] = hidden                                   # a 3 x 3 island without a corner, an L, a 3 x 3 ring
    fim_uv[150, 170] = shown
    fim_uv[150:153, 180] = fim_uv[152, 180:183] = hidden
    fim_uv[150:153, 190:193] = hidden
    fim_uv[151, 191] = -1
    tb['fim_uv'][0] = torch.from_numpy(fim_uv)
    tb['wim_uv'][0] = torch.tensor([0.25, 0.25, 0.5])
    tb['wim_uv'][0][tb['fim_uv'][0] < 0] = 0.0
    tex = compare_textures(r, tb)
    painted = (tex == 1.0).all(0)
    stays = lambda y, x, h, w: bool(painted[y:y + h, x:min(x + w, 384)].all())
    goes = lambda y, x, h, w: not bool(painted[max(y - 1, 0):y + h + 1, max(x - 1, 0):min(x + w + 1, 384)].any())
    assert goes(140, 100, 1, 1) and goes(140, 110, 2, 2) and stays(140, 120, 3, 3) and stays(140, 130, 4, 4) and goes(140, 140, 3, 2)
    assert goes(0, 0, 1, 1) and stays(254, 0, 2, 2) and stays(0, 30, 2, 3) and goes(0, 20, 1, 3) and goes(0, 40, 2, 2) and goes(0, 50, 2, 1)
    assert stays(30, 0, 3, 2) and goes(20, 0, 3, 1) and goes(40, 0, 2, 2) and goes(50, 0, 1, 2) and stays(254, 20, 2, 3) and goes(255, 30, 1, 3)
    assert goes(60, 382, 3, 2) and stays(70, 382, 3, 3) and goes(80, 383, 3, 1) and stays(90, 383, 3, 3) and stays(100, 381, 3, 3)
    assert goes(120, 382, 2, 4) and not painted[:, 384:].any() and not painted[150:153, 170:173].any() and not painted[150:153, 190:193].any()
    # through the pipeline: the reference view reads columns 378..389 of rows 56..127 and the top left corner, texel by texel
    n = 0
    for ty in list(range(56, 128)) + list(range(0, 8)):
        for tx in range(378, 390) if ty >= 56 else range(0, 56):
            show_texel(r, tb, 100 + n, ty, tx, 1 + 3 * (n // 84), 1 + 3 * (n % 84))
            n += 1
    assert 100 + n <= NH
    hip, ora = run_hip(r, False), run_oracle(r, False)
    compare(hip, ora)
    assert (ora[5][0, :3] == 1.0).all(0).sum() >= 9


def test_erosions_at_distance_one_two_seven_and_eight():
    """A single pixel that is not background (an object face) or is hand (a hand face), in the interior, on every border and in every
    corner: the 3 x 3 erosions clear Chebyshev distance 1 and keep distance 2, the 15 x 15 one clears 7 and keeps 8; the outside of
    the image counts as 1 (util.morph pads with ones)."""
    r, tb = blank_scene(seed=33)
    spots = [(60, 60), (0, 100), (255, 100), (100, 0), (100, 255), (0, 0), (0, 255), (255, 0), (255, 255), (7, 180), (180, 8), (248, 200)]
    for view in ('src', 'ref'):
        for n, (y, x) in enumerate(spots):
            if view == 'ref':
                y, x = x, y
            for dx, face in ((0, NH + 3 + n), (30, 7 + n)):                 # an object face; thirty columns on, a hand face
                xx = x + dx if x + dx < 256 and x not in (255,) else x - dx
                r[view + '_fim'][0, y, xx] = face
                r[view + '_wim'][0, y, xx] = torch.tensor([0.5, 0.25, 0.25])
    hip, ora = run_hip(r, True), run_oracle(r, True)
    compare(hip, ora)
    smb, smh, sbg, rbg = ora[7][0, 0], ora[9][0, 0], ora[0][0, 3], ora[1][0, 3]
    assert smb[59:62, 59:62].sum() == 0 and smb[58:63, 58:63].sum() == 16 and smb[61, 61] == 0 and smb[62, 62] == 1
    assert sbg[53:68, 53:68].sum() == 0 and sbg[52:69, 52:69].sum() == 17 * 17 - 15 * 15 and sbg[67, 67] == 0 and sbg[68, 68] == 1
    assert smh[59:62, 89:92].sum() == 0 and smh[58:63, 88:93].sum() == 16 and smh[59:62, 59:62].sum() == 9      # the object pixel is no hand
    assert smb[:2, :2].sum() == 0 and smb[2, 2] == 1 and smb[0, 2] == 1 and sbg[:8, :8].sum() == 0 and sbg[8, 8] == 1 and sbg[0, 8] == 1
    assert smb[254:, 254:].sum() == 0 and smb[253, 253] == 1 and sbg[248:, 248:].sum() == 0 and sbg[247, 247] == 1
    assert smb[0, 99:102].sum() == 0 and smb[1, 99:102].sum() == 0 and smb[2, 100] == 1 and sbg[7, 100] == 0 and sbg[8, 100] == 1
    assert sbg[0:15, 173:188].sum() == 0 and sbg[15, 180] == 1 and sbg[7, 172] == 1                      # (7, 180): the window ends at row 0
    assert rbg[60 - 7:60 + 8, 60 - 7:60 + 8].sum() == 0 and rbg[68, 68] == 1


def test_thresholds_of_faces_labels_atlas_coordinate_and_samplers():
    """Face indices NHAND - 1 (hand) and NHAND (object); segment labels 0, 6, 7 and 15; the atlas coordinate u = 1.5 exactly, where
    neither the hand nor the object flag fires (trainer.py:113-125); T_hand where the eroded hand mask is 0 and where it is 1; and
    sample points exactly at -1 and +1 in the sampler of the atlas (align_corners=False) and of the views (align_corners=True)."""
    r, tb = blank_scene(seed=34)
    nf = tb['n_faces']
    faces = [NH - 1, NH, 20, 21, NH + 1, nf - 1, 22, NH + 2, 23, 24, 25, 26]
    labels = [6, 7, 0, 6, 7, 15, 1, 0, 2, 3, 4, 5]
    us = [0.5, 2.5, 1.5, np.nextafter(f32(1.5), f32(0)), np.nextafter(f32(1.5), f32(2)), 1.5, 0.0, 1.5, 1.0, 0.25, 0.75, 1.25]
    corners = [(-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0)]
    for n, (f, lab, u) in enumerate(zip(faces, labels, us)):
        tb['sem_full'][f, 0] = lab
        tb['map_fn'][f] = torch.tensor([float(u), 0.5, 0.0])
        # the face's atlas triangle and its source triangle have their first vertices on a corner of the sampling square
        tb['faces_uv_coord'][0, f] = torch.tensor([corners[n % 4], corners[(n + 1) % 4], [0.0, 0.0]])
        cx, cy = corners[(n + 2) % 4]
        r['src_faces'][0, f] = torch.tensor([[cx, -cy, 1.0], [cx, cy, 1.0], [0.1, 0.2, 1.0]])
        # three strips of atlas texels, two wide (an occluded strip that narrow is opened away, so its texels are sampled): weights that
        # pick vertex 0, vertex 1, and a blend
        for x0, w in ((10, [1.0, 0.0, 0.0]), (13, [0.0, 1.0, 0.0]), (16, [0.25, 0.25, 0.5])):
            tb['fim_uv'][0, 10 + 8 * n:16 + 8 * n, x0:x0 + 2] = f
            tb['wim_uv'][0, 10 + 8 * n:16 + 8 * n, x0:x0 + 2] = torch.tensor(w)
        for view in ('src', 'ref'):
            y0, x0 = (12 + 20 * n, 30) if view == 'src' else (40, 8 + 20 * n)
            r[view + '_fim'][0, y0:y0 + 5, x0:x0 + 5] = f                   # 5 x 5: the eroded hand mask is 0 on all of it, 1 from two pixels off
            r[view + '_wim'][0, y0:y0 + 5, x0:x0 + 5] = torch.tensor([0.25, 0.5, 0.25])
            r[view + '_wim'][0, y0, x0:x0 + 5] = torch.tensor([1.0, 0.0, 0.0])          # sample points exactly on the corners
            r[view + '_wim'][0, y0 + 1, x0:x0 + 5] = torch.tensor([0.0, 1.0, 0.0])
    tex = compare_textures(r, tb)
    img = r['src_img'][0]
    for n in range(len(faces)):                                            # a sample point on a corner of the source image: a quarter of that pixel
        cx, cy = corners[(n + 2) % 4]
        want = 0.25 * img[:, 0 if cy < 0 else 255, 0 if cx < 0 else 255]
        assert (tex[:, 12 + 8 * n, 10] - want).abs().max() <= ATOL and (tex[:, 12 + 8 * n, 11] - want).abs().max() <= ATOL
        want = 0.25 * img[:, 255 if cy < 0 else 0, 0 if cx < 0 else 255]    # vertex 1: (cx, -cy)
        assert (tex[:, 12 + 8 * n, 13] - want).abs().max() <= ATOL
    for dexycb in (False, True):
        hip, ora = run_hip(r, True, dexycb), run_oracle(r, True, dexycb)
        compare(hip, ora)
        for i in (4, 5):
            assert torch.equal(hip[i][:, 5:].cpu(), ora[i][:, 5:])
    src_obj, src_hand, T, rmh = ora[2][0], ora[4][0], ora[6][0], ora[10][0, 0]       # (the DexYCB layout: 12 hand channels)
    px = lambda t, n: t[:, 12 + 20 * n + 2, 32]                             # the middle of face n's source block
    # channels: [image 0:3 | u, v, flag 3:6 | one-hots 6:]; the hand tensor's one-hots are labels 1..6, the object tensor's 7..15
    assert px(src_hand, 0)[6:].tolist() == [0, 0, 0, 0, 0, 1] and px(src_obj, 0)[6:].sum() == 0                       # NHAND - 1: hand, label 6
    assert px(src_hand, 0)[3:6].tolist() == [0.5, 0.5, 0] and px(src_obj, 0)[3:6].tolist() == [0, 0, 1]
    assert px(src_obj, 1)[6:].tolist() == [1] + [0] * 8 and px(src_hand, 1)[6:].sum() == 0                            # NHAND: object, label 7
    assert px(src_obj, 1)[3:6].tolist() == [2.5, 0.5, 0] and px(src_hand, 1)[3:6].tolist() == [0, 0, 1]
    assert px(src_obj, 5)[6:].tolist() == [0] * 8 + [1]                                                               # label 15
    assert px(src_obj, 2)[6:].sum() == 0 and px(src_hand, 2)[6:].sum() == 0                                           # label 0
    for n in (2, 5, 7):                                                    # u = 1.5: neither flag fires, both splits zero u, v and set their flag
        assert px(src_hand, n)[3:6].tolist() == [0, 0, 1] and px(src_obj, n)[3:6].tolist() == [0, 0, 1]
    assert px(src_hand, 3)[3] == us[3] and px(src_obj, 3)[3] == 0 and px(src_obj, 4)[3] == us[4] and px(src_hand, 4)[3] == 0
    assert rmh[40:45, 8:13].sum() == 0 and rmh[39, 7] == 0 and rmh[38, 6] == 1 and rmh[42, 30] == 1                  # hand 5 x 5 and its ring
    assert (T[40:45, 8:13] != -2).all() and (T[38, 6] == -2).all() and (T[42, 30] == -2).all()                       # object pixels: mask 1
    assert T[40, 8].tolist() == [corners[2][0], corners[2][1]]             # the flow at a sample point on the corner, exactly
