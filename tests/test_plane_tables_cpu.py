"""The tables hoig_adam_pack_step walks (ParamTree._build_plane_table, _build_plain_chunks in hoig_amd/nn.py), built on the CPU for the
real networks' schemas and for the tree of tests/test_adam_gpu.py: rows and plain chunks cover the flat buffer exactly once, in the
units the kernel assumes (docs/optimizer_parity.md)."""
import pytest
import torch

import adam_reference as A

CPU = torch.device('cpu')


def _generator(name):
    from hoig_amd.models.networks.generator import Generator
    return Generator(bg_dim=8, img_dim=3, obj_dim=3, img_cond_dim=3, obj_cond_dim=12, gen_name=name, device=CPU)


def _discriminator():
    from hoig_amd.models.networks.discriminator import PatchDiscriminator
    return PatchDiscriminator(input_nc=19, ndf=64, n_layers=4, norm_type='instance', device=CPU)


def _test_tree():
    from hoig_amd.nn import ParamTree
    return ParamTree(A.TREE_SHAPES, CPU, transposed_names=A.TREE_TRANSPOSED)


TREES = {'generator_spade_attn': lambda: _generator('generator_spade_attn'), 'generator_spade': lambda: _generator('generator_spade'),
         'generator_base': lambda: _generator('generator_base'), 'discriminator': _discriminator, 'test_tree': _test_tree}


@pytest.mark.parametrize('which', sorted(TREES))
def test_rows_and_plain_chunks_partition_the_flat_buffer(which):
    tree = TREES[which]()
    tree._ensure_plane_bufs()
    n = tree.flat.numel()
    rows = tree._plane_table.tolist()
    assert rows and tree._plain_chunks is not None, 'the fused step is not in use'
    assert tree.fused_step_tables() is not None and len(tree._plane_bufs) == 4 and all(b.numel() == n for b in tree._plane_bufs)
    chunks, nchunks = tree._plain_chunks
    chunks = chunks.tolist()[:nchunks]
    tiles = 0
    spans = []
    for off, co, rs, ci, flags, first in rows:
        assert off % 4 == 0 and co % 32 == 0 and ci % 32 == 0 and co > 0 and ci > 0 and rs > 0
        assert flags == (1 if co > 32 else 0) | (2 if ci > 32 else 0) and flags in (1, 2, 3)
        assert first == tiles
        tiles += (co // 32) * (ci // 32)
        spans.append((off, off + co * rs * ci))
        assert tree._plane_flags[off] == flags
    assert tiles == tree._plane_tiles
    for a, c in chunks:
        assert a % 4 == 0 and c % 4 == 0 and 0 < c <= 1024
        spans.append((a, a + c))
    spans.sort()
    at = 0
    for a, b in spans:          # no overlap, no gap
        assert a == at, (which, a, at)
        at = b
    assert at == n
    # every parameter lies inside one row or inside plain chunks, never across a row's edge
    row_spans = sorted((r[0], r[0] + r[1] * r[2] * r[3]) for r in rows)
    for name, off in tree._offsets.items():
        size = 1
        for s in tree._internal[name][0]:
            size *= s
        inside = [(a, b) for a, b in row_spans if a < off + size and off < b]
        assert len(inside) <= 1 and all(a <= off and off + size <= b for a, b in inside), name


def test_the_test_tree_has_every_kind_of_row():
    tree = _test_tree()
    tree._ensure_plane_bufs()
    rows = tree._plane_table.tolist()
    assert rows[0][0] == 0 and rows[1][0] == rows[0][0] + 64 * 9 * 32 and rows[2][0] == rows[1][0] + 32 * 9 * 64      # back to back
    assert sorted(r[4] for r in rows) == [1, 2, 3, 3, 3]
    assert [r[1:4] for r in rows if r[0] == tree._offsets['up.weight']] == [[96, 9, 64]]                            # (Ci, Co) swapped
    assert [r[1:4] for r in rows if r[0] == tree._offsets['s.mlp_gamma.weight']] == [[64, 9, 128]]                  # gamma | beta: one row
    assert tree._offsets['s.mlp_beta.weight'] not in tree._plane_flags
    chunks = tree._plain_chunks[0].tolist()[:tree._plain_chunks[1]]
    assert [tree._offsets['d.weight'], 1024] in chunks                          # exactly one chunk, between two rows
    f = tree._offsets['f.weight']
    assert [f, 1024] in chunks and sum(1 for a, c in chunks if f <= a < tree._offsets['s.mlp_gamma.weight']) > 9      # longer than a chunk
    assert chunks[-1][0] + chunks[-1][1] == tree.flat.numel() and chunks[-1][0] >= tree._offsets['s.mlp_gamma.bias']  # a plain tail
