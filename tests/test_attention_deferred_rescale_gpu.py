"""Fused attention at d = 40 / 80 (the deferred-shift softmax of csrc/attention.hip) against an fp64 reference, on inputs built
to take its rare branch.

At these head dims the QK^T MFMA returns s * scale * log2(e) - m with m the running shift, and m is only moved when a score of
the wave exceeds it by more than THR = 8 (log2 units).  Random data takes that branch essentially only at each group's first
tile, so every case here plants rows whose scores are prescribed exactly: row r's query is the unit vector of head dimension j,
so its scores are column j of K, which the test writes key by key.  Planted patterns: a jump past THR at tile 1, at a middle
tile, at the last full tile and inside a ragged last tile; a jump just below and just above THR; scores all near -300; scores
spread over +-60; several jumps in one row; a maximum at key 0 and nothing close to it later.  The remaining rows are random.
Tolerances are those of the attention kernel tests: rel-L2 <= 3e-3 and max-abs <= 2e-2 * max|ref| + 1e-3, on the whole
output and again on the planted rows alone."""
import os

import pytest
import torch

from attn_cases import build, check, dev, ref_attention

pytestmark = pytest.mark.gpu

def run(b, heads, lq, lk, d, causal=False, seed=0):
    from sdod.amd import ops
    q, k, v, rows = build(b, heads, lq, lk, d, seed)
    ref = ref_attention(q, k, v, heads, causal)
    dv = dev()
    out = ops.attention(q.to(dv), k.to(dv), v.to(dv), heads, causal=causal)
    torch.cuda.synchronize()
    out = out.cpu()
    tag = f'b{b} h{heads} {lq}x{lk} d{d} causal{causal}'
    check(out, ref, name=tag)
    check(out[:, rows], ref[:, rows], name=tag + ' planted rows')


@pytest.mark.parametrize('d', [40, 80])
@pytest.mark.parametrize('lk', [64, 65, 77, 4096])
def test_forced_rescale(d, lk):
    run(2, 2, 512, lk, d)


@pytest.mark.parametrize('d', [40, 80])
def test_forced_rescale_two_query_tiles(d):
    """lq >= 2048: two query tiles per wave, each with its own shift"""
    run(1, 2, 2048, 1000, d, seed=1)


@pytest.mark.parametrize('lk', [512, 320, 300])
def test_forced_rescale_d80_key_split(lk):
    """d = 80 on a small grid takes the key split inside the workgroup (two groups, merged through LDS): an even and an odd
    number of key tiles, and a ragged odd one; planted jumps fall into both groups' tiles"""
    run(1, 2, 256, lk, 80, seed=2)


@pytest.mark.parametrize('d', [40, 80])
def test_forced_rescale_causal(d):
    run(1, 2, 300, 300, d, causal=True, seed=3)


@pytest.mark.parametrize('d', [40, 80])
def test_forced_rescale_scalar_lds(d):
    """the same patterns through the scalar-LDS variant of the kernel (SDOD_ATTN_NO_TR)"""
    os.environ['SDOD_ATTN_NO_TR'] = '1'
    try:
        run(1, 2, 256, 333, d, seed=4)
    finally:
        os.environ.pop('SDOD_ATTN_NO_TR', None)
