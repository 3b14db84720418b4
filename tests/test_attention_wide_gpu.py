"""ops.attention_wide (sdod_attention_wide_f16, d = 256 / 512: the VAE's middle attention) against softmax(scale q k^T) v in
float64 on the same fp16-rounded inputs, with the attention tests' tolerances (attn_cases.check: rel-L2 <= 3e-3, max-abs <=
2e-2 max|ref|).  Batch 2 throughout.  Shapes: one tile; one tile + 8 ragged keys and queries; several tiles, both ragged; 17 key
tiles and 17 query blocks, which the launcher splits over the keys (the one-launch form runs on the same data too); lq != lk."""
import pytest
import torch

from attn_cases import LOG2E, check, dev, ref_attention

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (72, 72), (200, 200), (1088, 1088), (64, 200)]


def make(d, lq, lk, plant):
    """plant = 'late' / 'first': rows 3 and lq - 1 of both images get a key in the last / first tile whose score exceeds every other
    key's by >= 30 in log2 units (query = unit vector of column 0, that column of K = noise in [-1, 1] and one entry of
    34 / (scale log2 e)): the online rescale has to drop everything accumulated before it / survive every tile after it"""
    gen = torch.Generator().manual_seed(7 * d + 3 * lq + lk)
    q, k, v = (torch.randn(2, n, d, generator=gen) for n in (lq, lk, lk))
    if plant:
        key = lk - 3 if plant == 'late' else 5
        k[:, :, 0] = torch.rand(2, lk, generator=gen) * 2 - 1
        k[:, key, 0] = 34.0 / (d ** -0.5 * LOG2E)
        for row in (3, lq - 1):
            q[:, row] = 0.0
            q[:, row, 0] = 1.0
    return q.half(), k.half(), v.half()


@pytest.mark.parametrize('plant', [None, 'late', 'first'])
@pytest.mark.parametrize('lq,lk', SHAPES)
@pytest.mark.parametrize('d', [256, 512])
def test_attention_wide_vs_fp64(d, lq, lk, plant):
    from sdod.amd import ops
    q, k, v = make(d, lq, lk, plant)
    ref = ref_attention(q, k, v, 1, False)
    splits = ops.attention_wide_splits(2, lq, lk, d)
    assert (splits > 1) == (lk == 1088), splits                 # the key-split path runs at 1088, the one-launch path everywhere else
    if lq == lk and plant == 'late':
        # the graph's layout: q and k are the halves of one [B, L, 2d] buffer, out a view into wider rows
        qk = torch.cat([q, k], -1).to(dev())
        qd, kd = qk[:, :, :d], qk[:, :, d:]
        out = torch.zeros(2, lq, d + 64, dtype=torch.float16, device=dev())[:, :, 8:8 + d]
    else:
        qd, kd, out = q.to(dev()), k.to(dev()), None
    got = ops.attention_wide(qd, kd, v.to(dev()), out=out)
    check(got, ref, name=f'd{d} {lq}x{lk} {plant} splits{splits}')
    if splits > 1:
        check(ops.attention_wide(qd, kd, v.to(dev()), split=False), ref, name=f'd{d} {lq}x{lk} {plant} one launch')
