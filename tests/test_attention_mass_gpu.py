"""sdod_attention_mass_f16 (Self-Attention Guidance) against an fp64 torch computation on the same fp16 inputs.

Every case: batch 2, q and k column offsets into packed [rows][3 * heads * d] rows.  Asserted: the mass (not the thresholded mask)
within BOUND relative to max(mass_ref, lq / lk) -- lq / lk is the mean mass, so keys that collect next to nothing are measured against
the typical key; sum_j mass = lq within BOUND * lq; two calls bit-equal.  BOUND is four times the largest error measured over this grid
on an MI355X (MEASURED, DESIGN.md 6s: fp32 score accumulation, hardware exp2, one division per query; fp16 never enters)."""
import functools

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu

MEASURED = 2.52e-7          # largest error over the grid and the two extra cases, MI355X (the planted-row case)
BOUND = 4 * MEASURED
B = 2


@functools.lru_cache(maxsize=None)
def case(d, heads, lq, lk, planted=False):
    gen = torch.Generator().manual_seed(7 * d + 100 * heads + lq + 3 * lk)
    c = heads * d
    qbuf, kbuf = (torch.randn(B, l, 3 * c, generator=gen).half() for l in (lq, lk))
    if planted:         # query row 3 scores about 60 above every other row, against every key: the shift decides whether exp overflows
        kbuf[:, :, c::d][:, :, :heads] = 1.0
        qbuf[:, 3, 0:c:d] = 60.0 * d ** 0.5
    q, k = qbuf[:, :, :c].double(), kbuf[:, :, c:2 * c].double()
    qh, kh = (t.reshape(B, -1, heads, d).transpose(1, 2) for t in (q, k))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, dim=-1)
    return qbuf.to(AC.dev()), kbuf.to(AC.dev()), p.sum(2).mean(1)


GRID = [(d, h, l, l, False) for d in (40, 64, 80, 160) for h in (5, 8) for l in (1, 64, 80, 144)] + [(40, 8, 64, 77, False), (80, 8, 80, 80, True)]


@pytest.mark.parametrize('d,heads,lq,lk,planted', GRID)
def test_mass(d, heads, lq, lk, planted):
    from sdod.amd import ops
    qbuf, kbuf, ref = case(d, heads, lq, lk, planted)
    c = heads * d
    out = ops.attention_mass(qbuf[:, :, :c], kbuf[:, :, c:2 * c], heads)
    again = ops.attention_mass(qbuf[:, :, :c], kbuf[:, :, c:2 * c], heads)
    assert torch.equal(out, again)
    got = out.double().cpu()
    err = float(((got - ref).abs() / ref.clamp_min(lq / lk)).max())
    err_sum = float((got.sum(1) - lq).abs().max() / lq)
    print(f'attention_mass d{d} h{heads} lq{lq} lk{lk} planted={planted}: err {err:.3e}, sum {err_sum:.3e}, largest mass {float(ref.max()):.3f}')
    assert torch.isfinite(got).all() and err <= BOUND and err_sum <= BOUND, (err, err_sum)


def test_refusals():
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    dev = AC.dev()
    for shape_q, shape_k, heads, cols in (((B, 8, 96), (B, 8, 96), 2, 96),          # d = 48
                                           ((B, 8, 84), (B, 8, 84), 2, 80),          # row stride 84: no multiple of 8
                                           ((B, 8, 80), (B, 4097, 80), 2, 80)):      # lk > 4096
        q, k = (torch.zeros(s, dtype=torch.float16, device=dev)[:, :, :cols] for s in (shape_q, shape_k))
        with pytest.raises(SdodError) as e:
            ops.attention_mass(q, k, heads)
        assert e.value.code == 2
