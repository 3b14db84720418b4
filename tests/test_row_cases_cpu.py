"""The references and bounds of tests/row_cases.py, checked without a GPU: fp32 restatements of the kernels' arithmetic meet every
bound test_row_kernels_gpu.py applies, with room -- so a failure there means the kernel, not the test -- and the data can see what it
is meant to see: the LayerNorm fold WITHOUT eps misses the tolerance on the eps-sensitive kinds, and the peak sweep of the softmax
rows reaches every wave, chunk index, reduction step and element of a lane."""
import pytest
import torch

import row_cases as rc

M, N = 200, 160


@pytest.mark.parametrize('k', [64, 320, 1280])
def test_fold_restatement_meets_the_tolerance_and_sees_eps(k):
    gamma, beta = rc.ln_params(k); w, bias = rc.linear_params(N, k)
    for kind, eps in rc.LN_CASES:
        x = rc.ln_rows(kind, M, k)
        ref = rc.fold_ref(x, w, gamma, beta, bias, eps)
        r = rc.rel_l2(rc.fold_f32(x, w, gamma, beta, bias, eps), ref)
        print(f'K {k} {kind} eps {eps}: fold in fp32 rel-L2 {r:.2e}')
        assert r <= 1e-3, (k, kind, eps, r)                  # a third of FOLD_TOL
    for kind, eps in rc.EPS_VISIBLE:
        x = rc.ln_rows(kind, M, k)
        ref = rc.fold_ref(x, w, gamma, beta, bias, eps)
        r = rc.rel_l2(rc.fold_f32(x, w, gamma, beta, bias, eps, use_eps=False), ref)
        print(f'K {k} {kind} eps {eps}: WITHOUT eps rel-L2 {r:.2e}')
        assert r > rc.FOLD_TOL, (k, kind, eps, r)


def test_ln_kinds_are_what_they_say():
    k = 320
    for kind, want in (('offset', 100.0), ('nearconst', 100.0)):
        x = rc.ln_rows(kind, M, k).double()
        ratio = x.mean(1).abs() / x.std(1, unbiased=False)
        assert float((ratio / want - 1).abs().max()) < 0.15, (kind, float(ratio.min()), float(ratio.max()))
    assert torch.equal(rc.ln_rows('const', 3, 64), torch.full((3, 64), 3.0).half())
    v = rc.ln_rows('epsdom', M, k).double().var(1, unbiased=False)
    assert 0.5e-5 < float(v.min()) and float(v.max()) < 2e-5           # variance ~ eps
    assert float(rc.ln_rows('pilot', 4, 64)[:, 0].min()) == 1000.0
    x = rc.ln_rows('rowmix', 168, k).double()
    stats = {(round(float(a), 2), round(float(b), 3)) for a, b in zip(x.mean(1), x.std(1))}
    assert len(stats) == 168                                           # no two rows of a period share their statistics
    # const rows through the reference: exactly beta (LayerNorm), exactly t = beta . w^T + bias (fold)
    gamma, beta = rc.ln_params(k); w, bias = rc.linear_params(N, k)
    x = rc.ln_rows('const', 5, k)
    assert torch.equal(rc.ln_ref(x, gamma, beta), beta.double().expand(5, k))
    assert torch.allclose(rc.fold_ref(x, w, gamma, beta, bias), (w.double() @ beta.double() + bias.double()).expand(5, N), rtol=0, atol=1e-12)


@pytest.mark.parametrize('n', rc.SOFTMAX_NS)
def test_softmax_peak_sweep_covers_the_kernel(n):
    cols = rc.softmax_peak_columns(n)
    pos = [rc.softmax_position(n, c) for c in cols]
    cp = n // 8
    threads = min(cp, 256)
    assert {p[0] for p in pos} == set(range((threads + 63) // 64))     # every wave that holds a column
    assert {p[1] for p in pos} == set(range((cp + 255) // 256))        # every chunk index
    assert {p[3] for p in pos} == set(range(8))                        # every element of a 16-byte lane
    if cp >= 256:
        assert {p[2] for p in pos} >= set(rc.PEAK_LANES)
    assert 0 in cols and n - 1 in cols and len(cols) <= 64
    for kind in ('peak', 'twin'):
        x = rc.softmax_rows_kind(kind, n).double()
        assert x.shape[0] == len(cols)
        assert all(float(x[r, c]) == 300.0 for r, c in enumerate(cols))
        assert float(x.max(1).values.min() - x.median(1).values.max()) > 590   # spread beyond the fp32 exponent range (89 natural units)
        assert int((x == 300.0).sum()) == len(cols) * (2 if kind == 'twin' else 1)


@pytest.mark.parametrize('n', rc.SOFTMAX_NS)
def test_softmax_restatement_meets_close16(n):
    """zero violations at r = 2^-18, a quarter of the GPU test's 2^-16; the subnormal kinds really are subnormal"""
    for kind in rc.SOFTMAX_KINDS:
        x = rc.softmax_rows_kind(kind, n)
        ref = rc.softmax_ref(x)
        out = rc.softmax_f32(x)
        worst = rc.check_close16(out, ref, 2.0 ** -18, name=f'softmax in fp32 N {n} {kind}')
        sums = out.double().sum(1)
        assert float((sums - 1).abs().max()) <= rc.row_sum_bound(n), (n, kind)
        print(f'N {n} {kind}: worst |err| / bound {worst:.3f}')
        if kind in ('gauss3', 'gauss10') and n >= 2048:
            sub = (ref < 2.0 ** -14) & (ref > 2.0 ** -25)
            print(f'N {n} {kind}: {float(sub.double().mean()):.3f} of the references are fp16 subnormals')
            # (scale 10: a few large entries take the row, most of the rest is below half a subnormal and rounds to zero)
            assert float(sub.double().mean()) > (0.5 if kind == 'gauss3' else 0.005), (n, kind, float(sub.double().mean()))
            flushed = torch.where(out.double() < 2.0 ** -14, torch.zeros_like(ref), out.double())
            assert float(rc.close16_excess(flushed, ref, rc.SOFTMAX_R).max()) > 100        # a flush to zero fails by orders of magnitude


def test_close16_and_ulp16():
    v = torch.tensor([1.0, 1.5, 2.0, 0.999, 2.0 ** -14, 2.0 ** -15, 0.0, 65504.0, 3e-8], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 32.0, 2.0 ** -24], dtype=torch.float64)
    assert torch.equal(rc.ulp16(v), want)
    x = rc.all_finite_f16().double()
    nxt = torch.nextafter(x.half(), torch.tensor(float('inf')).half()).double()
    ok = torch.isfinite(nxt) & (x >= 0)
    assert torch.equal((nxt - x)[ok], rc.ulp16(x)[ok])                  # against the format itself, every non-negative value
    ref = torch.tensor([1.0 + 2.0 ** -12, 0.3, 1e-6], dtype=torch.float64)
    assert float(rc.close16_excess(ref.half(), ref, 0.0).max()) <= 1     # a correctly rounded value is always inside
    assert float(rc.close16_excess(torch.tensor([1.0 + 2.0 ** -10]).half(), ref[:1], 2.0 ** -16)[0]) > 1
    assert float(rc.close16_excess(torch.tensor([0.0]).half(), ref[2:], 2.0 ** -16)[0]) > 10   # 1e-6 flushed to zero


def test_epilogue_operands_are_exact():
    for n, k in ((160, 192), (320, 320)):
        for kind in rc.EPI_KINDS:
            s = rc.epilogue_scores(kind, 128, n)
            a, w, bias = rc.epilogue_operands(s, k)
            y = a.float() @ w.float().t() + bias                        # fp32, one exact term per element
            want = s.clone(); want.view(128, -1, 80)[:, :, 77:] = -30000.0
            assert torch.equal(y.double(), want)
            ref = rc.epilogue_ref(s)
            assert float(ref.view(128, -1, 80)[:, :, 77:].abs().max()) == 0
            assert float((ref.view(128, -1, 80).sum(-1) - 1).abs().max()) < 1e-12
            if kind in ('peak', 'twin'):
                v = s.view(128, -1, 80)[:, :, :77]
                assert {int(c) for c in v.argmax(-1).flatten()} == set(range(77)) or kind == 'twin'
                assert float(v.max(-1).values.min()) == 320.0 and float(v.median(-1).values.max()) < -300   # > 128 log2 units of spread
            # the kernel's arithmetic in fp32 (exp2 of the difference, fp32 sum, reciprocal) meets the bound at a quarter of r
            g = y.view(128, -1, 80)
            e = torch.exp2(g - g.max(-1, keepdim=True).values)
            out = (e * (1.0 / e.sum(-1, keepdim=True, dtype=torch.float32))).half().view(128, n)
            rc.check_close16(out, ref, 2.0 ** -18, name=f'epilogue softmax in fp32 N {n} {kind}')


def test_gelu_polynomial_holds_its_stated_error():
    """common.h: |error| <= 5.4e-7 over all x -- in emulated fp32 over every finite fp16 input, beyond the final fma's own rounding"""
    x = rc.all_finite_f16()
    ref = rc.gelu64(x)
    k = rc.gelu_poly_f32(x)
    over = (k - ref).abs() - 2.0 ** -23 * ref.abs()
    i = int(torch.argmax(over))
    print(f'gelu polynomial in fp32: worst |error| beyond fp32 rounding {float(over[i]):.3e} at x = {float(x[i])}')
    assert float(over[i]) <= 5.4e-7
    rc.check_close16(k.half(), ref, rc.GELU_R, 5.4e-7, name='gelu polynomial in fp32')
    # one coefficient off by 1e-5 is seen
    bad = ref + 1.5e-6 * (x.double().abs() < 3)
    assert float(rc.close16_excess(bad.half(), ref, rc.GELU_R, rc.GELU_A).max()) > 1


@pytest.mark.parametrize('name,c', [('silu', 1.0), ('quick_gelu', 1.702)])
def test_silu_restatement_is_within_half_an_ulp(name, c):
    x = rc.all_finite_f16()
    ref = rc.ACT_REF[name](x)
    if name == 'quick_gelu':       # the kernel's constant is the fp32 1.702f; the reference keeps the decimal one
        assert abs(float(torch.tensor(1.702, dtype=torch.float32)) - 1.702) < 1e-7
    k = rc.silu_f32(x, c)
    out = k.half()
    ulps = ((out.double() - ref).abs() / rc.ulp16(torch.maximum(out.double().abs(), ref.abs())))
    print(f'{name} in fp32: worst {float(ulps.max()):.5f} ulp16')
    assert torch.isfinite(out).all()
    rc.check_close16(out, ref, rc.ACT_BOUND[name][0] / 2, name=f'{name} in fp32')
