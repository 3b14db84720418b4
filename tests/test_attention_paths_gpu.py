"""The attention kernels of csrc/attention.hip at the layouts and in the variants the engine runs, against an fp64 reference
of the same operation on the same fp16-rounded inputs (attn_cases.ref_attention).

A. Row strides and column offsets through ops.attention_strided: a packed [B, L, 3C] QKV buffer (UNet self-attention, CLIP
   with the causal mask), K / V at column offsets inside a wider buffer (cross-attention), ldk != ldv, an output with
   ldo = C + 4 at a pointer that is 8- but not 16-byte aligned.  B = 2: the batch term of every base pointer takes part.  The
   unused columns hold 1000, the output allocation a sentinel, and contiguous copies through ops.attention must give the same
   bits (the dispatch depends on (B, heads, lq, lk, d, causal) only and the arithmetic order not on strides).
B. The classic online softmax (d = 64 / 160: running maximum, wave-uniform "skip the rescale" vote, alpha on O and l) on
   planted rows whose maximum jumps at a late tile, inside a ragged last tile, sits near -300 or spreads over +-60.
C. Two query tiles per wave (SDOD_ATTN_QT=2 forces them at small shapes; =1 the one-tile kernel on the same data) with a
   ragged lq, with waves that own no row, and with the causal mask; and three shapes that take them by themselves (lq >= 2048).
D. The scale argument: 0.05 and 0.3 against fp64 with the same scale; zero, negative and non-finite scales are errors.
E. sdod_xattn_fold_f16: W1, s1, t1 and W2 each against fp64, at L = 1, 40, 77 and 80, with K / V at column offsets in a wider
   buffer and row strides above C on wq / wo; the padding slots j >= L exactly (zero rows / columns, s1 = 0, t1 = -30000).

Tolerances are the attention kernel's own (attn_cases.check): rel-L2 <= 3e-3 and max-abs <= 2e-2 * max|ref| + 1e-3, on the
whole output and again on the planted rows alone.  A CPU model of the non-deferred branch (tile-wise online softmax, fp32
scores, P rounded to fp16, fp32 O, fp16 output) on the planted inputs of B gives rel-L2 1.1e-4 .. 1.9e-4 and max-abs / max|ref|
<= 3.5e-4: a correct kernel keeps more than 10x margin.  The fold's W1 / W2 are fp16 roundings of fp32 sums and use the Linear
kernels' check (rel-L2 <= 2e-3); s1 / t1 are fp32 fma chains of d terms and one multiply, bounded per element by
d * 2^-23 * alpha * sum_k |K_k s_k|.

Environment variables set (and removed again) by these tests: SDOD_ATTN_QT (1 / 2: query tiles per wave, read by
sdod_attention_f16 on every call) and SDOD_ATTN_NO_TR (scalar LDS reads instead of ds_read_b64_tr_b16)."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from attn_cases import LOG2E, build, check, dev, ref_attention

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A   # an fp16 bit pattern (203.25) no output of these cases comes near
FILLER = 1000.0     # large and finite: what the columns hold that no kernel may read


@contextlib.contextmanager
def environ(**kv):
    for name, val in kv.items():
        os.environ[name] = val
    try:
        yield
    finally:
        for name in kv:
            os.environ.pop(name, None)


@functools.lru_cache(maxsize=None)
def case(b, heads, lq, lk, d, causal=False, seed=0, scale=None):
    """(q, k, v, planted rows, fp64 reference) of one shape: built once, shared by the tests that run it, never written"""
    q, k, v, rows = build(b, heads, lq, lk, d, seed, scale)
    return q, k, v, rows, ref_attention(q, k, v, heads, causal, scale)


def run_planted(b, heads, lq, lk, d, causal=False, seed=0, scale=None, tag=''):
    from sdod.amd import ops
    q, k, v, rows, ref = case(b, heads, lq, lk, d, causal, seed, scale)
    dv = dev()
    out = ops.attention(q.to(dv), k.to(dv), v.to(dv), heads, scale=scale, causal=causal)
    torch.cuda.synchronize()
    out = out.cpu()
    tag = f'{tag} b{b} h{heads} {lq}x{lk} d{d} causal{causal} scale{scale}'
    check(out, ref, name=tag)
    check(out[:, rows], ref[:, rows], name=tag + ' planted rows')
    return out


# ------------------------------------------------------------------------------------------------ A. strides and offsets
def ptr(t, halves=0):
    return ctypes.c_void_p(t.data_ptr() + 2 * halves)


def widen(x, width, col):
    """x [B, L, C] inside a [B, L, width] buffer of FILLER at column offset col"""
    buf = torch.full(x.shape[:2] + (width,), FILLER, dtype=torch.float16)
    buf[:, :, col:col + x.shape[2]] = x
    return buf


def run_strided(layout, d, lk, causal=False):
    from sdod.amd import ops
    b, heads, lq = 2, 2, 100
    c = heads * d
    q, k, v, rows, ref = case(b, heads, lq, lk, d, causal, seed=10)
    dv = dev()
    if layout == 'packed':       # graphs.hip: self-attention / CLIP on the QKV projection's output
        assert lq == lk
        qkv = torch.cat([q, k, v], -1).to(dv)
        keep = (qkv,)
        qp, kp, vp, ldq, ldk, ldv = ptr(qkv), ptr(qkv, c), ptr(qkv, 2 * c), 3 * c, 3 * c, 3 * c
        off, ldo = 0, c
    elif layout == 'cross':      # graphs.hip: K | V of one layer inside the all-layers buffer
        w = 2 * c + 24
        kv = widen(k, w, 8)
        kv[:, :, c + 16:2 * c + 16] = v
        qd, kv = q.to(dv), kv.to(dv)
        keep = (qd, kv)
        qp, kp, vp, ldq, ldk, ldv = ptr(qd), ptr(kv, 8), ptr(kv, c + 16), c, w, w
        off, ldo = 4, c + 4
    else:                        # K and V in buffers of different widths
        qd, kb, vb = q.to(dv), widen(k, c + 8, 0).to(dv), widen(v, c + 40, 16).to(dv)
        keep = (qd, kb, vb)
        qp, kp, vp, ldq, ldk, ldv = ptr(qd), ptr(kb), ptr(vb, 16), c, c + 8, c + 40
        off, ldo = 4, c + 4
    n = b * lq * ldo
    alloc = torch.full((off + n + 64,), SENTINEL, dtype=torch.int16, device=dv)
    assert alloc.data_ptr() % 16 == 0
    ops.attention_strided(qp, kp, vp, ptr(alloc, off), b, heads, lq, lk, d, ldq, ldk, ldv, ldo, d ** -0.5, causal=causal)
    torch.cuda.synchronize()
    del keep
    got = alloc.cpu()
    tag = f'{layout} b{b} h{heads} {lq}x{lk} d{d} causal{causal}'
    body = got[off:off + n].view(b * lq, ldo)
    assert bool((got[:off] == SENTINEL).all()) and bool((got[off + n:] == SENTINEL).all()), f'{tag}: wrote outside the rows'
    assert bool((body[:, c:] == SENTINEL).all()), f'{tag}: wrote past column C of a row'
    out = body[:, :c].contiguous().view(torch.float16).view(b, lq, c)
    check(out, ref, name=tag)
    check(out[:, rows], ref[:, rows], name=tag + ' planted rows')
    same = ops.attention(q.to(dv), k.to(dv), v.to(dv), heads, causal=causal)
    torch.cuda.synchronize()
    assert torch.equal(same.cpu().view(torch.int16), out.view(torch.int16)), f'{tag}: differs from the contiguous call'


@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_packed_qkv_buffer(d):
    run_strided('packed', d, 100)


def test_packed_qkv_buffer_causal():
    """CLIP's form: d = 64, packed, causal"""
    run_strided('packed', 64, 100, causal=True)


@pytest.mark.parametrize('lk', [100, 77, 256])   # (256 at d = 80: the key split inside the workgroup)
@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_kv_at_column_offsets_of_a_wider_buffer(d, lk):
    run_strided('cross', d, lk)


@pytest.mark.parametrize('lk', [100, 77, 256])
@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_k_and_v_row_strides_differ(d, lk):
    run_strided('split', d, lk)


@pytest.mark.parametrize('what', ['ldq % 8', 'ldk < heads*d', 'ldo % 4', 'd = 48', 'q + 4 halves'])
def test_launcher_rejects_what_the_kernel_cannot_run(what):
    """an error, and nothing launched: the output keeps its sentinel (every buffer is large enough for what is asked)"""
    from sdod.amd import ops, _lib
    b, heads, lq, lk, d = 2, 2, 100, 100, 64
    c = heads * d
    dv = dev()
    q, k, v = (torch.zeros(b * lq * (c + 16) + 64, dtype=torch.float16, device=dv) for _ in range(3))
    out = torch.full((b * lq * (c + 16) + 64,), SENTINEL, dtype=torch.int16, device=dv)
    ldq = ldk = ldv = ldo = c
    qoff = 0
    if what == 'ldq % 8':
        ldq = c + 4
    elif what == 'ldk < heads*d':
        ldk = c - 8
    elif what == 'ldo % 4':
        ldo = c + 2
    elif what == 'd = 48':
        d = 48
        ldq = ldk = ldv = ldo = heads * d
    else:
        qoff = 4
    with pytest.raises(_lib.SdodError):
        ops.attention_strided(ptr(q, qoff), ptr(k), ptr(v), ptr(out), b, heads, lq, lk, d, ldq, ldk, ldv, ldo, d ** -0.5)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), f'{what}: the output was written'


# --------------------------------------------------------------------------- B. the non-deferred softmax on planted rows
@pytest.mark.parametrize('lk', [64, 65, 77, 1000])
@pytest.mark.parametrize('d', [64, 160])
def test_online_softmax_planted_rows(d, lk):
    run_planted(2, 2, 256, lk, d, seed=20)


@pytest.mark.parametrize('d', [64, 160])
def test_online_softmax_planted_rows_causal(d):
    run_planted(2, 2, 300, 300, d, causal=True, seed=21)


@pytest.mark.parametrize('d', [64, 160])
def test_online_softmax_planted_rows_scalar_lds(d):
    with environ(SDOD_ATTN_NO_TR='1'):
        run_planted(2, 2, 256, 333, d, seed=22, tag='no-tr')


# -------------------------------------------------------------------------------------- C. two query tiles per wave
@pytest.mark.parametrize('qt', ['2', '1'])
@pytest.mark.parametrize('lk', [77, 200])
@pytest.mark.parametrize('lq', [64, 129, 130, 200])   # 64: waves 2 and 3 own no row; 129: one row in the second workgroup
@pytest.mark.parametrize('d', [40, 64, 80])
def test_query_tiles_per_wave_ragged_lq(d, lq, lk, qt):
    with environ(SDOD_ATTN_QT=qt):
        run_planted(1, 2, lq, lk, d, seed=30, tag=f'qt{qt}')


@pytest.mark.parametrize('qt', ['2', '1'])
@pytest.mark.parametrize('l', [200, 300])
@pytest.mark.parametrize('d', [40, 64, 80])
def test_query_tiles_per_wave_causal(d, l, qt):
    """with two query tiles the wave's first row (the need_mask condition) and kend = q_block + 128 differ from the one-tile
    form: a first row taken too LARGE (the wave's last row, say) or kend = q_block + 64 leaves keys past the diagonal in and
    fails here.  One taken too small (wave * 16 for wave * 32) only sends tiles through the mask that need none, and the mask
    itself is exact per element -- the same bits, which no comparison of outputs can tell apart."""
    with environ(SDOD_ATTN_QT=qt):
        run_planted(1, 2, l, l, d, causal=True, seed=31, tag=f'qt{qt}')


@pytest.mark.parametrize('d,lq,lk', [(64, 2088, 2088), (64, 2304, 77), (40, 2088, 77)])
def test_two_query_tiles_natural_dispatch(d, lq, lk):
    """lq >= 2048 takes two query tiles by itself; 2088 = 16 full 128-row blocks + 40 rows"""
    assert 'SDOD_ATTN_QT' not in os.environ
    run_planted(1, 2, lq, lk, d, seed=32)


# ------------------------------------------------------------------------------------------------ D. the scale argument
@pytest.mark.parametrize('scale', [0.05, 0.3])
@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_custom_scale(d, scale):
    run_planted(2, 2, 128, 200, d, seed=40, scale=scale)


@pytest.mark.parametrize('scale', [0.0, -0.125, float('nan'), float('inf')])
@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_scale_must_be_positive_and_finite(d, scale):
    from sdod.amd import ops, _lib
    q, k, v, _, _ = case(2, 2, 128, 200, d, False, 40, 0.3)
    dv = dev()
    out = torch.full(q.shape, SENTINEL, dtype=torch.int16, device=dv).view(torch.float16)
    with pytest.raises(_lib.SdodError, match='scale'):
        ops.attention(q.to(dv), k.to(dv), v.to(dv), 2, scale=scale, out=out)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == SENTINEL).all()), 'the output was written'


# ------------------------------------------------------------------------------------------ E. xattn_fold against fp64
@pytest.mark.parametrize('L', [1, 40, 77, 80])
@pytest.mark.parametrize('heads,d', [(2, 40), (5, 64), (1, 80), (1, 160), (8, 160)])
def test_xattn_fold_against_fp64(heads, d, L):
    from sdod.amd import ops
    from test_kernels_gpu import check as check_linear
    n_img, c = 2, heads * d
    g = torch.Generator().manual_seed(1000 * heads + 10 * d + L)
    kk = torch.randn(n_img, L, c, generator=g).half()
    vv = torch.randn(n_img, L, c, generator=g).half()
    wq = (torch.randn(c, c, generator=g) / c ** 0.5).half()
    wo = (torch.randn(c, c, generator=g) / c ** 0.5).half()
    sq = torch.randn(c, generator=g); tq = torch.randn(c, generator=g)
    wide = (heads, d) in ((2, 40), (1, 160), (8, 160))      # row strides above C on wq / wo
    ldq, ldwo = (c + 8, c + 16) if wide else (c, c)
    ld_kv, k_off, v_off = 2 * c + 24, 8, c + 16
    kv = widen(kk, ld_kv, k_off)
    kv[:, :, v_off:v_off + c] = vv
    dv = dev()
    w1, s1, t1, w2 = ops.xattn_fold(kv.view(n_img * L, ld_kv).to(dv), k_off, v_off, n_img, L, widen(wq[None], ldq, 0)[0].to(dv),
                                    sq.to(dv), tq.to(dv), widen(wo[None], ldwo, 0)[0].to(dv), heads)
    torch.cuda.synchronize()
    w1 = w1.cpu().view(n_img, heads, 80, c); w2 = w2.cpu().view(n_img, c, heads, 80)
    s1 = s1.cpu().view(n_img, heads, 80); t1 = t1.cpu().view(n_img, heads, 80)
    tag = f'fold h{heads} d{d} L{L}'
    alpha = float(np.float32(d ** -0.5)) * LOG2E
    kh = kk.double().view(n_img, L, heads, d); vh = vv.double().view(n_img, L, heads, d)
    w1_ref = alpha * torch.einsum('ijhk,hkc->ihjc', kh, wq.double().view(heads, d, c))
    w2_ref = torch.einsum('chk,ijhk->ichj', wo.double().view(c, heads, d), vh)
    check_linear(w1[:, :, :L], w1_ref, name=tag + ' w1')
    check_linear(w2[..., :L], w2_ref, name=tag + ' w2')
    for got, vec, nm in ((s1, sq, 's1'), (t1, tq, 't1')):
        terms = kh * vec.double().view(heads, d)
        ref = alpha * terms.sum(-1).permute(0, 2, 1)
        bound = d * 2.0 ** -23 * alpha * terms.abs().sum(-1).permute(0, 2, 1)
        err = (got[..., :L].double() - ref).abs()
        worst = float((err / bound).max())
        assert torch.isfinite(got).all() and bool((err <= bound).all()), f'{tag} {nm}: error / bound {worst:.3f}'
    # the padding slots, exactly
    assert bool((w1[:, :, L:].contiguous().view(torch.int16) == 0).all()), f'{tag}: w1 padding rows'
    assert bool((w2[..., L:].contiguous().view(torch.int16) == 0).all()), f'{tag}: w2 padding columns'
    assert bool((s1[..., L:] == 0).all()) and bool((t1[..., L:] == -30000.0).all()), f'{tag}: s1 / t1 padding'
    assert not bool((t1[..., :L] == -30000.0).any()), f'{tag}: a valid slot carries the padding bias'
