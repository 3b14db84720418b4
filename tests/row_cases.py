"""Shared pieces of the row-kernel tests (test_row_kernels_gpu.py, test_row_cases_cpu.py): the kernels that reduce along a row --
the stand-alone LayerNorm, the LayerNorm statistics gathered inside the GEMMs (the "fold"), softmax_rows, the 80-column softmax
of the score GEMM's epilogue -- and the fp32 activation functions they share, against fp64 on data that can see their mistakes.

LayerNorm rows   ln_rows(kind, m, k): fp16 rows of the kinds in LN_KINDS.  `nearconst`, `epsdom` (and `normal` at eps = 0.5) are
                 the rows on which eps decides the result; `const` rows normalise to exactly the bias (variance 0: eps alone
                 keeps rstd finite); `offset` and `nearconst` sit at |row mean| / row std = 100, the edge of the fold's contract
                 (one-pass fp32 variance, include/sdod_hip.h at `ln`); `pilot` has one element of 1000 per row; `rowmix` gives
                 every row its own scale and mean, so that statistics stored at the wrong row show.
                 fold_f32() restates the fold's arithmetic in fp32; test_row_cases_cpu.py proves with it that the arithmetic
                 meets the GPU test's tolerance with room, and that the same arithmetic without eps does not.

Softmax rows     softmax_peak_columns(n) lists the columns a row's peak must visit so that every step of the kernel's maximum
                 reduction is the only path of some peak to the result; softmax_rows_kind() builds rows whose spread exceeds
                 the exponent range (a lost maximum overflows: inf / NaN, not a small error), flat rows, rows on a -60000 base
                 and Gaussian rows whose outputs are mostly fp16 subnormals.

close16          the bound for an fp16 output of an fp32 computation, against fp64:
                     |out - ref| <= ulp16(max(|out|, |ref|)) / 2 + r |ref| + a
                 (ulp16: the fp16 spacing, 2^-24 below 2^-14).  r and a are the fp32 chain's own error, stated where they are
                 defined below; test_row_cases_cpu.py checks fp32 restatements of the kernels against tighter values."""
import math

import torch

LN_KINDS = ('normal', 'offset', 'nearconst', 'const', 'epsdom', 'pilot', 'rowmix')
LN_CASES = [(k, 1e-5) for k in LN_KINDS] + [('normal', 0.5)]     # (kind, eps)
EPS_VISIBLE = [('nearconst', 1e-5), ('epsdom', 1e-5), ('normal', 0.5)]   # the cases on which dropping eps must exceed the tolerance
FOLD_TOL = 3e-3            # the suite's tolerance for the LayerNorm fold (test_kernels_gpu.py)
LN_TOL = 2e-3              # ... and for the stand-alone kernels

# close16 parameters (r, a).
# softmax: the fp32 chain is the argument scaling (<= 17 * 2^-24 where the result is not below half a subnormal), one ulp each
#   for the hardware exponential, the reciprocal and the product, a few for the sum: about 2e-6.  2^-16 leaves ~8x and is 1/32 of
#   an fp16 ulp.
SOFTMAX_R = 2.0 ** -16
# GELU: common.h states |error| <= 5.4e-7 for the polynomial; the hardware exponential adds one ulp on |x| Q <= 0.17 (2e-8);
#   rounded up.  r: the final fma's rounding.
GELU_R, GELU_A = 2.0 ** -23, 6e-7
# SiLU / quick-GELU: x * rcp(1 + exp(.)): relative errors only.
SILU_R = 2.0 ** -20


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------------------- LayerNorm
def ln_rows(kind, m, k, seed=0):
    """fp16 [m][k] rows of one of LN_KINDS"""
    g = _gen(1000 + seed)
    z = torch.randn(m, k, generator=g)
    if kind == 'normal':
        x = z
    elif kind == 'offset':
        x = 100 + z
    elif kind == 'nearconst':
        x = 3 + 0.03 * z
    elif kind == 'const':
        x = torch.full((m, k), 3.0)
    elif kind == 'epsdom':
        x = 3e-3 * z
    elif kind == 'pilot':
        x = z.clone()
        x[:, 0] = 1000.0
    elif kind == 'rowmix':
        r = torch.arange(m)
        scale = torch.pow(2.0, (r % 8 - 4).float())[:, None]
        x = scale * (z + (r % 21 - 10).float()[:, None])
    else:
        raise ValueError(kind)
    return x.half()


def ln_params(k, seed=0):
    """(gamma, beta) fp32 [k]"""
    g = _gen(2000 + seed)
    return 1 + 0.2 * torch.randn(k, generator=g), 0.3 * torch.randn(k, generator=g)


def linear_params(n, k, seed=0):
    """(w fp16 [n][k], bias fp32 [n])"""
    g = _gen(3000 + seed)
    return (torch.randn(n, k, generator=g) * k ** -0.5).half(), torch.randn(n, generator=g)


def ln_ref(x, gamma=None, beta=None, eps=1e-5):
    """fp64 LayerNorm of the fp16 rows x (two-pass, biased variance)"""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        y = y * gamma.double()
    if beta is not None:
        y = y + beta.double()
    return y


def fold_ref(x, w, gamma, beta, bias, eps=1e-5):
    """fp64 LayerNorm -> Linear on the fp16 x and the UNFOLDED fp16 w"""
    return ln_ref(x, gamma, beta, eps) @ w.double().t() + bias.double()


def gelu64(x):
    """x Phi(x) = x erfc(-x / sqrt 2) / 2 in fp64 (erfc keeps the negative tail's relative accuracy)"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def geglu_ref(y):
    """fp64 GEGLU of [value | gate] columns"""
    h = y.shape[-1] // 2
    return y[..., :h] * gelu64(y[..., h:])


def fold_params_f32(w, gamma, beta, bias):
    """what sdod_ln_fold_f16 produces: (w' = fp16(w * gamma) with the product in fp32, s = sum_k w', t = sum_k beta w + bias)"""
    wf = (w.float() * gamma.float()).half()
    s = wf.float().sum(1, dtype=torch.float32)
    t = (w.float() * beta.float()).sum(1, dtype=torch.float32) + (bias.float() if bias is not None else 0)
    return wf, s, t


def _oct_sum(p):
    """the kernels' oct_sum on [m][8] fp32 partials: xor-1, xor-2, then the half-row mirror"""
    p = p + p[:, [1, 0, 3, 2, 5, 4, 7, 6]]
    p = p + p[:, [2, 3, 0, 1, 6, 7, 4, 5]]
    p = p + p[:, [7, 6, 5, 4, 3, 2, 1, 0]]
    return p[:, 0]


def fold_stats_f32(x, eps, use_eps=True):
    """(mean, rstd) fp32 as the GEMMs gather them: a lane owns 8 consecutive columns of every 64-column slab and adds x and x^2
    one after the other in fp32; the 8 lanes of a row are summed by oct_sum; var = a2 / K - mean^2, clamped at 0"""
    m, k = x.shape
    assert k % 64 == 0
    xf = x.float().view(m, k // 64, 8, 8)
    a1 = torch.zeros(m, 8); a2 = torch.zeros(m, 8)
    for kt in range(k // 64):
        for e in range(8):
            v = xf[:, kt, :, e]
            a1 = a1 + v
            a2 = a2 + v * v
    a1 = _oct_sum(a1); a2 = _oct_sum(a2)
    kf = torch.tensor(float(k))
    mean = a1 / kf
    var = (a2 / kf - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + eps) if use_eps else torch.rsqrt(var)
    return mean, rstd


def fold_f32(x, w, gamma, beta, bias, eps=1e-5, use_eps=True):
    """the fold in fp32, rounded to fp16 as the kernel's store does: rstd * (acc - mean * s) + t on fp16-rounded folded weights"""
    wf, s, t = fold_params_f32(w, gamma, beta, bias)
    mean, rstd = fold_stats_f32(x, eps, use_eps)
    acc = x.float() @ wf.float().t()
    y = rstd[:, None] * (acc - mean[:, None] * s[None]) + t[None]
    return y.half()


def rel_l2(out, ref):
    out = out.detach().double().cpu().flatten(); ref = ref.detach().double().cpu().flatten()
    return float((out - ref).norm() / (ref.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------------------ close16
def ulp16(v):
    """the fp16 spacing at |v| (fp64 tensor): 2^(floor(log2 |v|) - 10), 2^-24 below 2^-14"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -14))        # |v| = m 2^e with m in [0.5, 1)
    return torch.pow(2.0, (e - 11).double())


def close16_excess(out, ref, r, a=0.0):
    """|out - ref| / bound, elementwise (fp64); <= 1 where the bound holds.  `a` may be a tensor broadcast against ref."""
    out = out.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    bound = 0.5 * ulp16(torch.maximum(out.abs(), ref.abs())) + r * ref.abs() + a
    return (out - ref).abs() / bound


def check_close16(out, ref, r, a=0.0, name=''):
    out = out.detach().cpu()
    assert torch.isfinite(out).all(), f'{name}: {int((~torch.isfinite(out)).sum())} non-finite outputs'
    ex = close16_excess(out, ref, r, a)
    bad = (ex > 1).nonzero()
    if bad.numel():
        i = tuple(bad[int(torch.argmax(ex[ex > 1]))].tolist())
        raise AssertionError(f'{name}: {bad.shape[0]} of {ex.numel()} elements outside the bound, worst {float(ex.max()):.3g}x at {i}: '
                             f'{float(out[i])!r} vs {float(ref.double().cpu()[i])!r}')
    return float(ex.max())


# ------------------------------------------------------------------------------------------------------------ softmax
SOFTMAX_NS = (8, 2056, 8192, 8200, 16384)
SOFTMAX_KINDS = ('peak', 'twin', 'flat', 'base', 'gauss3', 'gauss10')
# lanes of a wave such that every step of wave_max is the only path of one of them to lane 0 (which publishes the wave's
# maximum): the xor-1, xor-2, half-row-mirror and row-mirror steps lose lanes 1, 2, 4 and 8, the two row swaps lanes 16 and 32
PEAK_LANES = (0, 1, 2, 4, 8, 16, 31, 32, 63)


def softmax_position(n, col):
    """(wave, chunk index i, lane, element e) of softmax_rows_kernel that holds column `col`: thread t = 64 wave + lane keeps the
    16-byte chunks t + 256 i"""
    ch, e = divmod(col, 8)
    i, t = divmod(ch, 256)
    return t // 64, i, t % 64, e


def softmax_peak_columns(n):
    """columns for the peak sweep of an n-column row: every wave, every chunk index, the lanes of PEAK_LANES and every element of
    a 16-byte lane, as far as the row has them; the first and the last column always"""
    cp = n // 8
    nch = (cp + 255) // 256
    want = [(0, 0, 0, e) for e in range(8)]
    want += [(idx % 4, 0, lane, (3 * idx) % 8) for idx, lane in enumerate(PEAK_LANES)]
    want += [(w, i, PEAK_LANES[(i + w) % len(PEAK_LANES)], (4 * i + w + 5) % 8) for i in range(nch) for w in range(4)]
    cols = [0, n - 1, (cp - 1) * 8]
    for w, i, lane, e in want:
        col = ((64 * w + lane) + 256 * i) * 8 + e
        if col < n:
            cols.append(col)
    cols = sorted(set(cols))
    assert len(cols) <= 64
    return cols


def softmax_rows_kind(kind, n, seed=0):
    """fp16 [m][n] scores: 'peak' one entry at +300 over a -300 + N(0, 1) background, once per column of softmax_peak_columns;
    'twin' the same with a second, equal peak half a row away; 'flat' all -7; 'base' -60000 + 4 N(0, 1); 'gauss3' / 'gauss10'"""
    g = _gen(4000 + seed + n)
    if kind in ('peak', 'twin'):
        cols = softmax_peak_columns(n)
        x = torch.randn(len(cols), n, generator=g) - 300.0
        for r, c in enumerate(cols):
            x[r, c] = 300.0
            if kind == 'twin':
                x[r, (c + n // 2) % n] = 300.0
        return x.half()
    m = 8
    if kind == 'flat':
        return torch.full((m, n), -7.0).half()
    if kind == 'base':
        return (torch.randn(m, n, generator=g) * 4 - 60000.0).half()
    if kind == 'gauss3':
        return (torch.randn(m, n, generator=g) * 3).half()
    if kind == 'gauss10':
        return (torch.randn(m, n, generator=g) * 10).half()
    raise ValueError(kind)


def softmax_ref(x):
    return torch.softmax(x.double(), -1)


def softmax2_ref(s):
    """fp64 base-2 softmax over the last axis: 2^(s - max) / sum"""
    s = s.double()
    e = torch.exp2(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_f32(x):
    """softmax_rows_kernel's arithmetic in fp32: exp2((v - max) log2 e), fp32 sums, one reciprocal, fp16 store"""
    xf = x.float()
    v = xf - xf.max(1, keepdim=True).values
    e = torch.exp2(v * torch.tensor(1.4426950408889634, dtype=torch.float32))
    s = e.sum(1, keepdim=True, dtype=torch.float32)
    return (e * (1.0 / s)).half()


def row_sum_bound(n):
    """|sum of a softmax row's fp16 outputs - 1| in fp64: half a subnormal spacing per element at the worst, plus the relative
    rounding of the few large ones"""
    return n * 2.0 ** -25 + 2.0 ** -10


# ----------------------------------------------------------------------------------------- score-GEMM softmax epilogue
EPI_GROUP, EPI_KEYS = 80, 77         # an 80-column group holds a head's 77 keys and 3 padding columns (bias -30000)
EPI_KINDS = ('peak', 'twin', 'flat', 'gauss')


def epilogue_scores(kind, m, n, seed=0):
    """fp64 [m][n] scores in log2 units, each a multiple of 1/4 of magnitude <= 330 (exact as 0.5 * fp16); the padding columns are 0
    here and get their -30000 from the bias.  'peak': row r of every group has +320 at column r mod 77 over -320 + N(0, 1); 'twin'
    a second equal peak 38 columns on; 'flat' all -7; 'gauss' 10 N(0, 1) (outputs down to fp16 subnormals)"""
    assert n % EPI_GROUP == 0
    g = _gen(5000 + seed + n)
    groups = n // EPI_GROUP
    z = torch.randn(m, groups, EPI_GROUP, generator=g, dtype=torch.float64)
    if kind in ('peak', 'twin'):
        s = torch.round((z - 320.0) * 4) / 4
        r = torch.arange(m)
        s[r, :, r % EPI_KEYS] = 320.0
        if kind == 'twin':
            s[r, :, (r + 38) % EPI_KEYS] = 320.0
    elif kind == 'flat':
        s = torch.full_like(z, -7.0)
    elif kind == 'gauss':
        s = torch.round(z * 10 * 4) / 4
    else:
        raise ValueError(kind)
    s[:, :, EPI_KEYS:] = 0.0
    return s.reshape(m, n)


def epilogue_operands(scores, k):
    """(a fp16 [m][k], w fp16 [n][k], bias fp32 [n]) with a . w^T + bias = scores exactly (padding columns: -30000): w is half the
    identity and a twice the scores, so every row of the product is one exact term and zeros"""
    m, n = scores.shape
    assert k >= n
    a = torch.zeros(m, k, dtype=torch.float64)
    a[:, :n] = 2 * scores
    assert torch.equal(a.half().double(), a)
    w = torch.zeros(n, k)
    w[torch.arange(n), torch.arange(n)] = 0.5
    bias = torch.zeros(n)
    bias.view(-1, EPI_GROUP)[:, EPI_KEYS:] = -30000.0
    return a.half(), w.half(), bias


def epilogue_ref(scores):
    """fp64 base-2 softmax of every 80-column group, the padding columns at -30000 (exact zeros)"""
    m, n = scores.shape
    s = scores.double().view(m, n // EPI_GROUP, EPI_GROUP).clone()
    s[:, :, EPI_KEYS:] = -30000.0
    return softmax2_ref(s).reshape(m, n)


# -------------------------------------------------------------------------------------------------------- activations
def all_finite_f16():
    """the 63 488 finite fp16 values, in bit order"""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    x = x[torch.isfinite(x)]
    assert x.numel() == 63488
    return x


def silu64(x):
    x = x.double()
    return x / (1 + torch.exp(-x))


def quick_gelu64(x):
    x = x.double()
    return x / (1 + torch.exp(-1.702 * x))


ACT_REF = {'silu': silu64, 'gelu': gelu64, 'quick_gelu': quick_gelu64}
ACT_BOUND = {'silu': (SILU_R, 0.0), 'gelu': (GELU_R, GELU_A), 'quick_gelu': (SILU_R, 0.0)}     # (r, a) of close16


def _f32(v):
    return v.float().double()


def gelu_poly_f32(x):
    """common.h's gelu_erf_f in emulated fp32 (fp64 values rounded to fp32 after every fma; a correctly rounded exp2), as fp64"""
    x = x.double()
    a = x.abs()
    q = torch.full_like(a, float(torch.tensor(0.000488102092, dtype=torch.float32)))
    for c in (-0.0071987181, 0.052146631, 0.459595845, 1.15100054, 1.0):
        q = _f32(q * a + float(torch.tensor(c, dtype=torch.float32)))
    e = _f32(torch.exp2(-q))
    return _f32(-a * e + x.clamp_min(0.0))


def silu_f32(x, c=1.0):
    """x * (1 / (1 + exp(-c x))) with every operation rounded to fp32 and an exact reciprocal, as fp64 (c = 1.702: quick-GELU)"""
    x = x.double()
    arg = _f32(-float(torch.tensor(c, dtype=torch.float32)) * x) if c != 1.0 else -x
    return _f32(x * _f32(1.0 / _f32(1.0 + _f32(torch.exp(arg)))))
