"""Shared pieces of the glue-kernel tests (test_glue_kernels_gpu.py, test_glue_cases_cpu.py): the sampler-step base arithmetic
(cfg_combine, lincomb4, ddim_step, the v -> eps conversion) and the small kernels around the graphs (layout changes, latent_prep,
embedding, stage_unet_inputs, image_to_u8, timestep_features, the 16-byte-lane fp16 kernels), against references written from the
published formulas and include/sdod_hip.h -- not from the kernels.

Every step kernel has two references:
  *_f64   the mathematical formula in fp64 on the fp32 inputs, with S = the fp64 sum of the absolute values of its terms.  The bound
          of an fp32 evaluation is (r + 1) 2^-24 S, r = the roundings on the longest path from an input to the result:
              CFG (either mode)   sub, mul, add                              r = 3
              lincomb4, k terms   mul, k - 1 adds, div                       r = k + 1
              DDIM update         mul, sub, div, mul, add                    r = 5
              v -> eps            mul, add (the division by 1 is exact)      r = 2
          (first order, a path of r roundings of relative size 2^-24 / 2 each moves the result by at most r / 2 units of 2^-24 S:
          half the bound is room by construction.)
  *_f32   a numpy float32 restatement in the header's operation order: numpy rounds every float32 product, sum and quotient on its
          own (IEEE single), which is what the header promises of the kernels, so the GPU must equal it bit for bit.
test_glue_cases_cpu.py ties *_f32 to *_f64 within the bound (a mistake copied from a kernel into a restatement shows there) and
proves that the data sees the mistakes listed in MISTAKES.

Data.  step_eps(): the (uncond, cond) fp16 prediction pair; element (img, pix, ch) is of kind (img + pix + ch) % 3: 0 = independent
Gaussians on an offset that names (img, ch, pix), 1 = cond within one fp16 ulp of uncond (the guided difference cancels), 2 = both
near +-30.  An index mistake therefore reads a value that is wrong by far more than any bound."""
import math

import numpy as np
import torch

U = 2.0 ** -24                      # the unit of every fp32 bound here
F32 = np.float32

# ------------------------------------------------------------------------------------------------- A. sampler base arithmetic
STEP_SHAPES = [(1, 4, 1, 1), (3, 4, 5, 7), (2, 4, 16, 24), (2, 4, 256, 257)]      # (n, c, h, w); the last: 526 336 > 2048 * 256
# 0, 1, 7.5 and 30 have at most four mantissa bits, and so have the products with an fp16 value: on them most of the arithmetic is
# exact and the two modes give the same bits.  7.1 and 12.3 have full fp32 mantissas: every product rounds, which is what makes the
# restatement's distance to fp64 a measurement and "mode 0's formula in mode 1" visible (on the cancelling third mode 0's terms are
# 2 g - 1 times larger than mode 1's).
GUIDANCE = (0.0, 1.0, 7.5, 30.0, 7.1, 12.3)
GUIDANCE_FULL_MANTISSA = (7.1, 12.3)
PLMS_SETS = (((55.0, -59.0, 37.0, -9.0), 24.0), ((23.0, -16.0, 5.0), 12.0), ((3.0, -1.0), 2.0), ((1.0,), 1.0))
DDIM_PAIRS = ((999, 949), (501, 451), (51, 1), (1, 0))       # (t, t_prev); (1, 0) is the last step: alphas_prev[0] = abar[0]
MISTAKES = ('swapped rows', 'mode 0 formula in mode 1', 'c2 <-> c3', 'division dropped', 'dir * x0', 's_at <-> s_aprev')


def sd_alphas_cumprod():
    """ldm make_beta_schedule('linear', 1000, 0.00085, 0.012) and its cumulative product, fp64"""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def ddim_coef(t, t_prev):
    """(sqrt(1 - abar_t), sqrt(abar_t), sqrt(abar_prev), sqrt(1 - abar_prev)) as fp32 scalars: ldm's get_x_prev_and_pred_x0, sigma = 0"""
    ab = sd_alphas_cumprod()
    a_t, a_p = ab[t], ab[t_prev]
    return tuple(F32(v) for v in (math.sqrt(1 - a_t), math.sqrt(a_t), math.sqrt(a_p), math.sqrt(1 - a_p)))


def v_coef(t):
    """ldm predict_eps_from_z_and_v: eps = sqrt(abar_t) v + sqrt(1 - abar_t) x -> (coefficient of v, coefficient of x), fp32"""
    ab = sd_alphas_cumprod()
    return F32(math.sqrt(ab[t])), F32(math.sqrt(1 - ab[t]))


def _kinds(n, c, hw):
    img, pix, ch = np.meshgrid(np.arange(n), np.arange(hw), np.arange(c), indexing='ij')
    ident = (img * 4 + ch) * 0.5 + ((pix * 37) % 101) / 128.0
    return (img + pix + ch) % 3, ident


def _next16(a, up):
    """the fp16 neighbours of the finite fp16 array a: one ulp away from zero where `up`, towards zero elsewhere"""
    bits = a.view(np.uint16).astype(np.int32)
    mag = bits & 0x7FFF
    mag = np.where(up, np.minimum(mag + 1, 0x7BFF), np.maximum(mag - 1, 0))
    return ((bits & 0x8000) | mag).astype(np.uint16).view(np.float16)


def step_eps(n, c, h, w, seed=0):
    """(uncond, cond): fp16 [n][hw][c] each, the two halves of the UNet's NHWC prediction (see the module docstring)"""
    hw = h * w
    rng = np.random.default_rng(100 + seed)
    kind, ident = _kinds(n, c, hw)
    z0, z1 = rng.standard_normal((n, hw, c)), rng.standard_normal((n, hw, c))
    sign = np.where(rng.random((n, hw, c)) < 0.5, -1.0, 1.0)
    eu = np.where(kind == 2, sign * 30 + z0, z0 + ident).astype(np.float16)
    ec = np.where(kind == 2, sign * 30 + z1, z1 + ident + 0.125).astype(np.float16)
    step = rng.integers(0, 3, (n, hw, c))                     # kind 1: cond = uncond, one ulp above, one ulp below
    near = np.where(step == 0, eu, _next16(eu, step == 1))
    ec = np.where(kind == 1, near, ec)
    return np.ascontiguousarray(eu), np.ascontiguousarray(ec)


def pack_eps(eu, ec, uncond_first):
    """the kernel's input [2n][hw][c]: rows [0, n) are the unconditional half when uncond_first"""
    return np.concatenate([eu, ec] if uncond_first else [ec, eu], 0)


def nchw(a):
    """[n][hw][c] -> [n][c][hw], fp32"""
    return np.ascontiguousarray(a.astype(np.float32).transpose(0, 2, 1))


def step_latent(e, coef, seed=0):
    """the latent x fp32 [n][c][hw] for the prediction e (fp32, same shape): a third N(0, 1), a third 30 N(0, 1), a third within
    2^-12 of sqrt(1 - abar) e, so that x - sqrt(1 - abar) e cancels"""
    rng = np.random.default_rng(200 + seed)
    z = rng.standard_normal(e.shape)
    k = np.arange(e.size).reshape(e.shape) % 3
    x = np.where(k == 0, z, np.where(k == 1, 30 * z, float(coef[0]) * e.astype(np.float64) * (1 + z * 2.0 ** -12)))
    return x.astype(np.float32)


def step_history(shape, seed=0):
    """four fp32 arrays e0..e3 of `shape`: a third independent N(0, 1), a third near +-30, a third equal to within 2^-10 (the partial
    sums of the Adams-Bashforth combinations cancel)"""
    rng = np.random.default_rng(300 + seed)
    count = int(np.prod(shape))
    k = np.arange(count).reshape(shape) % 3
    common = rng.standard_normal(shape) * 3
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    out = []
    for _ in range(4):
        z = rng.standard_normal(shape)
        out.append(np.where(k == 0, z, np.where(k == 1, sign * 30 + z, common * (1 + z * 2.0 ** -10))).astype(np.float32))
    return out


# -- CFG: e = g e_c + (1 - g) e_u (mode 0, the reference driver) / e = e_u + g (e_c - e_u) (mode 1, ldm); inputs fp32 arrays
def cfg_f64(eu, ec, g, mode):
    """(value, S) in fp64; g is the fp32 scalar the kernel receives"""
    eu, ec, g = eu.astype(np.float64), ec.astype(np.float64), float(F32(g))
    if mode == 0:
        return g * ec + (1 - g) * eu, np.abs(g * ec) + np.abs((1 - g) * eu)
    return eu + g * (ec - eu), np.abs(eu) + np.abs(g * (ec - eu))


def cfg_f32(eu, ec, g, mode):
    eu, ec, g = eu.astype(np.float32), ec.astype(np.float32), F32(g)
    if mode == 0:
        return g * ec + (F32(1.0) - g) * eu
    return eu + g * (ec - eu)


CFG_R = 3


# -- lincomb4: (c0 e0 + c1 e1 + c2 e2 + c3 e3) / div, left to right; a term whose array is None is left out
def lincomb_f64(es, cs, div):
    terms = [float(F32(c)) * e.astype(np.float64) / float(F32(div)) for e, c in zip(es, cs) if e is not None]
    return sum(terms), sum(np.abs(t) for t in terms)


def lincomb_f32(es, cs, div):
    v = None
    for e, c in zip(es, cs):
        if e is None:
            continue
        p = F32(c) * e.astype(np.float32)
        v = p if v is None else v + p
    return v / F32(div)


def lincomb_r(es):
    return sum(e is not None for e in es) + 1


# -- ldm DDIM / PLMS update, eta = 0: x0 = (x - sqrt(1 - abar_t) e) / sqrt(abar_t); x' = sqrt(abar_prev) x0 + sqrt(1 - abar_prev) e
def ddim_f64(x, e, coef):
    s1m, s_at, s_ap, dirc = (float(v) for v in coef)
    x, e = x.astype(np.float64), e.astype(np.float64)
    x0 = (x - s1m * e) / s_at
    return s_ap * x0 + dirc * e, (np.abs(s_ap * x / s_at) + np.abs(s_ap * s1m * e / s_at) + np.abs(dirc * e))


def ddim_f32(x, e, coef):
    s1m, s_at, s_ap, dirc = (F32(v) for v in coef)
    x, e = x.astype(np.float32), e.astype(np.float32)
    x0 = (x - s1m * e) / s_at
    return s_ap * x0 + dirc * e


DDIM_R = 5


# -- v-prediction: eps = vc0 v + vc1 x (the host loop composes it as lincomb4([v, x], [vc0, vc1], 1): the division by 1 is exact)
def v_to_eps_f64(v, x, vc):
    a, b = float(vc[0]) * v.astype(np.float64), float(vc[1]) * x.astype(np.float64)
    return a + b, np.abs(a) + np.abs(b)


def v_to_eps_f32(v, x, vc):
    return (F32(vc[0]) * v.astype(np.float32) + F32(vc[1]) * x.astype(np.float32)) / F32(1.0)


V_R = 2


def plms_step_f32(eu, ec, g, mode, x, olds, cs, div, coef, vc=None):
    """one whole PLMS step as include/sdod_hip.h states it for sdod_plms_update: e_t = CFG (then v -> eps), e' = lincomb4 of e_t and
    the history, x <- DDIM update with e'.  eu / ec / x / olds fp32 [n][c][hw].  Returns (e_t, x')"""
    e = cfg_f32(eu, ec, g, mode)
    if vc is not None:
        e = v_to_eps_f32(e, x, vc)
    ep = lincomb_f32([e] + list(olds), cs, div)
    return e, ddim_f32(x, ep, coef)


def excess(out, ref, s, r):
    """max over the elements of |out - ref| / ((r + 1) 2^-24 S); an element with S == 0 must be exact"""
    err = np.abs(out.astype(np.float64) - ref)
    bound = (r + 1) * U * s
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits32(out, ref, name=''):
    """bit-for-bit equality of fp32 arrays, with the first mismatch in the message"""
    a, b = bits32(np.asarray(out)).reshape(-1), bits32(np.asarray(ref)).reshape(-1)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f'{name}: {bad.size} of {a.size} elements differ, first at {i}: {a[i:i + 1].view(np.float32)[0]!r} '
                             f'({a[i]:#010x}) vs {b[i:i + 1].view(np.float32)[0]!r} ({b[i]:#010x})')


def same_bits16(out, ref, name=''):
    a = np.ascontiguousarray(np.asarray(out)).view(np.uint16).reshape(-1)
    b = np.ascontiguousarray(np.asarray(ref)).view(np.uint16).reshape(-1)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f'{name}: {bad.size} of {a.size} halves differ, first at {i}: {a[i]:#06x} vs {b[i]:#06x}')


# ---------------------------------------------------------------------------------------------- B. layout, latent entry / exit
LATENT_SCALE = 1.0 / 0.18215
SECOND_SCALE = 0.7310585786300049            # no special value: products that round differently in fp32 than in fp64 must occur
LAYOUT_C, LAYOUT_HW, LAYOUT_N = (3, 4, 8, 9), (1, 35, 4096), (1, 3)
LAYOUT_BIG = (2, 9, 29128)                   # (n, c, hw): 524 304 elements, 16 more than one pass of 2048 * 256 threads
PREP_C, PREP_HW = (4, 16), (1, 35, 4096)

_EDGE16 = (65504.0, 65519.0, 65519.99, 65520.0, 65521.0, 65536.0, 1.0e5, 2.0 ** -24, 2.0 ** -25, 1.0000001 * 2.0 ** -25, 1.5 * 2.0 ** -24,
           2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 6.0e-5, 6.1e-5, 1.0, 0.0)


def layout_input(n, c, hw, scale, seed=0):
    """fp32 NCHW [n][c][hw]: N(0, 1) on an offset that names (img, ch, pix); the first elements of the flat array are replaced by
    +-(edge / scale) for the fp16 overflow edge (65504 -> 65520 -> inf), the subnormal range and +-0"""
    rng = np.random.default_rng(400 + seed + 7 * c + hw)
    img, ch, pix = np.meshgrid(np.arange(n), np.arange(c), np.arange(hw), indexing='ij')
    x = (rng.standard_normal((n, c, hw)) + 0.25 * img + 0.5 * ch + ((pix * 37) % 101) / 256.0).astype(np.float32)
    edges = np.array([s * v / scale for v in _EDGE16 for s in (1.0, -1.0)], np.float64).astype(np.float32)
    flat = x.reshape(-1)
    k = min(flat.size, edges.size)
    flat[:k] = edges[:k]
    return x


def to_nhwc16_f32(x, scale):
    """the contract of sdod_nchw_f32_to_nhwc_f16: the fp32 product, rounded to nearest-even fp16 (overflow: inf)"""
    with np.errstate(over='ignore'):
        return np.ascontiguousarray((x * F32(scale)).transpose(0, 2, 1).astype(np.float16))


def to_nhwc16_via_f64(x, scale):
    """the same through an fp64 product: NOT the contract; differs where the fp32 product lands on an fp16 tie"""
    with np.errstate(over='ignore'):
        return np.ascontiguousarray((x.astype(np.float64) * float(F32(scale))).transpose(0, 2, 1).astype(np.float16))


def nhwc16_input(n, c, hw, seed=0):
    """fp16 NHWC [n][hw][c]: Gaussians of three magnitudes on an identifying offset, then +-inf, +-0, +-65504 and subnormals in front"""
    rng = np.random.default_rng(500 + seed + 7 * c + hw)
    img, pix, ch = np.meshgrid(np.arange(n), np.arange(hw), np.arange(c), indexing='ij')
    mag = np.array([1.0, 1e-6, 3e3])[(pix + ch) % 3]
    x = ((rng.standard_normal((n, hw, c)) + 0.25 * img + 0.5 * ch) * mag).astype(np.float16)
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 1023 * 2.0 ** -24], np.float16)
    flat = x.reshape(-1)
    k = min(flat.size, special.size)
    flat[:k] = special[:k]
    return x


def prep_params(c, seed=0):
    """(w fp32 [c][c], b fp32 [c]) of the size of the VAE's post_quant_conv; rows of mixed sign so that the sum cancels"""
    rng = np.random.default_rng(600 + seed + c)
    return rng.standard_normal((c, c)).astype(np.float32), rng.standard_normal(c).astype(np.float32)


def prep_input(n, c, hw, seed=0):
    rng = np.random.default_rng(700 + seed + 7 * c + hw)
    img, ch, pix = np.meshgrid(np.arange(n), np.arange(c), np.arange(hw), indexing='ij')
    return ((rng.standard_normal((n, c, hw)) + 0.25 * img + 0.125 * ch + ((pix * 37) % 101) / 256.0) * 0.18215).astype(np.float32)


def prep_f64(x, w, b, scale):
    """(y fp64 NHWC [n][hw][c], S): y[img][pix][o] = sum_c w[o][c] (scale x[img][c][pix]) + b[o]; w None: the identity"""
    xs = x.astype(np.float64).transpose(0, 2, 1) * float(F32(scale))          # [n][hw][c]
    if w is None:
        y, s = xs.copy(), np.abs(xs)
    else:
        w64 = w.astype(np.float64)
        y, s = xs @ w64.T, np.abs(xs) @ np.abs(w64).T
    if b is not None:
        y, s = y + b.astype(np.float64), s + np.abs(b.astype(np.float64))
    return y, s


def prep_f32(x, w, b, scale, raw=False):
    """latent_prep in fp32, one rounding per operation, bias first then the channels in order (no contraction), as fp16 (raw: the
    fp32 accumulator in front of the fp16 rounding)"""
    xs = (x.astype(np.float32) * F32(scale)).transpose(0, 2, 1)
    c = x.shape[1]
    acc = np.zeros(xs.shape, np.float32) if b is None else np.broadcast_to(b.astype(np.float32), xs.shape).copy()
    if w is None:
        acc = acc + xs
    else:
        for o in range(c):
            for ch in range(c):
                acc[..., o] = acc[..., o] + w[o, ch] * xs[..., ch]
    return acc if raw else acc.astype(np.float16)


def prep_r(c):
    return (c + 2) * U


# embedding: the table is a function of (row, column) so that the GPU test can build all 49 408 rows on the device and the
# reference only the rows it gathers
VOCAB, SEQ = 49408, 77
EMB_WIDTHS = (8, 768, 1024, 1280)


def hashed_f16(rows, width, salt):
    """fp16 [len(rows)][width] of finite values 2^-7 <= |v| < 2^9, a function of (row id, column, salt) in exact integer arithmetic
    (torch int64: the same on every device)"""
    r = rows.to(torch.int64)[:, None]
    c = torch.arange(width, dtype=torch.int64, device=rows.device)[None, :]
    h = (((r * 1000003 + c * 7919 + salt) % (1 << 31)) * 40503) % (1 << 32)        # (below 2^47: no int64 wrap)
    h = (h >> 13) & 0xFFFF
    bits = (h & 0x83FF) | ((((h >> 10) & 0xF) + 8) << 10)
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits)
    return bits.to(torch.int16).view(torch.float16)


def embedding_ids(seed=0):
    """int32 [3 * 77]: row % seq wraps twice; ids 0 and 49407, the same id twice in a row, the rest spread over the vocabulary"""
    g = torch.Generator().manual_seed(800 + seed)
    ids = torch.randint(0, VOCAB, (3 * SEQ,), generator=g, dtype=torch.int32)
    ids[0], ids[1], ids[2], ids[3] = 0, VOCAB - 1, VOCAB - 1, 0
    ids[SEQ - 1], ids[SEQ] = 5, 5
    ids[-1] = VOCAB - 1
    return ids


def embedding_ref(ids, width):
    """fp16((float)table[id] + (float)pos[row % seq])"""
    t = hashed_f16(ids, width, 1)
    p = hashed_f16(torch.arange(ids.numel()) % SEQ, width, 2)
    return (t.float() + p.float()).half()


# --------------------------------------------------------------------------------------------- C. the 16-byte-lane kernels
LANE_COUNTS = (8, 8 * 300, 8 * (524288 + 3))
GUARD = 64                                   # halves on each side of every destination
CONCAT_C, CONCAT_ROWS = ((8, 8), (128, 64), (320, 1280)), (1, 50)
GEGLU_SHAPES = ((1, 8), (3, 800), (1639, 2560))          # (m, c): 1, 300 and 524 480 lanes (one pass is 524 288)


def lane_input(count, seed=0):
    """fp16 [count]: every finite fp16 value in a seeded order, repeated; `base` (the first min(count, 63488) values) is what a
    reference needs: element i is base[i % 63488]"""
    import row_cases as rc
    allv = rc.all_finite_f16()
    perm = torch.randperm(allv.numel(), generator=torch.Generator().manual_seed(900 + seed))
    base = allv[perm][:min(count, allv.numel())].contiguous()
    reps = -(-count // base.numel())
    return base.repeat(reps)[:count].contiguous(), base


# --------------------------------------------------------------------------------------- D. image_to_u8, timestep_features
U8_AB = ((1.0, 0.0), (0.5, 0.5))


def all_f16_patterns():
    """every one of the 65 536 fp16 bit patterns, in bit order (NaNs, +-inf and -0 included)"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def to_u8_f32(v16, a, b, mode):
    """include/sdod_hip.h: f = a v + b; mode 0: clamp(255 f, 0, 255); mode 1: 255 clamp(f, 0, 1); truncating cast.  clamp =
    fmin(fmax(f, lo), hi), which gives lo for NaN (np.fmax / np.fmin ignore a NaN operand as fmaxf / fminf do)"""
    with np.errstate(invalid='ignore', over='ignore'):
        f = F32(a) * v16.astype(np.float32) + F32(b)
        if mode == 0:
            f = np.fmin(np.fmax(F32(255.0) * f, F32(0.0)), F32(255.0))
        else:
            f = F32(255.0) * np.fmin(np.fmax(f, F32(0.0)), F32(1.0))
        assert f.dtype == np.float32 and not np.isnan(f).any()
        return f.astype(np.uint8)


TEMB_DIMS = (192, 320, 384)
TEMB_T = (999.0, 949.05, 499.5, 14.614641, 0.029, 1.0, 0.0)


def temb_f64(ts, dim):
    """(ref fp64 [len(ts)][dim], arg, exponent): cos | sin of arg = fp32(t) exp(-ln 1e4 j / half)"""
    half = dim // 2
    expo = -math.log(10000.0) * np.arange(half, dtype=np.float64) / half
    arg = np.array([float(F32(t)) for t in ts])[:, None] * np.exp(expo)[None, :]
    return np.concatenate([np.cos(arg), np.sin(arg)], 1), arg, np.broadcast_to(expo[None, :], arg.shape)


def temb_arg_f32(ts, dim):
    """the argument as the fp32 chain of context.cpp:257-274 forms it: t * expf(-logf(1e4) * j / half)"""
    half = dim // 2
    lp = -np.log(F32(10000.0))
    assert lp.dtype == np.float32
    e = np.exp(lp * np.arange(half).astype(np.float32) / F32(half))
    assert e.dtype == np.float32
    return np.array(ts, np.float32)[:, None] * e[None, :]


def temb_arg_term(arg, expo):
    """the bound's fp32-argument term: arg (|exponent| + 4) 2^-23 -- the exponent's two roundings (|exponent| 2^-23 absolute, which
    expf turns into a relative error of the same size), expf's own ulp and the product's rounding, with room"""
    return np.abs(arg) * (np.abs(expo) + 4) * 2.0 ** -23


def temb_bound(out, ref, arg, expo):
    """ulp16(max(|out|, |ref|)) / 2 + arg (|exponent| + 4) 2^-23 + 2^-22 (device cosf / sinf); cos and sin share the argument"""
    import row_cases as rc
    m = np.maximum(np.abs(out), np.abs(ref))
    half_ulp = 0.5 * rc.ulp16(torch.from_numpy(np.ascontiguousarray(m))).numpy()
    a = temb_arg_term(arg, expo)
    return half_ulp + np.concatenate([a, a], 1) + 2.0 ** -22
