"""The references and bounds of tests/glue_cases.py, checked without a GPU.  Per kernel: the float32 restatement that
test_glue_kernels_gpu.py holds the GPU to bit for bit lies within the fp64 formula's bound with room (its worst error is printed as
a fraction of the bound and must be <= 0.75), so a mistake copied from a kernel into a restatement shows here; and each mistake
named in glue_cases.MISTAKES, applied to the restatement, leaves the bound on these inputs -- so the data can see it.  Where the
output is fp16 the half-ulp term of the bound is the rounding itself; there the fp32 part is held to 0.75 on its own."""
import numpy as np
import pytest
import torch

import glue_cases as gl
import row_cases as rc

ROOM = 0.75


def _pair32(shape, seed=0):
    n, c, h, w = shape
    eu, ec = gl.step_eps(n, c, h, w, seed)
    return gl.nchw(eu), gl.nchw(ec)


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_cfg_restatement_is_inside_the_bound_and_the_data_sees_the_mistakes(shape):
    eu, ec = _pair32(shape)
    for mode in (0, 1):
        for g in gl.GUIDANCE:
            ref, s = gl.cfg_f64(eu, ec, g, mode)
            ex = gl.excess(gl.cfg_f32(eu, ec, g, mode), ref, s, gl.CFG_R)
            print(f'cfg {shape} mode {mode} g {g}: restatement {ex * (gl.CFG_R + 1):.2f} of {gl.CFG_R + 1} units')
            assert ex <= ROOM, (shape, mode, g, ex)
            swapped = gl.excess(gl.cfg_f32(ec, eu, g, mode), ref, s, gl.CFG_R)
            assert swapped > 1, ('swapped rows', shape, mode, g, swapped)
    if eu.size < 100:
        return              # four elements hold one cancelling pair: the rounding-level mistake below needs the larger shapes
    for g in gl.GUIDANCE_FULL_MANTISSA:   # (with a short g both formulas are exact on fp16 inputs: the same bits, no mistake to see)
        ref, s = gl.cfg_f64(eu, ec, g, 1)
        wrong = gl.excess(gl.cfg_f32(eu, ec, g, 0), ref, s, gl.CFG_R)
        print(f'cfg {shape} g {g}: mode 0 formula against mode 1 bound {wrong:.1f}x')
        assert wrong > 1, ('mode 0 formula in mode 1', shape, g, wrong)


def test_step_eps_is_what_it_says():
    n, c, h, w = 3, 4, 5, 7
    eu, ec = gl.step_eps(n, c, h, w)
    assert eu.shape == (n, h * w, c) and eu.dtype == np.float16
    kind, _ = gl._kinds(n, c, h * w)
    d = np.abs(ec.astype(np.float64) - eu.astype(np.float64))
    ulp = rc.ulp16(torch.from_numpy(np.abs(eu).astype(np.float64))).numpy()
    assert (d[kind == 1] <= ulp[kind == 1]).all() and (d[kind == 1] > 0).any() and (d[kind == 1] == 0).any()
    assert (np.abs(eu[kind == 2].astype(np.float64)) > 25).all() and (np.abs(ec[kind == 2].astype(np.float64)) > 25).all()
    assert abs((kind == 1).mean() - 1 / 3) < 0.05 and abs((kind == 2).mean() - 1 / 3) < 0.05
    # the three images differ everywhere a row mix-up (img for img + n, or another image) would read
    packed = gl.pack_eps(eu, ec, True).astype(np.float64)
    for a in range(2 * n):
        for b in range(a + 1, 2 * n):
            assert (packed[a] != packed[b]).mean() > 0.6, (a, b)
    assert np.array_equal(gl.pack_eps(eu, ec, False)[:n], ec)


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_lincomb_restatement_is_inside_the_bound_and_the_data_sees_the_mistakes(shape):
    n, c, h, w = shape
    hist = gl.step_history((n, c, h * w))
    for cs, div in gl.PLMS_SETS:
        es = hist[:len(cs)]
        ref, s = gl.lincomb_f64(es, cs, div)
        r = gl.lincomb_r(es)
        ex = gl.excess(gl.lincomb_f32(es, cs, div), ref, s, r)
        print(f'lincomb4 {shape} {len(cs)} terms: restatement {ex * (r + 1):.2f} of {r + 1} units')
        assert ex <= ROOM, (shape, cs, ex)
        if div != 1.0:
            assert gl.excess(gl.lincomb_f32(es, cs, 1.0), ref, s, r) > 1, ('division dropped', shape, cs)
        if len(cs) == 4:
            sw = (cs[0], cs[1], cs[3], cs[2])
            assert gl.excess(gl.lincomb_f32(es, sw, div), ref, s, r) > 1, ('c2 <-> c3', shape)
    # a NULL e1 with a non-NULL e2 is the combination without that term, not the one that stops at the first NULL
    es = [hist[0], None, hist[2], None]
    cs, div = (55.0, -59.0, 37.0, -9.0), 24.0
    ref, s = gl.lincomb_f64(es, cs, div)
    assert gl.lincomb_r(es) == 3 and gl.excess(gl.lincomb_f32(es, cs, div), ref, s, 3) <= ROOM
    assert gl.excess(gl.lincomb_f32([hist[0], None, None, None], cs, div), ref, s, 3) > 1


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_ddim_restatement_is_inside_the_bound_and_the_data_sees_the_mistakes(shape):
    _, e = _pair32(shape)
    for t, tp in gl.DDIM_PAIRS:
        coef = gl.ddim_coef(t, tp)
        x = gl.step_latent(e, coef)
        ref, s = gl.ddim_f64(x, e, coef)
        ex = gl.excess(gl.ddim_f32(x, e, coef), ref, s, gl.DDIM_R)
        print(f'ddim {shape} {t}->{tp}: restatement {ex * (gl.DDIM_R + 1):.2f} of {gl.DDIM_R + 1} units')
        assert ex <= ROOM, (shape, t, ex)
        s1m, s_at, s_ap, dirc = coef
        x0 = (x - s1m * e) / s_at
        assert gl.excess(s_ap * x0 + dirc * x0, ref, s, gl.DDIM_R) > 1, ('dir * x0', shape, t)
        assert gl.excess(gl.ddim_f32(x, e, (s1m, s_ap, s_at, dirc)), ref, s, gl.DDIM_R) > 1, ('s_at <-> s_aprev', shape, t)


def test_ddim_coefficients_are_the_sd_schedule():
    ab = gl.sd_alphas_cumprod()
    assert ab.shape == (1000,) and abs(ab[0] - 0.99915) < 1e-6 and abs(ab[999] - 0.0046602) < 1e-6      # ldm's published endpoints
    for t, tp in gl.DDIM_PAIRS:
        s1m, s_at, s_ap, dirc = (float(v) for v in gl.ddim_coef(t, tp))
        assert abs(s1m ** 2 + s_at ** 2 - 1) < 1e-6 and abs(s_ap ** 2 + dirc ** 2 - 1) < 1e-6 and s_ap > s_at


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_v_to_eps_and_the_whole_step_restatement(shape):
    eu, ec = _pair32(shape)
    t, tp = 501, 451
    coef, vc = gl.ddim_coef(t, tp), gl.v_coef(t)
    x = gl.step_latent(ec, coef)
    v = gl.cfg_f32(eu, ec, 7.5, 1)
    ref, s = gl.v_to_eps_f64(v, x, vc)
    ex = gl.excess(gl.v_to_eps_f32(v, x, vc), ref, s, gl.V_R)
    print(f'v -> eps {shape}: restatement {ex * (gl.V_R + 1):.2f} of {gl.V_R + 1} units')
    assert ex <= ROOM
    assert gl.excess(gl.v_to_eps_f32(v, x, (vc[1], vc[0])), ref, s, gl.V_R) > 1           # the two coefficients exchanged
    # the whole step is the composition of the pieces above, each in the order the header gives
    hist = gl.step_history(x.shape)
    (cs, div) = gl.PLMS_SETS[0]
    e_t, xn = gl.plms_step_f32(eu, ec, 7.5, 1, x, hist[1:], cs, div, coef, vc)
    assert np.array_equal(e_t, gl.v_to_eps_f32(v, x, vc))
    assert np.array_equal(xn, gl.ddim_f32(x, gl.lincomb_f32([e_t] + hist[1:], cs, div), coef))
    assert e_t.dtype == np.float32 and xn.dtype == np.float32


# ---------------------------------------------------------------------------------------------------------------- B
def test_layout_data_reaches_the_fp16_edges_and_tells_fp32_from_fp64_products():
    n, c, hw = gl.LAYOUT_BIG
    assert n * c * hw > 2048 * 256
    for scale in (gl.LATENT_SCALE, gl.SECOND_SCALE):
        x = gl.layout_input(n, c, hw, scale)
        y = gl.to_nhwc16_f32(x, scale)
        yf = y.astype(np.float64)
        assert np.isposinf(yf).any() and np.isneginf(yf).any() and (np.abs(yf) == 65504).any()
        sub = (np.abs(yf) > 0) & (np.abs(yf) < 2.0 ** -14)
        assert sub.any() and (y.view(np.uint16) == 0x8000).any() and (y.view(np.uint16) == 0).any()
        differ = int((y.view(np.uint16) != gl.to_nhwc16_via_f64(x, scale).view(np.uint16)).sum())
        print(f'scale {scale:.6f}: {differ} of {y.size} products round differently through fp64')
        if scale == gl.SECOND_SCALE:
            assert differ >= 1
    # the small shapes carry the same edge values (those that fit)
    x = gl.layout_input(1, 3, 35, gl.LATENT_SCALE)
    assert np.isinf(gl.to_nhwc16_f32(x, gl.LATENT_SCALE).astype(np.float64)).any()
    h = gl.nhwc16_input(1, 3, 35)
    assert np.isinf(h.astype(np.float64)).any() and not np.isnan(h.astype(np.float64)).any()


@pytest.mark.parametrize('c', gl.PREP_C)
def test_latent_prep_restatement_is_inside_the_bound(c):
    w, b = gl.prep_params(c)
    for hw in gl.PREP_HW:
        x = gl.prep_input(2, c, hw)
        for ww, bb in ((w, b), (w, None), (None, b), (None, None)):
            ref, s = gl.prep_f64(x, ww, bb, gl.LATENT_SCALE)
            raw = gl.prep_f32(x, ww, bb, gl.LATENT_SCALE, raw=True).astype(np.float64)
            part = float((np.abs(raw - ref) / (gl.prep_r(c) * s)).max())
            whole = float(rc.close16_excess(torch.from_numpy(gl.prep_f32(x, ww, bb, gl.LATENT_SCALE)), torch.from_numpy(ref), 0.0,
                                            torch.from_numpy(gl.prep_r(c) * s)).max())
            print(f'latent_prep c {c} hw {hw} w {ww is not None} b {bb is not None}: fp32 part {part:.2f}, with the fp16 rounding {whole:.2f}')
            assert part <= ROOM and whole <= 1.0, (c, hw, part, whole)
    # without w and b it is the layout change
    x = gl.prep_input(2, c, 35)
    assert np.array_equal(gl.prep_f32(x, None, None, gl.LATENT_SCALE).view(np.uint16), gl.to_nhwc16_f32(x, gl.LATENT_SCALE).view(np.uint16))
    # and a w transposed in the reference would be seen
    ref, s = gl.prep_f64(x, w, b, gl.LATENT_SCALE)
    wrong = gl.prep_f32(x, np.ascontiguousarray(w.T), b, gl.LATENT_SCALE)
    assert float(rc.close16_excess(torch.from_numpy(wrong), torch.from_numpy(ref), 0.0, torch.from_numpy(gl.prep_r(c) * s)).max()) > 1


def test_embedding_data():
    ids = gl.embedding_ids()
    assert ids.numel() == 3 * gl.SEQ and int(ids.min()) == 0 and int(ids.max()) == gl.VOCAB - 1
    assert bool((ids[1:] == ids[:-1]).any())
    for width in gl.EMB_WIDTHS:
        t = gl.hashed_f16(ids, width, 1)
        assert t.shape == (ids.numel(), width) and torch.isfinite(t).all()
        assert torch.equal(t[1], t[2]) and not torch.equal(t[0], t[1])
        ref = gl.embedding_ref(ids, width)
        p = gl.hashed_f16(torch.arange(ids.numel()) % gl.SEQ, width, 2)
        exact = t.double() + p.double()
        assert torch.isfinite(ref).all() and bool((ref.double() != exact).any())          # the sum is rounded somewhere
        assert not torch.equal(p[0], p[1]) and torch.equal(p[0], p[gl.SEQ])
        # a row is a function of its id alone, whatever else is gathered with it
        assert torch.equal(gl.hashed_f16(ids[5:9], width, 1), t[5:9])


# ---------------------------------------------------------------------------------------------------------------- C
def test_lane_input_covers_every_finite_value():
    x, base = gl.lane_input(gl.LANE_COUNTS[2])
    assert x.numel() == 8 * (524288 + 3) and x.numel() // 8 > 2048 * 256 and (x.numel() // 8) % 256 != 0
    assert base.numel() == 63488 and torch.equal(base.view(torch.int16).sort().values, rc.all_finite_f16().view(torch.int16).sort().values)
    assert torch.equal(x[63488:63488 + 100], base[:100])
    x, base = gl.lane_input(8)
    assert x.numel() == 8 and torch.equal(x, base)
    for m, c in gl.GEGLU_SHAPES:
        assert c % 8 == 0
    m, c = gl.GEGLU_SHAPES[-1]
    assert m * (c // 8) > 2048 * 256


# ---------------------------------------------------------------------------------------------------------------- D
def test_to_u8_restatement_at_the_special_values(oracle_lib):
    v = gl.all_f16_patterns()
    f = v.astype(np.float32)
    assert v.size == 65536 and np.isnan(f).sum() == 2046 and np.isinf(f).sum() == 2
    finite = np.isfinite(f)
    order = np.argsort(f[finite], kind='stable')
    for a, b in gl.U8_AB:
        for mode in (0, 1):
            out = gl.to_u8_f32(v, a, b, mode)
            assert (out[np.isnan(f)] == 0).all() and out[np.isposinf(f)] == 255 and out[np.isneginf(f)] == 0
            assert out[0x8000] == out[0x0000] == (0 if b == 0 else 127)               # -0 and +0
            assert (np.diff(out[finite][order].astype(np.int32)) >= 0).all()          # monotone in the pixel value
            assert set(np.unique(out)) == set(range(256))
        # the two modes are the same function away from the clamps (255 (a v + b) in both), and the test data reaches both clamps
        assert np.array_equal(gl.to_u8_f32(v, a, b, 0), gl.to_u8_f32(v, a, b, 1))
    # mode 0 at (1, 0) is the reference driver's loop (its comparisons leave NaN alone and the cast of NaN is undefined: no NaN)
    ok = ~np.isnan(f)
    src = np.ascontiguousarray(f[ok])
    ref = np.zeros(src.size, np.uint8)
    oracle_lib.oracle_to_uint8(ref.ctypes.data, src.ctypes.data, src.size)
    assert np.array_equal(gl.to_u8_f32(v, 1.0, 0.0, 0)[ok], ref)


@pytest.mark.parametrize('dim', gl.TEMB_DIMS)
def test_timestep_argument_in_fp32_is_inside_its_term(dim):
    ref, arg, expo = gl.temb_f64(gl.TEMB_T, dim)
    assert ref.shape == (len(gl.TEMB_T), dim)
    a32 = gl.temb_arg_f32(gl.TEMB_T, dim).astype(np.float64)
    term = gl.temb_arg_term(arg, expo)
    with np.errstate(invalid='ignore', divide='ignore'):
        frac = np.where(term > 0, np.abs(a32 - arg) / term, np.where(a32 == arg, 0.0, np.inf))
    print(f'timestep_features dim {dim}: the fp32 argument uses {frac.max():.2f} of its term')
    assert frac.max() <= ROOM
    # cos and sin of the fp32 argument, rounded to fp16, are inside the whole bound; a frequency table with half + 1 entries is not
    out = np.concatenate([np.cos(a32), np.sin(a32)], 1).astype(np.float16).astype(np.float64)
    assert (np.abs(out - ref) <= gl.temb_bound(out, ref, arg, expo)).all()
    half = dim // 2
    wrong_arg = np.array([float(np.float32(t)) for t in gl.TEMB_T])[:, None] * np.exp(-np.log(10000.0) * np.arange(half) / (half - 1))[None]
    wrong = np.concatenate([np.cos(wrong_arg), np.sin(wrong_arg)], 1).astype(np.float16).astype(np.float64)
    assert (np.abs(wrong - ref) > gl.temb_bound(wrong, ref, arg, expo)).any()


# ---------------------------------------------------------------------------------------------------------------- E
def test_wrappers_refuse_a_bad_destination_before_touching_the_library():
    """no GPU and no library call: the ValueError names the tensor that is wrong (CPU tensors fail the device check only AFTER these)"""
    from sdod.amd import ops
    a = torch.zeros(4, 16, dtype=torch.float16)
    good = torch.zeros(4, 16, dtype=torch.float16)
    cases = {
        'dtype': torch.zeros(4, 16, dtype=torch.float32),
        'short': torch.zeros(4, 8, dtype=torch.float16),
        'long': torch.zeros(5, 16, dtype=torch.float16),
        'strided': torch.zeros(4, 32, dtype=torch.float16)[:, ::2],
    }
    for what, bad in cases.items():
        for call in (lambda: ops.add(a, good, out=bad), lambda: ops.activation(a, 'silu', out=bad), lambda: ops.softmax_rows(a, out=bad)):
            with pytest.raises(ValueError, match=r'^out must'):
                call()
        with pytest.raises(ValueError, match=r'^b must'):
            ops.add(a, bad)
    g_in = torch.zeros(4, 32, dtype=torch.float16)
    for what, bad in cases.items():
        with pytest.raises(ValueError, match=r'^out must'):
            ops.geglu(g_in, out=bad)
    with pytest.raises(ValueError, match=r'^out must live on'):
        ops.add(a, good, out=torch.zeros(4, 16, dtype=torch.float16, device='meta'))
    # well-formed CPU tensors get as far as the device check
    with pytest.raises(ValueError, match='must live on the GPU'):
        ops.add(a, good, out=good)
