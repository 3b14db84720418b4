"""The sampler-step base arithmetic and the glue kernels of csrc/elementwise.hip against the references of tests/glue_cases.py.

A  cfg_combine (both modes, both row orders), lincomb4 (one to four terms, a NULL term in the middle, div = 0), ddim_step and the
   whole PLMS step with v-prediction: bit for bit against the float32 restatements, and inside the fp64 formulas' bounds.  The fused
   step kernels are tested elsewhere against "the launches they replace"; these are those launches' own contract.
B  the layout changes bit for bit (fp16 overflow edge, subnormals, a scale whose fp32 products round differently than fp64 ones),
   latent_prep with the VAE's post_quant_conv against fp64, embedding, stage_unet_inputs at its corners.
C  the 16-byte-lane fp16 kernels at 1 lane, 300 lanes and more than one pass of the grid with a ragged end, every destination a
   window inside a NaN-filled buffer whose 64 halves on either side must keep their bits.
D  image_to_u8 over all 65 536 fp16 patterns, timestep_features at the widths and fractional times the engine uses.
E  the refusals: misaligned pointers (nothing is launched: the NaN-filled destination keeps its bits), bad destinations of the wrappers.

tests/test_glue_cases_cpu.py proves without a GPU that the references meet every bound used here with room and that the data sees
the mistakes these tests are for."""
import ctypes

import numpy as np
import pytest
import torch

import glue_cases as gl
import row_cases as rc

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7E00          # torch's fp16 NaN fill


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def P(t, off=0):
    """device pointer `off` elements into t"""
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def lib():
    from sdod.amd import _lib
    return _lib.hip()


class Window:
    """`count` elements inside a NaN-filled device buffer with gl.GUARD elements on either side; the window starts 16-byte aligned"""

    def __init__(self, count, dtype=torch.float16):
        self.count = count
        self.buf = torch.full((gl.GUARD + count + gl.GUARD,), float('nan'), dtype=dtype, device=dev())
        self.view = self.buf[gl.GUARD:gl.GUARD + count]
        assert self.view.data_ptr() % 16 == 0

    def guards_intact(self):
        g = torch.cat([self.buf[:gl.GUARD], self.buf[gl.GUARD + self.count:]])
        return bool(torch.isnan(g).all()) and (g.dtype != torch.float16 or bool((g.view(torch.int16) == NAN_BITS).all()))

    def untouched(self):
        return self.guards_intact() and bool(torch.isnan(self.view).all())


# ------------------------------------------------------------------------------------------- A. sampler base arithmetic
_step_cache = {}


def _step_case(shape):
    """per shape, computed once and left unchanged: the fp16 pair, its fp32 NCHW form and the history arrays"""
    if shape not in _step_cache:
        n, c, h, w = shape
        eu, ec = gl.step_eps(n, c, h, w)
        _step_cache[shape] = dict(eu16=eu, ec16=ec, eu=gl.nchw(eu), ec=gl.nchw(ec), hist=gl.step_history((n, c, h * w)))
    return _step_cache[shape]


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_cfg_combine_is_the_header_formula_bit_for_bit(shape):
    from sdod.amd import ops
    n, c, h, w = shape
    k = _step_case(shape)
    for uf in (True, False):
        eps = T(gl.pack_eps(k['eu16'], k['ec16'], uf)).view(2 * n, h, w, c)
        for mode in (0, 1):
            for g in gl.GUIDANCE:
                out = ops.cfg_combine(eps, g, uncond_first=uf, mode=mode)
                assert out.shape == (n, c, h, w) and out.dtype == torch.float32
                out = out.cpu().numpy().reshape(n, c, h * w)
                name = f'cfg {shape} uncond_first {uf} mode {mode} g {g}'
                ref, s = gl.cfg_f64(k['eu'], k['ec'], g, mode)
                ex = gl.excess(out, ref, s, gl.CFG_R)
                print(f'{name}: {ex:.3f} of the fp64 bound')
                gl.same_bits32(out, gl.cfg_f32(k['eu'], k['ec'], g, mode), name)
                assert ex <= 1, name


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_lincomb4_one_to_four_terms_a_null_in_the_middle_and_div_zero(shape):
    from sdod.amd import ops
    k = _step_case(shape)
    hist = k['hist']
    dh = [T(e) for e in hist]
    for cs, div in gl.PLMS_SETS:
        es = hist[:len(cs)]
        out = ops.lincomb4(dh[:len(cs)], cs, div).cpu().numpy()
        name = f'lincomb4 {shape} {len(cs)} terms'
        ref, s = gl.lincomb_f64(es, cs, div)
        ex = gl.excess(out, ref, s, gl.lincomb_r(es))
        print(f'{name}: {ex:.3f} of the fp64 bound')
        gl.same_bits32(out, gl.lincomb_f32(es, cs, div), name)
        assert ex <= 1, name
    # through the C ABI: e1 NULL, e2 given (the header allows it, the wrapper cannot say it); the NULL term's coefficient is ignored
    count = hist[0].size
    cs, div = gl.PLMS_SETS[0]
    win = Window(count, torch.float32)
    assert lib().sdod_lincomb4_f32(P(win.view), P(dh[0]), None, P(dh[2]), None, cs[0], cs[1], cs[2], cs[3], div, count, None) == 0
    torch.cuda.synchronize()
    es = [hist[0], None, hist[2], None]
    gl.same_bits32(win.view.cpu().numpy(), gl.lincomb_f32(es, cs, div), f'lincomb4 {shape} NULL e1')
    assert win.guards_intact()
    # div = 0 is refused and nothing is written
    win = Window(count, torch.float32)
    assert lib().sdod_lincomb4_f32(P(win.view), P(dh[0]), P(dh[1]), None, None, 3.0, -1.0, 0.0, 0.0, 0.0, count, None) != 0
    torch.cuda.synchronize()
    assert win.untouched(), 'a refused lincomb4 wrote to its destination'


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_ddim_step_in_place_on_the_sd_schedule(shape):
    from sdod.amd import ops
    k = _step_case(shape)
    e = k['ec']
    de = T(e)
    for t, tp in gl.DDIM_PAIRS:
        coef = gl.ddim_coef(t, tp)
        x = gl.step_latent(e, coef)
        dx = T(x)
        ops.ddim_step(dx, de, *(float(v) for v in coef))
        out = dx.cpu().numpy()
        name = f'ddim {shape} {t}->{tp}'
        ref, s = gl.ddim_f64(x, e, coef)
        ex = gl.excess(out, ref, s, gl.DDIM_R)
        print(f'{name}: {ex:.3f} of the fp64 bound')
        gl.same_bits32(out, gl.ddim_f32(x, e, coef), name)
        assert ex <= 1, name
    gl.same_bits32(de.cpu().numpy(), e, 'the prediction is only read')


@pytest.mark.parametrize('shape', gl.STEP_SHAPES)
def test_plms_update_with_v_prediction_is_the_whole_step_restated(shape):
    """CFG -> v to eps -> lincomb4 -> DDIM in one launch against the restatement of the whole step (not against the separate launches:
    test_kernels_gpu.py::test_plms_update_equals_the_four_launches does that)"""
    from sdod.amd import ops
    n, c, h, w = shape
    k = _step_case(shape)
    eps = T(gl.pack_eps(k['eu16'], k['ec16'], True)).view(2 * n, h, w, c)
    t, tp = 501, 451
    coef, vc = gl.ddim_coef(t, tp), gl.v_coef(t)
    ddim = dict(sqrt_one_minus_at=float(coef[0]), sqrt_at=float(coef[1]), sqrt_a_prev=float(coef[2]), dir_coef=float(coef[3]))
    x = gl.step_latent(k['ec'], coef)
    for cs, div in gl.PLMS_SETS:
        olds = k['hist'][1:len(cs)]
        for g, v_coef in ((7.1, vc), (7.5, vc), (7.1, None)):
            dx = T(x).view(n, c, h, w)
            e_t = ops.plms_update(eps, dx, [T(o).view(n, c, h, w) for o in olds], cs, div, ddim, g, mode=1,
                                  v_coef=None if v_coef is None else (float(v_coef[0]), float(v_coef[1])))
            ref_e, ref_x = gl.plms_step_f32(k['eu'], k['ec'], g, 1, x, olds, cs, div, coef, v_coef)
            name = f'plms_update {shape} order {len(cs)} g {g} v_pred {v_coef is not None}'
            gl.same_bits32(e_t.cpu().numpy(), ref_e, name + ' e_t')
            gl.same_bits32(dx.cpu().numpy(), ref_x, name + ' x')


# ----------------------------------------------------------------------------------------- B. layout, latent entry / exit
def _layout_roundtrip(n, c, hw, scale):
    from sdod.amd import ops
    x = gl.layout_input(n, c, hw, scale)
    out = ops.nchw_f32_to_nhwc_f16(T(x), float(scale))
    assert out.shape == (n, hw, c) and out.dtype == torch.float16
    gl.same_bits16(out.cpu().numpy(), gl.to_nhwc16_f32(x, scale), f'nchw->nhwc n {n} c {c} hw {hw} scale {scale:.5f}')
    h = gl.nhwc16_input(n, c, hw)
    back = ops.nhwc_f16_to_nchw_f32(T(h))
    assert back.shape == (n, c, hw) and back.dtype == torch.float32
    gl.same_bits32(back.cpu().numpy(), h.astype(np.float32).transpose(0, 2, 1), f'nhwc->nchw n {n} c {c} hw {hw}')


@pytest.mark.parametrize('c', gl.LAYOUT_C)
def test_layout_changes_bit_for_bit(c):
    for hw in gl.LAYOUT_HW:
        for n in gl.LAYOUT_N:
            for scale in (gl.LATENT_SCALE, gl.SECOND_SCALE):
                _layout_roundtrip(n, c, hw, scale)


def test_layout_changes_beyond_one_pass_of_the_grid():
    n, c, hw = gl.LAYOUT_BIG
    for scale in (gl.LATENT_SCALE, gl.SECOND_SCALE):
        _layout_roundtrip(n, c, hw, scale)


@pytest.mark.parametrize('c', gl.PREP_C)
def test_latent_prep_with_the_post_quant_conv_vs_fp64(c):
    n = 2
    w, b = gl.prep_params(c)
    dw, db = T(w), T(b)
    for hw in gl.PREP_HW:
        x = gl.prep_input(n, c, hw)
        dx = T(x)
        for ww, bb, pw, pb in ((w, b, P(dw), P(db)), (w, None, P(dw), None), (None, b, None, P(db))):
            win = Window(n * hw * c)
            assert lib().sdod_latent_prep_f16(P(dx), pw, pb, P(win.view), n, c, hw, gl.LATENT_SCALE, None) == 0
            torch.cuda.synchronize()
            ref, s = gl.prep_f64(x, ww, bb, gl.LATENT_SCALE)
            name = f'latent_prep c {c} hw {hw} w {ww is not None} b {bb is not None}'
            worst = rc.check_close16(win.view.cpu().view(n, hw, c), torch.from_numpy(ref), 0.0, torch.from_numpy(gl.prep_r(c) * s), name=name)
            print(f'{name}: worst |err| / bound {worst:.3f}')
            assert win.guards_intact(), name
        # without w and b it is sdod_nchw_f32_to_nhwc_f16, bit for bit -- on the edge values too (inf, subnormals, -0)
        from sdod.amd import ops
        xe = gl.layout_input(n, c, hw, gl.LATENT_SCALE)
        dxe = T(xe)
        win = Window(n * hw * c)
        assert lib().sdod_latent_prep_f16(P(dxe), None, None, P(win.view), n, c, hw, gl.LATENT_SCALE, None) == 0
        plain = ops.nchw_f32_to_nhwc_f16(dxe, gl.LATENT_SCALE)
        gl.same_bits16(win.view.cpu().numpy(), plain.cpu().numpy().reshape(-1), f'latent_prep c {c} hw {hw} without w, b')
        assert win.guards_intact()


@pytest.mark.parametrize('width', gl.EMB_WIDTHS)
def test_embedding_bit_for_bit_over_the_whole_vocabulary(width):
    from sdod.amd import ops
    d = dev()
    table = gl.hashed_f16(torch.arange(gl.VOCAB, device=d), width, 1)
    pos = gl.hashed_f16(torch.arange(gl.SEQ, device=d), width, 2)
    ids = gl.embedding_ids()
    # the device builds the table the reference gathers from
    assert torch.equal(table[ids.long().to(d)].cpu().view(torch.int16), gl.hashed_f16(ids, width, 1).view(torch.int16))
    out = ops.embedding(ids.view(3, gl.SEQ).to(d), table, pos)
    assert out.shape == (3, gl.SEQ, width)
    gl.same_bits16(out.cpu().numpy().reshape(-1), gl.embedding_ref(ids, width).numpy().reshape(-1), f'embedding width {width}')


def test_stage_unet_inputs_at_its_corners():
    d = dev()
    g = torch.Generator().manual_seed(97)
    x = torch.randn(420, generator=g).to(d)
    # one copy, and a time row whose width (1283) does not divide the 2048 * 256 threads of a pass; 420 + 450 * 1283 > one pass
    row = torch.randn(1283, generator=g).half().to(d)
    xw, tw = Window(420, torch.float32), Window(450 * 1283)
    assert 420 + 450 * 1283 > 2048 * 256
    assert lib().sdod_stage_unet_inputs(P(x), P(xw.view), 420, 1, P(row), P(tw.view), 1283, 450, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(xw.view, x) and torch.equal(tw.view.view(450, 1283), row[None].expand(450, -1))
    assert xw.guards_intact() and tw.guards_intact()
    # no time row at all: temb_reps = 0 with NULL pointers; two copies of the latent
    xw = Window(840, torch.float32)
    assert lib().sdod_stage_unet_inputs(P(x), P(xw.view), 420, 2, None, None, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(xw.view[:420], x) and torch.equal(xw.view[420:], x) and xw.guards_intact()
    # a time row without a destination is refused, nothing written
    xw = Window(420, torch.float32)
    assert lib().sdod_stage_unet_inputs(P(x), P(xw.view), 420, 1, P(row), None, 1283, 2, None) != 0
    torch.cuda.synchronize()
    assert xw.untouched()


# ------------------------------------------------------------------------------------------- C. the 16-byte-lane kernels
def _periodic(out, base_out):
    """out (the kernel's result on gl.lane_input data) repeats its first len(base_out) elements: the input does, and the kernel is a
    function of the element alone"""
    p = base_out.numel()
    full = out.numel() // p * p
    body = out[:full].view(-1, p).view(torch.int16)
    return bool((body == base_out.view(torch.int16)[None]).all()) and torch.equal(out[full:].view(torch.int16), base_out[:out.numel() - full].view(torch.int16))


@pytest.mark.parametrize('count', gl.LANE_COUNTS)
def test_add_and_adapter_stage_bit_for_bit_inside_guard_bands(count):
    from sdod.amd import ops
    a, abase = gl.lane_input(count, 1)
    b, bbase = gl.lane_input(count, 2)
    da, db = a.to(dev()), b.to(dev())
    win = Window(count)
    ops.add(da, db, out=win.view)
    out = win.view.cpu()
    ref = (abase.float() + bbase.float()).half()
    assert torch.equal(out[:ref.numel()].view(torch.int16), ref.view(torch.int16)) and _periodic(out, ref), f'add {count}'
    assert win.guards_intact()
    ops.add(da, db, out=da)                                               # in place on the first operand
    assert torch.equal(da.cpu().view(torch.int16), out.view(torch.int16)), f'add in place {count}'
    for weight in (0.7, 1.0):
        win = Window(count)
        ops.adapter_stage(db, win.view, weight)
        out = win.view.cpu()
        ref = (torch.tensor(weight, dtype=torch.float32) * bbase.float()).half()
        assert torch.equal(out[:ref.numel()].view(torch.int16), ref.view(torch.int16)) and _periodic(out, ref), f'adapter_stage {count} {weight}'
        assert win.guards_intact()


@pytest.mark.parametrize('act', ['silu', 'gelu', 'quick_gelu', 'relu'])
@pytest.mark.parametrize('count', gl.LANE_COUNTS)
def test_activation_inside_guard_bands(count, act):
    from sdod.amd import ops
    x, base = gl.lane_input(count, 3)
    win = Window(count)
    ops.activation(x.to(dev()), act, out=win.view)
    out = win.view.cpu()
    assert win.guards_intact(), f'{act} {count}'
    first = out[:base.numel()]
    if act == 'relu':
        assert torch.equal(first.view(torch.int16), torch.where(base < 0, torch.zeros_like(base), base).view(torch.int16))
    else:
        r, a = rc.ACT_BOUND[act]
        rc.check_close16(first, rc.ACT_REF[act](base), r, a, name=f'activation {act} {count}')
    assert _periodic(out, first), f'{act} {count}: equal inputs, different outputs'


@pytest.mark.parametrize('m,c', gl.GEGLU_SHAPES)
def test_geglu_inside_guard_bands(m, c):
    from sdod.amd import ops
    gate, _ = gl.lane_input(m * c, 4)
    g = torch.Generator().manual_seed(31)
    value = (torch.randn(m, c, generator=g) * torch.tensor([1.0, 2.0 ** -10, 3.0])[torch.arange(c) % 3]).half()
    gate = gate.view(m, c)
    x = torch.cat([value, gate], 1).contiguous()
    win = Window(m * c)
    ops.geglu(x.to(dev()), out=win.view)
    out = win.view.cpu().view(m, c)
    assert win.guards_intact()
    ref = value.double() * rc.gelu64(gate)
    over = ref.abs() >= 65520
    assert torch.equal(out[over].double(), torch.sign(ref[over]) * float('inf')), 'overflow is not an infinity'
    rc.check_close16(out[~over], ref[~over], rc.GELU_R + 2.0 ** -24, value.double().abs()[~over] * rc.GELU_A, name=f'geglu {m}x{c}')


@pytest.mark.parametrize('rows', gl.CONCAT_ROWS)
@pytest.mark.parametrize('c0,c1', gl.CONCAT_C)
def test_concat_channels_bit_for_bit_inside_guard_bands(c0, c1, rows):
    a, _ = gl.lane_input(rows * c0, 5)
    b, _ = gl.lane_input(rows * c1, 6)
    da, db = a.to(dev()), b.to(dev())
    win = Window(rows * (c0 + c1))
    assert lib().sdod_concat_channels_f16(P(da), P(db), P(win.view), rows, c0, c1, None) == 0
    torch.cuda.synchronize()
    ref = torch.cat([a.view(rows, c0), b.view(rows, c1)], 1)
    assert torch.equal(win.view.cpu().view(torch.int16), ref.reshape(-1).view(torch.int16)) and win.guards_intact()


@pytest.mark.parametrize('reps', [1, 2])
@pytest.mark.parametrize('count', gl.LANE_COUNTS)
def test_add_feature_every_copy_inside_guard_bands(count, reps):
    """the ABI's per_copy is both the feature's length and the distance between the copies: the second copy at count + i proves the
    stride"""
    from sdod.amd import ops
    f, fbase = gl.lane_input(count, 7)
    h, _ = gl.lane_input(reps * count, 8)
    df = f.to(dev())
    win = Window(reps * count)
    win.view.copy_(h.to(dev()))
    ops.add_feature(win.view, df, reps)
    out = win.view.cpu()
    for r in range(reps):
        ref = (h[r * count:(r + 1) * count].float() + f.float()).half()
        assert torch.equal(out[r * count:(r + 1) * count].view(torch.int16), ref.view(torch.int16)), (count, reps, r)
    assert win.guards_intact() and torch.equal(df.cpu().view(torch.int16), f.view(torch.int16))


# --------------------------------------------------------------------------------- D. image_to_u8, timestep_features
def test_image_to_u8_every_fp16_pattern(oracle_lib):
    from sdod.amd import ops
    v = gl.all_f16_patterns()
    dv = T(v)
    for a, b in gl.U8_AB:
        for mode in (0, 1):
            got = ops.image_to_u8(dv, a=a, b=b, mode=mode).cpu().numpy()
            ref = gl.to_u8_f32(v, a, b, mode)
            bad = np.nonzero(got != ref)[0]
            assert bad.size == 0, f'image_to_u8 a {a} b {b} mode {mode}: {bad.size} patterns differ, first {int(bad[0]):#06x}: {got[bad[0]]} vs {ref[bad[0]]}'
    f = v.astype(np.float32)
    got = ops.image_to_u8(dv, a=1.0, b=0.0, mode=0).cpu().numpy()
    assert (got[np.isnan(f)] == 0).all() and got[0x7C00] == 255 and got[0xFC00] == 0 and got[0x8000] == 0       # NaN, +inf, -inf, -0
    ok = ~np.isnan(f)
    src = np.ascontiguousarray(f[ok])
    ref = np.zeros(src.size, np.uint8)
    oracle_lib.oracle_to_uint8(ref.ctypes.data, src.ctypes.data, src.size)
    assert np.array_equal(got[ok], ref)


@pytest.mark.parametrize('dim', gl.TEMB_DIMS)
def test_timestep_features_at_the_engine_widths_and_fractional_times(dim):
    from sdod.amd import ops
    ref, arg, expo = gl.temb_f64(gl.TEMB_T, dim)
    out = ops.timestep_features(torch.tensor(gl.TEMB_T, dtype=torch.float32, device=dev()), dim)
    assert out.shape == (len(gl.TEMB_T), dim)
    out = out.cpu().double().numpy()
    frac = np.abs(out - ref) / gl.temb_bound(out, ref, arg, expo)
    i = np.unravel_index(int(np.argmax(frac)), frac.shape)
    print(f'timestep_features dim {dim}: worst |err| / bound {frac.max():.3f} at t {gl.TEMB_T[i[0]]} column {i[1]}')
    assert np.isfinite(out).all() and frac.max() <= 1, (dim, i, out[i], ref[i])
    assert (out[-1, :dim // 2] == 1).all() and (out[-1, dim // 2:] == 0).all()           # t = 0


# ------------------------------------------------------------------------------------------------------- E. refusals
def test_misaligned_pointers_are_refused_and_nothing_is_written():
    L = lib()
    x = torch.ones(4096 + 16, dtype=torch.float16, device=dev())
    x2 = torch.ones(4096 + 16, dtype=torch.float16, device=dev())
    y = torch.full((8192 + 16,), float('nan'), dtype=torch.float16, device=dev())
    ids = torch.zeros(16, dtype=torch.int32, device=dev())

    def refused(rc_):
        return rc_ != 0 and b'misaligned' in L.sdod_hip_last_error()

    for act in (1, 2, 3, 4):
        assert refused(L.sdod_act_f16(P(x, 1), P(y), 4096, act, None)) and refused(L.sdod_act_f16(P(x), P(y, 4), 4096, act, None))
    assert refused(L.sdod_add_f16(P(x, 1), P(x2), P(y), 4096, None))
    assert refused(L.sdod_add_f16(P(x), P(x2, 2), P(y), 4096, None))
    assert refused(L.sdod_add_f16(P(x), P(x2), P(y, 7), 4096, None))
    assert refused(L.sdod_geglu_f16(P(x, 4), P(y), 8, 256, None)) and refused(L.sdod_geglu_f16(P(x), P(y, 1), 8, 256, None))
    assert refused(L.sdod_concat_channels_f16(P(x, 1), P(x2), P(y), 16, 64, 64, None))
    assert refused(L.sdod_concat_channels_f16(P(x), P(x2, 1), P(y), 16, 64, 64, None))
    assert refused(L.sdod_concat_channels_f16(P(x), P(x2), P(y, 1), 16, 64, 64, None))
    # embedding: 16 rows of 64 columns from a 64-row table (x) and 8 positions (x2); ids are all 0
    assert refused(L.sdod_embedding_f16(P(ids), P(x, 1), P(x2), P(y), 16, 8, 64, None))
    assert refused(L.sdod_embedding_f16(P(ids), P(x), P(x2, 1), P(y), 16, 8, 64, None))
    assert refused(L.sdod_embedding_f16(P(ids), P(x), P(x2), P(y, 1), 16, 8, 64, None))
    assert refused(L.sdod_embedding_f16(ctypes.c_void_p(ids.data_ptr() + 2), P(x), P(x2), P(y), 8, 8, 64, None))
    torch.cuda.synchronize()
    assert bool((y.view(torch.int16) == NAN_BITS).all()) and bool((x == 1).all()) and bool((x2 == 1).all())
    # and the same calls on aligned pointers run
    assert L.sdod_act_f16(P(x), P(y), 4096, 1, None) == 0 and L.sdod_add_f16(P(x), P(x2), P(y), 4096, None) == 0
    assert L.sdod_geglu_f16(P(x), P(y), 8, 256, None) == 0 and L.sdod_concat_channels_f16(P(x), P(x2), P(y), 16, 64, 64, None) == 0
    assert L.sdod_embedding_f16(P(ids), P(x), P(x2), P(y), 16, 8, 64, None) == 0
    torch.cuda.synchronize()
    assert bool((y[:1024] == 2).all()) and bool((y[1024:2048] == 1).all()) and bool(torch.isnan(y[4096:]).all())


def test_wrappers_refuse_a_bad_destination_or_operand_on_the_gpu():
    from sdod.amd import ops
    d = dev()
    a = torch.ones(4, 16, dtype=torch.float16, device=d)
    keep = torch.full((4, 16), float('nan'), dtype=torch.float16, device=d)
    bad = [torch.full((4, 16), float('nan'), dtype=torch.float32, device=d), keep[:2], keep.t(), torch.zeros(4, 16, dtype=torch.float16)]
    for out in bad:
        for call in (lambda: ops.add(a, a, out=out), lambda: ops.activation(a, 'silu', out=out), lambda: ops.softmax_rows(a, out=out)):
            with pytest.raises(ValueError, match=r'^out must'):
                call()
        with pytest.raises(ValueError, match=r'^out must'):
            ops.geglu(torch.ones(4, 32, dtype=torch.float16, device=d), out=out)
        with pytest.raises(ValueError, match=r'^b must'):
            ops.add(a, out)                                               # (a short b would be read past its end)
    torch.cuda.synchronize()
    assert bool(torch.isnan(keep).all()) and bool(torch.isnan(bad[0]).all())
