"""The ESRGAN dense-block convolution (sdod_dense_conv3x3_f16) and RRDBNet's input convolution (sdod_image_conv_in_unit_f16) on the GPU.

Exact data, as tests/conv_cases.py does it: ternary inputs and weights, small integer bias and residuals, power-of-two coefficients
(alpha in {1, 0.25}, slope in {0, 0.25}, c1 in {1, 0.5}).  9 * 192 + 8 < 2048, so every partial sum is an exact fp16 integer whatever
the summation order or FMA contraction; every epilogue stage is exact in fp32 and the fp64 reference is checked for fp16
representability (gemm_cases.assert_exact) before anything is launched.  The output must EQUAL the reference.

Memory safety of the access pattern: the input lives in a NaN-guarded allocation (conv_cases.guarded_nhwc: a tap that leaves the image
or leaks across images meets NaN or independent data), the channels of the wide rows outside [0, cin) and outside the written slice
are pre-filled with +Inf or NaN, the written slice must equal the reference bit for bit and every other element of every buffer must
be byte-identical afterwards."""
import functools

import pytest
import torch

import conv_cases as cc
import gemm_cases as gc
from gemm_cases import check_close, check_equal, dev
from sdod.amd import _lib, ops

pytestmark = pytest.mark.gpu

CINS = (64, 96, 128, 160, 192)
COUTS = (32, 64)
LD = 192
# several images per tile, whole rows, row segments, a tile edge inside a row, the widest input the graph takes
GEOMS = [(2, 8, 16), (2, 16, 24), (3, 8, 8), (1, 8, 64), (1, 8, 256), (2, 24, 16), (1, 16, 1024)]
# form -> (alpha, slope, c1, res1?, res2?)
FORMS = {'plain': (1.0, 0.0, 0.0, False, False), 'slope': (0.25, 0.25, 0.0, False, False), 'res1': (0.25, 0.0, 0.5, True, False),
         'res2': (1.0, 0.0, 1.0, True, True), 'slope_res2': (1.0, 0.25, 0.5, True, True)}
POISON = {'inf': float('inf'), 'nan': float('nan')}


def epilogue_ref(acc_plus_bias, form, res1, res2):
    """fp64: y = alpha * (acc + bias); LeakyReLU; + c1 * res1; + res2"""
    alpha, slope, c1, has1, has2 = FORMS[form]
    y = alpha * acc_plus_bias
    if slope != 0.0:
        y = torch.where(y < 0, slope * y, y)
    if has1:
        y = y + c1 * res1.double().reshape(y.shape)
    if has2:
        y = y + res2.double().reshape(y.shape)
    return y


@functools.lru_cache(None)
def exact_case(n, h, w, cin, cout, form, seed, ups=False):
    """(operands, exact fp64 reference [pixels][cout]) of one case, computed once; callers must not modify what they get"""
    gen = torch.Generator().manual_seed(seed)
    ho, wo = cc.out_size(h, w, ups=ups)
    d = dict(x=gc.ternary((n, h, w, cin), gen), w=gc.ternary((cout, 9 * cin), gen), bias=gc.small_ints((cout,), gen, torch.float32),
             res1=gc.small_ints((n, ho, wo, cout), gen), res2=gc.small_ints((n, ho, wo, cout), gen))
    ref = epilogue_ref(cc.ref_conv(d['x'], d['w'], d['bias'], ups=ups), form, d['res1'], d['res2'])
    gc.assert_exact(ref)
    return d, ref


def bits(t):
    return t.view(torch.int16)


def run_case(n, h, w, cin, cout, form, seed, place, poison='inf', ups=False):
    """place 'inplace': out is the input buffer, out_col = cin, ld = 192; 'second': out is columns [8, 8 + cout) of a second buffer"""
    d, ref = exact_case(n, h, w, cin, cout, form, seed, ups)
    alpha, slope, c1, has1, has2 = FORMS[form]
    dv = dev()
    ho, wo = cc.out_size(h, w, ups=ups)
    ld_in = LD if place == 'inplace' else cin + 8
    wide = torch.full((n, h, w, ld_in), POISON[poison], dtype=torch.float16)
    wide[..., :cin] = d['x']
    xin = cc.guarded_nhwc(wide, dv)
    if place == 'inplace':
        assert not ups and cin + cout <= LD
        out, ld_out, col = xin, LD, cin
    else:
        ld_out, col = cout + 16, 8
        out = torch.full((n, ho, wo, ld_out), POISON[poison], dtype=torch.float16, device=dv)
    res1 = d['res1'].to(dv) if has1 else None
    if has2:                                  # res2 aliases the written slice (the last convolution of an RRDB)
        out[..., col:col + cout] = d['res2'].to(dv)
    before_in, before_out = bits(xin._guard_buf).clone(), bits(out).clone()
    res1_before = bits(res1).clone() if has1 else None
    wdev, bias = d['w'].to(dv), d['bias'].to(dv)
    ops.dense_conv(xin, wdev, bias, out, n=n, h=h, wd=w, cin=cin, cout=cout, ld_in=ld_in, ld_out=ld_out, out_col=col, alpha=alpha, slope=slope,
                   res1=res1, ld_res1=cout, c1=c1, res2=out if has2 else None, res2_off=col, ld_res2=ld_out, upsample=int(ups))
    torch.cuda.synchronize()
    name = f'{(n, h, w)} cin{cin} cout{cout} {form} {place} {poison}' + (' ups' if ups else '')
    check_equal(out[..., col:col + cout].reshape(-1, cout), ref, name)
    # everything but the written slice is byte-identical: the guards, the poisoned channels, the input itself
    after_out = bits(out).clone()
    after_out[..., col:col + cout] = before_out[..., col:col + cout]
    assert torch.equal(after_out, before_out), f'{name}: the output buffer changed outside the written slice'
    if place != 'inplace':
        assert torch.equal(bits(xin._guard_buf), before_in), f'{name}: the input buffer changed'
    else:
        g = (w + 2) * ld_in
        assert torch.equal(bits(xin._guard_buf)[:g], before_in[:g]) and torch.equal(bits(xin._guard_buf)[-g:], before_in[-g:]), f'{name}: guards changed'
    if has1:
        assert torch.equal(bits(res1), res1_before), f'{name}: res1 changed'


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize('cin', CINS)
@pytest.mark.parametrize('cout', COUTS)
def test_every_width_and_epilogue(cin, cout):
    """all five cin against both cout, each epilogue form, out inside the input buffer where it fits and in a second buffer, both poisons"""
    for i, form in enumerate(FORMS):
        for place in ('inplace', 'second'):
            if place == 'inplace' and cin + cout > LD:
                continue
            run_case(2, 8, 16, cin, cout, form, 100 + i, place, poison='inf' if (i + (place == 'second')) % 2 else 'nan')


@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
def test_geometries(geom):
    """every geometry class on the dense block's own five convolutions (in place for 1 to 4, the residual forms for 5)"""
    n, h, w = geom
    big = h * w >= 8192
    for k, (cin, cout, form, place) in enumerate([(64, 32, 'slope', 'inplace'), (96, 32, 'slope', 'inplace'), (128, 32, 'plain', 'inplace'),
                                                   (160, 32, 'slope', 'inplace'), (192, 64, 'res1', 'second'), (192, 64, 'res2', 'second'),
                                                   (64, 64, 'slope_res2', 'second')]):
        if big and k not in (1, 5):          # the widest input: one in-place and one residual case (the fp64 reference is the cost)
            continue
        run_case(n, h, w, cin, cout, form, 200 + k, place, poison='nan' if k % 2 else 'inf')


@pytest.mark.parametrize('geom', [(2, 4, 6), (1, 8, 24), (3, 2, 4), (1, 4, 40)], ids=lambda g: 'x'.join(map(str, g)))
def test_upsample(geom):
    """nearest-2x folded into the gather (conv_up1 / conv_up2): cin = 64, both widths"""
    n, h, w = geom
    run_case(n, h, w, 64, 64, 'slope', 300, 'second', ups=True)
    run_case(n, h, w, 64, 32, 'res1', 301, 'second', poison='nan', ups=True)


def test_clipped_tiles():
    """sizes that are no multiple of the 8 x 32 tile, in both directions, and a single pixel"""
    for n, h, w in [(2, 5, 9), (1, 9, 33), (1, 1, 1), (2, 3, 70)]:
        run_case(n, h, w, 96, 32, 'slope', 400, 'inplace')
        run_case(n, h, w, 192, 64, 'res2', 401, 'second', poison='nan')


# ------------------------------------------------------------------------------------------------ the network's coefficients
@pytest.mark.parametrize('form', ['rdb5', 'rrdb5'])
def test_network_coefficients(form):
    """alpha = 0.2, c1 = 1 (an RDB's conv5) and alpha = 0.04, c1 = 0.2, res2 aliasing out (the third RDB's): random fp16 data against fp64"""
    n, h, w, cin, cout = 2, 16, 24, 192, 64
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(n, h, w, cin, generator=gen) * 0.5).half()
    wt = (torch.randn(cout, 9 * cin, generator=gen) * (9 * cin) ** -0.5).half()
    bias = torch.randn(cout, generator=gen) * 0.1
    r1 = torch.randn(n, h, w, cout, generator=gen).half()
    r2 = torch.randn(n, h, w, cout, generator=gen).half()
    alpha, c1 = (0.2, 1.0) if form == 'rdb5' else (0.04, 0.2)
    w3 = wt.double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    acc = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w3, bias.double(), padding=1).permute(0, 2, 3, 1)
    ref = alpha * acc + c1 * r1.double() + (r2.double() if form == 'rrdb5' else 0)
    dv = dev()
    xin = cc.guarded_nhwc(x, dv)
    out = r2.to(dv).clone()
    ops.dense_conv(xin, wt.to(dv), bias.to(dv), out, n=n, h=h, wd=w, cin=cin, cout=cout, ld_in=cin, ld_out=cout, alpha=alpha, res1=r1.to(dv),
                   ld_res1=cout, c1=c1, res2=out if form == 'rrdb5' else None, ld_res2=cout)
    check_close(out.reshape(-1, cout), ref.reshape(-1, cout), name=form)
    cc.guards_intact(xin)


# ------------------------------------------------------------------------------------------------ refusals
def _valid():
    dv = dev()
    n, h, w, cin, cout = 1, 8, 8, 64, 32
    buf = torch.zeros(n, h, w, LD, dtype=torch.float16, device=dv)
    other = torch.zeros(n, h, w, LD, dtype=torch.float16, device=dv)
    wt = torch.zeros(cout, 9 * cin, dtype=torch.float16, device=dv)
    bias = torch.zeros(cout, dtype=torch.float32, device=dv)
    kw = dict(n=n, h=h, wd=w, cin=cin, cout=cout, ld_in=LD, ld_out=LD, out_col=cin, alpha=1.0, slope=0.2)
    return buf, other, wt, bias, kw


REFUSALS = {
    'null input': lambda b, o, w, bi, kw: (None, w, bi, b, kw),
    'null weight': lambda b, o, w, bi, kw: (b, None, bi, b, kw),
    'null output': lambda b, o, w, bi, kw: (b, w, bi, None, kw),
    'misaligned input': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, in_off=4, out_col=0)),
    'misaligned output': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, out_off=4, out_col=0)),
    'misaligned residual': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, res1=o, res1_off=4, ld_res1=LD, c1=1.0)),
    'cin 80': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, cin=80, out_col=80)),
    'cin 224': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, cin=224, ld_in=224, out_col=0)),
    'cout 48': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, cout=48)),
    'cout 16': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, cout=16)),
    'ld_in not a multiple of 8': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, ld_in=100, out_col=0)),
    'ld_in below cin': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, ld_in=56, out_col=0)),
    'ld_out not a multiple of 8': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, ld_out=100, out_col=0)),
    'ld_res1 not a multiple of 8': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, res1=o, ld_res1=36, c1=1.0)),
    'out_col not a multiple of 8': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, out_col=68)),
    'slice beyond the row': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, out_col=168)),
    'zero height': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, h=0)),
    'negative width': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, wd=-8)),
    'zero images': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, n=0)),
    'too many pixels': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, n=65535, h=16384, wd=16384, out_col=0)),
    'upsample 2': lambda b, o, w, bi, kw: (b, w, bi, o, dict(kw, upsample=2, out_col=0)),
    'upsample in place': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, upsample=1)),
    'written slice inside the channels read': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, out_col=32)),
    'written slice straddles the channels read': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, out_col=48)),
    'output shifted onto the input by pixels': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, out_off=LD, n=1, h=4, out_col=0)),
    'other stride over the input': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, ld_out=96, out_col=64)),
    'non-finite alpha': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, alpha=float('nan'))),
    'non-finite slope': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, slope=float('inf'))),
    'residual partially over the written slice': lambda b, o, w, bi, kw: (b, w, bi, b, dict(kw, res2=b, res2_off=cin_of(kw) + 8, ld_res2=LD)),
}


def cin_of(kw):
    return kw['cin']


@pytest.mark.parametrize('why', list(REFUSALS))
def test_refusals(why):
    """every bad argument returns an error with a message and leaves both buffers untouched"""
    buf, other, wt, bias, kw = _valid()
    assert ops.dense_conv_ok(buf, wt, bias, buf, **kw) == 1            # the descriptor the refusals are derived from is taken
    for t in (buf, other):
        t.fill_(3.0)
    inp, w, bi, out, kw2 = REFUSALS[why](buf, other, wt, bias, kw)
    assert ops.dense_conv_ok(inp, w, bi, out, **kw2) == 0, why
    with pytest.raises(_lib.SdodError) as e:
        ops.dense_conv(inp, w, bi, out, **kw2)
    assert str(e.value), why
    torch.cuda.synchronize()
    assert bool((buf == 3.0).all()) and bool((other == 3.0).all()), f'{why}: a refused call wrote to a buffer'


# ------------------------------------------------------------------------------------------------ conv_first
def test_image_conv_in_unit_border_and_copy():
    """conv_first on u / 255 with the zero border in that space: fp64 reference on the fp16-rounded input; the second copy (pixel
    stride 192) equals the first bit for bit and leaves the other channels alone; the border differs from the encoder's normalisation"""
    gen = torch.Generator().manual_seed(11)
    n, h, w, cout = 2, 9, 13, 64
    img = torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8)
    wt = (torch.randn(cout, 3, 3, 3, generator=gen) * 27 ** -0.5).half()
    bias = torch.randn(cout, generator=gen) * 0.1
    packed = torch.zeros(cout, 64, dtype=torch.float16)
    packed[:, :27] = wt.permute(0, 2, 3, 1).reshape(cout, 27)
    dv = dev()
    wide = torch.full((n, h, w, LD), float('nan'), dtype=torch.float16, device=dv)
    y = ops.image_conv_in_unit(img.to(dv), packed.to(dv), bias.to(dv), out2=wide)
    x = (img.float() / 255.0).half().double().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x, wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
    check_close(y.reshape(-1, cout), ref.reshape(-1, cout), name='conv_first')
    assert torch.equal(bits(wide[..., :cout]), bits(y)) and bool(torch.isnan(wide[..., cout:]).all())
    signed = ops.image_conv_in(img.to(dv), (packed / 2).to(dv), (bias + wt.float().sum(dim=(1, 2, 3)) / 2).to(dv)).float().cpu()
    diff = (signed - y.float().cpu()).abs()
    assert float(diff[:, 1:-1, 1:-1].max()) < 2e-2 and float(diff[:, 0].max()) > 0.1, (float(diff[:, 1:-1, 1:-1].max()), float(diff[:, 0].max()))
