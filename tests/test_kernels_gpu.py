"""GPU parity tests of the individual gfx950 kernels, called through the C ABI (lib/libsdod.so).

Checker: plain PyTorch fp32 on the CPU of the same op on the same fp16-rounded inputs.
Tolerances (stated, fp16 in/out with fp32 accumulation): rel-L2 <= 2e-3 per kernel,
max-abs <= 2e-2 * max|ref|; integer / exact paths are compared bit-for-bit.

The kernels that reduce along a row (LayerNorm stand-alone and folded into the GEMMs, softmax_rows, the score GEMM's softmax
epilogue) and the activation functions meet only Gaussian rows of unit scale here; tests/test_row_kernels_gpu.py holds them to
fp64 on the rows that can see eps, a lost row maximum, misplaced statistics, flushed subnormals and a wrong coefficient."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gemm_cases import check_close as check, geglu_perm, run_gemm, tile_info, u8_tile

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def tgemm(*args, **kw):
    """ops.gemm on a named tile through tests/gemm_cases.run_gemm, which asks sdod_gemm_plan what the descriptor ran on and
    asserts it: the requested tile, or `runs_on=`, the substitute make_plan documents (a changed fallback is a test change)"""
    kw.setdefault('tag', 'kernels')
    return run_gemm(*args, **kw)[0]


def has_u8_form(tile):
    """a uint8-weight GEMM planned on this tile stays on it (the plan's answer; the others run on the fallback tile, 23)"""
    return tile > 0 and u8_tile(tile) == tile


def wave80(tile):
    """a wave owns 80 columns (one head): an odd number of 16-column blocks, so the GEGLU epilogue cannot pair value and gate"""
    i = tile_info(tile)
    return i['family'] == 'ring' and i['bn'] // i['wn'] == 80


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).half()


def test_library_and_device():
    from sdod.amd import ops
    info = ops.device_info()
    assert info['arch'].startswith('gfx950'), info
    assert info['cu_count'] == 256


# ------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize('m,n,k,tile', [
    (256, 128, 64, 1), (256, 128, 128, 2), (200, 72, 192, 3), (512, 16, 128, 4), (100, 136, 64, 5),
    (256, 128, 64, 6), (300, 200, 128, 6), (8192, 320, 320, 6), (256, 128, 192, 7), (333, 72, 640, 7), (200, 72, 64, 8),
    (1000, 320, 1280, 8), (128, 1280, 1280, 6), (128, 1280, 1280, 8),
    (300, 200, 128, 9), (8192, 320, 320, 9), (300, 200, 192, 10), (1000, 320, 1280, 10), (333, 72, 640, 11), (700, 136, 256, 12),
    (8192, 320, 320, 0), (333, 320, 640, 0), (128, 1280, 1280, 0), (77 * 2, 768, 768, 0), (4096, 4, 64, 0),
    (1000, 3, 1152, 0),
    # wave-specialised tiles (4 consumer + 4 loader waves): 23/24 128x128, 25 128x256, 26 256x128, 27/28 64x64, 29 128x64, 30 64x128, 31 64x160
    (300, 200, 128, 23), (8192, 320, 320, 23), (8192, 320, 320, 24), (1000, 320, 1280, 25), (700, 136, 256, 26), (128, 1280, 1280, 27),
    (200, 72, 64, 28), (333, 72, 640, 29), (100, 136, 64, 30), (8192, 320, 320, 31), (300, 200, 192, 31),
    # two slabs per barrier (32 64x64, 33 128x64, 34 64x128, 35 64x160, 36 128x128): odd and even slab counts, K = 64
    (200, 72, 64, 32), (128, 1280, 1280, 32), (333, 72, 704, 32), (333, 72, 640, 33), (100, 136, 192, 34), (8192, 320, 320, 35),
    (300, 200, 192, 35), (1000, 320, 1280, 36), (300, 200, 448, 36),
    # 32-row wave-specialised tiles (46 32x64, 47 32x128, 48 32x160)
    (512, 1280, 1280, 46), (100, 72, 64, 46), (512, 1280, 1280, 47), (70, 136, 192, 47), (512, 1280, 1280, 48), (333, 200, 640, 48),
])
def test_gemm_rows(m, n, k, tile):
    from sdod.amd import ops
    a = rnd((m, k), 1); w = rnd((n, k), 2, k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(3))
    res = rnd((m, n), 4)
    ref = F.silu(1.25 * (a.float() @ w.float().t()) + bias).half().float() + res.float()
    d = dev()
    # tile 0: the plan's own choice -- the skinny 256x16 tile for N <= 16, else the largest of 128x128 / 128x64 / 64x64 that
    # still makes 384 workgroups (none does here: 64x64)
    out = tgemm(a.to(d), w.to(d), bias.to(d), residual=res.to(d), act='silu', alpha=1.25, tile=tile,
                runs_on=tile or (4 if n <= 16 else 3))
    torch.cuda.synchronize()
    check(out, ref, name=f'gemm {m}x{n}x{k} tile{tile}')


@pytest.mark.parametrize('tile', [0, 8, 13, 20, 21, 23, 24, 27, 28, 29, 30, 31])
@pytest.mark.parametrize('case', ['rows', 'rows_split', 'conv', 'geglu'])
def test_gemm_uint8_weight_streaming(case, tile):
    """int8 weight path of BASELINE config 5: W stays affine-uint8 in memory (the reference's QNN encoding real = (q + offset) * scale,
    qnn_context.cpp:1018-1033), per-column (scale, offset) so that fused parameter groups can mix tensors; the reference for
    the check is the fp32 product with the DEQUANTISED weights."""
    g = torch.Generator().manual_seed(130)
    d = dev()
    # make_plan: a tile without a uint8 form (0, 20, 21 here) runs on tile 23; with GEGLU the wave-80 tiles (21, 31) first go to
    # tile 14, which has no uint8 form either
    runs_on = tile if has_u8_form(tile) and not (case == 'geglu' and wave80(tile)) else 23

    def quant(n, k):
        q = torch.randint(0, 256, (n, k), generator=g, dtype=torch.uint8)
        scale = (torch.rand(n, generator=g) * 0.5 + 0.75) * 2.0 / 255 * k ** -0.5        # two "tensors" with different encodings
        offset = torch.where(torch.arange(n) < n // 2, torch.tensor(-128.0), torch.tensor(-101.0))
        scale = torch.where(torch.arange(n) < n // 2, scale, scale * 1.7)
        wf = (q.float() + offset[:, None]) * scale[:, None]
        return q, scale.float(), (offset + 128).float(), wf

    if case in ('rows', 'rows_split'):
        m, n, k = (600, 320, 1280) if case == 'rows' else (128, 1280, 2560)
        a = rnd((m, k), 131)
        q, sc, of, wf = quant(n, k)
        bias = torch.randn(n, generator=g); res = rnd((m, n), 132)
        ref = (a.float() @ wf.t() + bias).half().float() + res.float()
        out = tgemm(a.to(d), q.to(d), bias.to(d), residual=res.to(d), w_scale=sc.to(d), w_off=of.to(d), tile=tile, runs_on=runs_on,
                    split_k=4 if case == 'rows_split' else 1)
    elif case == 'conv':
        nb, h, w_, cin, cout = 2, 16, 16, 128, 192
        x = rnd((nb, h, w_, cin), 133)
        q, sc, of, wf = quant(cout, 9 * cin)
        bias = torch.randn(cout, generator=g)
        ref = conv_ref(x, wf.half(), bias) if False else F.conv2d(x.float().permute(0, 3, 1, 2), wf.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), bias, padding=1).permute(0, 2, 3, 1)
        out = tgemm(x.to(d), q.to(d), bias.to(d), conv=dict(stride=1), w_scale=sc.to(d), w_off=of.to(d), tile=tile, runs_on=runs_on)
    else:
        m, c = 300, 320
        x = rnd((m, c), 134)
        q, sc, of, wf = quant(8 * c, c)
        b = torch.randn(8 * c, generator=g)
        y = x.float() @ wf.t() + b
        H = 4 * c
        ref = y[:, :H] * F.gelu(y[:, H:])
        perm = geglu_perm(H)
        out = tgemm(x.to(d), q[perm].contiguous().to(d), b[perm].contiguous().to(d), geglu=True, w_scale=sc[perm].contiguous().to(d),
                    w_off=of[perm].contiguous().to(d), tile=tile, runs_on=runs_on)
    check(out, ref, name=f'uint8 weights {case} tile{tile}')


@pytest.mark.parametrize('tile', [0, 6, 8, 9, 10, 17, 20, 21, 22, 23, 25, 27, 29, 31, 32, 33, 35, 36, 46, 47, 48])
@pytest.mark.parametrize('split', [2, 5, 16])
def test_gemm_split_k(split, tile):
    from sdod.amd import ops
    m, n, k = 128, 320, 2880
    a = rnd((m, k), 5); w = rnd((n, k), 6, k ** -0.5)
    bias = torch.randn(n, generator=torch.Generator().manual_seed(7))
    rb = torch.randn(2, n, generator=torch.Generator().manual_seed(8)).half()
    ref = a.float() @ w.float().t() + bias + rb.float().repeat_interleave(64, 0)
    d = dev()
    out = tgemm(a.to(d), w.to(d), bias.to(d), row_bias=rb.to(d), rows_per_img=64, split_k=split, tile=tile, runs_on=tile or 3)   # 0: the plan's 64x64
    check(out, ref, name=f'splitk {split} tile{tile}')


def test_gemm_bias_on_m_and_gelu():
    from sdod.amd import ops
    m, n, k = 512, 256, 512
    a = rnd((m, k), 9); w = rnd((n, k), 10, k ** -0.5)
    bias = torch.randn(m, generator=torch.Generator().manual_seed(11))
    d = dev()
    out = ops.gemm(a.to(d), w.to(d), bias.to(d), bias_on_m=True, act='gelu')
    check(out, F.gelu(a.float() @ w.float().t() + bias[:, None]), name='bias_on_m gelu')
    out = ops.gemm(a.to(d), w.to(d), None, act='quick_gelu')
    x = a.float() @ w.float().t()
    check(out, x * torch.sigmoid(1.702 * x), name='quick_gelu')


def conv_ref(x_nhwc, w_krsc, bias, stride=1, upsample=False):
    x = x_nhwc.float().permute(0, 3, 1, 2)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode='nearest')
    cout = w_krsc.shape[0]
    w = w_krsc.float().reshape(cout, 3, 3, -1).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, bias, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('tile', [0, 6, 7, 8, 9, 10, 11, 12, 13, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 46, 47, 48])
@pytest.mark.parametrize('n,h,w,cin,cout,stride,ups', [
    (2, 16, 16, 64, 128, 1, False), (1, 9, 7, 128, 64, 1, False), (2, 16, 16, 64, 64, 2, False),
    (1, 8, 8, 128, 128, 1, True), (2, 64, 64, 320, 320, 1, False), (2, 8, 8, 1280, 1280, 1, False),
    (1, 7, 7, 64, 64, 2, False),
])
def test_conv3x3(n, h, w, cin, cout, stride, ups, tile):
    from sdod.amd import ops
    x = rnd((n, h, w, cin), 20); wt = rnd((cout, 9 * cin), 21, (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(22))
    ref = conv_ref(x, wt, bias, stride, ups)
    d = dev()
    out = tgemm(x.to(d), wt.to(d), bias.to(d), conv=dict(stride=stride, upsample=ups), tile=tile, runs_on=tile or 3)   # 0: the plan's 64x64
    check(out, ref, name=f'conv {n}x{h}x{w} {cin}->{cout} s{stride} u{ups} tile{tile}')


def test_conv3x3_concat_rowbias_residual():
    from sdod.amd import ops
    n, h, w, c0, c1, cout = 2, 16, 16, 128, 64, 192
    x0 = rnd((n, h, w, c0), 30); x1 = rnd((n, h, w, c1), 31)
    wt = rnd((cout, 9 * (c0 + c1)), 32, (9 * (c0 + c1)) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(33))
    rb = torch.randn(n, cout, generator=torch.Generator().manual_seed(34)).half()
    res = rnd((n, h, w, cout), 35)
    ref = conv_ref(torch.cat([x0, x1], -1), wt, bias) + rb.float()[:, None, None, :]
    ref = ref.half().float() + res.float()
    d = dev()
    for tile in (0, 6, 7, 8, 9, 10, 11, 12, 17, 18, 19, 20, 21, 22):
        out = tgemm(x0.to(d), wt.to(d), bias.to(d), a2=x1.to(d), conv=dict(stride=1), row_bias=rb.to(d), rows_per_img=h * w,
                    residual=res.to(d), tile=tile, runs_on=tile or 3)
        check(out, ref, name=f'conv concat tile{tile}')


def test_conv1x1_two_sources():
    """1x1 skip convolution of a ResBlock whose input is a channel concat (h, skip) -- no concat tensor in HBM."""
    from sdod.amd import ops
    n, h, w, c0, c1, cout = 2, 8, 8, 1280, 640, 1280
    x0 = rnd((n, h, w, c0), 36); x1 = rnd((n, h, w, c1), 37)
    wt = rnd((cout, c0 + c1), 38, (c0 + c1) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(39))
    ref = torch.cat([x0, x1], -1).float() @ wt.float().t() + bias
    d = dev()
    out = ops.gemm(x0.to(d), wt.to(d), bias.to(d), a2=x1.to(d), conv=dict(stride=1, ksize=1))
    check(out, ref, name='conv1x1 concat')


@pytest.mark.parametrize('tile', [0, 6, 8, 10, 13, 14, 16, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 34, 36, 46, 47, 48, 57, 59, 61])
def test_gemm_fused_geglu(tile):
    """ff.net.0.proj + GEGLU in one launch: weight rows interleaved in 16-row [value | gate] blocks (tiles 21/22 cannot
    pair value and gate inside one wave: the planner must fall back, not skip the epilogue)"""
    from sdod.amd import ops
    m, c = 600, 320
    x = rnd((m, c), 90); w = rnd((8 * c, c), 91, c ** -0.5); b = torch.randn(8 * c, generator=torch.Generator().manual_seed(92))
    y = x.float() @ w.float().t() + b
    ref = y[:, :4 * c] * F.gelu(y[:, 4 * c:])
    H = 4 * c
    perm = geglu_perm(H)
    d = dev()
    # make_plan: fusions live in the LDS-DMA families (0 -> 14), and a wave that owns 80 columns cannot pair value and gate
    # (21, 22, 31, 48, 57, 59 -> 14)
    out = tgemm(x.to(d), w[perm].contiguous().to(d), b[perm].contiguous().to(d), geglu=True, tile=tile,
                runs_on=14 if tile == 0 or wave80(tile) else tile)
    assert out.shape == (m, H)
    check(out, ref, name=f'fused geglu tile{tile}')


@pytest.mark.parametrize('tile', [0, 6, 8, 11, 14, 18, 20, 21, 22, 23, 25, 26, 27, 28, 30, 31, 32, 33, 35, 36, 46, 47, 48, 56, 57, 58, 59, 60, 61])
@pytest.mark.parametrize('m,c,n', [(600, 320, 960), (8192, 320, 320), (200, 1280, 1280)])
def test_gemm_with_folded_layer_norm(tile, m, c, n):
    """LayerNorm -> Linear in one launch: row statistics gathered inside the GEMM, gamma folded into W"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(100)
    x = (torch.randn(m, c, generator=g) * 2 + torch.randn(m, 1, generator=g) * 3).half()     # per-row offsets
    w = rnd((n, c), 101, c ** -0.5)
    gamma = 1 + 0.2 * torch.randn(c, generator=g); beta = 0.3 * torch.randn(c, generator=g); bias = torch.randn(n, generator=g)
    ref = F.layer_norm(x.float(), (c,), gamma, beta, 1e-5) @ w.float().t() + bias
    d = dev()
    wf, s, t = ops.ln_fold(w.clone().to(d), gamma.to(d), beta.to(d), bias.to(d))
    out = tgemm(x.to(d), wf, t, ln_s=s, tile=tile, runs_on=tile or 14)   # 0: fusions live in the LDS-DMA families
    check(out, ref, tol=3e-3, name=f'ln-folded gemm {m}x{c}->{n} tile{tile}')


def test_gemm_ln_fold_with_geglu():
    from sdod.amd import ops
    g = torch.Generator().manual_seed(102)
    m, c = 500, 320
    H = 4 * c
    x = (torch.randn(m, c, generator=g) + 1.5).half()
    w = rnd((2 * H, c), 103, c ** -0.5); b = torch.randn(2 * H, generator=g)
    gamma = 1 + 0.2 * torch.randn(c, generator=g); beta = 0.3 * torch.randn(c, generator=g)
    y = F.layer_norm(x.float(), (c,), gamma, beta, 1e-5) @ w.float().t() + b
    ref = y[:, :H] * F.gelu(y[:, H:])
    perm = geglu_perm(H)
    d = dev()
    wf, s, t = ops.ln_fold(w[perm].contiguous().to(d), gamma.to(d), beta.to(d), b[perm].contiguous().to(d))
    for tile in (0, 14, 61):
        out = tgemm(x.to(d), wf, t, ln_s=s, geglu=True, tile=tile, runs_on=tile or 14)
        check(out, ref, tol=3e-3, name=f'ln-fold + geglu tile{tile}')


PANEL_TILES = {53: 320, 54: 640, 55: 1280}      # A-panel tiles and the K whose 80 KB row panel they are sized for


@pytest.mark.parametrize('case', ['plain', 'ln', 'geglu', 'ln_geglu', 'residual_bias', 'ragged', 'short_k'])
@pytest.mark.parametrize('tile', sorted(PANEL_TILES))
def test_gemm_apanel_tiles(tile, case):
    """gemm_apanel_kernel (tiles 53..55: a row panel x the whole K resident in LDS, the n-tiles of a workgroup streamed past
    it): every epilogue it carries -- LayerNorm fold, GEGLU, bias, residual -- on M / N that do not divide the tiles, several
    n-tiles per workgroup (the ring runs across tile boundaries) and more groups than n-tiles; bit-identical from launch to
    launch"""
    from sdod.amd import ops
    c = PANEL_TILES[tile] if case != 'short_k' else 192
    g = torch.Generator().manual_seed(400 + tile)
    m = {'plain': 8192 if tile == 53 else 2048, 'ln': 1000, 'geglu': 600, 'ln_geglu': 517, 'residual_bias': 777, 'ragged': 333, 'short_k': 300}[case]
    n = {'plain': 3 * c, 'ln': 3 * c, 'geglu': 8 * c if tile != 55 else 2560, 'ln_geglu': 2560, 'residual_bias': c, 'ragged': 200, 'short_k': 1024}[case]
    x = (torch.randn(m, c, generator=g) * 1.5 + torch.randn(m, 1, generator=g)).half()
    w = rnd((n, c), 410 + tile, c ** -0.5)
    bias = torch.randn(n, generator=g)
    d = dev()
    kw = dict(tile=tile)
    if case in ('ln', 'ln_geglu'):
        gamma = 1 + 0.2 * torch.randn(c, generator=g); beta = 0.3 * torch.randn(c, generator=g)
        y = F.layer_norm(x.float(), (c,), gamma, beta, 1e-5) @ w.float().t() + bias
    else:
        y = x.float() @ w.float().t() + (bias if case != 'plain' else 0)
    wd, bd = w, bias
    if case in ('geglu', 'ln_geglu'):
        H = n // 2
        ref = y[:, :H] * F.gelu(y[:, H:])
        perm = geglu_perm(H)
        wd, bd = w[perm].contiguous(), bias[perm].contiguous()
        kw['geglu'] = True
    else:
        ref = y
    if case in ('ln', 'ln_geglu'):
        wf, sv, tv = ops.ln_fold(wd.clone().to(d), gamma.to(d), beta.to(d), bd.to(d))
        run = lambda: tgemm(x.to(d), wf, tv, ln_s=sv, **kw)
    elif case == 'residual_bias':
        res = rnd((m, n), 420 + tile)
        ref = ref + res.float()
        run = lambda: tgemm(x.to(d), wd.to(d), bd.to(d), residual=res.to(d), **kw)
    elif case == 'plain':
        run = lambda: tgemm(x.to(d), wd.to(d), **kw)
    else:
        run = lambda: tgemm(x.to(d), wd.to(d), bd.to(d), **kw)
    out = run().clone()
    check(out, ref, tol=3e-3, name=f'a-panel tile{tile} {case} M{m} N{n} K{c}')
    for _ in range(3):
        assert torch.equal(run(), out), 'launch-to-launch difference'


def test_apanel_tiles_reject_what_they_cannot_run():
    from sdod.amd import ops, _lib
    d = dev()
    x = rnd((256, 1280), 430).to(d); w = rnd((256, 1280), 431).to(d)
    with pytest.raises(_lib.SdodError):
        tgemm(x, w, tile=53)                     # a 128-row panel of K = 1280 is 320 KB
    x0 = rnd((2, 16, 16, 64), 432).to(d); w0 = rnd((64, 576), 433).to(d)
    with pytest.raises(_lib.SdodError):
        tgemm(x0, w0, conv=dict(stride=1), tile=54)      # convolutions: never


@pytest.mark.parametrize('tile', [0, 7, 9, 12, 14, 23, 26, 27, 31, 32, 36, 46, 48])
def test_conv3x3_with_skip_tail_segment(tile):
    """ResBlock: out_layers.3 (3x3 on h) + skip_connection (1x1 on the concatenated block input) as ONE GEMM"""
    from sdod.amd import ops
    n, h, w, cmid, c0, c1 = 2, 16, 16, 128, 128, 64
    hmid = rnd((n, h, w, cmid), 93); x0 = rnd((n, h, w, c0), 94); x1 = rnd((n, h, w, c1), 95)
    w3 = rnd((cmid, 9 * cmid), 96, (9 * cmid) ** -0.5); w1 = rnd((cmid, c0 + c1), 97, (c0 + c1) ** -0.5)
    b3 = torch.randn(cmid, generator=torch.Generator().manual_seed(98)); b1 = torch.randn(cmid, generator=torch.Generator().manual_seed(99))
    ref = conv_ref(hmid, w3, b3) + (torch.cat([x0, x1], -1).float() @ w1.float().t() + b1)
    d = dev()
    wcat = torch.cat([w3, w1], 1).contiguous()
    out = tgemm(hmid.to(d), wcat.to(d), b3.to(d), conv=dict(stride=1), tail=(x0.to(d), x1.to(d)), bias2=b1.to(d), tile=tile,
                runs_on=tile or 14)   # 0: fusions live in the LDS-DMA families
    check(out, ref, name=f'conv + skip tail tile{tile}')


@pytest.mark.parametrize('case', ['rows_small_m', 'rows_ragged', 'rows_geglu_ln', 'conv', 'conv_split', 'halo', 'halo_split_tail', 'conv_rect',
                                  'halo_rect'])
def test_xcd_tile_orders_give_identical_bits(case):
    """sdod_gemm_desc::xcd_panels only permutes which workgroup computes which tile (gemm.hip: tile_of): every order --
    the per-shape choice, m-major, 2 / 4 / 8 panels, ragged panel widths included -- must produce the same bits"""
    from sdod.amd import ops
    d = dev()
    if case == 'rows_small_m':
        a = rnd((512, 1280), 300).to(d); w = rnd((1280, 1280), 301, 1280 ** -0.5).to(d)
        run = lambda x: tgemm(a, w, tile=28, xcd=x)                                   # 8 x 20 tiles
        ref = a.float().cpu() @ w.float().cpu().t()
    elif case == 'rows_ragged':
        a = rnd((333, 704), 302).to(d); w = rnd((200, 704), 303, 704 ** -0.5).to(d)     # 6 x 4 tiles of 64 x 64, ragged M and N
        res = rnd((333, 200), 304).to(d)
        run = lambda x: tgemm(a, w, residual=res, tile=32, xcd=x)
        ref = a.float().cpu() @ w.float().cpu().t() + res.float().cpu()
    elif case == 'rows_geglu_ln':
        a = rnd((600, 320), 305).to(d); w = rnd((2560, 320), 306, 320 ** -0.5).to(d)
        gamma = (1 + 0.1 * torch.randn(320, generator=torch.Generator().manual_seed(307))).to(d)
        beta = (0.1 * torch.randn(320, generator=torch.Generator().manual_seed(308))).to(d)
        bias = torch.randn(2560, generator=torch.Generator().manual_seed(309)).to(d)
        wf, sv, tv = ops.ln_fold(w.clone(), gamma, beta, bias)
        run = lambda x: tgemm(a, wf, tv, geglu=True, ln_s=sv, tile=14, xcd=x)         # 5 x 20 tiles: 3 panels of 3 + ... ragged
        ref = None
    elif case in ('conv', 'conv_split'):
        x0 = rnd((2, 16, 16, 256), 310).to(d); w = rnd((320, 9 * 256), 311, (9 * 256) ** -0.5).to(d)
        run = lambda x: tgemm(x0, w, conv=dict(stride=1), tile=28, split_k=3 if case == 'conv_split' else 1, xcd=x)
        ref = conv_ref(x0.cpu(), w.cpu(), None)
    elif case == 'halo':
        x0 = rnd((2, 32, 32, 192), 312).to(d); w = rnd((400, 9 * 192), 313, (9 * 192) ** -0.5).to(d)
        run = lambda x: tgemm(x0, w, conv=dict(stride=1), tile=38, split_k=1, xcd=x)  # 16 x 5 tiles of 128 x 80
        ref = conv_ref(x0.cpu(), w.cpu(), None)
    elif case == 'conv_rect':
        x0 = rnd((2, 24, 16, 128), 319).to(d); w = rnd((200, 9 * 128), 320, (9 * 128) ** -0.5).to(d)
        run = lambda x: tgemm(x0, w, conv=dict(stride=1), tile=28, split_k=1, xcd=x)  # 768 rows x 200 columns, h != w
        ref = conv_ref(x0.cpu(), w.cpu(), None)
    elif case == 'halo_rect':
        x0 = rnd((2, 32, 48, 64), 321).to(d); w = rnd((200, 9 * 64), 322, (9 * 64) ** -0.5).to(d)
        run = lambda x: tgemm(x0, w, conv=dict(stride=1), tile=50, split_k=1, xcd=x)  # 32 x 4 tiles of 96 x 64: two image rows of 48 each
        ref = conv_ref(x0.cpu(), w.cpu(), None)
    else:
        hm = rnd((2, 16, 16, 128), 314).to(d); t0 = rnd((2, 16, 16, 192), 315).to(d)
        w = torch.cat([rnd((192, 9 * 128), 316, (9 * 128) ** -0.5), rnd((192, 192), 317, 192 ** -0.5)], 1).contiguous().to(d)
        b1 = torch.randn(192, generator=torch.Generator().manual_seed(318)).to(d)
        run = lambda x: tgemm(hm, w, conv=dict(stride=1), tail=(t0, None), bias2=b1, tile=44, split_k=2, xcd=x)
        ref = None
    base = run(0).clone()
    if ref is not None:
        check(base, ref.reshape(base.shape), name=f'xcd order {case}')
    for x in (1, 2, 4, 8):
        assert torch.equal(run(x), base), f'{case}: {x} panels differ from the per-shape order'


HALO_TILES = list(range(37, 46)) + [49, 50, 51, 52]   # 49..52: 96- / 192-row tiles (image rows that are multiples of 3: config 5)


_HALO_RAN = {}      # tile -> launches that ran (not skipped) in this session


def _halo_gemm(ops, *args, **kw):
    """a halo-patch tile may decline a geometry (tile rows must divide the image, patch must fit LDS): skip, do not fail --
    and count what ran, so that a planner that declines everything cannot pass for green (the check at the end of the halo
    tests; the CPU suite holds the per-tile acceptance table, tests/test_host_cabi.py)"""
    try:
        out = tgemm(*args, **kw)
    except Exception as ex:
        if 'halo-patch tile does not take' in str(ex):
            _HALO_RAN.setdefault(kw.get('tile'), 0)
            pytest.skip('tile declines this geometry')
        raise
    _HALO_RAN[kw.get('tile')] = _HALO_RAN.get(kw.get('tile'), 0) + 1
    return out


@pytest.mark.parametrize('split', [0, 1, 3])
@pytest.mark.parametrize('tile', HALO_TILES)
@pytest.mark.parametrize('n,h,w,cin,cout', [
    (2, 64, 64, 128, 320), (2, 32, 32, 192, 160), (2, 16, 16, 256, 256), (2, 8, 8, 320, 192), (1, 8, 8, 64, 64),
    (3, 8, 8, 128, 80), (1, 128, 128, 64, 128), (5, 16, 16, 64, 48),
    # SD v2.1-768 geometry (rows that are multiples of 3): only the 96- / 192-row tiles take these
    (2, 96, 96, 64, 160), (2, 48, 48, 128, 80), (2, 24, 24, 192, 128), (1, 12, 12, 64, 200), (3, 12, 12, 128, 64),
])
def test_conv3x3_halo_patch_tiles(n, h, w, cin, cout, tile, split):
    """conv_halo_kernel (input patch resident in LDS, K walked chunk-major / tap-minor) against the fp32 convolution:
    row-segment tiles (w >= BM), whole-row tiles, tiles spanning several images (and more images than the batch holds),
    ragged N, uneven loader shares (BN = 80), one / default / three split-K slices"""
    from sdod.amd import ops
    x = rnd((n, h, w, cin), 120); wt = rnd((cout, 9 * cin), 121, (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(122))
    d = dev()
    out = _halo_gemm(ops, x.to(d), wt.to(d), bias.to(d), conv=dict(stride=1), tile=tile, split_k=split)
    ref = conv_ref(x, wt, bias)
    check(out, ref, name=f'halo conv {n}x{h}x{w} {cin}->{cout} tile{tile} split{split}')
    # opt-in: a split-K plan reduced INSIDE the GEMM launch (last K slice to arrive at the tile's counter reduces; fix_counters in
    # include/sdod_hip.h) -- the same sum in the same order as splitk_reduce_kernel, so the same bits, also on a second launch
    # (the counters must be back at zero)
    for _ in range(2):
        one_launch = tgemm(x.to(d), wt.to(d), bias.to(d), conv=dict(stride=1), tile=tile, split_k=split, fixup=True)
        assert torch.equal(one_launch, out), 'in-kernel split-K reduce differs from splitk_reduce_kernel'


@pytest.mark.parametrize('split', [1, 2])
@pytest.mark.parametrize('tile', HALO_TILES)
@pytest.mark.parametrize('hw', [16, 24])
def test_conv3x3_halo_concat_rowbias_residual_tail(hw, tile, split):
    """everything a ResBlock asks of one launch: two-source channel concat, time-embedding row bias, SiLU-less epilogue with
    residual, and the fused 1x1 skip connection as the extra split-K slice (24 x 24: the 96- / 192-row tiles)"""
    from sdod.amd import ops
    n, h, w, c0, c1, cout = 2, hw, hw, 128, 64, 192
    x0 = rnd((n, h, w, c0), 130); x1 = rnd((n, h, w, c1), 131)
    wt = rnd((cout, 9 * (c0 + c1)), 132, (9 * (c0 + c1)) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(133))
    rb = torch.randn(n, cout, generator=torch.Generator().manual_seed(134)).half()
    res = rnd((n, h, w, cout), 135)
    ref = conv_ref(torch.cat([x0, x1], -1), wt, bias) + rb.float()[:, None, None, :]
    ref = ref.half().float() + res.float()
    d = dev()
    out = _halo_gemm(ops, x0.to(d), wt.to(d), bias.to(d), a2=x1.to(d), conv=dict(stride=1), row_bias=rb.to(d), rows_per_img=h * w,
                     residual=res.to(d), tile=tile, split_k=split)
    check(out, ref, name=f'halo conv concat tile{tile} split{split}')
    # conv2 + skip tail (k_tail): out = conv3x3(hmid) + b3 + [x0 | x1] @ w1^T + b1
    cmid = 128
    hmid = rnd((n, h, w, cmid), 136)
    w3 = rnd((cmid, 9 * cmid), 137, (9 * cmid) ** -0.5); w1 = rnd((cmid, c0 + c1), 138, (c0 + c1) ** -0.5)
    b3 = torch.randn(cmid, generator=torch.Generator().manual_seed(139)); b1 = torch.randn(cmid, generator=torch.Generator().manual_seed(140))
    ref = conv_ref(hmid, w3, b3) + (torch.cat([x0, x1], -1).float() @ w1.float().t() + b1)
    wcat = torch.cat([w3, w1], 1).contiguous()
    out = _halo_gemm(ops, hmid.to(d), wcat.to(d), b3.to(d), conv=dict(stride=1), tail=(x0.to(d), x1.to(d)), bias2=b1.to(d), tile=tile, split_k=split)
    check(out, ref, name=f'halo conv + skip tail tile{tile} split{split}')
    one_launch = tgemm(hmid.to(d), wcat.to(d), b3.to(d), conv=dict(stride=1), tail=(x0.to(d), x1.to(d)), bias2=b1.to(d), tile=tile, split_k=split, fixup=True)
    assert torch.equal(one_launch, out)


@pytest.mark.parametrize('split', [0, 2])
@pytest.mark.parametrize('tile', HALO_TILES)
@pytest.mark.parametrize('n,h,w,cin,cout', [(2, 32, 32, 128, 160), (2, 16, 16, 192, 128), (1, 8, 8, 128, 128), (3, 4, 4, 64, 80), (1, 64, 64, 64, 64),
                                            (2, 48, 48, 64, 80), (2, 12, 12, 128, 128), (1, 24, 24, 64, 64)])
def test_conv3x3_halo_patch_tiles_with_upsampling(n, h, w, cin, cout, tile, split):
    """Upsample.conv: nearest-2x folded into the halo-patch kernel -- the patch is cut from the low-resolution source and the
    per-tap fragment addresses map output (y, x) onto source (y >> 1, x >> 1)"""
    from sdod.amd import ops
    x = rnd((n, h, w, cin), 150); wt = rnd((cout, 9 * cin), 151, (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(152))
    d = dev()
    out = _halo_gemm(ops, x.to(d), wt.to(d), bias.to(d), conv=dict(stride=1, upsample=True), tile=tile, split_k=split)
    ref = conv_ref(x, wt, bias, 1, True)
    check(out, ref, name=f'halo upconv {n}x{h}x{w} {cin}->{cout} tile{tile} split{split}')


@pytest.mark.parametrize('split', [0, 1, 3])
@pytest.mark.parametrize('tile', HALO_TILES)
@pytest.mark.parametrize('case', ['plain64', 'plain16', 'images8', 'resblock', 'upsample', 'rows48', 'resblock24'])
def test_conv3x3_halo_patch_uint8_weights(case, tile, split):
    """config 5 through the halo-patch kernel: the weight slabs stream as affine-uint8 codes (64-byte rows), the zero point is
    folded into the fragment expansion (q + offset is an exact fp16 integer) and the per-column scale into the epilogue;
    reference = fp32 convolution with the DEQUANTISED weights.  Two encodings inside one launch (fused parameter groups),
    ragged N, concat + row bias + residual, nearest-2x upsampling, split-K."""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(160)
    n, h, w, c0, c1, cout, ups = {'plain64': (2, 64, 64, 128, 0, 320, False), 'plain16': (2, 16, 16, 256, 0, 200, False),
                                  'images8': (3, 8, 8, 128, 0, 80, False), 'resblock': (2, 16, 16, 128, 64, 192, False),
                                  'upsample': (2, 16, 16, 192, 0, 128, True), 'rows48': (2, 48, 48, 128, 0, 200, False),
                                  'resblock24': (2, 24, 24, 128, 64, 192, False)}[case]
    cin = c0 + c1
    q = torch.randint(0, 256, (cout, 9 * cin), generator=g, dtype=torch.uint8)
    first = torch.arange(cout) < cout // 2
    scale = ((torch.rand(cout, generator=g) * 0.5 + 0.75) * 2.0 / 255 * (9 * cin) ** -0.5) * torch.where(first, 1.0, 1.7)
    offset = torch.where(first, torch.tensor(-128.0), torch.tensor(-77.0))
    wf = (q.float() + offset[:, None]) * scale[:, None]
    x0 = rnd((n, h, w, c0), 161)
    x1 = rnd((n, h, w, c1), 162) if c1 else None
    bias = torch.randn(cout, generator=g)
    x = torch.cat([x0, x1], -1) if c1 else x0
    ref = conv_ref(x, wf, bias, 1, ups)
    d = dev()
    kw = dict(conv=dict(stride=1, upsample=True) if ups else dict(stride=1), w_scale=scale.float().to(d), w_off=(offset + 128).float().to(d),
              tile=tile, split_k=split)
    if case.startswith('resblock'):
        rb = torch.randn(n, cout, generator=g).half()
        res = rnd((n, h, w, cout), 163)
        ref = (ref + rb.float()[:, None, None, :]).half().float() + res.float()
        kw.update(a2=x1.to(d), row_bias=rb.to(d), rows_per_img=h * w, residual=res.to(d))
    out = _halo_gemm(ops, x0.to(d), q.to(d), bias.to(d), **kw)
    check(out, ref, name=f'halo conv uint8 {case} tile{tile} split{split}')
    if split != 1:   # the opt-in in-kernel split-K reduce sees the already scaled accumulators: same bits as the reduce kernel
        assert torch.equal(tgemm(x0.to(d), q.to(d), bias.to(d), fixup=True, **kw), out)


def test_every_halo_tile_ran_some_geometry():
    """no green-by-skip: of the cases above, every halo tile must have RUN (and passed) a good number"""
    if not _HALO_RAN:
        pytest.skip('the halo tests did not run in this session')
    for t in HALO_TILES:
        assert _HALO_RAN.get(t, 0) >= 6, (t, _HALO_RAN)


def test_halo_tiles_reject_what_they_cannot_run():
    from sdod.amd import ops
    d = dev()
    x = rnd((2, 16, 16, 64), 141).to(d); wt = rnd((64, 9 * 64), 142, 0.05).to(d)
    with pytest.raises(Exception):
        tgemm(x, wt, None, conv=dict(stride=2), tile=38)               # stride 2
    with pytest.raises(Exception):
        tgemm(rnd((256, 64), 143).to(d), rnd((64, 64), 144).to(d), None, tile=38)      # rows mode


def test_conv_small_cin_via_im2col():
    from sdod.amd import ops
    n, h, w, cin, cout = 2, 64, 64, 4, 320
    x = rnd((n, h, w, cin), 40); wt = rnd((cout, 9 * cin), 41, (9 * cin) ** -0.5)
    bias = torch.randn(cout, generator=torch.Generator().manual_seed(42))
    ref = conv_ref(x, wt, bias)
    d = dev()
    wpad = torch.zeros(cout, 64, dtype=torch.float16); wpad[:, :36] = wt
    cols = ops.im2col3x3_small(x.to(d), 64)
    out = ops.gemm(cols, wpad.to(d), bias.to(d)).reshape(n, h, w, cout)
    check(out, ref, name='conv cin=4')


# -------------------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize('n,hw,c,g,dtype,silu', [
    (2, 4096, 320, 32, torch.float16, True), (2, 64, 2560, 32, torch.float16, True), (1, 16384, 128, 32, torch.float16, False),
    (2, 1024, 960, 32, torch.float16, True), (1, 100, 64, 32, torch.float32, False), (3, 7, 8, 2, torch.float32, True),
    (2, 256, 1920, 32, torch.float16, False),
    # the VAE decoder's big maps (256^2 x 256 ch, 512^2 x 128 ch): > 128 statistics chunks per image, i.e. the
    # gn_collapse_kernel path of norms.hip; (2, 65536, 256) is its batched variant
    (1, 65536, 256, 32, torch.float16, True), (1, 262144, 128, 32, torch.float16, True), (2, 65536, 256, 32, torch.float16, False),
    (2, 1024, 320, 32, torch.float16, True), (2, 1024, 640, 32, torch.float16, True), (2, 256, 1280, 32, torch.float16, True),
    (4, 4096, 320, 32, torch.float16, True), (2, 9216, 320, 32, torch.float16, True), (2, 2304, 640, 32, torch.float16, False),
    (2, 576, 1280, 32, torch.float16, True), (2, 144, 1280, 32, torch.float16, True),
])
def test_group_norm(n, hw, c, g, dtype, silu):
    from sdod.amd import ops
    gen = torch.Generator().manual_seed(50)
    x = (torch.randn(n, hw, c, generator=gen) * 2 + 3).to(dtype)   # non-zero mean exercises the shifted sums
    wt = 1 + 0.1 * torch.randn(c, generator=gen); b = 0.1 * torch.randn(c, generator=gen)
    eps = 1e-6
    ref = F.group_norm(x.float().permute(0, 2, 1), g, wt, b, eps).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    d = dev()
    out = ops.group_norm_nhwc(x.to(d), g, wt.to(d), b.to(d), eps, silu)
    check(out, ref, tol=2e-3 if dtype == torch.float16 else 2e-5, name=f'gn {n}x{hw}x{c}')


@pytest.mark.parametrize('n,hw,c0,c1,silu', [
    (2, 4096, 320, 0, True), (3, 4096, 320, 0, True), (1, 4096, 1024, 0, False), (2, 4096, 640, 320, True), (2, 1024, 1280, 640, True),
    (4, 256, 2560, 0, True), (5, 1024, 640, 0, False), (1, 16384, 512, 0, True), (5, 1000, 640, 0, True),
])
def test_group_norm_one_launch_grid_kernel(n, hw, c0, c1, silu):
    """maps >= 5 MB: the one-launch kernel with the grid barrier (norms.hip: gn_grid_kernel) -- whole-chip grids that do not
    divide the batch (n = 3, 5), pixel counts that do not divide the workgroups, channel concat, in place (y == x), and the
    barrier re-armed over many back-to-back launches; results bit-identical from launch to launch"""
    from sdod.amd import ops, _lib
    c = c0 + c1
    assert _lib.hip().sdod_group_norm_launches(hw, c, 32, 0) == 1
    g = torch.Generator().manual_seed(70)
    x0 = (torch.randn(n, hw, c0, generator=g) * 2 + torch.randn(n, 1, c0, generator=g)).half()
    x1 = (torch.randn(n, hw, c1, generator=g) * 3 - 1).half() if c1 else None
    w = 1 + 0.2 * torch.randn(c, generator=g); b = 0.3 * torch.randn(c, generator=g)
    xc = torch.cat([x0] + ([x1] if c1 else []), -1).float()
    ref = F.group_norm(xc.permute(0, 2, 1), 32, w, b, 1e-5).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    d = dev()
    a0 = x0.to(d); a1 = x1.to(d) if c1 else None
    outs = [ops.group_norm_nhwc(a0, 32, w.to(d), b.to(d), 1e-5, silu, x2=a1).clone() for _ in range(12)]
    torch.cuda.synchronize()
    check(outs[0], ref, name=f'grid gn {n}x{hw}x{c0}+{c1}')
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), 'launch-to-launch difference'
    if not c1:                                  # in place
        y = a0.clone()
        ops.group_norm_nhwc(y, 32, w.to(d), b.to(d), 1e-5, silu, out=y)
        assert torch.equal(y, outs[0])


@pytest.mark.parametrize('n,hw_side,cin,cout,c1,split,with_res', [
    (2, 8, 1280, 1280, 0, 6, True),       # 8x8 level ResBlock out conv (identity skip): V = 8, 256-thread tier
    (2, 16, 1280, 1280, 640, 6, False),   # feeds a GroupNorm over the concat (h | skip): groups of 60 straddle the boundary
    (2, 32, 640, 640, 0, 3, True),        # 32x32 level: V = 4, 1024-thread tier, 6 vectors per thread
    (4, 16, 640, 1280, 0, 5, False),      # batch 4 (config 4), time-embedding row bias
])
def test_group_norm_with_fused_splitk_reduce(n, hw_side, cin, cout, c1, split, with_res):
    """sdod_group_norm_reduce_nhwc == split-K phase 2 followed by the plain GroupNorm, bit for bit (x and y)"""
    from sdod.amd import ops
    d = dev()
    hw = hw_side * hw_side
    x = rnd((n, hw_side, hw_side, cin), 60).to(d)
    wt = rnd((cout, 9 * cin), 61, (9 * cin) ** -0.5).to(d)
    gen = torch.Generator().manual_seed(62)
    bias = torch.randn(cout, generator=gen).to(d)
    temb = rnd((n, cout), 63).to(d)
    res = rnd((n, hw_side, hw_side, cout), 64).to(d) if with_res else None
    x2 = rnd((n, hw, c1), 65, 2.0).to(d) if c1 else None
    gw = (1 + 0.1 * torch.randn(cout + c1, generator=gen)).to(d); gb = (0.1 * torch.randn(cout + c1, generator=gen)).to(d)
    kw = dict(residual=res, row_bias=temb, rows_per_img=hw, conv=dict(stride=1), split_k=split, tile=8)
    full = tgemm(x, wt, bias, **kw).clone()                                         # phases 1 + 2
    y_ref = ops.group_norm_nhwc(full.reshape(n, hw, cout), 32, gw, gb, 1e-5, True, x2=x2)
    out, _, _, desc = run_gemm(x, wt, bias, phase=1, want_desc=True, tag='kernels', **kw)
    out.fill_(float('nan'))                                                         # phase 1 must not have written it
    y = ops.group_norm_reduce(desc, n, hw, 32, gw, gb, 1e-5, True, x2=x2)
    torch.cuda.synchronize()
    assert torch.equal(out, full), 'x written by the fused kernel differs from splitk_reduce'
    # bit equality holds where the plain GroupNorm is the same (image, group) kernel: not under the forced pair path, and not for
    # maps >= 5 MB, which the plain call gives to the one-launch grid kernel (different reduction order: tolerance below)
    same_kernel = os.environ.get('SDOD_GN_PATH') != 'two' and n * hw * (cout + c1) * 2 < (5 << 20)
    if same_kernel:
        assert torch.equal(y, y_ref), 'GroupNorm output differs from reduce + GroupNorm'
    ref = F.silu(F.group_norm(torch.cat([full.reshape(n, hw, cout).float().cpu()] + ([x2.float().cpu()] if c1 else []), -1).permute(0, 2, 1),
                              32, gw.cpu(), gb.cpu(), 1e-5).permute(0, 2, 1))
    check(y, ref, name='gn fused reduce')


@pytest.mark.parametrize('n,hw,c,dtype,path', [
    (1, 16384, 512, torch.float16, 0),    # 16 MB fp16 map: the one-launch grid kernel
    (1, 16384, 512, torch.float32, 3),    # fp32: statistics + apply launches (the pilot shift comes from the workspace)
    (1, 65536, 128, torch.float32, 3),    # ... with more chunks than the apply pass reduces inline (collapse launch)
    (2, 1024, 640, torch.float16, 1),     # (image, group) one-launch kernel
    (2, 100, 64, torch.float32, 2),       # small-map LDS kernel
])
def test_group_norm_in_place_is_safe(n, hw, c, dtype, path):
    """y == x on every GroupNorm path: each path is asserted to be the one that runs"""
    from sdod.amd import ops, _lib
    assert _lib.hip().sdod_group_norm_path(n, hw, c, 0, 32, 0 if dtype == torch.float16 else 1) == path
    gen = torch.Generator().manual_seed(52)
    x = (torch.randn(n, hw, c, generator=gen) * 2 + 3).to(dtype)
    wt = 1 + 0.1 * torch.randn(c, generator=gen); b = 0.1 * torch.randn(c, generator=gen)
    ref = F.silu(F.group_norm(x.float().permute(0, 2, 1), 32, wt, b, 1e-6).permute(0, 2, 1))
    d = dev()
    xd = x.to(d)
    out = ops.group_norm_nhwc(xd, 32, wt.to(d), b.to(d), 1e-6, True, out=xd)
    assert out.data_ptr() == xd.data_ptr()
    check(out, ref, name=f'gn in place path {path}')


def _gn_big_case(seed=71, n=2, hw=4096, c=320):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, hw, c, generator=g) * 2 + torch.randn(n, 1, c, generator=g)).half()
    w = 1 + 0.2 * torch.randn(c, generator=g); b = 0.3 * torch.randn(c, generator=g)
    ref = F.silu(F.group_norm(x.float().permute(0, 2, 1), 32, w, b, 1e-5).permute(0, 2, 1))
    return x, w, b, ref


def test_group_norm_grid_barrier_timeout_is_reported_not_silent():
    """VERDICT r2 #4a / ADVICE r2: a grid barrier that cannot meet (here: a shard counter clobbered, so no arrival is ever the
    last one) gives up after ~1 s and its output is garbage -- that must surface: sticky status, the next call refuses, and
    after re-zeroing the workspace + clear_error everything works again"""
    from sdod.amd import ops, _lib
    lib = _lib.hip()
    d = dev()
    x, w, b, ref = _gn_big_case()
    xd, wd, bd = x.to(d), w.to(d), b.to(d)
    assert lib.sdod_group_norm_path(2, 4096, 320, 0, 32, 0) == 0
    good = ops.group_norm_nhwc(xd, 32, wd, bd, 1e-5, True)
    torch.cuda.synchronize()
    assert lib.sdod_group_norm_status() == 0
    check(good, ref, name='grid gn before the clobber')
    ws = ops.workspace(lib.sdod_group_norm_workspace_bytes(2, 32), d, 'gn')
    ws[32 * 3] = 1.0e9                      # shard counter 2 (one word per 128-byte line) holds garbage
    torch.cuda.synchronize()
    try:
        ops.group_norm_nhwc(xd, 32, wd, bd, 1e-5, True)       # launches; the workgroups spin, give up, flag
        torch.cuda.synchronize()
        assert lib.sdod_group_norm_status() == 4, 'timed-out grid barrier was not reported'   # LIBSDOD_RUNTIME_ERROR
        with pytest.raises(_lib.SdodError) as ei:
            ops.group_norm_nhwc(xd, 32, wd, bd, 1e-5, True)
        assert ei.value.code == 4 and 'grid barrier' in str(ei.value)
    finally:
        ws.zero_()
        torch.cuda.synchronize()
        assert lib.sdod_group_norm_clear_error() == 0
    again = ops.group_norm_nhwc(xd, 32, wd, bd, 1e-5, True)
    torch.cuda.synchronize()
    assert lib.sdod_group_norm_status() == 0
    assert torch.equal(again, good)


def test_group_norm_grid_kernel_from_two_streams_is_correct_or_reported():
    """two one-launch GroupNorms at once (own workspace each, as the header asks): both grids must be co-resident for their
    barriers to meet.  Either both results are right, or the timeout is reported -- never silent garbage."""
    from sdod.amd import ops, _lib
    import ctypes
    lib = _lib.hip()
    d = dev()
    x, w, b, ref = _gn_big_case(seed=72)
    xd, wd, bd = x.to(d), w.to(d), b.to(d)
    nbytes = lib.sdod_group_norm_workspace_bytes(2, 32)
    streams = [torch.cuda.Stream(device=d) for _ in range(2)]
    wss = [torch.zeros(nbytes // 4, dtype=torch.float32, device=d) for _ in range(2)]
    outs = [[torch.empty_like(xd) for _ in range(6)] for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(6):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                rc = lib.sdod_group_norm_nhwc(xd.data_ptr(), None, outs[s][i].data_ptr(), wd.data_ptr(), bd.data_ptr(), 2, 4096, 320, 0, 32,
                                              ctypes.c_float(1e-5), 1, 0, wss[s].data_ptr(), ctypes.c_void_p(streams[s].cuda_stream))
                assert rc in (0, 4)
    torch.cuda.synchronize()
    if lib.sdod_group_norm_status() != 0:
        lib.sdod_group_norm_clear_error()          # reported: acceptable (the grids starved each other); nothing to compare
        return
    for s in range(2):
        for o in outs[s]:
            check(o, ref, name='grid gn on two streams')
            assert torch.equal(o, outs[0][0])


def test_group_norm_concat_sources():
    from sdod.amd import ops
    gen = torch.Generator().manual_seed(51)
    n, hw, c0, c1 = 2, 256, 1280, 640   # 1920/32 = 60 channels per group: groups straddle the concat boundary
    x0 = torch.randn(n, hw, c0, generator=gen).half(); x1 = (torch.randn(n, hw, c1, generator=gen) * 3 - 1).half()
    wt = 1 + 0.1 * torch.randn(c0 + c1, generator=gen); b = 0.1 * torch.randn(c0 + c1, generator=gen)
    ref = F.silu(F.group_norm(torch.cat([x0, x1], -1).float().permute(0, 2, 1), 32, wt, b, 1e-5).permute(0, 2, 1))
    d = dev()
    out = ops.group_norm_nhwc(x0.to(d), 32, wt.to(d), b.to(d), 1e-5, True, x2=x1.to(d))
    check(out, ref, name='gn concat')


@pytest.mark.parametrize('shape,groups,dtype,silu,affine', [
    ((2, 320, 64, 64), 32, torch.float16, True, True),      # UNet 64x64 map, torch's default layout: slab of 40,960 -> statistics + apply
    ((2, 1280, 8, 8), 32, torch.float16, False, True),      # one launch, slab in registers, 16-byte vectors
    ((1, 30, 7, 5), 3, torch.float16, True, True),          # nothing divides anything: scalar path, channels not a multiple of 8
    ((2, 128, 128, 128), 32, torch.float32, True, False),   # fp32, 65,536-element slabs, no affine parameters
    ((3, 64, 16, 16), 8, torch.bfloat16, False, True),      # bf16
    ((2, 96, 1000), 4, torch.float16, True, True),          # [N, C, L] input, 24,000-element slabs
    ((1, 8, 300, 301), 2, torch.float16, False, True),      # 361,200-element slabs that are not whole vectors per chunk
    ((2, 4104, 4, 4), 8, torch.float32, False, True),       # more than 4096 channels
])
def test_group_norm_nchw_kernel(shape, groups, dtype, silu, affine):
    """sdod_group_norm_nchw: the operator on torch's default layout (a group = one contiguous slab): no transpose, any
    channel count, fp16 / bf16 / fp32, out of place and launch-to-launch reproducible; against F.group_norm in fp32 on the
    same rounded inputs (in place: tests/test_group_norm_gpu.py)"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(hash(shape) % 1000)
    x = (torch.randn(shape, generator=g) * 1.7 + torch.randn((shape[0], shape[1]) + (1,) * (len(shape) - 2), generator=g)).to(dtype)
    c = shape[1]
    w = 1 + 0.2 * torch.randn(c, generator=g) if affine else None
    b = 0.3 * torch.randn(c, generator=g) if affine else None
    ref = F.group_norm(x.float(), groups, w, b, 1e-5)
    if silu:
        ref = F.silu(ref)
    d = dev()
    xd = x.to(d)
    out = ops.group_norm_nchw(xd, groups, w.to(d) if affine else None, b.to(d) if affine else None, 1e-5, silu)
    assert out.shape == x.shape and out.dtype == dtype and out.is_contiguous()
    tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
    check(out, ref, tol=tol, name=f'gn nchw {shape} {dtype}')
    again = ops.group_norm_nchw(xd, groups, w.to(d) if affine else None, b.to(d) if affine else None, 1e-5, silu)
    assert torch.equal(again, out)


def test_efficient_gn_takes_either_layout_without_a_copy_path_difference():
    """sdod.EfficientGN(impl='eff'): an NCHW-contiguous tensor runs the NCHW kernel, the same values in channels_last run the
    NHWC kernels as a view; both agree with nn.GroupNorm, keep their memory format, and bf16 / odd channel counts are HIP too"""
    import sdod
    d = dev()
    g = torch.Generator().manual_seed(91)
    x = (torch.randn(2, 320, 32, 32, generator=g) * 2 + 0.5).half()
    m = sdod.EfficientGN(32, 320, impl='eff').to(d).half()
    with torch.no_grad():
        m.weight.copy_(1 + 0.1 * torch.randn(320, generator=g)); m.bias.copy_(0.1 * torch.randn(320, generator=g))
        ref = F.group_norm(x.float(), 32, m.weight.float().cpu(), m.bias.float().cpu(), 1e-5)
        y0 = m(x.to(d))
        y1 = m(x.to(d).contiguous(memory_format=torch.channels_last))
    assert y0.is_contiguous() and y1.is_contiguous(memory_format=torch.channels_last)
    check(y0, ref, name='EfficientGN nchw'); check(y1, ref, name='EfficientGN channels_last')
    m2 = sdod.EfficientGN(5, 35, impl='eff').to(d).to(torch.bfloat16)
    x2 = torch.randn(2, 35, 9, 9, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        y2 = m2(x2.to(d))
    check(y2, F.group_norm(x2.float(), 5, None, None, 1e-5), tol=1e-2, name='EfficientGN bf16, 35 channels')


def test_efficient_gn_module_matches_reference_golden(golden_dir):
    """sdod.EfficientGN(impl='eff') on the GPU vs outputs of the reference's own module (tests/golden/gn_efficient.npz,
    generated by oracle/gen_golden.py from /root/reference/sdod/efficient_gn.py)."""
    import sdod
    g = np.load(os.path.join(golden_dir, 'gn_efficient.npz'))
    d = dev()
    for ci in range(5):
        x = torch.from_numpy(g[f'c{ci}_x']); w = torch.from_numpy(g[f'c{ci}_w']); b = torch.from_numpy(g[f'c{ci}_b'])
        groups = int(g[f'c{ci}_groups'])
        for eps in (1e-5, 1e-6):
            m = sdod.EfficientGN(groups, x.shape[1], eps=eps, impl='eff').to(d)
            with torch.no_grad():
                m.weight.copy_(w); m.bias.copy_(b)
                y = m(x.to(d))
            ref = torch.from_numpy(g[f'c{ci}_eff_{eps:g}'])
            assert y.shape == ref.shape
            check(y, ref, tol=2e-5, name=f'EfficientGN eff c{ci} eps{eps:g}')
        m = sdod.EfficientGN(groups, x.shape[1], affine=False, impl='eff').to(d)
        with torch.no_grad():
            check(m(x.to(d)), torch.from_numpy(g[f'c{ci}_eff_noaffine']), tol=2e-5, name=f'EfficientGN noaffine c{ci}')


def test_layer_norm():
    from sdod.amd import ops
    # 8 / 16 / 32 / 64 lanes per row (norms.hip: layer_norm_kernel<LPR>), row counts that do not fill the last wave, more rows
    # than one pass of the grid covers, widths that do not fill the lane groups
    for m, c in ((8192, 320), (2048, 640), (512, 1280), (154, 768), (18432, 320), (77, 1024), (3, 64), (1, 8), (1031, 328),
                 (70000, 320), (45, 2048), (9, 3072)):
        gen = torch.Generator().manual_seed(60)
        x = (torch.randn(m, c, generator=gen) + 0.5).half()
        wt = 1 + 0.1 * torch.randn(c, generator=gen); b = 0.1 * torch.randn(c, generator=gen)
        d = dev()
        out = ops.layer_norm(x.to(d), wt.to(d), b.to(d), 1e-5)
        check(out, F.layer_norm(x.float(), (c,), wt, b, 1e-5), name=f'ln {m}x{c}')


# -------------------------------------------------------------------------------------------- attention
def attn_ref(q, k, v, heads, causal=False):
    b, lq, c = q.shape
    d = c // heads
    qh = q.float().reshape(b, lq, heads, d).transpose(1, 2)
    kh = k.float().reshape(b, -1, heads, d).transpose(1, 2)
    vh = v.float().reshape(b, -1, heads, d).transpose(1, 2)
    o = F.scaled_dot_product_attention(qh, kh, vh, is_causal=causal)
    return o.transpose(1, 2).reshape(b, lq, c)


@pytest.mark.parametrize('b,heads,lq,lk,d,causal', [
    (1, 2, 128, 128, 40, False), (2, 8, 4096, 4096, 40, False), (2, 8, 1024, 1024, 80, False),
    (2, 8, 256, 256, 160, False), (2, 8, 64, 64, 160, False), (2, 8, 4096, 77, 40, False),
    (2, 8, 1024, 77, 80, False), (2, 8, 256, 77, 160, False), (2, 12, 77, 77, 64, True), (1, 3, 200, 333, 64, False),
    (1, 2, 100, 100, 80, True),
    # d = 80 on a small grid: the key/value split inside the workgroup (two groups of four waves, merged through LDS) -- an even
    # number of key tiles, an odd one (ragged last round), a ragged last tile, and one group with a single tile
    (1, 4, 512, 1024, 80, False), (2, 3, 200, 333, 80, False), (1, 2, 64, 257, 80, False), (1, 8, 1024, 320, 80, False),
])
@pytest.mark.parametrize('use_tr', [True, False])
def test_attention(b, heads, lq, lk, d, causal, use_tr):
    from sdod.amd import ops
    if not use_tr and lq * lk > 1024 * 1024:
        pytest.skip('scalar-LDS fallback only checked on small cases')
    q = rnd((b, lq, heads * d), 70); k = rnd((b, lk, heads * d), 71); v = rnd((b, lk, heads * d), 72)
    ref = attn_ref(q, k, v, heads, causal)
    dv = dev()
    if use_tr:
        os.environ.pop('SDOD_ATTN_NO_TR', None)
    else:
        os.environ['SDOD_ATTN_NO_TR'] = '1'
    try:
        out = ops.attention(q.to(dv), k.to(dv), v.to(dv), heads, causal=causal)
        torch.cuda.synchronize()
    finally:
        os.environ.pop('SDOD_ATTN_NO_TR', None)
    check(out, ref, tol=3e-3, name=f'attn b{b} h{heads} {lq}x{lk} d{d} causal{causal} tr{use_tr}')


def test_attention_peaked_rows_force_rescale():
    """One key dominates late in the sequence: the running max jumps at a chosen tile (online-softmax rescale path)."""
    from sdod.amd import ops
    b, heads, l, d = 1, 2, 512, 40
    q = rnd((b, l, heads * d), 73); k = rnd((b, l, heads * d), 74); v = rnd((b, l, heads * d), 75)
    k[:, 300] = q[:, 17] * 6.0
    k[:, 450] = q[:, 200] * 9.0
    ref = attn_ref(q, k, v, heads)
    dv = dev()
    check(ops.attention(q.to(dv), k.to(dv), v.to(dv), heads), ref, tol=3e-3, name='attn peaked')


# ------------------------------------------------------------------------------------------ elementwise
def test_elementwise_and_layout():
    from sdod.amd import ops
    d = dev()
    x = rnd((300, 2 * 640), 80)
    check(ops.geglu(x.to(d)), x[:, :640].float() * F.gelu(x[:, 640:].float()), name='geglu')
    a = rnd((4096, 8), 81); bb = rnd((4096, 8), 82)
    check(ops.add(a.to(d), bb.to(d)), a.float() + bb.float(), name='add')
    check(ops.activation(a.to(d), 'silu'), F.silu(a.float()), name='silu')
    c0 = rnd((50, 128), 83); c1 = rnd((50, 64), 84)
    assert torch.equal(ops.concat_channels(c0.to(d), c1.to(d)).cpu(), torch.cat([c0, c1], -1))
    z = torch.randn(2, 4, 64, 64, generator=torch.Generator().manual_seed(85))
    nhwc = ops.nchw_f32_to_nhwc_f16(z.to(d), 1.0 / 0.18215)
    assert torch.equal(nhwc.cpu(), (z * np.float32(1.0 / 0.18215)).permute(0, 2, 3, 1).half())
    back = ops.nhwc_f16_to_nchw_f32(nhwc)
    assert torch.equal(back.cpu(), nhwc.cpu().float().permute(0, 3, 1, 2))
    s = rnd((64, 4096), 86, 3.0)
    check(ops.softmax_rows(s.to(d)), torch.softmax(s.float(), -1), name='softmax')
    s = rnd((16, 9216), 90, 3.0)       # SD v2.1-768 VAE attention row (96x96 latent): the 8-chunk variant
    check(ops.softmax_rows(s.to(d)), torch.softmax(s.float(), -1), name='softmax 9216')
    ids = torch.randint(0, 1000, (2, 77), generator=torch.Generator().manual_seed(87), dtype=torch.int32)
    table = rnd((1000, 768), 88); pos = rnd((77, 768), 89)
    check(ops.embedding(ids.to(d), table.to(d), pos.to(d)), table[ids.long()].float() + pos.float()[None], name='embedding')


def test_timestep_features_vs_oracle(oracle_lib):
    """context.cpp:257-274 restated in oracle/sdod_oracle.c; the GPU writes fp16, so compare after rounding."""
    from sdod.amd import ops
    ts = np.array([999.0, 949.05, 499.5, 49.949936, 1.0, 0.0], np.float32)
    ref = np.zeros((len(ts), 320), np.float32)
    for i, t in enumerate(ts):
        oracle_lib.oracle_timestep_features(float(t), 320, ref[i].ctypes.data)
    out = ops.timestep_features(torch.from_numpy(ts).to(dev()), 320).float().cpu().numpy()
    assert np.abs(out - ref).max() <= 2e-3, np.abs(out - ref).max()   # fp16 rounding of values in [-1, 1] plus device sin/cos


def test_sampler_kernels_bit_exact_vs_oracle(oracle_lib, golden_dir):
    """CFG combine + DPM-Solver++ update on the GPU reproduce the reference's host arithmetic bit for bit
    (trajectory from tests/golden/dpm_steps20.json, generated by the reference's own dpm_solver.cpp)."""
    import json
    from sdod.amd import ops
    g = json.load(open(os.path.join(golden_dir, 'dpm_steps20.json')))
    f = lambda key: np.array(g[key], np.uint32).view(np.float32)
    sig, alp, phi, i2r = f('sigmas_bits'), f('alphas_bits'), f('phis_bits'), f('i2rs_bits')
    d = dev()
    x = torch.from_numpy(f('x0_bits').copy()).to(d)
    yprev = torch.zeros_like(x)
    for s, rec in enumerate(g['trajectory']):
        eps = torch.from_numpy(np.array(rec['eps_bits'], np.uint32).view(np.float32).copy()).to(d)
        order = 1 if s == 0 else 2
        ratio = np.float32(sig[s + 1] / sig[s])
        if order == 1:
            c_prev = np.float32(0); c_cur = np.float32(-alp[s + 1] * phi[s + 1])
        else:
            c_prev = np.float32(np.float32(alp[s + 1] * phi[s + 1]) * i2r[s + 1])
            c_cur = np.float32(np.float32(-alp[s + 1] * phi[s + 1]) * np.float32(np.float32(1) + i2r[s + 1]))
        ops.dpm_update(x, eps, yprev, order, float(sig[s]), float(alp[s]), float(ratio), float(c_prev), float(c_cur))
        got = x.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np.array(rec['x_bits'], np.uint32)), f'step {s}'
    # CFG, reference form (mode 0) vs oracle_cfg_combine
    rng = np.random.default_rng(3)
    eps16 = torch.from_numpy(rng.standard_normal((2, 64, 4)).astype(np.float16))   # [2n=2][hw][c]
    out = ops.cfg_combine(eps16.to(d), 7.5, uncond_first=False, mode=0).cpu().numpy()
    ec = eps16[0].float().numpy().T.copy(); eu = eps16[1].float().numpy().T.copy()
    ref = np.zeros_like(ec)
    oracle_lib.oracle_cfg_combine(ref.ctypes.data, ec.ctypes.data, eu.ctypes.data, 7.5, ec.size)
    assert np.array_equal(out.reshape(-1).view(np.uint32), ref.reshape(-1).view(np.uint32))


def test_device_rng_philox_words_bit_exact_and_normals_vs_oracle():
    """sdod_randn_f32: the Philox4x32-10 words are bit-exact against the numpy restatement (itself pinned by the published
    known-answer vectors, tests/test_oracle_host.py); the normals match a float64 Box-Muller of the same words to fp32
    rounding; the stream is a pure function of (seed, stream id, index)."""
    from oracle import philox_oracle as PH
    from sdod.amd import ops
    d = dev()
    for seed, stream, count in ((42, 0, 16384), (42, 7, 16384), (2 ** 40 + 12345, 2 ** 33 + 5, 1001)):
        z, w = ops.randn((count,), seed, stream, d, return_words=True)
        w_ref, z_ref = PH.randn(count, seed, stream)
        assert np.array_equal(w.cpu().numpy().view(np.uint32), w_ref.reshape(-1)[:count])          # integer part: bit-exact
        zc = z.cpu().numpy().astype(np.float64)
        assert np.isfinite(zc).all() and np.abs(zc - z_ref).max() <= 2e-5 * max(1.0, np.abs(z_ref).max())
    z = ops.randn((1, 4, 64, 64), 42, 3, d)
    assert torch.equal(z, ops.randn((1, 4, 64, 64), 42, 3, d))
    assert torch.equal(z.flatten()[:4096], ops.randn((4096,), 42, 3, d))                          # prefix-stable: index-keyed
    assert not torch.equal(z, ops.randn((1, 4, 64, 64), 42, 4, d)) and not torch.equal(z, ops.randn((1, 4, 64, 64), 43, 3, d))
    big = ops.randn((1 << 20,), 1, 0, d).double()
    assert abs(float(big.mean())) < 5e-3 and abs(float(big.var()) - 1.0) < 5e-3 and abs(float((big ** 4).mean()) - 3.0) < 5e-2


def test_stage_unet_inputs_matches_the_copies_it_replaces():
    from sdod.amd import ops
    d = dev()
    g = torch.Generator().manual_seed(95)
    x = torch.randn(2, 4, 16, 16, generator=g).to(d)
    temb = torch.randn(3, 20160, generator=g).half().to(d)
    x_dst = torch.full((4, 4, 16, 16), float('nan'), device=d); t_dst = torch.full((4, 20160), float('nan'), dtype=torch.float16, device=d)
    ops.stage_unet_inputs(x, x_dst, temb[1], t_dst)
    assert torch.equal(x_dst[:2], x) and torch.equal(x_dst[2:], x) and torch.equal(t_dst, temb[1].unsqueeze(0).expand(4, -1))


def test_image_to_u8_vs_oracle(oracle_lib):
    from sdod.amd import ops
    rng = np.random.default_rng(4)
    img = (rng.standard_normal((1, 32, 32, 3)) * 0.8).astype(np.float16)
    d = dev()
    got = ops.image_to_u8(torch.from_numpy(img).to(d), a=1.0, b=0.0, mode=0).cpu().numpy()
    f32 = img.astype(np.float32).reshape(-1)
    ref = np.zeros(f32.size, np.uint8)
    oracle_lib.oracle_to_uint8(ref.ctypes.data, f32.ctypes.data, f32.size)
    assert np.array_equal(got.reshape(-1), ref)
    got = ops.image_to_u8(torch.from_numpy(img).to(d), a=0.5, b=0.5, mode=1).cpu().numpy()
    ref = (255.0 * np.clip((f32 + np.float32(1.0)) / np.float32(2.0), 0, 1)).astype(np.uint8)
    assert np.array_equal(got.reshape(-1), ref)


@pytest.mark.parametrize('case', ['64x64 C320 d40', '32x32 C640 d80', '16x16 C1280 d160', '8x8 C1280 d160', 'sd21 24x24 C1280 d64',
                                  '8x12 C1280 d160', '16x24 C640 d80'])
def test_folded_cross_attention_matches_linear_attention_linear(case):
    """The cross-attention block as two GEMMs (sdod_xattn_fold_f16 once per prompt; per evaluation a LayerNorm-folded score GEMM
    with per-image weights and the row softmax in its epilogue, then P . (V Wo^T) + bias + residual with per-image weights)
    against the three-op form it replaces -- LayerNorm -> to_q -> softmax(q k^T / sqrt d) v -> to_out + residual in fp32 torch
    (the reference's /attn2/* ops, analyze_results.py:69-79).  Tolerance as the attention / Linear kernel tests.
    The image is HxW: 8x12 (the deepest level of a 64x96 latent) is 96 rows, which only the 32-row softmax tile divides -- the
    plan replaces tile 31 by 48 there; 16x24 is 384 rows."""
    from sdod.amd import ops
    hh, ww = (int(v) for v in case.split(' C')[0].split()[-1].split('x')); c = int(case.split('C')[1].split()[0]); d = int(case.split(' d')[1])
    heads, L, B, cd = c // d, 77, 2, 768
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    rows = hh * ww
    x = (torch.randn(B * rows, c, generator=g) * 1.5 + 0.3).half().cuda()
    ctx = torch.randn(B * L, cd, generator=g).half().cuda()
    wq = (torch.randn(c, c, generator=g) / c ** 0.5).half().cuda(); wo = (torch.randn(c, c, generator=g) / c ** 0.5).half().cuda()
    wk = (torch.randn(c, cd, generator=g) / cd ** 0.5).half().cuda(); wv = (torch.randn(c, cd, generator=g) / cd ** 0.5).half().cuda()
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).cuda(); beta = (0.1 * torch.randn(c, generator=g)).cuda()
    bo = (0.1 * torch.randn(c, generator=g)).cuda()
    # reference, fp32, on the same fp16 parameters
    xf = x.float()
    ln = torch.nn.functional.layer_norm(xf, (c,), gamma, beta, 1e-5)
    q = (ln @ wq.float().t()).view(B, rows, heads, d).transpose(1, 2)
    k = (ctx.float() @ wk.float().t()).view(B, L, heads, d).transpose(1, 2)
    v = (ctx.float() @ wv.float().t()).view(B, L, heads, d).transpose(1, 2)
    att = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1) @ v
    ref = att.transpose(1, 2).reshape(B * rows, c) @ wo.float().t() + bo + xf
    # the folded form: K | V projection (one GEMM per prompt), fold, then two GEMMs
    kv = ops.gemm(ctx, torch.cat([wk, wv], 0))
    wq_f, sq, tq = ops.ln_fold(wq.clone(), gamma, beta)
    w1, s1, t1, w2 = ops.xattn_fold(kv, 0, c, B, L, wq_f, sq, tq, wo, heads)
    assert float(w1[:, :, :].view(B, heads, 80, c)[:, :, 77:].abs().max()) == 0 and float(w2.view(B, c, heads, 80)[..., 77:].abs().max()) == 0
    p = ops.gemm(x, w1, t1, ln_s=s1, rows_per_img=rows, softmax_cols=80)
    for tile in (31, 48, 56, 57, 58, 59, 60):      # every tile that carries the softmax epilogue (one that does not divide the image is re-planned)
        # make_plan: a tile whose rows do not divide the image is replaced by 31 (64 rows) or 48 (32 rows)
        runs_on = tile if rows % tile_info(tile)['bm'] == 0 else (31 if rows % 64 == 0 else 48)
        kw = dict(ln_s=s1, rows_per_img=rows, softmax_cols=80, tile=tile, runs_on=runs_on)
        assert torch.equal(tgemm(x, w1, t1, **kw), p) or rel_l2(tgemm(x, w1, t1, **kw).float().cpu(), p.float().cpu()) < 1e-3, tile
    pv = p.float().view(B * rows, heads, 80)
    assert float(pv[..., 77:].abs().max()) == 0 and float((pv.sum(-1) - 1).abs().max()) < 5e-3
    out = ops.gemm(p, w2, bo, residual=x, rows_per_img=rows)
    check(out, ref, tol=4e-3, name=f'folded cross-attention {case}')
    if rows == 96:
        assert run_gemm(x, w1, t1, ln_s=s1, rows_per_img=rows, softmax_cols=80, tile=31, runs_on=48, tag='kernels')[1] == 48


@pytest.mark.parametrize('rows', [24, 8])
def test_per_image_weights_refuse_images_no_32_row_tile_divides(rows):
    """rows_per_img = 24 (4x6) and 8 (2x4) are the deepest levels of a (16, 24) and an (8, 16) latent.  No tile of the per-image
    GEMMs divides them (the smallest has 32 rows, and a tile must not straddle two weight matrices), so sdod_gemm refuses the
    descriptor -- with and without the softmax epilogue -- and writes nothing.  The UNet builder never emits the form there:
    graphs.hip takes the folded cross-attention only where L % 32 == 0 (`xfold`) and otherwise keeps Linear -> attention kernel
    -> Linear, which sees only the flattened row count."""
    from sdod.amd import _lib, ops
    g = torch.Generator().manual_seed(700 + rows)
    B, c, nk = 2, 320, 640
    x = torch.randn(B * rows, c, generator=g).half().cuda()
    w1 = (torch.randn(B, nk, c, generator=g) / c ** 0.5).half().cuda(); w2 = (torch.randn(B, c, nk, generator=g) / nk ** 0.5).half().cuda()
    s1 = torch.ones(B, nk).cuda(); t1 = torch.zeros(B, nk).cuda()
    p = torch.full((B * rows, nk), float('nan'), dtype=torch.float16).cuda()
    with pytest.raises(_lib.SdodError, match='rows_per_img a multiple of 32'):
        ops.gemm(x, w1, t1, ln_s=s1, rows_per_img=rows, softmax_cols=80, out=p)
    out = torch.full((B * rows, c), float('nan'), dtype=torch.float16).cuda()
    with pytest.raises(_lib.SdodError, match='rows_per_img a multiple of 32'):
        ops.gemm(torch.zeros_like(p), w2, None, residual=x, rows_per_img=rows, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(p).all() and torch.isnan(out).all(), 'a refused GEMM wrote to its destination'


def test_latent_im2col_equals_latent_prep_then_im2col():
    """sdod_latent_im2col_f16 (the UNet's input convolution: NCHW fp32 latent -> K = 64 im2col matrix in one launch) against the
    two launches it replaces, bit for bit, odd sizes included"""
    from sdod.amd import ops
    for n, c, h, w, scale in ((2, 4, 64, 64, 1.0), (1, 4, 17, 9, 0.5), (3, 4, 8, 8, 1.0 / 0.18215)):
        x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(n * 100 + h)).cuda()
        ref = ops.im2col3x3_small(ops.nchw_f32_to_nhwc_f16(x, scale), 64)
        assert torch.equal(ops.latent_im2col(x, 64, scale), ref), (n, c, h, w)


@pytest.mark.parametrize('k,v_pred,stage', [(1, False, True), (2, False, True), (3, False, False), (3, True, True)])
def test_plms_update_equals_the_four_launches(k, v_pred, stage):
    """sdod_plms_update (guidance + multistep combination + DDIM update + staging of the next evaluation's inputs in one launch)
    against cfg_combine -> [v -> eps] -> lincomb4 -> ddim_step -> stage_unet_inputs, bit for bit"""
    from sdod.amd import ops
    from sdod.amd.samplers import PlmsSchedule, PLMS_ORDERS
    g = torch.Generator().manual_seed(10 * k + v_pred)
    n, c, h, w, tw = 2, 4, 16, 24, 96
    eps = torch.randn(2 * n, h, w, c, generator=g).half().cuda()
    x = torch.randn(n, c, h, w, generator=g).cuda()
    old = [torch.randn(n, c, h, w, generator=g).cuda() for _ in range(k)]
    temb_row = torch.randn(tw, generator=g).half().cuda()
    sch = PlmsSchedule(20)
    coefs, div = PLMS_ORDERS[k]
    vc = sch.v_to_eps_coef(7) if v_pred else None
    # reference: the separate launches
    xr = x.clone()
    e_t = ops.cfg_combine(eps, 7.5, uncond_first=True, mode=1)
    if vc is not None:
        e_t = ops.lincomb4([e_t, xr], [vc[0], vc[1]], 1.0)
    ops.ddim_step(xr, ops.lincomb4([e_t] + old, coefs, div), **sch.coef(7))
    xs_ref = torch.empty(2 * n, c, h, w, device='cuda'); ts_ref = torch.empty(2 * n, tw, dtype=torch.float16, device='cuda')
    ops.stage_unet_inputs(xr, xs_ref, temb_row, ts_ref)
    # fused
    xf = x.clone()
    xs = torch.zeros_like(xs_ref); ts = torch.zeros_like(ts_ref)
    e_f = ops.plms_update(eps, xf, old, coefs, div, sch.coef(7), 7.5, mode=1, v_coef=vc, stage=(xs, temb_row, ts) if stage else None)
    assert torch.equal(e_f, e_t) and torch.equal(xf, xr)
    if stage:
        assert torch.equal(xs, xs_ref) and torch.equal(ts, ts_ref)


@pytest.mark.parametrize('order,stage,uncond_first', [(1, True, True), (2, True, False), (2, False, True)])
def test_dpm_step_equals_the_three_launches(order, stage, uncond_first):
    """sdod_dpm_step (the reference driver's per-step arithmetic in one launch: context.cpp:359-373 guidance, dpm_solver.cpp:139-180
    update, :348-352 staging) against cfg_combine -> dpm_update -> stage_unet_inputs, bit for bit"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(40 + order)
    n, c, h, w, tw = 1, 4, 16, 24, 96
    eps = torch.randn(2 * n, h, w, c, generator=g).half().cuda()
    x = torch.randn(n, c, h, w, generator=g).cuda(); y = torch.randn(n, c, h, w, generator=g).cuda()
    temb_row = torch.randn(tw, generator=g).half().cuda()
    coef = dict(order=order, sigma_s=0.73, alpha_s=0.68, sigma_ratio=0.91, c_prev=-0.12, c_cur=0.31)
    xr, yr = x.clone(), y.clone()
    e = ops.cfg_combine(eps, 7.5, uncond_first=uncond_first, mode=0)
    ops.dpm_update(xr, e, yr, **coef)
    xs_ref = torch.empty(2 * n, c, h, w, device='cuda'); ts_ref = torch.empty(2 * n, tw, dtype=torch.float16, device='cuda')
    ops.stage_unet_inputs(xr, xs_ref, temb_row, ts_ref)
    xf, yf = x.clone(), y.clone()
    xs = torch.zeros_like(xs_ref); ts = torch.zeros_like(ts_ref)
    ops.dpm_step(eps, xf, yf, coef, 7.5, mode=0, uncond_first=uncond_first, stage=(xs, temb_row, ts) if stage else None)
    assert torch.equal(xf, xr) and torch.equal(yf, yr)
    if stage:
        assert torch.equal(xs, xs_ref) and torch.equal(ts, ts_ref)


@pytest.mark.parametrize('n,h,w,cout', [(2, 64, 64, 320), (1, 17, 9, 320), (3, 8, 8, 128), (2, 96, 96, 320)])
def test_conv_in_equals_im2col_then_gemm(n, h, w, cout):
    """sdod_conv_in_f16 (the UNet's input convolution in one launch: im2col rows built in LDS + the K = 64 product) against the two
    launches it replaces (sdod_latent_im2col_f16 -> sdod_gemm_f16): the same fp16 operands, the same two MFMA K steps, bias in
    fp32 -- and against the fp32 convolution"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(n * 1000 + h)
    x = torch.randn(n, 4, h, w, generator=g).cuda()
    wt = (torch.randn(cout, 4, 3, 3, generator=g) / 6).half()
    bias = torch.randn(cout, generator=g).cuda()
    wk = torch.zeros(cout, 64, dtype=torch.float16)
    wk[:, :36] = wt.permute(0, 2, 3, 1).reshape(cout, 36)              # k = tap * c + channel
    wk = wk.cuda()
    out = ops.conv_in(x, wk, bias)
    two = ops.gemm(ops.latent_im2col(x, 64, 1.0), wk, bias).view(n, h, w, cout)
    assert torch.equal(out, two)
    ref = F.conv2d(x.half().float().cpu(), wt.float(), bias.cpu(), padding=1).permute(0, 2, 3, 1)
    check(out, ref, name=f'conv_in {n}x{h}x{w} -> {cout}')
