"""Seamless tiling without a GPU: the host answers of the library under the circular border modes (sdod_gemm_desc::pad_mode 2 / 3 / 4),
the refusals that come before any launch, the structs and symbols, Txt2Img's argument rule, and the fp64 reference the GPU tests
(test_conv_wrap_gpu.py, test_tiling_gpu.py) compare against.

ref_conv_wrap   conv_cases.ref_conv with the border rule of a pad_mode: F.pad(..., mode='circular') on the wrapped axes, zeros on the
                other, then padding=0 -- the output size of pad_mode 0, so conv_cases.exact_conv(pad_mode=0) supplies the operands."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import gemm_cases as gc

WRAP_MODES = (2, 3, 4)
WRAP_OF = {0: (False, False), 2: (True, True), 3: (True, False), 4: (False, True)}     # pad_mode -> (x wraps, y wraps)


def pad_wrap(x, mode):
    """NCHW: one pixel of border on every side, circular on the axes `mode` wraps and zero on the others"""
    wx, wy = WRAP_OF[mode]
    x = F.pad(x, (1, 1, 0, 0), mode='circular') if wx else F.pad(x, (1, 1, 0, 0))
    return F.pad(x, (0, 0, 1, 1), mode='circular') if wy else F.pad(x, (0, 0, 1, 1))


def ref_conv_wrap(x0, w, bias=None, *, mode, x1=None, stride=1, ups=False, row_bias=None, residual=None, tail=None, bias2=None):
    """conv_cases.ref_conv (same operands, same [n * ho * wo][cout] fp64 result, same exactness check) with the border of pad_mode
    `mode` in {0, 2, 3, 4}; the wrap acts on the upsampled image, i.e. in output coordinates"""
    x = (x0 if x1 is None else torch.cat([x0, x1], -1)).double().permute(0, 3, 1, 2)
    cout, cin = w.shape[0], x.shape[1]
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode='nearest')
    w3 = w[:, :9 * cin].double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    y = F.conv2d(pad_wrap(x, mode), w3, None if bias is None else bias.double(), stride=stride, padding=0).permute(0, 2, 3, 1)
    if row_bias is not None:
        y = y + row_bias.double()[:, None, None, :]
    if residual is not None:
        y = y + residual.double()
    if tail is not None:
        t = torch.cat([s for s in tail if s is not None], -1).double()
        assert t.shape[:3] == y.shape[:3] and w.shape[1] == 9 * cin + t.shape[-1]
        y = y + t @ w[:, 9 * cin:].double().t()
        if bias2 is not None:
            y = y + bias2.double()
    y = y.reshape(-1, cout).contiguous()
    gc.assert_exact(y)
    return y


# geometries the GPU tests run: (n, h, w, stride, ups)
GEOMS = ([(n, h, w, 1, False) for n, h, w in cc.RECTS] + [(n, h, w, 1, True) for n, h, w in cc.RECTS_UPS] +
         [(2, 1, 2, 1, False), (1, 2, 1, 1, False)] + [(n, h, w, 2, False) for n, h, w in [(2, 8, 12), (1, 9, 5), (3, 5, 9)]])


# ------------------------------------------------------------------------------------------------------ the reference helper
@pytest.mark.parametrize('mode', WRAP_MODES)
def test_reference_is_exact_and_differs_from_the_zero_border(mode):
    for n, h, w, stride, ups in GEOMS:
        d = cc.exact_conv(n, h, w, 64, 0, 24, 77 + h + 3 * w, stride=stride, pad_mode=0, ups=ups)
        ref = ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=mode, stride=stride, ups=ups)          # (assert_exact inside)
        zero = cc.ref_conv(d['x0'], d['w'], d['bias'], stride=stride, ups=ups)
        assert ref.shape == zero.shape
        assert torch.equal(ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=0, stride=stride, ups=ups), zero)
        assert not torch.equal(ref, zero), (mode, n, h, w, stride, ups)


@pytest.mark.parametrize('mode', WRAP_MODES)
def test_reference_commutes_with_a_roll_along_wrapped_axes_only(mode):
    n, h, w = 2, 8, 12
    d = cc.exact_conv(n, h, w, 64, 0, 24, 311, pad_mode=0)
    wx, wy = WRAP_OF[mode]

    def conv(x):
        return ref_conv_wrap(x, d['w'], d['bias'], mode=mode).reshape(n, h, w, -1)

    y = conv(d['x0'])
    for sy, sx in ((3, 0), (0, 5), (3, 5)):
        same = torch.equal(conv(torch.roll(d['x0'], (sy, sx), (1, 2))), torch.roll(y, (sy, sx), (1, 2)))
        assert same == ((wy or sy == 0) and (wx or sx == 0)), (mode, sy, sx, same)


def test_reference_with_every_epilogue_piece_is_exact():
    d = cc.exact_conv(2, 8, 12, 64, 64, 24, 5, pad_mode=0)
    ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=2, x1=d['x1'], row_bias=d['row_bias'], residual=d['residual'])
    d = cc.exact_conv(2, 8, 12, 64, 0, 24, 6, tail=(64, 64))
    ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=3, tail=(d['t0'], d['t1']), bias2=d['bias2'])
    d = cc.exact_conv_u8(2, 8, 12, 64, 64, 40, 7)
    ref = ref_conv_wrap(d['x0'], d['wf'], d['bias'], mode=2, x1=d['x1'], row_bias=d['row_bias'])
    assert not torch.equal(ref, cc.ref_conv(d['x0'], d['wf'], d['bias'], x1=d['x1'], row_bias=d['row_bias']))


# --------------------------------------------------------------------------------------------- host answers equal pad_mode 0
def _desc(n, h, w, mode, tile=0, ups=False, stride=1, split=0):
    d = cc.conv_desc(n, h, w, 64, 64, ups=ups, stride=stride, tile=tile, split=split)
    if stride == 2:
        ho, wo = cc.out_size(h, w, 2)
        d.M = n * ho * wo
    d.pad_mode = mode
    return d


def _answers(d, tile):
    from sdod.amd import _lib
    lib = _lib.hip()
    return (lib.sdod_gemm_halo_ok(ctypes.byref(d), tile), gc.plan_of(d), int(lib.sdod_gemm_workspace_bytes(ctypes.byref(d))),
            lib.sdod_gemm_xcd_panels(ctypes.byref(d)))


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_tiles_answer_the_wrap_modes_as_mode_0(tile):
    taken = 0
    for ups, geoms in ((False, cc.RECTS), (True, cc.RECTS_UPS), (False, cc.RECTS_ENGINE)):
        for n, h, w in geoms:
            for split in (0, 3):
                base = _answers(_desc(n, h, w, 0, tile, ups, split=split), tile)
                taken += base[0]
                for mode in WRAP_MODES:
                    assert _answers(_desc(n, h, w, mode, tile, ups, split=split), tile) == base, (tile, n, h, w, ups, mode)
    assert taken > 0


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_tiles_still_decline_pad_mode_1(tile):
    from sdod.amd import _lib
    for n, h, w in cc.RECTS + cc.RECTS_ENGINE:
        d = _desc(n, h, w, 1, tile)
        assert _lib.hip().sdod_gemm_halo_ok(ctypes.byref(d), tile) == 0


@pytest.mark.parametrize('tile', [0, 3, 14, 27, 46])
def test_implicit_plans_answer_the_wrap_modes_as_mode_0(tile):
    for stride in (1, 2):
        for n, h, w in cc.RECTS + cc.RECTS_ENGINE:
            for split in (0, 3):
                base = _answers(_desc(n, h, w, 0, tile, stride=stride, split=split), 37)[1:]
                for mode in WRAP_MODES:
                    assert _answers(_desc(n, h, w, mode, tile, stride=stride, split=split), 37)[1:] == base, (tile, n, h, w, stride, mode)


# ------------------------------------------------------------------------------------------------ refusals before any launch
def _refused(d, words):
    """the argument check answers before the launch: the operand pointers are fakes that must never be dereferenced"""
    from sdod.amd import _lib
    with pytest.raises(_lib.SdodError) as ex:
        _lib.check(_lib.hip().sdod_gemm_f16(ctypes.byref(d), None))
    assert words in str(ex.value), str(ex.value)


def test_wrap_modes_are_refused_where_they_mean_nothing():
    d = cc.conv_desc(2, 8, 16, 64, 64)
    d.ksize = 1; d.K = 64; d.ldw = 64; d.pad_mode = 2
    _refused(d, 'needs a 3x3 conv')
    d = _desc(2, 8, 16, 5)
    _refused(d, 'pad_mode must be 0 .. 4')
    d = _desc(2, 8, 16, -1)
    _refused(d, 'pad_mode must be 0 .. 4')
    d = gc.rows_desc(64, 64, 64, pad_mode=2)
    _refused(d, 'convolutions only')
    d = _desc(2, 8, 16, 1)                       # pad_mode 1 keeps its refusals: stride 1 is one
    _refused(d, 'pad_mode 1 needs')


def test_graph_wrap_is_refused_outside_unet_and_vae_decoder():
    from sdod.amd import _lib, engine as E
    cfg = E.sd14_config(16, 24)
    for kind in (E.TEXT_ENCODER, E.TEMB, E.VAE_ENCODER, E.VAE_ENCODER_MASKED):
        for wrap in (1, 2, 3):
            with pytest.raises(_lib.SdodError):
                E.Graph(kind, cfg, 1, wrap=wrap)
        E.Graph(kind, cfg, 1, wrap=0)
    with pytest.raises(_lib.SdodError):
        E.Graph(E.UNET, E.sd14_config(16, 24, concat_channels=5), 2, wrap=3)
    for wrap in (-1, 4):
        with pytest.raises(_lib.SdodError):
            E.Graph(E.UNET, cfg, 2, wrap=wrap)
    plain = E.UNet(cfg, 2).param_table()
    for wrap in (0, 1, 2, 3):                    # the parameters of a wrapped graph are the plain graph's
        assert E.UNet(cfg, 2, wrap=wrap).param_table() == plain
    tcfg = E.copy_config(cfg)
    tcfg.tiling = 3
    assert E.UNet(tcfg, 2).param_table() == plain and E.VaeDecoder(tcfg, 1).param_table() == E.VaeDecoder(cfg, 1).param_table()
    E.TextEncoder(tcfg, 2)                       # cfg.tiling is read by UNet and VaeDecoder only


# ------------------------------------------------------------------------------------------------------- structs and symbols
def test_structs_keep_their_size_and_the_symbols_are_bound():
    from sdod.amd import _lib, engine as E
    assert _lib.GemmDesc._fields_[-1][0] == 'pad_mode'
    assert ctypes.sizeof(E.ModelConfig) == 64 and ctypes.sizeof(E.AdapterConfig) == 12
    lib = _lib.hip()
    for s in ('sdod_conv_in_wrap_f16', 'sdod_im2col3x3_small_wrap_f16'):
        assert s in _lib.HIP_SYMBOLS and getattr(lib, s).argtypes is not None
    assert 'sdod_graph_create_wrap' in E.ENGINE_SYMBOLS and hasattr(lib, 'sdod_graph_create_wrap')
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include')
    hip_h, eng_h = open(os.path.join(root, 'sdod_hip.h')).read(), open(os.path.join(root, 'sdod_engine.h')).read()
    assert 'sdod_conv_in_wrap_f16(' in hip_h and 'sdod_im2col3x3_small_wrap_f16(' in hip_h and 'sdod_graph_create_wrap(' in eng_h


def test_config_copies_carry_tiling():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 24)
    assert cfg.tiling == 0 and E.copy_config(cfg).tiling == 0
    cfg.tiling = 1
    cp = E.copy_config(cfg)
    assert cp.tiling == 1 and (cp.latent_h, cp.latent_w) == (16, 24)
    cp.tiling = 3
    assert cfg.tiling == 1 and E.sd14_config(16, 24).tiling == 0


# ----------------------------------------------------------------------------------------------------------- the argument rule
def test_tiling_check_build_truth_table():
    from sdod.amd.pipeline import tiling_check_build
    for tiling, wrap in ((False, 0), (True, 3), ('xy', 3), ('x', 1), ('y', 2)):
        assert tiling_check_build(tiling, False, False, None, False) == wrap
    # off: nothing is refused (the combinations are those of every build before)
    assert tiling_check_build(False, True, True, (16, 16), True) == 0
    for tiling in (True, 'xy', 'x', 'y'):
        for name, args in (('with_vae_encoder', (True, False, None, False)), ('inpaint_unet', (False, True, None, False)),
                           ('hires_hw', (False, False, (16, 24), False)), ('adapter', (False, False, None, True))):
            with pytest.raises(ValueError, match=name):
                tiling_check_build(tiling, *args)
    for bad in ('yx', 'XY', '', 1, 0, 3, 2.0, None, ('x',), ['x', 'y'], b'x'):
        with pytest.raises(ValueError, match='tiling must be'):
            tiling_check_build(bad, False, False, None, False)


def test_txt2img_refuses_before_any_device_work():
    """no GPU here: a constructor that reached device work would fail with something other than ValueError"""
    from sdod.amd.pipeline import Txt2Img
    for kw in (dict(tiling='z'), dict(tiling=True, with_vae_encoder=True), dict(tiling='x', inpaint_unet=True),
               dict(tiling='y', hires_hw=(16, 16)), dict(tiling='xy', adapter=True)):
        with pytest.raises(ValueError):
            Txt2Img(state_dicts={}, latent_hw=(16, 24), with_text_encoder=False, **kw)
