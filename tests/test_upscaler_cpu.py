"""The ESRGAN upscaler without a GPU: the checkpoint converter (three namings, refusals), the engine's parameter table and config
mirror, every argument check of Txt2Img / Upscaler on objects made with __new__, and the fp32 restatement the GPU tests compare with."""
import ctypes
import os

import pytest
import torch

import rrdb_ref as R
from sdod.amd import convert as C
from sdod.amd import engine as E
from sdod.amd import pipeline as PL
from sdod.amd import upscale as UP
from sdod.amd import weights as Wt


@pytest.fixture(scope='module')
def sd2():
    return Wt.synthetic_state_dict(R.param_table(2), seed=3)


# ------------------------------------------------------------------------------------------------ converter
NAMINGS = {'basicsr': lambda sd: sd, 'new_arch': R.to_new_arch, 'old_arch': R.to_old_arch}


def test_three_namings_convert_to_identical_containers(sd2, tmp_path):
    blobs = []
    for name, rename in NAMINGS.items():
        for wrapper in (None, 'params_ema', 'params'):
            src = rename(sd2)
            src = src if wrapper is None else {wrapper: src}
            ck = str(tmp_path / f'{name}_{wrapper}.pth')
            torch.save(src, ck)
            out = C.convert_upscaler(ck, str(tmp_path / f'{name}_{wrapper}'))
            assert os.path.basename(out) == 'upscaler.sdodw'
            blobs.append(open(out, 'rb').read())
    assert all(b == blobs[0] for b in blobs) and len(blobs) == 9
    back = Wt.load(out)
    assert list(back) == [n for n, _ in R.param_table(2)] == Wt.names(out)
    assert all(torch.equal(back[k], sd2[k].half()) for k in back)


def test_command_line_with_only_the_upscaler(sd2, tmp_path):
    ck = str(tmp_path / 'x4.pth')
    torch.save({'params_ema': sd2}, ck)
    C.main(['--upscaler', ck, '--out', str(tmp_path / 'models')])
    assert UP.blocks_in(Wt.names(str(tmp_path / 'models' / 'upscaler.sdodw'))) == 2


@pytest.mark.parametrize('nb', [1, 6, 23])
def test_num_blocks_is_read_from_the_keys(nb):
    sd = {n: torch.zeros(s) for n, s in R.param_table(nb)}
    for rename in NAMINGS.values():
        part, found = C.upscaler_parameters(rename(sd))
        assert found == nb and list(part) == [n for n, _ in R.param_table(nb)]
        assert all(v.dtype == torch.float16 for v in part.values())


def test_refusals_name_their_reason(sd2):
    x2 = dict(sd2, **{'conv_first.weight': torch.zeros(64, 12, 3, 3)})
    with pytest.raises(ValueError, match='x2 model'):
        C.upscaler_state_dict(x2)
    x1 = {k: v for k, v in sd2.items() if not k.startswith('conv_up2.')}
    with pytest.raises(ValueError, match='no conv_up2'):
        C.upscaler_state_dict(x1)
    with pytest.raises(ValueError, match='no conv_up2'):
        C.upscaler_state_dict(R.to_new_arch(x1))
    wide = {n: torch.zeros((96 if s[0] == 64 else s[0],) + tuple(s[1:])) for n, s in R.param_table(1)}
    with pytest.raises(ValueError, match='widths 96 / 32'):
        C.upscaler_state_dict(wide)
    grow = {n: torch.zeros((16 if s[0] == 32 else s[0],) + tuple(s[1:])) for n, s in R.param_table(1)}
    with pytest.raises(ValueError, match='widths 64 / 16'):
        C.upscaler_state_dict(grow)
    compact = {f'body.{i}.weight': torch.zeros(64, 64, 3, 3) for i in range(4)}
    with pytest.raises(ValueError, match='SRVGGNetCompact'):
        C.upscaler_state_dict(compact)
    with pytest.raises(ValueError, match='neither conv_first.weight nor model.0.weight'):
        C.upscaler_state_dict({'layers.0.weight': torch.zeros(3)})
    with pytest.raises(ValueError, match='neither conv_first'):
        C.upscaler_state_dict({'params_ema': {'foo.weight': torch.zeros(3)}})


def test_shape_mismatch_and_missing_tensor_raise(sd2):
    bad = dict(sd2, **{'body.1.rdb2.conv3.weight': torch.zeros(32, 128, 1, 1)})
    with pytest.raises(ValueError, match='body.1.rdb2.conv3.weight'):
        C.upscaler_parameters(bad)
    missing = {k: v for k, v in sd2.items() if k != 'conv_hr.bias'}
    with pytest.raises(KeyError, match='conv_hr.bias'):
        C.upscaler_parameters(missing)


# ------------------------------------------------------------------------------------------------ engine and config
@pytest.mark.parametrize('nb', [1, 6, 23])
def test_param_table_equals_the_restatements(nb):
    assert E.Upscaler(nb, (8, 16), 2).param_table() == R.param_table(nb)
    assert C.upscaler_table(nb) == R.param_table(nb)


def test_config_mirror():
    assert [n for n, _ in E.UpscalerConfig._fields_] == ['num_blocks', 'in_h', 'in_w']
    assert ctypes.sizeof(E.UpscalerConfig) == 12 and E.UPSCALER == 7
    assert 'sdod_graph_create_upscaler' in E.ENGINE_SYMBOLS
    from sdod.amd import _lib
    assert {'sdod_dense_conv3x3_f16', 'sdod_dense_conv3x3_ok', 'sdod_image_conv_in_unit_f16'} <= set(_lib.HIP_SYMBOLS)
    fields = [n for n, _ in _lib.DenseConvDesc._fields_]
    assert fields[:6] == ['inp', 'w', 'bias', 'out', 'res1', 'res2'] and fields[-3:] == ['alpha', 'slope', 'c1']
    assert ctypes.sizeof(_lib.DenseConvDesc) == 6 * 8 + 11 * 4 + 3 * 4


def test_the_library_refuses_bad_configurations():
    lib = E._engine()
    h = ctypes.c_void_p()
    from sdod.amd._lib import SdodError, check
    for bad in ((0, 0, 0), (0, 8, 8), (24, 8, 8), (1, 4, 8), (1, 8, 12), (1, 1032, 8), (-1, 8, 8)):
        cfg = E.UpscalerConfig(*bad)
        with pytest.raises(SdodError):
            check(lib.sdod_graph_create_upscaler(ctypes.byref(h), ctypes.byref(cfg), 1))
        assert not h.value
    with pytest.raises(SdodError):
        check(lib.sdod_graph_create_upscaler(ctypes.byref(h), None, 1))
    cfg = E.sd14_config(8, 8)       # the kind is refused by the existing create functions
    acfg = E.AdapterConfig(0, 0, 0)
    for call in (lambda: lib.sdod_graph_create(ctypes.byref(h), 7, ctypes.byref(cfg), 1),
                 lambda: lib.sdod_graph_create_ex(ctypes.byref(h), 7, ctypes.byref(cfg), ctypes.byref(acfg), 1),
                 lambda: lib.sdod_graph_create_wrap(ctypes.byref(h), 7, ctypes.byref(cfg), ctypes.byref(acfg), 0, 1)):
        with pytest.raises(SdodError):
            check(call())
        assert not h.value


def test_python_checks_raise_value_error_before_any_device_work(sd2):
    for bad in (0, 24, True, 2.0, '3'):
        with pytest.raises(ValueError):
            E.upscaler_check_config(bad, (8, 8))
    for bad in ((8,), (4, 8), (8, 12), (1032, 8), 'ab', None, (8, 8, 8)):
        with pytest.raises(ValueError):
            E.upscaler_check_config(1, bad)
    with pytest.raises(ValueError, match='exactly one'):
        UP.upscaler_check_build(None, None, (8, 8), None)
    with pytest.raises(ValueError, match='exactly one'):
        UP.upscaler_check_build(sd2, 'x.sdodw', (8, 8), None)
    with pytest.raises(ValueError, match='num_blocks=3'):
        UP.upscaler_check_build(sd2, None, (8, 8), 3)
    with pytest.raises(ValueError, match='body.N'):
        UP.upscaler_check_build({'conv_first.weight': torch.zeros(1)}, None, (8, 8), None)
    assert UP.upscaler_check_build(sd2, None, (8, 16), None) == (2, (8, 16))
    up = UP.Upscaler.__new__(UP.Upscaler)
    up.image_hw = (8, 16)
    for bad in (torch.zeros(1, 8, 16, 3), torch.zeros(8, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 8, 3, dtype=torch.uint8),
                torch.zeros(1, 8, 16, 1, dtype=torch.uint8), torch.zeros(0, 8, 16, 3, dtype=torch.uint8), None):
        with pytest.raises(ValueError):
            up.upscale(bad)
        with pytest.raises(ValueError):
            up.upscale_float(bad)


def test_pipeline_checks_on_an_object_made_with_new(sd2, tmp_path):
    kw = dict(upscaler=True, tiling=False, latent_hw=8, state_dicts={'upscaler': sd2}, models_dir=None)
    assert PL.upscaler_check_build(**kw) == dict(state_dict=sd2, image_hw=(64, 64))
    assert PL.upscaler_check_build(**dict(kw, latent_hw=(8, 16))) ['image_hw'] == (64, 128)
    assert PL.upscaler_check_build(**dict(kw, upscaler=False)) is None
    for tiling in (True, 'x', 'y', 'xy'):
        with pytest.raises(ValueError, match='tiling'):
            PL.upscaler_check_build(**dict(kw, tiling=tiling))
    with pytest.raises(ValueError, match='1024'):
        PL.upscaler_check_build(**dict(kw, latent_hw=136))
    with pytest.raises(ValueError, match="state_dicts\\['upscaler'\\]"):
        PL.upscaler_check_build(**dict(kw, state_dicts={}))
    with pytest.raises(ValueError, match='upscaler.sdodw'):
        PL.upscaler_check_build(**dict(kw, state_dicts=None, models_dir=str(tmp_path)))
    with pytest.raises(ValueError):
        PL.upscaler_check_build(**dict(kw, state_dicts=None))
    Wt.save(str(tmp_path / 'upscaler.sdodw'), {k: v.half() for k, v in sd2.items()})
    assert PL.upscaler_check_build(**dict(kw, state_dicts=None, models_dir=str(tmp_path))) == \
        dict(path=str(tmp_path / 'upscaler.sdodw'), image_hw=(64, 64))
    pipe = PL.Txt2Img.__new__(PL.Txt2Img)
    x_T, ctx2 = torch.zeros(1, 4, 8, 8), torch.zeros(2, 77, 768)
    for call in (lambda: pipe.upscale(torch.zeros(1, 64, 64, 3, dtype=torch.uint8)), lambda: pipe.generate_upscaled(ctx2, x_T),
                 lambda: pipe.generate_upscaled_graphed(ctx2, x_T)):
        with pytest.raises(ValueError, match='upscaler=True'):
            call()
    up = UP.Upscaler.__new__(UP.Upscaler)
    up.image_hw = (64, 64)
    pipe.upscaler = up
    with pytest.raises(ValueError, match='64, 64, 3'):
        pipe.upscale(torch.zeros(1, 32, 64, 3, dtype=torch.uint8))
    pipe.cfg = E.sd14_config(8, 8)
    with pytest.raises(ValueError):
        pipe.generate_upscaled(ctx2, x_T, steps=0)
    with pytest.raises(ValueError):
        pipe.generate_upscaled_graphed(ctx2, x_T, sampler='nope')
    pipe.hires = object()
    with pytest.raises(ValueError, match='hires_hw'):
        pipe.generate_upscaled_graphed(ctx2, x_T)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope='module')
def small():
    img = R.sample_image(2, 8, 16)
    sd = R.synthetic(2)
    return img, sd, R.upscale(sd, img)


def test_restatement_output(small):
    img, sd, (y, u8) = small
    assert tuple(y.shape) == (2, 32, 64, 3) == tuple(u8.shape) and y.dtype == torch.float32 and u8.dtype == torch.uint8
    assert torch.isfinite(y).all() and float(y.std()) > 0.05 and float((y[0] - y[1]).abs().max()) > 0.05
    assert torch.equal(u8, torch.round(255 * y.clamp(0, 1)).to(torch.uint8))
    y_flip, _ = R.upscale(sd, img.flip(2))
    assert float((y_flip - y).abs().max()) > 0.05 and float((y_flip.flip(2) - y).abs().max()) > 1e-3   # the weights are not symmetric


def test_border_differs_from_the_signed_reparametrisation(small):
    """conv_first pads with zeros in the [0, 1] space: folding 2 u / 255 - 1 into its weights agrees in the interior only"""
    img, sd, (y, _) = small
    y2 = R.upscale_signed_reparam(sd, img)
    assert float((y2 - y).abs().max()) > 1e-2          # (the network spreads the border over the whole of so small an image)
    # conv_first alone: the two agree off the border and differ on it by the missing taps' worth
    w, b = sd['conv_first.weight'], sd['conv_first.bias']
    x = img.permute(0, 3, 1, 2).float() / 255
    unit = torch.nn.functional.conv2d(x, w, b, padding=1)
    signed = torch.nn.functional.conv2d(2 * x - 1, w / 2, b + w.sum(dim=(1, 2, 3)) / 2, padding=1)
    assert float((unit - signed)[:, :, 1:-1, 1:-1].abs().max()) < 1e-5 and float((unit - signed)[:, :, 0].abs().max()) > 0.1


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: f'nb{c[0]}')
def test_spread_of_the_uint8_comparison_weights(case):
    """the weights the GPU test compares bytes with: at least 10 % of the reference's bytes at 0 or 255, at least 50 % strictly inside"""
    nb, b, h, w = case
    img = R.sample_image(b, h, w)
    _, u8 = R.upscale(R.spread_weights(nb, img), img)
    sat = float(((u8 == 0) | (u8 == 255)).float().mean())
    print(f'nb {nb}: {sat:.3f} of the bytes saturated')
    assert sat >= 0.10 and 1.0 - sat >= 0.50
