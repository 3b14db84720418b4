"""FreeU without a GPU: the closed form of the Fourier filter against the published torch.fft formulation, the version-2 factor
against the published lines, the site rule on the oracle UNet's pop order, the argument checks (which run before any device work),
the switch's own refusals and the exported symbols.  The GPU side is tests/test_freeu_gpu.py."""
import ctypes

import pytest
import torch

import freeu_ref as FR


@pytest.mark.parametrize('hw', FR.SIZES)
def test_closed_form_is_the_published_fft_filter(hw):
    """fp64, <= 1e-12: the shifted box [H//2-1 : H//2+1, W//2-1 : W//2+1] is the frequency set {0, -1 mod H} x {0, -1 mod W} -- a side
    of 1 has one member, a side of 2 both, and +1 is never in it"""
    g = torch.Generator().manual_seed(100 * hw[0] + hw[1])
    x = torch.randn(2, 3, *hw, generator=g, dtype=torch.float64) + torch.randn(2, 3, 1, 1, generator=g, dtype=torch.float64)
    for s in (0.0, 0.2, 0.9, 2.0):
        want = FR.fourier_filter_fft(x, 1, s)
        got = FR.fourier_filter(x, s)
        err = float((got - want).abs().max())
        assert err <= 1e-12, (hw, s, err)
    assert torch.equal(FR.fourier_filter(x, 1.0), x)
    assert FR.frequency_set(1) == [0] and FR.frequency_set(2) == [0, 1] and FR.frequency_set(5) == [0, 4]


def test_version_2_factor_is_the_published_lines_where_they_are_defined():
    g = torch.Generator().manual_seed(5)
    h = torch.randn(2, 8, 4, 6, generator=g, dtype=torch.float64)
    for b in (0.0, 1.0, 1.3, 2.0):
        pub = FR.backbone_factor_published(h, b)
        assert torch.isfinite(pub).all()
        assert float((FR.backbone_factor(h, b, 2) - pub).abs().max()) <= 1e-12
        assert torch.equal(FR.backbone_factor(h, b, 1), torch.full((2, 1, 4, 6), b, dtype=torch.float64))
    # the departure: max == min (a 1 x 1 map, a constant mean) is 0 / 0 = NaN as published and factor 1 here
    one = torch.randn(2, 8, 1, 1, generator=g, dtype=torch.float64)
    const = torch.randn(1, 8, 1, 1, generator=g, dtype=torch.float64).expand(2, 8, 3, 3)
    for t in (one, const):
        assert torch.isnan(FR.backbone_factor_published(t, 1.4)).all()
        assert torch.equal(FR.backbone_factor(t, 1.4, 2), torch.ones(2, 1, *t.shape[-2:], dtype=torch.float64))
    # and the scaled tensor: first half of the channels only
    hh, _ = FR.apply_site(h, h, 1.5, 1.0, 1)
    assert torch.equal(hh[:, 4:], h[:, 4:]) and torch.equal(hh[:, :4], h[:, :4] * 1.5)


def test_site_rule_on_the_oracle_unet():
    """both 4 MC is stage 1, both 2 MC stage 2, on the (backbone, skip) widths the oracle's own decoder pops"""
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel()
    pairs = FR.decoder_pairs(unet)
    assert len(pairs) == 12
    stages = [FR.site_stage(a, b, 320) for a, b in pairs]
    assert [i for i, st in enumerate(stages) if st] == [0, 1, 2, 3, 4, 7]
    assert [st for st in stages if st] == [1, 1, 1, 1, 1, 2]
    with torch.device('meta'):
        small = S.UNetModel(model_ch=64, heads=1)
    assert [i for i, (a, b) in enumerate(FR.decoder_pairs(small)) if FR.site_stage(a, b, 64)] == [0, 1, 2, 3, 4, 7]


def test_restatement_at_the_identity_is_the_plain_unet_and_moves_otherwise():
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(8, 8)
    sd = {**Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234), **Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235)}
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict(sd, assign=True)
    unet.eval()
    g = torch.Generator().manual_seed(7)
    x, ctx, t = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 77, 768, generator=g), torch.tensor([999.0, 501.0])
    with torch.no_grad():
        plain = unet(x, t, ctx)
        same = FR.freeu_unet(unet, x, t, ctx, 1.0, 1.0, 1.0, 1.0, 1)
        moved = FR.freeu_unet(unet, x, t, ctx, 2.0, 2.0, 0.0, 0.0, 1)
    assert float((same - plain).abs().max()) <= 1e-5 * float(plain.abs().max())
    assert float((moved - plain).norm() / plain.norm()) > 5e-2


# ------------------------------------------------------------------ argument checks
def test_freeu_check_args_and_presets():
    from sdod.amd import freeu as FU
    assert FU.freeu_check_args(1.3, 1.4, 0.9, 0.2) == (1.3, 0.9, 1.4, 0.2, 2.0, 0.0, 0.0, 0.0)        # the block is (b1, s1, b2, s2, version)
    assert FU.freeu_check_args(1, 1, 1, 1, 1) == (1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
    assert FU.freeu_check_args(0, 10, 0.0, 10.0, 2)[:4] == (0.0, 0.0, 10.0, 10.0)
    assert FU.preset(2, 'sd14') == (1.3, 1.4, 0.9, 0.2) and FU.preset(2, 'sd21') == (1.4, 1.6, 0.9, 0.2)
    assert FU.preset(1, 'sd14') == (1.2, 1.4, 0.9, 0.2) and FU.preset(1, 'sd21') == (1.1, 1.2, 0.9, 0.2)
    assert FU.IDENTITY[:5] == (1.0, 1.0, 1.0, 1.0, 2.0)
    with pytest.raises(ValueError, match='preset'):
        FU.preset(3)
    for bad in (float('nan'), float('inf'), -0.1, 10.5, 'big', None, True, [1.0]):
        for pos in range(4):
            args = [1.0, 1.0, 1.0, 1.0]
            args[pos] = bad
            with pytest.raises(ValueError, match='freeu'):
                FU.freeu_check_args(*args)
    for bad in (0, 3, 2.5, '2', None, True):
        with pytest.raises(ValueError, match='version'):
            FU.freeu_check_args(1.0, 1.0, 1.0, 1.0, bad)


@pytest.mark.parametrize('bad', [1, 0, 'yes', 2.0, (1.3, 1.4, 0.9, 0.2)])
def test_freeu_check_build_refuses_before_any_device_work(bad):
    from sdod.amd import freeu as FU, pipeline as PL
    assert FU.freeu_check_build(False) is False and FU.freeu_check_build(None) is False and FU.freeu_check_build(True) is True
    with pytest.raises(ValueError, match='freeu must be'):
        FU.freeu_check_build(bad)
    with pytest.raises(ValueError, match='freeu must be'):                  # the constructor: before it touches the device
        PL.Txt2Img(state_dicts={}, latent_hw=16, freeu=bad)


def test_setters_need_the_flag_and_validate_first():
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    assert pipe.freeu is False
    for call in (lambda: pipe.set_freeu(1.3, 1.4, 0.9, 0.2), pipe.clear_freeu):
        with pytest.raises(RuntimeError, match='freeu=True'):
            call()
    pipe.freeu = True                                                       # (no unet on this object: a check that passed would fail on it)
    for args in ((float('nan'), 1, 1, 1), (1, 1, 1, 11), (1, 1, -1, 1), (1, 1, 1, 1, 3)):
        with pytest.raises(ValueError, match='freeu'):
            pipe.set_freeu(*args)


# ------------------------------------------------------------------ library, host side
def test_new_symbols_are_exported_and_bound():
    from sdod.amd import _lib, engine as E, ops
    lib = _lib.hip()
    assert 'sdod_freeu_f16' in _lib.HIP_SYMBOLS and len(lib.sdod_freeu_f16.argtypes) == 11
    E._engine()
    for s in ('sdod_graph_enable_freeu', 'sdod_graph_freeu_input'):
        assert s in E.ENGINE_SYMBOLS and getattr(lib, s).argtypes is not None
    assert hasattr(ops, 'freeu')
    assert ctypes.sizeof(E.ModelConfig) == 16 * 4                           # the public layout did not move: the switch is no field


def test_switch_is_for_unet_graphs_and_changes_no_parameter():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    assert cfg.freeu == 0 and E.copy_config(cfg).freeu == 0
    c2 = E.copy_config(cfg); c2.freeu = 1
    assert E.copy_config(c2).freeu == 1 and cfg.freeu == 0
    assert E.UNet(c2, 2).param_table() == E.UNet(cfg, 2).param_table()      # no weights; the table is readable without a device
    assert E.UNet(cfg, 2).freeu_input() == -1                               # (with the switch the slot exists once finalized)
    for g in (E.Temb(c2, 1), E.VaeDecoder(c2, 1)):                          # the attribute is read by UNet graphs only ...
        with pytest.raises(Exception, match='UNET graph only'):             # ... and the switch refuses every other kind
            g.enable_freeu()
    for extra in (dict(control_inputs=1), dict(adapter_reps=2), dict(tiling=3), dict(concat_channels=5)):
        c = E.copy_config(c2)
        for k, v in extra.items():
            setattr(c, k, v)
        assert len(E.UNet(c, 2).param_table()) > 0                          # composes with the other creation paths
