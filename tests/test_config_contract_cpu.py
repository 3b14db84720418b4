"""The configuration contract, checked where a graph is created (include/sdod_engine.h at the fields of sdod_model_config; no device):

* head geometry of the kinds that build transformers (UNET, CONTROLNET): one of num_heads / head_dim decides, it divides the channels of
  every level (MC, 2 MC, 4 MC) and the head dim is one the attention kernel takes.  Everything else is INVALID_ARGUMENT naming the
  field -- not a kernel's message at execute(), not another model, not a dead process;
* every accepted geometry declares exactly the parameters of the oracle model of that width (names and shapes);
* TEXT_ENCODER: text_heads is checked before it divides;
* the two host-only predicates the builder and the kernels share: sdod_attention_head_dim_ok (the one list of head dims) and
  sdod_xattn_fold_ok (the folded cross-attention's whole contract), against plain restatements of what include/sdod_hip.h documents."""
import itertools

import pytest
import torch

WIDTHS = (64, 128, 192, 256, 320, 640)
HEADS = ((8, 0), (5, 0), (7, 0), (0, 40), (0, 48), (0, 64), (0, 80), (0, 160), (0, 0), (-8, 0))
HEAD_DIMS = (40, 64, 80, 160)      # include/sdod_hip.h at sdod_attention_f16


def rule(mc, num_heads, head_dim):
    """the header's rule restated: None when create must succeed, else the field its message must name"""
    if num_heads < 0:
        return 'num_heads'
    for c in (mc, 2 * mc, 4 * mc):
        if num_heads > 0:           # num_heads decides, head_dim is ignored
            if c % num_heads or c // num_heads not in HEAD_DIMS:
                return 'num_heads'
        elif head_dim <= 0 or c % head_dim or head_dim not in HEAD_DIMS:
            return 'head_dim'
    return None


def config(mc, num_heads, head_dim, hw=16, ctx=768):
    from sdod.amd import engine as E
    cfg = E.sd14_config(hw, hw)
    cfg.model_channels, cfg.num_heads, cfg.head_dim, cfg.context_dim = mc, num_heads, head_dim, ctx
    return cfg


def test_the_restated_rule_on_known_answers():
    """the restatement itself: the SD geometries pass; heads that give d = 64 / 128 / 256 or 8 / 16 / 32, heads that do not divide, a
    head_dim that does not divide (and would silently build another model), zero and negative values are refused"""
    assert rule(320, 8, 0) is None and rule(320, 0, 64) is None
    assert [mc for mc in WIDTHS if rule(mc, 8, 0) is None] == [320]
    assert {mc: rule(mc, 0, 64) for mc in WIDTHS} == dict.fromkeys(WIDTHS)
    assert rule(320, 5, 0) == rule(64, 8, 0) == rule(320, 7, 0) == rule(320, -8, 0) == 'num_heads'
    assert rule(64, 0, 48) == rule(320, 0, 0) == rule(64, 0, 40) == 'head_dim'
    assert sum(rule(mc, nh, hd) is None for mc in WIDTHS for nh, hd in HEADS) == 6 + 1 + 2 + 2 + 2     # d64 | 8 heads | d40 | d80 | d160


@pytest.mark.parametrize('kind', ['unet', 'controlnet'])
@pytest.mark.parametrize('num_heads,head_dim', HEADS)
@pytest.mark.parametrize('mc', WIDTHS)
def test_create_accepts_exactly_the_documented_head_geometries(mc, num_heads, head_dim, kind):
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    make = E.UNet if kind == 'unet' else E.ControlNet
    field = rule(mc, num_heads, head_dim)
    if field is None:
        g = make(config(mc, num_heads, head_dim), 2)
        assert len(g.param_table()) > 100
        return
    with pytest.raises(SdodError) as err:
        make(config(mc, num_heads, head_dim), 2)
    assert err.value.code == 2 and field in str(err.value), str(err.value)      # LIBSDOD_INVALID_ARGUMENT


@pytest.mark.parametrize('linear', [0, 1])
@pytest.mark.parametrize('mc,num_heads,head_dim', [(mc, nh, hd) for mc in WIDTHS for nh, hd in HEADS if rule(mc, nh, hd) is None])
def test_accepted_geometry_declares_the_oracle_model_of_that_width(mc, num_heads, head_dim, linear):
    """UNET + TEMB parameter tables against the oracle's meta-device state dict: names and shapes, both ways"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E
    cfg = config(mc, num_heads, head_dim, ctx=128 if mc < 192 else 768)
    cfg.linear_proj = linear
    table = dict(E.UNet(cfg, 2).param_table())
    table.update(dict(E.Temb(cfg, 2).param_table()))
    with torch.device('meta'):
        ref = S.UNetModel(model_ch=mc, heads=num_heads, head_dim=head_dim or None, context_dim=cfg.context_dim, use_linear=bool(linear))
    sd = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert set(table) == set(sd), sorted(set(table) ^ set(sd))[:6]
    assert {k: tuple(s) for k, s in table.items()} == sd


def test_head_dim_is_ignored_when_num_heads_decides():
    from sdod.amd import engine as E
    a = E.UNet(config(320, 8, 0), 2).param_table()
    assert E.UNet(config(320, 8, 48), 2).param_table() == a == E.UNet(config(320, 8, -3), 2).param_table()


def test_the_other_kinds_do_not_read_the_head_fields():
    """TEMB, the VAE halves and the text encoder build no UNet transformer: a head geometry the UNet refuses is none of their business"""
    from sdod.amd import engine as E
    good = E.sd14_config(16, 16)
    for cls in (E.Temb, E.VaeDecoder, E.VaeEncoder, E.TextEncoder):
        assert cls(config(320, 0, 0), 1).param_table() == cls(good, 1).param_table()


def test_text_encoder_heads_are_checked_before_they_divide():
    from oracle import sd_torch as S
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError

    def text_cfg(dim, heads, layers=2, vocab=1000):
        cfg = E.sd14_config(16, 16)
        cfg.context_dim, cfg.text_heads, cfg.text_layers, cfg.vocab_size = dim, heads, layers, vocab
        return cfg
    for heads in (0, -2, 5, 4):         # zero, negative, not dividing 128, dividing it into heads of 32
        with pytest.raises(SdodError) as err:
            E.TextEncoder(text_cfg(128, heads), 2)
        assert err.value.code == 2 and 'text_heads' in str(err.value), str(err.value)
    table = {k: tuple(s) for k, s in E.TextEncoder(text_cfg(128, 2), 2).param_table()}
    with torch.device('meta'):
        ref = S.ClipTextModel(vocab=1000, d=128, layers=2, heads=2, inter=512)
    assert table == {k: tuple(v.shape) for k, v in ref.state_dict().items()}


def test_image_encoder_heads_are_checked_before_they_divide():
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    for heads in (0, -4, 3):
        with pytest.raises(SdodError):
            E.ImageEncoder(E.VisionConfig(32, 16, 128, 1, heads, 256, 64, 0), 1)
    assert len(E.ImageEncoder(E.VisionConfig(32, 16, 128, 1, 2, 256, 64, 0), 1).param_table()) > 10


# ------------------------------------------------------------------------------------------------ the shared predicates
def test_head_dim_predicate_is_the_attention_kernels_list():
    """what tests/test_attention_paths_gpu.py::test_launcher_rejects_what_the_kernel_cannot_run expects of the launcher: d = 48
    refused, d = 64 taken; and every other d up to 512"""
    from sdod.amd import _lib
    lib = _lib.hip()
    assert lib.sdod_attention_head_dim_ok(48) == 0 and lib.sdod_attention_head_dim_ok(64) == 1
    assert [d for d in range(-8, 513) if lib.sdod_attention_head_dim_ok(d)] == list(HEAD_DIMS)


def fold_ok(heads, d, l_keys, rows):
    """include/sdod_hip.h at sdod_xattn_fold_ok, restated"""
    launch = heads >= 1 and 8 <= d <= 160 and d % 8 == 0 and 1 <= l_keys <= 80 and (heads * d) % 80 == 0
    if rows == 0:
        return launch
    return launch and heads % 4 == 0 and (heads * d) % 64 == 0 and rows > 0 and rows % 32 == 0


def test_fold_predicate_states_the_documented_contract():
    from sdod.amd import _lib
    lib = _lib.hip()
    grid = itertools.product(range(1, 33), (8, 40, 44, 64, 80, 160, 168), (1, 77, 80, 81), (16, 32, 64, 0))
    got = {k: lib.sdod_xattn_fold_ok(*k) for k in grid}
    assert got == {k: int(fold_ok(*k)) for k in got}
    assert sum(got.values()) > 100                                          # (not vacuous)
    # known answers: the SD levels fold; 4 / 8 / 12 heads of 64 (the levels that passed the builder's old gate and failed in the kernel) do not
    assert all(got[(h, d, 77, 64)] for h, d in ((8, 40), (8, 80), (8, 160), (20, 64), (16, 40), (32, 40), (4, 80), (16, 80), (4, 160)))
    assert not got[(4, 64, 77, 64)] and not got[(8, 64, 77, 64)] and not got[(12, 64, 77, 64)] and got[(5, 64, 77, 0)]
    for bad in ((0, 40, 77, 32), (-4, 40, 77, 32), (8, 0, 77, 32), (8, -40, 77, 32), (8, 40, 0, 32), (8, 40, 77, -32)):
        assert lib.sdod_xattn_fold_ok(*bad) == 0, bad
