"""Inpainting checkpoints (9-channel UNet, ldm `conditioning_key: hybrid`), everything that needs no GPU: the parameter table and
the config mirror, the fp32 torch restatement of the definition that tests/test_inpaint_concat_gpu.py compares the GPU chain with
(checked against itself where it can be), the argument contract of Txt2Img.inpaint_concat (ValueError before any device work) and
the checkpoint converter.

The definition (runwayml scripts/inpaint_st.py, diffusers StableDiffusionInpaintPipeline), with init_u8 uint8 [n, 8H, 8W, 3] and mask_u8
uint8 [n, 8H, 8W] (255 = repaint):  m = mask_u8 >= 128;  masked image (2 u / 255 - 1) * (1 - m);  c_lat = 0.18215 * (mean +
exp(0.5 * clamp(logvar, -30, 20)) * n1) from the VAE encoder's moments of the masked image;  c_mask = F.interpolate(m, size=(H, W))
(nearest: m[8 i, 8 j]);  UNet input cat(x, c_mask, c_lat), the same five channels in both guidance halves;  the ordinary sampler from
pure noise."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------ the restatement (imported by test_inpaint_concat_gpu.py)
def binarise(mask_u8):
    """m: bool [n, 8H, 8W], True = repaint"""
    return mask_u8 >= 128


def masked_image(init_u8, mask_u8):
    """fp32 NCHW [n, 3, 8H, 8W]: (2 u / 255 - 1) * (1 - m), the encoder's input"""
    m = binarise(mask_u8)
    x = 2.0 * (init_u8.float() / 255.0) - 1.0
    return (x * (1.0 - m.float())[..., None]).permute(0, 3, 1, 2).contiguous()


def latent_mask(mask_u8):
    """c_mask fp32 [n, H, W]: the binarised mask through F.interpolate(size=(H, W)) (nearest)"""
    m = binarise(mask_u8).float()
    return F.interpolate(m[:, None], size=(mask_u8.shape[1] // 8, mask_u8.shape[2] // 8))[:, 0]


@torch.no_grad()
def concat_conditioning(enc, init_u8, mask_u8, n1):
    """(cond fp32 [n, 5, H, W] = c_mask | c_lat, moments fp32 [n, 8, H, W]) with enc an fp32 ldm encoder + quant_conv"""
    moments = enc(masked_image(init_u8, mask_u8))
    mean, logvar = torch.chunk(moments, 2, dim=1)
    c_lat = 0.18215 * (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * n1)
    return torch.cat([latent_mask(mask_u8)[:, None], c_lat], 1), moments


def concat_unet(unet9, cond):
    """the eps model the sampler oracles call: x [b, 4, H, W] -> unet9(cat(x, c_mask, c_lat)), cond repeated over the guidance batch"""
    def model(x, t, ctx):
        reps = x.shape[0] // cond.shape[0]
        return unet9(torch.cat([x, cond.repeat(reps, 1, 1, 1)], 1), t, ctx)
    return model


def mask128():
    """the `_mask128` recipe of tests/test_inpaint_gpu.py: keep for columns < 48, repaint for columns >= 80, and a ramp between them
    that shifts with the row, so the edge of the binarised mask is not aligned to the 8 x 8 blocks"""
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    ramp = ((xx - 50.0 - (yy % 3)) / 28.0).clamp(0.0, 1.0)
    m = (255.0 * ramp).round().to(torch.uint8)
    m[:, :48] = 0
    m[:, 80:] = 255
    return m[None]


def mask_census(mask_u8):
    """(latent positions with c_mask = 1, with c_mask = 0, 8 x 8 blocks that hold both values of the binarised mask)"""
    m = binarise(mask_u8)
    c = latent_mask(mask_u8)
    n, h, w = m.shape
    s = m.reshape(n, h // 8, 8, w // 8, 8).sum(dim=(2, 4))
    return int((c == 1).sum()), int((c == 0).sum()), int(((s > 0) & (s < 64)).sum())


# ------------------------------------------------------------------ parameter table and config mirror
def test_param_table_of_a_9_channel_unet():
    from sdod.amd import engine as E
    t9 = E.UNet(E.sd14_config(16, 16, concat_channels=5), 2).param_table()
    t4 = E.UNet(E.sd14_config(16, 16, concat_channels=0), 2).param_table()
    today = E.UNet(E.sd14_config(16, 16), 2).param_table()
    d9 = dict(t9)
    assert d9['input_blocks.0.0.weight'] == (320, 9, 3, 3) and d9['input_blocks.0.0.bias'] == (320,)
    assert d9['out.2.weight'] == (4, 320, 3, 3) and d9['out.2.bias'] == (4,)
    assert t4 == today                                                     # entry for entry
    assert [n for n, _ in t9] == [n for n, _ in t4]
    assert [(n, s) for (n, s), (_, s4) in zip(t9, t4) if s != s4] == [('input_blocks.0.0.weight', (320, 9, 3, 3))]
    # SD 2 inpainting (512-inpainting-ema): the same one entry
    s9 = dict(E.UNet(E.sd21_config(16, 16, concat_channels=5), 2).param_table())
    assert s9['input_blocks.0.0.weight'] == (320, 9, 3, 3) and s9['out.2.weight'] == (4, 320, 3, 3)
    # the other graphs do not depend on it
    for cls in (E.Temb, E.VaeDecoder, E.VaeEncoder, E.TextEncoder):
        assert cls(E.sd14_config(16, 16, concat_channels=5), 1).param_table() == cls(E.sd14_config(16, 16), 1).param_table()


def test_a_concat_width_the_input_convolution_cannot_take_is_refused():
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    for cc in (7, 3, -1):                     # 9 * 11 > 96; 9 * 7 <= 64 (no K = 96 form); negative
        with pytest.raises(SdodError):
            E.UNet(E.sd14_config(16, 16, concat_channels=cc), 2)
    cfg = E.sd14_config(16, 16, concat_channels=5)
    cfg.model_channels = 192                  # the im2col + GEMM branch has no second source
    cfg.num_heads, cfg.head_dim = 0, 64       # (a head geometry this width admits: the refusal is the input convolution's)
    with pytest.raises(SdodError, match='concat_channels'):
        E.UNet(cfg, 2)
    cfg.concat_channels = 0
    assert dict(E.UNet(cfg, 2).param_table())['input_blocks.0.0.weight'] == (192, 4, 3, 3)


def test_model_config_mirror_has_the_size_the_library_fills():
    """the C side fills the struct through a pointer: guard words behind the mirror must survive, and the last field must be written"""
    from sdod.amd import engine as E

    class Guarded(ctypes.Structure):
        _fields_ = [('cfg', E.ModelConfig), ('guard', ctypes.c_uint32 * 8)]

    lib = E._engine()
    for fill in (lib.sdod_model_config_sd14, lib.sdod_model_config_sd21):
        g = Guarded()
        ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
        fill(ctypes.cast(ctypes.byref(g), ctypes.POINTER(E.ModelConfig)))
        assert list(g.guard) == [0xA5A5A5A5] * 8
        assert g.cfg.concat_channels == 0 and g.cfg.latent_channels == 4 and g.cfg.text_arch in (0, 1)
    names = [n for n, _ in E.ModelConfig._fields_]
    assert names[-1] == 'concat_channels' and names[-2] == 'weight_quant'
    assert ctypes.sizeof(E.ModelConfig) == 4 * len(names) == 64
    # every field the header declares, in its order
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'sdod_engine.h')).read()
    body = hdr[hdr.index('typedef struct sdod_model_config {'):hdr.index('} sdod_model_config;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.findall(r'\bint\s+(\w+)\s*;', body) == names


def test_new_symbols_resolve_and_are_bound():
    from sdod.amd import _lib, engine as E
    lib = _lib.hip()
    for s in ('sdod_conv_in_cat_f16', 'sdod_masked_image_conv_in_f16', 'sdod_inpaint_cond_f32'):
        assert s in _lib.HIP_SYMBOLS and getattr(lib, s).argtypes is not None
    assert 'sdod_graph_param_device' in E.ENGINE_SYMBOLS and hasattr(lib, 'sdod_graph_param_device')
    assert E.MaskedVaeEncoder(E.sd14_config(16, 16), 1).param_table() == E.VaeEncoder(E.sd14_config(16, 16), 1).param_table()


# ------------------------------------------------------------------ the restatement against itself
def test_latent_mask_is_nearest_interpolation_and_the_top_left_pixel():
    g = torch.Generator().manual_seed(3)
    for mask in (mask128(), torch.randint(0, 256, (2, 40, 56), generator=g, dtype=torch.uint8)):
        m = binarise(mask)
        c = latent_mask(mask)
        h, w = mask.shape[1] // 8, mask.shape[2] // 8
        assert c.dtype == torch.float32 and tuple(c.shape) == (mask.shape[0], h, w)
        assert torch.equal(c, F.interpolate(m[:, None].float(), size=(h, w))[:, 0])
        assert torch.equal(c, m[:, ::8, ::8].float())
        assert set(c.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(binarise(torch.tensor([[[0, 127, 128, 255]]], dtype=torch.uint8)), torch.tensor([[[False, False, True, True]]]))
    # not the 8 x 8 block mean that latent blending uses
    m = mask128()
    mean = 1.0 - (16320 - m.reshape(1, 16, 8, 16, 8).to(torch.int64).sum(dim=(2, 4))).float() / 16320.0
    assert not torch.equal(latent_mask(m), mean)


def test_mask128_meets_what_the_chain_test_needs():
    ones, zeros, mixed = mask_census(mask128())
    assert (ones, zeros, mixed) == (118, 138, 16)
    assert ones >= 64 and zeros >= 64 and mixed >= 1                    # both values well populated, an edge inside 8 x 8 blocks
    ones_i, zeros_i, mixed_i = mask_census(255 - mask128())
    assert ones_i >= 64 and zeros_i >= 64 and mixed_i == mixed


def test_masked_image_is_exactly_zero_where_repainted():
    g = torch.Generator().manual_seed(4)
    u8 = torch.randint(0, 256, (2, 16, 24, 3), generator=g, dtype=torch.uint8)
    mask = torch.randint(0, 256, (2, 16, 24), generator=g, dtype=torch.uint8)
    x = masked_image(u8, mask)
    m = binarise(mask)[:, None].expand_as(x)
    assert tuple(x.shape) == (2, 3, 16, 24)
    assert bool((x[m] == 0.0).all()) and int(m.sum()) > 100
    plain = (2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2)
    assert torch.equal(x[~m], plain[~m])
    assert bool((plain != 0.0).all())                                  # no uint8 value maps to 0.0: 127 -> -0.0039, 128 -> +0.0039
    assert float(plain.abs().min()) > 0.0039


def test_the_oracle_unet_takes_nine_channels_and_the_concatenation_order():
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet9 = S.UNetModel(in_ch=9)
    sd = unet9.state_dict()
    assert tuple(sd['input_blocks.0.0.weight'].shape) == (320, 9, 3, 3) and tuple(sd['out.2.weight'].shape) == (4, 320, 3, 3)
    seen = []

    def fake(x, t, ctx):
        seen.append(x)
        return x[:, :4]

    cond = torch.arange(5.0).reshape(1, 5, 1, 1).expand(1, 5, 2, 2) + 10
    x = torch.arange(4.0).reshape(1, 4, 1, 1).expand(2, 4, 2, 2).contiguous()
    out = concat_unet(fake, cond)(x, None, None)
    assert tuple(seen[0].shape) == (2, 9, 2, 2) and tuple(out.shape) == (2, 4, 2, 2)
    assert seen[0][0, :, 0, 0].tolist() == [0, 1, 2, 3, 10, 11, 12, 13, 14]            # x (4), c_mask (1), c_lat (4)
    assert torch.equal(seen[0][0, 4:], seen[0][1, 4:])                                  # both guidance halves: the same five channels


# ------------------------------------------------------------------ argument contract
def _args(n=1, hw=16):
    g = torch.Generator().manual_seed(1)
    return (torch.randint(0, 256, (n, 8 * hw, 8 * hw, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (n, 8 * hw, 8 * hw), generator=g, dtype=torch.uint8), torch.randn(n, 4, hw, hw, generator=g))


def _bare_pipe():
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)                               # no constructor: no graphs, no device
    pipe.cfg = E.sd14_config(16, 16, concat_channels=5)
    pipe.n = 1
    pipe.cfg_split = False
    return pipe


def test_inpaint_concat_check_args_accepts_the_contract():
    from sdod.amd.pipeline import inpaint_concat_check_args
    init, mask, x_T = _args()
    for sampler in ('plms', 'dpm'):
        inpaint_concat_check_args(init, mask, x_T, 20, sampler, None, (4, 16, 16), 1)
    inpaint_concat_check_args(init, mask, x_T.half(), 1, 'plms', torch.zeros(1, 4, 16, 16), (4, 16, 16), 1)


@pytest.mark.parametrize('case', ['mask_shape', 'mask_rank', 'mask_dtype', 'init_dtype', 'init_rank', 'size', 'batch', 'x_shape', 'x_dtype', 'x_none',
                                  'sampler', 'steps_zero', 'steps_frac', 'noise_shape', 'noise_type'])
def test_inpaint_concat_argument_errors_raise_before_device_work(case):
    """through Txt2Img.inpaint_concat and inpaint_concat_graphed themselves, on an object that has no device at all: any device work
    would fail with something other than ValueError"""
    pipe = _bare_pipe()
    init, mask, x_T = _args()
    kw = dict(steps=20, sampler='plms')
    if case == 'mask_shape':
        mask = mask[:, :-8]
    elif case == 'mask_rank':
        mask = mask[..., None]
    elif case == 'mask_dtype':
        mask = mask.float()
    elif case == 'init_dtype':
        init = init.float()
    elif case == 'init_rank':
        init = init[0]
    elif case == 'size':
        init, mask, x_T = _args(hw=24)
    elif case == 'batch':
        init, mask, x_T = _args(n=2)
    elif case == 'x_shape':
        x_T = x_T[:, :, :8]
    elif case == 'x_dtype':
        x_T = x_T.to(torch.int32)
    elif case == 'x_none':
        x_T = None
    elif case == 'sampler':
        kw['sampler'] = 'ddim'
    elif case == 'steps_zero':
        kw['steps'] = 0
    elif case == 'steps_frac':
        kw['steps'] = 2.5
    elif case == 'noise_shape':
        kw['noise'] = torch.zeros(1, 5, 16, 16)
    elif case == 'noise_type':
        kw['noise'] = (torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16))
    for fn in (pipe.inpaint_concat, pipe.inpaint_concat_graphed):
        with pytest.raises(ValueError):
            fn(None, init, mask, x_T, **kw)


def test_inpaint_concat_needs_a_pipeline_built_for_it():
    """good arguments on a pipeline without the 9-channel UNet: RuntimeError (after the argument checks, before any device work)"""
    pipe = _bare_pipe()
    init, mask, x_T = _args()
    for fn in (pipe.inpaint_concat, pipe.inpaint_concat_graphed):
        with pytest.raises(RuntimeError):
            fn(None, init, mask, x_T)
    pipe.masked_encoder = None
    with pytest.raises(RuntimeError):
        pipe.inpaint_concat(None, init, mask, x_T)


def test_generate_refuses_an_inpaint_unet_without_staged_conditioning():
    pipe = _bare_pipe()
    pipe.inpaint_unet, pipe._cond_staged = True, False
    _, _, x_T = _args()
    for fn in (pipe.generate, pipe.generate_graphed):
        with pytest.raises(RuntimeError, match='inpaint_concat'):
            fn(None, x_T)
    with pytest.raises(RuntimeError, match='inpaint_concat'):
        pipe._set_context(None)                                          # what every sampler calls before its first evaluation


# ------------------------------------------------------------------ checkpoint conversion
def _mini_tables():
    """a miniature of the real 9-channel tables: the entries this work changes or relies on, with their real names and shapes"""
    from sdod.amd import engine as E
    cfg = E.sd14_config(concat_channels=5)
    unet = dict(E.UNet(cfg, 2).param_table())
    enc = dict(E.VaeEncoder(cfg, 1).param_table())
    pick = lambda d, names: [(n, d[n]) for n in names]
    return {'unet': pick(unet, ['input_blocks.0.0.weight', 'input_blocks.0.0.bias', 'out.2.weight', 'out.2.bias']),
            'temb': [('time_embed.0.bias', (1280,))], 'vae': [('post_quant_conv.weight', (4, 4, 1, 1))],
            'text': [('text_model.final_layer_norm.weight', (768,))]}, pick(enc, ['encoder.conv_in.weight', 'quant_conv.bias'])


def test_a_9_channel_checkpoint_converts_and_round_trips(tmp_path, monkeypatch):
    from sdod.amd import convert, weights as Wt
    tables, enc_table = _mini_tables()
    assert dict(tables['unet'])['input_blocks.0.0.weight'] == (320, 9, 3, 3)
    seen = []

    def fake_tables(cfg=None):
        seen.append(None if cfg is None else cfg.concat_channels)
        return tables

    monkeypatch.setattr(convert, 'parameter_tables', fake_tables)
    monkeypatch.setattr(convert, 'vae_encoder_table', lambda cfg=None: enc_table)
    g = torch.Generator().manual_seed(5)
    allt = dict(tables, vae_enc=enc_table)
    prefixes = dict(convert.GRAPHS, **convert.OPTIONAL_GRAPHS)
    sd = {prefixes[gr][0] + n: torch.randn(s, generator=g) for gr, t in allt.items() for n, s in t}
    src = str(tmp_path / 'sd-v1-5-inpainting.ckpt')
    torch.save({'state_dict': sd}, src)
    out = tmp_path / 'models'
    convert.main(['--ckpt', src, '--out', str(out), '--inpaint'])
    assert seen == [5]                                                   # the tables were asked for with concat_channels = 5
    back = Wt.load(str(out / 'unet.sdodw'))
    assert [(n, tuple(t.shape)) for n, t in back.items()] == tables['unet']          # container -> parameter table, entry for entry
    assert torch.equal(back['input_blocks.0.0.weight'], sd['model.diffusion_model.input_blocks.0.0.weight'].half())
    assert (out / 'vae_encoder.sdodw').exists()                          # --inpaint implies the encoder the masked graph loads
    # a 4-channel checkpoint is refused by shape, not silently padded
    sd4 = dict(sd)
    sd4['model.diffusion_model.input_blocks.0.0.weight'] = torch.randn(320, 4, 3, 3, generator=g)
    src4 = str(tmp_path / 'sd-v1-4.ckpt')
    torch.save({'state_dict': sd4}, src4)
    with pytest.raises(ValueError, match='input_blocks.0.0.weight'):
        convert.main(['--ckpt', src4, '--out', str(tmp_path / 'm4'), '--inpaint'])


def test_split_state_dict_on_the_full_9_channel_table():
    """key / shape level on the real table (no payloads: meta tensors)"""
    from sdod.amd import convert, engine as E, weights as Wt
    cfg = E.sd14_config(concat_channels=5)
    table = E.UNet(cfg, 2).param_table()
    with torch.device('meta'):
        sd = {'model.diffusion_model.' + n: torch.empty(s) for n, s in table}
    tables = {'unet': table}
    # (split_state_dict converts dtype: meta tensors stay meta)
    parts, unused = convert.split_state_dict(sd, tables)
    assert tuple(parts['unet']['input_blocks.0.0.weight'].shape) == (320, 9, 3, 3) and unused == []
    synth = Wt.synthetic_state_dict([e for e in table if e[0].startswith('input_blocks.0.0') or e[0].startswith('out.2')], seed=1)
    assert tuple(synth['input_blocks.0.0.weight'].shape) == (320, 9, 3, 3)          # synthetic_state_dict follows the table
