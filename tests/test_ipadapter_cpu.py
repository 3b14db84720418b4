"""Image prompts without a GPU: the vision-tower restatement of tests/ipadapter_ref.py against transformers'
CLIPVisionModelWithProjection, the converter's block table and refusals, every refusal of Txt2Img(ip_adapter=True) and of its setters
before any device work, the weights definition, and the parameter tables of the new graphs."""
import ctypes

import numpy as np
import pytest
import torch

import ipadapter_ref as IR


# ------------------------------------------------------------------ the vision restatement is HF's model
@pytest.mark.parametrize('act,heads,width', [('gelu', 2, 128), ('quick_gelu', 4, 256)])
def test_vision_restatement_equals_transformers(act, heads, width):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(width)
    cfg = CLIPVisionConfig(hidden_size=width, intermediate_size=2 * width, projection_dim=64, num_hidden_layers=2, num_attention_heads=heads,
                           image_size=28, patch_size=14, hidden_act=act)
    model = CLIPVisionModelWithProjection(cfg).eval()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, v in sd.items():                                             # biases and norms off their initial 0 / 1
        if v.dim() == 1:
            v.add_(0.1 * torch.randn(v.shape))
    model.load_state_dict(sd)
    from sdod.amd import engine as E
    enc = E.ImageEncoder(E.VisionConfig(28, 14, width, 2, heads, 2 * width, 64, int(act == 'quick_gelu')), 1)
    want = dict(enc.checkpoint_table())
    floats = {k: v for k, v in sd.items() if v.is_floating_point()}
    assert set(want) == set(floats)                                      # key by key: HF's names, the checkpoint's shapes
    assert all(tuple(floats[k].shape) == tuple(want[k]) for k in want)
    img = torch.randint(0, 256, (2, 28, 28, 3), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(torch.uint8)
    pixel_values = IR.patch_rows(img, 1).reshape(2, 28, 28, 3).permute(0, 3, 1, 2).contiguous()      # (u / 255 - mean) / std, NCHW
    with torch.no_grad():
        ref = model(pixel_values=pixel_values).image_embeds
    got = IR.vision_forward(sd, img, 14, heads, act == 'quick_gelu')
    err = float((got - ref).abs().max() / ref.abs().max())
    assert got.shape == ref.shape and err < 1e-5, err                    # fp32 rounding
    got64 = IR.vision_forward({k: v.double() for k, v in floats.items()}, img, 14, heads, act == 'quick_gelu')
    assert float((got64.float() - ref).abs().max() / ref.abs().max()) < 1e-5


def test_patch_rows_follow_the_conv_weights_flattening():
    img = torch.randint(0, 256, (1, 28, 28, 3), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(torch.uint8)
    w = torch.randn(8, 3, 14, 14, generator=torch.Generator().manual_seed(3))
    x = IR.patch_rows(img, 1).reshape(1, 28, 28, 3).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x, w, stride=14).flatten(2).transpose(1, 2).reshape(4, 8)
    got = IR.patch_rows(img, 14) @ w.reshape(8, -1).T
    assert float((got - ref).abs().max()) < 1e-4
    padded = IR.patch_rows(img, 14, kpad=640)
    assert tuple(padded.shape) == (4, 640) and float(padded[:, 588:].abs().max()) == 0


# ------------------------------------------------------------------ the weights definition
@pytest.mark.parametrize('hw', [(8, 8), (8, 16), (16, 16)])
def test_weights_definition(hw):
    ih, iw = 8 * hw[0], 8 * hw[1]
    for scale in (0.0, 0.7, 1.0):
        none = IR.ip_weights(scale, hw)
        full = IR.ip_weights(scale, hw, torch.full((ih, iw), 255, dtype=torch.uint8))
        zero = IR.ip_weights(scale, hw, torch.zeros(ih, iw, dtype=torch.uint8))
        soft = IR.ip_weights(scale, hw, IR.soft_mask(hw, 4))
        for lvl, ds in enumerate(IR.LEVELS):
            shape = ((hw[0] // ds) * (hw[1] // ds), 2)
            assert all(tuple(w[lvl].shape) == shape and w[lvl].dtype == torch.float32 for w in (none, full, zero, soft))
            assert all(bool((w[lvl][:, 0] == 1).all()) for w in (none, full, zero, soft))
            assert torch.equal(none[lvl], full[lvl]) and bool((none[lvl][:, 1] == np.float32(scale)).all())
            assert bool((zero[lvl][:, 1] == 0).all())
            # random bytes, against the definition spelled out pixel by pixel in exact arithmetic, rounded as the definition rounds
            m = IR.soft_mask(hw, 4).numpy().astype(np.int64)
            b = 8 * ds
            for (y, x) in ((0, 0), (hw[0] // ds - 1, hw[1] // ds - 1)):
                s = int(m[y * b:(y + 1) * b, x * b:(x + 1) * b].sum())
                want = np.float32(scale) * (np.float32(s) / np.float32(255 * b * b))
                assert soft[lvl][y * (hw[1] // ds) + x, 1].item() == float(want)
    half = torch.zeros(ih, iw, dtype=torch.uint8); half[:, :iw // 2] = 255
    w = IR.ip_weights(1.0, hw, half)
    assert w[0].view(hw[0], hw[1], 2)[0, 0, 1] == 1 and w[0].view(hw[0], hw[1], 2)[0, hw[1] - 1, 1] == 0
    assert w[3].view(hw[0] // 8, hw[1] // 8, 2)[0, 0, 1] == (0.5 if hw[1] == 8 else 1.0)


# ------------------------------------------------------------------ the converter
def _checkpoint(tokens=4, embed=1024, dialect='flat', ctx=768):
    from sdod.amd import ip_adapter as IP
    g = torch.Generator().manual_seed(tokens + embed)
    proj = {'proj.weight': torch.randn(tokens * ctx, embed, generator=g), 'proj.bias': torch.randn(tokens * ctx, generator=g),
            'norm.weight': torch.randn(ctx, generator=g), 'norm.bias': torch.randn(ctx, generator=g)}
    kv = {}
    for j, (_, width) in enumerate(IP.BLOCKS):
        for which in 'kv':
            kv[f'{2 * j + 1}.to_{which}_ip.weight'] = torch.randn(width, ctx, generator=g)
    if dialect == 'nested':
        return {'image_proj': proj, 'ip_adapter': kv}
    return {**{'image_proj.' + k: v for k, v in proj.items()}, **{'ip_adapter.' + k: v for k, v in kv.items()}}


def test_block_table_is_the_attn_processors_order():
    from sdod.amd import engine as E, ip_adapter as IP
    names = [b for b, _ in IP.BLOCKS]
    assert names == [f'input_blocks.{i}.1' for i in (1, 2, 4, 5, 7, 8)] + [f'output_blocks.{i}.1' for i in range(3, 12)] + ['middle_block.1']
    assert [w for _, w in IP.BLOCKS] == [320, 320, 640, 640, 1280, 1280] + [1280] * 3 + [640] * 3 + [320] * 3 + [1280]
    cfg = E.copy_config(E.sd14_config(16, 16)); cfg.ip_tokens = 4
    table = dict(E.UNet(cfg, 2).param_table())
    keys = {IP.unet_key(j, w) for j in range(16) for w in 'kv'}
    assert keys == {n for n in table if '_ip.' in n}                      # every block of the UNet, once
    assert all(table[IP.unet_key(j, w)] == (IP.BLOCKS[j][1], 768) for j in range(16) for w in 'kv')


@pytest.mark.parametrize('dialect', ['flat', 'nested'])
def test_converter_maps_both_key_dialects(dialect, tmp_path):
    from sdod.amd import convert, ip_adapter as IP, weights
    ck = _checkpoint(dialect=dialect)
    part = IP.adapter_parameters(ck, torch.float32)
    flat = IP.flatten(ck)
    assert len(part) == 36
    for j in range(16):
        for w in 'kv':
            assert torch.equal(part[IP.unet_key(j, w)], flat[f'ip_adapter.{2 * j + 1}.to_{w}_ip.weight'])
    assert all(torch.equal(part[n], flat['image_proj.' + n]) for n in ('proj.weight', 'proj.bias', 'norm.weight', 'norm.bias'))
    path = tmp_path / ('ip-adapter_sd15.safetensors' if dialect == 'flat' else 'ip-adapter_sd15.bin')
    if dialect == 'flat':
        from safetensors.torch import save_file
        save_file(ck, str(path))
    else:
        torch.save(ck, str(path))
    out = convert.convert_ip_adapter(str(path), str(tmp_path / 'models'))
    assert out.endswith('ip_adapter.sdodw') and weights.shapes(out)['proj.weight'] == (4 * 768, 1024)
    back = weights.load(out)
    assert set(back) == set(part) and all(torch.equal(back[k], part[k].half()) for k in part)
    assert IP.ip_sources(None, str(tmp_path / 'models')) == (4, 1024, None)
    convert.main(['--ip-adapter', str(path), '--out', str(tmp_path / 'cli')])
    assert (tmp_path / 'cli' / 'ip_adapter.sdodw').exists()


def test_converter_refusals_by_name():
    from sdod.amd import ip_adapter as IP
    ck = _checkpoint()
    for extra, word in (({'image_proj.latents': torch.zeros(1, 16, 768)}, 'image_proj.latents'),
                        ({'image_proj.layers.0.0.to_q.weight': torch.zeros(4, 4)}, 'image_proj.layers')):
        with pytest.raises(ValueError, match=word):
            IP.adapter_parameters({**ck, **extra})
    with pytest.raises(ValueError, match='plus'):
        IP.adapter_parameters({'image_proj': {'latents': torch.zeros(1)}, 'ip_adapter': {}})
    xl = {**ck, **{f'ip_adapter.{2 * j + 1}.to_{w}_ip.weight': torch.zeros(640, 2048) for j in range(16, 70) for w in 'kv'}}
    with pytest.raises(ValueError, match='SDXL'):
        IP.adapter_parameters(xl)
    with pytest.raises(ValueError, match='SDXL'):
        IP.adapter_parameters({**ck, 'ip_adapter.1.to_k_ip.weight': torch.zeros(640, 2048)})
    with pytest.raises(ValueError, match='context width'):
        IP.adapter_parameters(_checkpoint(ctx=1024))
    swapped = dict(ck)
    swapped['ip_adapter.5.to_k_ip.weight'], swapped['ip_adapter.9.to_k_ip.weight'] = ck['ip_adapter.9.to_k_ip.weight'], ck['ip_adapter.5.to_k_ip.weight']
    with pytest.raises(ValueError, match=r'ip_adapter\.5\.to_k_ip\.weight: 1280 rows, but input_blocks\.4\.1 \(cross-attention 2\) is 640 wide'):
        IP.adapter_parameters(swapped)
    missing = {k: v for k, v in ck.items() if k != 'ip_adapter.31.to_v_ip.weight'}
    with pytest.raises(KeyError, match='ip_adapter.31.to_v_ip.weight'):
        IP.adapter_parameters(missing)
    with pytest.raises(ValueError, match='not an IP-Adapter'):
        IP.adapter_parameters({'model.diffusion_model.out.2.weight': torch.zeros(1)})
    with pytest.raises(ValueError, match='proj.weight'):
        IP.adapter_parameters({**ck, 'image_proj.proj.weight': torch.zeros(17 * 768, 1024)})


def test_image_encoder_conversion(tmp_path):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from sdod.amd import convert, engine as E, ip_adapter as IP, weights
    torch.manual_seed(0)
    cfg = CLIPVisionConfig(hidden_size=128, intermediate_size=256, projection_dim=64, num_hidden_layers=2, num_attention_heads=2, image_size=28,
                           patch_size=14, hidden_act='quick_gelu')
    sd = CLIPVisionModelWithProjection(cfg).state_dict()
    assert IP.vision_config_of(sd) == (28, 14, 128, 2, 2, 256, 64, 1)
    part = IP.image_encoder_parameters(sd, torch.float32)
    enc = E.ImageEncoder(E.VisionConfig(28, 14, 128, 2, 2, 256, 64, 1), 1)
    assert {k: tuple(v.shape) for k, v in part.items() if k != IP.CONFIG_KEY} == dict(enc.param_table())
    pw = part['vision_model.embeddings.patch_embedding.weight']
    assert torch.equal(pw[:, :588], sd['vision_model.embeddings.patch_embedding.weight'].reshape(128, -1)) and float(pw[:, 588:].abs().max()) == 0
    assert part[IP.CONFIG_KEY].tolist() == [28, 14, 128, 2, 2, 256, 64, 1]
    from safetensors.torch import save_file
    (tmp_path / 'enc').mkdir()
    save_file({k: v.contiguous() for k, v in sd.items() if v.is_floating_point()}, str(tmp_path / 'enc' / 'model.safetensors'))
    out = convert.convert_image_encoder(str(tmp_path / 'enc'), str(tmp_path / 'models'))
    assert weights.shapes(out)['vision_model.embeddings.class_embedding'] == (1, 128)
    weights.save(str(tmp_path / 'models' / 'ip_adapter.sdodw'), IP.adapter_parameters(_checkpoint(embed=64)))
    assert IP.ip_sources(None, str(tmp_path / 'models')) == (4, 64, (28, 14, 128, 2, 2, 256, 64, 1))
    weights.save(str(tmp_path / 'models' / 'ip_adapter.sdodw'), IP.adapter_parameters(_checkpoint(embed=128)))
    with pytest.raises(ValueError, match='64-wide'):
        IP.ip_sources(None, str(tmp_path / 'models'))
    with pytest.raises(ValueError, match='not a CLIPVisionModelWithProjection'):
        IP.image_encoder_parameters({'text_model.x': torch.zeros(1)})


# ------------------------------------------------------------------ the pipeline's refusals, before any device work
def test_build_refusals_name_ip_adapter():
    from sdod.amd import ip_adapter as IP, pipeline as PL
    assert IP.ip_check_build(False) is False and IP.ip_check_build(None) is False and IP.ip_check_build(True) is True
    for bad in (1, 'yes', 4, 0.5):
        with pytest.raises(ValueError, match='ip_adapter must be'):
            IP.ip_check_build(bad)
    cases = [(dict(regions=2), 'regions'), (dict(prompt_chunks=2), 'prompt_chunks'), (dict(cfg_split=True), 'cfg_split'),
             (dict(hires_hw=32), 'hires_hw'), (dict(controlnet=True), 'controlnet'), (dict(adapter=True), 'adapter'), (dict(tiling=True), 'tiling'),
             (dict(inpaint_unet=True), 'inpaint_unet'), (dict(model='sd21'), 'sd21'), (dict(weight_quant=True), 'uint8')]
    for kw, word in cases:
        with pytest.raises(ValueError, match=f'ip_adapter cannot be combined with .*{word}'):
            IP.ip_check_build(True, **kw)
        with pytest.raises(ValueError, match=f'ip_adapter cannot be combined with .*{word}'):      # raised before any device work
            PL.Txt2Img(state_dicts={}, latent_hw=16, with_text_encoder=False, ip_adapter=True, **kw)

    class Codes:
        shape = (320, 320)

        def payload(self):
            return b''
    with pytest.raises(ValueError, match='ip_adapter cannot be combined with uint8 weights'):
        PL.Txt2Img(state_dicts={'unet': {'w': Codes()}}, latent_hw=16, ip_adapter=True)
    with pytest.raises(ValueError, match=r"state_dicts\['ip_adapter'\]"):
        PL.Txt2Img(state_dicts={'unet': {}}, latent_hw=16, ip_adapter=True)
    with pytest.raises(ValueError, match='ip_adapter.sdodw'):
        PL.Txt2Img(models_dir='/nonexistent-models-dir', latent_hw=16, ip_adapter=True)
    with pytest.raises(ValueError, match='proj.weight'):
        PL.Txt2Img(state_dicts={'unet': {}, 'ip_adapter': {'proj.weight': torch.zeros(17 * 768, 64)}}, latent_hw=16, ip_adapter=True)


def test_setters_need_the_flag_and_check_their_arguments():
    from sdod.amd import engine as E, ip_adapter as IP
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    assert pipe.ip_tokens == 0
    for call in (lambda: pipe.set_image_prompt(embeds=torch.zeros(1, 1024)), pipe.clear_image_prompt,
                 lambda: pipe.set_image_prompt(torch.zeros(1, 224, 224, 3, dtype=torch.uint8)), lambda: pipe.image_embeds(torch.zeros(1))):
        with pytest.raises(RuntimeError, match='ip_adapter=True'):
            call()
    pipe.ip_tokens, pipe.ip_proj_dim, pipe.ip_image_size, pipe.n = 4, 1024, 224, 2
    pipe.cfg = E.sd14_config(8, 16)
    img = torch.zeros(2, 224, 224, 3, dtype=torch.uint8)
    emb = torch.zeros(2, 1024)
    mask = torch.zeros(64, 128, dtype=torch.uint8)
    out = IP.ip_check_args(pipe, img, None, 0.7, mask.numpy())
    assert out[0] is img or torch.equal(out[0], img)
    assert out[1] is None and out[2] == 0.7 and torch.is_tensor(out[3]) and tuple(out[3].shape) == (64, 128)
    out = IP.ip_check_args(pipe, None, emb.half().numpy(), 1, None)
    assert out[0] is None and out[1].dtype == torch.float16 and out[2] == 1.0 and out[3] is None
    bad_calls = [dict(image_u8=img, embeds=emb), dict(), dict(image_u8=img.float()), dict(image_u8=img[:1]), dict(image_u8=img[:, :112]),
                 dict(image_u8=img[..., :1]), dict(image_u8=[[0]]), dict(embeds=emb[:1]), dict(embeds=emb[:, :768]), dict(embeds=emb.double()),
                 dict(embeds=emb.to(torch.int32)), dict(embeds=torch.full((2, 1024), float('nan'))), dict(embeds=emb, weight=-0.1),
                 dict(embeds=emb, weight=float('nan')), dict(embeds=emb, weight=float('inf')), dict(embeds=emb, weight='1'), dict(embeds=emb, weight=True),
                 dict(embeds=emb, mask_u8=mask.float()), dict(embeds=emb, mask_u8=mask[:32]), dict(embeds=emb, mask_u8=mask[None]),
                 dict(embeds=emb, mask_u8=torch.zeros(128, 64, dtype=torch.uint8))]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            pipe.set_image_prompt(**kw)                                  # raises before any device work (there is no device object here)
    pipe.ip_image_size = None                                            # no image encoder: image_u8 is refused, by name
    with pytest.raises(ValueError, match='no image encoder'):
        pipe.set_image_prompt(img)
    with pytest.raises(ValueError, match='no image encoder'):
        pipe.image_embeds(img)


# ------------------------------------------------------------------ library, host side
def test_new_symbols_are_exported_and_bound():
    from sdod.amd import _lib, engine as E, ops
    lib = _lib.hip()
    for s in ('sdod_xattn_fold_ip_f16', 'sdod_ip_weights_f32', 'sdod_patch_embed_u8_f16', 'sdod_vit_tokens_f16'):
        assert s in _lib.HIP_SYMBOLS and getattr(lib, s).argtypes is not None
    E._engine()
    for s in ('sdod_graph_create_ip', 'sdod_graph_create_vision'):
        assert s in E.ENGINE_SYMBOLS and getattr(lib, s).argtypes is not None
    assert all(hasattr(ops, n) for n in ('xattn_fold_ip', 'ip_weights', 'patch_embed', 'vit_tokens'))
    assert ctypes.sizeof(E.IpConfig) == 4 and ctypes.sizeof(E.VisionConfig) == 32
    assert [n for n, _ in E.VisionConfig._fields_] == ['image_size', 'patch', 'width', 'layers', 'heads', 'mlp_dim', 'proj_dim', 'quick_gelu']
    # the public layouts did not move
    assert _lib.GemmDesc._fields_[-1][0] == 'pad_mode' and ctypes.sizeof(E.ModelConfig) == 16 * 4 and ctypes.sizeof(E.RegionConfig) == 4
    assert (E.IMAGE_ENCODER, E.IMAGE_PROJ) == (10, 11) and tuple(getattr(E.vit_h14_config(), n) for n, _ in E.VisionConfig._fields_) == \
        (224, 14, 1280, 32, 16, 5120, 1024, 0)


def test_ip_config_travels_with_copies_and_only_adds_parameters():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    assert cfg.ip_tokens == 0 and E.copy_config(cfg).ip_tokens == 0
    c2 = E.copy_config(cfg); c2.ip_tokens = 4
    assert E.copy_config(c2).ip_tokens == 4 and cfg.ip_tokens == 0
    plain, ip = E.UNet(cfg, 2).param_table(), E.UNet(c2, 2).param_table()
    assert [p for p in ip if '_ip.' not in p[0]] == plain and len(ip) == len(plain) + 32
    assert E.Temb(c2, 2).param_table() == E.Temb(cfg, 2).param_table()   # the flag is the UNet's alone
    for bad, word in ((17, 'ip_tokens'), (-1, 'ip_tokens')):
        cb = E.copy_config(cfg); cb.ip_tokens = bad
        with pytest.raises(Exception, match=word):
            E.UNet(cb, 2)
    for field, value, word in (('context_len', 154, 'context_len'), ('weight_quant', 1, 'weight_quant'), ('concat_channels', 5, 'concat_channels')):
        cb = E.copy_config(c2); setattr(cb, field, value)
        with pytest.raises(Exception, match=word):
            E.UNet(cb, 2)
    for field in ('regions', 'control_inputs', 'tiling', 'adapter_reps'):
        cb = E.copy_config(c2); setattr(cb, field, 2 if field in ('regions', 'adapter_reps') else 1)
        if field == 'regions':
            cb.context_len = 154
        with pytest.raises(ValueError, match='image prompt'):
            E.UNet(cb, 2)


def test_vision_graphs_have_their_own_entry_point():
    from sdod.amd import _lib, engine as E
    lib = E._engine()
    cfg = E.sd14_config(16, 16)
    h = ctypes.c_void_p()
    for kind in (E.IMAGE_ENCODER, E.IMAGE_PROJ):                         # the other create functions refuse the kinds
        assert lib.sdod_graph_create(ctypes.byref(h), kind, ctypes.byref(cfg), 2) != 0 and not h.value
        assert lib.sdod_graph_create_ip(ctypes.byref(h), kind, ctypes.byref(cfg), ctypes.byref(E.IpConfig(4)), 2) != 0 and not h.value
    v = E.vit_h14_config()
    assert lib.sdod_graph_create_vision(ctypes.byref(h), E.UNET, ctypes.byref(cfg), ctypes.byref(v), ctypes.byref(E.IpConfig(4)), 2) != 0
    assert lib.sdod_graph_create_vision(ctypes.byref(h), E.IMAGE_ENCODER, None, None, None, 2) != 0
    assert lib.sdod_graph_create_vision(ctypes.byref(h), E.IMAGE_PROJ, ctypes.byref(cfg), ctypes.byref(v), None, 2) != 0
    for bad in ((224, 14, 1280, 32, 10, 5120, 1024, 0), (225, 14, 1280, 32, 16, 5120, 1024, 0), (224, 14, 1280, 0, 16, 5120, 1024, 0),
                (224, 14, 1290, 32, 16, 5120, 1024, 0), (224, 14, 1280, 32, 16, 5120, 1000, 0), (224, 14, 1280, 32, 16, 5120, 1024, 2)):
        with pytest.raises(_lib.SdodError):
            E.ImageEncoder(E.VisionConfig(*bad), 1)
    enc = E.ImageEncoder(v, 1)
    t = dict(enc.param_table())
    assert t['vision_model.embeddings.patch_embedding.weight'] == (1280, 640) and t['vision_model.embeddings.position_embedding.weight'] == (257, 1280)
    assert t['visual_projection.weight'] == (1024, 1280) and len(t) == 5 + 32 * 16 + 3
    assert dict(enc.checkpoint_table())['vision_model.embeddings.patch_embedding.weight'] == (1280, 3, 14, 14)
    proj = E.ImageProj(cfg, 1024, 4, 2)
    assert proj.param_table() == [('proj.weight', (3072, 1024)), ('proj.bias', (3072,)), ('norm.weight', (768,)), ('norm.bias', (768,))]
    text = E.TextEncoder(cfg, 1).param_table()                          # the text tower keeps its table: the shared block lists the same names
    assert len(text) == 196 and text[0][0] == 'text_model.embeddings.token_embedding.weight' and text[2][0] == 'text_model.encoder.layers.0.layer_norm1.weight'
