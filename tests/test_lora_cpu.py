"""LoRA adapters, the host side (no GPU): key mapping against the graphs' parameter tables, the file reader, the host merge against
a direct fp64 formula, what is refused, and the argument checks of Txt2Img.set_loras."""
import re

import pytest
import torch


def _factors(shape, rank, gen, conv_down=False):
    """a self-consistent kohya pair for a weight of canonical `shape`: (down, up)"""
    out, cin = shape[0], shape[1]
    if len(shape) == 4:
        kh = shape[2]
        return torch.randn(rank, cin, kh, kh, generator=gen) * 0.1, torch.randn(out, rank, 1, 1, generator=gen) * 0.1
    return torch.randn(rank, cin, generator=gen) * 0.1, torch.randn(out, rank, generator=gen) * 0.1


_ATTN_MODULES = ['proj_in', 'proj_out', 'transformer_blocks_0_ff_net_0_proj', 'transformer_blocks_0_ff_net_2'] + \
    [f'transformer_blocks_0_{a}_{m}' for a in ('attn1', 'attn2') for m in ('to_q', 'to_k', 'to_v', 'to_out_0')]


def _unet_attention_blocks():
    """diffusers' attention blocks of the SD 1.x UNet, in network order"""
    return [f'down_blocks_{i}_attentions_{j}' for i in range(3) for j in range(2)] + ['mid_block_attentions_0'] + \
           [f'up_blocks_{i}_attentions_{j}' for i in (1, 2, 3) for j in range(3)]


@pytest.fixture(scope='module')
def tables():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    return dict(E.UNet(cfg, 2).param_table()), dict(E.TextEncoder(cfg, 1).param_table())


def test_attention_modules_map_one_to_one_onto_the_unet_table(tables):
    from sdod.amd import lora as L
    unet = tables[0]
    assert len(_ATTN_MODULES) == 12      # proj_in, proj_out, four projections each of attn1 and attn2, ff.net.0.proj, ff.net.2
    keys = [f'lora_unet_{b}_{m}' for b in _unet_attention_blocks() for m in _ATTN_MODULES]
    mapped = [L.map_key(k, 'sd14') for k in keys]
    assert all(g == 'unet' for g, _ in mapped)
    names = [n for _, n in mapped]
    want = sorted(n for n in unet if n.endswith('.weight') and len(unet[n]) >= 2 and
                  re.search(r'\.1\.(proj_in|proj_out|transformer_blocks\.)', n))
    assert len(set(names)) == len(names) and sorted(names) == want
    gen = torch.Generator().manual_seed(0)
    for k, n in zip(keys, names):
        down, up = _factors(unet[n], 4, gen)
        assert (up.shape[0], down.shape[1]) == tuple(unet[n][:2]), (k, n)
    # input_blocks indices increase with (i, j)
    idx = [int(re.match(r'input_blocks\.(\d+)\.', L.map_key(f'lora_unet_down_blocks_{i}_attentions_{j}_proj_in')[1]).group(1))
           for i in range(3) for j in range(2)]
    assert idx == sorted(idx) and len(set(idx)) == 6 and idx == [1, 2, 4, 5, 7, 8]


def test_convolution_modules_map_one_to_one_onto_the_unet_table(tables):
    from sdod.amd import lora as L
    unet = tables[0]
    res = [f'down_blocks_{i}_resnets_{j}' for i in range(4) for j in range(2)] + ['mid_block_resnets_0', 'mid_block_resnets_1'] + \
          [f'up_blocks_{i}_resnets_{j}' for i in range(4) for j in range(3)]
    names = []
    for r in res:
        for conv in ('conv1', 'conv2', 'conv_shortcut'):
            n = L.map_key(f'lora_unet_{r}_{conv}')[1]
            if conv == 'conv_shortcut' and n not in unet:      # only the ResBlocks that change width have one
                continue
            names.append(n)
    names += [L.map_key(f'lora_unet_down_blocks_{i}_downsamplers_0_conv')[1] for i in range(3)]
    names += [L.map_key(f'lora_unet_up_blocks_{i}_upsamplers_0_conv')[1] for i in range(3)]
    want = sorted(n for n in unet if n.endswith('.weight') and len(unet[n]) == 4 and
                  re.search(r'(in_layers\.2|out_layers\.3|skip_connection|\.op|\.conv)\.weight$', n))
    assert len(set(names)) == len(names) and sorted(names) == want
    gen = torch.Generator().manual_seed(1)
    for n in names:
        down, up = _factors(unet[n], 4, gen)
        assert (up.shape[0], down.shape[1]) == tuple(unet[n][:2]) and down.shape[2:] == unet[n][2:]
    # every matrix of the UNet but the input / output convolutions is reachable
    attn = {L.map_key(f'lora_unet_{b}_{m}')[1] for b in _unet_attention_blocks() for m in _ATTN_MODULES}
    rest = sorted(n for n in unet if len(unet[n]) >= 2 and n not in attn and n not in names)
    assert rest == ['input_blocks.0.0.weight', 'out.2.weight'], rest


def test_text_modules_map_one_to_one_onto_the_text_table(tables):
    from sdod.amd import lora as L
    text = tables[1]
    mods = [f'self_attn_{m}_proj' for m in ('q', 'k', 'v', 'out')] + ['mlp_fc1', 'mlp_fc2']
    mapped = [L.map_key(f'lora_te_text_model_encoder_layers_{n}_{m}') for n in range(12) for m in mods]
    assert all(g == 'text' for g, _ in mapped)
    names = [n for _, n in mapped]
    want = sorted(n for n in text if n.startswith('text_model.encoder.layers.') and len(text[n]) == 2)
    assert len(names) == 72 and sorted(names) == want
    gen = torch.Generator().manual_seed(2)
    for n in names:
        down, up = _factors(text[n], 4, gen)
        assert (up.shape[0], down.shape[1]) == tuple(text[n])


def test_read_lora_round_trip(tmp_path):
    from safetensors.torch import save_file
    from sdod.amd import lora as L
    gen = torch.Generator().manual_seed(3)
    a, b = 'lora_unet_mid_block_attentions_0_proj_in', 'lora_te_text_model_encoder_layers_0_mlp_fc1'
    raw = {f'{a}.lora_down.weight': torch.randn(4, 1280, 1, 1, generator=gen).half(), f'{a}.lora_up.weight': torch.randn(1280, 4, 1, 1, generator=gen).half(),
           f'{a}.alpha': torch.tensor(2.0),
           f'{b}.lora_down.weight': torch.randn(8, 768, generator=gen), f'{b}.lora_up.weight': torch.randn(3072, 8, generator=gen)}
    path = tmp_path / 'adapter.safetensors'
    save_file(raw, str(path))
    got = L.read_lora(str(path))
    assert sorted(got) == sorted([a, b]) and got.other == ()
    assert torch.equal(got[a][0], raw[f'{a}.lora_down.weight']) and torch.equal(got[a][1], raw[f'{a}.lora_up.weight']) and got[a][2] == 2.0
    assert torch.equal(got[b][1], raw[f'{b}.lora_up.weight']) and got[b][2] == 8.0          # no alpha: alpha = rank
    torch.save(raw, str(tmp_path / 'adapter.pt'))
    again = L.read_lora(str(tmp_path / 'adapter.pt'))
    assert sorted(again) == sorted(got) and again[a][2] == 2.0
    ent, skipped = L.entries_for(got, 'sd14', 0.5, 2.0)
    assert skipped == [] and [e[0] for e in ent['unet']] == ['middle_block.1.proj_in.weight']
    assert ent['unet'][0][3] == pytest.approx(0.5 * 2.0 / 4) and ent['text'][0][3] == pytest.approx(2.0 * 8.0 / 8)
    assert ent['text'][0][0] == 'text_model.encoder.layers.0.mlp.fc1.weight'


def test_merged_state_dict_matches_the_direct_formula():
    import torch.nn.functional as F
    from sdod.amd import lora as L
    gen = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    sd = {'lin.weight': r(24, 40).float(), 'c1.weight': r(16, 16, 1, 1).half(), 'c3.weight': r(12, 8, 3, 3).float(), 'lin.bias': r(24).float()}
    ent = [('lin.weight', r(24, 3).float(), r(3, 40).float(), 0.7),
           ('c1.weight', r(16, 2, 1, 1).half(), r(2, 16, 1, 1).half(), -1.5),
           ('c3.weight', r(12, 4, 1, 1).float(), r(4, 8, 3, 3).float(), 0.9),
           ('lin.weight', r(24, 5).float(), r(5, 40).float(), 0.25)]                      # a second adapter on the same weight
    out = L.merged_state_dict(sd, ent)
    assert out['lin.bias'] is sd['lin.bias'] and all(out[k].dtype == sd[k].dtype and out[k].shape == sd[k].shape for k in sd)
    lin = sd['lin.weight'].double() + 0.7 * ent[0][1].double() @ ent[0][2].double() + 0.25 * ent[3][1].double() @ ent[3][2].double()
    assert torch.equal(out['lin.weight'], lin.float())
    c1 = sd['c1.weight'].double() - 1.5 * (ent[1][1].double().reshape(16, 2) @ ent[1][2].double().reshape(2, 16)).reshape(16, 16, 1, 1)
    assert torch.equal(out['c1.weight'], c1.half())
    # the 3x3 case by what the convolution computes: conv(x, W + dW) = conv(x, W) + scale * conv1x1(conv3x3(x, down), up)
    x = r(2, 8, 6, 5)
    up, down = ent[2][1].double(), ent[2][2].double()
    want = F.conv2d(x, sd['c3.weight'].double(), padding=1) + 0.9 * F.conv2d(F.conv2d(x, down, padding=1), up)
    got = F.conv2d(x, out['c3.weight'].double(), padding=1)
    # out is the fp32 rounding of the fp64 sum: 2^-24 relative per weight, 72 of them per output
    assert float((got - want).abs().max()) <= 72 * 2.0 ** -24 * float(x.abs().max()) * float(out['c3.weight'].abs().max())
    with pytest.raises(ValueError):
        L.merged_state_dict(sd, [('lin.weight', r(24, 3), r(3, 41), 1.0)])
    with pytest.raises(KeyError):
        L.merged_state_dict(sd, [('nope.weight', r(24, 3), r(3, 40), 1.0)])


def test_refusals():
    from sdod.amd import lora as L
    z = lambda *s: torch.zeros(*s)
    ok = 'lora_unet_mid_block_attentions_0_proj_in'
    raw = {f'{ok}.lora_down.weight': z(4, 1280), f'{ok}.lora_up.weight': z(1280, 4)}
    bad = {'lora_unet_down_blocks_0_resnets_0_time_emb_proj': ((4, 1280), (320, 4)),
           'lora_unet_conv_in': ((4, 4, 3, 3), (320, 4, 1, 1)),
           'lora_te_text_model_encoder_layers_0_mlp_fc1': ((4, 1024), (4096, 4))}
    for k, (d, u) in bad.items():
        raw[f'{k}.lora_down.weight'] = z(*d)
        raw[f'{k}.lora_up.weight'] = z(*u)
    loha = 'lora_unet_mid_block_attentions_0_proj_out'
    for t in ('hada_w1_a', 'hada_w1_b', 'hada_w2_a', 'hada_w2_b'):
        raw[f'{loha}.{t}'] = z(4, 4)
    dora = 'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn1_to_q'
    raw.update({f'{dora}.lora_down.weight': z(4, 1280), f'{dora}.lora_up.weight': z(1280, 4), f'{dora}.dora_scale': z(1, 1280)})
    with pytest.raises(ValueError) as e:
        L.entries_for(raw, 'sd21')
    for k in list(bad) + [loha, dora]:
        assert k in str(e.value), k
    assert 'TEMB' in str(e.value) and 'OpenCLIP' in str(e.value)
    ent, skipped = L.entries_for(raw, 'sd21', strict=False)
    assert sorted(skipped) == sorted(list(bad) + [loha, dora])
    assert [x[0] for x in ent['unet']] == ['middle_block.1.proj_in.weight'] and ent['text'] == []
    ent14, skipped14 = L.entries_for(raw, 'sd14', strict=False)                          # on sd14 the text module is taken
    assert len(ent14['text']) == 1 and 'lora_te_text_model_encoder_layers_0_mlp_fc1' not in skipped14
    for k in ('lora_unet_conv_out', 'lora_unet_down_blocks_3_attentions_0_proj_in', 'lora_unet_up_blocks_0_attentions_0_proj_in',
              'lora_unet_up_blocks_3_upsamplers_0_conv', 'lora_te_text_model_embeddings_token_embedding', 'something_else'):
        with pytest.raises(ValueError):
            L.map_key(k, 'sd14')


def test_set_loras_argument_checks():
    from sdod.amd.pipeline import Txt2Img
    p = Txt2Img.__new__(Txt2Img)
    with pytest.raises(RuntimeError, match='loras=True'):
        p.set_loras([])
    with pytest.raises(RuntimeError, match='loras=True'):
        p.clear_loras()
    p._loras = True
    for bad in (float('nan'), float('inf'), '0.8', None, True):
        with pytest.raises(ValueError, match='strength'):
            p.set_loras([({}, bad)])
        with pytest.raises(ValueError, match='strength'):
            p.set_loras([({}, 1.0, bad)])
    with pytest.raises(ValueError):
        p.set_loras([({},)])
    with pytest.raises(ValueError):
        p.set_loras(['adapter.safetensors'])
