"""img2img on the host side (no GPU): the opt-in VAE-encoder checkpoint split, ldm's img2img schedule indices, the strength
domain, and the ctypes mirror of the GEMM descriptor's new pad_mode field.

LdmEncoder is the fp32 restatement of ldm's `Encoder` (ch 128, ch_mult (1, 2, 4, 4), 2 ResBlocks per level, double_z) + the
`quant_conv` of AutoencoderKL, built from oracle.sd_torch's VAE blocks; the GPU tests (test_img2img_gpu.py) use it as the oracle."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


class LdmDownsample(nn.Module):
    """ldm Downsample(with_conv=True): F.pad(x, (0, 1, 0, 1)) then a 3x3 stride-2 pad-0 conv"""

    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1), mode='constant', value=0))


class LdmEncoder(nn.Module):
    """first_stage_model.{encoder, quant_conv}: forward(x in [-1, 1], NCHW) -> moments [n, 8, h / 8, w / 8]"""

    def __init__(self, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4):
        super().__init__()
        from oracle import sd_torch as S
        self.encoder = nn.Module()
        e = self.encoder
        e.conv_in = nn.Conv2d(3, ch, 3, padding=1)
        block_in = ch
        downs = []
        for i_level, m in enumerate(ch_mult):
            d = nn.Module()
            d.block = nn.ModuleList()
            block_out = ch * m
            for _ in range(num_res_blocks):
                d.block.append(S.VaeResnetBlock(block_in, block_out))
                block_in = block_out
            if i_level != len(ch_mult) - 1:
                d.downsample = LdmDownsample(block_in)
            downs.append(d)
        e.down = nn.ModuleList(downs)
        e.mid = nn.Module()
        e.mid.block_1 = S.VaeResnetBlock(block_in, block_in)
        e.mid.attn_1 = S.VaeAttnBlock(block_in)
        e.mid.block_2 = S.VaeResnetBlock(block_in, block_in)
        e.norm_out = S._norm(block_in)
        e.conv_out = nn.Conv2d(block_in, 2 * z_channels, 3, padding=1)
        self.quant_conv = nn.Conv2d(2 * z_channels, 2 * z_channels, 1)
        self.n_levels = len(ch_mult)

    def forward(self, x):
        e = self.encoder
        h = e.conv_in(x)
        for i, d in enumerate(e.down):
            for blk in d.block:
                h = blk(h)
            if i != self.n_levels - 1:
                h = d.downsample(h)
        h = e.mid.block_2(e.mid.attn_1(e.mid.block_1(h)))
        h = e.conv_out(F.silu(e.norm_out(h)))
        return self.quant_conv(h)


def ldm_img2img_indices(strength, steps):
    """ldm scripts/img2img.py + DDIMSampler (ddim_discretize 'uniform', eta 0), restated: (t_enc, the index / timestep sequence
    of DDIMSampler.decode, sqrt(alphas[t_enc]), sqrt(1 - alphas[t_enc]))"""
    betas = torch.linspace(0.00085 ** 0.5, 0.0120 ** 0.5, 1000, dtype=torch.float64) ** 2
    alphas_cumprod = torch.tensor(np.cumprod((1.0 - betas).numpy(), axis=0), dtype=torch.float32)
    c = 1000 // steps
    ddim_timesteps = np.asarray(list(range(0, 1000, c))) + 1
    ddim_alphas = alphas_cumprod[ddim_timesteps]
    t_enc = int(strength * steps)
    timesteps = ddim_timesteps[:t_enc]
    seq = [(int(step), t_enc - i - 1) for i, step in enumerate(np.flip(timesteps))]
    return t_enc, seq, float(torch.sqrt(ddim_alphas)[t_enc]), float(np.sqrt(1. - ddim_alphas)[t_enc])


def test_ldm_encoder_oracle_size():
    with torch.device('meta'):
        m = LdmEncoder()
    assert sum(p.numel() for p in m.encoder.parameters()) == 34_163_592
    assert sum(p.numel() for p in m.quant_conv.parameters()) == 72


def test_vae_encoder_split_is_opt_in_and_complete():
    """the opt-in table consumes every first_stage_model.encoder.* / quant_conv.* key of an ldm checkpoint (34,163,664
    values, shapes equal); the default tables and split are those of the txt2img graphs only"""
    from oracle import sd_torch as S
    from sdod.amd import convert
    with torch.device('meta'):
        enc, vae = LdmEncoder(), S.AutoencoderKLDecode()
    sd = {'first_stage_model.' + k: v for k, v in enc.state_dict().items()}
    sd.update({'first_stage_model.' + k: v for k, v in vae.state_dict().items()})
    table = convert.vae_encoder_table()
    names = {n for n, _ in table}
    assert names == set(enc.state_dict())
    assert sum(int(np.prod(s)) for _, s in table) == 34_163_664
    parts, unused = convert.split_state_dict(sd, {'vae_enc': table})
    assert len(parts['vae_enc']) == len(table)
    assert not [k for k in unused if k.startswith(('first_stage_model.encoder.', 'first_stage_model.quant_conv.'))]
    assert convert.OPTIONAL_GRAPHS['vae_enc'] == ('first_stage_model.', 'vae_encoder')
    # default: no encoder graph, and its keys are left over as before
    assert 'vae_enc' not in convert.GRAPHS
    tables = convert.parameter_tables()
    assert set(tables) == {'unet', 'temb', 'vae', 'text'}
    parts2, unused2 = convert.split_state_dict(sd, {'vae': tables['vae']})
    assert set(parts2) == {'vae'}
    assert 'first_stage_model.encoder.conv_in.weight' in unused2 and 'first_stage_model.quant_conv.bias' in unused2


def test_convert_cli_writes_the_encoder_only_when_asked(tmp_path, monkeypatch):
    from sdod.amd import convert, weights as Wt
    tables = {'unet': [('out.2.bias', (4,))], 'temb': [('time_embed.0.weight', (8, 4))],
              'vae': [('post_quant_conv.weight', (4, 4, 1, 1))], 'text': [('text_model.final_layer_norm.weight', (16,))]}
    monkeypatch.setattr(convert, 'parameter_tables', lambda cfg=None: tables)
    monkeypatch.setattr(convert, 'vae_encoder_table', lambda cfg=None: [('quant_conv.weight', (8, 8, 1, 1)), ('quant_conv.bias', (8,))])
    g = torch.Generator().manual_seed(3)
    sd = {convert.GRAPHS[gr][0] + n: torch.randn(s, generator=g) for gr, t in tables.items() for n, s in t}
    sd['first_stage_model.quant_conv.weight'] = torch.randn(8, 8, 1, 1, generator=g)
    sd['first_stage_model.quant_conv.bias'] = torch.randn(8, generator=g)
    src = str(tmp_path / 'model.ckpt')
    torch.save(sd, src)
    plain = tmp_path / 'plain'
    convert.main(['--ckpt', src, '--out', str(plain)])
    assert sorted(p.name for p in plain.iterdir()) == ['temb.sdodw', 'text_encoder.sdodw', 'unet.sdodw', 'vae_decoder.sdodw']
    withenc = tmp_path / 'enc'
    convert.main(['--ckpt', src, '--out', str(withenc), '--vae-encoder'])
    assert (withenc / 'vae_encoder.sdodw').exists()
    back = Wt.load(str(withenc / 'vae_encoder.sdodw'))
    assert torch.equal(back['quant_conv.bias'].float(), sd['first_stage_model.quant_conv.bias'].half().float())


@pytest.mark.parametrize('steps', [20, 50])
@pytest.mark.parametrize('strength', [0.05, 0.3, 0.5, 0.75, 0.99])
def test_img2img_schedule_matches_ldm(strength, steps):
    from sdod.amd.pipeline import img2img_schedule
    t_enc, seq, sa, s1a = ldm_img2img_indices(strength, steps)
    if not 1 <= t_enc <= steps - 1:
        with pytest.raises(ValueError):
            img2img_schedule(strength, steps)
        return
    sch, te = img2img_schedule(strength, steps)
    assert te == t_enc
    ours = [(int(sch.timesteps[t_enc - i - 1]), t_enc - i - 1) for i in range(t_enc)]
    assert ours == seq
    assert np.float32(sch.sqrt_alphas[t_enc]) == np.float32(sa)
    assert np.float32(sch.sqrt_one_minus_alphas[t_enc]) == np.float32(s1a)


@pytest.mark.parametrize('strength,steps', [(0.0, 50), (1.0, 50), (0.01, 50), (0.04, 20), (-0.1, 50), (1.5, 50), (0.5, 1)])
def test_img2img_strength_outside_domain_raises(strength, steps):
    from sdod.amd.pipeline import img2img_schedule
    with pytest.raises(ValueError):
        img2img_schedule(strength, steps)


def test_gemm_desc_mirror_has_pad_mode_at_the_c_offset():
    """the ctypes mirror ends with pad_mode, at the offset the C compiler gives the field (sizeof / offsetof from a C build)"""
    import os
    import subprocess
    from sdod.amd._lib import GemmDesc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert GemmDesc._fields_[-1] == ('pad_mode', ctypes.c_int)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sdod_hip.h"\n'
           'int main(void){printf("%zu %zu\\n", offsetof(sdod_gemm_desc, pad_mode), sizeof(sdod_gemm_desc));return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'o.c')
        with open(c, 'w') as f:
            f.write(src)
        exe = os.path.join(d, 'o')
        subprocess.check_call(['cc', '-I', os.path.join(root, 'include'), c, '-o', exe])
        off, size = map(int, subprocess.check_output([exe]).split())
    assert GemmDesc.pad_mode.offset == off
    assert ctypes.sizeof(GemmDesc) == size
