"""The VAE graphs' fused middle attention (sdod_graph_create_vae / fused_attn): against the four-launch form and the
fp32 torch oracle at a 16 x 24 latent (batch 2, vae_channels 128 and 64), the op tables of both forms, and the latent size that
did not build before -- 128 x 136, 17408 positions -- through the old create path.  Bound everywhere: rel-L2 <= 1e-2, what
test_full_size_gpu._vae_case asks of the decoder against the oracle."""
import functools
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-2


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _decode(g, sd, z):
    g.load_state_dict(sd)
    g.finalize()
    g.z.copy_(z)
    g.execute()
    torch.cuda.synchronize()
    g.check()
    eager = g.img.clone()
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.img), 'hipGraph replay differs from eager execution'
    return eager.float().cpu().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def decoder_case(ch):
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 24)
    cfg.vae_channels = ch
    graphs = {'fused': E.VaeDecoder(cfg, 2, fused_attn=True), 'four': E.VaeDecoder(cfg, 2, fused_attn=False),
              'create_vae_0': E.Graph(E.VAE_DECODER, cfg, 2, fused_attn=False)}
    sd = Wt.synthetic_state_dict(graphs['four'].param_table(), seed=1235 + ch)
    assert graphs['fused'].param_table() == graphs['four'].param_table()
    z = torch.randn(2, 4, 16, 24, generator=torch.Generator().manual_seed(12)) * 0.18215 * 4
    with torch.device('meta'):
        ref_model = S.AutoencoderKLDecode(ch=ch)
    ref_model.load_state_dict(sd, assign=True)
    with torch.no_grad():
        ref = ref_model.eval()(z)
    graphs['create_vae_0'].load_state_dict(sd)
    graphs['create_vae_0'].finalize()
    return {'fused': _decode(graphs['fused'], sd, z), 'four': _decode(graphs['four'], sd, z), 'ref': ref,
            'tables': {k: g.op_table() for k, g in graphs.items()}}


@pytest.mark.parametrize('ch', [128, 64])
def test_decoder_fused_vs_four_launch_and_oracle(ch):
    c = decoder_case(ch)
    r_pair, r_ref = rel_l2(c['fused'], c['four']), rel_l2(c['fused'], c['ref'])
    print(f'vae decoder ch{ch} 16x24 b2: fused vs four-launch rel-L2 {r_pair:.3e}, fused vs oracle {r_ref:.3e}')
    assert torch.isfinite(c['fused']).all() and r_pair <= TOL and r_ref <= TOL, (r_pair, r_ref)


@pytest.mark.parametrize('ch', [128, 64])
def test_op_tables(ch):
    t = decoder_case(ch)['tables']
    labels = [lab for lab, _, _ in t['fused']]
    assert labels.count('attention_wide') == 1 and 'softmax_rows' not in labels
    fl, by = next((f, b) for lab, f, b in t['fused'] if lab == 'attention_wide')
    assert fl == 4.0 * 2 * 384 * 384 * 4 * ch and by >= 4 * 2 * 384 * 4 * ch * 2
    assert [lab for lab, _, _ in t['four']].count('softmax_rows') == 2
    assert t['create_vae_0'] == t['four']                # fused_attn = 0 is the graph sdod_graph_create builds


def test_encoder_fused_vs_four_launch_and_oracle():
    from test_img2img_cpu import LdmEncoder
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 24)
    gen = torch.Generator().manual_seed(8)
    u8 = torch.randint(0, 256, (2, 128, 192, 3), generator=gen, dtype=torch.uint8)
    sd = Wt.synthetic_state_dict(E.VaeEncoder(cfg, 2).param_table(), seed=1238)
    out = {}
    for fused in (True, False):
        g = E.VaeEncoder(cfg, 2, fused_attn=fused)
        g.load_state_dict(sd)
        g.finalize()
        g.img.copy_(u8)
        g.execute()
        torch.cuda.synchronize()
        g.check()
        out[fused] = g.moments.cpu().clone()
        assert ('attention_wide' in [lab for lab, _, _ in g.op_table()]) == fused
    with torch.device('meta'):
        ref_model = LdmEncoder(ch=128)
    ref_model.load_state_dict(sd, assign=True)
    with torch.no_grad():
        ref = ref_model.eval()((2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2))
    r_pair, r_ref = rel_l2(out[True], out[False]), rel_l2(out[True], ref)
    print(f'vae encoder 16x24 b2: fused vs four-launch rel-L2 {r_pair:.3e}, fused vs oracle {r_ref:.3e}')
    assert torch.isfinite(out[True]).all() and r_pair <= TOL and r_ref <= TOL, (r_pair, r_ref)


def test_latent_128x136_builds_and_matches_oracle():
    """17408 positions, vae_channels 64, through the create path that refused it: above 16384 the block is the fused one"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(128, 136)
    cfg.vae_channels = 64
    g = E.VaeDecoder(cfg, 1)
    sd = Wt.synthetic_state_dict(g.param_table(), seed=1299)
    z = torch.randn(1, 4, 128, 136, generator=torch.Generator().manual_seed(13)) * 0.18215 * 4
    out = _decode(g, sd, z)
    assert 'attention_wide' in [lab for lab, _, _ in g.op_table()]
    with torch.device('meta'):
        ref_model = S.AutoencoderKLDecode(ch=64)
    ref_model.load_state_dict(sd, assign=True)
    t0 = time.time()
    with torch.no_grad():
        ref = ref_model.eval()(z)
    r = rel_l2(out, ref)
    print(f'vae decoder ch64 128x136 (L = 17408): rel-L2 vs oracle {r:.3e}, oracle {time.time() - t0:.1f} s on the CPU')
    assert out.shape == (1, 3, 1024, 1088) and torch.isfinite(out).all() and r <= TOL, r


def test_pipeline_argument():
    from sdod.amd.pipeline import Txt2Img
    with pytest.raises(ValueError, match='vae_attention'):
        Txt2Img(vae_attention='nonsense')
