"""HyperTile through the engine and the pipeline.

(1) A model_channels-64 UNet graph (the smallest width of test_engine_widths_gpu.py, its weights and its bound) at a 16 x 24 latent with
    (tile, max_depth) = (8, 0) and (8, 1), against the oracle UNet with the rearrangement wrapped around its attn1 modules
    (hypertile_ref.py).  The bound is UNET_TOL = 1e-2 of test_engine_widths_gpu.py: the same comparison -- graph against fp32 oracle --
    of which the tiled graph changes only the softmax domains.
(2) The same graph with tile = 64 tiles no level: launch labels and output bits of the graph without the switch; and the switch is
    refused after finalize.
(3) Txt2Img(hypertile=8) at a 16 x 16 latent: generate_graphed equals generate byte for byte, both differ from the pipeline without
    the switch, bad values raise ValueError."""
import pytest
import torch

import hypertile_ref as HR
from test_engine_widths_gpu import UNET_TOL, Width, labels_of, rel_l2

pytestmark = pytest.mark.gpu

HW = (16, 24)


@pytest.fixture(autouse=True)
def static_plan(monkeypatch):
    monkeypatch.setenv('SDOD_AUTOTUNE', '0')


@pytest.fixture(scope='module')
def w64():
    return Width(64, 128, seed=6400)


@pytest.fixture(scope='module')
def inputs():
    gen = torch.Generator().manual_seed(311)
    return torch.randn(2, 4, *HW, generator=gen), torch.randn(2, 77, 128, generator=gen).half(), torch.tensor([999.0, 251.0])


def build_graphs(w64, hypertile):
    from sdod.amd import engine as E
    cfg = E.sd14_config(*HW)
    cfg.model_channels, cfg.num_heads, cfg.head_dim, cfg.context_dim = 64, 0, 64, 128
    cfg.hypertile = hypertile
    g, tg = E.UNet(cfg, 2), E.Temb(cfg, 2)
    for graph in (g, tg):
        graph.load_state_dict(w64.load)
        graph.finalize()
    return g, tg


def run(g, tg, inputs):
    x, ctx, t = inputs
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    g.execute()
    torch.cuda.synchronize()
    g.check()
    return g.eps.clone()


@pytest.mark.parametrize('tile,max_depth,tiled', [(8, 0, 5), (8, 1, 10)])
def test_tiled_graph_matches_the_wrapped_oracle(w64, inputs, tile, max_depth, tiled):
    from oracle import sd_torch as S
    g, tg = build_graphs(w64, (tile, max_depth))
    assert labels_of(g).count('attn_tiled_d64') == tiled                 # five transformer blocks per level: 2 down, 3 up
    eager = run(g, tg, inputs)
    with torch.device('meta'):
        unet = S.UNetModel(model_ch=64, head_dim=64, context_dim=128)
    unet.load_state_dict(w64.sd, assign=True)
    x, ctx, t = inputs
    with torch.no_grad():
        plain = unet.eval()(x, t, ctx.float())
        ref = HR.wrap_oracle(unet, HW, tile, max_depth)(x, t, ctx.float())
    out = eager.float().cpu().permute(0, 3, 1, 2)
    r, r_img, away = rel_l2(out, ref), [rel_l2(out[i], ref[i]) for i in range(2)], rel_l2(ref, plain)
    print(f'hypertile w64 {HW} tile {tile} depth {max_depth}: rel-L2 {r:.3e}, per image {r_img[0]:.3e} {r_img[1]:.3e}, oracle moved by {away:.3e}')
    assert torch.isfinite(out).all() and r <= UNET_TOL and max(r_img) <= UNET_TOL, (r, r_img)
    assert away > 10 * UNET_TOL or away > r, 'the wrapped oracle must differ from the plain one for the comparison to mean anything'
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.eps), 'hipGraph replay differs from eager execution'


def test_a_rule_that_tiles_nothing_changes_nothing(w64, inputs):
    plain, tg = build_graphs(w64, None)
    same, _ = build_graphs(w64, (64, 3))
    assert labels_of(same) == labels_of(plain) and not any(lab.startswith('attn_tiled') for lab in labels_of(plain))
    assert same.stats() == plain.stats()
    assert torch.equal(run(same, tg, inputs), run(plain, tg, inputs))
    with pytest.raises(Exception, match='before finalize'):
        plain.enable_hypertile(8, 0)


def test_pipeline_takes_the_switch():
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(16, 16)
    weights = {'unet': Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234),
               'temb': Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235),
               'vae': Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1236)}
    kw = dict(state_dicts=weights, images_per_gpu=1, latent_hw=16, with_text_encoder=False)
    for bad in (4, (8, 5), 'on', 8.5):
        with pytest.raises(ValueError, match='hypertile'):
            Txt2Img(hypertile=bad, **kw)
    pipe, plain = Txt2Img(hypertile=8, **kw), Txt2Img(**kw)
    assert pipe.hypertile == (8, 0) and plain.hypertile is None
    assert labels_of(pipe.unet).count('attn_tiled_d40') == 5 and labels_of(plain.unet).count('attn_tiled_d40') == 0
    gen = torch.Generator().manual_seed(77)
    c = (torch.randn(2, 77, 768, generator=gen) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, 16, 16, generator=gen)
    eager = pipe.generate(c, x_T, 4, 7.5, 'plms').clone()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, 'plms'), eager)
    assert not torch.equal(plain.generate(c, x_T, 4, 7.5, 'plms'), eager)
