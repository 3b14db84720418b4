"""Reference-only control through the engine: E.UNet(cfg, 4, reference=2), rows [uncond, cond, ref_u, ref_c].

A model_channels-64 graph (test_engine_widths_gpu.py's smallest width, weights and bound UNET_TOL: the same comparison, graph against
fp32 oracle) at 16 x 16 against the oracle with the shared keys wrapped around its attn1 modules (reference_ref.py); the weights are
written into the input of a graph CAPTURED at the identity, whose replays must follow them.  self_w = (1, 1) has the plain graphs' bits.
Txt2Img(reference=True) at 16 x 16: clear_reference() gives the plain pipeline's image; a captured trajectory equals the eager one with a
reference set, and still does after a second set_reference, which it follows without a recapture."""
import pytest
import torch

import reference_ref as RR
from test_engine_widths_gpu import UNET_TOL, Width, labels_of, rel_l2, static_plan  # noqa: F401  (autouse: the static tile plan)

pytestmark = pytest.mark.gpu

HW = (16, 16)


@pytest.fixture(scope='module')
def w64():
    return Width(64, 128, seed=6400)


@pytest.fixture(scope='module')
def inputs():
    gen = torch.Generator().manual_seed(411)
    return torch.randn(4, 4, *HW, generator=gen), torch.randn(4, 77, 128, generator=gen).half(), torch.full((4,), 999.0)


def build_graphs(w64, batch, **kw):
    from sdod.amd import engine as E
    cfg = E.sd14_config(*HW)
    cfg.model_channels, cfg.num_heads, cfg.head_dim, cfg.context_dim = 64, 0, 64, 128
    g, tg = E.UNet(cfg, batch, **kw), E.Temb(cfg, batch)
    for graph in (g, tg):
        graph.load_state_dict(w64.load)
        graph.finalize()
    return g, tg


def run(g, tg, inputs, **kw):
    x, ctx, t = (v[:g.batch] for v in inputs)
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    g.execute(**kw)
    torch.cuda.synchronize()
    g.check()
    return g.eps.clone()


def test_reference_graph_matches_the_wrapped_oracle(w64, inputs):
    from oracle import sd_torch as S
    g, tg = build_graphs(w64, 4, reference=2)
    assert labels_of(g).count('attn_shared_d64') == 16                   # every transformer block's attn1
    with torch.device('meta'):
        unet = S.UNetModel(model_ch=64, head_dim=64, context_dim=128)
    unet.load_state_dict(w64.sd, assign=True)
    x, ctx, t = inputs
    self_w = [1.0, 1.0]
    with torch.no_grad():
        plain = unet.eval()(x, t, ctx.float())
        RR.wrap_oracle(unet, 2, self_w)
    run(g, tg, inputs, use_hip_graph=True)                               # captured at the identity
    for ws in ((0.5, 0.0), (0.0, 0.0)):
        self_w[:] = ws
        g.reference_self_w.copy_(torch.tensor(ws))
        with torch.no_grad():
            ref = unet(x, t, ctx.float())
        eager = run(g, tg, inputs)
        out = eager.float().cpu().permute(0, 3, 1, 2)
        r, r_img, away = rel_l2(out, ref), [rel_l2(out[i], ref[i]) for i in range(4)], rel_l2(ref[:2], plain[:2])
        assert torch.isfinite(out).all() and r <= UNET_TOL and max(r_img) <= UNET_TOL, (r, r_img)
        assert away > 10 * UNET_TOL, 'the wrapped oracle must differ from the plain one for the comparison to mean anything'
        for _ in range(2):
            assert torch.equal(run(g, tg, inputs, use_hip_graph=True), eager), 'hipGraph replay differs from eager execution'


def test_self_weight_one_is_the_graph_without_the_switch(w64, inputs):
    g, tg = build_graphs(w64, 4, reference=2)
    assert g.reference_self_w.tolist() == [1.0, 1.0]
    out = run(g, tg, inputs)
    assert torch.equal(out, run(*build_graphs(w64, 4), inputs)), 'differs from the batch-4 graph without the switch'
    assert torch.equal(out[:2], run(*build_graphs(w64, 2), inputs)), 'the first two rows differ from the plain pair graph'


def test_switch_refusals(w64):
    from sdod.amd import engine as E
    cfg = E.sd14_config(*HW)
    for msg, make in (('anchors must be 1 or 2', lambda: E.UNet(cfg, 4, reference=3)),
                      ('multiple of anchors', lambda: E.UNet(cfg, 5, reference=2)),
                      ('multiple of anchors', lambda: E.UNet(cfg, 2, reference=2)),
                      ('excludes', lambda: E.UNet(cfg, 4, sag=True, reference=2)),
                      ('excludes', lambda: E.UNet(cfg, 4, reference=2).enable_hypertile(8, 0)),
                      ('UNET graph only', lambda: E.VaeDecoder(cfg, 1).enable_reference(1)),
                      ('before finalize', lambda: build_graphs(w64, 4)[0].enable_reference(2))):
        with pytest.raises(Exception, match=msg):
            make()


def test_pipeline_reference():
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(*HW)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table(),
              'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    kw = dict(state_dicts={k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}, images_per_gpu=1,
              latent_hw=16, with_text_encoder=False, with_vae_encoder=True)
    pipe, plain = Txt2Img(reference=True, **kw), Txt2Img(**kw)
    gen = torch.Generator().manual_seed(78)
    c = (torch.randn(2, 77, 768, generator=gen) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, 16, 16, generator=gen)
    pics = torch.randint(0, 256, (2, 128, 128, 3), generator=gen, dtype=torch.uint8)
    args = (c, x_T, 4, 7.5, 'euler_a')
    base = plain.generate(*args).clone()
    pipe.set_reference(pics[0], 0.5, seed=5)
    with pytest.raises(ValueError, match='clear_reference'):
        pipe.generate(c, x_T, 4, 7.5, 'plms')
    first = pipe.generate(*args).clone()
    assert not torch.equal(first, base), 'the reference changed nothing'
    assert torch.equal(pipe.generate_graphed(*args), first), 'captured differs from eager'
    captured = len(pipe._traj)
    pipe.set_reference(pics[1], 0.25, noise=torch.randn(4, 16, 16, generator=gen))
    second = pipe.generate(*args).clone()
    assert not torch.equal(second, first)
    assert torch.equal(pipe.generate_graphed(*args), second) and len(pipe._traj) == captured, 'the captured trajectory did not follow'
    pipe.clear_reference()
    assert torch.equal(pipe.generate(*args), base) and torch.equal(pipe.generate_graphed(*args), base), 'differs from the plain pipeline'
