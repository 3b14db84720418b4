"""sdod_graph_enable_sag (Self-Attention Guidance) on the smallest UNet width the config contract accepts (mc 64, head
dim 64, 16 x 24 and 32 x 32 latents: middle maps of 6 and 16 tokens, 4 heads).

(1) The graph with the switch has the bits of the graph without it in out0, one more launch (attn_mass_d64) and one more output.
(2) Its mass output against the fp32 oracle's (oracle/sd_torch.py) middle_block.1 attn1 probabilities, averaged over heads and summed
    over queries, from a pre-hook on that module's input.  The engine's fp16 path moves the scores themselves, so the bound is the one
    tests/test_engine_widths_gpu.py holds this width's UNet output to against the same oracle: rel-L2 <= UNET_TOL = 1e-2.
(3) enable_sag on another kind, or after finalize, is refused."""
import pytest
import torch

from test_engine_widths_gpu import UNET_TOL, Width, rel_l2, static_plan, width_config  # noqa: F401  (static_plan: autouse fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def w64():
    return Width(64, 128, seed=6400)


@pytest.mark.parametrize('hw', [(16, 24), (32, 32)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_mass_output_and_unchanged_eps(w64, hw):
    from sdod.amd import engine as E
    cfg = width_config(64, 64, 128, hw[0])
    cfg.latent_w = hw[1]
    plain, sag = E.UNet(cfg, 2), E.UNet(cfg, 2, sag=True)
    tg = E.Temb(cfg, 2)
    for g in (plain, sag, tg):
        g.load_state_dict(w64.load)
        g.finalize()
    gen = torch.Generator().manual_seed(113)
    x, ctx, t = torch.randn(2, 4, *hw, generator=gen), torch.randn(2, 77, 128, generator=gen).half(), torch.tensor([999.0, 251.0])
    tg.t.copy_(t); tg.execute()
    for g in (plain, sag):
        g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
        g.execute()
    torch.cuda.synchronize()
    assert torch.equal(plain.eps, sag.eps)
    labels = lambda g: [lab for lab, _, _ in g.op_table()]
    assert [lab for lab in labels(sag) if lab != 'attn_mass_d64'] == labels(plain) and labels(sag).count('attn_mass_d64') == 1
    assert plain.sag_output() == -1 and not hasattr(plain, 'sag_mass') and sag.sag_output() == 1
    eager = sag.sag_mass.clone()
    sag.execute(use_hip_graph=True); sag.execute(use_hip_graph=True, static_unchanged=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, sag.sag_mass) and torch.equal(plain.eps, sag.eps)

    unet, seen = w64.oracle(64), []
    attn1 = unet.middle_block[1].transformer_blocks[0].attn1
    hook = attn1.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    with torch.no_grad():
        unet(x, t, ctx.float())
        hook.remove()
        q, k = (f(seen[0]).reshape(2, -1, attn1.heads, 64).transpose(1, 2) for f in (attn1.to_q, attn1.to_k))
        ref = torch.softmax(q @ k.transpose(-1, -2) * attn1.scale, dim=-1).sum(2).mean(1)
    r = rel_l2(eager.cpu(), ref)
    print(f'sag engine w64 {hw}: mass rel-L2 {r:.3e}, mass range {float(ref.min()):.3f} .. {float(ref.max()):.3f}')
    assert tuple(eager.shape) == tuple(ref.shape) == (2, hw[0] * hw[1] // 64) and r <= UNET_TOL, r


def test_refusals(w64):
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    cfg = width_config(64, 64, 128, 16)
    with pytest.raises(SdodError):
        E.Temb(cfg, 2).enable_sag()
    g = E.UNet(cfg, 2)
    g.load_state_dict(w64.load)
    g.finalize()
    with pytest.raises(SdodError):
        g.enable_sag()
