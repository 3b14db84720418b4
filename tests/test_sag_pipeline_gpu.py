"""Txt2Img(sag=True) (Self-Attention Guidance) on synthetic SD v1.4 weights: latent 16 x 16 with one image and 16 x 24
with two (so the uncond rows are a real slice of the pair), plms / euler_a / dpmpp_2m.

(1) After clear_sag() -- and as built -- the latents are the plain pipeline's, bit for bit.
(2) With set_sag(0.75) they differ, and generate_graphed equals generate bit for bit, on a capture of its own.
(3) One _unet_eps() equals the four steps composed by hand from ops and the two graphs, bit for bit.
(4) The entry points the pass is not wired into raise ValueError naming it, as does a guidance scale of 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, G = 4, 7.5


@pytest.fixture(scope='module')
def weights():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    return {'unet': Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234),
            'temb': Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235),
            'vae': Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1236)}


@pytest.fixture(scope='module', params=[(1, 16, 16), (2, 16, 24)], ids=lambda p: f'n{p[0]}-{p[1]}x{p[2]}')
def rig(weights, request):
    from sdod.amd.pipeline import Txt2Img
    n, h, w = request.param
    kw = dict(state_dicts=weights, images_per_gpu=n, latent_hw=(h, w), with_text_encoder=False)
    g = torch.Generator().manual_seed(131 + w)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    return dict(pipe=Txt2Img(sag=True, **kw), plain=Txt2Img(**kw), ctx2=ctx2, x_T=torch.randn(n, 4, h, w, generator=g), n=n)


@pytest.mark.parametrize('sampler', ['plms', 'euler_a', 'dpmpp_2m'])
def test_cleared_is_plain_and_captured_is_eager(rig, sampler):
    pipe, plain, c, x_T = rig['pipe'], rig['plain'], rig['ctx2'], rig['x_T']
    assert pipe.sag_unet.batch == rig['n'] and pipe.unet.batch == 2 * rig['n'] and plain.sag_unet is None and not hasattr(plain.unet, 'sag_mass')
    z_plain = plain._sample(sampler, c, x_T, STEPS, G)
    assert torch.equal(pipe._sample(sampler, c, x_T, STEPS, G), z_plain)                    # as built: off
    pipe.set_sag(0.75)
    z = pipe._sample(sampler, c, x_T, STEPS, G)
    assert torch.isfinite(z).all() and not torch.equal(z, z_plain)
    eager = pipe.generate(c, x_T, STEPS, G, sampler)
    assert torch.equal(pipe.generate_graphed(c, x_T, STEPS, G, sampler), eager)
    assert torch.equal(pipe.generate_graphed(c, x_T, STEPS, G, sampler), eager)             # a replay
    n_graphs = len(pipe._traj)
    pipe.clear_sag()
    assert torch.equal(pipe._sample(sampler, c, x_T, STEPS, G), z_plain)
    base = plain.generate(c, x_T, STEPS, G, sampler)
    assert torch.equal(pipe.generate_graphed(c, x_T, STEPS, G, sampler), base) and len(pipe._traj) == n_graphs + 1     # keyed by the scale
    assert not torch.equal(base, eager)


@pytest.mark.parametrize('abs_', [(0.6, 0.8, 1.0), (1.0, 2.5, 0.37)], ids=['ddim', 'k'])
def test_unet_eps_is_the_four_steps(rig, abs_):
    from sdod.amd import ops
    pipe, n = rig['pipe'], rig['n']
    a, b, ss = abs_
    temb = pipe.time_embeddings([481.0])
    pipe._set_context(rig['ctx2'])
    ops.stage_unet_inputs(rig['x_T'].cuda() * ss, pipe.unet.x, temb[0], pipe._temb_dst)
    pipe.set_sag(0.75)
    try:
        pipe._sag_stage(a, b, ss, G)
        got = pipe._unet_eps().clone()
        with pytest.raises(ValueError, match='Self-Attention Guidance'):                    # an evaluation no sampler prepared
            pipe._unet_eps()
    finally:
        pipe.clear_sag()
    unet, su = pipe.unet, pipe.sag_unet
    unet.execute()
    pair = unet.eps.clone()
    assert (unet.sag_mass > 1).any() and (unet.sag_mass < 1).any()                          # both sides of the mask are exercised
    ops.sag_degrade(unet.x[:n], unet.eps[:n], unet.sag_mass[:n], a, b, ss, out=su.x)
    su.temb.copy_(unet.temb[:n])
    su.execute()
    ops.sag_fold(unet.eps, su.eps, 0.75, G)
    assert torch.equal(got, unet.eps) and torch.equal(got[:n], pair[:n]) and not torch.equal(got[n:], pair[n:])


def test_other_entry_points_refuse_while_on(rig):
    pipe, c, x_T = rig['pipe'], rig['ctx2'], rig['x_T']
    pipe.set_sag()
    try:
        for call in (lambda: pipe.sample_dpm(c, x_T, STEPS, G), lambda: pipe.generate(c, x_T, STEPS, G, 'dpm'),
                     lambda: pipe.sample_ddim_from(c, x_T, 2, STEPS, G), lambda: pipe.sample_lcm(c, x_T, STEPS, 1.5),
                     lambda: pipe.sample_k(c, x_T, 'euler', STEPS, 0.0)):
            with pytest.raises(ValueError, match='Self-Attention Guidance'):
                call()
    finally:
        pipe.clear_sag()
