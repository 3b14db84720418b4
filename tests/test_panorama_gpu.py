"""MultiDiffusion panoramas through the pipeline on the GPU: Txt2Img(canvas_hw=...) with synthetic weights (the `sds` recipe of
test_tiling_gpu.py), the UNet at 16 x 16 windows.

Oracle parity of a short trajectory: the reference is oracle.sd_torch.UNetModel in fp32 on the window crops, one batch per step,
followed by the float64 restatement of the canvas step (tests/panorama_ref.py).  Bound: final canvas latent rel-L2 <= 2e-2, the bound
test_tiling_gpu.py states for its 20-step sampler chain on these graphs; this chain has 2 steps.  Chunked runs (n = 1: two chunks;
three windows at n = 2: a partly filled chunk) and the wrapped canvas are held to the same reference at the same bound.  Bit-exact:
the graphed entry against the eager one, and a canvas equal to the window against sample_k."""
import pytest
import torch

import panorama_ref as R

pytestmark = pytest.mark.gpu

WIN = (16, 16)
TOL = 2e-2
STEPS, GUIDANCE = 2, 7.5


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def sds():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(*WIN)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    return {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}


@pytest.fixture(scope='module')
def oracle_unet(sds):
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    return unet.eval()


@pytest.fixture(scope='module')
def pipes(sds):
    """(canvas, n, wrap) -> Txt2Img, built once"""
    from sdod.amd.pipeline import Txt2Img
    made = {}

    def get(canvas, n, wrap=False, with_vae=True):
        key = (canvas, n, wrap)
        if key not in made:
            made[key] = Txt2Img(state_dicts=sds, images_per_gpu=n, latent_hw=WIN, with_text_encoder=False, with_vae=with_vae, canvas_hw=canvas,
                                canvas_wrap=wrap)
        return made[key]
    return get


@pytest.fixture(scope='module')
def inputs():
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    return ctx2, {c: torch.randn(1, 4, *c, generator=g) for c in ((16, 24), (16, 40), (16, 32), (16, 16))}


_refs = {}


@torch.no_grad()
def reference(unet, ctx2, x_T, sampler, stride, wrap):
    """the fp32 oracle UNet on the window crops of c_in * x as one batch per step, then the float64 restatement of the canvas step; the
    schedule's scalars are the host's (sdod.amd.samplers.KSchedule, held to k-diffusion's by test_ksamplers_*.py)"""
    from oracle import pipeline_oracle as PO
    from sdod.amd import panorama as PN
    from sdod.amd.samplers import KSchedule
    canvas = tuple(x_T.shape[-2:])
    key = (canvas, sampler, stride, wrap)
    if key in _refs:
        return _refs[key]
    oy, ox = PN.plan_windows(canvas, WIN, stride, wrap)
    n_win = len(oy) * len(ox)
    wgt = PN.window_weights(WIN, 'uniform')
    wsum = torch.from_numpy(PN.weight_sum(canvas, WIN, oy, ox, wgt, wrap))
    wgt = torch.from_numpy(wgt)
    sch = KSchedule(STEPS, 'karras')
    c16 = ctx2.float()
    geom = (wgt, wsum, oy, ox, WIN, wrap, n_win)
    x, _ = R.step(None, x_T, dict(a=float(sch.sigmas[0])), *geom, dtype=torch.float64)
    den_prev = None
    for i in range(STEPS):
        crops = R.crops(x * sch.c_in(i), oy, ox, WIN, wrap).float()
        t = torch.tensor(float(sch.times[i]), dtype=torch.float32).reshape(1).expand(n_win)
        e_u, e_c = PO.guided_eps(unet, crops, t, c16[0:1], c16[1:2], GUIDANCE)
        eps = torch.cat([e_u, e_c]).permute(0, 2, 3, 1)[None]                # [1, 2 n_win, wh, ww, c], as the kernel reads it
        x, den_prev = R.step(eps, x, sch.coef(sampler, i), *geom, guidance=GUIDANCE, mode=1, den_prev=den_prev, dtype=torch.float64)
    _refs[key] = x
    return x


@pytest.mark.parametrize('canvas,stride,n,wrap,what', [
    ((16, 24), 8, 2, False, 'two windows in one evaluation'),
    ((16, 24), 8, 1, False, 'two chunks'),
    ((16, 40), 16, 2, False, 'three windows: a partly filled last chunk'),
    ((16, 32), 8, 2, True, 'wrapped: four windows, one across the seam, two chunks'),
])
@pytest.mark.parametrize('sampler', ['euler', 'dpmpp_2m'])
def test_trajectory_matches_the_oracle(pipes, oracle_unet, inputs, sampler, canvas, stride, n, wrap, what):
    """Reached on MI355X (the test prints them): 3.7e-3 .. 5.2e-3.  Two steps of euler and of dpmpp_2m are the same
    arithmetic (the first step of DPM++ 2M is first order, b = -expm1(-h) = 1 - s'/s; the last step is x' = den), so the pairs agree."""
    ctx2, x_Ts = inputs
    pipe = pipes(canvas, n, wrap)
    z = pipe.sample_panorama(ctx2.cuda(), x_Ts[canvas], sampler, STEPS, GUIDANCE, schedule='karras', stride=stride)
    torch.cuda.synchronize()
    ref = reference(oracle_unet, ctx2, x_Ts[canvas], sampler, stride, wrap)
    r = rel_l2(z.cpu(), ref)
    print(f'panorama {canvas} stride {stride} n {n} wrap {wrap} {sampler} ({what}): final canvas latent rel-L2 {r:.3e}')
    assert z.shape == (1, 4) + canvas and z.dtype == torch.float32 and torch.isfinite(z).all()
    assert r <= TOL, r
    pipe.unet.check()


def test_graphed_equals_eager_bit_for_bit_with_drawn_noise(pipes, inputs):
    ctx2, x_Ts = inputs
    pipe = pipes((16, 24), 2)
    c, x_T = ctx2.cuda(), x_Ts[(16, 24)]
    images = []
    for seed in (3, 4):             # the second replay runs the cached graph with another seed: the graph bakes none
        kw = dict(sampler='euler_a', steps=3, guidance=GUIDANCE, schedule='karras', stride=8, weights='gaussian', seed=seed, image_index=1)
        eager = pipe.generate_panorama(c, x_T, **kw)
        graphed = pipe.generate_panorama_graphed(c, x_T, **kw)
        torch.cuda.synchronize()
        assert eager.shape == (1, 128, 192, 3) and eager.dtype == torch.uint8
        assert torch.equal(graphed, eager)
        images.append(eager.clone())
    assert not torch.equal(images[0], images[1])
    assert len(pipe._traj) == 1
    # injected step noise takes the same path
    sn = torch.randn(2, 1, 4, 16, 24, generator=torch.Generator().manual_seed(9))
    kw = dict(sampler='euler_a', steps=3, guidance=GUIDANCE, schedule='karras', stride=8, weights='gaussian', step_noise=sn)
    assert torch.equal(pipe.generate_panorama_graphed(c, x_T, **kw), pipe.generate_panorama(c, x_T, **kw))
    pipe.unet.check()


def test_graphed_equals_eager_with_chunks(pipes, inputs):
    ctx2, x_Ts = inputs
    pipe = pipes((16, 40), 2)
    c, x_T = ctx2.cuda(), x_Ts[(16, 40)]
    kw = dict(sampler='dpmpp_2m', steps=3, guidance=GUIDANCE, stride=16)
    eager = pipe.generate_panorama(c, x_T, **kw)
    assert eager.shape == (1, 128, 320, 3)
    assert torch.equal(pipe.generate_panorama_graphed(c, x_T, **kw), eager)
    assert torch.equal(pipe.generate_panorama_graphed(c, x_T, **kw), eager)


@pytest.mark.parametrize('sampler', ['euler', 'euler_a', 'dpmpp_2m'])
def test_a_canvas_equal_to_the_window_is_sample_k(pipes, inputs, sampler):
    ctx2, x_Ts = inputs
    pipe = pipes((16, 16), 1)
    c, x_T = ctx2.cuda(), x_Ts[(16, 16)]
    kw = dict(schedule='karras', eta=1.0, seed=11, image_index=2)
    z = pipe.sample_panorama(c, x_T, sampler, 3, GUIDANCE, **kw)
    want = pipe.sample_k(c, x_T, sampler, 3, GUIDANCE, **kw)
    torch.cuda.synchronize()
    assert torch.equal(z.view(torch.int32), want.view(torch.int32))
    assert torch.equal(pipe.decode_canvas(z), pipe.decode(want, mode=1))


def test_wrapped_canvas_decoder_has_the_circular_x_border(pipes, sds, inputs):
    from sdod.amd import engine as E
    pipe = pipes((16, 32), 2, True)
    assert pipe.canvas_wrap and pipe.canvas_hw == (16, 32)
    assert pipe.canvas_vae.cfg.tiling == 1 and pipe.unet.cfg.tiling == 0 and pipe.vae.cfg.tiling == 0 and pipe.tiling == 0
    assert (pipe.canvas_vae.cfg.latent_h, pipe.canvas_vae.cfg.latent_w) == (16, 32)
    made = {}
    for tiling in (1, 0):
        cfg = E.sd14_config(16, 32)
        cfg.tiling = tiling
        g = E.VaeDecoder(cfg, 1)
        g.load_state_dict(sds['vae'])
        g.finalize()
        made[tiling] = g
    assert pipe.canvas_vae.op_table() == made[1].op_table() and pipe.canvas_vae.op_details() == made[1].op_details()
    z = torch.randn(1, 4, 16, 32, generator=torch.Generator().manual_seed(12)).cuda() * 0.18215 * 4
    img = pipe.decode_canvas(z)
    outs = {}
    for tiling, g in made.items():
        g.z.copy_(z)
        g.execute()
        torch.cuda.synchronize()
        outs[tiling] = g.img.clone()
    assert img.shape == (1, 128, 256, 3) and img.dtype == torch.uint8
    assert torch.equal(pipe.canvas_vae.img, outs[1]) and not torch.equal(pipe.canvas_vae.img, outs[0])
    # and a pipeline without canvas_hw has none of it
    plain = pipes((16, 24), 2)
    assert plain.canvas_vae is not None and plain.canvas_vae.cfg.tiling == 0 and not plain.canvas_wrap


def test_without_canvas_nothing_is_built(sds):
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=WIN, with_text_encoder=False)
    assert pipe.canvas_hw is None and pipe.canvas_vae is None and pipe._pano is None
    with pytest.raises(ValueError, match='built without canvas_hw'):
        pipe.sample_panorama(torch.zeros(2, 77, 768, dtype=torch.float16), torch.zeros(1, 4, 16, 16), 'euler', 2)
