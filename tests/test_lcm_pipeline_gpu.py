"""LCM few-step sampling through the pipeline, latent 16 x 16, synthetic weights (the fixtures' pattern of tests/test_ksamplers_gpu.py).

Against the fp32 CPU restatement of tests/lcm_ref.py (the oracle UNet plus the cond_proj term), 4 steps with injected step noise:
unguided with the guidance embedding (w = 8), guided (CFG 1.5), unguided on model='sd21' (latent 24, the size of the sd21 pipeline
tests; 2 steps).  Tolerance: the project's chain tolerance, final latent rel-L2 <= 2e-2 and >= 99 % of the uint8 pixels within 2 LSB.

Bit for bit: graphed against eager, device noise against injected noise from the same streams, one step (which draws nothing),
img2img_lcm against its parts; clear_loras() against the rows before set_loras().

lora_time_modules: the adapted time-embedding rows against a pipeline built from the host merge (rel-L2 <= 5e-3, the TEMB graph's own
tolerance and the one tests/test_lora_engine_gpu.py holds the text encoder's device merge to), and a captured trajectory following
set_loras() without a recapture.

A pipeline without the new arguments: the launch counts and arena bytes recorded on the parent commit."""
import numpy as np
import pytest
import torch

import lcm_ref as R

pytestmark = pytest.mark.gpu

# launch count and activation-arena bytes at 16x16 from before this feature: the batch-2 UNet graph as tests/test_freeu_gpu.py records
# it, and the 4-row TEMB graph a 4-step schedule makes, recorded on the parent commit
PARENT_UNET = (321, 4260096)
PARENT_TEMB4 = (5, 23296)


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def w16():
    """synthetic weights at latent 16 and the CPU models of oracle.sd_torch on them; cond_proj as a trained projection is sized"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table(),
              'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    cond_proj = (torch.randn(320, 256, generator=torch.Generator().manual_seed(7)) / 16.0).half()
    with torch.device('meta'):
        unet, vae = S.UNetModel(), S.AutoencoderKLDecode()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    img = torch.stack([128 + 90 * torch.sin(xx / 11 + k) * torch.cos(yy / 17) for k in range(3)], -1)
    u8 = (img + 10 * torch.randn(128, 128, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]
    return dict(cfg=cfg, sds=sds, cond_proj=cond_proj, unet=unet.eval(), vae=vae.eval(), ctx2=ctx2, u8=u8,
                noise=(torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)),
                x_T=torch.randn(1, 4, 16, 16, generator=g), x_T2=torch.randn(2, 4, 16, 16, generator=g),
                step_noise=torch.randn(3, 1, 4, 16, 16, generator=g))


@pytest.fixture(scope='module')
def guided(w16):
    """a pipeline without any of the new arguments"""
    from sdod.amd.pipeline import Txt2Img
    return Txt2Img(state_dicts=w16['sds'], images_per_gpu=1, latent_hw=16, with_text_encoder=False, with_vae_encoder=True)


@pytest.fixture(scope='module')
def embedded(w16):
    """unguided, with the guidance embedding"""
    from sdod.amd.pipeline import Txt2Img
    sds = dict(w16['sds'], temb={**w16['sds']['temb'], 'time_embed.cond_proj.weight': w16['cond_proj']})
    return Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, with_text_encoder=False, unguided=True, guidance_embed=True)


def _image_check(img, img_ref, what):
    img = img.cpu().numpy()
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print(f'{what}: uint8 image max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == img_ref.shape and frac >= 0.99, frac


# ------------------------------------------------------------------ the unguided build
def test_unguided_build_has_one_row_per_image(w16, embedded):
    from sdod.amd.pipeline import Txt2Img
    assert embedded.unet.batch == 1 and embedded.unguided and embedded.guidance_embed
    assert tuple(embedded.unet.x.shape) == (1, 4, 16, 16) and tuple(embedded.unet.ctx.shape) == (1, 77, 768)
    two = Txt2Img(state_dicts=w16['sds'], images_per_gpu=2, latent_hw=16, with_text_encoder=False, with_vae=False, unguided=True)
    assert two.unet.batch == 2 and tuple(two.unet.eps.shape) == (2, 16, 16, 4) and not two.guidance_embed
    # one evaluation against the CPU oracle's conditional row (the bound of tests/test_engine_gpu.py's UNet evaluations: rel-L2 1e-2)
    ctx2, x = w16['ctx2'], w16['x_T2']
    t = torch.tensor([499.0])
    temb = two.time_embeddings(t.numpy())
    two._set_context(ctx2.cuda(), lcm=True)
    assert torch.equal(two.unet.ctx.cpu(), ctx2[1:2].expand(2, -1, -1))
    from sdod.amd import ops
    ops.stage_unet_inputs(x.cuda(), two.unet.x, temb[0], two._temb_dst)
    out = two._unet_eps().float().cpu().permute(0, 3, 1, 2)
    ref = R.unet_eval(w16['unet'], x, t.expand(2), ctx2[1:2].float().expand(2, -1, -1))
    r = rel_l2(out, ref)
    print(f'unguided UNet b2 16x16 rel-L2 vs the oracle conditional row {r:.3e}')
    assert torch.isfinite(out).all() and r <= 1e-2, r
    assert rel_l2(out, R.unet_eval(w16['unet'], x, t.expand(2), ctx2[0:1].float().expand(2, -1, -1))) > 10 * r      # not the unconditional one
    # a sampler of the pair raises on it, before it stages anything
    with pytest.raises(ValueError, match='unguided=True'):
        two.sample_plms(ctx2.cuda(), x)
    z = two.sample_lcm(ctx2.cuda(), x, 2, seed=4)
    assert tuple(z.shape) == (2, 4, 16, 16) and torch.isfinite(z).all()
    assert not torch.equal(two.sample_lcm(ctx2.cuda(), x, 2, seed=5), z)          # two steps: one draw, from the seed's streams


# ------------------------------------------------------------------ chains against the restatement
def test_unguided_chain_with_the_guidance_embedding(w16, embedded):
    r, pipe = w16, embedded
    ctx2 = r['ctx2'].cuda()
    z_ref = R.sample_lcm(r['unet'], r['ctx2'], r['x_T'], 4, r['step_noise'], w=8.0, cond_proj=r['cond_proj'])
    z, den = pipe.sample_lcm(ctx2, r['x_T'], 4, 8.0, step_noise=r['step_noise'], return_denoised=True)
    rl = rel_l2(z.cpu(), z_ref)
    away = rel_l2(R.sample_lcm(r['unet'], r['ctx2'], r['x_T'], 4, r['step_noise']), z_ref)
    print(f'LCM chain unguided w = 8: final latent rel-L2 {rl:.3e}; without the embedding the restatement is {away:.3e} away')
    assert torch.isfinite(z).all() and rl <= 2e-2, rl
    assert away > 2e-2                           # the embedding is visible at this tolerance
    assert rel_l2(den, z) < 1e-6                 # the last step: c_skip x + c_out den with c_skip = 4e-8
    from oracle import pipeline_oracle as PO
    img = pipe.generate_lcm(ctx2, r['x_T'], 4, 8.0, step_noise=r['step_noise'])
    assert torch.equal(img, pipe.decode(z, mode=1))
    _image_check(img, PO.decode_u8(r['vae'], z_ref, mode=1), 'LCM chain unguided w = 8')
    # another w is another trajectory, and the cache key carries it
    assert not torch.equal(pipe.sample_lcm(ctx2, r['x_T'], 4, 2.0, step_noise=r['step_noise']), z)
    assert {k[1] for k in pipe._temb_cache} >= {8.0, 2.0} and all(isinstance(k[0], tuple) for k in pipe._temb_cache)


def test_guided_chain(w16, guided):
    r, pipe = w16, guided
    ctx2 = r['ctx2'].cuda()
    z_ref = R.sample_lcm(r['unet'], r['ctx2'], r['x_T'], 4, r['step_noise'], guidance=1.5)
    z = pipe.sample_lcm(ctx2, r['x_T'], 4, 1.5, step_noise=r['step_noise'])
    rl = rel_l2(z.cpu(), z_ref)
    print(f'LCM chain guided 1.5: final latent rel-L2 {rl:.3e}')
    assert torch.isfinite(z).all() and rl <= 2e-2, rl
    from oracle import pipeline_oracle as PO
    img = pipe.generate_lcm(ctx2, r['x_T'], 4, 1.5, step_noise=r['step_noise'])
    assert torch.equal(img, pipe.decode(z, mode=1))
    _image_check(img, PO.decode_u8(r['vae'], z_ref, mode=1), 'LCM chain guided 1.5')
    # guidance None is CFG at 1
    assert torch.equal(pipe.sample_lcm(ctx2, r['x_T'], 4, step_noise=r['step_noise']), pipe.sample_lcm(ctx2, r['x_T'], 4, 1.0, step_noise=r['step_noise']))


def test_unguided_chain_on_sd21():
    """v-prediction, 64-wide heads, context 1024; latent 24 as tests/test_pipeline_gpu.py's sd21 pipeline test.  Two steps -- one with
    fresh noise, then the last -- keep the CPU side of this case short; the four-step grid runs in the two sd14 cases."""
    from oracle import pipeline_oracle as PO, sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd21_config(24, 24)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=2100 + i) for i, (k, t) in enumerate(tables.items())}
    with torch.device('meta'):
        unet, vae = S.UNetModel(context_dim=1024, head_dim=64, use_linear=True), S.AutoencoderKLDecode()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=24, model='sd21', with_text_encoder=False, unguided=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = torch.randn(2, 77, 1024, generator=g).half()
    x_T = torch.randn(1, 4, 24, 24, generator=g)
    sn = torch.randn(1, 1, 4, 24, 24, generator=g)
    z_ref = R.sample_lcm(unet.eval(), ctx2, x_T, 2, sn, v_prediction=True)
    z = pipe.sample_lcm(ctx2.cuda(), x_T, 2, step_noise=sn)
    rl = rel_l2(z.cpu(), z_ref)
    print(f'LCM chain unguided sd21 (v-prediction): final latent rel-L2 {rl:.3e}')
    assert pipe.unet.batch == 1 and torch.isfinite(z).all() and rl <= 2e-2, rl
    _image_check(pipe.generate_lcm(ctx2.cuda(), x_T, 2, step_noise=sn), PO.decode_u8(vae.eval(), z_ref, mode=1), 'LCM chain unguided sd21')


# ------------------------------------------------------------------ equalities, bit for bit
@pytest.mark.parametrize('which', ['embedded', 'guided'])
def test_graphed_equals_eager_and_device_noise_equals_injected(w16, guided, embedded, which):
    from sdod.amd import ops
    r = w16
    pipe, g = (embedded, 8.0) if which == 'embedded' else (guided, 1.5)
    c, x_T = r['ctx2'].cuda(), r['x_T']
    eager = pipe.generate_lcm(c, x_T, 4, g, step_noise=r['step_noise'])
    n_before = len(pipe._traj or {})
    graphed = pipe.generate_lcm_graphed(c, x_T, 4, g, step_noise=r['step_noise']).clone()
    assert torch.equal(graphed, eager) and len(pipe._traj) == n_before + 1
    # device noise is the injected noise of the documented streams: family 3 + i behind step i
    eager1 = pipe.generate_lcm(c, x_T, 4, g, seed=31, image_index=3)
    inj = torch.stack([ops.randn((1, 4, 16, 16), 31, ((3 + i) << 32) | 3, 'cuda') for i in range(3)])
    assert torch.equal(pipe.generate_lcm(c, x_T, 4, g, step_noise=inj), eager1) and not torch.equal(eager1, eager)
    graphed1 = pipe.generate_lcm_graphed(c, x_T, 4, g, seed=31, image_index=3).clone()
    assert torch.equal(graphed1, eager1) and len(pipe._traj) == n_before + 1              # a replay, not a new capture
    eager2 = pipe.generate_lcm(c, x_T, 4, g, seed=32, image_index=3)
    assert torch.equal(pipe.generate_lcm_graphed(c, x_T, 4, g, seed=32, image_index=3), eager2) and not torch.equal(eager2, eager1)
    assert len(pipe._traj) == n_before + 1                                              # the graph bakes no seed
    assert not torch.equal(pipe.generate_lcm(c, x_T, 4, g, seed=31, image_index=4), eager1)
    # one step: works, draws nothing, and its graph has no noise input
    one = pipe.generate_lcm(c, x_T, 1, g, seed=1)
    assert torch.equal(pipe.generate_lcm(c, x_T, 1, g, seed=2, image_index=9), one)
    assert torch.equal(pipe.generate_lcm_graphed(c, x_T, 1, g, seed=3), one) and len(pipe._traj) == n_before + 2
    assert len(pipe._traj[('lcm', 1, g, (1, 4, 16, 16), 50, 1.0)][1]) == 2
    z, den = pipe.sample_lcm(c, x_T, 1, g, return_denoised=True)
    assert torch.isfinite(z).all() and rel_l2(z, den) < 1e-6


def test_img2img_lcm_is_its_parts(w16, guided):
    from sdod.amd.samplers import LcmSchedule
    r, pipe = w16, guided
    c, u8 = r['ctx2'].cuda(), r['u8']
    strength, steps = 0.5, 4
    sch = LcmSchedule(steps, strength=strength)
    assert sch.timesteps.tolist() == [499, 379, 259, 139]
    x, z0 = pipe.encode(u8, noise=r['noise'], return_z0=True, coef=sch.start())
    a, b = (float(np.float32(v)) for v in sch.start())              # the kernel takes the coefficients as fp32
    want_x = a * z0.cpu().double() + b * r['noise'][1].double()
    assert bool(((x.cpu().double() - want_x).abs() <= 2.0 ** -23 * (want_x.abs() + 1.0)).all())
    z = pipe.sample_lcm(c, x, steps, 1.5, strength=strength, step_noise=r['step_noise'])
    want = pipe.decode(z, mode=1)
    got = pipe.img2img_lcm(c, u8, strength, steps, 1.5, noise=r['noise'], step_noise=r['step_noise'])
    assert torch.equal(got, want)
    assert not torch.equal(got, pipe.generate_lcm(c, x, steps, 1.5, step_noise=r['step_noise']))       # strength moves the grid
    # device noise, everywhere: the encoder's two streams and the steps' own
    x2 = pipe.encode(u8, 31, 3, coef=sch.start())
    want2 = pipe.decode(pipe.sample_lcm(c, x2, steps, 1.5, strength=strength, seed=31, image_index=3), mode=1)
    assert torch.equal(pipe.img2img_lcm(c, u8, strength, steps, 1.5, seed=31, image_index=3), want2) and not torch.equal(want2, got)


# ------------------------------------------------------------------ LoRA on the time conditioning
def _time_lora():
    g = torch.Generator().manual_seed(3)

    def mod(out, inp, rank=4):
        return {'lora_down.weight': torch.randn(rank, inp, generator=g) * 0.05, 'lora_up.weight': torch.randn(out, rank, generator=g) * 0.05,
                'alpha': torch.tensor(4.0)}
    mods = {'lora_unet_down_blocks_1_resnets_0_time_emb_proj': mod(640, 1280), 'lora_unet_time_embedding_linear_1': mod(1280, 320),
            'lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q': mod(320, 320)}
    return {f'{m}.{k}': v for m, d in mods.items() for k, v in d.items()}


def test_lora_time_modules(w16):
    from sdod.amd import lycoris as L
    from sdod.amd.pipeline import Txt2Img
    r = w16
    c, x_T, sn = r['ctx2'].cuda(), r['x_T'], r['step_noise']
    pipe = Txt2Img(state_dicts=r['sds'], images_per_gpu=1, latent_hw=16, with_text_encoder=False, loras=True, lora_time_modules=True)
    f = _time_lora()
    times = np.asarray([999.0, 759.0, 499.0, 259.0], dtype=np.float32)
    base_rows = pipe.time_embeddings(times).clone()
    cached = pipe.time_embeddings(times)
    base_img = pipe.generate_lcm_graphed(c, x_T, 4, 1.5, step_noise=sn).clone()           # captured BEFORE the adapter is set
    n_graphs = len(pipe._traj)
    assert pipe.set_loras([(f, 1.0)]) == []
    assert pipe.time_embeddings(times) is cached and cached.data_ptr() == pipe._temb_cache[tuple(float(t) for t in times)].data_ptr()
    # the rows of a pipeline built from the host merge of the same file
    ent, _ = L.entries_for(f, 'sd14', 1.0, 1.0, time_modules=True)
    assert len(ent['temb']) == 2 and len(ent['unet']) == 1
    merged = dict(r['sds'], temb=L.merged_state_dict(r['sds']['temb'], ent['temb']), unet=L.merged_state_dict(r['sds']['unet'], ent['unet']))
    host = Txt2Img(state_dicts=merged, images_per_gpu=1, latent_hw=16, with_text_encoder=False)
    want_rows = host.time_embeddings(times)
    rl, moved = rel_l2(cached.float(), want_rows.float()), rel_l2(cached.float(), base_rows.float())
    print(f'time-embedding rows, device merge vs host merge: rel-L2 {rl:.3e} (tolerance 5e-3); moved from the base rows by {moved:.3e}')
    assert rl <= 5e-3 and moved >= 10 * 5e-3
    # a schedule length met later: its TEMB graph starts from the adapters in force
    three = pipe.time_embeddings(times[:3])
    assert rel_l2(three.float(), want_rows[:3].float()) <= 5e-3 and rel_l2(three.float(), base_rows[:3].float()) >= 10 * 5e-3
    # the captured trajectory follows without a recapture, and gives the adapted pipeline's eager result
    eager = pipe.generate_lcm(c, x_T, 4, 1.5, step_noise=sn)
    graphed = pipe.generate_lcm_graphed(c, x_T, 4, 1.5, step_noise=sn).clone()
    assert len(pipe._traj) == n_graphs and torch.equal(graphed, eager) and not torch.equal(graphed, base_img)
    z = pipe.sample_lcm(c, x_T, 4, 1.5, step_noise=sn)
    z_host = host.sample_lcm(c, x_T, 4, 1.5, step_noise=sn)
    print(f'adapted chain, device merge vs host merge: final latent rel-L2 {rel_l2(z, z_host):.3e}')
    assert rel_l2(z, z_host) <= 2e-2
    # clear_loras() restores the rows, bit for bit, in the same memory
    assert pipe.clear_loras() == []
    assert torch.equal(cached, base_rows) and pipe.time_embeddings(times) is cached
    assert rel_l2(pipe.time_embeddings(times[:3]).float(), base_rows[:3].float()) <= 1e-3
    assert torch.equal(pipe.generate_lcm_graphed(c, x_T, 4, 1.5, step_noise=sn), base_img) and len(pipe._traj) == n_graphs


# ------------------------------------------------------------------ nothing for a pipeline without the arguments
def test_a_pipeline_without_the_arguments_builds_the_parent_graphs(w16, guided):
    from sdod.amd import engine as E
    pipe = guided
    assert not pipe.unguided and not pipe.guidance_embed and not pipe.lora_time_modules and pipe._time_networks == ()
    s = pipe.unet.stats()
    assert pipe.unet.batch == 2 and (s['launches'], s['arena_bytes']) == PARENT_UNET
    tg = pipe._temb_graph(4)
    st = tg.stats()
    print(f'plain TEMB b4: {st["launches"]} launches, arena {st["arena_bytes"]} B')
    assert (st['launches'], st['arena_bytes']) == PARENT_TEMB4
    assert tg.cond_proj_dim == 0 and not hasattr(tg, 'w') and tg.base_bytes() == 0
    raw = E.Graph(E.TEMB, w16['cfg'], 4)                  # sdod_graph_create, the entry point of every build before this one
    assert raw.param_table() == tg.param_table()
    raw.load_state_dict(w16['sds']['temb']); raw.finalize()
    assert raw.op_table() == tg.op_table() and raw.op_details() == tg.op_details() and raw.stats() == st
    assert all(isinstance(k, tuple) and all(isinstance(v, float) for v in k) for k in pipe._temb_cache)      # keys are the times alone
