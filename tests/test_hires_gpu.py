"""The two-pass hires fix on the GPU, on ONE rig: Txt2Img(latent_hw=(8, 16), hires_hw=(16, 24)) -- both ratios, 2x and 1.5x, in one
resize -- plus the fp32 oracle modules.

Stated tolerances (fp16 GPU vs fp32 CPU, the project's chain bounds): the second pass from an injected latent, final latent rel-L2
<= 2e-2 and >= 99 % of the bytes within 2 LSB.  Bit-exact: generate_hires against its public parts, generate_hires_graphed against
eager, clear_loras against the image before set_loras, the two UNets' merged parameter bytes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lora_cases as C
from test_img2img_cpu import ldm_img2img_indices

pytestmark = pytest.mark.gpu

LO, HI = (8, 16), (16, 24)


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def rig():
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(*LO)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=LO, hires_hw=HI, with_vae=True, with_text_encoder=False, loras=True)
    with torch.device('meta'):
        unet, vae = S.UNetModel(), S.AutoencoderKLDecode()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, *LO, generator=g)
    return pipe, sds, unet.eval(), vae.eval(), ctx2, x_T


def test_rig_shape(rig):
    pipe = rig[0]
    hi = pipe.hires
    assert hi is not None and hi.hires is None and hi.text is None and hi.encoder is None and hi.vae is not None
    assert pipe._latent_shape == (4, 8, 16) and hi._latent_shape == (4, 16, 24)
    assert hi.unet is not pipe.unet and hi.unet.stats()['weight_bytes'] == pipe.unet.stats()['weight_bytes']
    assert hi.unet.base_bytes() == pipe.unet.base_bytes() > 0


@torch.no_grad()
def _oracle_second_pass(unet, vae, ctx2, z_lo, nu, denoise, steps, guidance):
    """fp32 restatement: F.interpolate (bilinear), the start formula, ldm's DDIM decode loop (eta 0, CFG) as
    test_img2img_gpu._oracle_img2img, decode_first_stage -> 255 clamp((x + 1) / 2)"""
    from oracle import pipeline_oracle as PO
    t_enc, seq, sa, s1a = ldm_img2img_indices(denoise, steps)
    x = sa * F.interpolate(z_lo, size=HI, mode='bilinear', align_corners=False) + s1a * nu
    ac = torch.tensor(PO._alphas_cumprod(), dtype=torch.float32)
    ddim_t = np.asarray(list(range(0, 1000, 1000 // steps))) + 1
    alphas = ac[ddim_t]
    alphas_prev = torch.tensor([float(ac[0])] + ac[ddim_t[:-1]].tolist())
    s1m = torch.sqrt(1. - alphas)
    c16 = ctx2.float()
    for step, index in seq:
        t = torch.full((x.shape[0],), float(step))
        e_u, e_c = PO.guided_eps(unet, x, t, c16[0:1], c16[1:2], guidance)
        e_t = e_u + guidance * (e_c - e_u)
        a_t, a_prev = alphas[index], alphas_prev[index]
        pred_x0 = (x - s1m[index] * e_t) / a_t.sqrt()
        x = a_prev.sqrt() * pred_x0 + (1. - a_prev).sqrt() * e_t
    return x, PO.decode_u8(vae, x, mode=1), t_enc


def test_second_pass_matches_oracle(rig):
    from sdod.amd import ops
    from sdod.amd.samplers import PlmsSchedule
    pipe, _, unet, vae, ctx2, _ = rig
    g = torch.Generator().manual_seed(5)
    z_lo = 0.8 * torch.randn(1, 4, *LO, generator=g)
    nu = torch.randn(1, 4, *HI, generator=g)
    z_ref, img_ref, t_enc = _oracle_second_pass(unet, vae, ctx2, z_lo, nu, 0.5, 20, 7.5)
    assert t_enc == 10
    c = ctx2.cuda()
    img = pipe.hires_from_latent(c, z_lo, 'plms', 7.5, hires_steps=20, hires_seed=1, denoise=0.5, upscaler='bilinear', hires_noise=nu)
    sch = PlmsSchedule(20)
    x = ops.latent_resize(z_lo.cuda(), HI, 'bilinear', float(sch.sqrt_alphas[10]), float(sch.sqrt_one_minus_alphas[10]), nu.cuda())
    z = pipe.hires.sample_ddim_from(c, x, 10, 20, 7.5)
    assert torch.equal(img, pipe.hires.decode(z, mode=1))
    r = rel_l2(z.cpu(), z_ref)
    print('hires second pass final latent rel-L2', r)
    assert torch.isfinite(z).all() and r <= 2e-2, r
    diff = np.abs(img.cpu().numpy().astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 192, 3) and frac >= 0.99, frac


def test_generate_hires_is_its_public_parts(rig):
    from sdod.amd import ops
    from sdod.amd.samplers import KSchedule, PlmsSchedule
    pipe, _, _, _, ctx2, x_T = rig
    c, hi = ctx2.cuda(), pipe.hires
    # 'plms': DDIM second pass, device noise of family 2 of hires_seed = seed + 1
    got = pipe.generate_hires(c, x_T, 6, 7.5, 'plms', hires_steps=10, denoise=0.5, upscaler='bicubic', seed=11, image_index=3)
    z_lo = pipe.sample_plms(c, x_T, 6, 7.5)
    sch = PlmsSchedule(10)
    x = ops.latent_resize(z_lo, HI, 'bicubic', float(sch.sqrt_alphas[5]), float(sch.sqrt_one_minus_alphas[5]), seed=12, image_index=3)
    want = hi.decode(hi.sample_ddim_from(c, x, 5, 10, 7.5), mode=1)
    assert got.shape == (1, 128, 192, 3) and torch.equal(got, want)
    # 'euler_a' on Karras with device noise: pass 1 on `seed`, pass 2 (start noise and step noise) on hires_seed
    kw = dict(hires_steps=8, denoise=0.5, upscaler='bilinear', schedule='karras', eta=1.0, seed=21, image_index=2)
    got = pipe.generate_hires(c, x_T, 6, 7.5, 'euler_a', **kw)
    assert torch.equal(got, pipe.generate_hires(c, x_T, 6, 7.5, 'euler_a', hires_seed=22, **kw))       # the default is seed + 1
    assert not torch.equal(got, pipe.generate_hires(c, x_T, 6, 7.5, 'euler_a', hires_seed=21, **kw))
    z_lo = pipe.sample_k(c, x_T, 'euler_a', 6, 7.5, 'karras', 1.0, 0, 21, 2)
    first = 8 - 4
    x = ops.latent_resize(z_lo, HI, 'bilinear', 1.0, float(KSchedule(8, 'karras').sigmas[first]), seed=22, image_index=2)
    want = hi.decode(hi.sample_k(c, x, 'euler_a', 8, 7.5, 'karras', 1.0, first, 22, 2), mode=1)
    assert torch.equal(got, want)
    # ... and with every noise injected
    g = torch.Generator().manual_seed(6)
    sn, hn, hsn = torch.randn(5, 1, 4, *LO, generator=g), torch.randn(1, 4, *HI, generator=g), torch.randn(3, 1, 4, *HI, generator=g)
    got = pipe.generate_hires(c, x_T, 6, 7.5, 'euler_a', step_noise=sn, hires_noise=hn, hires_step_noise=hsn, **kw)
    z_lo = pipe.sample_k(c, x_T, 'euler_a', 6, 7.5, 'karras', 1.0, 0, step_noise=sn)
    x = ops.latent_resize(z_lo, HI, 'bilinear', 1.0, float(KSchedule(8, 'karras').sigmas[first]), hn.cuda())
    want = hi.decode(hi.sample_k(c, x, 'euler_a', 8, 7.5, 'karras', 1.0, first, step_noise=hsn), mode=1)
    assert torch.equal(got, want)
    assert torch.equal(got, pipe.hires_from_latent(c, z_lo, 'euler_a', 7.5, hires_steps=8, hires_seed=22, denoise=0.5, upscaler='bilinear', schedule='karras',
                                                   hires_noise=hn, hires_step_noise=hsn))


def test_generate_hires_graphed_equals_eager(rig):
    pipe, _, _, _, ctx2, x_T = rig
    c = ctx2.cuda()
    x2 = torch.randn(1, 4, *LO, generator=torch.Generator().manual_seed(8))
    kw = dict(steps=6, guidance=7.5, sampler='dpmpp_2m', hires_steps=8, denoise=0.5, upscaler='bilinear', schedule='karras')
    e1 = pipe.generate_hires(c, x_T, seed=3, **kw)
    g1 = pipe.generate_hires_graphed(c, x_T, seed=3, **kw).clone()                      # (the replay's output buffer is reused)
    assert g1.shape == (1, 128, 192, 3) and g1.dtype == torch.uint8 and torch.equal(g1, e1)
    g2 = pipe.generate_hires_graphed(c, x2, seed=4, image_index=1, **kw).clone()
    assert torch.equal(g2, pipe.generate_hires(c, x2, seed=4, image_index=1, **kw))
    assert not torch.equal(g2, g1)
    assert pipe.use_hip_graph and pipe.hires.use_hip_graph                              # the capture put both switches back
    kwa = dict(steps=4, guidance=7.5, sampler='euler_a', hires_steps=6, denoise=0.5, upscaler='nearest-exact', schedule='karras')
    ga = pipe.generate_hires_graphed(c, x_T, seed=5, **kwa).clone()
    assert torch.equal(ga, pipe.generate_hires(c, x_T, seed=5, **kwa))
    gb = pipe.generate_hires_graphed(c, x2, seed=6, hires_seed=60, **kwa).clone()
    assert torch.equal(gb, pipe.generate_hires(c, x2, seed=6, hires_seed=60, **kwa)) and not torch.equal(ga, gb)
    gp = pipe.generate_hires_graphed(c, x_T, 4, 7.5, 'plms', hires_steps=6, denoise=0.5, seed=7)
    assert torch.equal(gp, pipe.generate_hires(c, x_T, 4, 7.5, 'plms', hires_steps=6, denoise=0.5, seed=7))
    pipe.unet.check(); pipe.hires.unet.check()


def test_upscalers_differ_and_denoise_domain(rig):
    pipe, _, _, _, ctx2, x_T = rig
    c = ctx2.cuda()
    z_lo = pipe.sample_k(c, x_T, 'dpmpp_2m', 4, 7.5, 'karras')
    imgs = [pipe.hires_from_latent(c, z_lo, 'dpmpp_2m', 7.5, hires_steps=6, denoise=0.5, upscaler=u, hires_seed=9).cpu()
            for u in ('nearest-exact', 'bilinear', 'bicubic')]
    assert all(i.shape == (1, 128, 192, 3) for i in imgs)
    assert not torch.equal(imgs[0], imgs[1]) and not torch.equal(imgs[1], imgs[2]) and not torch.equal(imgs[0], imgs[2])
    # t_enc == 0 (and t_enc == steps): refused as img2img refuses them, by the same schedule function
    for fn in (pipe.generate_hires, pipe.generate_hires_graphed):
        for denoise in (0.1, 1.0):                                    # int(0.1 * 6) = 0; int(1.0 * 6) = 6 = steps
            with pytest.raises(ValueError, match=r'outside \[1, steps - 1\]'):
                fn(c, x_T, 4, 7.5, 'dpmpp_2m', hires_steps=6, denoise=denoise)
    with pytest.raises(ValueError, match=r'outside \[1, steps - 1\]'):
        pipe.hires_from_latent(c, z_lo, 'dpmpp_2m', 7.5, hires_steps=6, hires_seed=1, denoise=0.1)


def test_loras_reach_both_unets(rig):
    pipe, sds, _, _, ctx2, x_T = rig
    c = ctx2.cuda()
    names = ['input_blocks.1.0.in_layers.2.weight', 'middle_block.1.transformer_blocks.0.ff.net.2.weight']
    ent = C.make_entries(sds['unet'], names, 4, 1.0, seed=5)
    adapter = C.kohya_state_dict(ent, 4.0)
    kw = dict(steps=4, guidance=7.5, sampler='dpmpp_2m', hires_steps=6, denoise=0.5, seed=2)
    z_lo = pipe.sample_k(c, x_T, 'dpmpp_2m', 4, 7.5, 'karras')
    before = pipe.generate_hires(c, x_T, **kw).clone()
    second_before = pipe.hires_from_latent(c, z_lo, 'dpmpp_2m', 7.5, hires_steps=6, denoise=0.5, hires_seed=3).clone()
    graphed_before = pipe.generate_hires_graphed(c, x_T, **kw).clone()
    assert torch.equal(graphed_before, before)
    base = [pipe.unet.packed_param(n).clone() for n in names]
    for n, b in zip(names, base):
        assert torch.equal(pipe.hires.unet.packed_param(n), b)
    assert pipe.set_loras([(adapter, 1.0)]) == []
    try:
        for n, b in zip(names, base):
            merged = pipe.unet.packed_param(n)
            assert not torch.equal(merged, b)
            assert torch.equal(pipe.hires.unet.packed_param(n), merged)           # the same merge on the same bytes
        # the second pass alone, from the SAME latent: only the hires UNet's adapter can change it
        assert not torch.equal(pipe.hires_from_latent(c, z_lo, 'dpmpp_2m', 7.5, hires_steps=6, denoise=0.5, hires_seed=3), second_before)
        after = pipe.generate_hires(c, x_T, **kw).clone()
        assert not torch.equal(after, before)
        assert torch.equal(pipe.generate_hires_graphed(c, x_T, **kw), after)      # captured before set_loras, replayed after it
    finally:
        pipe.clear_loras()
    for n, b in zip(names, base):
        assert torch.equal(pipe.unet.packed_param(n), b) and torch.equal(pipe.hires.unet.packed_param(n), b)
    assert torch.equal(pipe.generate_hires(c, x_T, **kw), before)
    assert torch.equal(pipe.hires_from_latent(c, z_lo, 'dpmpp_2m', 7.5, hires_steps=6, denoise=0.5, hires_seed=3), second_before)
    assert torch.equal(pipe.generate_hires_graphed(c, x_T, **kw), before)
