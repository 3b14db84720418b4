"""Inpainting on the GPU: the three kernels it adds, bit for bit against numpy / the launches they fuse, and the whole chain (mask
reduction -> encoder -> start latent -> masked DDIM -> decode -> pixel composite) against an fp32 CPU restatement of the definition
(ldm DDIMSampler.ddim_sampling(mask=, x0=) on scripts/img2img.py's start, blended after every step) with injected noise.

Stated tolerances (fp16 GPU vs fp32 CPU), the chain tolerances of test_img2img_gpu.py / test_pipeline_gpu.py: final latent rel-L2 <=
2e-2 and >= 99 % of the uint8 pixels within 2 LSB.  Everything else here is bit-exact: mask_to_latent and image_composite against
integer / fp32 numpy, the fused step against cfg_combine -> (lincomb4) -> ddim_step -> torch's fp32 blend -> stage_unet_inputs, in-kernel
noise against sdod_randn_f32, the kept region against z0 and the init image, the all-255 mask against img2img(), graphed against eager."""
import numpy as np
import pytest
import torch

from test_img2img_cpu import LdmEncoder, ldm_img2img_indices

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------ latent keep-mask
def _keep_numpy(mask):
    n, h, w = mask.shape
    s = mask.reshape(n, h // 8, 8, w // 8, 8).astype(np.int64).sum(axis=(2, 4))
    return (16320 - s).astype(np.float32) / np.float32(16320.0)


@pytest.mark.parametrize('n,hl,wl', [(1, 16, 16), (2, 16, 24), (1, 64, 64), (3, 5, 7)])
def test_mask_to_latent_bit_exact(n, hl, wl):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(n * 100 + wl)
    single = torch.zeros(n, 8 * hl, 8 * wl, dtype=torch.uint8)
    single[n - 1, 8 * hl - 3, 8 * wl - 10] = 255
    sparse = torch.randint(0, 256, (n, 8 * hl, 8 * wl), generator=g, dtype=torch.uint8)
    sparse[torch.rand(sparse.shape, generator=g) < 0.7] = 0
    masks = {'random': torch.randint(0, 256, (n, 8 * hl, 8 * wl), generator=g, dtype=torch.uint8), 'sparse': sparse,
             'zeros': torch.zeros(n, 8 * hl, 8 * wl, dtype=torch.uint8), 'full': torch.full((n, 8 * hl, 8 * wl), 255, dtype=torch.uint8),
             'single': single}
    for name, m in masks.items():
        got = ops.mask_to_latent(m.cuda()).cpu().numpy()
        want = _keep_numpy(m.numpy())
        assert got.shape == (n, hl, wl) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert float(ops.mask_to_latent(masks['zeros'].cuda()).min()) == 1.0
    assert float(ops.mask_to_latent(masks['full'].cuda()).abs().max()) == 0.0
    k = ops.mask_to_latent(single.cuda()).cpu()
    assert int((k != 1.0).sum()) == 1 and float(k.min()) == float(np.float32(16065) / np.float32(16320))


def test_mask_to_latent_refuses_another_factor():
    import ctypes
    from sdod.amd import _lib
    lib = _lib.hip()
    m = torch.zeros(1, 64, 64, dtype=torch.uint8, device='cuda')
    out = torch.full((1, 16, 16), 7.0, device='cuda')
    rc = lib.sdod_mask_to_latent_f32(ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(out.data_ptr()), 1, 16, 16, 4, None)
    torch.cuda.synchronize()
    assert rc != 0 and b'factor' in lib.sdod_hip_last_error()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ pixel composite
@pytest.mark.parametrize('n,h,w', [(1, 128, 128), (2, 7, 9), (1, 1, 1), (1, 512, 512)])
def test_image_composite_bit_exact(n, h, w):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(h * 3 + w)
    img = (1.4 * torch.randn(n, h, w, 3, generator=g)).half().cuda()        # beyond both clamp bounds
    init = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    mask = torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8)
    mask[torch.rand(mask.shape, generator=g) < 0.25] = 0
    mask[torch.rand(mask.shape, generator=g) < 0.25] = 255
    d = ops.image_to_u8(img, 0.5, 0.5, 1).cpu().numpy().astype(np.int64)
    u = init.numpy().astype(np.int64)
    k = mask.numpy().astype(np.int64)[..., None]
    want = ((d * k + u * (255 - k) + 127) // 255).astype(np.uint8)
    got = ops.image_composite(img, init.cuda(), mask.cuda(), 0.5, 0.5, 1).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[mask.numpy() == 0], init.numpy()[mask.numpy() == 0])
    assert np.array_equal(got[mask.numpy() == 255], d.astype(np.uint8)[mask.numpy() == 255])
    zeros, full = torch.zeros_like(mask).cuda(), torch.full_like(mask, 255).cuda()
    assert torch.equal(ops.image_composite(img, init.cuda(), zeros), init.cuda())
    assert torch.equal(ops.image_composite(img, init.cuda(), full), ops.image_to_u8(img, 0.5, 0.5, 1))
    # mode 0 shares the device function as well
    d0 = ops.image_to_u8(img, 1.0, 0.0, 0)
    assert torch.equal(ops.image_composite(img, init.cuda(), full, 1.0, 0.0, 0), d0)


# ------------------------------------------------------------------ the fused step
COEF = dict(sqrt_one_minus_at=0.7310585786, sqrt_at=0.6823278038, sqrt_a_prev=0.7615941559, dir_coef=0.6480542737)
KNOWN = (0.7615941559, 0.6480542737)


def _step_inputs(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(2 * n, h, w, c, generator=g).half().cuda()
    x = torch.randn(n, c, h, w, generator=g).cuda()
    z0 = torch.randn(n, c, h, w, generator=g).cuda()
    nu = torch.randn(n, c, h, w, generator=g).cuda()
    keep = torch.rand(n, h, w, generator=g)
    keep[torch.rand(n, h, w, generator=g) < 0.3] = 1.0
    keep[torch.rand(n, h, w, generator=g) < 0.3] = 0.0
    temb_row = torch.randn(520, generator=g).half().cuda()
    return eps, x, z0, nu, keep.cuda(), temb_row


def _composed(eps, x, z0, keep, known, nu, guidance, v_coef, stage):
    """the separate launches + torch's eager fp32 blend (every operation rounded on its own)"""
    from sdod.amd import ops
    e = ops.cfg_combine(eps, guidance, uncond_first=True, mode=1)
    if v_coef is not None:
        e = ops.lincomb4([e, x], [v_coef[0], v_coef[1]], 1.0)
    xn = x.clone()
    ops.ddim_step(xn, e, **COEF)
    if keep is not None:
        k = keep[:, None]
        kn = z0 if known is None else known[0] * z0 + known[1] * nu
        xn = k * kn + (1 - k) * xn
    if stage is not None:
        ops.stage_unet_inputs(xn, stage[0], stage[1], stage[2])
    return xn


def _direct_last_step(eps, x, z0, keep, noise, guidance, v_coef):
    """sdod_ddim_inpaint_step with last = 1 and a non-NULL noise pointer, filled in here and not by ops"""
    import ctypes
    from sdod.amd import _lib
    lib = _lib.hip()
    n, c, h, w = x.shape
    a = _lib.DdimInpaintStepArgs()
    a.eps_nhwc, a.x, a.z0, a.keep, a.noise = (ctypes.c_void_p(t.data_ptr()) for t in (eps, x, z0, keep, noise))
    a.n, a.c, a.hw, a.uncond_first, a.mode, a.last = n, c, h * w, 1, 1, 1
    a.guidance = guidance
    if v_coef is not None:
        a.v_pred, a.vc0, a.vc1 = 1, v_coef[0], v_coef[1]
    a.sqrt_one_minus_at, a.sqrt_at, a.sqrt_a_prev, a.dir_coef = (COEF[k] for k in ('sqrt_one_minus_at', 'sqrt_at', 'sqrt_a_prev', 'dir_coef'))
    torch.cuda.synchronize()
    _lib.check(lib.sdod_ddim_inpaint_step(ctypes.byref(a), None))
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', [(2, 4, 16, 24), (2, 4, 10, 13), (1, 4, 64, 64), (3, 4, 5, 7)])
@pytest.mark.parametrize('v_pred', [False, True])
@pytest.mark.parametrize('staged', [False, True])
@pytest.mark.parametrize('case', ['injected', 'device', 'last', 'plain'])
def test_ddim_inpaint_step_equals_the_composition(shape, v_pred, staged, case):
    """(2, 4, 10, 13) and (3, 4, 5, 7): hw % 4 != 0, so a thread's four elements straddle channels, and the element count is not a
    multiple of a block's span (1024)"""
    from sdod.amd import ops
    n, c, h, w = shape
    eps, x, z0, nu, keep, temb_row = _step_inputs(n, c, h, w, seed=h * 31 + w)
    guidance, seed, level, idx0 = 7.5, 987654321, 4, 5
    v_coef = (0.83, 0.557) if v_pred else None

    def stage():
        return (torch.full((2 * n, c, h, w), -3.0, device='cuda'), temb_row, torch.zeros(2 * n, 520, dtype=torch.float16, device='cuda')) \
            if staged else None

    if case == 'device':          # in-kernel noise == sdod_randn_f32 on stream ((3 + level) << 32) | (image_index + i)
        nu = torch.cat([ops.randn((1, c, h, w), seed, ((3 + level) << 32) | (idx0 + i), 'cuda') for i in range(n)])
    known = None if case == 'last' else KNOWN
    kw = dict(z0=z0, keep=keep, known=known, noise=None if case in ('device', 'last') else nu, seed=seed, noise_level=level, image_index=idx0)
    if case == 'plain':
        kw = {}
    s_ref, s_got = stage(), stage()
    want = _composed(eps, x, z0, None if case == 'plain' else keep, known, nu, guidance, v_coef, s_ref)
    got = x.clone()
    ops.ddim_inpaint_step(eps, got, COEF, guidance, mode=1, v_coef=v_coef, stage=s_got, **kw)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if staged:
        assert torch.equal(s_got[0].view(torch.int32), s_ref[0].view(torch.int32)) and torch.equal(s_got[2], s_ref[2])
        assert torch.equal(s_got[0][:n].view(torch.int32), got.view(torch.int32))
    if case == 'plain':          # == cfg_combine + ddim_step
        e = ops.cfg_combine(eps, guidance, uncond_first=True, mode=1)
        if v_pred:
            e = ops.lincomb4([e, x], list(v_coef), 1.0)
        two = x.clone()
        ops.ddim_step(two, e, **COEF)
        assert torch.equal(got, two)
    elif case == 'last':         # the kernel gets last = 1 AND a noise pointer (ops forwards it): NaNs there change nothing; keep == 1 -> z0
        again = x.clone()
        ops.ddim_inpaint_step(eps, again, COEF, guidance, v_coef=v_coef, z0=z0, keep=keep, known=None,
                              noise=torch.full_like(x, float('nan')))
        assert torch.equal(again, got)
        direct = x.clone()                                           # and through the C ABI itself, field by field
        _direct_last_step(eps, direct, z0, keep, torch.full_like(x, float('nan')), guidance, v_coef)
        assert torch.equal(direct, got)
        k = keep[:, None].expand_as(got)
        assert torch.equal(got[k == 1.0], z0[k == 1.0]) and torch.equal(got[k == 0.0], _composed(eps, x, z0, None, None, nu, guidance, v_coef, None)[k == 0.0])
    else:
        assert not torch.equal(got, _composed(eps, x, z0, None, None, nu, guidance, v_coef, None))


def test_ddim_inpaint_step_device_noise_depends_on_level_seed_and_index():
    from sdod.amd import ops
    eps, x, z0, nu, keep, _ = _step_inputs(2, 4, 16, 16, seed=3)
    outs = []
    for seed, level, idx0 in ((1, 0, 0), (2, 0, 0), (1, 1, 0), (1, 0, 1)):
        got = x.clone()
        ops.ddim_inpaint_step(eps, got, COEF, 7.5, z0=z0, keep=keep, known=KNOWN, seed=seed, noise_level=level, image_index=idx0)
        outs.append(got)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(outs[a], outs[b])
    # image 1 at image_index 0 draws the stream of image 0 at image_index 1
    n0 = ops.randn((1, 4, 16, 16), 1, (3 << 32) | 1, 'cuda')
    a = x.clone()
    ops.ddim_inpaint_step(eps, a, COEF, 7.5, z0=z0, keep=keep, known=KNOWN, seed=1, noise_level=0, image_index=0)
    b = x.clone()
    inj = torch.cat([ops.randn((1, 4, 16, 16), 1, (3 << 32) | 0, 'cuda'), n0])
    ops.ddim_inpaint_step(eps, b, COEF, 7.5, z0=z0, keep=keep, known=KNOWN, noise=inj)
    assert torch.equal(a, b)


def test_ddim_inpaint_step_refuses_bad_arguments_and_leaves_outputs_untouched():
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    n, c, h, w = 2, 4, 16, 16
    eps, x, z0, nu, keep, temb_row = _step_inputs(n, c, h, w, seed=9)
    x_dst = torch.full((2 * n, c, h, w), -3.0, device='cuda')
    temb_dst = torch.zeros(2 * n, 520, dtype=torch.float16, device='cuda')
    before = x.clone()

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(x, before) and bool((x_dst == -3.0).all()) and bool((temb_dst == 0).all())

    stage = (x_dst, temb_row, temb_dst)
    with pytest.raises(SdodError):                                   # keep without z0
        ops.ddim_inpaint_step(eps, x, COEF, 7.5, keep=keep, known=KNOWN, noise=nu, stage=stage)
    assert untouched()
    with pytest.raises(SdodError):                                   # a mode that does not exist
        ops.ddim_inpaint_step(eps, x, COEF, 7.5, z0=z0, keep=keep, known=KNOWN, noise=nu, mode=2, stage=stage)
    assert untouched()
    with pytest.raises(SdodError):                                   # sqrt_at = 0: a division by zero
        ops.ddim_inpaint_step(eps, x, dict(COEF, sqrt_at=0.0), 7.5, z0=z0, keep=keep, known=KNOWN, noise=nu, stage=stage)
    assert untouched()
    big = torch.zeros(n * c * h * w + 4, device='cuda')
    with pytest.raises(SdodError):                                   # noise not 16-byte aligned
        ops.ddim_inpaint_step(eps, x, COEF, 7.5, z0=z0, keep=keep, known=KNOWN, noise=big[1:1 + n * c * h * w], stage=stage)
    assert untouched()
    # c * hw not a multiple of 4
    eps3 = torch.zeros(2, 5, 1, 3, dtype=torch.float16, device='cuda')
    x3 = torch.ones(1, 3, 5, 1, device='cuda')
    with pytest.raises(SdodError):
        ops.ddim_inpaint_step(eps3, x3, COEF, 7.5)
    torch.cuda.synchronize()
    assert bool((x3 == 1.0).all())
    # and the same call with good arguments goes through
    ops.ddim_inpaint_step(eps, x, COEF, 7.5, z0=z0, keep=keep, known=KNOWN, noise=nu, stage=stage)
    assert not untouched()


# ------------------------------------------------------------------ the whole chain at latent 16
def _mask128():
    """a keep region (columns < 48: mask 0), a repaint region (columns >= 80: mask 255) and a soft edge between them that is not
    aligned to the 8 x 8 blocks (a linear ramp over 29 columns, shifted by the row), so keep takes 0, 1 and values between"""
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    ramp = ((xx - 50.0 - (yy % 3)) / 28.0).clamp(0.0, 1.0)
    m = (255.0 * ramp).round().to(torch.uint8)
    m[:, :48] = 0
    m[:, 80:] = 255
    return m[None]


@pytest.fixture(scope='module')
def rig16():
    """the rig16 recipe of test_img2img_gpu.py (synthetic weights, latent 16, injected noise) + a mask and per-step noise"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(16, 16)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'text': E.TextEncoder(cfg, 1).param_table(),
              'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, with_vae_encoder=True)
    with torch.device('meta'):
        unet, vae, enc = S.UNetModel(), S.AutoencoderKLDecode(), LdmEncoder()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    enc.load_state_dict(sds['vae_enc'], assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    img = torch.stack([128 + 90 * torch.sin(xx / 11 + k) * torch.cos(yy / 17) for k in range(3)], -1)
    u8 = (img + 10 * torch.randn(128, 128, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]
    n1 = torch.randn(1, 4, 16, 16, generator=g)
    n2 = torch.randn(1, 4, 16, 16, generator=g)
    step_noise = torch.randn(9, 1, 4, 16, 16, generator=g)             # strength 0.5, 20 steps: t_enc = 10, nine noise levels
    return dict(pipe=pipe, unet=unet.eval(), vae=vae.eval(), enc=enc.eval(), ctx2=ctx2, u8=u8, noise=(n1, n2), step_noise=step_noise,
                mask=_mask128())


STRENGTH, STEPS, GUIDANCE = 0.5, 20, 7.5


@torch.no_grad()
def _oracle_inpaint(unet, vae, enc, ctx2, u8, mask, noise, step_noise, strength, steps, guidance):
    """the definition in fp32 on the CPU: ldm scripts/img2img.py's start (encode_first_stage -> sample -> 0.18215 -> stochastic_encode),
    then per DDIM step (eta 0, CFG) the blend x = keep * q_sample(z0, timesteps[index - 1], nu) + (1 - keep) * x' -- z0 itself after
    the last step -- decode_first_stage -> 255 clamp((x + 1) / 2), and the integer pixel composite"""
    from oracle import pipeline_oracle as PO
    t_enc, seq, sa, s1a = ldm_img2img_indices(strength, steps)
    s = mask.reshape(mask.shape[0], mask.shape[1] // 8, 8, mask.shape[2] // 8, 8).to(torch.int64).sum(dim=(2, 4))
    keep = ((16320 - s).float() / 16320.0)[:, None]
    moments = enc((2.0 * (u8.float() / 255.0) - 1.0).half().float().permute(0, 3, 1, 2))
    mean, logvar = torch.chunk(moments, 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    z0 = 0.18215 * (mean + std * noise[0])
    x = sa * z0 + s1a * noise[1]
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
        if index >= 1:
            abar = ac[ddim_t[index - 1]]                                  # ldm q_sample at timesteps[index - 1]
            known = abar.sqrt() * z0 + (1. - abar).sqrt() * step_noise[index - 1]
        else:
            known = z0
        x = keep * known + (1. - keep) * x
    d = PO.decode_u8(vae, x, mode=1).astype(np.int64)
    k = mask.numpy().astype(np.int64)[..., None]
    comp = ((d * k + u8.numpy().astype(np.int64) * (255 - k) + 127) // 255).astype(np.uint8)
    return x, comp, seq, z0, keep


def test_inpaint_chain_matches_oracle_and_keeps_what_it_must(rig16):
    r = rig16
    pipe, ctx2, u8, mask = r['pipe'], r['ctx2'].cuda(), r['u8'], r['mask']
    z_ref, img_ref, seq, z0_ref, keep_ref = _oracle_inpaint(r['unet'], r['vae'], r['enc'], r['ctx2'], u8, mask, r['noise'], r['step_noise'],
                                                            STRENGTH, STEPS, GUIDANCE)
    from sdod.amd import ops
    from sdod.amd.pipeline import img2img_schedule
    _, t_enc = img2img_schedule(STRENGTH, STEPS)
    keep = ops.mask_to_latent(mask.cuda())
    assert torch.equal(keep.cpu(), keep_ref[:, 0])
    kc = keep.cpu()
    assert int((kc == 1).sum()) >= 64 and int((kc == 0).sum()) >= 64 and int(((kc > 0) & (kc < 1)).sum()) >= 32   # all three regions
    x, z0 = pipe.encode(u8, strength=STRENGTH, steps=STEPS, noise=r['noise'], return_z0=True)
    assert torch.equal(x, pipe.encode(u8, strength=STRENGTH, steps=STEPS, noise=r['noise']))      # encode() itself is unchanged
    trace = []
    z = pipe.sample_ddim_inpaint(ctx2, x, z0, keep, t_enc, STEPS, GUIDANCE, step_noise=r['step_noise'].cuda(), trace=trace)
    assert trace == seq                                               # timestep / index sequence: exact
    rl = rel_l2(z.cpu(), z_ref)
    print('inpaint final latent rel-L2', rl, '; z0 rel-L2', rel_l2(z0.cpu(), z0_ref))
    assert torch.isfinite(z).all() and rl <= 2e-2, rl
    trace2 = []
    img = pipe.inpaint(ctx2, u8, mask, STRENGTH, STEPS, GUIDANCE, noise=r['noise'], step_noise=r['step_noise'], trace=trace2)
    assert trace2 == seq
    assert torch.equal(img, ops.image_composite(_vae_img(pipe, z), u8.cuda(), mask.cuda()))
    img = img.cpu().numpy()
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 128, 3) and frac >= 0.99, frac
    # invariants: the kept latent region is z0 bit for bit, the kept pixels are the init image's bit for bit
    k4 = keep[:, None].expand_as(z)
    assert torch.equal(z[k4 == 1.0].view(torch.int32), z0[k4 == 1.0].view(torch.int32))
    assert not torch.equal(z[k4 < 1.0], z0[k4 < 1.0])
    m = mask.numpy()
    assert np.array_equal(img[m == 0], u8.numpy()[m == 0])
    plain = pipe.inpaint(ctx2, u8, mask, STRENGTH, STEPS, GUIDANCE, noise=r['noise'], step_noise=r['step_noise'], composite=False)
    assert torch.equal(plain, pipe.decode(z, mode=1))
    assert np.array_equal(img[m == 255], plain.cpu().numpy()[m == 255])


def _vae_img(pipe, z):
    pipe.vae.z.copy_(z)
    pipe.vae.execute(pipe.use_hip_graph)
    return pipe.vae.img


def test_inpaint_with_a_full_mask_is_img2img(rig16):
    """mask all 255: keep = 0 everywhere, 0 * known + 1 * x' is x' for finite known, and the fused step repeats cfg_combine +
    ddim_step, so the plain decode equals img2img() with the same arguments bit for bit -- injected and device noise"""
    r = rig16
    pipe, ctx2, u8 = r['pipe'], r['ctx2'].cuda(), r['u8']
    full = torch.full((1, 128, 128), 255, dtype=torch.uint8)
    a = pipe.inpaint(ctx2, u8, full, STRENGTH, STEPS, GUIDANCE, noise=r['noise'], step_noise=r['step_noise'], composite=False)
    b = pipe.img2img(ctx2, u8, STRENGTH, STEPS, GUIDANCE, noise=r['noise'])
    assert torch.equal(a, b)
    a2 = pipe.inpaint(ctx2, u8, full, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3, composite=False)
    b2 = pipe.img2img(ctx2, u8, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3)
    assert torch.equal(a2, b2) and not torch.equal(a2, a)
    # composite with k = 255 everywhere returns the decoded bytes
    assert torch.equal(pipe.inpaint(ctx2, u8, full, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3), b2)
    # and a mask of zeros returns the init image
    none = torch.zeros(1, 128, 128, dtype=torch.uint8)
    assert torch.equal(pipe.inpaint(ctx2, u8, none, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3).cpu(), u8)


def test_inpaint_graphed_equals_eager(rig16):
    r = rig16
    pipe, c, u8, mask = r['pipe'], r['ctx2'].cuda(), r['u8'], r['mask']
    eager = pipe.inpaint(c, u8, mask, STRENGTH, STEPS, GUIDANCE, noise=r['noise'], step_noise=r['step_noise'])
    graphed = pipe.inpaint_graphed(c, u8, mask, STRENGTH, STEPS, GUIDANCE, noise=r['noise'], step_noise=r['step_noise']).clone()
    assert torch.equal(graphed, eager)
    # device noise: the graph takes it as inputs drawn on the streams the eager path draws in its kernels
    eager2 = pipe.inpaint(c, u8, mask, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3)
    graphed2 = pipe.inpaint_graphed(c, u8, mask, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3).clone()
    assert torch.equal(graphed2, eager2)
    assert not torch.equal(graphed2, graphed)
    # the mask is an input of the graph: a replay with another mask of the same shape gives that mask's eager result
    other = mask.flip(2).contiguous()
    eager3 = pipe.inpaint(c, u8, other, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3)
    n_graphs = len(pipe._traj)
    graphed3 = pipe.inpaint_graphed(c, u8, other, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3).clone()
    assert len(pipe._traj) == n_graphs                                # a replay, not a new capture
    assert torch.equal(graphed3, eager3) and not torch.equal(graphed3, graphed2)
    # composite=False is a graph of its own and the plain decode
    plain = pipe.inpaint_graphed(c, u8, mask, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3, composite=False).clone()
    assert torch.equal(plain, pipe.inpaint(c, u8, mask, STRENGTH, STEPS, GUIDANCE, seed=31, image_index=3, composite=False))
    with pytest.raises(ValueError):
        pipe.inpaint_graphed(c, u8, mask[:, :64], STRENGTH, STEPS, GUIDANCE)
    with pytest.raises(ValueError):
        pipe.inpaint(c, u8, mask, 1.0, STEPS, GUIDANCE)


def test_img2img_is_untouched_by_inpainting(rig16):
    """img2img() after inpainting runs on the same pipeline: same result as before them, and graphed == eager still"""
    r = rig16
    pipe, c, u8 = r['pipe'], r['ctx2'].cuda(), r['u8']
    a = pipe.img2img(c, u8, STRENGTH, STEPS, GUIDANCE, noise=r['noise'])
    pipe.inpaint(c, u8, r['mask'], STRENGTH, STEPS, GUIDANCE, noise=r['noise'], step_noise=r['step_noise'])
    b = pipe.img2img(c, u8, STRENGTH, STEPS, GUIDANCE, noise=r['noise'])
    assert torch.equal(a, b)
    assert torch.equal(pipe.img2img_graphed(c, u8, STRENGTH, STEPS, GUIDANCE, noise=r['noise']), a)


# ------------------------------------------------------------------ the product size: the kernels at their real grids
def test_inpaint_product_size_graphed_equals_eager():
    """latent 64 (512 x 512 image), n = 1, three steps (strength 0.75 of 4): inpaint_graphed against inpaint, device noise"""
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, with_vae_encoder=True)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    u8 = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(512.), torch.arange(512.), indexing='ij')
    mask = (255.0 * ((xx + 0.5 * yy - 250.0) / 100.0).clamp(0.0, 1.0)).round().to(torch.uint8)[None]
    trace = []
    eager = pipe.inpaint(ctx2, u8, mask, 0.75, 4, 7.5, seed=11, image_index=2, trace=trace)
    assert [i for _, i in trace] == [2, 1, 0]
    graphed = pipe.inpaint_graphed(ctx2, u8, mask, 0.75, 4, 7.5, seed=11, image_index=2).clone()
    assert eager.shape == (1, 512, 512, 3) and torch.equal(graphed, eager)
    m = mask.numpy()
    assert (m == 0).any() and (m == 255).any()
    assert np.array_equal(eager.cpu().numpy()[m == 0], u8.numpy()[m == 0])
    full = torch.full_like(mask, 255)
    assert torch.equal(pipe.inpaint(ctx2, u8, full, 0.75, 4, 7.5, seed=11, image_index=2, composite=False),
                       pipe.img2img(ctx2, u8, 0.75, 4, 7.5, seed=11, image_index=2))
