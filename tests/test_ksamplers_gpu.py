"""The k-diffusion samplers (Euler, Euler ancestral, DPM++ 2M; discrete and Karras schedules) on the GPU.

Bit for bit: the fused step sdod_k_step against the launches it replaces (cfg_combine -> lincomb4 -> lincomb4 -> one fp32 multiply ->
stage_unet_inputs), its in-kernel noise against sdod_randn_f32, graphed against eager, euler_a at eta = 0 against euler, img2img against
its parts, and 'plms' with the new keywords at their defaults against the call without them.

Against fp64: a point-mass trajectory without a UNet (eps = fp16((x - z) / sigma), whose exact solution is z), bound 2e-5 absolute on the
final latent = 4 x the 4.9e-6 that numpy fp32 in the kernel's operation order stays within over the six sampler x schedule combinations.

Against an fp32 CPU restatement in k-diffusion's operation order (x * c_in, fractional t, CFG mode 1) at latent 16 with synthetic
weights: the project's chain tolerance, final latent rel-L2 <= 2e-2 and >= 99 % of the uint8 pixels within 2 LSB."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_SAMPLERS = ('euler', 'euler_a', 'dpmpp_2m')


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------ the fused step against the separate launches
SIGMA = 4.4998425189583315
EPS_DEN = (1.0, -SIGMA)
V_DEN = (1.0 / (SIGMA * SIGMA + 1.0), -SIGMA / (SIGMA * SIGMA + 1.0) ** 0.5)
STEP_CASES = {                                  # (a, b, cprev, u)
    'euler': (0.7699723632996166, 0.2300276367003834, 0.0, 0.0),
    'ancestral_injected': (0.5930, 0.4070, 0.0, 2.1903),
    'ancestral_device': (0.5930, 0.4070, 0.0, 2.1903),
    'second_order': (0.7699723632996166, 0.3493368915874824, -0.11930925488709897, 0.0),
    'last': (0.0, 1.0, 0.0, 0.0),
    'start': (14.614641489691584, 0.0, 0.0, 0.0),
}
STAGE_SCALE = 0.27730186345778407
TEMB_W = 520


def _step_inputs(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(2 * n, h, w, c, generator=g).half().cuda()
    x = (3.0 * torch.randn(n, c, h, w, generator=g)).cuda()
    den_prev = torch.randn(n, c, h, w, generator=g).cuda()
    nu = torch.randn(n, c, h, w, generator=g).cuda()
    temb_row = torch.randn(TEMB_W, generator=g).half().cuda()
    return eps, x, den_prev, nu, temb_row


def _coef(case, v_pred):
    a, b, cprev, u = STEP_CASES[case]
    d0, d1 = V_DEN if v_pred else EPS_DEN
    return dict(d0=d0, d1=d1, a=a, b=b, cprev=cprev, u=u, stage_scale=STAGE_SCALE)


def _composed(eps, x, coef, den_prev, nu, guidance, stage):
    """the separate launches: returns (x', den); stage = (x_dst, temb_row, temb_dst) receives stage_scale * x' and the time row"""
    from sdod.amd import ops
    if eps is None:
        den = None
        xn = ops.lincomb4([x], [coef['a']], 1.0)
    else:
        e = ops.cfg_combine(eps, guidance, uncond_first=True, mode=1)
        den = ops.lincomb4([x, e], [coef['d0'], coef['d1']], 1.0)
        terms, cs = [x, den], [coef['a'], coef['b']]
        if coef['cprev'] != 0.0:
            terms.append(den_prev); cs.append(coef['cprev'])
        if coef['u'] != 0.0:
            terms.append(nu); cs.append(coef['u'])
        xn = ops.lincomb4(terms, cs, 1.0)
    if stage is not None:
        scaled = xn * torch.tensor(np.float32(coef['stage_scale']), device=xn.device)     # one fp32 multiply
        assert scaled.dtype == torch.float32
        ops.stage_unet_inputs(scaled, stage[0], stage[1], stage[2])
    return xn, den


@pytest.mark.parametrize('shape', [(2, 4, 16, 24), (2, 4, 10, 13), (1, 4, 64, 64), (3, 4, 5, 7)])
@pytest.mark.parametrize('v_pred', [False, True])
@pytest.mark.parametrize('staged', [False, True])
@pytest.mark.parametrize('case', list(STEP_CASES))
def test_k_step_equals_the_composition(shape, v_pred, staged, case):
    """(2, 4, 10, 13) and (3, 4, 5, 7): hw % 4 != 0, so a thread's four elements straddle channels, and the element count is not a
    multiple of a block's span (1024)"""
    from sdod.amd import ops
    n, c, h, w = shape
    eps, x, den_prev, nu, temb_row = _step_inputs(n, c, h, w, seed=h * 31 + w)
    guidance, seed, level, idx0 = 7.5, 987654321, 4, 5
    coef = _coef(case, v_pred)
    start = case == 'start'
    with_prev = case in ('second_order', 'last')          # DPM++ 2M keeps den_prev through its last step, where cprev == 0

    def stage():
        return (torch.full((2 * n, c, h, w), -3.0, device='cuda'), temb_row, torch.zeros(2 * n, TEMB_W, dtype=torch.float16, device='cuda')) \
            if staged else None

    if case == 'ancestral_device':   # in-kernel noise == sdod_randn_f32 on stream ((3 + level) << 32) | (image_index + i)
        nu = torch.cat([ops.randn((1, c, h, w), seed, ((3 + level) << 32) | (idx0 + i), 'cuda') for i in range(n)])
    s_ref, s_got = stage(), stage()
    want, den = _composed(None if start else eps, x, coef, den_prev, nu, guidance, s_ref)
    got, dp = x.clone(), den_prev.clone()
    kw = dict(den_prev=dp if with_prev else None, noise=nu if case == 'ancestral_injected' else None, seed=seed, noise_level=level,
              image_index=idx0, mode=1, stage=s_got)
    ops.k_step(None if start else eps, got, coef, guidance, **kw)
    assert torch.equal(bits(got), bits(want))
    if with_prev:
        assert torch.equal(bits(dp), bits(den))
    if staged:
        assert torch.equal(bits(s_got[0]), bits(s_ref[0])) and torch.equal(s_got[2], s_ref[2])
        assert torch.equal(s_got[2], temb_row[None].expand(2 * n, -1))
        assert torch.equal(bits(s_got[0][:n]), bits(got * torch.tensor(np.float32(STAGE_SCALE), device='cuda')))
    if case == 'last':               # x' = den
        assert torch.equal(got, den)
    if coef['u'] == 0.0:             # nothing is drawn or read: NaNs in `noise` change nothing
        again, dp2 = x.clone(), den_prev.clone()
        ops.k_step(None if start else eps, again, coef, guidance, **dict(kw, den_prev=dp2 if with_prev else None,
                                                                         noise=torch.full_like(x, float('nan')), stage=None))
        assert torch.equal(bits(again), bits(got))
    else:
        assert not torch.equal(got, _composed(eps, x, dict(coef, u=0.0), den_prev, nu, guidance, None)[0])
    if case == 'second_order':       # and the history matters
        assert not torch.equal(got, _composed(eps, x, dict(coef, cprev=0.0), den_prev, nu, guidance, None)[0])


def test_k_step_device_noise_depends_on_level_seed_and_index():
    from sdod.amd import ops
    eps, x, _, _, _ = _step_inputs(2, 4, 16, 16, seed=3)
    coef = _coef('ancestral_device', False)
    outs = []
    for seed, level, idx0 in ((1, 0, 0), (2, 0, 0), (1, 1, 0), (1, 0, 1)):
        got = x.clone()
        ops.k_step(eps, got, coef, 7.5, seed=seed, noise_level=level, image_index=idx0)
        outs.append(got)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(outs[a], outs[b])
    # image 1 at image_index 0 draws the stream of image 0 at image_index 1
    inj = torch.cat([ops.randn((1, 4, 16, 16), 1, (3 << 32) | 0, 'cuda'), ops.randn((1, 4, 16, 16), 1, (3 << 32) | 1, 'cuda')])
    b = x.clone()
    ops.k_step(eps, b, coef, 7.5, noise=inj)
    assert torch.equal(outs[0], b)
    # the same two images one index apart: image 0 at index 1 has image 1's noise at index 0 (identical eps and x for both images)
    eps1 = torch.cat([eps[0:1], eps[0:1], eps[2:3], eps[2:3]])
    x1 = torch.cat([x[0:1], x[0:1]])
    at0, at1 = x1.clone(), x1.clone()
    ops.k_step(eps1, at0, coef, 7.5, seed=1, noise_level=2, image_index=0)
    ops.k_step(eps1, at1, coef, 7.5, seed=1, noise_level=2, image_index=1)
    assert torch.equal(at0[1], at1[0]) and not torch.equal(at0[0], at1[0])


def test_k_step_refuses_bad_arguments_and_leaves_outputs_untouched():
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    n, c, h, w = 2, 4, 16, 16
    eps, x, den_prev, nu, temb_row = _step_inputs(n, c, h, w, seed=9)
    x_dst = torch.full((2 * n, c, h, w), -3.0, device='cuda')
    temb_dst = torch.zeros(2 * n, TEMB_W, dtype=torch.float16, device='cuda')
    x0, dp0 = x.clone(), den_prev.clone()
    stage = (x_dst, temb_row, temb_dst)
    good = _coef('second_order', False)
    anc = _coef('ancestral_injected', False)

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(bits(x), bits(x0)) and torch.equal(bits(den_prev), bits(dp0)) and bool((x_dst == -3.0).all()) and \
            bool((temb_dst == 0).all())

    def refused(*args, **kw):
        with pytest.raises(SdodError):
            ops.k_step(*args, **kw)
        assert untouched()

    refused(eps, x, good, 7.5, den_prev=den_prev, mode=2, stage=stage)                              # a mode that does not exist
    refused(eps, x, good, 7.5, den_prev=None, stage=stage)                                          # cprev != 0 without den_prev
    big = torch.zeros(n * c * h * w + 4, device='cuda')
    off = big[1:1 + n * c * h * w].view(n, c, h, w)
    refused(eps, x, anc, 7.5, den_prev=den_prev, noise=off, stage=stage)                            # noise not 16-byte aligned
    refused(eps, x, good, 7.5, den_prev=off, stage=stage)                                           # den_prev not 16-byte aligned
    assert bool((big == 0).all())
    refused(eps, off, _coef('euler', False), 7.5, stage=stage)                                      # x not 16-byte aligned
    assert bool((big == 0).all())
    sbig = torch.full((2 * n * c * h * w + 4,), -3.0, device='cuda')
    refused(eps, x, good, 7.5, den_prev=den_prev, stage=(sbig[1:1 + 2 * n * c * h * w], temb_row, temb_dst))   # x_stage misaligned
    assert bool((sbig == -3.0).all())
    for key in ('d0', 'd1', 'a', 'b', 'cprev', 'u', 'stage_scale'):                                 # a non-finite scalar
        for bad in (float('nan'), float('inf'), -float('inf')):
            refused(eps, x, dict(good, **{key: bad}), 7.5, den_prev=den_prev, noise=nu, stage=stage)
    refused(eps, x, good, float('nan'), den_prev=den_prev, stage=stage)                             # guidance is one of them
    for key in ('b', 'cprev', 'u'):                                                                 # the start form takes a alone
        refused(None, x, dict(_coef('start', False), **{key: 0.5}), den_prev=den_prev, noise=nu, stage=stage)
    # c * hw not a multiple of 4
    eps3 = torch.zeros(2, 5, 1, 3, dtype=torch.float16, device='cuda')
    x3 = torch.ones(1, 3, 5, 1, device='cuda')
    with pytest.raises(SdodError):
        ops.k_step(eps3, x3, _coef('euler', False), 7.5)
    with pytest.raises(SdodError):
        ops.k_step(None, x3, _coef('start', False))
    torch.cuda.synchronize()
    assert bool((x3 == 1.0).all()) and untouched()
    # and the same call with good arguments goes through
    ops.k_step(eps, x, good, 7.5, den_prev=den_prev, stage=stage)
    torch.cuda.synchronize()
    assert not torch.equal(x, x0) and not torch.equal(den_prev, dp0) and not bool((x_dst == -3.0).any()) and bool((temb_dst == temb_row).all())


# ------------------------------------------------------------------ a trajectory without a UNet: eps of a point mass at z
@pytest.mark.parametrize('schedule', ['discrete', 'karras'])
@pytest.mark.parametrize('sampler', K_SAMPLERS)
def test_point_mass_trajectory_matches_fp64(sampler, schedule):
    """the data distribution is the single point z: eps(x, sigma) = (x - z) / sigma, every sampler's exact answer is z.  The GPU runs
    ops.k_step on eps rounded to fp16 (what a UNet would hand it); the reference is the same linear form in fp64, with the fp64
    coefficients, fed the same fp16 eps and noise."""
    from sdod.amd import ops
    from sdod.amd.samplers import KSchedule
    n, c, h, w = 2, 4, 10, 13
    steps = 10
    k = KSchedule(steps, schedule)
    g = torch.Generator().manual_seed(2024)
    z = (0.8 * torch.randn(n, c, h, w, generator=g)).cuda()
    x_T = torch.randn(n, c, h, w, generator=g)
    noise = torch.randn(steps - 1, n, c, h, w, generator=g).cuda()
    x = x_T.cuda()
    den_prev = torch.empty_like(x) if sampler == 'dpmpp_2m' else None
    ops.k_step(None, x, dict(a=float(k.sigmas[0])))
    ref = x.double().cpu().numpy()                                  # the start product is one fp32 rounding of fp32 inputs: shared
    ref_prev = np.zeros_like(ref)
    eps_max = 0.0
    for i in range(steps):
        cf = k.coef(sampler, i)
        e16 = ((x - z) / float(k.sigmas[i])).half()                 # [n, c, h, w]
        eps = torch.cat([e16, e16]).permute(0, 2, 3, 1).contiguous()    # both guidance halves, NHWC
        nu = noise[i] if cf['u'] != 0.0 else None
        ops.k_step(eps, x, cf, 7.5, den_prev=den_prev, noise=nu, mode=1)
        e = e16.double().cpu().numpy()
        eps_max = float(np.abs(e).max())
        den = cf['d0'] * ref + cf['d1'] * e
        nxt = cf['a'] * ref + cf['b'] * den
        if cf['cprev'] != 0.0:
            nxt = nxt + cf['cprev'] * ref_prev
        if cf['u'] != 0.0:
            nxt = nxt + cf['u'] * nu.double().cpu().numpy()
        ref_prev, ref = den, nxt
    got = x.double().cpu().numpy()
    err = float(np.abs(got - ref).max())
    off = float(np.abs(got - z.double().cpu().numpy()).max())
    bound = float(k.sigmas[steps - 1]) * eps_max * 2.0 ** -11 + 2e-5
    print(f'point mass {sampler} {schedule}: |gpu - fp64| max {err:.3e} (bound 2e-5); |gpu - z| max {off:.3e} (bound {bound:.3e})')
    assert np.isfinite(got).all()
    assert err <= 2e-5, err
    assert off <= bound, (off, bound)


# ------------------------------------------------------------------ the whole chain at latent 16
@pytest.fixture(scope='module')
def rig16():
    """the rig16 recipe of test_inpaint_gpu.py: synthetic weights, latent 16, the CPU models of oracle.sd_torch on the same weights"""
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
        unet, vae = S.UNetModel(), S.AutoencoderKLDecode()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    img = torch.stack([128 + 90 * torch.sin(xx / 11 + k) * torch.cos(yy / 17) for k in range(3)], -1)
    u8 = (img + 10 * torch.randn(128, 128, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]
    n1 = torch.randn(1, 4, 16, 16, generator=g)
    n2 = torch.randn(1, 4, 16, 16, generator=g)
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    step_noise = torch.randn(7, 1, 4, 16, 16, generator=g)              # 8 steps: seven fresh draws
    return dict(pipe=pipe, unet=unet.eval(), vae=vae.eval(), ctx2=ctx2, u8=u8, noise=(n1, n2), x_T=x_T, step_noise=step_noise)


def _karras_sigmas_and_times(steps, rho=7.0):
    """k-diffusion's get_sigmas_karras between the ends of its DiscreteSchedule, and DiscreteSchedule.sigma_to_t, restated with torch in
    float64 from the oracle's alphas_cumprod (independent of sdod.amd.samplers).  ldm keeps alphas_cumprod as a float32 buffer and
    k-diffusion's CompVisDenoiser builds its sigma table from that buffer, so the table starts from the float32 values here too (as
    pipeline_oracle.plms_sample takes them)"""
    from oracle import pipeline_oracle as PO
    ac = torch.from_numpy(PO._alphas_cumprod()).to(torch.float32).double()
    table = ((1 - ac) / ac) ** 0.5
    log_sigmas = table.log()
    ramp = torch.linspace(0, 1, steps, dtype=torch.float64)
    lo, hi = table[0] ** (1 / rho), table[-1] ** (1 / rho)
    sigmas = torch.cat([(hi + ramp * (lo - hi)) ** rho, torch.zeros(1, dtype=torch.float64)])
    log_sigma = sigmas[:-1].log()
    dists = log_sigma - log_sigmas[:, None]
    low_idx = dists.ge(0).cumsum(dim=0).argmax(dim=0).clamp(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    wgt = ((low - log_sigma) / (low - high)).clamp(0, 1)
    t = (1 - wgt) * low_idx + wgt * high_idx
    return sigmas, t


@torch.no_grad()
def _oracle_k(unet, vae, ctx2, x_T, sampler, steps, guidance, step_noise, eta=1.0):
    """fp32 on the CPU, k-diffusion's operation order: x = sigma_0 x_T; per step the model sees x * c_in at the fractional time
    sigma_to_t(sigma), CFG mode 1 on its output, denoised = x + eps * (-sigma), then sample_euler_ancestral / sample_dpmpp_2m"""
    from oracle import pipeline_oracle as PO
    sig64, t64 = _karras_sigmas_and_times(steps)
    sigmas, times = sig64.float(), t64.float()
    c16 = ctx2.float()
    x = x_T * sigmas[0]
    old_denoised = None
    for i in range(steps):
        s, s_next = sigmas[i], sigmas[i + 1]
        c_in = 1 / (s ** 2 + 1) ** 0.5
        e_u, e_c = PO.guided_eps(unet, x * c_in, times[i].reshape(1).expand(x.shape[0]), c16[0:1], c16[1:2], guidance)
        eps = e_u + guidance * (e_c - e_u)
        denoised = x + eps * (-s)
        if sampler == 'euler_a':
            sigma_up = min(float(s_next), eta * float((s_next ** 2 * (s ** 2 - s_next ** 2) / s ** 2) ** 0.5))
            sigma_down = float((s_next ** 2 - sigma_up ** 2) ** 0.5)
            d = (x - denoised) / s
            x = x + d * (sigma_down - s)
            if s_next > 0:
                x = x + step_noise[i] * sigma_up
        else:
            if s_next == 0:
                x = denoised
            else:
                t, t_next = -s.log(), -s_next.log()
                h = t_next - t
                if old_denoised is None:
                    x = (s_next / s) * x - (-h).expm1() * denoised
                else:
                    h_last = t - (-sigmas[i - 1].log())
                    r = h_last / h
                    denoised_d = (1 + 1 / (2 * r)) * denoised - (1 / (2 * r)) * old_denoised
                    x = (s_next / s) * x - (-h).expm1() * denoised_d
            old_denoised = denoised
    return x, PO.decode_u8(vae, x, mode=1)


@pytest.mark.parametrize('sampler', ['euler_a', 'dpmpp_2m'])
def test_k_chain_matches_the_restatement(rig16, sampler):
    """8 steps on the Karras schedule, latent 16, euler_a with injected step noise.  Tolerance: the chain tolerance of
    test_pipeline_gpu.py / test_img2img_gpu.py / test_inpaint_gpu.py, final latent rel-L2 <= 2e-2 and >= 99 % of the uint8 pixels within
    2 LSB.  The restatement itself moves by rel-L2 8e-4 (euler_a) / 7e-4 (dpmpp_2m), every pixel within 1 LSB, when its model input and
    output are rounded to fp16 and the output is perturbed by 1e-3 relative (CPU, fp32): the chain is well conditioned at sigma 14.6.
    Values on MI355X: not recorded yet (the test prints them)."""
    from sdod.amd.samplers import KSchedule
    r = rig16
    pipe, ctx2 = r['pipe'], r['ctx2'].cuda()
    sn = r['step_noise'] if sampler == 'euler_a' else None
    z_ref, img_ref = _oracle_k(r['unet'], r['vae'], r['ctx2'], r['x_T'], sampler, 8, 7.5, sn)
    # the host schedule against the restatement's own: the same float32 alphas_cumprod, the same formulas, float64 in numpy here and
    # in torch there.  A few ulp (1e-16) of log / exp / pow, raised to rho = 7 and, in sigma_to_t, divided by the table's smallest
    # log-sigma spacing (3.3e-3): 1e-9 holds with three decimal orders to spare
    sig64, t64 = _karras_sigmas_and_times(8)
    k = KSchedule(8, 'karras')
    assert np.allclose(k.sigmas, sig64.numpy(), rtol=1e-9, atol=0) and np.allclose(k.times, t64.numpy(), rtol=1e-9, atol=1e-9)
    z = pipe.sample_k(ctx2, r['x_T'], sampler, 8, 7.5, 'karras', step_noise=sn)
    rl = rel_l2(z.cpu(), z_ref)
    print(f'k chain {sampler} karras: final latent rel-L2', rl)
    assert torch.isfinite(z).all() and rl <= 2e-2, rl
    img = pipe.generate(ctx2, r['x_T'], 8, 7.5, sampler, schedule='karras', step_noise=sn)
    assert torch.equal(img, pipe.decode(z, mode=1))
    img = img.cpu().numpy()
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print(f'k chain {sampler} karras: uint8 image max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 128, 3) and frac >= 0.99, frac


# ------------------------------------------------------------------ equalities, bit for bit
@pytest.mark.parametrize('sampler', K_SAMPLERS)
def test_generate_graphed_equals_eager(rig16, sampler):
    r = rig16
    pipe, c, x_T = r['pipe'], r['ctx2'].cuda(), r['x_T']
    kw = dict(schedule='karras')
    if sampler == 'euler_a':         # injected noise
        eager = pipe.generate(c, x_T, 8, 7.5, sampler, step_noise=r['step_noise'], **kw)
        graphed = pipe.generate_graphed(c, x_T, 8, 7.5, sampler, step_noise=r['step_noise'], **kw).clone()
        assert torch.equal(graphed, eager)
    # device noise (euler_a; the others draw none and the seed plays no part)
    eager1 = pipe.generate(c, x_T, 8, 7.5, sampler, seed=31, image_index=3, **kw)
    n_before = len(pipe._traj or {})
    graphed1 = pipe.generate_graphed(c, x_T, 8, 7.5, sampler, seed=31, image_index=3, **kw).clone()
    assert torch.equal(graphed1, eager1)
    n_graphs = len(pipe._traj)
    assert n_graphs == n_before + (0 if sampler == 'euler_a' else 1)      # euler_a: the injected-noise call above captured it
    # a second replay with another seed: that seed's eager result -- the graph bakes no seed
    eager2 = pipe.generate(c, x_T, 8, 7.5, sampler, seed=32, image_index=3, **kw)
    graphed2 = pipe.generate_graphed(c, x_T, 8, 7.5, sampler, seed=32, image_index=3, **kw).clone()
    assert len(pipe._traj) == n_graphs                                    # a replay, not a new capture
    assert torch.equal(graphed2, eager2)
    assert torch.equal(graphed2, graphed1) == (sampler != 'euler_a')
    if sampler == 'euler_a':
        assert not torch.equal(graphed1, graphed)
        # the image index shifts the stream as the seed does
        assert not torch.equal(pipe.generate(c, x_T, 8, 7.5, sampler, seed=31, image_index=4, **kw), eager1)
    # the discrete schedule is another trajectory and another graph
    d = pipe.generate_graphed(c, x_T, 8, 7.5, sampler, seed=31, image_index=3).clone()
    assert len(pipe._traj) == n_graphs + 1
    assert torch.equal(d, pipe.generate(c, x_T, 8, 7.5, sampler, seed=31, image_index=3)) and not torch.equal(d, graphed1)


def test_euler_a_with_eta_zero_is_euler(rig16):
    r = rig16
    pipe, c, x_T = r['pipe'], r['ctx2'].cuda(), r['x_T']
    for schedule in ('discrete', 'karras'):
        e = pipe.generate(c, x_T, 6, 7.5, 'euler', schedule=schedule)
        assert torch.equal(pipe.generate(c, x_T, 6, 7.5, 'euler_a', schedule=schedule, eta=0.0, seed=5), e)
        assert torch.equal(pipe.generate(c, x_T, 6, 7.5, 'euler_a', schedule=schedule, eta=0.0,
                                         step_noise=torch.full((5, 1, 4, 16, 16), float('nan'))), e)
        assert not torch.equal(pipe.generate(c, x_T, 6, 7.5, 'euler_a', schedule=schedule, seed=5), e)
    assert torch.equal(pipe.generate_graphed(c, x_T, 6, 7.5, 'euler_a', eta=0.0, seed=9), pipe.generate(c, x_T, 6, 7.5, 'euler'))


def test_img2img_with_a_k_sampler_is_its_parts(rig16):
    from sdod.amd.samplers import KSchedule
    r = rig16
    pipe, c, u8 = r['pipe'], r['ctx2'].cuda(), r['u8']
    strength, steps = 0.5, 12
    t_enc = int(strength * steps)
    first = steps - t_enc
    sn = r['step_noise'][:t_enc - 1]
    sig = float(KSchedule(steps, 'karras').sigmas[first])
    # the start latent: z0 + sigmas[first] * n2, from sdod_encode_latent_f32 with the coefficients (1, sigmas[first])
    x, z0 = pipe.encode(u8, strength=strength, steps=steps, noise=r['noise'], return_z0=True, coef=(1.0, sig))
    # (each of the two roundings there -- the product, the sum; or one, if the compiler fuses them -- is within half an ulp of its result)
    prod = float(np.float32(sig)) * r['noise'][1].double()               # the kernel takes the coefficient as fp32
    assert bool(((x.cpu().double() - (z0.cpu().double() + prod)).abs() <= 2.0 ** -24 * (prod.abs() + x.cpu().double().abs())).all())
    z = pipe.sample_k(c, x, 'euler_a', steps, 7.5, 'karras', first=first, step_noise=sn)
    want = pipe.decode(z, mode=1)
    got = pipe.img2img(c, u8, strength, steps, 7.5, noise=r['noise'], sampler='euler_a', schedule='karras', step_noise=sn)
    assert torch.equal(got, want)
    graphed = pipe.img2img_graphed(c, u8, strength, steps, 7.5, noise=r['noise'], sampler='euler_a', schedule='karras', step_noise=sn).clone()
    assert torch.equal(graphed, got)
    # device noise, everywhere: the encoder's two streams and the steps' own
    x2 = pipe.encode(u8, 31, 3, strength, steps, coef=(1.0, sig))
    want2 = pipe.decode(pipe.sample_k(c, x2, 'euler_a', steps, 7.5, 'karras', first=first, seed=31, image_index=3), mode=1)
    got2 = pipe.img2img(c, u8, strength, steps, 7.5, seed=31, image_index=3, sampler='euler_a', schedule='karras')
    assert torch.equal(got2, want2) and not torch.equal(got2, got)
    n_graphs = len(pipe._traj)
    graphed2 = pipe.img2img_graphed(c, u8, strength, steps, 7.5, seed=31, image_index=3, sampler='euler_a', schedule='karras').clone()
    assert len(pipe._traj) == n_graphs and torch.equal(graphed2, got2)
    # the other two samplers, graphed against eager; DPM++ 2M starts first-order at `first`
    for sampler in ('euler', 'dpmpp_2m'):
        e = pipe.img2img(c, u8, strength, steps, 7.5, noise=r['noise'], sampler=sampler, schedule='karras')
        assert torch.equal(pipe.img2img_graphed(c, u8, strength, steps, 7.5, noise=r['noise'], sampler=sampler, schedule='karras'), e)
        assert not torch.equal(e, got)
    # and ldm's DDIM path is what it was: sampler=None is the call without the keyword
    a = pipe.img2img(c, u8, strength, steps, 7.5, noise=r['noise'])
    assert torch.equal(pipe.img2img(c, u8, strength, steps, 7.5, noise=r['noise'], sampler=None, schedule='discrete', eta=1.0, step_noise=None), a)
    assert torch.equal(pipe.img2img_graphed(c, u8, strength, steps, 7.5, noise=r['noise']), a)
    assert torch.equal(pipe.encode(u8, strength=strength, steps=steps, noise=r['noise'], coef=None),
                       pipe.encode(u8, strength=strength, steps=steps, noise=r['noise']))


def test_old_samplers_are_untouched_by_the_new_keywords(rig16):
    r = rig16
    pipe, c, x_T = r['pipe'], r['ctx2'].cuda(), r['x_T']
    for sampler, steps in (('plms', 4), ('dpm', 3)):
        a = pipe.generate(c, x_T, steps, 7.5, sampler)
        assert torch.equal(pipe.generate(c, x_T, steps, 7.5, sampler, schedule='discrete', eta=1.0, seed=0, image_index=0, step_noise=None), a)
        assert torch.equal(pipe.generate(c, x_T, steps, 7.5, sampler, seed=77, image_index=5), a)      # they draw nothing
        assert torch.equal(pipe.generate_graphed(c, x_T, steps, 7.5, sampler), a)
        assert torch.equal(pipe.decode(pipe._sample(sampler, c, x_T, steps, 7.5), mode=1 if sampler == 'plms' else 0), a)
        with pytest.raises(ValueError):
            pipe.generate(c, x_T, steps, 7.5, sampler, schedule='karras')
    with pytest.raises(ValueError):
        pipe.generate_pipelined(c, x_T, 4, 7.5, 'euler')
