"""The LCM kernels on the GPU.

sdod_lcm_step, bit for bit against the launches it replaces (cfg_combine or nhwc_f16_to_nchw_f32 -> lincomb4 -> lincomb4 ->
stage_unet_inputs), its in-kernel noise against sdod_randn_f32.

sdod_guidance_features_f16 against samplers.guidance_embedding (fp64), per element within 4 * 2^-24 * |arg| + 2^-11 with arg =
(w - 1) * 1000 * f_j: four fp32 roundings on the way to the argument (f_j, v, the product, the exp's own error) and fp16's half-ulp
below 1.  At the worst argument (14 000 rad) that is 3.9e-3: a sine without range reduction, wrong by order 1, cannot pass.

The TEMB graph with cond_proj against the fp32 CPU restatement (tests/lcm_ref.py) on the same fp16 weights, at the tolerance
tests/test_engine_gpu.py asks of the plain TEMB graph (rel-L2 5e-3); a zero cond_proj gives the plain graph's bits."""
import numpy as np
import pytest
import torch

import lcm_ref as R

pytestmark = pytest.mark.gpu

TEMB_W = 520


def bits(t):
    return t.view(torch.int32)


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------ the fused step against the separate launches
def _coef(case, v_pred):
    from sdod.amd.samplers import LcmSchedule
    sch = LcmSchedule(4)
    if case == 'last':
        return sch.coef(3, v_pred)
    cf = sch.coef(1, v_pred)             # a middle step: 759 -> 499
    if case == 'a_zero':
        return dict(cf, a=0.0)
    if case == 'a_zero_last':
        return dict(cf, a=0.0, u=0.0)
    if case == 'a_large':                # (the schedule's own a = sqrt(abar') c_skip is 1e-9: the x term is below an ulp of b den)
        return dict(cf, a=0.3)
    return cf


STEP_CASES = ('middle_injected', 'middle_device', 'last', 'a_zero', 'a_zero_last', 'a_large')


def _step_inputs(n, c, h, w, guided, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((2 * n if guided else n), h, w, c, generator=g).half().cuda()
    x = (1.5 * torch.randn(n, c, h, w, generator=g)).cuda()
    nu = torch.randn(n, c, h, w, generator=g).cuda()
    temb_row = torch.randn(TEMB_W, generator=g).half().cuda()
    return eps, x, nu, temb_row


def _composed(eps, x, coef, nu, guidance, stage):
    """the separate launches: returns (x', den); stage = (x_dst, temb_row, temb_dst) receives x' unscaled and the time row"""
    from sdod.amd import ops
    e = ops.nhwc_f16_to_nchw_f32(eps) if guidance is None else ops.cfg_combine(eps, guidance, uncond_first=True, mode=1)
    den = ops.lincomb4([x, e], [coef['d0'], coef['d1']], 1.0)
    terms, cs = ([x, den], [coef['a'], coef['b']]) if coef['a'] != 0.0 else ([den], [coef['b']])
    if coef['u'] != 0.0:
        terms.append(nu); cs.append(coef['u'])
    xn = ops.lincomb4(terms, cs, 1.0)
    if stage is not None:
        ops.stage_unet_inputs(xn, stage[0], stage[1], stage[2])
    return xn, den


@pytest.mark.parametrize('shape', [(2, 4, 16, 24), (2, 4, 10, 13), (3, 4, 5, 7), (1, 4, 64, 64)])
@pytest.mark.parametrize('guided', [True, False])
@pytest.mark.parametrize('v_pred', [False, True])
@pytest.mark.parametrize('staged', [False, True])
@pytest.mark.parametrize('case', STEP_CASES)
def test_lcm_step_equals_the_composition(shape, guided, v_pred, staged, case):
    """(2, 4, 10, 13) and (3, 4, 5, 7): hw % 4 != 0, so a thread's four elements straddle channels, and the element count is not a
    multiple of a block's span (1024)"""
    from sdod.amd import ops
    n, c, h, w = shape
    eps, x, nu, temb_row = _step_inputs(n, c, h, w, guided, seed=h * 31 + w)
    guidance = 1.5 if guided else None
    seed, level, idx0 = 987654321, 2, 5
    coef = _coef(case, v_pred)
    rows = 2 * n if guided else n

    def stage():
        return (torch.full((rows, c, h, w), -3.0, device='cuda'), temb_row, torch.zeros(rows, TEMB_W, dtype=torch.float16, device='cuda')) \
            if staged else None

    if case == 'middle_device':      # in-kernel noise == sdod_randn_f32 on stream ((3 + level) << 32) | (image_index + i)
        nu = torch.cat([ops.randn((1, c, h, w), seed, ((3 + level) << 32) | (idx0 + i), 'cuda') for i in range(n)])
    s_ref, s_got = stage(), stage()
    want, den = _composed(eps, x, coef, nu, guidance, s_ref)
    got, den_out = x.clone(), torch.full_like(x, 7.0)
    kw = dict(den_out=den_out, noise=None if case == 'middle_device' else nu, seed=seed, noise_level=level, image_index=idx0, mode=1, stage=s_got)
    ops.lcm_step(eps, got, coef, guidance, **kw)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(den_out), bits(den))
    if staged:
        assert torch.equal(bits(s_got[0]), bits(s_ref[0])) and torch.equal(s_got[2], s_ref[2])
        assert torch.equal(s_got[2], temb_row[None].expand(rows, -1))
        for r in range(rows // n):           # x' itself, unscaled, in every copy
            assert torch.equal(bits(s_got[0][r * n:(r + 1) * n]), bits(got))
    if coef['u'] == 0.0:             # nothing is drawn or read: NaNs in `noise` change nothing
        again = x.clone()
        ops.lcm_step(eps, again, coef, guidance, **dict(kw, den_out=None, noise=torch.full_like(x, float('nan')), stage=None))
        assert torch.equal(bits(again), bits(got))
    else:
        assert not torch.equal(got, _composed(eps, x, dict(coef, u=0.0), nu, guidance, None)[0])
    if case == 'a_zero_last':        # b den alone
        assert torch.equal(got, den * torch.tensor(np.float32(coef['b']), device='cuda'))
    if case == 'a_large':            # the x term is there
        assert not torch.equal(got, _composed(eps, x, dict(coef, a=0.0), nu, guidance, None)[0])
    if guided:                       # the unguided form reads the first n rows as they are, whatever guidance / mode / uncond_first say
        plain = x.clone()
        ops.lcm_step(eps[:n].contiguous(), plain, coef, None, **dict(kw, den_out=None, stage=None, mode=5, uncond_first=False))
        assert torch.equal(bits(plain), bits(_composed(eps[:n].contiguous(), x, coef, nu, None, None)[0])) and not torch.equal(plain, got)


def test_lcm_step_device_noise_depends_on_level_seed_and_index():
    from sdod.amd import ops
    eps, x, _, _ = _step_inputs(2, 4, 16, 16, False, seed=3)
    coef = _coef('middle_device', False)
    outs = []
    for seed, level, idx0 in ((1, 0, 0), (2, 0, 0), (1, 1, 0), (1, 0, 1)):
        got = x.clone()
        ops.lcm_step(eps, got, coef, None, seed=seed, noise_level=level, image_index=idx0)
        outs.append(got)
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(outs[a], outs[b])
    inj = torch.cat([ops.randn((1, 4, 16, 16), 1, (3 << 32) | 0, 'cuda'), ops.randn((1, 4, 16, 16), 1, (3 << 32) | 1, 'cuda')])
    b = x.clone()
    ops.lcm_step(eps, b, coef, None, noise=inj)
    assert torch.equal(outs[0], b)


def test_lcm_step_refuses_bad_arguments_and_leaves_outputs_untouched():
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    n, c, h, w = 2, 4, 16, 16
    eps, x, nu, temb_row = _step_inputs(n, c, h, w, True, seed=9)
    x_dst = torch.full((2 * n, c, h, w), -3.0, device='cuda')
    temb_dst = torch.zeros(2 * n, TEMB_W, dtype=torch.float16, device='cuda')
    den_out = torch.full_like(x, 7.0)
    x0 = x.clone()
    stage = (x_dst, temb_row, temb_dst)
    good = _coef('middle_injected', False)

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(bits(x), bits(x0)) and bool((den_out == 7.0).all()) and bool((x_dst == -3.0).all()) and bool((temb_dst == 0).all())

    def refused(*args, **kw):
        with pytest.raises(SdodError):
            ops.lcm_step(*args, **kw)
        assert untouched()

    refused(eps, x, good, 1.5, den_out=den_out, noise=nu, mode=2, stage=stage)                       # a mode that does not exist
    big = torch.zeros(n * c * h * w + 4, device='cuda')
    off = big[1:1 + n * c * h * w].view(n, c, h, w)
    refused(eps, x, good, 1.5, den_out=den_out, noise=off, stage=stage)                             # noise not 16-byte aligned
    refused(eps, x, good, 1.5, den_out=off, noise=nu, stage=stage)                                  # den_out not 16-byte aligned
    refused(eps, off, good, 1.5, den_out=den_out, noise=nu, stage=stage)                            # x not 16-byte aligned
    assert bool((big == 0).all())
    sbig = torch.full((2 * n * c * h * w + 4,), -3.0, device='cuda')
    refused(eps, x, good, 1.5, den_out=den_out, noise=nu, stage=(sbig[1:1 + 2 * n * c * h * w], temb_row, temb_dst))   # x_stage misaligned
    assert bool((sbig == -3.0).all())
    for key in ('d0', 'd1', 'a', 'b', 'u'):                                                         # a non-finite scalar
        for bad in (float('nan'), float('inf'), -float('inf')):
            refused(eps, x, dict(good, **{key: bad}), 1.5, den_out=den_out, noise=nu, stage=stage)
    refused(eps, x, good, float('nan'), den_out=den_out, noise=nu, stage=stage)                     # guidance is one of them
    eps3 = torch.zeros(1, 5, 1, 3, dtype=torch.float16, device='cuda')                              # c * hw not a multiple of 4
    x3 = torch.ones(1, 3, 5, 1, device='cuda')
    with pytest.raises(SdodError):
        ops.lcm_step(eps3, x3, good, None)
    torch.cuda.synchronize()
    assert bool((x3 == 1.0).all()) and untouched()
    ops.lcm_step(eps, x, good, 1.5, den_out=den_out, noise=nu, stage=stage)                         # the same call with good arguments goes through
    torch.cuda.synchronize()
    assert not torch.equal(x, x0) and not bool((den_out == 7.0).any()) and not bool((x_dst == -3.0).any()) and bool((temb_dst == temb_row).all())


# ------------------------------------------------------------------ the guidance-scale features
@pytest.mark.parametrize('dim', [256, 32])
def test_guidance_features_match_fp64(dim):
    from sdod.amd import ops
    from sdod.amd.samplers import guidance_embedding
    worst = 0.0
    for ws in ([1.0, 1.5, 8.0], [15.0, 1.0, 8.0]):               # n = 3, w over {1, 1.5, 8, 15}
        w = torch.tensor(ws, dtype=torch.float32)
        got = ops.guidance_features(w.cuda(), dim).cpu()
        assert got.shape == (3, dim) and got.dtype == torch.float16
        ref = guidance_embedding(np.asarray(ws), dim)
        half = dim // 2
        f = np.exp(-np.arange(half) * np.log(10000.0) / (half - 1))
        arg = np.abs((np.asarray(ws)[:, None] - 1.0) * 1000.0 * f[None, :])
        bound = np.concatenate([arg, arg], axis=1) * 4 * 2.0 ** -24 + 2.0 ** -11
        err = np.abs(got.double().numpy() - ref)
        print(f'guidance features dim {dim} w {ws}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}, bound at the worst argument {bound.max():.3e}')
        assert (err <= bound).all(), float((err / bound).max())
        worst = max(worst, float(err.max()))
        for i, wv in enumerate(ws):
            if wv == 1.0:            # exact: sin 0 | cos 0
                assert torch.equal(got[i], torch.cat([torch.zeros(half), torch.ones(half)]).half())
    assert worst > 0.0               # fp16 output of an fp32 argument: the comparison is not vacuous
    # the project's timestep features use the other layout: cosine first, divisor half
    t = ops.timestep_features(torch.tensor([7000.0], device='cuda'), dim).cpu()
    assert not torch.equal(t[0], ops.guidance_features(torch.tensor([8.0], device='cuda'), dim).cpu()[0])


# ------------------------------------------------------------------ the TEMB graph with cond_proj
@pytest.fixture(scope='module')
def temb_rig():
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    sd = Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235)
    unet_sd = Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234)
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**unet_sd, **sd}, assign=True)
    return dict(cfg=cfg, sd=sd, unet=unet.eval())


def _cond_proj(dim, seed=7):
    # the size a trained projection has next to the timestep features: unit-norm features in, contributions of order 1 out
    return (torch.randn(320, dim, generator=torch.Generator().manual_seed(seed)) / dim ** 0.5).half()


@pytest.mark.parametrize('dim', [256, 32])
def test_temb_graph_with_cond_proj_matches_the_restatement(temb_rig, dim):
    """batch 4, mixed t and w; dim 32 takes the padded-weight path (the GEMM's K step is 64)"""
    from sdod.amd import engine as E
    r = temb_rig
    cp = _cond_proj(dim)
    g = E.Temb(r['cfg'], 4, cond_proj_dim=dim)
    g.load_state_dict({**r['sd'], 'time_embed.cond_proj.weight': cp})
    g.finalize()
    t = torch.tensor([999.0, 759.0, 499.0, 259.0])
    w = torch.tensor([8.0, 1.0, 15.0, 1.5])
    g.t.copy_(t); g.w.copy_(w)
    g.execute()
    torch.cuda.synchronize()
    out = g.out.float().cpu()
    ref = R.temb_rows(r['unet'], t, w, cp)
    assert out.shape == ref.shape
    rl = rel_l2(out, ref)
    plain = rel_l2(R.temb_rows(r['unet'], t), ref)
    print(f'TEMB with cond_proj dim {dim}: rel-L2 {rl:.3e} (tolerance 5e-3); the plain rows are {plain:.3e} away')
    assert torch.isfinite(out).all() and rl <= 5e-3, rl
    assert plain > 10 * 5e-3                     # the term is visible at this tolerance: leaving it out could not pass
    eager = g.out.clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.out, eager)


def test_a_zero_cond_proj_gives_the_plain_graphs_bits(temb_rig):
    from sdod.amd import engine as E
    r = temb_rig
    t = torch.tensor([999.0, 759.0, 499.0, 259.0])
    plain = E.Temb(r['cfg'], 4)
    plain.load_state_dict(r['sd']); plain.finalize()
    plain.t.copy_(t); plain.execute()
    for dim in (256, 32):
        g = E.Temb(r['cfg'], 4, cond_proj_dim=dim)
        g.load_state_dict({**r['sd'], 'time_embed.cond_proj.weight': torch.zeros(320, dim)})
        g.finalize()
        g.t.copy_(t); g.w.copy_(torch.tensor([8.0, 1.0, 15.0, 1.5]))
        g.execute()
        torch.cuda.synchronize()
        assert torch.equal(g.out, plain.out)
        assert g.stats()['launches'] > plain.stats()['launches']               # the features and the GEMM
    assert not hasattr(plain, 'w')
    with pytest.raises(Exception):
        plain._io(False, 1)
