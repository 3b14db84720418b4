"""The k-diffusion samplers on the host (no GPU): the sigma tables and schedules of sdod.amd.samplers.KSchedule against recorded values,
the linear form KSchedule.coef() reduces the three published algorithms to (Euler, Euler ancestral, DPM++ 2M) against those algorithms
written out in k-diffusion's own operation order in fp64, and the argument contract of the pipeline entry points.

The recorded values were computed from this repository's scaled_linear_alphas_cumprod (float32 cumprod, the table every sampler here
uses) in float64; they are asserted to 1e-8 relative.  They are written down to 8 (the table's ends: 10) decimals, which for the
small ones is fewer than 8 significant digits, so a recorded value stands for the interval of half a unit of its last decimal around
it: the bound is 1e-8 relative or that half unit, whichever is larger, and never more."""
import numpy as np
import pytest
import torch

from sdod.amd.samplers import K_SAMPLERS, KSchedule

REL = 1e-8


def close(got, want, rel=REL, decimals=None):
    """|got - want| <= rel |want|; decimals: `want` is a recorded value rounded to that many decimals (see the module docstring)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = rel * np.abs(want)
    if decimals is not None:
        bound = np.maximum(bound, 0.5 * 10.0 ** -decimals)
    return bool(np.all(np.abs(got - want) <= bound))


# ------------------------------------------------------------------ tables and schedules
def test_k_samplers_names():
    assert K_SAMPLERS == ('euler', 'euler_a', 'dpmpp_2m')


def test_sigma_table_ends():
    k = KSchedule(20)
    assert close(k.sigma_max, 14.6146414897, decimals=10) and close(k.sigma_min, 0.0291675332, decimals=10)
    assert k.sigma_table.dtype == np.float64 and k.sigma_table.shape == (1000,)
    assert np.all(np.diff(k.sigma_table) > 0)


def test_discrete_schedule_values():
    k = KSchedule(20, 'discrete')
    assert k.sigmas.dtype == np.float64 and k.sigmas.shape == (21,) and k.times.shape == (20,)
    want_t = np.linspace(999, 0, 20)
    # the round trip t -> sigma -> t: 1e-8 relative, and where the wanted time is 0 the same bound relative to the grid's scale
    assert np.all(np.abs(k.times - want_t) <= REL * np.maximum(np.abs(want_t), 1.0)), np.abs(k.times - want_t).max()
    assert close(k.sigmas[[1, 10, 18]], [10.74680243, 1.48058063, 0.23216425], decimals=8)
    assert close(k.sigmas[0], k.sigma_max) and close(k.sigmas[19], k.sigma_min) and k.sigmas[20] == 0.0


def test_karras_schedule_values():
    k = KSchedule(20, 'karras')
    assert k.sigmas.shape == (21,) and k.times.shape == (20,)
    assert close(k.sigmas[[1, 10, 18]], [11.72536842, 1.09079028, 0.04848191], decimals=8)
    assert close(k.times[[1, 10, 18]], [961.73279093, 380.13180985, 1.78294944], decimals=8)
    assert close(k.sigmas[0], k.sigma_max) and close(k.sigmas[19], k.sigma_min) and k.sigmas[20] == 0.0
    assert close(k.times[0], 999.0) and abs(k.times[19]) <= REL
    # rho is the published formula's exponent: another rho, another interior, the same ends
    k5 = KSchedule(20, 'karras', rho=5.0)
    assert close(k5.sigmas[[0, 19]], k.sigmas[[0, 19]]) and not close(k5.sigmas[10], k.sigmas[10], 1e-3)


def test_sigma_to_t_inverts_the_table_and_clamps():
    k = KSchedule(7)
    t = k.sigma_to_t(k.sigma_table)
    assert np.abs(t - np.arange(1000)).max() <= 1e-9
    assert close(k.t_to_sigma(np.arange(1000.0)), k.sigma_table, 1e-14)
    assert k.sigma_to_t(1e-3) == 0.0 and k.sigma_to_t(100.0) == 999.0               # clamped to [0, 999]
    # between two integer levels: linear in log sigma
    mid = np.exp(0.25 * np.log(k.sigma_table[500]) + 0.75 * np.log(k.sigma_table[501]))
    assert abs(float(k.sigma_to_t(mid)) - 500.75) <= 1e-9
    assert close(k.t_to_sigma(500.75), mid, 1e-13)


@pytest.mark.parametrize('schedule', ['discrete', 'karras'])
@pytest.mark.parametrize('steps', [1, 2, 12, 20, 50])
def test_sigmas_strictly_decreasing(schedule, steps):
    k = KSchedule(steps, schedule)
    assert k.sigmas.shape == (steps + 1,) and np.all(np.diff(k.sigmas) < 0) and k.sigmas[-1] == 0.0
    assert np.all(np.diff(k.times) < 0) and np.all((k.times >= 0) & (k.times <= 999))
    for i in range(steps + 1):
        assert k.c_in(i) == float(1.0 / np.sqrt(k.sigmas[i] ** 2 + 1.0))
    assert k.c_in(steps) == 1.0


# ------------------------------------------------------------------ the coefficients
@pytest.mark.parametrize('schedule', ['discrete', 'karras'])
def test_coefficient_identities(schedule):
    k = KSchedule(12, schedule)
    for i in range(12):
        s, s1 = k.sigmas[i], k.sigmas[i + 1]
        for eta in (0.3, 1.0, 2.5):
            c = k.coef('euler_a', i, eta=eta)
            up, down = c['u'], c['a'] * s
            assert abs(up * up + down * down - s1 * s1) <= 1e-12 * s1 * s1, (i, eta)
            assert 0.0 <= up <= s1
            assert c['b'] == 1.0 - c['a'] and c['cprev'] == 0.0
        assert k.coef('euler_a', i, eta=0.0) == k.coef('euler', i)                   # exactly
        for name in K_SAMPLERS:
            c = k.coef(name, i)
            assert (c['d0'], c['d1']) == (1.0, -s) and c['stage_scale'] == k.c_in(i + 1)
            cv = k.coef(name, i, v_prediction=True)
            assert close(cv['d0'], 1.0 / (s * s + 1.0), 1e-15) and close(cv['d1'], -s / np.sqrt(s * s + 1.0), 1e-15)
            assert {q: cv[q] for q in ('a', 'b', 'cprev', 'u')} == {q: c[q] for q in ('a', 'b', 'cprev', 'u')}
    for name in K_SAMPLERS:
        c = k.coef(name, 11)
        assert (c['a'], c['b'], c['cprev'], c['u']) == (0.0, 1.0, 0.0, 0.0), name   # the last step returns den
        assert set(c) == {'d0', 'd1', 'a', 'b', 'cprev', 'u', 'stage_scale'} and all(type(v) is float for v in c.values())
    assert k.coef('dpmpp_2m', 0)['cprev'] == 0.0
    assert k.coef('dpmpp_2m', 1)['cprev'] != 0.0
    assert k.coef('dpmpp_2m', 5, first=5)['cprev'] == 0.0                            # img2img: the first executed step has no history
    assert k.coef('euler', 3)['u'] == 0.0 and k.coef('dpmpp_2m', 3)['u'] == 0.0


def test_coef_refuses_bad_arguments():
    k = KSchedule(5)
    with pytest.raises(ValueError):
        k.coef('heun', 0)
    with pytest.raises(ValueError):
        k.coef('euler', 5)
    with pytest.raises(ValueError):
        k.coef('euler_a', 0, eta=-0.1)
    with pytest.raises(ValueError):
        KSchedule(0)
    with pytest.raises(ValueError):
        KSchedule(5, 'exponential')


# ------------------------------------------------------------------ the published algorithms, in their own operation order (fp64)
def _eps_model(x, sigma):
    """an arbitrary smooth eps(x, sigma), the same for every algorithm below"""
    grid = np.linspace(-1.0, 1.0, x.size).reshape(x.shape)
    return np.sin(1.3 * x / np.sqrt(sigma * sigma + 1.0) + grid) + 0.2 * np.cos(sigma) * grid + 0.05 * x / (1.0 + sigma)


def _denoised(x, sigma, v_prediction):
    """k-diffusion's DiscreteEpsDDPMDenoiser / DiscreteVDDPMDenoiser.forward (sigma_data = 1): the model sees c_in * x; returns (denoised,
    the model output)"""
    c_in = 1.0 / np.sqrt(sigma * sigma + 1.0)
    out = _eps_model(x * c_in, sigma)
    if v_prediction:
        c_skip, c_out = 1.0 / (sigma * sigma + 1.0), -sigma / np.sqrt(sigma * sigma + 1.0)
        return out * c_out + x * c_skip, out
    return x + out * (-sigma), out


def _published(sampler, sigmas, x, noises, eta, v_prediction):
    """sample_euler / sample_euler_ancestral / sample_dpmpp_2m of the k-diffusion package, statement by statement"""
    old_denoised = None
    for i in range(len(sigmas) - 1):
        denoised, _ = _denoised(x, sigmas[i], v_prediction)
        if sampler == 'euler':
            d = (x - denoised) / sigmas[i]                       # to_d
            dt = sigmas[i + 1] - sigmas[i]
            x = x + d * dt
        elif sampler == 'euler_a':
            sf, st = sigmas[i], sigmas[i + 1]                    # get_ancestral_step
            sigma_up = min(st, eta * (st ** 2 * (sf ** 2 - st ** 2) / sf ** 2) ** 0.5)
            sigma_down = (st ** 2 - sigma_up ** 2) ** 0.5
            d = (x - denoised) / sigmas[i]
            dt = sigma_down - sigmas[i]
            x = x + d * dt
            if sigmas[i + 1] > 0:
                x = x + noises[i] * sigma_up
        else:
            if sigmas[i + 1] == 0:                               # sigma_fn(t_next) / sigma_fn(t) = 0, -expm1(-h) = 1 with h = inf
                x = denoised
            else:
                t, t_next = -np.log(sigmas[i]), -np.log(sigmas[i + 1])
                h = t_next - t
                if old_denoised is None:
                    x = (np.exp(-t_next) / np.exp(-t)) * x - np.expm1(-h) * denoised
                else:
                    h_last = t - (-np.log(sigmas[i - 1]))
                    r = h_last / h
                    denoised_d = (1 + 1 / (2 * r)) * denoised - (1 / (2 * r)) * old_denoised
                    x = (np.exp(-t_next) / np.exp(-t)) * x - np.expm1(-h) * denoised_d
            old_denoised = denoised
    return x


def _linear_form(sampler, k, x, noises, eta, v_prediction):
    den_prev = np.zeros_like(x)
    for i in range(k.steps):
        c = k.coef(sampler, i, eta=eta, v_prediction=v_prediction)
        e = _eps_model(x * k.c_in(i), k.sigmas[i])
        den = c['d0'] * x + c['d1'] * e
        xn = c['a'] * x + c['b'] * den
        if c['cprev'] != 0.0:
            xn = xn + c['cprev'] * den_prev
        if c['u'] != 0.0:
            xn = xn + c['u'] * noises[i]
        den_prev, x = den, xn
    return x


@pytest.mark.parametrize('schedule', ['discrete', 'karras'])
@pytest.mark.parametrize('sampler', K_SAMPLERS)
@pytest.mark.parametrize('v_prediction', [False, True])
def test_linear_form_equals_the_published_algorithms(sampler, schedule, v_prediction):
    k = KSchedule(12, schedule)
    rng = np.random.default_rng(11)
    x0 = k.sigmas[0] * rng.standard_normal((2, 4, 5, 7))
    noises = rng.standard_normal((12, 2, 4, 5, 7))
    worst = 0.0
    for eta in ((0.0, 0.6, 1.0) if sampler == 'euler_a' else (1.0,)):
        want = _published(sampler, k.sigmas, x0.copy(), noises, eta, v_prediction)
        got = _linear_form(sampler, k, x0.copy(), noises, eta, v_prediction)
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))))
    print(f'{sampler} {schedule} v={v_prediction}: linear form vs published order, max relative difference {worst:.2e}')
    assert worst <= 1e-12, worst


def test_ancestral_noise_matters_and_eta0_is_euler():
    k = KSchedule(12, 'karras')
    rng = np.random.default_rng(3)
    x0 = k.sigmas[0] * rng.standard_normal((1, 4, 4, 4))
    noises = rng.standard_normal((12, 1, 4, 4, 4))
    e = _linear_form('euler', k, x0.copy(), noises, 1.0, False)
    assert np.array_equal(_linear_form('euler_a', k, x0.copy(), noises, 0.0, False), e)
    assert not np.allclose(_linear_form('euler_a', k, x0.copy(), noises, 1.0, False), e)


# ------------------------------------------------------------------ the argument contract, without a device
LAT = (4, 16, 16)


def test_k_check_args_accepts_the_documented_calls():
    from sdod.amd.pipeline import img2img_k_check_args, k_check_args
    for s in K_SAMPLERS:
        for sch in ('discrete', 'karras'):
            k_check_args(s, 20, sch, 1.0, None, LAT, 1)
            k_check_args(s, 20, sch, 0.0, None, LAT, 1, old_samplers=True)
    k_check_args('euler_a', 20, 'karras', 1.0, torch.zeros(19, 1, 4, 16, 16), LAT, 1)
    k_check_args('euler_a', 20, 'karras', 1.0, torch.zeros(9, 2, 4, 16, 16), LAT, 2, first=10)
    k_check_args('euler_a', 1, 'discrete', 1.0, torch.zeros(0, 1, 4, 16, 16), LAT, 1)
    k_check_args('plms', 20, 'discrete', 1.0, None, LAT, 1, old_samplers=True)
    k_check_args('dpm', 20, 'discrete', 1.0, None, LAT, 1, old_samplers=True)
    assert img2img_k_check_args(0.5, 20, None, 'discrete', 1.0, None, LAT, 1) == 10
    assert img2img_k_check_args(0.5, 20, 'euler_a', 'karras', 1.0, torch.zeros(9, 1, 4, 16, 16), LAT, 1) == 10
    assert img2img_k_check_args(0.75, 8, 'dpmpp_2m', 'karras', 1.0, None, LAT, 1) == 6


@pytest.mark.parametrize('case', ['sampler', 'old_sampler_not_allowed', 'schedule', 'eta', 'eta_nan', 'steps_zero', 'steps_frac', 'first',
                                  'noise_shape', 'noise_rows', 'noise_dtype', 'noise_type', 'noise_not_ancestral', 'plms_schedule',
                                  'plms_noise', 'dpm_schedule'])
def test_k_check_args_refuses(case):
    from sdod.amd.pipeline import k_check_args
    kw = dict(sampler='euler_a', steps=20, schedule='karras', eta=1.0, step_noise=None, latent=LAT, n_images=1, first=0, old_samplers=True)
    if case == 'sampler':
        kw['sampler'] = 'heun'
    elif case == 'old_sampler_not_allowed':
        kw.update(sampler='plms', schedule='discrete', old_samplers=False)
    elif case == 'schedule':
        kw['schedule'] = 'exponential'
    elif case == 'eta':
        kw['eta'] = -0.5
    elif case == 'eta_nan':
        kw['eta'] = float('nan')
    elif case == 'steps_zero':
        kw['steps'] = 0
    elif case == 'steps_frac':
        kw['steps'] = 2.5
    elif case == 'first':
        kw['first'] = 20
    elif case == 'noise_shape':
        kw['step_noise'] = torch.zeros(19, 1, 4, 16, 8)
    elif case == 'noise_rows':
        kw['step_noise'] = torch.zeros(20, 1, 4, 16, 16)
    elif case == 'noise_dtype':
        kw['step_noise'] = torch.zeros(19, 1, 4, 16, 16, dtype=torch.float16)
    elif case == 'noise_type':
        kw['step_noise'] = np.zeros((19, 1, 4, 16, 16), np.float32)
    elif case == 'noise_not_ancestral':
        kw.update(sampler='euler', step_noise=torch.zeros(19, 1, 4, 16, 16))
    elif case == 'plms_schedule':
        kw.update(sampler='plms')
    elif case == 'plms_noise':
        kw.update(sampler='plms', schedule='discrete', step_noise=torch.zeros(19, 1, 4, 16, 16))
    elif case == 'dpm_schedule':
        kw.update(sampler='dpm')
    with pytest.raises(ValueError):
        k_check_args(**kw)


def test_img2img_k_check_args_refuses():
    from sdod.amd.pipeline import img2img_k_check_args
    with pytest.raises(ValueError):
        img2img_k_check_args(1.0, 20, 'euler', 'discrete', 1.0, None, LAT, 1)         # t_enc == steps
    with pytest.raises(ValueError):
        img2img_k_check_args(0.5, 20, None, 'karras', 1.0, None, LAT, 1)              # DDIM has no karras schedule
    with pytest.raises(ValueError):
        img2img_k_check_args(0.5, 20, None, 'discrete', 1.0, torch.zeros(9, 1, 4, 16, 16), LAT, 1)
    with pytest.raises(ValueError):
        img2img_k_check_args(0.5, 20, 'plms', 'discrete', 1.0, None, LAT, 1)          # img2img's samplers: None or a k-sampler
    with pytest.raises(ValueError):
        img2img_k_check_args(0.5, 20, 'euler_a', 'karras', 1.0, torch.zeros(19, 1, 4, 16, 16), LAT, 1)   # t_enc - 1 = 9 rows


def test_entry_points_refuse_before_any_device_work():
    """on an object without a constructor (no device, no graphs): the ValueError comes before anything touches them"""
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    pipe.cfg = E.sd14_config(16, 16)
    pipe.n = 1
    x_T = torch.zeros(1, 4, 16, 16)
    u8 = torch.zeros(1, 128, 128, 3, dtype=torch.uint8)
    for fn in (pipe.generate, pipe.generate_graphed):
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'heun')
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'euler', schedule='cosine')
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'euler_a', eta=-1.0)
        with pytest.raises(ValueError):
            fn(None, x_T, 0, 7.5, 'dpmpp_2m')
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'euler_a', step_noise=torch.zeros(3, 1, 4, 16, 16))
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'plms', schedule='karras')
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'dpm', step_noise=torch.zeros(19, 1, 4, 16, 16))
        with pytest.raises(TypeError):
            fn(None, x_T, 20, 7.5, 'euler', 'karras')                                  # the new arguments are keyword-only
    with pytest.raises(ValueError):
        pipe.sample_k(None, x_T, 'plms')
    with pytest.raises(ValueError):
        pipe.sample_k(None, x_T, 'euler', first=20)
    for fn in (pipe.img2img, pipe.img2img_graphed):
        with pytest.raises(ValueError):
            fn(None, u8, 0.5, 20, 7.5, sampler='heun')
        with pytest.raises(ValueError):
            fn(None, u8, 0.5, 20, 7.5, schedule='karras')
        with pytest.raises(ValueError):
            fn(None, u8, 0.5, 20, 7.5, sampler='euler_a', step_noise=torch.zeros(10, 1, 4, 16, 16))
    for name in K_SAMPLERS:
        with pytest.raises(ValueError):
            pipe.generate_pipelined(None, x_T, 20, 7.5, name)


# ------------------------------------------------------------------ the graphed entry points' static inputs, without a device
def test_graphed_entry_points_fill_their_static_inputs(monkeypatch):
    """Each *_graphed method describes its graph's static inputs to Txt2Img._replay; here _graphed hands out CPU statics and a graph that
    counts its replays, and ops.randn records what would be drawn.  The draws are compared with the rule written out by hand: image i of
    a noise input comes from Philox stream (family << 32) | (image_index + i) of the seed, family 1 = n1, 2 = n2 (of hires_seed = seed + 1:
    hires_noise), 3 + first + r = row r of the step noise, first = 0 for a whole trajectory and steps - t_enc for one that starts at a
    level.  One image per call here, image_index 3, so every stream ends in 3."""
    import inspect
    from sdod.amd import engine as E, ops
    from sdod.amd.pipeline import Txt2Img

    def bare(h, w):
        p = Txt2Img.__new__(Txt2Img)
        p.cfg, p.n, p.device, p.cfg_split = E.sd14_config(h, w), 1, torch.device('cpu'), False
        return p
    pipe = bare(16, 24)
    pipe.hires = bare(24, 32)
    pipe.encoder = pipe.masked_encoder = object()                       # the entry points only ask whether they exist
    calls, draws = [], []

    class Graph:
        replays = 0

        def replay(self):
            self.replays += 1

    def graphed(key, inputs, run):
        statics = [torch.zeros(tuple(shape), dtype=dtype) for shape, dtype in inputs]
        run(*statics)                                                   # the eager twin below: the statics arrive under its argument names
        calls.append((Graph(), [(tuple(shape), dtype) for shape, dtype in inputs], statics))
        return calls[-1][0], statics, 'out'

    def randn(shape, seed, stream_id, device, out=None):
        assert tuple(out.shape) == tuple(shape) and out.dtype == torch.float32
        draws.append((tuple(shape), seed, stream_id))
        return out
    monkeypatch.setattr(pipe, '_graphed', graphed)
    monkeypatch.setattr(ops, 'randn', randn)
    for name in ('generate', 'img2img', 'inpaint', 'inpaint_concat', 'generate_hires'):
        sig = inspect.signature(getattr(Txt2Img, name))
        monkeypatch.setattr(pipe, name, lambda *a, _sig=sig, **kw: _sig.bind(pipe, *a, **kw))      # TypeError for a name the eager method lacks

    def call(fn, *a, **kw):
        del draws[:]
        n = len(calls)
        assert fn(*a, **kw) == 'out' and len(calls) == n + 1 and calls[-1][0].replays == 1
        return calls[-1][1], calls[-1][2], sorted(draws)

    lo, hi = (1, 4, 16, 24), (1, 4, 24, 32)
    f16, f32, u8 = torch.float16, torch.float32, torch.uint8
    ctx = torch.full((2, 77, 768), 0.5, dtype=f16)
    img, mask = torch.full((1, 128, 192, 3), 7, dtype=u8), torch.full((1, 128, 192), 255, dtype=u8)
    x_T = torch.full(lo, 2.0)
    c_, i_, m_ = (tuple(ctx.shape), f16), (tuple(img.shape), u8), (tuple(mask.shape), u8)

    def stream(family):
        return (family << 32) | 3
    at = dict(seed=31, image_index=3)

    # no noise passed: everything is drawn
    req, _, got = call(pipe.generate_graphed, ctx, x_T, 4, 7.5, 'euler_a', **at)
    assert req == [c_, (lo, f32), ((3,) + lo, f32)]
    assert got == sorted((lo, 31, stream(f)) for f in (3, 4, 5))
    req, _, got = call(pipe.img2img_graphed, ctx, img, 0.5, 6, 7.5, sampler='euler_a', **at)            # t_enc = 3, first = 3
    assert req == [c_, i_, (lo, f32), (lo, f32), ((2,) + lo, f32)]
    assert got == sorted((lo, 31, stream(f)) for f in (1, 2, 6, 7))
    req, _, got = call(pipe.inpaint_graphed, ctx, img, mask, 0.5, 6, 7.5, **at)                         # t_enc = 3
    assert req == [c_, i_, m_, (lo, f32), (lo, f32), ((2,) + lo, f32)]
    assert got == sorted((lo, 31, stream(f)) for f in (1, 2, 3, 4))
    req, _, got = call(pipe.inpaint_concat_graphed, ctx, img, mask, x_T, 4, 7.5, 'plms', **at)
    assert req == [c_, i_, m_, (lo, f32), (lo, f32)]
    assert got == [(lo, 31, stream(1))]
    req, _, got = call(pipe.generate_hires_graphed, ctx, x_T, 4, 7.5, 'euler_a', hires_steps=6, denoise=0.5, **at)   # t_enc = 3, first = 3
    assert req == [c_, (lo, f32), (hi, f32), ((3,) + lo, f32), ((2,) + hi, f32)]
    assert got == sorted([(lo, 31, stream(f)) for f in (3, 4, 5)] + [(hi, 32, stream(f)) for f in (2, 6, 7)])
    _, _, got = call(pipe.generate_hires_graphed, ctx, x_T, 4, 7.5, 'euler_a', hires_steps=6, denoise=0.5, hires_seed=90, **at)
    assert got == sorted([(lo, 31, stream(f)) for f in (3, 4, 5)] + [(hi, 90, stream(f)) for f in (2, 6, 7)])

    # every noise passed: nothing is drawn, the statics hold the caller's values
    n1, n2, sn2, sn3 = torch.full(lo, 1.0), torch.full(lo, -2.0), torch.full((2,) + lo, 3.0), torch.full((3,) + lo, 4.0)
    hn, hsn = torch.full(hi, 5.0), torch.full((2,) + hi, 6.0)
    for fn, a, kw, want in (
            (pipe.generate_graphed, (ctx, x_T, 4, 7.5, 'euler_a'), dict(step_noise=sn3), [ctx, x_T, sn3]),
            (pipe.img2img_graphed, (ctx, img, 0.5, 6, 7.5), dict(sampler='euler_a', noise=(n1, n2), step_noise=sn2), [ctx, img, n1, n2, sn2]),
            (pipe.inpaint_graphed, (ctx, img, mask, 0.5, 6, 7.5), dict(noise=(n1, n2), step_noise=sn2), [ctx, img, mask, n1, n2, sn2]),
            (pipe.inpaint_concat_graphed, (ctx, img, mask, x_T, 4, 7.5, 'plms'), dict(noise=n1), [ctx, img, mask, x_T, n1]),
            (pipe.generate_hires_graphed, (ctx, x_T, 4, 7.5, 'euler_a'),
             dict(hires_steps=6, denoise=0.5, step_noise=sn3, hires_noise=hn, hires_step_noise=hsn), [ctx, x_T, hn, sn3, hsn])):
        _, statics, got = call(fn, *a, **kw, **at)
        assert got == [] and len(statics) == len(want)
        assert all(torch.equal(s, w) for s, w in zip(statics, want))

    # a sampler that draws no step noise gets no step-noise input
    for sampler in ('dpmpp_2m', 'euler', 'plms', 'dpm'):
        req, _, got = call(pipe.generate_graphed, ctx, x_T, 4, 7.5, sampler, **at)
        assert req == [c_, (lo, f32)] and got == []
    req, _, got = call(pipe.img2img_graphed, ctx, img, 0.5, 6, 7.5, **at)
    assert req == [c_, i_, (lo, f32), (lo, f32)] and got == sorted((lo, 31, stream(f)) for f in (1, 2))
    req, _, got = call(pipe.generate_hires_graphed, ctx, x_T, 4, 7.5, 'dpmpp_2m', hires_steps=6, denoise=0.5, **at)
    assert req == [c_, (lo, f32), (hi, f32)] and got == [(hi, 32, stream(2))]

    # under cfg_split the four entry points with an eager fallback hand every argument to their eager twin and capture nothing
    pipe.cfg_split, n = True, len(calls)
    for fn, a, kw in ((pipe.generate_graphed, (ctx, x_T, 4, 7.5, 'euler_a'), dict(schedule='karras', eta=0.5, step_noise=sn3)),
                      (pipe.img2img_graphed, (ctx, img, 0.5, 6, 7.5),
                       dict(sampler='euler_a', schedule='karras', eta=0.5, noise=(n1, n2), step_noise=sn2)),
                      (pipe.inpaint_graphed, (ctx, img, mask, 0.5, 6, 7.5), dict(noise=(n1, n2), step_noise=sn2, composite=False)),
                      (pipe.inpaint_concat_graphed, (ctx, img, mask, x_T, 4, 7.5, 'dpm'), dict(noise=n1, composite=False))):
        twin = getattr(Txt2Img, fn.__name__[:-len('_graphed')])
        want = inspect.signature(twin).bind(pipe, *a, **kw, **at).arguments
        got = fn(*a, **kw, **at).arguments
        assert got.keys() == want.keys() and all(got[k] is want[k] or got[k] == want[k] for k in want), fn.__name__
    assert len(calls) == n
