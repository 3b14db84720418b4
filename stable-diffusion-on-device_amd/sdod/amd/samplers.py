"""Sampler schedules on the host (numpy), applied on the GPU by the kernels of include/sdod_hip.h.

PLMS follows the public ldm `PLMSSampler` with eta = 0 (config 1's CPU reference, `scripts/txt2img.py --plms`; the ldm
repository is not part of /root/reference).  Index arithmetic (timestep sequence, alpha-bar lookups)
is integer/float64 work done here and must match the oracle exactly; the per-element arithmetic runs on device in IEEE
fp32 in ldm's operation order.  DPM-Solver++(2M) uses the C++ solver tables (host.DpmSolver)."""
import numpy as np


def scaled_linear_alphas_cumprod(n=1000, linear_start=0.00085, linear_end=0.0120):
    """ldm make_beta_schedule('linear'): betas = linspace(sqrt(s), sqrt(e), n, float64)**2; cumprod(1-betas) -> float32"""
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, n, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas, axis=0).astype(np.float32)


class PlmsSchedule:
    def __init__(self, steps=20, n_train=1000):
        c = n_train // steps
        self.timesteps = np.asarray(list(range(0, n_train, c))) + 1          # ldm make_ddim_timesteps('uniform') + 1
        ac = scaled_linear_alphas_cumprod(n_train)
        self.alphas = ac[self.timesteps]                                     # float32
        self.alphas_prev = np.asarray([ac[0]] + ac[self.timesteps[:-1]].tolist(), dtype=np.float32)
        self.sqrt_one_minus_alphas = np.sqrt(np.float32(1.0) - self.alphas).astype(np.float32)
        self.steps = len(self.timesteps)
        self.time_range = np.flip(self.timesteps)                           # descending: 951, 901, ..., 1
        # v-prediction models (SD 2.1-768): eps = sqrt(abar_t) v + sqrt(1 - abar_t) x  (ldm predict_eps_from_z_and_v)
        self.sqrt_alphas = np.sqrt(self.alphas).astype(np.float32)

    def v_to_eps_coef(self, index):
        """(coefficient of v, coefficient of x) at ddim index `index`"""
        return float(self.sqrt_alphas[index]), float(self.sqrt_one_minus_alphas[index])

    def coef(self, index):
        """fp32 scalars of get_x_prev_and_pred_x0 at ddim index `index` (sigma_t = 0)"""
        a_t = np.float32(self.alphas[index]); a_prev = np.float32(self.alphas_prev[index])
        return dict(sqrt_one_minus_at=float(self.sqrt_one_minus_alphas[index]), sqrt_at=float(np.sqrt(a_t)),
                    sqrt_a_prev=float(np.sqrt(a_prev)), dir_coef=float(np.sqrt(np.float32(1.0) - a_prev)))


# Adams-Bashforth combinations of the eps history (newest first): (coefficients, divisor)
PLMS_ORDERS = {1: ((3.0, -1.0), 2.0), 2: ((23.0, -16.0, 5.0), 12.0), 3: ((55.0, -59.0, 37.0, -9.0), 24.0)}


# ---------------------------------------------------------------------------------------------------------------------------------
# k-diffusion's sigma-space samplers (Karras et al. 2022; the public k-diffusion package's sample_euler, sample_euler_ancestral,
# sample_dpmpp_2m, DiscreteSchedule and get_sigmas_karras).  The tables are float64 numpy; the per-element arithmetic runs on the
# device in one launch per step (include/sdod_hip.h: sdod_k_step).
K_SAMPLERS = ('euler', 'euler_a', 'dpmpp_2m')
K_SCHEDULES = ('discrete', 'karras')


class KSchedule:
    """Noise levels of a k-diffusion trajectory over the model's 1000 training levels sigma_t = sqrt((1 - abar_t) / abar_t).
    sigmas: float64 [steps + 1], strictly decreasing, last entry 0.  schedule 'discrete': t_to_sigma(linspace(999, 0, steps))
    (k-diffusion DiscreteSchedule.get_sigmas); 'karras': (smax^(1/rho) + r (smin^(1/rho) - smax^(1/rho)))^rho, r = linspace(0, 1, steps),
    between sigma_999 and sigma_0 (get_sigmas_karras).  times[i] = sigma_to_t(sigmas[i]), float64 [steps]: the model time of step i's
    evaluation, fractional in general."""

    def __init__(self, steps=20, schedule='discrete', rho=7.0, n_train=1000):
        steps = int(steps)
        if steps < 1:
            raise ValueError(f'steps must be a positive integer, got {steps}')
        if schedule not in K_SCHEDULES:
            raise ValueError(f'schedule must be one of {K_SCHEDULES}, got {schedule!r}')
        ac = scaled_linear_alphas_cumprod(n_train).astype(np.float64)
        self.sigma_table = np.sqrt((1.0 - ac) / ac)                          # sigma_t, t = 0 .. n_train - 1, increasing
        self.log_sigma_table = np.log(self.sigma_table)
        self.sigma_min, self.sigma_max = float(self.sigma_table[0]), float(self.sigma_table[-1])
        self.steps, self.schedule, self.rho = steps, schedule, float(rho)
        if schedule == 'discrete':
            body = self.t_to_sigma(np.linspace(n_train - 1, 0, steps))
        else:
            r = np.linspace(0.0, 1.0, steps)
            lo, hi = self.sigma_min ** (1.0 / self.rho), self.sigma_max ** (1.0 / self.rho)
            body = (hi + r * (lo - hi)) ** self.rho
        self.sigmas = np.concatenate([np.asarray(body, dtype=np.float64).reshape(-1), [0.0]])
        self.times = self.sigma_to_t(self.sigmas[:-1])

    def sigma_to_t(self, sigma):
        """k-diffusion DiscreteSchedule.sigma_to_t: linear interpolation in log sigma between the neighbouring integer t, clamped to
        [0, n_train - 1]"""
        ls = self.log_sigma_table
        log_sigma = np.log(np.asarray(sigma, dtype=np.float64))
        low = np.clip(np.searchsorted(ls, log_sigma, side='right') - 1, 0, len(ls) - 2)   # the last table entry <= log_sigma
        w = np.clip((ls[low] - log_sigma) / (ls[low] - ls[low + 1]), 0.0, 1.0)
        return (1.0 - w) * low + w * (low + 1)

    def t_to_sigma(self, t):
        """k-diffusion DiscreteSchedule.t_to_sigma: the inverse of sigma_to_t"""
        t = np.asarray(t, dtype=np.float64)
        low = np.floor(t).astype(np.int64)
        high = np.ceil(t).astype(np.int64)
        w = t - low
        return np.exp((1.0 - w) * self.log_sigma_table[low] + w * self.log_sigma_table[high])

    def c_in(self, i):
        """the model-input scale at level i: the UNet sees c_in * x (k-diffusion DiscreteEpsDDPMDenoiser.get_scalings, sigma_data = 1)"""
        return float(1.0 / np.sqrt(self.sigmas[i] ** 2 + 1.0))

    def coef(self, sampler, i, eta=1.0, v_prediction=False, first=0):
        """the scalars of step i (sigmas[i] -> sigmas[i + 1]) in the one linear form the three published algorithms reduce to,
            den = d0 x + d1 e ;  x' = a x + b den + cprev den_prev + u nu
        (e: the guided model output, x: the unscaled latent, den_prev: the previous step's den, nu: fresh unit noise), and stage_scale =
        c_in(i + 1) for the next evaluation's input.  den: eps models (1, -s); v models (1 / (s^2 + 1), -s / sqrt(s^2 + 1)).
          euler     d = (x - den) / s ; x + d (s' - s)                     a = s'/s, b = 1 - s'/s
          euler_a   up = min(s', eta sqrt(s'^2 (s^2 - s'^2) / s^2)), down = sqrt(s'^2 - up^2) ; x + d (down - s) + up nu
          dpmpp_2m  h = log s - log s', E = -expm1(-h): (s'/s) x + E den_d, den_d = (1 + 1/(2r)) den - 1/(2r) den_prev with
                    r = (log s_prev - log s) / h; first order (den_d = den) at the trajectory's first step (i == first) and to s' = 0
        The step to s' = 0 is (a, b, cprev, u) = (0, 1, 0, 0) for all three: the result is den.  Returns a dict of Python floats."""
        if sampler not in K_SAMPLERS:
            raise ValueError(f'sampler must be one of {K_SAMPLERS}, got {sampler!r}')
        if not 0 <= i < self.steps:
            raise ValueError(f'step {i} is outside [0, {self.steps - 1}]')
        if not eta >= 0.0:
            raise ValueError(f'eta must be >= 0, got {eta}')
        s, s1 = float(self.sigmas[i]), float(self.sigmas[i + 1])
        if v_prediction:
            d0, d1 = 1.0 / (s * s + 1.0), -s / np.sqrt(s * s + 1.0)
        else:
            d0, d1 = 1.0, -s
        a, b, cprev, u = 0.0, 1.0, 0.0, 0.0
        if s1 > 0.0:
            if sampler == 'euler':
                a = s1 / s
                b = 1.0 - a
            elif sampler == 'euler_a':
                up = min(s1, float(eta) * np.sqrt(s1 * s1 * (s * s - s1 * s1) / (s * s)))
                down = np.sqrt(s1 * s1 - up * up)
                a = down / s
                b = 1.0 - a
                u = up
            else:
                h = np.log(s) - np.log(s1)
                e = -np.expm1(-h)
                a = s1 / s
                if i == first:
                    b = e
                else:
                    r = (np.log(float(self.sigmas[i - 1])) - np.log(s)) / h
                    b = e * (1.0 + 1.0 / (2.0 * r))
                    cprev = -e / (2.0 * r)
        return dict(d0=float(d0), d1=float(d1), a=float(a), b=float(b), cprev=float(cprev), u=float(u), stage_scale=self.c_in(i + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# Latent Consistency Models (Luo et al. 2023; the public diffusers LCMScheduler): 2 to 8 evaluations of a distilled checkpoint, each
# followed by the consistency function's boundary-condition mix and a fresh noising to the next level.  The tables are float64 numpy;
# the per-element arithmetic runs on the device in one launch per step (include/sdod_hip.h: sdod_lcm_step).
class LcmSchedule:
    """The timestep grid and step scalars of an LCM trajectory.  The distillation's `original_steps` training-schedule steps, k =
    n_train // original_steps apart, cut to their first int(original_steps * strength) and read from the top:
        origin = arange(1, int(original_steps * strength) + 1) * k - 1 ;  timesteps = origin[::-1][floor(linspace(0, len(origin), steps,
        endpoint=False))]
    timesteps: int64 [steps], strictly decreasing; alphas_cumprod: float64, the table PLMS uses.  strength < 1 (img2img): the
    trajectory starts at the lower level timesteps[0]."""

    def __init__(self, steps=4, original_steps=50, strength=1.0, n_train=1000, timestep_scaling=10.0, sigma_data=0.5):
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
            raise ValueError(f'steps must be a positive integer, got {steps!r}')
        if isinstance(original_steps, bool) or not isinstance(original_steps, (int, np.integer)) or not 1 <= original_steps <= n_train:
            raise ValueError(f'original_steps must be an integer in [1, {n_train}], got {original_steps!r}')
        if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) or not 0.0 < float(strength) <= 1.0:
            raise ValueError(f'strength must be in (0, 1], got {strength!r}')
        k = n_train // int(original_steps)
        origin = np.arange(1, int(int(original_steps) * float(strength)) + 1, dtype=np.int64) * k - 1
        if steps > len(origin):
            raise ValueError(f'steps = {steps} is more than the {len(origin)} levels that original_steps = {original_steps} and strength = '
                             f'{strength} leave')
        self.steps, self.original_steps, self.strength = int(steps), int(original_steps), float(strength)
        self.timestep_scaling, self.sigma_data = float(timestep_scaling), float(sigma_data)
        self.timesteps = origin[::-1][np.floor(np.linspace(0, len(origin), self.steps, endpoint=False)).astype(np.int64)]
        self.alphas_cumprod = scaled_linear_alphas_cumprod(n_train).astype(np.float64)

    def scalings(self, i):
        """(c_skip, c_out) of the consistency function's boundary condition at step i, on s = timestep_scaling * t"""
        s = self.timestep_scaling * float(self.timesteps[i])
        sd2 = self.sigma_data * self.sigma_data
        return sd2 / (s * s + sd2), s / np.sqrt(s * s + sd2)

    def start(self):
        """(z0_coef, noise_coef) of img2img's start latent at timesteps[0]: x = sqrt(abar) z0 + sqrt(1 - abar) noise"""
        ab = self.alphas_cumprod[self.timesteps[0]]
        return float(np.sqrt(ab)), float(np.sqrt(1.0 - ab))

    def coef(self, i, v_prediction=False):
        """the scalars of step i in the linear form of KSchedule.coef (no history term),
            den = d0 x + d1 e ;  x' = a x + b den + u nu
        den: the x0 prediction, eps models ((x - sqrt(1 - abar) e) / sqrt(abar)) or v models (sqrt(abar) x - sqrt(1 - abar) v);
        x' = sqrt(abar') (c_skip x + c_out den) + sqrt(1 - abar') nu with abar' at timesteps[i + 1]; the last step returns the
        consistency function's value c_skip x + c_out den and draws nothing (u = 0).  Returns a dict of Python floats."""
        if not 0 <= i < self.steps:
            raise ValueError(f'step {i} is outside [0, {self.steps - 1}]')
        ab = self.alphas_cumprod[self.timesteps[i]]
        if v_prediction:
            d0, d1 = np.sqrt(ab), -np.sqrt(1.0 - ab)
        else:
            d0, d1 = 1.0 / np.sqrt(ab), -np.sqrt(1.0 - ab) / np.sqrt(ab)
        c_skip, c_out = self.scalings(i)
        if i + 1 < self.steps:
            ab1 = self.alphas_cumprod[self.timesteps[i + 1]]
            a, b, u = np.sqrt(ab1) * c_skip, np.sqrt(ab1) * c_out, np.sqrt(1.0 - ab1)
        else:
            a, b, u = c_skip, c_out, 0.0
        return dict(d0=float(d0), d1=float(d1), a=float(a), b=float(b), u=float(u))


def guidance_embedding(w, dim=256):
    """the guidance-scale embedding of a full LCM checkpoint (its time_embedding.cond_proj input), float64 [len(w), dim]:
    v = (w - 1) * 1000, f_j = exp(-j ln(10000) / (dim/2 - 1)), [sin(v f_j) | cos(v f_j)] -- sine first and the divisor dim/2 - 1, both
    unlike the timestep features (sdod_timestep_features_f16).  The reference of sdod_guidance_features_f16."""
    if dim < 4 or dim % 2:
        raise ValueError(f'dim must be even and at least 4, got {dim}')
    v = (np.atleast_1d(np.asarray(w, dtype=np.float64)) - 1.0) * 1000.0
    half = dim // 2
    f = np.exp(-np.arange(half, dtype=np.float64) * np.log(10000.0) / (half - 1))
    arg = v[:, None] * f[None, :]
    return np.concatenate([np.sin(arg), np.cos(arg)], axis=1)
