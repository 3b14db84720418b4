"""Restatements for the LCM tests, independent of sdod.amd.samplers: the published multistep consistency step in float64, the
timestep grid and alpha-bar table, the refusal cases of sdod_lcm_step, and an fp32 CPU chain on the oracle UNet (oracle.sd_torch)
with the guidance-scale embedding's cond_proj term in front of its time MLP.  No device."""
import math

import numpy as np
import torch

TIMESTEPS = {                                    # (steps, strength) -> the grid, checked by hand (original_steps = 50)
    (1, 1.0): [999], (2, 1.0): [999, 499], (4, 1.0): [999, 759, 499, 259],
    (8, 1.0): [999, 879, 759, 639, 499, 379, 259, 139], (4, 0.5): [499, 379, 259, 139],
}


def alphas_cumprod():
    """ldm's scaled-linear schedule as its float32 buffer holds it, in float64"""
    betas = np.linspace(0.00085 ** 0.5, 0.0120 ** 0.5, 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas).astype(np.float32).astype(np.float64)


def timesteps(steps, original_steps=50, strength=1.0):
    """diffusers LCMScheduler.set_timesteps, in its own words: every k-th training step, the first int(original_steps * strength) of
    them, reversed, `steps` of them picked at the floor of an even spacing"""
    k = 1000 // original_steps
    origin = [i * k - 1 for i in range(1, int(original_steps * strength) + 1)][::-1]
    return [origin[int(math.floor(i * len(origin) / steps))] for i in range(steps)]


def published_step(x, model_out, t, t_next, nu, v_prediction=False, timestep_scaling=10.0, sigma_data=0.5):
    """one multistep-consistency step as published (float64 numpy): predicted x0 from eps (or v), the boundary-condition mix
    den = c_out x0 + c_skip x, then -- unless this is the last step (t_next None) -- noised to t_next.  Returns (x', x0)."""
    ac = alphas_cumprod()
    a = ac[t]
    if v_prediction:
        x0 = math.sqrt(a) * x - math.sqrt(1.0 - a) * model_out
    else:
        x0 = (x - math.sqrt(1.0 - a) * model_out) / math.sqrt(a)
    s = timestep_scaling * t
    c_skip = sigma_data ** 2 / (s ** 2 + sigma_data ** 2)
    c_out = s / math.sqrt(s ** 2 + sigma_data ** 2)
    den = c_out * x0 + c_skip * x
    if t_next is None:
        return den, x0
    a1 = ac[t_next]
    return math.sqrt(a1) * den + math.sqrt(1.0 - a1) * nu, x0


# ---- the refusals of sdod_lcm_step: a good call (BASE) and, per case, the struct fields that make it a bad one.  A pointer field takes
# ('null',) or ('offset', bytes).
BASE = dict(n=2, c=4, hw=256, guided=1, uncond_first=1, mode=1, noise_level=1, stage_reps=2, guidance=1.5, d0=1.2, d1=-0.7, a=0.3, b=0.9, u=0.4)
POINTERS = ('eps_nhwc', 'x', 'den_out', 'noise', 'x_stage', 'temb_row', 'temb_dst')
SCALARS = ('guidance', 'd0', 'd1', 'a', 'b', 'u')
REFUSALS = [(f'{p} NULL', {p: ('null',)}) for p in ('eps_nhwc', 'x')] + \
    [(f'{p} misaligned', {p: ('offset', 4)}) for p in ('x', 'den_out', 'noise', 'x_stage')] + \
    [(f'{s} = {v}', {s: v}) for s in SCALARS for v in (float('nan'), float('inf'), -float('inf'))] + [
    ('c hw no multiple of 4', dict(c=1, hw=255)), ('c hw no multiple of 4, unguided', dict(c=3, hw=5, guided=0)),
    ('n = 0', dict(n=0)), ('n = -1', dict(n=-1)), ('c = 0', dict(c=0)), ('hw = 0', dict(hw=0)),
    ('temb_row without temb_dst', dict(temb_dst=('null',))), ('temb_row without temb_dst, unguided', dict(temb_dst=('null',), guided=0)),
]


def fill_args(pointers, over=None, temb=(0, 0)):
    """sdod_lcm_step_args from BASE, the addresses `pointers` {field: int} and temb = (width, reps), with the fields of `over` replaced"""
    from sdod.amd import _lib
    v = dict(BASE, temb_width=temb[0], temb_reps=temb[1], **{p: pointers.get(p) for p in POINTERS})
    for key, val in (over or {}).items():
        if isinstance(val, tuple):
            v[key] = None if val[0] == 'null' else pointers[key] + val[1]
        else:
            v[key] = val
    a = _lib.LcmStepArgs()
    for key, val in v.items():
        setattr(a, key, val)
    return a


# ---- the model side, fp32 on the CPU
def guidance_features(w, dim=256):
    """diffusers get_guidance_scale_embedding in torch float64: [sin | cos] of (w - 1) 1000 exp(-j ln(1e4) / (dim/2 - 1))"""
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000.0) / (half - 1)))
    arg = ((w.double() - 1.0) * 1000.0)[:, None] * f[None, :]
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=1)


@torch.no_grad()
def time_embedding(unet, t, w=None, cond_proj=None):
    """the oracle UNet's time MLP on timestep_embedding(t) (+ guidance_features(w) @ cond_proj^T, a full LCM checkpoint's t_emb + cond_proj(w_emb))"""
    from oracle import sd_torch as S
    feat = S.timestep_embedding(t, unet.model_ch)
    if cond_proj is not None:
        feat = feat + guidance_features(w, cond_proj.shape[1]).float() @ cond_proj.float().t()
    return unet.time_embed(feat)


@torch.no_grad()
def temb_rows(unet, t, w=None, cond_proj=None):
    """what the TEMB graph puts out: the embedding pushed through every ResBlock's emb_layers, in the order the UNet visits them"""
    from oracle import sd_torch as S
    emb = time_embedding(unet, t, w, cond_proj)
    blocks = [m[0] for m in list(unet.input_blocks) + [unet.middle_block] + list(unet.output_blocks) if isinstance(m[0], S.ResBlock)]
    blocks.insert(blocks.index(unet.middle_block[0]) + 1, unet.middle_block[2])
    return torch.cat([b.emb_layers(emb) for b in blocks], dim=1)


@torch.no_grad()
def unet_eval(unet, x, t, ctx, w=None, cond_proj=None):
    """oracle.sd_torch.UNetModel.forward with the embedding of time_embedding()"""
    emb = time_embedding(unet, t, w, cond_proj)
    hs, h = [], x
    for m in unet.input_blocks:
        h = m(h, emb, ctx)
        hs.append(h)
    h = unet.middle_block(h, emb, ctx)
    for m in unet.output_blocks:
        h = m(torch.cat([h, hs.pop()], dim=1), emb, ctx)
    return unet.out(h)


@torch.no_grad()
def sample_lcm(unet, ctx2, x, steps, step_noise, guidance=None, w=None, cond_proj=None, v_prediction=False, original_steps=50, strength=1.0):
    """fp32 on the CPU, the published algorithm in diffusers' operation order.  guidance None: one conditional evaluation per step
    (w, cond_proj: the guidance embedding); a number: CFG mode 1 on the (uncond, cond) pair."""
    ac = torch.from_numpy(alphas_cumprod()).float()
    ts = timesteps(steps, original_steps, strength)
    c = ctx2.float()
    n = x.shape[0]
    x = x.clone().float()
    for i, t in enumerate(ts):
        tt = torch.full((n,), float(t))
        ww = None if w is None else torch.full((n,), float(w))
        e = unet_eval(unet, x, tt, c[1:2].expand(n, -1, -1), ww, cond_proj)
        if guidance is not None:
            e_u = unet_eval(unet, x, tt, c[0:1].expand(n, -1, -1), ww, cond_proj)
            e = e_u + guidance * (e - e_u)
        a = ac[t]
        x0 = a.sqrt() * x - (1 - a).sqrt() * e if v_prediction else (x - (1 - a).sqrt() * e) / a.sqrt()
        s = torch.tensor(10.0 * t)
        c_skip, c_out = 0.25 / (s ** 2 + 0.25), s / (s ** 2 + 0.25).sqrt()
        den = c_out * x0 + c_skip * x
        if i + 1 < len(ts):
            a1 = ac[ts[i + 1]]
            x = a1.sqrt() * den + (1 - a1).sqrt() * step_noise[i]
        else:
            x = den
    return x
