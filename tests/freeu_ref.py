"""Restatement of FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024) on the modules of oracle.sd_torch.UNetModel.
Test infrastructure, not product.

  fourier_filter_fft   the published Fourier_filter: fftn, fftshift, scale the box [H//2-1 : H//2+1, W//2-1 : W//2+1], back, .real
  fourier_filter       its closed form: the box is the frequency set {0, -1 mod H} x {0, -1 mod W}, four (or two, or one) DFT coefficients
  backbone_factor      version 1: b; version 2: (b - 1) (m - min m) / (max m - min m) + 1 with m the channel mean, per sample -- and 1
                       where max m == min m, the one departure from the published code (0 / 0 there)
  freeu_unet           UNetModel.forward with both applied between hs.pop() and the concatenation, by the channel rule; `control`
                       (13 residuals, 13 scales) adds cldm's ControlledUnetModel terms in front of them
"""
import math

import torch

from oracle import sd_torch as S

SIZES = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (4, 4), (8, 8), (12, 8), (16, 24), (32, 32), (5, 7)]


def fourier_filter_fft(x, threshold, scale):
    """the published function, any float dtype: x [B, C, H, W]"""
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    B, C, H, W = x_freq.shape
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def frequency_set(n):
    """the frequencies of one axis inside the threshold-1 box, as a set: {0} for a side of 1, both frequencies for a side of 2"""
    return sorted({0, (-1) % n})


def fourier_filter(x, scale):
    """closed form of fourier_filter_fft(x, 1, scale): x [B, C, H, W]; computed in x's dtype"""
    B, C, H, W = x.shape
    y = torch.arange(H, dtype=x.dtype).view(H, 1)
    xx = torch.arange(W, dtype=x.dtype).view(1, W)
    low = torch.zeros_like(x)
    for ky in frequency_set(H):
        for kx in frequency_set(W):
            ang = 2 * math.pi * (ky * y / H + kx * xx / W)
            cs, sn = torch.cos(ang), torch.sin(ang)
            re = (x * cs).sum((-2, -1), keepdim=True)           # X = sum v e^{-i ang}
            im = -(x * sn).sum((-2, -1), keepdim=True)
            low = low + (re * cs - im * sn)                     # Re(X e^{+i ang})
    return x + (scale - 1.0) * low / (H * W)


def backbone_factor_published(h, b):
    """version 2's lines as published (NaN where max == min): h [B, C, H, W] -> [B, 1, H, W]"""
    hidden_mean = h.mean(1).unsqueeze(1)
    B = hidden_mean.shape[0]
    hidden_max, _ = torch.max(hidden_mean.view(B, -1), dim=-1, keepdim=True)
    hidden_min, _ = torch.min(hidden_mean.view(B, -1), dim=-1, keepdim=True)
    hidden_mean = (hidden_mean - hidden_min.unsqueeze(2).unsqueeze(3)) / (hidden_max - hidden_min).unsqueeze(2).unsqueeze(3)
    return (b - 1) * hidden_mean + 1


def backbone_factor(h, b, version):
    if version == 1:
        return torch.full_like(h[:, :1], b)
    m = h.mean(1, keepdim=True)
    mn = m.amin((-2, -1), keepdim=True)
    mx = m.amax((-2, -1), keepdim=True)
    rng = mx - mn
    t = (m - mn) / torch.where(rng > 0, rng, torch.ones_like(rng))
    return torch.where(rng > 0, (b - 1) * t + 1, torch.ones_like(t))


def apply_site(h, skip, b, s, version):
    """one site: channels [0, C/2) of h times the factor, skip through the filter"""
    half = h.shape[1] // 2
    h = torch.cat([h[:, :half] * backbone_factor(h, b, version), h[:, half:]], 1)
    return h, fourier_filter(skip, s)


def site_stage(h_ch, skip_ch, mc):
    if h_ch == skip_ch == 4 * mc:
        return 1
    if h_ch == skip_ch == 2 * mc:
        return 2
    return 0


def decoder_pairs(unet, hw=(8, 8)):
    """(backbone channels, skip channels) of every output block in pop order, from a meta-device forward of the oracle's own modules"""
    with torch.device('meta'):
        x = torch.zeros(1, 4, *hw)
        emb = unet.time_embed(S.timestep_embedding(torch.zeros(1), unet.model_ch))
        ctx = torch.zeros(1, 77, 768)
        hs, h = [], x
        for m in unet.input_blocks:
            h = m(h, emb, ctx)
            hs.append(h)
        h = unet.middle_block(h, emb, ctx)
        pairs = []
        for m in unet.output_blocks:
            sk = hs.pop()
            pairs.append((h.shape[1], sk.shape[1]))
            h = m(torch.cat([h, sk], 1), emb, ctx)
    return pairs


def freeu_unet(unet, x, timesteps, context, b1, b2, s1, s2, version=2, control=None, round_sites=False):
    """UNetModel.forward with FreeU; control = (13 fp32 NCHW residuals, 13 scales) applies cldm's additions first (ComfyUI's order).
    round_sites: the two tensors of every site are rounded to fp16 before FreeU acts (the sensitivity probe of the GPU test)."""
    mc = unet.model_ch
    emb = unet.time_embed(S.timestep_embedding(timesteps, mc))
    hs, h = [], x
    for m in unet.input_blocks:
        h = m(h, emb, context)
        hs.append(h)
    h = unet.middle_block(h, emb, context)
    res = None
    if control is not None:
        res = [float(sc) * c for sc, c in zip(control[1], control[0])]
        h = h + res.pop()
    for m in unet.output_blocks:
        sk = hs.pop()
        if res is not None:
            sk = sk + res.pop()
        stage = site_stage(h.shape[1], sk.shape[1], mc)
        if stage:
            if round_sites:
                h, sk = h.half().float(), sk.half().float()
            h, sk = apply_site(h, sk, b1 if stage == 1 else b2, s1 if stage == 1 else s2, version)
        h = m(torch.cat([h, sk], dim=1), emb, context)
    return unet.out(h)


class FreeUModel:
    """the fp32 chain's model for the sampler restatements: unet(x, t, ctx) with FreeU"""

    def __init__(self, unet, b1, b2, s1, s2, version=2):
        self.unet, self.args = unet, (b1, b2, s1, s2, version)

    def __call__(self, x, t, ctx):
        with torch.no_grad():
            return freeu_unet(self.unet, x, t, ctx, *self.args)
