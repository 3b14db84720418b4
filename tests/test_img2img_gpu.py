"""img2img on the GPU: the kernels it adds (asymmetric-pad stride-2 convolution, fused image input convolution, the start-latent
kernel), the VAE encoder graph against the fp32 oracle (test_img2img_cpu.LdmEncoder), and the whole chain (encoder ->
stochastic_encode -> ldm DDIM decode -> uint8) against the CPU oracle with injected noise.

Stated tolerances (fp16 GPU vs fp32 CPU): convolutions rel-L2 <= 2e-3; encoder mean / logvar rel-L2 <= 3e-3 each; final latent
rel-L2 <= 2e-2 and >= 99 % of the uint8 pixels within 2 LSB (as the txt2img chain, test_pipeline_gpu.py).  Bit-exact: the fused
input convolution against its unfused launches, in-kernel noise against sdod_randn_f32, the graphed img2img against eager."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_img2img_cpu import LdmEncoder, ldm_img2img_indices

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------ asymmetric-pad stride-2 convolution
def _tiles_accepting(desc_fn):
    """tile ids the planner runs this convolution on when forced (halo-patch tiles must decline pad_mode)"""
    import ctypes
    from sdod.amd import _lib
    lib = _lib.hip()
    out = []
    for t in range(1, lib.sdod_gemm_num_tiles() + 1):
        d = desc_fn(t)
        info = (ctypes.c_int * 7)()
        lib.sdod_gemm_tile_info(t, info)
        if info[5] == 2:                                   # halo-patch tile: pad_mode 1 is stride 2, never taken
            assert lib.sdod_gemm_halo_ok(ctypes.byref(d), t) == 0
            continue
        if info[5] == 3:                                   # A-panel tile: rows only
            continue
        tile, splits = ctypes.c_int(), ctypes.c_int()
        assert lib.sdod_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(splits)) == 0
        if tile.value == t:
            out.append(t)
    return out


@pytest.mark.parametrize('n,h,w,c', [(1, 512, 512, 128), (1, 256, 256, 256), (1, 128, 128, 512), (2, 37, 45, 64)])
def test_downsample_conv_pad_mode_matches_ldm(n, h, w, c):
    """conv=dict(stride=2, pad_mode=1) == F.conv2d(F.pad(x, (0, 1, 0, 1)), stride=2) on every tile the planner takes, and far from
    the symmetric-pad convolution (so the padding is exercised)"""
    from sdod.amd import ops
    from sdod.amd._lib import GemmDesc
    g = torch.Generator().manual_seed(h * 7 + c)
    x = torch.randn(n, c, h, w, generator=g).half()
    wt = (torch.randn(c, c, 3, 3, generator=g) / (3 * c ** 0.5)).half()
    b = (0.1 * torch.randn(c, generator=g))
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), b, stride=2).permute(0, 2, 3, 1)
    sym = F.conv2d(x.float(), wt.float(), b, stride=2, padding=1).permute(0, 2, 3, 1)
    ho, wo = (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1
    assert ref.shape == (n, ho, wo, c)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    wk = wt.permute(0, 2, 3, 1).reshape(c, 9 * c).contiguous().cuda()
    bd = b.cuda()

    def desc(t):
        d = GemmDesc()
        d.M, d.N, d.K = n * ho * wo, c, 9 * c
        d.ldw = d.ldo = 9 * c
        d.ldo = c
        d.a_mode = 1
        d.n_img, d.h_in, d.w_in, d.c0, d.c1 = n, h, w, c, 0
        d.stride, d.ksize, d.pad_mode, d.tile = 2, 3, 1, t
        return d

    tiles = _tiles_accepting(desc)
    assert tiles, 'no tile takes the convolution'
    out = ops.gemm(xd, wk, bd, conv=dict(stride=2, pad_mode=1))
    assert out.shape == (n, ho, wo, c)
    r = rel_l2(out.float().cpu(), ref)
    assert r <= 2e-3, ('auto', r)
    if sym.shape == ref.shape:                                       # (odd sizes: the symmetric conv has one more row / column)
        assert rel_l2(sym, ref) > 0.05
        assert rel_l2(out.float().cpu(), sym) > 0.05
    for t in tiles:
        o = ops.gemm(xd, wk, bd, conv=dict(stride=2, pad_mode=1), tile=t)
        r = rel_l2(o.float().cpu(), ref)
        assert r <= 2e-3, (t, r)


def test_pad_mode_refused_where_it_cannot_apply():
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    x = torch.zeros(1, 16, 16, 64, dtype=torch.float16, device='cuda')
    wk = torch.zeros(64, 576, dtype=torch.float16, device='cuda')
    with pytest.raises(SdodError):
        ops.gemm(x, wk, conv=dict(stride=1, pad_mode=1))            # pad_mode 1 is the stride-2 Downsample only
    with pytest.raises(SdodError):
        ops.gemm(x, wk, conv=dict(stride=2, pad_mode=1), tile=37)   # halo-patch tile: declined


# ------------------------------------------------------------------ fused image input convolution
@pytest.mark.parametrize('n,h,w,cout', [(1, 512, 512, 128), (2, 37, 29, 128), (1, 128, 128, 64)])
def test_image_conv_in_equals_normalise_im2col_gemm(n, h, w, cout):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(n * 100 + h)
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    wt = (torch.randn(cout, 3, 3, 3, generator=g) / 5).half()
    bias = 0.1 * torch.randn(cout, generator=g)
    wk = torch.zeros(cout, 64, dtype=torch.float16)
    wk[:, :27] = wt.permute(0, 2, 3, 1).reshape(cout, 27)              # k = tap * 3 + channel
    wk, bd = wk.cuda(), bias.cuda()
    out = ops.image_conv_in(u8.cuda(), wk, bd)
    x16 = (2.0 * (u8.float() / 255.0) - 1.0).half()                   # NHWC fp16, ldm's normalisation rounded once
    two = ops.gemm(ops.im2col3x3_small(x16.cuda(), 64), wk, bd).view(n, h, w, cout)
    assert torch.equal(out, two)
    ref = F.conv2d(x16.float().permute(0, 3, 1, 2), wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    assert rel_l2(out.float().cpu(), ref) <= 2e-3


# ------------------------------------------------------------------ start latent
def test_encode_latent_noise_and_formula():
    from sdod.amd import ops
    n, c, h, w = 2, 4, 16, 24
    g = torch.Generator().manual_seed(11)
    mom = torch.randn(n, 2 * c, h, w, generator=g)
    mom[:, c:] *= 25.0                                                # logvar beyond both clamp bounds
    mom = mom.cuda()
    seed, idx0, sa, s1a = 123456789, 5, 0.61, 0.79
    z0 = torch.empty(n, c, h, w, device='cuda')
    x = ops.encode_latent(mom, sa, s1a, seed, idx0, z0=z0)
    n1 = torch.cat([ops.randn((1, c, h, w), seed, (1 << 32) | (idx0 + i), 'cuda') for i in range(n)])
    n2 = torch.cat([ops.randn((1, c, h, w), seed, (2 << 32) | (idx0 + i), 'cuda') for i in range(n)])
    z0b = torch.empty_like(z0)
    xb = ops.encode_latent(mom, sa, s1a, n1=n1, n2=n2, z0=z0b)
    assert torch.equal(x, xb) and torch.equal(z0, z0b)               # in-kernel draw == sdod_randn_f32 on the stated streams
    m = mom.cpu()
    mean, logvar = m[:, :c], torch.clamp(m[:, c:], -30.0, 20.0)
    z_ref = 0.18215 * (mean + torch.exp(0.5 * logvar) * n1.cpu())
    x_ref = torch.tensor(sa, dtype=torch.float32) * z_ref + torch.tensor(s1a, dtype=torch.float32) * n2.cpu()
    for got, want in ((z0b.cpu(), z_ref), (xb.cpu(), x_ref)):
        err = ((got - want).abs() / want.abs().clamp(min=1.0)).max()
        assert float(err) <= 1e-6, float(err)


# ------------------------------------------------------------------ VAE encoder graph
@pytest.fixture(scope='module')
def enc64():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(64, 64)
    table = E.VaeEncoder(cfg, 1).param_table()
    sd = Wt.synthetic_state_dict(table, seed=1238)
    with torch.device('meta'):
        oracle = LdmEncoder()
    oracle.load_state_dict(sd, assign=True)
    oracle.eval()
    g = torch.Generator().manual_seed(8)
    yy, xx = torch.meshgrid(torch.arange(512.), torch.arange(512.), indexing='ij')
    smooth = torch.stack([128 + 100 * torch.sin(xx / 37 + k) * torch.cos(yy / 53 - k) for k in range(3)], -1)
    u8 = torch.stack([smooth, smooth.flip(0)]) + 20 * torch.randn(2, 512, 512, 3, generator=g)
    u8 = u8.clamp(0, 255).to(torch.uint8)
    with torch.no_grad():
        ref = oracle((2.0 * (u8.float() / 255.0) - 1.0).half().float().permute(0, 3, 1, 2))
    return cfg, sd, u8, ref


@pytest.mark.parametrize('batch', [1, 2])
def test_vae_encoder_64_matches_oracle(enc64, batch):
    from sdod.amd import engine as E
    cfg, sd, u8, ref = enc64
    g = E.VaeEncoder(cfg, batch)
    g.load_state_dict(sd)
    g.finalize()
    g.img.copy_(u8[:batch])
    g.execute()
    torch.cuda.synchronize()
    out = g.moments.cpu().clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.moments.cpu(), out)
    r_mean, r_logvar = rel_l2(out[:, :4], ref[:batch, :4]), rel_l2(out[:, 4:], ref[:batch, 4:])
    st = g.stats()
    print(f'VAE encoder 512px b{batch}: mean rel-L2 {r_mean:.2e}, logvar rel-L2 {r_logvar:.2e}, {st["launches"]} launches')
    assert torch.isfinite(out).all()
    assert r_mean <= 3e-3 and r_logvar <= 3e-3, (r_mean, r_logvar)


# ------------------------------------------------------------------ the whole chain at latent 16
@pytest.fixture(scope='module')
def rig16():
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
    return pipe, unet.eval(), vae.eval(), enc.eval(), ctx2, u8, (n1, n2)


@torch.no_grad()
def _oracle_img2img(unet, vae, enc, ctx2, u8, noise, strength, steps, guidance):
    """ldm scripts/img2img.py restated in fp32: encode_first_stage -> sample -> get_first_stage_encoding -> stochastic_encode
    -> DDIMSampler.decode (eta 0, CFG) -> decode_first_stage -> 255 clamp((x + 1) / 2)"""
    from oracle import pipeline_oracle as PO
    t_enc, seq, sa, s1a = ldm_img2img_indices(strength, steps)
    moments = enc((2.0 * (u8.float() / 255.0) - 1.0).half().float().permute(0, 3, 1, 2))
    mean, logvar = torch.chunk(moments, 2, dim=1)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    z0 = 0.18215 * (mean + std * noise[0])
    x = sa * z0 + s1a * noise[1]
    ac = torch.tensor(PO._alphas_cumprod(), dtype=torch.float32)
    c = 1000 // steps
    ddim_t = np.asarray(list(range(0, 1000, c))) + 1
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
    return x, PO.decode_u8(vae, x, mode=1), seq


def test_img2img_chain_matches_oracle(rig16):
    pipe, unet, vae, enc, ctx2, u8, noise = rig16
    strength, steps, guidance = 0.5, 20, 7.5
    z_ref, img_ref, seq = _oracle_img2img(unet, vae, enc, ctx2, u8, noise, strength, steps, guidance)
    from sdod.amd.pipeline import img2img_schedule
    _, t_enc = img2img_schedule(strength, steps)
    x = pipe.encode(u8, strength=strength, steps=steps, noise=noise)
    trace = []
    z = pipe.sample_ddim_from(ctx2.cuda(), x, t_enc, steps, guidance, trace=trace)
    assert trace == seq                                              # timestep / index sequence: exact
    r = rel_l2(z.cpu(), z_ref)
    print('img2img final latent rel-L2', r)
    assert torch.isfinite(z).all() and r <= 2e-2, r
    img = pipe.img2img(ctx2.cuda(), u8, strength, steps, guidance, noise=noise).cpu().numpy()
    assert torch.equal(torch.from_numpy(img), pipe.decode(z, mode=1).cpu())
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 128, 3) and frac >= 0.99, frac


def test_img2img_graphed_equals_eager(rig16):
    pipe, unet, vae, enc, ctx2, u8, noise = rig16
    c = ctx2.cuda()
    eager = pipe.img2img(c, u8, 0.5, 20, 7.5, noise=noise)
    graphed = pipe.img2img_graphed(c, u8, 0.5, 20, 7.5, noise=noise).clone()   # (the replay's output buffer is reused)
    assert torch.equal(graphed, eager)
    # device noise: the graph takes it as an input drawn on the same streams the eager path draws in the kernel
    eager2 = pipe.img2img(c, u8, 0.5, 20, 7.5, seed=31, image_index=3)
    graphed2 = pipe.img2img_graphed(c, u8, 0.5, 20, 7.5, seed=31, image_index=3)
    assert torch.equal(graphed2, eager2)
    assert not torch.equal(graphed2, graphed)
    with pytest.raises(ValueError):
        pipe.img2img(c, u8, 1.0, 20, 7.5)
