"""Inpainting checkpoints (9-channel UNet) on the GPU: the kernels this adds against fp32 torch / the launches they fuse, the graphs
against the fp32 oracles, and the whole chain (masked encoder -> conditioning -> PLMS or DPM-Solver++ from pure noise -> decode ->
pixel composite) against the fp32 restatement of the definition in tests/test_inpaint_concat_cpu.py, with injected x_T and noise.

Stated tolerances, all of them the project's own for the same kind of comparison: one convolution kernel against fp32 F.conv2d on
the fp16-rounded operands rel-L2 <= 2e-3 (test_kernels_gpu.py, test_img2img_gpu.py); one UNet evaluation rel-L2 <= 1e-2
(test_engine_gpu.py); encoder moments rel-L2 <= 3e-3 each (test_img2img_gpu.py); the chain: final latent rel-L2 <= 2e-2 and >= 99 %
of the uint8 pixels within 2 LSB (test_pipeline_gpu.py).  Everything else is bit-exact."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_img2img_cpu import LdmEncoder
from test_inpaint_concat_cpu import binarise, concat_conditioning, concat_unet, latent_mask, mask128, mask_census, masked_image

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _pack(wt, kpad):
    """[cout, cin, 3, 3] -> the PK_CONV3_SMALL rows [cout, kpad]: k = tap * cin + channel, zero beyond 9 cin"""
    cout, cin = wt.shape[:2]
    wk = torch.zeros(cout, kpad, dtype=torch.float16)
    wk[:, :9 * cin] = wt.half().permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    return wk


# ------------------------------------------------------------------ the two-source input convolution
@pytest.mark.parametrize('cout', [64, 128, 256, 320])
@pytest.mark.parametrize('n,h,w', [(1, 5, 7), (4, 5, 7), (1, 16, 16), (4, 9, 11), (1, 64, 64), (4, 64, 64)])
def test_conv_in_cat_matches_conv2d_and_the_two_launch_form(n, h, w, cout):
    """sdod_conv_in_cat_f16 (x | cond read in place, K = 81 -> 96, three MFMA K steps) and the two-launch form on the same packed
    weights (im2col of the materialised 9-channel tensor to kpad = 128, then the K = 128 GEMM), each against fp32 F.conv2d on the
    fp16-rounded operands: rel-L2 <= 2e-3.  5 x 7 and 9 x 11 end in a partial pixel tile (35, 140, 99, 396 rows).
    The pair itself: both accumulate each output in fp32 over k ascending in blocks of 32 (the GEMM's K = 64 slab is two
    v_mfma_f32_16x16x32_f16 steps, its last 32 columns are zeros), and within a block the MFMA's own order; equality is asserted."""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + cout)
    x = torch.randn(n, 4, h, w, generator=g)
    cond = torch.randn(n, 5, h, w, generator=g)
    cond[:, 0] = (cond[:, 0] > 0).float()                                 # a 0 / 1 mask channel, as in use
    wt = (torch.randn(cout, 9, 3, 3, generator=g) / 9).half()
    bias = torch.randn(cout, generator=g)
    wk = _pack(wt, 128).cuda()
    out = ops.conv_in_cat(x.cuda(), cond.cuda(), wk, bias.cuda())
    cat = torch.cat([x, cond], 1)
    ref = F.conv2d(cat.half().float(), wt.float(), bias, padding=1).permute(0, 2, 3, 1)
    r1 = rel_l2(out.float().cpu(), ref)
    two = ops.gemm(ops.latent_im2col(cat.cuda().contiguous(), 128, 1.0), wk, bias.cuda()).view(n, h, w, cout)
    r2 = rel_l2(two.float().cpu(), ref)
    r12 = rel_l2(out.float().cpu(), two.float().cpu())
    print(f'conv_in_cat {n}x{h}x{w} -> {cout}: one launch rel-L2 {r1:.2e}, im2col + GEMM {r2:.2e}, between them {r12:.2e}')
    assert out.shape == (n, h, w, cout) and torch.isfinite(out).all()
    assert r1 <= 2e-3 and r2 <= 2e-3, (r1, r2)
    assert torch.equal(out, two), r12
    # columns 96..127 of the packed rows are neither loaded nor multiplied: NaNs there change nothing
    wk2 = wk.clone()
    wk2[:, 96:] = float('nan')
    assert torch.equal(ops.conv_in_cat(x.cuda(), cond.cuda(), wk2, bias.cuda()), out)


def test_conv_in_cat_refuses_what_it_cannot_do():
    from sdod.amd import _lib
    lib = _lib.hip()
    x = torch.zeros(1, 4, 8, 8, device='cuda'); cond = torch.zeros(1, 5, 8, 8, device='cuda')
    w = torch.zeros(320, 128, dtype=torch.float16, device='cuda'); b = torch.zeros(320, device='cuda')
    y = torch.full((1, 8, 8, 320), 7.0, dtype=torch.float16, device='cuda')
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for c, cc, cout in ((4, 3, 320), (4, 7, 320), (4, 5, 192)):          # 9 * 7 <= 64, 9 * 11 > 96, an unsupported Cout
        assert lib.sdod_conv_in_cat_f16(P(x), P(cond), P(w), P(b), P(y), 1, 8, 8, c, cc, cout, None) != 0
    assert lib.sdod_conv_in_cat_f16(P(x), None, P(w), P(b), P(y), 1, 8, 8, 4, 5, 320, None) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@pytest.mark.parametrize('n,h,w,cout', [(1, 16, 16, 128), (2, 13, 9, 64), (1, 128, 128, 128), (1, 24, 40, 320)])
def test_masked_image_conv_in(n, h, w, cout):
    """all-zero mask: sdod_image_conv_in_f16 bit for bit; random mask: the K = 64 GEMM on an im2col of the fp16 masked image built in
    torch, bit for bit (0.0 where mask >= 128)"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(n * 100 + h)
    u8 = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    mask = torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8)
    mask[0, :2, :3] = torch.tensor([[127, 128, 129], [0, 255, 128]], dtype=torch.uint8)      # both sides of the threshold
    wt = (torch.randn(cout, 3, 3, 3, generator=g) / 5).half()
    bias = (0.1 * torch.randn(cout, generator=g)).cuda()
    wk = _pack(wt, 64).cuda()
    zero = torch.zeros_like(mask)
    assert torch.equal(ops.masked_image_conv_in(u8.cuda(), zero.cuda(), wk, bias), ops.image_conv_in(u8.cuda(), wk, bias))
    out = ops.masked_image_conv_in(u8.cuda(), mask.cuda(), wk, bias)
    x16 = (2.0 * (u8.float() / 255.0) - 1.0).half()
    x16[mask >= 128] = 0.0
    assert torch.equal(x16.float(), masked_image(u8, mask).permute(0, 2, 3, 1).half().float())   # the restatement, rounded once
    two = ops.gemm(ops.im2col3x3_small(x16.cuda(), 64), wk, bias).view(n, h, w, cout)
    assert torch.equal(out, two)
    assert not torch.equal(out, ops.image_conv_in(u8.cuda(), wk, bias))
    full = torch.full_like(mask, 255)
    only_bias = ops.masked_image_conv_in(u8.cuda(), full.cuda(), wk, bias)            # an all-zero image: the bias
    assert torch.equal(only_bias, bias.half().expand(n, h, w, cout))


# ------------------------------------------------------------------ the conditioning launch
@pytest.mark.parametrize('n,h,w', [(1, 16, 16), (2, 16, 24), (1, 64, 64), (3, 6, 10)])
def test_inpaint_cond_bit_exact(n, h, w):
    from sdod.amd import ops
    c = 4
    g = torch.Generator().manual_seed(n * 10 + w)
    mom = torch.randn(n, 2 * c, h, w, generator=g)
    mom[:, c:] *= 25.0                                                # logvar beyond both clamp bounds
    mom = mom.cuda()
    mask = torch.randint(0, 256, (n, 8 * h, 8 * w), generator=g, dtype=torch.uint8)
    n1 = torch.randn(n, c, h, w, generator=g).cuda()
    seed, idx0 = 123456789, 5
    out = ops.inpaint_cond(mom, mask.cuda(), n1=n1)
    assert out.shape == (n, 1 + c, h, w) and out.dtype == torch.float32
    want0 = (mask.numpy()[:, ::8, ::8] >= 128).astype(np.float32)
    assert np.array_equal(out[:, 0].cpu().numpy().view(np.uint32), want0.view(np.uint32))
    assert torch.equal(out[:, 0].cpu(), latent_mask(mask))
    z0 = torch.empty(n, c, h, w, device='cuda')
    ops.encode_latent(mom, 0.6, 0.8, n1=n1, n2=n1, z0=z0)
    assert torch.equal(out[:, 1:].contiguous().view(torch.int32), z0.view(torch.int32))
    # drawn noise == injected sdod_randn_f32 on stream (1 << 32) | (image_index + i)
    drawn = ops.inpaint_cond(mom, mask.cuda(), seed=seed, image_index=idx0)
    inj = torch.cat([ops.randn((1, c, h, w), seed, (1 << 32) | (idx0 + i), 'cuda') for i in range(n)])
    assert torch.equal(drawn, ops.inpaint_cond(mom, mask.cuda(), n1=inj)) and not torch.equal(drawn, out)
    assert not torch.equal(drawn, ops.inpaint_cond(mom, mask.cuda(), seed=seed, image_index=idx0 + 1))
    # reps = 2: two identical copies, [reps][n][5][hw]
    dst = torch.full((2 * n, 1 + c, h, w), -3.0, device='cuda')
    ops.inpaint_cond(mom, mask.cuda(), n1=n1, out=dst, reps=2)
    assert torch.equal(dst[:n], out) and torch.equal(dst[n:], out)


def test_inpaint_cond_refuses_bad_arguments_and_leaves_the_destination_untouched():
    from sdod.amd import _lib
    lib = _lib.hip()
    n, c, h, w = 1, 4, 16, 16
    mom = torch.zeros(n, 2 * c, h, w, device='cuda')
    mask = torch.zeros(n, 8 * h, 8 * w, dtype=torch.uint8, device='cuda')
    big = torch.full((n * (1 + c) * h * w + 8,), 7.0, device='cuda')
    n1 = torch.zeros(n * c * h * w + 8, device='cuda')
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(mom_=mom, mask_=mask, n1_=None, dst=big, factor=8, reps=1, h_=h, w_=w):
        return lib.sdod_inpaint_cond_f32(P(mom_), P(mask_), P(n1_), P(dst), n, c, h_, w_, factor, reps, 0, 0, None)

    assert call(factor=4) != 0 and b'factor' in lib.sdod_hip_last_error()
    assert call(mom_=None) != 0
    assert call(mask_=None) != 0
    assert call(dst=None) != 0
    assert call(dst=big[1:]) != 0 and b'misaligned' in lib.sdod_hip_last_error()
    assert call(n1_=n1[1:]) != 0 and b'misaligned' in lib.sdod_hip_last_error()
    assert call(reps=0) != 0
    assert call(h_=3, w_=5) != 0                                       # hw % 4 != 0
    torch.cuda.synchronize()
    assert bool((big == 7.0).all())
    assert call(n1_=n1) == 0                                           # zero moments, zero noise: mask channel 0, latent channels 0
    torch.cuda.synchronize()
    assert bool((big[:n * (1 + c) * h * w] == 0.0).all()) and bool((big[n * (1 + c) * h * w:] == 7.0).all())


# ------------------------------------------------------------------ graphs
@pytest.fixture(scope='module')
def weights16():
    """synthetic weights at latent 16 for the 9-channel UNet and the other graphs (the rig16 recipe of test_inpaint_gpu.py)"""
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16, concat_channels=5)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'text': E.TextEncoder(cfg, 1).param_table(),
              'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    assert dict(tables['unet'])['input_blocks.0.0.weight'] == (320, 9, 3, 3)
    return {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}


def _eval_unet(g, tg, x, t, ctx, cond=None):
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    if cond is not None:
        g.cond.copy_(cond)
    g.execute()
    torch.cuda.synchronize()
    eager = g.eps.float().cpu().permute(0, 3, 1, 2).clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.eps.float().cpu().permute(0, 3, 1, 2), eager)
    return eager


def test_unet_9_channels_one_evaluation_and_the_packed_input_weights(weights16):
    from oracle import sd_torch as S
    from sdod.amd import engine as E
    sds = weights16
    cfg9, cfg4 = E.sd14_config(16, 16, concat_channels=5), E.sd14_config(16, 16)
    tg = E.Temb(cfg9, 2); tg.load_state_dict(sds['temb']); tg.finalize()
    g9 = E.UNet(cfg9, 2); g9.load_state_dict(sds['unet']); g9.finalize()
    assert tuple(g9.cond.shape) == (2, 5, 16, 16) and g9.cond.dtype == torch.float32
    assert tuple(g9.x.shape) == (2, 4, 16, 16) and tuple(g9.eps.shape) == (2, 16, 16, 4)        # inputs 0-2 and output 0 as before
    assert 'conv_in_cat' in [l for l, _, _ in g9.op_table()] and 'conv_in' not in [l for l, _, _ in g9.op_table()]
    # packed rows: [tap][channel] in columns 0..80, zero from 81 to 127
    w9 = sds['unet']['input_blocks.0.0.weight']
    packed = g9.packed_param('input_blocks.0.0.weight').cpu().view(320, 128)
    assert torch.equal(packed, _pack(w9, 128)) and bool((packed[:, 81:] == 0).all()) and bool((packed[:, :81] != 0).any())
    with torch.device('meta'):
        unet9 = S.UNetModel(in_ch=9)
    unet9.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 16, 16, generator=gen)
    cond = torch.randn(2, 5, 16, 16, generator=gen)
    cond[:, 0] = (cond[:, 0] > 0).float()
    ctx = torch.randn(2, 77, 768, generator=gen).half()
    t = torch.tensor([999.0, 501.0])
    with torch.no_grad():
        ref = unet9(torch.cat([x, cond], 1), t, ctx.float())
    out = _eval_unet(g9, tg, x, t, ctx, cond)
    r = rel_l2(out, ref)
    print(f'9-channel UNet b2 16x16: rel-L2 vs fp32 oracle {r:.3e}, {g9.stats()["launches"]} launches')
    assert torch.isfinite(out).all() and r <= 1e-2, r
    with torch.no_grad():                                                   # the conditioning is read: another cond, another output
        ref_b = unet9(torch.cat([x, cond.flip(0)], 1), t, ctx.float())
    out_b = _eval_unet(g9, tg, x, t, ctx, cond.flip(0).contiguous())
    assert rel_l2(out_b, ref_b) <= 1e-2 and rel_l2(out_b, out) > 1e-2
    del g9
    # cond = 0 and the five extra weight channels zero: the 4-channel graph on the remaining weights
    sd4 = dict(sds['unet']); sd4['input_blocks.0.0.weight'] = w9[:, :4].contiguous()
    sd9z = dict(sds['unet']); wz = w9.clone(); wz[:, 4:] = 0; sd9z['input_blocks.0.0.weight'] = wz
    g4 = E.UNet(cfg4, 2); g4.load_state_dict(sd4); g4.finalize()
    assert not hasattr(g4, 'cond') and [l for l, _, _ in g4.op_table()].count('conv_in') == 1
    with pytest.raises(Exception):
        g4._io(False, 3)
    p4 = g4.packed_param('input_blocks.0.0.weight').cpu().view(320, 64)      # the 4-channel packing: today's bytes
    assert torch.equal(p4, _pack(w9[:, :4], 64))
    out4 = _eval_unet(g4, tg, x, t, ctx)
    del g4
    g9z = E.UNet(cfg9, 2); g9z.load_state_dict(sd9z); g9z.finalize()
    out9z = _eval_unet(g9z, tg, x, t, ctx, torch.zeros(2, 5, 16, 16))
    r = rel_l2(out9z, out4)
    print(f'9-channel graph with zero cond and zero extra weights vs the 4-channel graph: rel-L2 {r:.3e}')
    assert r <= 1e-2, r


@pytest.fixture(scope='module')
def rig9(weights16):
    from oracle import sd_torch as S
    from sdod.amd.pipeline import Txt2Img
    sds = weights16
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, with_text_encoder=False, inpaint_unet=True)
    with torch.device('meta'):
        unet9, vae, enc = S.UNetModel(in_ch=9), S.AutoencoderKLDecode(), LdmEncoder()
    unet9.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    enc.load_state_dict(sds['vae_enc'], assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    img = torch.stack([128 + 90 * torch.sin(xx / 11 + k) * torch.cos(yy / 17) for k in range(3)], -1)
    u8 = (img + 10 * torch.randn(128, 128, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]
    n1 = torch.randn(1, 4, 16, 16, generator=g)
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    mask = mask128()
    cond_ref, mom_ref = concat_conditioning(enc.eval(), u8, mask, n1)
    return dict(pipe=pipe, unet9=unet9.eval(), vae=vae.eval(), enc=enc, ctx2=ctx2, u8=u8, n1=n1, x_T=x_T, mask=mask, cond_ref=cond_ref,
                mom_ref=mom_ref)


def test_generate_needs_staged_conditioning(rig9):
    """runs first on the fresh pipeline: nothing staged yet"""
    r = rig9
    pipe = r['pipe']
    if not pipe._cond_staged:
        for fn in (pipe.generate, pipe.generate_graphed):
            with pytest.raises(RuntimeError, match='inpaint_concat'):
                fn(r['ctx2'].cuda(), r['x_T'])
    assert pipe.encoder is None and pipe.masked_encoder is not None and tuple(pipe.unet.cond.shape) == (2, 5, 16, 16)


def test_masked_encoder_and_conditioning_match_the_restatement(rig9):
    from sdod.amd import engine as E
    r = rig9
    pipe, u8, mask = r['pipe'], r['u8'], r['mask']
    plain = E.VaeEncoder(pipe.cfg, 1)
    pipe.stage_inpaint_cond(u8.cuda(), mask.cuda(), noise=r['n1'])
    torch.cuda.synchronize()
    mom = pipe.masked_encoder.moments.cpu()
    r_mean, r_logvar = rel_l2(mom[:, :4], r['mom_ref'][:, :4]), rel_l2(mom[:, 4:], r['mom_ref'][:, 4:])
    print(f'masked encoder 128px: mean rel-L2 {r_mean:.2e}, logvar rel-L2 {r_logvar:.2e}')
    assert torch.isfinite(mom).all() and r_mean <= 3e-3 and r_logvar <= 3e-3, (r_mean, r_logvar)
    cond = pipe.unet.cond.cpu()
    assert torch.equal(cond[0], cond[1])                                  # both guidance halves
    assert torch.equal(cond[:1, 0], r['cond_ref'][:, 0])                  # c_mask: exact
    print('c_lat rel-L2', rel_l2(cond[:1, 1:], r['cond_ref'][:, 1:]))
    ones, zeros, mixed = mask_census(mask)
    assert ones >= 64 and zeros >= 64 and mixed >= 1                      # both values of c_mask, an edge inside 8 x 8 blocks
    # an all-zero mask: the plain encoder's moments, bit for bit
    plain.load_state_dict(pipe._sd['vae_enc']); plain.finalize()
    plain.img.copy_(u8); plain.execute()
    pipe.masked_encoder.img.copy_(u8); pipe.masked_encoder.mask.zero_(); pipe.masked_encoder.execute()
    torch.cuda.synchronize()
    assert torch.equal(plain.moments, pipe.masked_encoder.moments)
    assert [l for l, _, _ in pipe.masked_encoder.op_table()][1:] == [l for l, _, _ in plain.op_table()][1:]
    assert plain.op_table()[0][0] == 'image_conv_in' and pipe.masked_encoder.op_table()[0][0] == 'masked_image_conv_in'


def _vae_img(pipe, z):
    pipe.vae.z.copy_(z)
    pipe.vae.execute(pipe.use_hip_graph)
    return pipe.vae.img


@pytest.mark.parametrize('sampler', ['plms', 'dpm'])
def test_inpaint_concat_chain_matches_the_restatement(rig9, oracle_lib, sampler):
    from oracle import pipeline_oracle as PO
    from sdod.amd import ops
    r = rig9
    pipe, ctx2, u8, mask, x_T, n1 = r['pipe'], r['ctx2'].cuda(), r['u8'], r['mask'], r['x_T'], r['n1']
    ones, zeros, mixed = mask_census(mask)
    assert ones >= 64 and zeros >= 64 and mixed >= 1
    model = concat_unet(r['unet9'], r['cond_ref'])
    c16 = r['ctx2'].float()
    if sampler == 'plms':
        z_ref = PO.plms_sample(model, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5)
    else:
        z_ref = PO.dpm_sample(model, oracle_lib, c16[0:1], c16[1:2], x_T, steps=20, guidance=7.5)
    d = PO.decode_u8(r['vae'], z_ref, mode=1).astype(np.int64)
    k = mask.numpy().astype(np.int64)[..., None]
    img_ref = ((d * k + u8.numpy().astype(np.int64) * (255 - k) + 127) // 255).astype(np.uint8)
    # the chain in its parts: conditioning, then the ordinary sampler
    pipe.stage_inpaint_cond(u8.cuda(), mask.cuda(), noise=n1)
    before = pipe.unet.cond.clone()
    z = pipe.sample_plms(ctx2, x_T, 20, 7.5) if sampler == 'plms' else pipe.sample_dpm(ctx2, x_T, 20, 7.5)
    assert torch.equal(pipe.unet.cond.view(torch.int32), before.view(torch.int32))        # static: no sampler launch writes there
    rl = rel_l2(z.cpu(), z_ref)
    print(f'inpaint_concat {sampler} final latent rel-L2', rl)
    assert torch.isfinite(z).all() and rl <= 2e-2, rl
    img = pipe.inpaint_concat(ctx2, u8, mask, x_T, 20, 7.5, sampler, noise=n1)
    assert torch.equal(pipe.unet.cond.view(torch.int32), before.view(torch.int32))
    assert torch.equal(img, ops.image_composite(_vae_img(pipe, z), u8.cuda(), mask.cuda()))
    img = img.cpu().numpy()
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 128, 3) and frac >= 0.99, frac
    m = mask.numpy()
    assert (m == 0).any() and np.array_equal(img[m == 0], u8.numpy()[m == 0])             # kept pixels: the init image's, bit for bit
    plain = pipe.inpaint_concat(ctx2, u8, mask, x_T, 20, 7.5, sampler, noise=n1, composite=False)
    assert torch.equal(plain, pipe.decode(z, mode=1))
    assert np.array_equal(img[m == 255], plain.cpu().numpy()[m == 255])
    # the conditioning matters: the inverted mask gives another latent
    inv = (255 - mask).contiguous()
    pipe.stage_inpaint_cond(u8.cuda(), inv.cuda(), noise=n1)
    z_inv = pipe.sample_plms(ctx2, x_T, 20, 7.5) if sampler == 'plms' else pipe.sample_dpm(ctx2, x_T, 20, 7.5)
    assert not torch.equal(pipe.unet.cond, before) and rel_l2(z_inv.cpu(), z.cpu()) > 2e-2


def test_inpaint_concat_graphed_equals_eager(rig9):
    r = rig9
    pipe, c, u8, mask, x_T, n1 = r['pipe'], r['ctx2'].cuda(), r['u8'], r['mask'], r['x_T'], r['n1']
    for sampler in ('plms', 'dpm'):
        eager = pipe.inpaint_concat(c, u8, mask, x_T, 20, 7.5, sampler, noise=n1)
        graphed = pipe.inpaint_concat_graphed(c, u8, mask, x_T, 20, 7.5, sampler, noise=n1).clone()
        assert torch.equal(graphed, eager), sampler
    # device noise: the graph takes it as an input drawn on the stream the eager path draws in its kernel
    eager2 = pipe.inpaint_concat(c, u8, mask, x_T, 20, 7.5, seed=31, image_index=3)
    graphed2 = pipe.inpaint_concat_graphed(c, u8, mask, x_T, 20, 7.5, seed=31, image_index=3).clone()
    assert torch.equal(graphed2, eager2)
    assert not torch.equal(graphed2, pipe.inpaint_concat(c, u8, mask, x_T, 20, 7.5, noise=n1))
    # the mask is an input of the graph: a replay with another mask of the same shape gives that mask's eager result
    other = mask.flip(2).contiguous()
    eager3 = pipe.inpaint_concat(c, u8, other, x_T, 20, 7.5, seed=31, image_index=3)
    n_graphs = len(pipe._traj)
    graphed3 = pipe.inpaint_concat_graphed(c, u8, other, x_T, 20, 7.5, seed=31, image_index=3).clone()
    assert len(pipe._traj) == n_graphs                                # a replay, not a new capture
    assert torch.equal(graphed3, eager3) and not torch.equal(graphed3, graphed2)
    plain = pipe.inpaint_concat_graphed(c, u8, mask, x_T, 20, 7.5, seed=31, image_index=3, composite=False).clone()
    assert torch.equal(plain, pipe.inpaint_concat(c, u8, mask, x_T, 20, 7.5, seed=31, image_index=3, composite=False))
    with pytest.raises(ValueError):
        pipe.inpaint_concat_graphed(c, u8, mask[:, :64], x_T)
    with pytest.raises(ValueError):
        pipe.inpaint_concat(c, u8, mask, x_T, sampler='ddim')


def test_a_pipeline_without_inpaint_unet_has_none_of_it(weights16):
    from sdod.amd.pipeline import Txt2Img
    sds = dict(weights16)
    sds['unet'] = dict(sds['unet'])
    sds['unet']['input_blocks.0.0.weight'] = sds['unet']['input_blocks.0.0.weight'][:, :4].contiguous()
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, with_text_encoder=False, with_vae=False)
    assert pipe.masked_encoder is None and pipe.encoder is None and not hasattr(pipe.unet, 'cond') and pipe.cfg.concat_channels == 0
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (1, 128, 128, 3), generator=g, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        pipe.inpaint_concat(None, u8, mask128(), torch.randn(1, 4, 16, 16, generator=g))
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    z = pipe.sample_plms(ctx2, torch.randn(1, 4, 16, 16, generator=g), 4, 7.5)               # and it samples without any conditioning
    assert torch.isfinite(z).all()
    # a 9-channel checkpoint does not load into it, nor a 4-channel one into an inpaint_unet pipeline
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    g4 = E.UNet(E.sd14_config(16, 16), 2)
    with pytest.raises(SdodError):
        g4.set_param('input_blocks.0.0.weight', weights16['unet']['input_blocks.0.0.weight'])
