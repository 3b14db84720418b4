"""Rectangular latents on the GPU: the UNet, VAE decoder and VAE encoder graphs at (16, 24) and (8, 16) -- the second has a 1 x 2
deepest level, the smallest size the rule admits -- against the fp32 oracle, and the pipeline's entry points at (16, 24).

Stated tolerances (fp16 GPU vs fp32 CPU): one UNet evaluation rel-L2 <= 5e-3; VAE decode rel-L2 <= 1e-2 (test_engine_gpu.py); VAE
encoder mean / logvar rel-L2 <= 3e-3 each (test_img2img_gpu.py); the 20-step PLMS chain: trace exact, final latent rel-L2 <= 2e-2,
>= 99 % of the bytes within 2 LSB (test_pipeline_gpu.py).  Bit-exact: eager against the hip-graph replay, every *_graphed entry point
against its eager form, latent_hw=16 against latent_hw=(16, 16)."""
import numpy as np
import pytest
import torch

from test_img2img_cpu import LdmEncoder

pytestmark = pytest.mark.gpu

HW = (16, 24)


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope='module')
def sds():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(*HW)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table(),
              'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    return {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}


@pytest.fixture(scope='module')
def oracles(sds):
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet, vae, enc = S.UNetModel(), S.AutoencoderKLDecode(), LdmEncoder()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    enc.load_state_dict(sds['vae_enc'], assign=True)
    return unet.eval(), vae.eval(), enc.eval()


@pytest.fixture(scope='module')
def unet_inputs():
    g = torch.Generator().manual_seed(21)
    return {hw: torch.randn(2, 4, *hw, generator=g) for hw in ((16, 24), (8, 16))}, torch.randn(2, 77, 768, generator=g).half(), \
        torch.tensor([999.0, 251.0])


_unet_out = {}


def _run_unet(sds, hw, x, ctx, t):
    from sdod.amd import engine as E
    cfg = E.sd14_config(*hw)
    g = E.UNet(cfg, 2)
    g.load_state_dict(sds['unet'])
    g.finalize()
    tg = E.Temb(cfg, 2)
    tg.load_state_dict(sds['temb'])
    tg.finalize()
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    g.execute()
    torch.cuda.synchronize()
    eager = g.eps.clone()
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True, static_unchanged=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.eps), 'hipGraph replay differs from eager execution'
    g.check()
    assert eager.shape == (2,) + tuple(hw) + (4,)
    return eager.float().cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize('hw', [(16, 24), (8, 16)])
def test_unet_rectangular_matches_oracle(sds, oracles, unet_inputs, hw):
    xs, ctx, t = unet_inputs
    out = _run_unet(sds, hw, xs[hw], ctx, t)
    _unet_out[hw] = out
    with torch.no_grad():
        ref = oracles[0](xs[hw], t, ctx.float())
    r = rel_l2(out, ref)
    print(f'unet {hw} b2 rel-L2 {r:.3e}')
    assert torch.isfinite(out).all() and r <= 5e-3, r


def test_unet_transposed_size_is_not_the_transpose(sds, oracles, unet_inputs):
    """(24, 16) on the transposed input: finite, and NOT the (16, 24) result transposed (the convolutions' taps are not symmetric) --
    an h / w swap anywhere in the builder would make the two coincide or read out of its rows"""
    xs, ctx, t = unet_inputs
    xt = xs[(16, 24)].transpose(2, 3).contiguous()
    out = _run_unet(sds, (24, 16), xt, ctx, t)
    assert out.shape == (2, 4, 24, 16) and torch.isfinite(out).all()
    wide = _unet_out[(16, 24)] if (16, 24) in _unet_out else _run_unet(sds, (16, 24), xs[(16, 24)], ctx, t)
    assert rel_l2(out, wide.transpose(2, 3)) > 0.05
    with torch.no_grad():
        ref = oracles[0](xt, t, ctx.float())
    r = rel_l2(out, ref)
    print(f'unet (24, 16) b2 rel-L2 {r:.3e}')
    assert r <= 5e-3, r


def test_vae_decoder_rectangular(sds, oracles):
    from sdod.amd import engine as E
    g = E.VaeDecoder(E.sd14_config(8, 16), 1)
    g.load_state_dict(sds['vae'])
    g.finalize()
    z = torch.randn(1, 4, 8, 16, generator=torch.Generator().manual_seed(12)) * 0.18215 * 4
    with torch.no_grad():
        ref = oracles[1](z)
    g.z.copy_(z)
    g.execute()
    torch.cuda.synchronize()
    eager = g.img.clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.img)
    out = eager.float().cpu().permute(0, 3, 1, 2)
    r = rel_l2(out, ref)
    print('vae decoder (8, 16) rel-L2', r)
    assert out.shape == (1, 3, 64, 128) and torch.isfinite(out).all() and r <= 1e-2, r


def _image(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(float(h)), torch.arange(float(w)), indexing='ij')
    img = torch.stack([128 + 90 * torch.sin(xx / 11 + k) * torch.cos(yy / 17) for k in range(3)], -1)
    return (img + 10 * torch.randn(h, w, 3, generator=g)).clamp(0, 255).to(torch.uint8)[None]


def test_vae_encoder_rectangular(sds, oracles):
    from sdod.amd import engine as E
    g = E.VaeEncoder(E.sd14_config(*HW), 1)
    g.load_state_dict(sds['vae_enc'])
    g.finalize()
    u8 = _image(128, 192, 8)
    with torch.no_grad():
        ref = oracles[2]((2.0 * (u8.float() / 255.0) - 1.0).half().float().permute(0, 3, 1, 2))
    g.img.copy_(u8)
    g.execute()
    torch.cuda.synchronize()
    out = g.moments.cpu().clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.moments.cpu(), out)
    r_mean, r_logvar = rel_l2(out[:, :4], ref[:, :4]), rel_l2(out[:, 4:], ref[:, 4:])
    print(f'VAE encoder 128 x 192: mean rel-L2 {r_mean:.2e}, logvar rel-L2 {r_logvar:.2e}')
    assert out.shape == (1, 8, 16, 24) and torch.isfinite(out).all()
    assert r_mean <= 3e-3 and r_logvar <= 3e-3, (r_mean, r_logvar)


# ------------------------------------------------------------------ the pipeline at (16, 24)
@pytest.fixture(scope='module')
def rig(sds):
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=HW, with_text_encoder=False, with_vae_encoder=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, *HW, generator=g)
    n1, n2 = torch.randn(1, 4, *HW, generator=g), torch.randn(1, 4, *HW, generator=g)
    return pipe, ctx2, x_T, _image(128, 192, 5), (n1, n2)


def test_plms_20_steps_rectangular_matches_oracle(rig, oracles):
    from oracle import pipeline_oracle as PO
    pipe, ctx2, x_T, _, _ = rig
    unet, vae, _ = oracles
    assert pipe._latent_shape == (4, 16, 24)
    tr_gpu, tr_cpu = [], []
    z = pipe.sample_plms(ctx2.cuda(), x_T, steps=20, guidance=7.5, trace=tr_gpu)
    c16 = ctx2.float()
    z_ref = PO.plms_sample(unet, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5, trace=tr_cpu)
    assert tr_gpu == tr_cpu
    r = rel_l2(z.cpu(), z_ref)
    print('plms (16, 24) final latent rel-L2', r)
    assert z.shape == (1, 4, 16, 24) and torch.isfinite(z).all() and r <= 2e-2, r
    img = pipe.decode(z, mode=1).cpu().numpy()
    img_ref = PO.decode_u8(vae, z_ref, mode=1)
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 192, 3) and frac >= 0.99, frac


def test_graphed_forms_equal_eager_rectangular(rig):
    pipe, ctx2, x_T, u8, noise = rig
    c = ctx2.cuda()
    kw = dict(steps=6, guidance=7.5, sampler='dpmpp_2m', schedule='karras')
    eager = pipe.generate(c, x_T, **kw)
    assert eager.shape == (1, 128, 192, 3) and eager.dtype == torch.uint8
    assert torch.equal(pipe.generate_graphed(c, x_T, **kw), eager)
    kwa = dict(steps=4, guidance=7.5, sampler='euler_a', schedule='karras', seed=5, image_index=2)
    assert torch.equal(pipe.generate_graphed(c, x_T, **kwa), pipe.generate(c, x_T, **kwa))                 # step noise [3, 1, 4, 16, 24]
    img, ev = pipe.generate_pipelined(c, x_T, steps=4, guidance=7.5, sampler='plms')
    ev.synchronize()
    assert torch.equal(img, pipe.generate(c, x_T, steps=4, guidance=7.5, sampler='plms'))
    x = pipe.encode(u8, strength=0.5, steps=10, noise=noise)
    assert x.shape == (1, 4, 16, 24) and torch.isfinite(x).all()
    e_i2i = pipe.img2img(c, u8, 0.5, 10, 7.5, noise=noise)
    assert e_i2i.shape == (1, 128, 192, 3)
    assert torch.equal(pipe.img2img_graphed(c, u8, 0.5, 10, 7.5, noise=noise), e_i2i)
    assert torch.equal(pipe.img2img_graphed(c, u8, 0.5, 10, 7.5, seed=31, image_index=3), pipe.img2img(c, u8, 0.5, 10, 7.5, seed=31, image_index=3))
    mask = torch.zeros(1, 128, 192, dtype=torch.uint8)
    mask[:, 24:100, 70:170] = 255
    mask[:, 40:60, 10:40] = 128
    e_inp = pipe.inpaint(c, u8, mask, 0.5, 10, 7.5, seed=7)
    assert e_inp.shape == (1, 128, 192, 3)
    assert torch.equal(e_inp.cpu()[mask == 0], u8[mask == 0])                   # kept pixels are the init image's
    assert not torch.equal(e_inp.cpu()[mask == 255], u8[mask == 255])
    assert torch.equal(pipe.inpaint_graphed(c, u8, mask, 0.5, 10, 7.5, seed=7), e_inp)
    for fn in (pipe.inpaint, pipe.inpaint_graphed):
        with pytest.raises(ValueError):
            fn(c, u8, torch.zeros(1, 128, 128, dtype=torch.uint8), 0.5, 10, 7.5)
    with pytest.raises(ValueError):
        pipe.generate(c, x_T, 4, 7.5, 'euler_a', step_noise=torch.zeros(3, 1, 4, 24, 16))
    pipe.unet.check()


def test_inpaint_concat_rectangular(sds):
    """the 9-channel entry points at (16, 24): the conditioning launch and the fused concat input convolution on a rectangle"""
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    sd9 = Wt.synthetic_state_dict(E.UNet(E.sd14_config(*HW, concat_channels=5), 2).param_table(), seed=1234)
    pipe = Txt2Img(state_dicts={**sds, 'unet': sd9}, images_per_gpu=1, latent_hw=HW, with_text_encoder=False, inpaint_unet=True)
    g = torch.Generator().manual_seed(78)
    c = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, *HW, generator=g)
    u8 = _image(128, 192, 6)
    mask = torch.zeros(1, 128, 192, dtype=torch.uint8)
    mask[:, 30:90, 100:180] = 255
    eager = pipe.inpaint_concat(c, u8, mask, x_T, 4, 7.5, 'plms', seed=3)
    assert eager.shape == (1, 128, 192, 3)
    assert torch.equal(eager.cpu()[mask == 0], u8[mask == 0])
    assert pipe.unet.cond.shape == (2, 5, 16, 24)
    assert torch.equal(pipe.unet.cond[:, 0].cpu(), (mask[:, ::8, ::8] >= 128).float().expand(2, -1, -1))
    assert torch.equal(pipe.inpaint_concat_graphed(c, u8, mask, x_T, 4, 7.5, 'plms', seed=3), eager)
    with pytest.raises(ValueError):
        pipe.inpaint_concat(c, u8, torch.zeros(1, 128, 128, dtype=torch.uint8), x_T, 4, 7.5, 'plms')


def test_integer_latent_hw_is_the_square_pair(sds):
    from sdod.amd.pipeline import Txt2Img
    g = torch.Generator().manual_seed(79)
    c = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    outs = []
    for hw in (16, (16, 16)):
        pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=hw, with_text_encoder=False)
        assert pipe.hires is None and pipe._latent_shape == (4, 16, 16)
        outs.append((pipe.generate(c, x_T, steps=4, guidance=7.5, sampler='plms').cpu(), [o[0] for o in pipe.unet.op_table()], pipe.unet.stats()))
        del pipe
    assert outs[0][0].shape == (1, 128, 128, 3)
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2]
