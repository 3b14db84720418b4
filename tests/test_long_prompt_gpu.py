"""Long, weighted prompts on the GPU: sdod_context_assemble_f16 against fp64, the UNet graph with 154 / 231 / 308 cross-attention
keys against the CPU oracle, and a Txt2Img(prompt_chunks=2) pipeline end to end (16x16 latent, synthetic weights).

Tolerances.  Kernel: |out - ref| <= 2^-10 |ref| + 2^-24 -- one fp16 rounding (2^-11 relative, 2^-25 absolute below the normal range)
plus the fp32 error of the two sums, which the fixed-order summation keeps below 2^-11 at a conditioning sum|x| / |sum x| <= 16
(asserted on the inputs).  UNet evaluation: rel-L2 <= 1e-2; CLIP: rel-L2 <= 5e-3; 20-step PLMS: final latent rel-L2 <= 2e-2, images
within 2 LSB on >= 99 % of the pixels -- the project's stated tolerances for the same comparisons at 77 keys."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------ the kernel
def _kernel_inputs(shape, seed):
    p, k, t, d = shape
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(p, k, t, d, generator=gen) + 0.5).half()
    w = torch.rand(p, k, t, generator=gen) + 0.5
    return x, w


def _kernel_ref(x, w):
    """fp64 on the fp16 values: x w (sum x / sum x w) per (prompt, chunk); also the conditioning of both sums"""
    xd, wd = x.double(), w.double()[..., None]
    xw = xd * wd
    s0, s1 = xd.sum((2, 3), keepdim=True), xw.sum((2, 3), keepdim=True)
    cond = max(float((xd.abs().sum((2, 3), keepdim=True) / s0.abs()).max()), float((xw.abs().sum((2, 3), keepdim=True) / s1.abs()).max()))
    return xw * (s0 / s1), cond


@pytest.mark.parametrize('shape', [(2, 2, 77, 768), (1, 3, 77, 1024), (2, 1, 5, 72)])
def test_context_assemble_matches_fp64(shape):
    from sdod.amd import ops
    x, w = _kernel_inputs(shape, seed=sum(shape))
    ref, cond = _kernel_ref(x, w)
    assert cond <= 16.0, cond
    out = ops.context_assemble(x.cuda(), w.cuda())
    p, k, t, d = shape
    assert out.shape == (p, k * t, d) and out.dtype == torch.float16
    err = (out.cpu().double().reshape(shape) - ref).abs()
    bound = 2.0 ** -10 * ref.abs() + 2.0 ** -24
    worst = float((err / bound).max())
    print(f'context_assemble {shape}: conditioning {cond:.2f}, worst error / bound {worst:.3f}')
    assert torch.isfinite(out).all() and worst <= 1.0, worst


def test_context_assemble_identity_zero_chunk_and_determinism():
    from sdod.amd import ops
    x, w = _kernel_inputs((2, 2, 77, 768), seed=5)
    xg, wg = x.cuda(), w.cuda()
    flat = xg.reshape(2, 154, 768)
    assert torch.equal(ops.context_assemble(xg, torch.ones_like(wg)), flat)      # s0 == s1 bit for bit, r == 1
    assert torch.equal(ops.context_assemble(xg, None), flat)                     # the copy
    a = ops.context_assemble(xg, wg)
    assert torch.equal(a, ops.context_assemble(xg, wg))                          # two runs, equal bits
    assert not torch.equal(a, flat)
    wz = wg.clone()
    wz[1, 0] = 0.0                                                               # the guard: s1 == 0 -> r = 1 -> zeros, not NaN
    z = ops.context_assemble(xg, wz).reshape(2, 2, 77, 768)
    assert torch.isfinite(z).all() and bool((z[1, 0] == 0).all())
    keep = torch.ones(2, 2, dtype=torch.bool, device='cuda'); keep[1, 0] = False
    assert torch.equal(z[keep], a.reshape(2, 2, 77, 768)[keep])                  # the other chunks do not see it
    out = torch.empty(2, 154, 768, dtype=torch.float16, device='cuda')
    assert ops.context_assemble(xg, wg, out=out) is out and torch.equal(out, a)
    with pytest.raises(ValueError):
        ops.context_assemble(xg, wg[:, :1])
    with pytest.raises(Exception, match='alias'):
        ops.context_assemble(xg, wg, out=flat)


# ------------------------------------------------------------------ the UNet graph with a longer context
@pytest.fixture(scope='module')
def unet_rig():
    """synthetic UNet + time-MLP weights, the CPU oracle on them, and the projected time embedding of t = 999 for batch 2"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    sd = {**Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234), **Wt.synthetic_state_dict(E.Temb(cfg, 2).param_table(), seed=1235)}
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict(sd, assign=True)
    tg = E.Temb(cfg, 2)
    tg.load_state_dict(sd)
    tg.finalize()
    t = torch.tensor([999.0, 999.0])
    tg.t.copy_(t); tg.execute()
    torch.cuda.synchronize()
    return sd, unet.eval(), t, tg.out.clone()


@pytest.mark.parametrize('context_len', [154, 231, 308])
def test_unet_graph_with_long_context(unet_rig, context_len):
    from sdod.amd import engine as E
    sd, unet, t, temb = unet_rig
    cfg = E.sd14_config(16, 16)
    cfg.context_len = context_len
    g = E.UNet(cfg, 2)
    g.load_state_dict(sd)
    g.finalize()
    assert g.ctx.shape == (2, context_len, 768)
    labels = [o[0] for o in g.op_table()]
    assert 'xattn_fold' not in labels and sum(lab.startswith('attn_d') for lab in labels) == 32      # 16 self + 16 cross attention launches
    gen = torch.Generator().manual_seed(context_len)
    x = torch.randn(2, 4, 16, 16, generator=gen)
    ctx = torch.randn(2, context_len, 768, generator=gen).half()
    with torch.no_grad():
        ref = unet(x, t, ctx.float())
    g.x.copy_(x); g.temb.copy_(temb); g.ctx.copy_(ctx)
    g.execute()
    torch.cuda.synchronize()
    out = g.eps.float().cpu().permute(0, 3, 1, 2)
    r = rel_l2(out, ref)
    print(f'unet 16x16 b2, {context_len} keys: rel-L2 {r:.3e}, {g.stats()["launches"]} launches, {g.tune_source()}')
    assert torch.isfinite(out).all() and r <= 1e-2, r
    eager = g.eps.clone()
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True, static_unchanged=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.eps), 'hipGraph replay differs from eager execution'
    # the keys behind the first chunk are read: changing only them changes the result (and the first 77 alone do not define it)
    ctx2 = ctx.clone()
    ctx2[:, 77:] = torch.randn(2, context_len - 77, 768, generator=gen).half()
    g.ctx.copy_(ctx2)
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.isfinite(g.eps).all() and not torch.equal(eager, g.eps)
    g.check()


# ------------------------------------------------------------------ the pipeline
PROMPT = ('a (photograph:1.3) of an [astronaut] riding a ((horse)) on the moon, (highly detailed:1.2), sharp focus, '
          'studio lighting BREAK (oil painting:0.8) of a horse')
NEGATIVE = '(blurry:1.4), [watermark], text'


@pytest.fixture(scope='module')
def rig(golden_dir):
    from oracle import sd_torch as S
    from sdod.amd import engine as E, host, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(16, 16)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'text': E.TextEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    tok = host.Tokenizer(os.path.join(golden_dir, 'ctokenizer_synthetic.txt'))
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, tokenizer=tok, prompt_chunks=2)
    with torch.device('meta'):
        unet, vae, clip = S.UNetModel(), S.AutoencoderKLDecode(), S.ClipTextModel()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    vae.load_state_dict(sds['vae'], assign=True)
    clip.load_state_dict(sds['text'], assign=True)
    return pipe, unet.eval(), vae.eval(), clip.eval(), tok


@pytest.fixture(scope='module')
def chunks(rig):
    """(ids_uncond [2, 77], ids_cond [2, 77], weights [2, 2, 77]) of the module's prompt pair"""
    from sdod.amd import prompts as PR
    tok = rig[4]
    iu, wu = PR.pad_chunks(*PR.chunk_prompt(tok, NEGATIVE), 2, tok)
    ic, wc = PR.chunk_prompt(tok, PROMPT)
    assert ic.shape == (2, 77) and int((wc != 1).sum()) > 10 and int((wu != 1).sum()) > 2      # two real chunks, weighted tokens in both
    return iu, ic, np.stack([wu, wc])


def test_pipeline_shapes(rig):
    pipe = rig[0]
    assert pipe.prompt_chunks == 2 and pipe.unet.ctx.shape == (2, 154, 768) and pipe.unet.cfg.context_len == 154
    assert pipe.cfg.context_len == 77 and pipe.text.ids.shape == (4, 77) and pipe.text.out.shape == (4, 77, 768)


def test_unweighted_chunks_match_the_oracle_clip_per_chunk(rig, chunks):
    pipe, _, _, clip, _ = rig
    iu, ic, _ = chunks
    ctx2 = pipe.encode_chunks(iu, ic)
    assert ctx2.shape == (2, 154, 768) and ctx2.dtype == torch.float16
    with torch.no_grad():
        ref = clip(torch.from_numpy(np.concatenate([iu, ic]))).reshape(2, 154, 768)     # each chunk on its own, then concatenated
    r = rel_l2(ctx2.float().cpu(), ref)
    print('clip, 2 chunks x 2 prompts: rel-L2', r)
    assert r <= 5e-3, r


def test_weighted_chunks_are_context_assemble_of_the_unweighted(rig, chunks):
    from sdod.amd import ops
    pipe = rig[0]
    iu, ic, w = chunks
    plain = pipe.encode_chunks(iu, ic)
    weighted = pipe.encode_chunks(iu, ic, w)
    want = ops.context_assemble(plain.reshape(2, 2, 77, 768), torch.from_numpy(w).cuda())
    assert torch.equal(weighted, want) and not torch.equal(weighted, plain)
    assert torch.equal(pipe.encode_chunks(iu, ic, torch.from_numpy(w)), want)            # a torch tensor is taken as well
    assert torch.equal(pipe.encode_chunks(iu, ic, np.ones_like(w)), plain)
    assert torch.equal(pipe.encode_prompt_weighted(PROMPT, NEGATIVE), weighted)


def test_short_prompt_is_padded_with_empty_chunks(rig):
    from sdod.amd import prompts as PR
    pipe, tok = rig[0], rig[4]
    text, neg = 'a photograph of an astronaut riding a horse', ''
    got = pipe.encode_prompt(text, neg)
    iu, _ = PR.pad_chunks(*PR.chunk_prompt(tok, neg, emphasis=False), 2, tok)
    ic, _ = PR.pad_chunks(*PR.chunk_prompt(tok, text, emphasis=False), 2, tok)
    assert got.shape == (2, 154, 768) and torch.equal(got, pipe.encode_chunks(iu, ic))
    assert torch.equal(got, pipe.encode_tokens(pipe._ids(neg), pipe._ids(text)))
    assert torch.equal(got, pipe.encode_prompt_weighted(text, neg))                       # nothing weighted: all-ones weights change no bit


def test_plms_20_steps_from_the_assembled_context_matches_oracle(rig, chunks):
    from oracle import pipeline_oracle as PO
    pipe, unet, vae, _, _ = rig
    ctx2 = pipe.encode_chunks(*chunks)
    x_T = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(42))
    tr_gpu, tr_cpu = [], []
    z = pipe.sample_plms(ctx2, x_T, steps=20, guidance=7.5, trace=tr_gpu)
    c16 = ctx2.float().cpu()                      # the oracle consumes the SAME fp16 context the GPU used
    z_ref = PO.plms_sample(unet, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5, trace=tr_cpu)
    assert tr_gpu == tr_cpu
    r = rel_l2(z.cpu(), z_ref)
    print('plms, 154 keys: final latent rel-L2', r)
    assert torch.isfinite(z).all() and r <= 2e-2, r
    img = pipe.decode(z, mode=1).cpu().numpy()
    img_ref = PO.decode_u8(vae, z_ref, mode=1)
    diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
    frac = float((diff <= 2).mean())
    print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
    assert img.shape == (1, 128, 128, 3) and frac >= 0.99, frac


@pytest.mark.parametrize('sampler', ['plms', 'dpm', 'euler_a'])
def test_generate_graphed_equals_generate(rig, chunks, sampler):
    pipe = rig[0]
    ctx2 = pipe.encode_chunks(*chunks)
    x_T = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(7))
    kw = dict(steps=4, guidance=7.5, sampler=sampler, seed=11)        # PLMS, as ldm, takes a step count that divides 1000; 4 reaches its order 3
    a = pipe.generate(ctx2, x_T, **kw).clone()
    b = pipe.generate_graphed(ctx2, x_T, **kw).clone()
    assert a.shape == (1, 128, 128, 3) and torch.equal(a, b)
    ctx3 = pipe.encode_chunks(chunks[0], chunks[1])                                       # another context through the same graph
    c = pipe.generate_graphed(ctx3, x_T, **kw).clone()
    assert torch.equal(c, pipe.generate(ctx3, x_T, **kw)) and not torch.equal(c, a)
