"""T2I-Adapter structural control on the GPU: the five kernels bit for bit against their definitions, the ADAPTER graph against the fp32
restatement (tests/adapter_ref.py), the UNet's feature slots against the fp32 oracle with forward hooks behind input_blocks 2 / 5 / 8 /
11, and the pipeline (set_adapter_hint / clear_adapter_hint, eager and captured, every entry point reading the same slots).

Stated tolerances, all of them the project's own for the same kind of comparison: an fp16 graph against the fp32 oracle rel-L2 <= 1e-2
(test_engine_gpu.py, test_inpaint_concat_gpu.py); a 20-step PLMS chain's final latent rel-L2 <= 2e-2
(test_inpaint_concat_chain_matches_the_restatement); sdod_act_f16's existing codes against torch's definitions as test_kernels_gpu.py
checks them (gemm_cases.check_close).  Everything else is bit-exact."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import adapter_ref as AR
from gemm_cases import check_close

pytestmark = pytest.mark.gpu

# launch count and activation-arena bytes of the batch-2 16x16 UNet graph WITHOUT adapter inputs, recorded from the commit before
# this feature on the same weights and device (every GEMM tile from tune/gfx950.tune, none timed in process): a graph built with
# adapter_reps = 0 must still be that graph
PARENT_LAUNCHES = 321
PARENT_ARENA_BYTES = 4260096


# sdod_act_f16 at (+inf, -inf) for the codes that existed before
ACT_AT_INF = {'silu': ('inf', 'nan'), 'gelu': ('nan', 'nan'), 'quick_gelu': ('inf', 'nan')}


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize('ch', [1, 3])
def test_pixel_unshuffle_is_torchs(ch):
    from sdod.amd import ops
    n, h, w = 2, 2, 3
    img = (torch.arange(n * 8 * h * 8 * w * ch) % 251).to(torch.uint8).reshape(n, 8 * h, 8 * w, ch)      # every position distinct
    ref = F.pixel_unshuffle(img.permute(0, 3, 1, 2).float() / 255, 8).permute(0, 2, 3, 1).half()
    out = ops.pixel_unshuffle_u8(img.cuda())
    assert tuple(out.shape) == (n, h, w, 64 * ch) and out.dtype == torch.float16
    assert torch.equal(out.cpu(), ref)


def test_avg_pool2_is_the_fp32_expression():
    from sdod.amd import ops
    g = torch.Generator().manual_seed(21)
    n, h, w, c = 2, 4, 6, 8
    x = (torch.randn(n, h, w, c, generator=g) * torch.exp2(torch.randint(-9, 10, (n, h, w, c), generator=g).float())).half()
    assert float(x.abs().max() / x.abs().min()) > 2.0 ** 12                                               # several binades
    f = x.float()
    ref = (((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + (f[:, 1::2, 0::2] + f[:, 1::2, 1::2])) * 0.25).half()
    out = ops.avg_pool2(x.cuda())
    assert tuple(out.shape) == (n, h // 2, w // 2, c)
    assert torch.equal(out.cpu(), ref)


def test_relu_and_the_existing_act_codes():
    from sdod.amd import ops
    g = torch.Generator().manual_seed(22)
    x = (torch.randn(64, generator=g) * 3).half()
    x[:8] = torch.tensor([0.0, -0.0, float('inf'), float('-inf'), -1.0, 1.0, 65504.0, -65504.0]).half()
    out = ops.activation(x.cuda(), 'relu').cpu()
    assert torch.equal(out, torch.relu(x)) and bool((x < 0).any()) and float(out[2]) == float('inf') and float(out[3]) == 0.0
    # the codes that existed before, on the same vector: 0 copies the bytes; 1-3 against torch's definitions, as test_kernels_gpu.py
    # checks them, at every finite input (0, -0 and +-65504 included; the small values on their own as well, so that the two
    # 65504s do not carry the norm).  At +-inf the kernels' rcp / exp2 forms give what ACT_AT_INF records from the commit before
    # this feature -- torch's values but for gelu(+inf), which has always been NaN here (-|x| * 2^-inf = -inf * 0).
    assert torch.equal(ops.activation(x.cuda(), None).cpu().view(torch.int16), x.view(torch.int16))
    fin, small = torch.isfinite(x), x.abs() < 100
    f = x.float()
    for act, ref in (('silu', F.silu(f)), ('gelu', F.gelu(f)), ('quick_gelu', f * torch.sigmoid(1.702 * f))):
        out = ops.activation(x.cuda(), act).cpu()
        check_close(out[fin], ref[fin], name=act)
        check_close(out[small], ref[small], name=act + ' (|x| < 100)')
        got = tuple('nan' if v != v else str(v) for v in out[2:4].tolist())
        assert got == ACT_AT_INF[act], (act, got)
        if act != 'gelu':
            assert got == tuple('nan' if v != v else str(v) for v in ref[2:4].tolist()), (act, got)
    # ReLU is no GEMM epilogue: refused there, not ignored
    a = torch.zeros(64, 64, dtype=torch.float16, device='cuda')
    with pytest.raises(Exception, match='RELU'):
        ops.gemm(a, a, None, act='relu')


@pytest.mark.parametrize('weight', [1.0, 0.0, 0.37])
def test_adapter_stage_scales_in_fp32(weight):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(23)
    src = (torch.randn(4096, generator=g) * 4).half()
    dst = torch.full((4096,), -7.0, dtype=torch.float16, device='cuda')
    ops.adapter_stage(src.cuda(), dst, weight)
    assert torch.equal(dst.cpu(), (weight * src.float()).half())
    if weight == 1.0:
        assert torch.equal(dst.cpu(), src)


@pytest.mark.parametrize('reps', [1, 2])
@pytest.mark.parametrize('per_copy', [8, 2 * 16 * 24 * 320])
def test_add_feature_adds_to_every_copy_and_nothing_else(reps, per_copy):
    """per_copy = 245,760: a rectangular map, 30,720 threads = more than one workgroup per copy"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(24 + reps)
    guard = 64
    buf = (torch.randn(reps * per_copy + guard, generator=g) * 2).half()
    f = torch.randn(per_copy, generator=g).half()
    dev, fd = buf.cuda(), f.cuda()
    ops.add_feature(dev[:reps * per_copy], fd, reps)
    out = dev.cpu()
    for r in range(reps):
        assert torch.equal(out[r * per_copy:(r + 1) * per_copy], (buf[r * per_copy:(r + 1) * per_copy].float() + f.float()).half()), r
    assert torch.equal(out[reps * per_copy:].view(torch.int16), buf[reps * per_copy:].view(torch.int16))  # the guard behind h
    assert torch.equal(fd.cpu().view(torch.int16), f.view(torch.int16))                                   # the feature is only read


def test_the_kernels_refuse_bad_arguments_and_leave_the_destination_untouched():
    from sdod.amd import _lib
    lib = _lib.hip()
    img = torch.zeros(1 * 16 * 16 * 3 + 16, dtype=torch.uint8, device='cuda')
    x = torch.ones(4096 + 16, dtype=torch.float16, device='cuda')
    y = torch.full((4096 + 16,), 7.0, dtype=torch.float16, device='cuda')
    # pixel unshuffle: factor != 8, a channel count it does not take, null and misaligned pointers
    assert lib.sdod_pixel_unshuffle_u8_f16(P(img), P(y), 1, 2, 2, 3, 4, None) != 0 and b'factor' in lib.sdod_hip_last_error()
    assert lib.sdod_pixel_unshuffle_u8_f16(P(img), P(y), 1, 2, 2, 2, 8, None) != 0
    assert lib.sdod_pixel_unshuffle_u8_f16(P(img), P(y), 1, 0, 2, 3, 8, None) != 0
    assert lib.sdod_pixel_unshuffle_u8_f16(None, P(y), 1, 2, 2, 3, 8, None) != 0
    assert lib.sdod_pixel_unshuffle_u8_f16(P(img), P(y[1:]), 1, 2, 2, 3, 8, None) != 0 and b'misaligned' in lib.sdod_hip_last_error()
    # average pool: an odd size, channels no multiple of 8
    assert lib.sdod_avg_pool2_f16(P(x), P(y), 1, 3, 4, 8, None) != 0 and b'even' in lib.sdod_hip_last_error()
    assert lib.sdod_avg_pool2_f16(P(x), P(y), 1, 4, 5, 8, None) != 0
    assert lib.sdod_avg_pool2_f16(P(x), P(y), 1, 4, 4, 12, None) != 0
    assert lib.sdod_avg_pool2_f16(P(x), P(y[4:]), 1, 4, 4, 8, None) != 0
    # activation: a misaligned count (ReLU takes the same checks as the other codes)
    assert lib.sdod_act_f16(P(x), P(y), 100, 4, None) != 0
    assert lib.sdod_act_f16(P(x), None, 64, 4, None) != 0
    # stage: a misaligned count, a non-finite weight, a misaligned pointer
    assert lib.sdod_adapter_stage_f16(P(x), P(y), 4095, 1.0, None) != 0
    assert lib.sdod_adapter_stage_f16(P(x), P(y), 4096, float('nan'), None) != 0 and b'finite' in lib.sdod_hip_last_error()
    assert lib.sdod_adapter_stage_f16(P(x), P(y), 4096, float('inf'), None) != 0
    assert lib.sdod_adapter_stage_f16(P(x[1:]), P(y), 4096, 1.0, None) != 0
    # feature add (y is its destination): reps outside {1, 2}, a misaligned count or pointer
    assert lib.sdod_add_feature_f16(P(y), P(x), 2048, 3, None) != 0 and b'reps' in lib.sdod_hip_last_error()
    assert lib.sdod_add_feature_f16(P(y), P(x), 2048, 0, None) != 0
    assert lib.sdod_add_feature_f16(P(y), P(x), 2044, 2, None) != 0
    assert lib.sdod_add_feature_f16(P(y[2:]), P(x), 2048, 1, None) != 0
    assert lib.sdod_add_feature_f16(P(y), None, 2048, 1, None) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((x == 1.0).all())
    assert lib.sdod_add_feature_f16(P(y), P(x), 2048, 2, None) == 0                    # and the good call writes exactly its range
    torch.cuda.synchronize()
    assert bool((y[:4096] == 8.0).all()) and bool((y[4096:] == 7.0).all())


# ------------------------------------------------------------------ graphs
@pytest.fixture(scope='module')
def weights16():
    """the weights16 recipe of tests/test_inpaint_concat_gpu.py on the 4-channel UNet, plus the two adapters"""
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'text': E.TextEncoder(cfg, 1).param_table(),
              'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    sds['adapter'] = Wt.synthetic_state_dict(AR.param_table(3), seed=1239)
    sds['adapter1'] = Wt.synthetic_state_dict(AR.param_table(1), seed=1240)
    return sds


def hint128(ch=3, phase=0.0):
    """a smooth 128 x 128 pattern with edges, uint8 [1, 128, 128, ch]"""
    yy, xx = torch.meshgrid(torch.arange(128.), torch.arange(128.), indexing='ij')
    img = torch.stack([128 + 100 * torch.sin(xx / 7 + k + phase) * torch.cos(yy / 5 - phase) for k in range(ch)], -1)
    img[:, 40:44] = 255.0
    return img.clamp(0, 255).to(torch.uint8)[None]


@pytest.mark.parametrize('hc', [3, 1])
def test_adapter_graph_matches_the_restatement(weights16, hc):
    from sdod.amd import engine as E
    sd = weights16['adapter' if hc == 3 else 'adapter1']
    g = E.Adapter(E.sd14_config(16, 16, adapter_hint_channels=hc), 1)
    assert g.param_table() == AR.param_table(hc)
    g.load_state_dict(sd); g.finalize()
    assert tuple(g.hint.shape) == (1, 128, 128, hc)
    labels = [l for l, _, _ in g.op_table()]
    assert labels[0] == 'pixel_unshuffle' and labels.count('avg_pool2') == 3 and labels.count('relu') == 8

    def run(hint, hip_graph=False):
        g.hint.copy_(hint)
        g.execute(use_hip_graph=hip_graph)
        torch.cuda.synchronize()
        return [o.clone() for o in g.out]

    hint = hint128(hc)
    outs = run(hint)
    refs = AR.adapter_forward(sd, hint)
    for k, (o, r) in enumerate(zip(outs, refs)):
        rl = rel_l2(o.float().cpu().permute(0, 3, 1, 2), r)
        print(f'adapter graph, {hc}-channel hint, output {k} {tuple(o.shape)}: rel-L2 vs fp32 restatement {rl:.3e}')
        assert tuple(o.shape) == tuple(r.permute(0, 2, 3, 1).shape) and torch.isfinite(o).all() and rl <= 1e-2, (k, rl)
    replay = run(hint, hip_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(outs, replay))
    other = run(hint128(hc, phase=1.3), hip_graph=True)
    assert all(not torch.equal(a, b) and rel_l2(b.float(), a.float()) > 1e-2 for a, b in zip(outs, other))
    refs2 = AR.adapter_forward(sd, hint128(hc, phase=1.3))
    assert all(rel_l2(o.float().cpu().permute(0, 3, 1, 2), r) <= 1e-2 for o, r in zip(other, refs2))


@pytest.fixture(scope='module')
def unets(weights16):
    """the UNet without and with adapter inputs on the same weights, the oracle, one set of inputs and the oracle's plain output"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E
    sds = weights16
    tg = E.Temb(E.sd14_config(16, 16), 2); tg.load_state_dict(sds['temb']); tg.finalize()
    g0 = E.UNet(E.sd14_config(16, 16), 2); g0.load_state_dict(sds['unet']); g0.finalize()
    g2 = E.UNet(E.sd14_config(16, 16, adapter_reps=2), 2); g2.load_state_dict(sds['unet']); g2.finalize()
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    unet.eval()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 16, 16, generator=gen)
    ctx = torch.randn(2, 77, 768, generator=gen).half()
    t = torch.tensor([999.0, 501.0])
    with torch.no_grad():
        ref0 = unet(x, t, ctx.float())
    feats = [6.0 * torch.randn(1, c, h, w, generator=gen) for _, h, w, c in E.adapter_feature_shapes(g2.cfg, 1)]
    return dict(tg=tg, g0=g0, g2=g2, unet=unet, x=x, ctx=ctx, t=t, ref0=ref0, feats=feats)


def _eval(g, r):
    tg = r['tg']
    tg.t.copy_(r['t']); tg.execute()
    g.x.copy_(r['x']); g.temb.copy_(tg.out); g.ctx.copy_(r['ctx'])
    g.execute()
    torch.cuda.synchronize()
    eager = g.eps.clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.eps, eager)
    return eager.float().cpu().permute(0, 3, 1, 2)


def test_unet_with_zero_slots_is_the_plain_graph_plus_four_launches(unets):
    r = unets
    g0, g2 = r['g0'], r['g2']
    assert not hasattr(g0, 'adapter_feat') and len(g2.adapter_feat) == 4
    assert [tuple(f.shape) for f in g2.adapter_feat] == [(1, 16, 16, 320), (1, 8, 8, 640), (1, 4, 4, 1280), (1, 2, 2, 1280)]
    assert all(f.dtype == torch.float16 and not bool(f.any()) for f in g2.adapter_feat)                # zeroed at finalize
    with pytest.raises(Exception):
        g0._io(False, 3)
    with pytest.raises(Exception):
        g2._io(False, 7)
    s0, s2 = g0.stats(), g2.stats()
    print(f'UNet b2 16x16: {s0["launches"]} launches, arena {s0["arena_bytes"]} B; with adapter inputs {s2["launches"]}, {s2["arena_bytes"]} B')
    assert (s0['launches'], s0['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES)
    assert s2['launches'] - s0['launches'] == 4 and s2['weight_bytes'] == s0['weight_bytes']
    l0, l2 = [l for l, _, _ in g0.op_table()], [l for l, _, _ in g2.op_table()]
    assert l2.count('add_feature') == 4 and 'add_feature' not in l0 and [l for l in l2 if l != 'add_feature'] == l0
    out0, out2 = _eval(g0, r), _eval(g2, r)
    assert torch.equal(out2, out0)
    rl = rel_l2(out0, r['ref0'])
    print(f'plain graph vs fp32 oracle rel-L2 {rl:.3e}')
    assert rl <= 1e-2


@pytest.mark.parametrize('case', [0, 1, 2, 3, 'all'])
def test_unet_features_match_the_hooked_oracle(unets, case):
    """only level k set, then all four: against the oracle with hooks behind input_blocks 2 / 5 / 8 / 11, the same features in both
    batch rows.  The features are large enough that the oracle itself moves by more than 5e-2: a level that is ignored cannot pass."""
    r = unets
    g2 = r['g2']
    feats = [f if case == 'all' or case == k else None for k, f in enumerate(r['feats'])]
    with AR.hooked(r['unet'], feats) as m, torch.no_grad():
        ref = m(r['x'], r['t'], r['ctx'].float())
    moved = rel_l2(ref, r['ref0'])
    assert moved > 5e-2, moved                                                       # on the CPU, before any GPU work
    assert not any(bool(s.any()) for s in g2.adapter_feat)                           # every test leaves the slots zero
    if 'zero' not in r:
        r['zero'] = _eval(g2, r)
    zero = r['zero']
    for slot, f in zip(g2.adapter_feat, feats):
        if f is None:
            slot.zero_()
        else:
            slot.copy_(f.permute(0, 2, 3, 1).half())
    out = _eval(g2, r)
    for slot in g2.adapter_feat:
        slot.zero_()
    rl, away = rel_l2(out, ref), rel_l2(out, zero)
    print(f'UNet with features at level {case}: rel-L2 vs hooked oracle {rl:.3e}, vs the zero-feature output {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(out).all() and rl <= 1e-2 and away > 1e-2, (rl, away)
    assert rel_l2(zero, r['ref0']) <= 1e-2


# ------------------------------------------------------------------ pipeline
@pytest.fixture(scope='module')
def rig(weights16):
    from oracle import sd_torch as S
    from sdod.amd.pipeline import Txt2Img
    sds = weights16
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=16, with_text_encoder=False, with_vae_encoder=True)
    pipe = Txt2Img(adapter=True, **kw)
    plain = Txt2Img(**kw)
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**sds['unet'], **sds['temb']}, assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    u8 = torch.randint(0, 256, (1, 128, 128, 3), generator=g, dtype=torch.uint8)
    return dict(pipe=pipe, plain=plain, unet=unet.eval(), ctx2=ctx2, x_T=x_T, u8=u8, hint=hint128(3), hint_b=hint128(3, phase=1.3))


def test_pipeline_construction(rig):
    pipe, plain = rig['pipe'], rig['plain']
    assert pipe.adapter is not None and pipe.adapter.batch == 1 and pipe.unet.cfg.adapter_reps == 2 and pipe.cfg.adapter_reps == 0
    assert tuple(pipe.adapter.hint.shape) == (1, 128, 128, 3) and len(pipe.unet.adapter_feat) == 4
    assert plain.adapter is None and not hasattr(plain.unet, 'adapter_feat')
    assert plain.unet.stats()['launches'] + 4 == pipe.unet.stats()['launches']
    assert plain.unet.stats()['arena_bytes'] == pipe.unet.stats()['arena_bytes']
    with pytest.raises(RuntimeError, match='adapter=True'):
        plain.set_adapter_hint(rig['hint'])
    with pytest.raises(RuntimeError, match='adapter=True'):
        plain.clear_adapter_hint()
    with pytest.raises(ValueError):
        pipe.set_adapter_hint(rig['hint'][..., :1])
    with pytest.raises(ValueError):
        pipe.set_adapter_hint(rig['hint'], float('inf'))


def test_refused_combinations(weights16):
    from sdod.amd.pipeline import Txt2Img
    for kw in (dict(cfg_split=True), dict(hires_hw=32), dict(inpaint_unet=True), dict(model='sd21')):
        with pytest.raises(ValueError, match='adapter'):
            Txt2Img(state_dicts=weights16, latent_hw=16, with_text_encoder=False, adapter=True, **kw)


@pytest.mark.parametrize('sampler', ['plms', 'dpmpp_2m'])
def test_eager_and_captured_are_the_same_and_a_new_hint_needs_no_capture(rig, sampler):
    pipe, plain, c, x_T = rig['pipe'], rig['plain'], rig['ctx2'].cuda(), rig['x_T']
    pipe.set_adapter_hint(rig['hint'])
    eager = pipe.generate(c, x_T, 4, 7.5, sampler)
    graphed = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert torch.equal(graphed, eager)
    base = plain.generate(c, x_T, 4, 7.5, sampler)
    assert not torch.equal(eager, base)
    # another hint: the captured trajectory reads the same slots
    n_graphs = len(pipe._traj)
    pipe.set_adapter_hint(rig['hint_b'])
    graphed_b = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs                                  # a replay, not a new capture
    assert not torch.equal(graphed_b, graphed) and torch.equal(graphed_b, pipe.generate(c, x_T, 4, 7.5, sampler))
    # another weight: the same
    pipe.set_adapter_hint(rig['hint_b'], 0.5)
    graphed_w = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs and not torch.equal(graphed_w, graphed_b)
    # weight 0 and a cleared hint: the pipeline built without the feature, bit for bit, eager and captured
    pipe.set_adapter_hint(rig['hint_b'], 0.0)
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
    pipe.set_adapter_hint(rig['hint'])
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), graphed)
    pipe.clear_adapter_hint()
    assert not any(bool(s.any()) for s in pipe.unet.adapter_feat)
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
    assert len(pipe._traj) == n_graphs
    assert torch.equal(plain.generate_graphed(c, x_T, 4, 7.5, sampler), base)


def test_hinted_latents_match_the_hooked_oracle(rig, weights16):
    """20 PLMS steps with a hint against the sampler restatement (oracle/pipeline_oracle.py) on the hooked fp32 UNet, the features
    from the fp32 adapter restatement: the bound of test_inpaint_concat_chain_matches_the_restatement for its final latents"""
    from oracle import pipeline_oracle as PO
    pipe, x_T = rig['pipe'], rig['x_T']
    c16 = rig['ctx2'].float()
    feats = AR.adapter_forward(weights16['adapter'], rig['hint'])
    with AR.hooked(rig['unet'], feats) as m:
        z_ref = PO.plms_sample(m, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5)
    pipe.clear_adapter_hint()
    z_plain = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
    moved = rel_l2(z_ref, z_plain)                                       # the hint matters: far outside the bound below
    assert moved > 5e-2, moved
    pipe.set_adapter_hint(rig['hint'])
    for out, ref in zip(pipe.adapter.out, feats):                        # what was staged: the adapter's own outputs, weight 1
        assert rel_l2(out.float().cpu().permute(0, 3, 1, 2), ref) <= 1e-2
    for out, slot in zip(pipe.adapter.out, pipe.unet.adapter_feat):
        assert torch.equal(out, slot)
    before = [s.clone() for s in pipe.unet.adapter_feat]
    z = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5)
    assert all(torch.equal(a, b) for a, b in zip(before, pipe.unet.adapter_feat))        # static: no sampler launch writes there
    rl = rel_l2(z.cpu(), z_ref)
    print(f'hinted plms final latent rel-L2 vs hooked oracle {rl:.3e} (against the unhinted latent: {moved:.3e})')
    assert torch.isfinite(z).all() and rl <= 2e-2, rl
    pipe.clear_adapter_hint()


def test_img2img_runs_conditioned(rig):
    pipe, plain, c, u8 = rig['pipe'], rig['plain'], rig['ctx2'].cuda(), rig['u8']
    g = torch.Generator().manual_seed(5)
    noise = (torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g))
    pipe.clear_adapter_hint()
    cleared = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
    assert torch.equal(cleared, plain.img2img(c, u8, 0.5, 8, 7.5, noise=noise))
    pipe.set_adapter_hint(rig['hint'])
    n_graphs = len(pipe._traj)
    hinted = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
    assert len(pipe._traj) == n_graphs and not torch.equal(hinted, cleared)
    assert torch.equal(hinted, pipe.img2img(c, u8, 0.5, 8, 7.5, noise=noise))
    pipe.clear_adapter_hint()
