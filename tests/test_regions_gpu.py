"""Regional prompts on the GPU: the UNET graph with regions (launch list, accuracy against the fp32 restatement tests/regions_ref.py,
capture) and the pipeline Txt2Img(regions=2) (construction, encode_regions, set_regions / clear_regions, eager against captured, the
20-step PLMS latent, one LoRA case).  Synthetic weights, batch 2, latents (16, 16) and (8, 16).

Stated tolerances, the project's own for the same comparisons: an fp16 graph against the fp32 restatement rel-L2 <= 1e-2; a 20-step
PLMS chain's final latent <= 2e-2; everything else is bit-exact.  Where a test relies on the masks mattering, the fp32 restatement is
first shown, on the CPU, to move by more than 5e-2 when the masks are swapped, and the two GPU results must lie farther than 1e-2
apart."""
import numpy as np
import pytest
import torch

import lora_cases as LC
import regions_ref as RR

pytestmark = pytest.mark.gpu

# launch count and activation-arena bytes of the batch-2 16x16 UNet graph without the feature, as tests/test_adapter_gpu.py and
# tests/test_controlnet_gpu.py record them
PARENT_LAUNCHES = 321
PARENT_ARENA_BYTES = 4260096
SIZES = [(16, 16), (8, 16)]


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


@pytest.fixture(scope='module')
def weights():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    return {'unet': Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234),
            'temb': Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235),
            'vae': Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1236),
            'text': Wt.synthetic_state_dict(E.TextEncoder(cfg, 1).param_table(), seed=1237),
            'vae_enc': Wt.synthetic_state_dict(E.VaeEncoder(cfg, 1).param_table(), seed=1238)}


@pytest.fixture(scope='module')
def oracle(weights):
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**weights['unet'], **weights['temb']}, assign=True)
    return unet.eval()


def _inputs(hw, k, seed=7):
    gen = torch.Generator().manual_seed(seed + hw[0] + k)
    x = torch.randn(2, 4, *hw, generator=gen)
    ctx = (torch.randn(2, 77 * k, 768, generator=gen) * 0.5).half()
    return x, ctx, torch.tensor([999.0, 501.0])


_graphs = {}


def _graph(weights, hw, k):
    """one finalized (UNet with k regions, Temb) per size, shared by the tests of this module"""
    from sdod.amd import engine as E
    if (hw, k) not in _graphs:
        cfg = E.sd14_config(*hw)
        tg = E.Temb(cfg, 2); tg.load_state_dict(weights['temb']); tg.finalize()
        c = E.copy_config(cfg)
        if k:
            c.context_len, c.regions = 77 * k, k
        g = E.UNet(c, 2); g.load_state_dict(weights['unet']); g.finalize()
        _graphs[(hw, k)] = (g, tg)
    return _graphs[(hw, k)]


def _eval(g, tg, x, ctx, t, ws=None):
    """eager, then the hip-graph replay: bit-equal; returns NCHW fp32 on the CPU"""
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    if ws is not None:
        for slot, w in zip(g.region_w, ws):
            slot.copy_(w)
    g.execute()
    torch.cuda.synchronize()
    eager = g.eps.clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.eps, eager)
    return nchw(eager)


# ------------------------------------------------------------------ the graph
def test_plain_graph_is_unchanged(weights):
    g, _ = _graph(weights, (16, 16), 0)
    s = g.stats()
    assert (s['launches'], s['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES) and not hasattr(g, 'region_w')
    labels = [l for l, _, _ in g.op_table()]
    assert 'region_blend' not in labels and len(labels) == PARENT_LAUNCHES
    # the launch list of the graph from before the feature: 16 transformers -- the 10 at L = 256 and 64 folded (two GEMMs), the 6 at
    # L = 16 and 4 in the three-launch form (Linear, attention, Linear): 16 self- and 6 cross-attention launches
    assert sum(l.startswith('attn_d') for l in labels) == 16 + 6
    assert not any(d in g.op_details() for d in ('rows M512 N1280 K320 x1', 'rows M512 N320 K1280 x1', 'rows M128 N640 K1280 x1'))
    assert g.tune_source()['shapes_tuned_in_process'] == 0
    with pytest.raises(Exception):
        g._io(False, 3)                                                  # no fourth input


@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('hw', SIZES)
def test_launch_list_with_regions(weights, hw, k):
    g, _ = _graph(weights, hw, k)
    plain, _ = _graph(weights, hw, 0)
    labels, details = [l for l, _, _ in g.op_table()], g.op_details()
    pl = [l for l, _, _ in plain.op_table()]
    assert [tuple(w.shape) for w in g.region_w] == [((hw[0] >> l) * (hw[1] >> l), k) for l in range(4)]
    assert all(torch.equal(w.cpu(), r) for w, r in zip(g.region_w, RR.background_weights(k, hw)))         # region 0 everywhere at finalize
    assert tuple(g.ctx.shape) == (2, 77 * k, 768)
    # folded where L % 32 == 0 -- the same launch count per block as the plain fold, both GEMMs k times as wide -- and otherwise, per
    # block, one attention launch per (image, region) and a blend launch in the place of the one attention launch
    levels = [(hw[0] >> l) * (hw[1] >> l) for l in range(4)]
    blocks = [5, 5, 5, 1]                                                # transformers per level: 2 down + 3 up, and the middle block at the last
    folded = sum(n for L, n in zip(levels, blocks) if L % 32 == 0)
    fallback = 16 - folded
    assert (folded, fallback) == (10, 6)                                 # (16, 16): L = 256, 64 | 16, 4;  (8, 16): L = 128, 32 | 8, 2
    pd = plain.op_details()
    for L, n, C in zip(levels, blocks, (320, 640, 1280, 1280)):
        # the score GEMM, N = k * heads * 80, and the output GEMM, K = k * heads * 80 (counted against the plain graph: at k = 3 the
        # score GEMM of the C = 640 level has the shape of that level's q|k|v projection; the output GEMM may be planned split-K)
        score, out_gemm = f'rows M{2 * L} N{640 * k} K{C} x1', f'rows M{2 * L} N{C} K{640 * k} x'
        want = n if L % 32 == 0 else 0
        assert details.count(score) - pd.count(score) == want, (L, C, score)
        assert sum(l != 'splitk_reduce' and d.startswith(out_gemm) for l, d in zip(labels, details)) - \
            sum(l != 'splitk_reduce' and d.startswith(out_gemm) for l, d in zip(pl, pd)) == want, (L, C, out_gemm)
    assert labels.count('region_blend') == fallback
    cross = sum(l.startswith('attn_d') for l in labels) - 16
    assert cross == fallback * 2 * k
    reduces = labels.count('splitk_reduce') - pl.count('splitk_reduce')   # (the wider GEMMs may be planned split-K: a reduce launch each)
    assert len(labels) - reduces == len(pl) + fallback * (2 * k - 1 + 1)  # 2 k - 1 more attention launches and one blend per such block
    assert g.tune_source()['shapes_tuned_in_process'] == 0, g.tune_source()
    assert g.stats()['weight_bytes'] == plain.stats()['weight_bytes']


@pytest.mark.parametrize('k', [2, 3])
@pytest.mark.parametrize('hw', SIZES)
def test_unet_with_regions_matches_the_restatement(weights, oracle, hw, k):
    g, tg = _graph(weights, hw, k)
    x, ctx, t = _inputs(hw, k)
    split = RR.column_split(hw, 52, k)
    if k == 3:
        split[2, 8 * hw[0] // 2:] = split[1, 8 * hw[0] // 2:]          # the third region takes the lower half of the second
        split[1, 8 * hw[0] // 2:] = 0
    cases = {'split52': RR.region_weights(split), 'soft': RR.region_weights(RR.soft_masks(hw, k, seed=3)),
             'swapped': RR.region_weights(split.flip(0))}
    ref = {n: RR.regional_unet(oracle, w)(x, t, ctx.float()) for n, w in cases.items()}
    moved = rel_l2(ref['swapped'], ref['split52'])
    assert moved > 5e-2, moved                                           # masks matter: on the CPU, before any GPU work
    out = {}
    for n, w in cases.items():
        out[n] = _eval(g, tg, x, ctx, t, w)
        r = rel_l2(out[n], ref[n])
        print(f'UNet {hw} {k} regions, {n}: rel-L2 vs the fp32 restatement {r:.3e}')
        assert torch.isfinite(out[n]).all() and r <= 1e-2, (n, r)
    away = rel_l2(out['swapped'], out['split52'])
    print(f'UNet {hw} {k} regions: swapped masks move the output by {away:.3e} (restatement {moved:.3e})')
    assert away > 1e-2, away
    # region 0 everywhere: the plain oracle on the first 77 rows
    with torch.no_grad():
        plain0 = oracle(x, t, ctx[:, :77].float())
    o = _eval(g, tg, x, ctx, t, RR.background_weights(k, hw))
    r0 = rel_l2(o, plain0)
    # the same prompt in every region, soft masks: the plain oracle
    same = torch.cat([ctx[:, :77]] * k, 1)
    o = _eval(g, tg, x, same, t, cases['soft'])
    r1 = rel_l2(o, plain0)
    print(f'UNet {hw} {k} regions: region 0 everywhere {r0:.3e}, same prompt in every region {r1:.3e} (vs the plain fp32 oracle)')
    assert r0 <= 1e-2 and r1 <= 1e-2, (r0, r1)
    for slot, w in zip(g.region_w, RR.background_weights(k, hw)):
        slot.copy_(w)


def test_a_replay_picks_up_new_masks(weights):
    """the weights are inputs the kernels read: the captured graph needs no recapture, at the folded levels and at the others"""
    hw, k = (16, 16), 2
    g, tg = _graph(weights, hw, k)
    x, ctx, t = _inputs(hw, k)
    wa = RR.region_weights(RR.column_split(hw, 52, k)); wb = RR.region_weights(RR.column_split(hw, 52, k).flip(0))
    a = _eval(g, tg, x, ctx, t, wa)
    b = _eval(g, tg, x, ctx, t, wb)
    assert rel_l2(a, b) > 1e-2
    for slot, w in zip(g.region_w, wa):
        slot.copy_(w)
    g.execute(use_hip_graph=True, static_unchanged=True); torch.cuda.synchronize()
    assert torch.equal(nchw(g.eps), a)
    prev = a
    for lvl in (3, 2, 1, 0):                                             # one level at a time, the deepest (blend kernel) first
        g.region_w[lvl].copy_(wb[lvl])
        g.execute(use_hip_graph=True, static_unchanged=True); torch.cuda.synchronize()
        cur = nchw(g.eps)
        assert not torch.equal(cur, prev), lvl                           # every level's weights are read by the replay
        prev = cur
    assert torch.equal(prev, b)
    for slot, w in zip(g.region_w, RR.background_weights(k, hw)):
        slot.copy_(w)


# ------------------------------------------------------------------ the pipeline
class _Words:
    """a stand-in tokenizer: SOT, one id per word, EOT, EOT padding (CLIP's layout; the ids are arbitrary but fixed)"""

    def encode(self, text):
        ids = [49406] + [1000 + sum(map(ord, w)) % 40000 for w in text.split()][:75]
        return ids + [49407] * (77 - len(ids))


@pytest.fixture(scope='module')
def rig(weights, oracle):
    from sdod.amd.pipeline import Txt2Img
    kw = dict(state_dicts=weights, images_per_gpu=1, latent_hw=16, tokenizer=_Words(), with_vae_encoder=True, loras=True)
    pipe = Txt2Img(regions=2, **kw)
    plain = Txt2Img(**kw)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 154, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    m = RR.column_split((16, 16), 52)
    return dict(pipe=pipe, plain=plain, unet=oracle, ctx2=ctx2, x_T=x_T, masks=m, swapped=m.flip(0))


def test_pipeline_construction_and_refusals(rig, weights):
    from sdod.amd.pipeline import Txt2Img
    pipe, plain = rig['pipe'], rig['plain']
    assert pipe.regions == 2 and pipe.unet.cfg.regions == 2 and pipe.unet.cfg.context_len == 154 and pipe.cfg.context_len == 77
    assert pipe.cfg.regions == 0 and pipe.text.batch == 4 and tuple(pipe.unet.ctx.shape) == (2, 154, 768) and len(pipe.unet.region_w) == 4
    assert plain.regions == 0 and plain.text.batch == 2 and not hasattr(plain.unet, 'region_w')
    assert (plain.unet.stats()['launches'], plain.unet.stats()['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES)
    for call in (lambda: plain.set_regions(rig['masks']), plain.clear_regions, lambda: plain.encode_regions(['a', 'b'])):
        with pytest.raises(RuntimeError, match='regions=k'):
            call()
    for bad in (rig['masks'].float(), rig['masks'][:1], rig['masks'][:, :64], torch.zeros(3, 128, 128, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            pipe.set_regions(bad)
    for kw in (dict(prompt_chunks=2), dict(cfg_split=True), dict(hires_hw=32), dict(controlnet=True), dict(adapter=True), dict(tiling=True),
               dict(inpaint_unet=True), dict(model='sd21'), dict(weight_quant=True)):
        with pytest.raises(ValueError, match='regions'):
            Txt2Img(state_dicts=weights, latent_hw=16, with_text_encoder=False, regions=2, **kw)
    assert all(torch.equal(w.cpu(), r) for w, r in zip(pipe.unet.region_w, RR.background_weights(2, (16, 16))))


def test_encode_regions(rig):
    pipe, plain = rig['pipe'], rig['plain']
    c = pipe.encode_regions(['a red fox', 'a snowy owl'], 'blurry')
    assert tuple(c.shape) == (2, 154, 768) and c.dtype == torch.float16 and bool(torch.isfinite(c).all())
    fox, owl = plain.encode_prompt('a red fox', 'blurry'), plain.encode_prompt('a snowy owl', 'blurry')
    for got, want in ((c[0, :77], fox[0]), (c[0, 77:], fox[0]), (c[1, :77], fox[1]), (c[1, 77:], owl[1])):
        assert rel_l2(got.float(), want.float()) <= 2e-3                 # the same encoder at another batch (other GEMM tiles)
    assert torch.equal(c[0, :77], c[0, 77:]) and not torch.equal(c[1, :77], c[1, 77:])
    assert torch.equal(pipe.encode_regions(('a red fox', 'a snowy owl'), 'blurry'), c)
    for bad in (['one'], ['a', 'b', 'c'], 'ab', None, ['a', 7]):
        with pytest.raises(ValueError, match='exactly 2'):
            pipe.encode_regions(bad)
    with pytest.raises(ValueError, match='negative'):
        pipe.encode_regions(['a', 'b'], ['x', 'y'])
    with pytest.raises(ValueError):
        pipe.encode_chunks(np.zeros((1, 77), np.int64), np.zeros((1, 77), np.int64))


@pytest.mark.parametrize('sampler', ['plms', 'dpmpp_2m'])
def test_eager_and_captured_are_the_same_and_new_masks_need_no_capture(rig, sampler):
    pipe, c, x_T = rig['pipe'], rig['ctx2'].cuda(), rig['x_T']
    pipe.clear_regions()
    base = pipe.generate(c, x_T, 4, 7.5, sampler).clone()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base)
    n_graphs = len(pipe._traj)
    pipe.set_regions(rig['masks'])
    assert all(torch.equal(w.cpu(), r) for w, r in zip(pipe.unet.region_w, RR.region_weights(rig['masks'])))
    graphed = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs                                   # no new trajectory: a replay of the same capture
    assert not torch.equal(graphed, base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), graphed)
    pipe.set_regions(rig['swapped'].numpy())
    swapped = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs and not torch.equal(swapped, graphed)
    assert torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), swapped)
    pipe.clear_regions()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
    assert len(pipe._traj) == n_graphs
    # region 0 everywhere IS the plain pipeline on the first prompt, to the fp16 graphs' accuracy (other GEMM shapes, same numbers)
    plain = rig['plain'].generate(c[:, :77].contiguous(), x_T, 4, 7.5, sampler)
    assert base.shape == plain.shape and base.dtype == plain.dtype


def test_pipelined_entry_point_and_img2img_run_with_regions(rig):
    pipe, c, x_T = rig['pipe'], rig['ctx2'].cuda(), rig['x_T']
    pipe.set_regions(rig['masks'])
    try:
        img = pipe.generate(c, x_T, 4, 7.5, 'plms')
        piped, ev = pipe.generate_pipelined(c, x_T, 4, 7.5, 'plms')
        ev.synchronize()                                                 # (the images are valid once the decode's event has completed)
        assert torch.equal(piped, img)
        u8 = torch.randint(0, 256, (1, 128, 128, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
        g = torch.Generator().manual_seed(6)
        noise = (torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g))
        a = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
        assert torch.equal(a, pipe.img2img(c, u8, 0.5, 8, 7.5, noise=noise))
        pipe.set_regions(rig['swapped'])
        assert not torch.equal(pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise), a)
    finally:
        pipe.clear_regions()


def test_regional_latents_match_the_restatement_chain(rig):
    """20 PLMS steps with two regions split at pixel column 52 against the sampler restatement (oracle/pipeline_oracle.py) on the fp32
    regional UNet; the swapped masks give another latent"""
    from oracle import pipeline_oracle as PO
    pipe, x_T = rig['pipe'], rig['x_T']
    c16 = rig['ctx2'].float()
    model = RR.regional_unet(rig['unet'], RR.region_weights(rig['masks']))
    other = RR.regional_unet(rig['unet'], RR.region_weights(rig['swapped']))
    x2, t2 = x_T.repeat(2, 1, 1, 1), torch.tensor([981.0, 981.0])
    moved = rel_l2(other(x2, t2, c16), model(x2, t2, c16))              # the restatement's first evaluation under both mask orders
    assert moved > 5e-2, moved                                           # on the CPU, before any GPU work
    z_ref = PO.plms_sample(model, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5)
    try:
        pipe.set_regions(rig['masks'])
        z = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
        pipe.set_regions(rig['swapped'])
        z_sw = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
    finally:
        pipe.clear_regions()
    rl, away = rel_l2(z, z_ref), rel_l2(z_sw, z)
    print(f'regional plms final latent rel-L2 vs the restatement chain {rl:.3e}, vs the swapped-mask latent {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(z).all() and rl <= 2e-2 and away > 1e-2, (rl, away)


def test_set_loras_re_derives_the_region_fold(rig, weights):
    """an adapter on every attn2 weight (to_q and to_out go into the fold's W1 / W2, to_k and to_v into the K/V projection): the
    UNet with regions against the restatement on host-merged weights; clear_loras() restores the base output bit for bit"""
    from oracle import sd_torch as S
    from sdod.amd import lora as L
    pipe = rig['pipe']
    g = pipe.unet
    names = [n for n in LC.unet_targets(g.param_table()) if '.attn2.' in n]
    entries = LC.make_entries(weights['unet'], names, 4, 1.0, seed=5)       # scale 1: an update as large as the weights' own spread
    with torch.device('meta'):
        merged = S.UNetModel()
    merged.load_state_dict({**L.merged_state_dict(weights['unet'], entries), **weights['temb']}, assign=True)
    hw, k = (16, 16), 2
    x, ctx, t = _inputs(hw, k)
    ws = RR.region_weights(rig['masks'])
    ref = RR.regional_unet(merged.eval(), ws)(x, t, ctx.float())
    ref_base = RR.regional_unet(rig['unet'], ws)(x, t, ctx.float())
    assert rel_l2(ref, ref_base) > 5e-2                                  # the adapter matters: on the CPU, before any GPU work
    _, tg = _graph(weights, hw, 0)

    def run(fresh):
        tg.t.copy_(t); tg.execute()
        g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
        g.execute(use_hip_graph=True, static_unchanged=not fresh); torch.cuda.synchronize()
        return nchw(g.eps)
    pipe.set_regions(rig['masks'])
    try:
        base = run(True)
        assert rel_l2(base, ref_base) <= 1e-2
        g.set_loras(entries)
        out = run(False)                                                 # static_unchanged: the engine itself knows its fold is stale
        r = rel_l2(out, ref)
        print(f'UNet with regions and a LoRA on attn2: rel-L2 vs the restatement on merged weights {r:.3e}, vs the base output {rel_l2(out, base):.3e}')
        assert r <= 1e-2 and rel_l2(out, base) > 1e-2, r
        g.set_loras([])
        assert torch.equal(run(False), base)
    finally:
        g.set_loras([])
        pipe._ctx_fresh = True
        pipe.clear_regions()
