"""Image prompts on the GPU: the IMAGE_ENCODER and IMAGE_PROJ graphs and the UNET graph with ip_tokens against the
fp32 restatements of tests/ipadapter_ref.py, and the pipeline Txt2Img(ip_adapter=True).  Synthetic weights, batch 2, latents
(16, 16) and (8, 16): the first has two folded levels and two in the three-launch form, the second one and three.

Stated tolerances, the project's own for the same comparisons: an fp16 graph against the fp32 restatement rel-L2 <= 1e-2 (the
encoder graphs <= 5e-3, the text encoder test's bound); a 20-step PLMS chain's final latent <= 2e-2; everything else is bit-exact.
Before any GPU work the restatement is shown, on the CPU, to move by more than 5e-2 between s = 1 and s = 0."""
import pytest
import torch

import ipadapter_ref as IR
import lora_cases as LC

pytestmark = pytest.mark.gpu

# launch count and activation-arena bytes of the batch-2 16x16 UNet graph without the feature, as tests/test_regions_gpu.py records them
PARENT_LAUNCHES = 321
PARENT_ARENA_BYTES = 4260096
SIZES = [(16, 16), (8, 16)]
IP_SPREAD = 4.0                                                          # to_k_ip / to_v_ip ~ N(0, 16 / fan_in): see test_..._matches_the_restatement
VISION = {'d80': (28, 14, 320, 2, 4, 1280, 128, 0), 'd64': (56, 14, 128, 2, 2, 512, 64, 1)}


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


@pytest.fixture(scope='module')
def weights():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    table = E.UNet(cfg, 2).param_table()
    ip = IR.synthetic_ip_state_dict(table, seed=4321, spread=IP_SPREAD)
    enc = E.ImageEncoder(E.VisionConfig(*VISION['d80']), 1)
    image_encoder = Wt.synthetic_state_dict(enc.checkpoint_table(), seed=1241)
    return {'unet': Wt.synthetic_state_dict(table, seed=1234),
            'temb': Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235),
            'vae': Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1236),
            'vae_enc': Wt.synthetic_state_dict(E.VaeEncoder(cfg, 1).param_table(), seed=1238),
            'ip_kv': ip,
            'proj': {T: Wt.synthetic_state_dict(E.ImageProj(cfg, 128, T, 2).param_table(), seed=1240 + T) for T in (4, 16)},
            'image_encoder': image_encoder}


@pytest.fixture(scope='module')
def oracle(weights):
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**weights['unet'], **weights['temb']}, assign=True)
    return unet.eval()


def _inputs(hw, T, seed=11):
    gen = torch.Generator().manual_seed(seed + hw[0] + T)
    x = torch.randn(2, 4, *hw, generator=gen)
    ctx = (torch.randn(2, 77, 768, generator=gen) * 0.5).half()
    tok = torch.randn(2, T, 768, generator=gen).half()
    return x, ctx, tok, torch.tensor([999.0, 501.0])


_graphs = {}


def _graph(weights, hw, T):
    """one finalized (UNet with T image tokens, Temb) per size, shared by the tests of this module"""
    from sdod.amd import engine as E
    if (hw, T) not in _graphs:
        cfg = E.sd14_config(*hw)
        tg = E.Temb(cfg, 2); tg.load_state_dict(weights['temb']); tg.finalize()
        c = E.copy_config(cfg)
        c.ip_tokens = T
        g = E.UNet(c, 2); g.load_state_dict({**weights['unet'], **weights['ip_kv']}); g.finalize()
        _graphs[(hw, T)] = (g, tg)
    return _graphs[(hw, T)]


def _eval(g, tg, x, ctx, t, tok=None, ws=None):
    """eager, then the hip-graph replay: bit-equal; returns NCHW fp32 on the CPU"""
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    if tok is not None:
        g.ip_ctx.copy_(tok)
    if ws is not None:
        for slot, w in zip(g.ip_w, ws):
            slot.copy_(w)
    g.execute()
    torch.cuda.synchronize()
    eager = g.eps.clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.eps, eager)
    return nchw(eager)


# ------------------------------------------------------------------ the image side
@pytest.mark.parametrize('name', ['d80', 'd64'])
def test_image_encoder_matches_the_restatement(name):
    from sdod.amd import engine as E, weights as Wt
    v = VISION[name]
    enc = E.ImageEncoder(E.VisionConfig(*v), 2)
    sd = Wt.synthetic_state_dict(enc.checkpoint_table(), seed=1250 + v[2])
    enc.load_state_dict(sd); enc.finalize()
    tokens = (v[0] // v[1]) ** 2 + 1
    assert tokens == {'d80': 5, 'd64': 17}[name] and v[2] // v[4] == {'d80': 80, 'd64': 64}[name]
    img = torch.randint(0, 256, (2, v[0], v[0], 3), generator=torch.Generator().manual_seed(v[0]), dtype=torch.int32).to(torch.uint8)
    ref = IR.vision_forward(sd, img, v[1], v[4], bool(v[7]))
    enc.img.copy_(img)
    enc.execute(); torch.cuda.synchronize()
    eager = enc.out.clone()
    enc.execute(use_hip_graph=True); torch.cuda.synchronize()
    assert torch.equal(enc.out, eager)
    r = rel_l2(eager.float().cpu(), ref)
    labels = [l for l, _, _ in enc.op_table()]
    print(f'image encoder {name}: rel-L2 vs the fp32 restatement {r:.3e}, {len(labels)} launches')
    assert tuple(eager.shape) == (2, v[6]) and torch.isfinite(eager).all() and r <= 5e-3, r
    assert labels.count('patch_embed') == 1 and labels.count('vit_tokens') == 1 and sum(l.startswith('attn_d') for l in labels) == v[3]
    assert not torch.equal(eager[0], eager[1])


@pytest.mark.parametrize('T', [4, 16])
def test_image_projection_matches_the_restatement(weights, T):
    from sdod.amd import engine as E
    g = E.ImageProj(E.sd14_config(16, 16), 128, T, 2)
    g.load_state_dict(weights['proj'][T]); g.finalize()
    e = torch.randn(2, 128, generator=torch.Generator().manual_seed(T)).half()
    e[0] = 0                                                             # the unconditional row: image_proj(zeros)
    ref = IR.image_proj(weights['proj'][T], e.float(), T)
    g.embeds.copy_(e)
    g.execute(); torch.cuda.synchronize()
    eager = g.out.clone()
    g.execute(use_hip_graph=True); torch.cuda.synchronize()
    assert torch.equal(g.out, eager) and tuple(eager.shape) == (2, T, 768)
    r = rel_l2(eager.float().cpu(), ref)
    print(f'image projection T{T}: rel-L2 vs the fp32 restatement {r:.3e}')
    assert r <= 5e-3, r


# ------------------------------------------------------------------ the UNet
def test_plain_graph_is_unchanged(weights):
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    g = E.UNet(cfg, 2); g.load_state_dict(weights['unet']); g.finalize()
    s = g.stats()
    assert (s['launches'], s['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES) and not hasattr(g, 'ip_w') and not hasattr(g, 'ip_ctx')
    labels = [l for l, _, _ in g.op_table()]
    assert 'region_blend' not in labels and len(labels) == PARENT_LAUNCHES
    assert sum(l.startswith('attn_d') for l in labels) == 16 + 6
    assert not any('_ip' in n for n, _ in g.param_table())
    assert not any(d in g.op_details() for d in ('rows M512 N1280 K320 x1', 'rows M512 N320 K1280 x1', 'rows M128 N640 K1280 x1'))
    assert g.tune_source()['shapes_tuned_in_process'] == 0
    with pytest.raises(Exception):
        g._io(False, 3)                                                  # no fourth input
    # an all-zero image-prompt configuration builds the same graph through the new entry point
    import ctypes
    h = ctypes.c_void_p()
    lib = g._lib
    from sdod.amd._lib import check
    check(lib.sdod_graph_create_ip(ctypes.byref(h), E.UNET, ctypes.byref(cfg), ctypes.byref(E.IpConfig(0)), 2))
    try:
        assert lib.sdod_graph_num_params(h) == len(g.param_table())
    finally:
        lib.sdod_graph_destroy(h)


@pytest.mark.parametrize('T', [4, 16])
@pytest.mark.parametrize('hw', SIZES)
def test_launch_list_with_an_image_prompt(weights, hw, T):
    from sdod.amd import engine as E
    g, _ = _graph(weights, hw, T)
    plain = E.UNet(E.sd14_config(*hw), 2); plain.load_state_dict(weights['unet']); plain.finalize()
    labels, details = [l for l, _, _ in g.op_table()], g.op_details()
    pl, pd = [l for l, _, _ in plain.op_table()], plain.op_details()
    assert [tuple(w.shape) for w in g.ip_w] == [((hw[0] >> l) * (hw[1] >> l), 2) for l in range(4)] and tuple(g.ip_ctx.shape) == (2, T, 768)
    assert all(torch.equal(w.cpu(), r) for w, r in zip(g.ip_w, IR.ip_weights(0.0, hw)))                  # (1, 0) at finalize
    levels = [(hw[0] >> l) * (hw[1] >> l) for l in range(4)]
    blocks = [5, 5, 5, 1]
    folded = sum(n for L, n in zip(levels, blocks) if L % 32 == 0)
    fallback = 16 - folded
    assert (folded, fallback) == (10, 6)
    for L, n, C in zip(levels, blocks, (320, 640, 1280, 1280)):
        score, out_gemm = f'rows M{2 * L} N1280 K{C} x1', f'rows M{2 * L} N{C} K1280 x'
        want = n if L % 32 == 0 else 0
        assert details.count(score) - pd.count(score) == want, (L, C, score)
        assert sum(l != 'splitk_reduce' and d.startswith(out_gemm) for l, d in zip(labels, details)) - \
            sum(l != 'splitk_reduce' and d.startswith(out_gemm) for l, d in zip(pl, pd)) == want, (L, C, out_gemm)
    assert labels.count('region_blend') == fallback
    assert sum(l.startswith('attn_d') for l in labels) - 16 == fallback * 4                             # one per (image, segment)
    reduces = labels.count('splitk_reduce') - pl.count('splitk_reduce')
    assert len(labels) - reduces == len(pl) + fallback * 4                                              # 3 more attention launches and one blend
    # the image tokens' K / V of all 16 blocks: 32 more matrices [C, 768], and nothing else
    extra = sum(2 * c * 768 * 2 for _, c in __import__('sdod.amd.ip_adapter', fromlist=['BLOCKS']).BLOCKS)
    assert 0 <= g.stats()['weight_bytes'] - plain.stats()['weight_bytes'] - extra < 4096
    assert g.tune_source()['shapes_tuned_in_process'] == 0, g.tune_source()         # every tile from the shipped tables (gfx950_ip.tune)


@pytest.mark.parametrize('T', [4, 16])
@pytest.mark.parametrize('hw', SIZES)
def test_unet_with_an_image_prompt_matches_the_restatement(weights, oracle, hw, T):
    x, ctx, tok, t = _inputs(hw, T)
    cases = {'s1': IR.ip_weights(1.0, hw), 's0.5 soft': IR.ip_weights(0.5, hw, IR.soft_mask(hw, 5)), 's0': IR.ip_weights(0.0, hw)}
    ref = {n: IR.ip_unet(oracle, weights['ip_kv'], tok.float(), w)(x, t, ctx.float()) for n, w in cases.items()}
    moved = rel_l2(ref['s1'], ref['s0'])
    print(f'restatement {hw} T{T}: s = 1 moves the output by {moved:.3e} against s = 0')
    assert moved > 5e-2, moved                                           # the image prompt matters: on the CPU, before any GPU work
    with torch.no_grad():
        plain = oracle(x, t, ctx.float())
    assert rel_l2(ref['s0'], plain) < 1e-5                               # s = 0 is the plain model
    g, tg = _graph(weights, hw, T)
    out = {}
    for n, w in cases.items():
        out[n] = _eval(g, tg, x, ctx, t, tok, w)
        r = rel_l2(out[n], ref[n])
        print(f'UNet {hw} T{T}, {n}: rel-L2 vs the fp32 restatement {r:.3e}')
        assert torch.isfinite(out[n]).all() and r <= 1e-2, (n, r)
    assert rel_l2(out['s1'], out['s0']) > 1e-2
    r0 = rel_l2(out['s0'], plain)
    other = _eval(g, tg, x, ctx, t, tok.flip(0).contiguous() * 2, cases['s0'])
    print(f'UNet {hw} T{T}: s = 0 vs the plain fp32 oracle {r0:.3e}')
    assert r0 <= 1e-2 and torch.equal(other, out['s0'])                  # weight 0: exact zeros whatever the tokens are


def test_a_replay_picks_up_new_tokens_and_weights(weights):
    hw, T = (16, 16), 4
    g, tg = _graph(weights, hw, T)
    x, ctx, tok, t = _inputs(hw, T)
    wa, wb = IR.ip_weights(1.0, hw), IR.ip_weights(0.6, hw, IR.soft_mask(hw, 8))
    a = _eval(g, tg, x, ctx, t, tok, wa)
    b = _eval(g, tg, x, ctx, t, tok, wb)
    assert rel_l2(a, b) > 1e-3
    for slot, w in zip(g.ip_w, wa):
        slot.copy_(w)
    g.execute(use_hip_graph=True, static_unchanged=True); torch.cuda.synchronize()
    assert torch.equal(nchw(g.eps), a)
    prev = a
    for lvl in (3, 2, 1, 0):                                             # one level at a time, the deepest (blend kernel) first
        g.ip_w[lvl].copy_(wb[lvl])
        g.execute(use_hip_graph=True, static_unchanged=True); torch.cuda.synchronize()
        cur = nchw(g.eps)
        assert not torch.equal(cur, prev), lvl
        prev = cur
    assert torch.equal(prev, b)
    g.ip_ctx.copy_(tok.flip(0).contiguous())                             # new tokens: the static launches run again
    g.execute(use_hip_graph=True); torch.cuda.synchronize()
    c = nchw(g.eps)
    assert not torch.equal(c, b) and torch.equal(c, _eval(g, tg, x, ctx, t, tok.flip(0).contiguous(), wb))
    for slot, w in zip(g.ip_w, IR.ip_weights(0.0, hw)):
        slot.copy_(w)


# ------------------------------------------------------------------ the pipeline
@pytest.fixture(scope='module')
def rig(weights, oracle):
    from sdod.amd import ip_adapter as IP
    from sdod.amd.pipeline import Txt2Img
    enc = dict(weights['image_encoder'])
    enc[IP.CONFIG_KEY] = torch.tensor(VISION['d80'], dtype=torch.float32)
    sds = {'unet': weights['unet'], 'temb': weights['temb'], 'vae': weights['vae'], 'vae_enc': weights['vae_enc'],
           'ip_adapter': {**weights['proj'][4], **weights['ip_kv']}, 'image_encoder': enc}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, with_text_encoder=False, with_vae_encoder=True, loras=True, ip_adapter=True)
    g = torch.Generator().manual_seed(78)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    embeds = [torch.randn(1, 128, generator=g), torch.randn(1, 128, generator=g)]
    image = torch.randint(0, 256, (1, 28, 28, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    return dict(pipe=pipe, sds=sds, unet=oracle, ctx2=ctx2, x_T=x_T, embeds=embeds, image=image, mask=IR.soft_mask((16, 16), 9))


def _ref_tokens(weights, embeds):
    """[uncond ; cond] rows as the pipeline stages them: image_proj(zeros) ; image_proj(embeds), on the fp16 embeddings"""
    e = torch.cat([torch.zeros_like(embeds), embeds]).half().float()
    return IR.image_proj(weights['proj'][4], e, 4)


def test_pipeline_construction(rig, weights):
    pipe = rig['pipe']
    assert pipe.ip_tokens == 4 and pipe.ip_proj_dim == 128 and pipe.ip_image_size == 28 and pipe.unet.cfg.ip_tokens == 4 and pipe.cfg.ip_tokens == 0
    assert pipe.image_proj.batch == 2 and pipe.image_proj.out.data_ptr() == pipe.unet.ip_ctx.data_ptr()
    assert all(torch.equal(w.cpu(), r) for w, r in zip(pipe.unet.ip_w, IR.ip_weights(0.0, (16, 16))))
    pipe.set_image_prompt(embeds=rig['embeds'][0], weight=0.7, mask_u8=rig['mask'])
    try:
        assert all(torch.equal(w.cpu(), r) for w, r in zip(pipe.unet.ip_w, IR.ip_weights(0.7, (16, 16), rig['mask'])))
        r = rel_l2(pipe.unet.ip_ctx.float().cpu(), _ref_tokens(weights, rig['embeds'][0]))
        assert r <= 5e-3, r
    finally:
        pipe.clear_image_prompt()
    assert all(torch.equal(w.cpu(), r) for w, r in zip(pipe.unet.ip_w, IR.ip_weights(0.0, (16, 16))))


@pytest.mark.parametrize('sampler', ['plms', 'dpmpp_2m'])
def test_eager_and_captured_are_the_same_and_a_new_image_prompt_needs_no_capture(rig, sampler):
    pipe, c, x_T = rig['pipe'], rig['ctx2'].cuda(), rig['x_T']
    pipe.clear_image_prompt()
    base = pipe.generate(c, x_T, 4, 7.5, sampler).clone()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base)
    n_graphs = len(pipe._traj)
    try:
        pipe.set_image_prompt(embeds=rig['embeds'][0], weight=1.0)
        graphed = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
        assert len(pipe._traj) == n_graphs                               # no new trajectory: a replay of the same capture
        assert not torch.equal(graphed, base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), graphed)
        pipe.set_image_prompt(embeds=rig['embeds'][1], weight=0.6, mask_u8=rig['mask'])       # another image, weight and mask
        other = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
        assert len(pipe._traj) == n_graphs and not torch.equal(other, graphed)
        assert torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), other)                      # a fresh eager run
    finally:
        pipe.clear_image_prompt()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
    assert len(pipe._traj) == n_graphs


def test_image_and_its_embeds_give_identical_images(rig):
    pipe, c, x_T = rig['pipe'], rig['ctx2'].cuda(), rig['x_T']
    try:
        pipe.set_image_prompt(rig['image'], weight=0.8)
        a = pipe.generate(c, x_T, 4, 7.5, 'plms').clone()
        e = pipe.image_embeds(rig['image'])
        assert tuple(e.shape) == (1, 128) and e.dtype == torch.float16
        pipe.set_image_prompt(embeds=e.cpu(), weight=0.8)
        assert torch.equal(pipe.generate(c, x_T, 4, 7.5, 'plms'), a)
        pipe.set_image_prompt(embeds=rig['embeds'][0], weight=0.8)
        assert not torch.equal(pipe.generate(c, x_T, 4, 7.5, 'plms'), a)
    finally:
        pipe.clear_image_prompt()


def test_img2img_runs_with_an_image_prompt(rig):
    pipe, c = rig['pipe'], rig['ctx2'].cuda()
    u8 = torch.randint(0, 256, (1, 128, 128, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    g = torch.Generator().manual_seed(6)
    noise = (torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g))
    pipe.clear_image_prompt()
    base = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
    try:
        pipe.set_image_prompt(embeds=rig['embeds'][0], weight=1.0)
        a = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
        assert not torch.equal(a, base) and torch.equal(a, pipe.img2img(c, u8, 0.5, 8, 7.5, noise=noise))
    finally:
        pipe.clear_image_prompt()


def test_latents_with_an_image_prompt_match_the_restatement_chain(rig, weights):
    """20 PLMS steps with an image prompt at weight 1 against the sampler restatement (oracle/pipeline_oracle.py) on the fp32 UNet
    with decoupled cross-attention"""
    from oracle import pipeline_oracle as PO
    pipe, x_T = rig['pipe'], rig['x_T']
    c16 = rig['ctx2'].float()
    tok = _ref_tokens(weights, rig['embeds'][0])
    ws = IR.ip_weights(1.0, (16, 16))

    model = IR.ip_unet(rig['unet'], weights['ip_kv'], tok, ws)         # (the sampler restatement evaluates [uncond ; cond] rows at once)
    off = IR.ip_unet(rig['unet'], weights['ip_kv'], tok, IR.ip_weights(0.0, (16, 16)))
    x2, t2 = x_T.repeat(2, 1, 1, 1), torch.tensor([981.0, 981.0])
    moved = rel_l2(model(x2, t2, c16), off(x2, t2, c16))
    assert moved > 5e-2, moved                                           # on the CPU, before any GPU work
    z_ref = PO.plms_sample(model, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5)
    try:
        pipe.set_image_prompt(embeds=rig['embeds'][0], weight=1.0)
        z = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
        pipe.clear_image_prompt()
        z0 = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
    finally:
        pipe.clear_image_prompt()
    rl, away = rel_l2(z, z_ref), rel_l2(z0, z)
    print(f'image-prompt plms final latent rel-L2 vs the restatement chain {rl:.3e}, vs the latent without the prompt {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(z).all() and rl <= 2e-2 and away > 1e-2, (rl, away)


def test_set_loras_re_derives_the_image_prompt_fold(rig, weights):
    """an adapter on every attn2 weight of the base model (to_q and to_out go into the fold's W1 / W2 of BOTH segments): the UNet
    with an image prompt against the restatement on host-merged weights; set_loras([]) restores the base output bit for bit"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E, lora as L
    pipe = rig['pipe']
    g = pipe.unet
    names = [n for n in LC.unet_targets(g.param_table()) if '.attn2.' in n and '_ip' not in n]
    entries = LC.make_entries(weights['unet'], names, 4, 1.0, seed=5)
    with torch.device('meta'):
        merged = S.UNetModel()
    merged.load_state_dict({**L.merged_state_dict(weights['unet'], entries), **weights['temb']}, assign=True)
    hw = (16, 16)
    x, ctx, _, t = _inputs(hw, 4)
    tok = _ref_tokens(weights, rig['embeds'][0])
    ws = IR.ip_weights(1.0, hw)
    ref = IR.ip_unet(merged.eval(), weights['ip_kv'], tok, ws)(x, t, ctx.float())
    ref_base = IR.ip_unet(rig['unet'], weights['ip_kv'], tok, ws)(x, t, ctx.float())
    assert rel_l2(ref, ref_base) > 5e-2                                  # the adapter matters: on the CPU, before any GPU work
    tg = E.Temb(E.sd14_config(*hw), 2); tg.load_state_dict(weights['temb']); tg.finalize()

    def run(fresh):
        tg.t.copy_(t); tg.execute()
        g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
        g.execute(use_hip_graph=True, static_unchanged=not fresh); torch.cuda.synchronize()
        return nchw(g.eps)
    pipe.set_image_prompt(embeds=rig['embeds'][0], weight=1.0)
    try:
        base = run(True)
        assert rel_l2(base, ref_base) <= 1e-2
        g.set_loras(entries)
        out = run(False)                                                 # static_unchanged: the engine itself knows its fold is stale
        r = rel_l2(out, ref)
        print(f'UNet with an image prompt and a LoRA on attn2: rel-L2 vs the restatement on merged weights {r:.3e}, vs the base output {rel_l2(out, base):.3e}')
        assert r <= 1e-2 and rel_l2(out, base) > 1e-2, r
        g.set_loras([])
        assert torch.equal(run(False), base)
    finally:
        g.set_loras([])
        pipe._ctx_fresh = True
        pipe.clear_image_prompt()


def test_two_images_per_gpu_take_two_image_prompts(rig):
    from sdod.amd.pipeline import Txt2Img
    pipe2 = Txt2Img(state_dicts=rig['sds'], images_per_gpu=2, latent_hw=16, with_text_encoder=False, ip_adapter=True)
    c = rig['ctx2'].cuda()
    x_T = rig['x_T'].repeat(2, 1, 1, 1)                                   # the same noise for both images
    A, B = rig['embeds']
    C = torch.randn(1, 128, generator=torch.Generator().manual_seed(3))
    pipe2.set_image_prompt(embeds=torch.cat([A, B]), weight=1.0)
    ab = pipe2.generate(c, x_T, 4, 7.5, 'plms').clone()
    assert not torch.equal(ab[0], ab[1])                                 # only the image prompts differ
    pipe2.set_image_prompt(embeds=torch.cat([A, C]), weight=1.0)
    ac = pipe2.generate(c, x_T, 4, 7.5, 'plms').clone()
    assert torch.equal(ac[0], ab[0]) and not torch.equal(ac[1], ab[1])   # image 0 reads its own prompt alone, image 1 the other
    pipe2.set_image_prompt(embeds=torch.cat([C, B]), weight=1.0)
    cb = pipe2.generate(c, x_T, 4, 7.5, 'plms')
    assert torch.equal(cb[1], ab[1]) and not torch.equal(cb[0], ab[0])
