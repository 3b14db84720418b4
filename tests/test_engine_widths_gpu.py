"""Oracle parity of the graphs at the widths the configuration contract admits (tests/test_config_contract_cpu.py) but no SD checkpoint
has: model_channels 64 / 128 / 192, model_channels 320 with head dims 40 / 80 / 160, a VAE 64 or 256 wide, a text tower 128 wide.
Same pattern as tests/test_engine_gpu.py -- seeded synthetic weights, the fp32 CPU oracle of oracle/sd_torch.py on the same tensors --
at the small sizes where every form the builders choose between is reached:

  case        config                              latent   what it reaches
  w64         mc 64, head_dim 64, ctx 128         32x32    no level folds (heads 1 / 2 / 4: level 2 passed the old gate and failed in the
                                                           kernel); GroupNorm at 2 channels per group; one-launch conv_in at 64
  w128        mc 128, head_dim 64, ctx 128        32x32    the same at heads 2 / 4 / 8; GroupNorm at 4 channels per group
  w192        mc 192, head_dim 64, ctx 768        16x16    im2col + GEMM input convolution, wrap 0 and wrap 3 (latent_prep + wrapped
                                                           im2col); GroupNorm at 6 channels per group
  w320_d40    mc 320, head_dim 40                 32x32    fold at heads 8 / 16 / 32; plain d = 40 attention, 32 heads at L = 16
  w320_d80    mc 320, head_dim 80                 32x32    fold at heads 4 / 8 / 16
  w320_d160   mc 320, head_dim 160                32x32    level 0 (2 heads) plain d = 160 attention at L = 1024; fold at levels 1, 2
  w64_u8      w64, weight_quant 1, uint8 weights  16x16    LayerNorm launches and separate skip GEMMs at small widths
  w64_lin     w64, linear_proj 1                  16x16    Linear projections off SD 2's width

Each UNet case asserts: finite; rel-L2 <= 1e-2 against the oracle for the batch AND for each image alone (a per-image stride mistake
in the folded GEMMs moves one image only); TEMB <= 5e-3; two hipGraph replays, the second with static_unchanged, equal to the eager
bits; the launch list holds the forms of the table above; no GEMM shape was timed in process (SDOD_AUTOTUNE=0: the static plan).
Then the VAE decoder and encoder 64 and 256 wide (<= 1e-2), the text tower 128 wide in both dialects (<= 5e-3, replay = eager), and
regional prompts and an image prompt at w64 32x32, where only sdod_xattn_fold_ok keeps level 2 off the fold (<= 1e-2).  Tolerances
are the project's own for the same comparisons (tests/test_engine_gpu.py, tests/test_pipeline_gpu.py for uint8 weights).

Measured on the MI355X (rel-L2 against the oracle: the batch; the worse single image; TEMB; launches per evaluation):

  w64                 1.92e-3   1.97e-3   5.1e-4   319
  w128                1.65e-3   1.65e-3   4.9e-4   342
  w192 wrap 0         1.34e-3   1.35e-3   4.9e-4   343
  w192 wrap 3         1.43e-3   1.43e-3   4.9e-4   344
  w320_d40            1.67e-3   1.67e-3   4.8e-4   346
  w320_d80            1.66e-3   1.75e-3   4.8e-4   341
  w320_d160           1.70e-3   1.71e-3   4.8e-4   341
  w64_u8              1.75e-3   1.80e-3   3.6e-4   402   (the fp16 graph of that size: 319)
  w64_lin             1.78e-3   1.82e-3   4.9e-4   319
  w64 regions (2)     1.91e-3   1.96e-3            (6.8e-2 away from "region 0 everywhere")
  w64 image prompt    2.35e-3   2.42e-3            (8.1e-1 away from no image prompt)
  VAE decoder         ch 64: 1.23e-3   ch 256: 1.35e-3
  VAE encoder         ch 64: 1.71e-3 (mean 1.88e-3, logvar 1.62e-3)   ch 256: 1.45e-3 (mean 1.47e-3, logvar 1.42e-3)
  text tower d 128    HF names: 9.9e-4   open_clip names: 1.01e-3

With the fold decided by sdod_xattn_fold_ok no kernel needed a fix: every width the contract admits ran within tolerance the first time
it ran.  (Behind the builder's old gate w64, w128 and the two w64 forks returned INVALID_ARGUMENT from the first execute().)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

UNET_TOL, TEMB_TOL, VAE_TOL, TEXT_TOL = 1e-2, 5e-3, 1e-2, 5e-3


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(autouse=True)
def static_plan(monkeypatch):
    """the static tile plan decides: nothing is timed and the launch list is the same in every process"""
    monkeypatch.setenv('SDOD_AUTOTUNE', '0')


def width_config(mc, head_dim, ctx, hw, **kw):
    from sdod.amd import engine as E
    cfg = E.sd14_config(hw, hw)
    cfg.model_channels, cfg.num_heads, cfg.head_dim, cfg.context_dim = mc, 0, head_dim, ctx
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


class Width:
    """one width's seeded UNET + TEMB state dict (canonical layouts, ldm names) and the oracles that share its tensors"""

    def __init__(self, mc, ctx, seed, linear=False, quant=False):
        from sdod.amd import engine as E, weights as Wt
        self.mc, self.ctx, self.linear = mc, ctx, linear
        cfg = width_config(mc, 64, ctx, 16, linear_proj=int(linear))     # (the tables do not depend on the head dim or the size)
        self.sd = Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=seed)
        self.sd.update(Wt.synthetic_state_dict(E.Temb(cfg, 2).param_table(), seed=seed + 1))
        self.load = self.sd
        if quant:       # per-tensor affine uint8, as tests/test_pipeline_gpu.py: the oracle computes on the SAME dequantised values
            self.load = Wt.quantize_state_dict(self.sd)
            self.sd = {k: (v.dequantize() if isinstance(v, Wt.QuantU8) else v) for k, v in self.load.items()}
        self._oracles = {}

    def oracle(self, head_dim, tiling=None):
        from oracle import sd_torch as S
        key = (head_dim, tiling)
        if key not in self._oracles:
            with torch.device('meta'):
                m = S.UNetModel(model_ch=self.mc, head_dim=head_dim, context_dim=self.ctx, use_linear=self.linear)
            m.load_state_dict(self.sd, assign=True)
            if tiling:
                from test_tiling_gpu import flip
                m = flip(m, tiling)
            self._oracles[key] = m.eval()
        return self._oracles[key]


@pytest.fixture(scope='module')
def w64():
    return Width(64, 128, seed=6400)


@pytest.fixture(scope='module')
def w128():
    return Width(128, 128, seed=12800)


@pytest.fixture(scope='module')
def w192():
    return Width(192, 768, seed=19200)


@pytest.fixture(scope='module')
def w320():
    return Width(320, 768, seed=32000)


def temb_reference(unet, t):
    """the TEMB graph's output: the time embedding through every ResBlock's emb_layers, in the order the UNet visits them"""
    from oracle import sd_torch as S
    emb = unet.time_embed(S.timestep_embedding(t, unet.model_ch))
    blocks = [m[0] for m in list(unet.input_blocks) + [unet.middle_block] + list(unet.output_blocks) if isinstance(m[0], S.ResBlock)]
    blocks.insert(blocks.index(unet.middle_block[0]) + 1, unet.middle_block[2])
    return torch.cat([b.emb_layers(emb) for b in blocks], dim=1)


def labels_of(g):
    return [lab for lab, _, _ in g.op_table()]


def count_forms(g):
    """the forms in the per-evaluation launch list.  A transformer block has one self-attention launch (lq == lk) and, in the
    three-launch form, one cross-attention launch on the 77 keys; the folded form has none (its xattn_fold launch is in the
    once-per-prompt list, which op_table() does not show), so: folded blocks = self-attention launches - cross-attention launches"""
    labels = labels_of(g)
    attn, self_attn, cross_attn = {}, 0, 0
    for lab, det in zip(labels, g.op_details()):
        if lab.startswith('attn_d'):
            attn[lab] = attn.get(lab, 0) + 1
            shape = dict((k.rstrip('0123456789'), int(k[len(k.rstrip('0123456789')):])) for k in det.split())
            if shape['lk'] == 77 and shape['lq'] != 77:
                cross_attn += 1
            else:
                assert shape['lq'] == shape['lk'], det
                self_attn += 1
    assert self_attn == 16, (self_attn, cross_attn)
    return {'xattn_fold': self_attn - cross_attn, 'attn': attn, 'conv_in': labels.count('conv_in'),
            'latent_im2col': labels.count('latent_im2col'), 'latent_prep': labels.count('latent_prep'), 'im2col_wrap': labels.count('im2col_wrap'),
            'layer_norm': labels.count('layer_norm')}


def run_unet_case(name, width, cfg, head_dim, seed, wrap=None, tiling=None):
    """builds UNET + TEMB on `cfg`, evaluates once, checks accuracy (batch and each image), the replays and the tile provenance;
    returns the graph for the caller's look at the launch list"""
    from sdod.amd import engine as E
    hw, ctx_dim = cfg.latent_h, cfg.context_dim
    g = E.UNet(cfg, 2, wrap=wrap)
    g.load_state_dict(width.load)
    g.finalize()
    tg = E.Temb(cfg, 2)
    tg.load_state_dict(width.load)
    tg.finalize()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 4, hw, hw, generator=gen)
    ctx = torch.randn(2, 77, ctx_dim, generator=gen).half()
    t = torch.tensor([999.0, 251.0])
    unet = width.oracle(head_dim, tiling)
    with torch.no_grad():
        ref = unet(x, t, ctx.float())
        ref_temb = temb_reference(unet, t)
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    g.execute()
    torch.cuda.synchronize()
    g.check()
    eager = g.eps.clone()
    out = eager.float().cpu().permute(0, 3, 1, 2)
    r_temb = rel_l2(tg.out.float().cpu(), ref_temb)
    r = rel_l2(out, ref)
    r_img = [rel_l2(out[i], ref[i]) for i in range(2)]
    print(f'widths {name}: unet rel-L2 {r:.3e}, per image {r_img[0]:.3e} {r_img[1]:.3e}, temb {r_temb:.3e}, {g.stats()["launches"]} launches, '
          f'{count_forms(g)}')
    assert tuple(tg.out.shape) == tuple(ref_temb.shape) and r_temb <= TEMB_TOL, r_temb
    assert torch.isfinite(out).all()
    assert r <= UNET_TOL, r
    assert max(r_img) <= UNET_TOL, r_img
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True, static_unchanged=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.eps), 'hipGraph replay differs from eager execution'
    for graph in (g, tg):
        assert graph.tune_source()['shapes_tuned_in_process'] == 0, graph.tune_source()
    return g


def attn_details(g, label):
    return [d for (lab, _, _), d in zip(g.op_table(), g.op_details()) if lab == label]


# ------------------------------------------------------------------------------------------------ UNet + TEMB
def test_w64_no_level_folds(w64):
    g = run_unet_case('w64', w64, width_config(64, 64, 128, 32), 64, seed=101)
    f = count_forms(g)
    # 16 transformers, heads 1 / 2 / 4 / 4: 16 self-attention and 16 cross-attention launches, no fold; the one-launch conv_in
    assert f['xattn_fold'] == 0 and f['attn'] == {'attn_d64': 32}, f
    assert (f['conv_in'], f['latent_im2col'], f['latent_prep'], f['im2col_wrap']) == (1, 0, 0, 0) and f['layer_norm'] == 0, f
    assert sum('h4 lq64 lk77' in d for d in attn_details(g, 'attn_d64')) == 5           # level 2's cross-attention: the old gate's fold


def test_w128_no_level_folds(w128):
    g = run_unet_case('w128', w128, width_config(128, 64, 128, 32), 64, seed=102)
    f = count_forms(g)
    assert f['xattn_fold'] == 0 and f['attn'] == {'attn_d64': 32}, f
    assert (f['conv_in'], f['latent_im2col'], f['latent_prep'], f['im2col_wrap']) == (1, 0, 0, 0), f
    assert sum('h4 lq256 lk77' in d for d in attn_details(g, 'attn_d64')) == 5 and sum('h8 lq64 lk77' in d for d in attn_details(g, 'attn_d64')) == 5


@pytest.mark.parametrize('wrap', [0, 3])
def test_w192_im2col_input_convolution(w192, wrap):
    g = run_unet_case(f'w192 wrap{wrap}', w192, width_config(192, 64, 768, 16), 64, seed=103, wrap=wrap, tiling='xy' if wrap else None)
    f = count_forms(g)
    assert f['xattn_fold'] == 0 and f['attn'] == {'attn_d64': 32} and f['conv_in'] == 0, f          # heads 3 / 6 / 12: 12 * 64 is no multiple of 80
    assert (f['latent_im2col'], f['latent_prep'], f['im2col_wrap']) == ((0, 1, 1) if wrap else (1, 0, 0)), f


def test_w320_head_dim_40(w320):
    g = run_unet_case('w320_d40', w320, width_config(320, 40, 768, 32), 40, seed=104)
    f = count_forms(g)
    # levels 0 .. 2 fold (15 transformers, heads 8 / 16 / 32); the middle block at L = 16 is the plain cross-attention with 32 heads
    assert f['xattn_fold'] == 15 and f['attn'] == {'attn_d40': 17} and f['conv_in'] == 1, f
    assert sum('h32 lq16 lk77' in d for d in attn_details(g, 'attn_d40')) == 1
    assert sum('lk77' in d.split() for d in attn_details(g, 'attn_d40')) == 1                      # ... and no other on the text keys


def test_w320_head_dim_80(w320):
    g = run_unet_case('w320_d80', w320, width_config(320, 80, 768, 32), 80, seed=105)
    f = count_forms(g)
    assert f['xattn_fold'] == 15 and f['attn'] == {'attn_d80': 17} and f['conv_in'] == 1, f
    assert [d for d in attn_details(g, 'attn_d80') if 'lk77' in d.split()] == ['B2 h16 lq16 lk77']    # the middle block, L = 16


def test_w320_head_dim_160(w320):
    g = run_unet_case('w320_d160', w320, width_config(320, 160, 768, 32), 160, seed=106)
    f = count_forms(g)
    # level 0 has 2 heads (160 columns: no 64-deep K slabs): 5 plain cross-attentions at L = 1024; levels 1 and 2 fold; the middle is plain
    assert f['xattn_fold'] == 10 and f['attn'] == {'attn_d160': 16 + 5 + 1} and f['conv_in'] == 1, f
    assert sum('h2 lq1024 lk77' in d for d in attn_details(g, 'attn_d160')) == 5
    assert sorted(set(d for d in attn_details(g, 'attn_d160') if 'lk77' in d.split())) == ['B2 h2 lq1024 lk77', 'B2 h8 lq16 lk77']


def test_w64_uint8_weights(w64):
    from sdod.amd import engine as E
    wq = Width(64, 128, seed=6400, quant=True)
    g = run_unet_case('w64_u8', wq, width_config(64, 64, 128, 16, weight_quant=1), 64, seed=107)
    f = count_forms(g)
    assert f['xattn_fold'] == 0 and f['attn'] == {'attn_d64': 32} and f['layer_norm'] == 48, f          # three LayerNorm launches per transformer
    plain = E.UNet(width_config(64, 64, 128, 16), 2)
    plain.load_state_dict(w64.load)
    plain.finalize()
    # ... and on top of them the skip convolutions' own GEMMs (14 ResBlocks change width) and ff.net.2 / proj_out uncomposed (16)
    print('widths w64_u8: launches', g.stats()['launches'], 'fp16 graph', plain.stats()['launches'])
    assert count_forms(plain)['layer_norm'] == 0 and g.stats()['launches'] > plain.stats()['launches'] + 48


def test_w64_linear_projections():
    wl = Width(64, 128, seed=6410, linear=True)
    g = run_unet_case('w64_lin', wl, width_config(64, 64, 128, 16, linear_proj=1), 64, seed=108)
    f = count_forms(g)
    assert f['xattn_fold'] == 0 and f['attn'] == {'attn_d64': 32} and f['conv_in'] == 1, f
    assert dict(g.param_table())['input_blocks.1.1.proj_in.weight'] == (64, 64)


# ------------------------------------------------------------------------------------------------ regions and image prompts at w64
def _w64_inputs(k, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(2, 4, 32, 32, generator=gen), (torch.randn(2, 77 * k, 128, generator=gen) * 0.5).half(), torch.tensor([999.0, 501.0])


def _w64_temb(w64, t):
    from sdod.amd import engine as E
    tg = E.Temb(width_config(64, 64, 128, 32), 2)
    tg.load_state_dict(w64.load)
    tg.finalize()
    tg.t.copy_(t); tg.execute()
    return tg


def _eager_then_replay(g):
    g.execute()
    torch.cuda.synchronize()
    g.check()
    eager = g.eps.clone()
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True, static_unchanged=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.eps), 'hipGraph replay differs from eager execution'
    assert g.tune_source()['shapes_tuned_in_process'] == 0, g.tune_source()
    return eager.float().cpu().permute(0, 3, 1, 2)


def test_w64_regional_prompts_take_the_per_region_form(w64):
    """two regional prompts at w64 32x32: level 2 (4 heads of 64 on 64 pixels) passed the old gate; the shared predicate declines it,
    so every block is one attention launch per (image, region) and a blend"""
    import regions_ref as RR
    from sdod.amd import engine as E
    k = 2
    x, ctx, t = _w64_inputs(k, seed=109)
    ws = RR.region_weights(RR.soft_masks((32, 32), k, seed=3))
    tg = _w64_temb(w64, t)
    g = E.UNet(width_config(64, 64, 128, 32, context_len=77 * k, regions=k), 2)
    g.load_state_dict(w64.load)
    g.finalize()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    for slot, w in zip(g.region_w, ws):
        slot.copy_(w)
    out = _eager_then_replay(g)
    ref = RR.regional_unet(w64.oracle(64), ws)(x, t, ctx.float())
    plain = RR.regional_unet(w64.oracle(64), RR.background_weights(k, (32, 32)))(x, t, ctx.float())
    r, r_img, away = rel_l2(out, ref), [rel_l2(out[i], ref[i]) for i in range(2)], rel_l2(out, plain)
    labels = labels_of(g)
    print(f'widths w64 regions: rel-L2 {r:.3e}, per image {r_img[0]:.3e} {r_img[1]:.3e}, against region 0 everywhere {away:.3e}')
    assert torch.isfinite(out).all() and r <= UNET_TOL and max(r_img) <= UNET_TOL, (r, r_img)
    assert away > UNET_TOL                                                 # (the masks matter)
    assert labels.count('region_blend') == 16 and sum(lab.startswith('attn_d') for lab in labels) == 16 + 16 * 2 * k


def test_w64_image_prompt_takes_the_per_segment_form(w64):
    import ipadapter_ref as IR
    from sdod.amd import engine as E
    T = 4
    x, ctx, t = _w64_inputs(1, seed=110)
    tok = torch.randn(2, T, 128, generator=torch.Generator().manual_seed(111)).half()
    cfg = width_config(64, 64, 128, 32, ip_tokens=T)
    ip_sd = IR.synthetic_ip_state_dict(E.UNet(cfg, 2).param_table(), seed=4321, spread=4.0, ctx_dim=128)
    ws = IR.ip_weights(0.5, (32, 32), IR.soft_mask((32, 32), 5))
    tg = _w64_temb(w64, t)
    g = E.UNet(cfg, 2)
    g.load_state_dict({**w64.load, **ip_sd})
    g.finalize()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx); g.ip_ctx.copy_(tok)
    for slot, w in zip(g.ip_w, ws):
        slot.copy_(w)
    out = _eager_then_replay(g)
    ref = IR.ip_unet(w64.oracle(64), ip_sd, tok.float(), ws)(x, t, ctx.float())
    off = IR.ip_unet(w64.oracle(64), ip_sd, tok.float(), IR.ip_weights(0.0, (32, 32)))(x, t, ctx.float())
    r, r_img, away = rel_l2(out, ref), [rel_l2(out[i], ref[i]) for i in range(2)], rel_l2(out, off)
    labels = labels_of(g)
    print(f'widths w64 image prompt: rel-L2 {r:.3e}, per image {r_img[0]:.3e} {r_img[1]:.3e}, against no image prompt {away:.3e}')
    assert torch.isfinite(out).all() and r <= UNET_TOL and max(r_img) <= UNET_TOL, (r, r_img)
    assert away > UNET_TOL                                                 # (the image tokens matter)
    assert labels.count('region_blend') == 16 and sum(lab.startswith('attn_d') for lab in labels) == 16 + 16 * 2 * 2


# ------------------------------------------------------------------------------------------------ VAE halves
@pytest.mark.parametrize('ch', [64, 256])
def test_vae_decoder_width(ch):
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(8, 8)
    cfg.vae_channels = ch
    g = E.VaeDecoder(cfg, 1)
    sd = Wt.synthetic_state_dict(g.param_table(), seed=1235 + ch)
    with torch.device('meta'):
        ref_model = S.AutoencoderKLDecode(ch=ch)
    ref_model.load_state_dict(sd, assign=True)       # (strict: the table is the oracle's state dict of that width)
    g.load_state_dict(sd)
    g.finalize()
    z = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(12)) * 0.18215 * 4
    with torch.no_grad():
        ref = ref_model.eval()(z)
    g.z.copy_(z)
    g.execute()
    torch.cuda.synchronize()
    g.check()
    eager = g.img.clone()
    out = eager.float().cpu().permute(0, 3, 1, 2)
    r = rel_l2(out, ref)
    print(f'widths vae decoder ch{ch}: rel-L2 {r:.3e}, {g.stats()["launches"]} launches')
    assert torch.isfinite(out).all() and r <= VAE_TOL, r
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(eager, g.img) and g.tune_source()['shapes_tuned_in_process'] == 0


@pytest.mark.parametrize('ch', [64, 256])
def test_vae_encoder_width(ch):
    from test_img2img_cpu import LdmEncoder
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(8, 8)
    cfg.vae_channels = ch
    g = E.VaeEncoder(cfg, 1)
    sd = Wt.synthetic_state_dict(g.param_table(), seed=1238 + ch)
    with torch.device('meta'):
        ref_model = LdmEncoder(ch=ch)
    ref_model.load_state_dict(sd, assign=True)
    g.load_state_dict(sd)
    g.finalize()
    gen = torch.Generator().manual_seed(8)
    yy, xx = torch.meshgrid(torch.arange(64.), torch.arange(64.), indexing='ij')
    smooth = torch.stack([128 + 100 * torch.sin(xx / 5 + k) * torch.cos(yy / 7 - k) for k in range(3)], -1)
    u8 = (smooth[None] + 20 * torch.randn(1, 64, 64, 3, generator=gen)).clamp(0, 255).to(torch.uint8)
    with torch.no_grad():
        ref = ref_model.eval()((2.0 * (u8.float() / 255.0) - 1.0).permute(0, 3, 1, 2))
    g.img.copy_(u8)
    g.execute()
    torch.cuda.synchronize()
    g.check()
    out = g.moments.cpu().clone()
    r, r_mean, r_logvar = rel_l2(out, ref), rel_l2(out[:, :4], ref[:, :4]), rel_l2(out[:, 4:], ref[:, 4:])
    print(f'widths vae encoder ch{ch}: rel-L2 {r:.3e} (mean {r_mean:.3e}, logvar {r_logvar:.3e}), {g.stats()["launches"]} launches')
    assert torch.isfinite(out).all() and r <= VAE_TOL and r_mean <= VAE_TOL and r_logvar <= VAE_TOL, (r, r_mean, r_logvar)
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.moments.cpu(), out) and g.tune_source()['shapes_tuned_in_process'] == 0


# ------------------------------------------------------------------------------------------------ text tower
@pytest.mark.parametrize('arch', [0, 1])
def test_text_encoder_width_128(arch):
    from oracle import sd_torch as S
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    cfg.context_dim, cfg.text_heads, cfg.text_layers, cfg.vocab_size, cfg.text_arch = 128, 2, 2, 1000, arch
    g = E.TextEncoder(cfg, 2)
    sd = Wt.synthetic_state_dict(g.param_table(), seed=1236 + arch)
    with torch.device('meta'):
        ref_model = S.OpenClipTextModel(vocab=1000, d=128, layers=2, heads=2, run_layers=2) if arch else \
            S.ClipTextModel(vocab=1000, d=128, layers=2, heads=2, inter=512)
    ref_model.load_state_dict(sd, assign=True)
    g.load_state_dict(sd)
    g.finalize()
    ids = torch.randint(0, 1000, (2, 77), generator=torch.Generator().manual_seed(5))
    ids[0, 10:] = 999
    g.ids.copy_(ids.int())
    g.execute()
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = ref_model.eval()(ids)
    first = g.out.clone()
    r = rel_l2(first.float().cpu(), ref)
    r_img = [rel_l2(first[i].float().cpu(), ref[i]) for i in range(2)]
    print(f'widths text tower d128 arch{arch}: rel-L2 {r:.3e}, per prompt {r_img[0]:.3e} {r_img[1]:.3e}')
    assert tuple(first.shape) == (2, 77, 128) and torch.isfinite(first).all() and r <= TEXT_TOL and max(r_img) <= TEXT_TOL, (r, r_img)
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(first, g.out) and g.tune_source()['shapes_tuned_in_process'] == 0
