"""FreeU on the GPU: sdod_freeu_f16 against the fp64 restatement (tests/freeu_ref.py) on the same fp16 inputs, the UNet graph with
the switch against the fp32 restatement on the oracle UNet, alone and behind control inputs, the switch on every other kind of UNET
graph against the unswitched graph of the same configuration, and the pipeline (set_freeu / clear_freeu; eager, captured and
pipelined generation, img2img, inpainting, a panorama canvas, a rectangle with a hires pass).

Stated tolerances.  Kernel, skip filter: |out - ref| <= ulp_fp16(ref) + 2^-12 max|v| of the plane -- the final rounding, and the fp32
sums (up to 1536 terms x 2^-24 x max|v| x 4 coefficients x |s - 1| <= 1, about 1e-4 max|v|).  Backbone: version 1 bit for bit against
half(float(h) * b); version 2 within ulp_fp16(ref) + 2^-12 |h| (the fp32 mean over <= 1280 channels and one division).  Graph against
the fp32 restatement: rel-L2 <= 1e-2, the project's own; a 20-step PLMS chain's final latent <= 2e-2.  Where a test relies on FreeU
mattering, the restatement is first shown, on the CPU, to move by more than 5e-2 and the GPU result must lie farther than 1e-2 from
the plain one.  Everything else is bit-exact."""
import ctypes

import pytest
import torch

import controlnet_ref as CR
import freeu_ref as FR

pytestmark = pytest.mark.gpu

# launch count and activation-arena bytes of the batch-2 16x16 UNet graph without any switch, as tests/test_adapter_gpu.py and
# tests/test_controlnet_gpu.py record them from before their features
PARENT_LAUNCHES = 321
PARENT_ARENA_BYTES = 4260096

SHAPES = [(1, 1, 128), (1, 2, 128), (2, 2, 256), (8, 8, 1280), (12, 8, 256), (16, 24, 128), (32, 32, 640)]
N = 2
GUARD = 64
GUARD_VALUE = -77.0


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int16)


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ulp16(ref):
    """spacing of fp16 at |ref| (2^-24 below the normal range)"""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - 10)


def params(b1, s1, b2, s2, version):
    return torch.tensor([b1, s1, b2, s2, float(version), 0, 0, 0], dtype=torch.float32, device='cuda')


_cache = {}


def _inputs(shape):
    """fp16 NHWC h and skip [N, H, W, C] drawn like the ControlNet test's segments -- normal x 2^randint(-8, 9) -- plus a per-channel
    offset so that DC is not negligible; made once per shape and never written"""
    if shape not in _cache:
        H, W, C = shape
        g = torch.Generator().manual_seed(1000 * H + 10 * W + C)
        mk = lambda: ((torch.randn(N, H, W, C, generator=g) * torch.exp2(torch.randint(-8, 9, (N, H, W, C), generator=g).float())
                       + 4.0 * torch.randn(1, 1, 1, C, generator=g)).half())
        _cache[shape] = (mk(), mk())
    return _cache[shape]


def _guarded(t):
    """a device copy of t inside a buffer with guard regions before and behind it: (buffer, view)"""
    buf = torch.full((t.numel() + 2 * GUARD,), GUARD_VALUE, dtype=torch.float16, device='cuda')
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == GUARD_VALUE).all()) and bool((buf[-GUARD:] == GUARD_VALUE).all())


def _run(shape, prm, stage):
    from sdod.amd import ops
    h, skip = _inputs(shape)
    hb, hd = _guarded(h)
    sb, sd = _guarded(skip)
    scratch = torch.full((N * shape[0] * shape[1] + 2 * GUARD,), GUARD_VALUE, dtype=torch.float32, device='cuda')
    ops.freeu(hd, sd, prm, stage, scratch[GUARD:GUARD + N * shape[0] * shape[1]])
    torch.cuda.synchronize()
    assert _guards_intact(hb) and _guards_intact(sb) and _guards_intact(scratch)
    return hd.cpu(), sd.cpu()


# ------------------------------------------------------------------ sdod_freeu_f16
@pytest.mark.parametrize('shape', SHAPES)
def test_skip_filter_against_fp64(shape):
    """b = 1: h keeps its bits; every s, both stages' slots; guards intact; a second run on fresh copies gives the same bits"""
    h, skip = _inputs(shape)
    v = skip.double().permute(0, 3, 1, 2)
    vmax = v.abs().amax((-2, -1), keepdim=True)
    worst = 0.0
    for k, s in enumerate((0.0, 0.2, 0.9, 2.0)):
        stage = 1 + k % 2
        prm = params(1.0, s, 7.0, 3.0, 2) if stage == 1 else params(7.0, 3.0, 1.0, s, 1)      # the other stage's values must not be read
        hd, sd = _run(shape, prm, stage)
        assert torch.equal(bits(hd), bits(h))
        ref = FR.fourier_filter(v, s)
        err = (sd.double().permute(0, 3, 1, 2) - ref).abs()
        bound = ulp16(ref) + 2.0 ** -12 * vmax
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (shape, s, float((err / bound).max()))
        hd2, sd2 = _run(shape, prm, stage)
        assert torch.equal(bits(sd2), bits(sd)) and torch.equal(bits(hd2), bits(hd))
        if s != 1.0 and shape[0] * shape[1] > 1:
            assert not torch.equal(bits(sd), bits(skip))
    print(f'skip filter {shape}: worst error / bound {worst:.3f}')


@pytest.mark.parametrize('shape', SHAPES)
def test_backbone_against_its_definitions(shape):
    """s = 1: skip keeps its bits.  Version 1 bit for bit; version 2 against fp64; channels [C/2, C) keep their bits"""
    h, skip = _inputs(shape)
    C = shape[2]
    for b in (0.0, 1.3, 2.0):
        hd, sd = _run(shape, params(b, 1.0, 9.0, 9.0, 1), 1)
        assert torch.equal(bits(sd), bits(skip))
        want = h.clone()
        want[..., :C // 2] = (h[..., :C // 2].float() * torch.tensor(b, dtype=torch.float32)).half()
        assert torch.equal(bits(hd), bits(want)), (shape, b)
    worst = 0.0
    for b in (0.0, 1.4, 2.0):
        hd, sd = _run(shape, params(9.0, 9.0, b, 1.0, 2), 2)
        assert torch.equal(bits(sd), bits(skip))
        assert torch.equal(bits(hd[..., C // 2:]), bits(h[..., C // 2:]))
        h64 = h.double().permute(0, 3, 1, 2)
        ref = h64[:, :C // 2] * FR.backbone_factor(h64, b, 2)
        err = (hd.double().permute(0, 3, 1, 2)[:, :C // 2] - ref).abs()
        bound = ulp16(ref) + 2.0 ** -12 * h64[:, :C // 2].abs()
        worst = max(worst, float((err / bound).max()))
        assert torch.isfinite(hd).all() and bool((err <= bound).all()), (shape, b, float((err / bound).max()))
        hd2, _ = _run(shape, params(9.0, 9.0, b, 1.0, 2), 2)
        assert torch.equal(bits(hd2), bits(hd))
        if shape[0] * shape[1] == 1:                      # max == min: factor 1, not the published 0 / 0
            assert torch.equal(bits(hd), bits(h))
    print(f'backbone v2 {shape}: worst error / bound {worst:.3f}')


def test_constant_mean_gives_factor_one_and_no_nan():
    """every pixel holds the same channel vector: max m == min m bit for bit, the published code's NaN case"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(3)
    vec = (torch.randn(256, generator=g) * 8).half()
    h = vec.view(1, 1, 1, 256).expand(N, 4, 6, 256).contiguous()
    hb, hd = _guarded(h)
    sb, sd = _guarded(h)
    ops.freeu(hd, sd, params(1.6, 1.0, 1.0, 1.0, 2), 1)
    torch.cuda.synchronize()
    assert torch.equal(bits(hd.cpu()), bits(h)) and torch.equal(bits(sd.cpu()), bits(h)) and _guards_intact(hb) and _guards_intact(sb)
    assert torch.isnan(FR.backbone_factor_published(h.double().permute(0, 3, 1, 2), 1.6)).all()


def test_identity_keeps_every_bit_even_of_nan():
    from sdod.amd import ops
    h, skip = (t.clone() for t in _inputs((8, 8, 1280)))
    h[0, 1, 2, 5] = float('nan'); skip[1, 3, 4, 700] = float('nan'); skip[0, 0, 0, 0] = float('inf')
    for version in (1, 2):
        for stage, prm in ((1, params(1.0, 1.0, 3.0, 0.0, version)), (2, params(3.0, 0.0, 1.0, 1.0, version))):
            hb, hd = _guarded(h)
            sb, sd = _guarded(skip)
            ops.freeu(hd, sd, prm, stage)
            torch.cuda.synchronize()
            assert torch.equal(bits(hd.cpu()), bits(h)) and torch.equal(bits(sd.cpu()), bits(skip))


def test_a_captured_launch_reads_its_parameters_on_the_device():
    from sdod.amd import ops
    shape = (12, 8, 256)
    h, skip = _inputs(shape)
    hd, sd = h.cuda(), skip.cuda()
    scratch = torch.empty(N * 96, dtype=torch.float32, device='cuda')
    prm = params(1.0, 1.0, 1.0, 1.0, 2)
    ops.freeu(hd, sd, prm, 1, scratch)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.freeu(hd, sd, prm, 1, scratch)
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(bits(hd.cpu()), bits(h)) and torch.equal(bits(sd.cpu()), bits(skip))          # the identity
    prm.copy_(params(1.5, 0.2, 1.0, 1.0, 2))
    g.replay(); torch.cuda.synchronize()
    want_h, want_s = _run(shape, params(1.5, 0.2, 1.0, 1.0, 2), 1)
    assert torch.equal(bits(hd.cpu()), bits(want_h)) and torch.equal(bits(sd.cpu()), bits(want_s))
    assert not torch.equal(bits(want_h), bits(h)) and not torch.equal(bits(want_s), bits(skip))


def test_bad_arguments_are_refused_and_leave_the_tensors_untouched():
    from sdod.amd import _lib
    lib = _lib.hip()
    n, H, W, C = 2, 4, 4, 128
    h = torch.full((n * H * W * C + 16,), 7.0, dtype=torch.float16, device='cuda')
    s = torch.full((n * H * W * C + 16,), 5.0, dtype=torch.float16, device='cuda')
    prm = params(2.0, 0.0, 2.0, 0.0, 1)
    sc = torch.zeros(n * H * W + 4, dtype=torch.float32, device='cuda')
    good = (P(h), P(s), n, H, W, C, P(prm), 1, P(sc), 3, None)

    def with_(**kw):
        names = ('h', 'skip', 'n', 'H', 'W', 'C', 'params', 'stage', 'scratch', 'phases', 'stream')
        a = dict(zip(names, good))
        a.update(kw)
        return tuple(a[k] for k in names)
    bad = [with_(C=64), with_(C=192), with_(C=0), with_(h=None), with_(skip=None), with_(params=None), with_(scratch=None),
           with_(h=P(h[4:])), with_(skip=P(s[4:])), with_(H=0), with_(W=0), with_(n=0), with_(stage=0), with_(stage=3), with_(phases=0),
           with_(phases=4), with_(H=1025), with_(params=ctypes.c_void_p(prm.data_ptr() + 2))]
    for args in bad:
        assert lib.sdod_freeu_f16(*args) != 0 and lib.sdod_hip_last_error()
    torch.cuda.synchronize()
    assert bool((h == 7.0).all()) and bool((s == 5.0).all())
    assert lib.sdod_freeu_f16(*good) == 0                                   # the good call writes its range only
    torch.cuda.synchronize()
    numel = n * H * W * C
    assert bool((h[numel:] == 7.0).all()) and bool((s[numel:] == 5.0).all())
    hv = h[:numel].view(n, H, W, C)
    assert bool((hv[..., :C // 2] == 14.0).all()) and bool((hv[..., C // 2:] == 7.0).all())
    assert bool((s[:numel] == 0.0).all())                                  # a constant plane is all DC: s = 0 removes it


# ------------------------------------------------------------------ graphs
SIZES = [(16, 16), (8, 16)]          # the square the other feature tests use, and a rectangle whose deepest level is 1 x 2
STRONG = (2.0, 2.0, 0.0, 0.0)        # (b1, b2, s1, s2): the presets are gentle on random weights, these move the output


@pytest.fixture(scope='module')
def weights():
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    return {'unet': Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234),
            'temb': Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235),
            'vae': Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1236),
            'vae_enc': Wt.synthetic_state_dict(E.VaeEncoder(cfg, 1).param_table(), seed=1238)}


@pytest.fixture(scope='module')
def oracle(weights):
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**weights['unet'], **weights['temb']}, assign=True)
    return unet.eval()


def _graphs(weights, hw, **extra):
    """(time embedding, plain UNet, UNet with the switch) at one size on the same weights"""
    from sdod.amd import engine as E
    cfg = E.sd14_config(*hw)
    for k, v in extra.items():
        setattr(cfg, k, v)
    tg = E.Temb(E.sd14_config(*hw), 2); tg.load_state_dict(weights['temb']); tg.finalize()
    g0 = E.UNet(cfg, 2); g0.load_state_dict(weights['unet']); g0.finalize()
    c1 = E.copy_config(cfg); c1.freeu = 1
    g1 = E.UNet(c1, 2); g1.load_state_dict(weights['unet']); g1.finalize()
    return tg, g0, g1


def _inputs_for(hw, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(2, 4, *hw, generator=gen), torch.randn(2, 77, 768, generator=gen).half(), torch.tensor([999.0, 501.0])


def _eval(tg, g, x, ctx, t):
    tg.t.copy_(t); tg.execute()
    g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx)
    g.execute()
    torch.cuda.synchronize()
    eager = g.eps.clone()
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(g.eps, eager)
    return nchw(eager)


def _set(g, b1, b2, s1, s2, version):
    from sdod.amd import freeu as FU
    g.freeu.copy_(torch.tensor(FU.freeu_check_args(b1, b2, s1, s2, version), dtype=torch.float32))


@pytest.fixture(scope='module')
def square(weights):
    tg, g0, g1 = _graphs(weights, (16, 16))
    return dict(tg=tg, g0=g0, g1=g1)


def test_a_graph_without_the_switch_is_the_parent_graph(weights, square):
    """same launch list, arena and inputs as the graph sdod_graph_create has always made; the switch adds twelve launches, one input"""
    from sdod.amd import engine as E, freeu as FU
    g0, g1 = square['g0'], square['g1']
    raw = E.Graph(E.UNET, E.sd14_config(16, 16), 2)                          # sdod_graph_create, the entry point of every build before this one
    assert raw.param_table() == g0.param_table() == g1.param_table()
    raw.load_state_dict(weights['unet']); raw.finalize()
    assert raw.op_table() == g0.op_table() and raw.op_details() == g0.op_details() and raw.stats() == g0.stats()
    s0, s1 = g0.stats(), g1.stats()
    print(f'UNet b2 16x16: {s0["launches"]} launches, arena {s0["arena_bytes"]} B; with FreeU {s1["launches"]}, {s1["arena_bytes"]} B')
    assert (s0['launches'], s0['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES)
    assert g0.freeu_input() == -1 and not hasattr(g0, 'freeu')
    with pytest.raises(Exception):
        g0._io(False, 3)
    l0, l1 = [l for l, _, _ in g0.op_table()], [l for l, _, _ in g1.op_table()]
    assert not [l for l in l0 if l.startswith('freeu')]
    assert l1.count('freeu_filter') == 6 and l1.count('freeu_scale') == 6 and s1['weight_bytes'] == s0['weight_bytes']
    details = [d for (l, _, _), d in zip(g1.op_table(), g1.op_details()) if l == 'freeu_filter']
    assert details == ['n2 hw4 c1280 stage1'] * 3 + ['n2 hw16 c1280 stage1'] * 2 + ['n2 hw64 c640 stage2']
    assert all(b > 0 for l, _, b in g1.op_table() if l.startswith('freeu'))
    assert g1.freeu_input() == 3 and g1.freeu.tolist() == list(FU.IDENTITY)
    assert g1.tune_source()['shapes_tuned_in_process'] == 0
    with pytest.raises(Exception, match='before finalize'):
        g1.enable_freeu()


def test_identity_graph_has_the_plain_graphs_bits(square):
    r = square
    x, ctx, t = _inputs_for((16, 16))
    out0 = _eval(r['tg'], r['g0'], x, ctx, t)
    assert torch.equal(_eval(r['tg'], r['g1'], x, ctx, t), out0)
    _set(r['g1'], 1.0, 1.0, 1.0, 1.0, 1)                                     # version 1 at b = s = 1: the identity too
    assert torch.equal(_eval(r['tg'], r['g1'], x, ctx, t), out0)
    r['g1'].freeu.copy_(torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0, 0, 0, 0]))
    r['out0'] = out0


@pytest.mark.parametrize('hw', SIZES)
def test_graph_matches_the_restatement(weights, oracle, square, hw):
    """versions 1 and 2 at STRONG against the fp32 restatement; the fp16-site sensitivity of the restatement itself is printed next to
    each figure (the same fp32 model with the two tensors of every site rounded to fp16)"""
    x, ctx, t = _inputs_for(hw)
    with torch.no_grad():
        ref0 = oracle(x, t, ctx.float())
        refs = {v: FR.freeu_unet(oracle, x, t, ctx.float(), *STRONG, v) for v in (1, 2)}
        sens = {v: rel_l2(FR.freeu_unet(oracle, x, t, ctx.float(), *STRONG, v, round_sites=True), refs[v]) for v in (1, 2)}
    moved = {v: rel_l2(refs[v], ref0) for v in (1, 2)}
    assert min(moved.values()) > 5e-2, moved                                 # on the CPU, before any GPU work
    tg, g0, g1 = (square['tg'], square['g0'], square['g1']) if hw == (16, 16) else _graphs(weights, hw)
    plain = _eval(tg, g0, x, ctx, t)
    assert rel_l2(plain, ref0) <= 1e-2
    for v in (1, 2):
        _set(g1, *STRONG, v)
        out = _eval(tg, g1, x, ctx, t)
        rl, away = rel_l2(out, refs[v]), rel_l2(out, plain)
        print(f'FreeU graph {hw} v{v}: rel-L2 vs fp32 restatement {rl:.3e}, vs the plain output {away:.3e} '
              f'(oracle moved {moved[v]:.3e}, fp16-site sensitivity {sens[v]:.3e})')
        assert torch.isfinite(out).all() and rl <= 1e-2 and away > 1e-2, (v, rl, away)
    g1.freeu.copy_(torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0, 0, 0, 0]))
    assert torch.equal(_eval(tg, g1, x, ctx, t), plain)


def test_freeu_acts_behind_the_control_additions(weights, oracle):
    """a graph with control inputs AND the switch against cldm's ControlledUnetModel with FreeU applied to the tensors the decoder
    pops, i.e. after the additions (ComfyUI's order)"""
    from sdod.amd import engine as E
    tg, g0, g1 = _graphs(weights, (16, 16), control_inputs=1)
    labels = [l for l, _, _ in g1.op_table()]
    assert labels.count('add_control') == 1 and labels.index('add_control') < labels.index('freeu_filter')
    assert g1.freeu_input() == 3 + 14 and g0.freeu_input() == -1
    x, ctx, t = _inputs_for((16, 16))
    gen = torch.Generator().manual_seed(11)
    res = [(4.0 * torch.randn(b, c, h, w, generator=gen)).half() for b, h, w, c in E.control_residual_shapes(g1.cfg, 2)]
    scales = [0.5 + 0.1 * k for k in range(13)]
    with torch.no_grad():
        ctl = CR.controlled_unet(oracle, x, t, ctx.float(), [c.float() for c in res], scales)
        ref = FR.freeu_unet(oracle, x, t, ctx.float(), *STRONG, 2, control=([c.float() for c in res], scales))
    moved = rel_l2(ref, ctl)
    assert moved > 5e-2, moved
    for g in (g0, g1):
        for slot, r in zip(g.control_res, res):
            slot.copy_(r.permute(0, 2, 3, 1))
        g.control_scale.copy_(torch.tensor(scales))
    base = _eval(tg, g0, x, ctx, t)
    assert torch.equal(_eval(tg, g1, x, ctx, t), base) and rel_l2(base, ctl) <= 1e-2          # identity: the controlled graph's bits
    _set(g1, *STRONG, 2)
    out = _eval(tg, g1, x, ctx, t)
    rl, away = rel_l2(out, ref), rel_l2(out, base)
    print(f'FreeU behind control inputs: rel-L2 vs restatement {rl:.3e}, vs the controlled output {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(out).all() and rl <= 1e-2 and away > 1e-2, (rl, away)


def _variant(name):
    """(config, quantised weights?) of every other way a UNET graph is created or sized: the switch must compose with each"""
    from sdod.amd import engine as E
    cfg = E.sd21_config(16, 16) if name == 'sd21' else E.sd14_config(16, 16, concat_channels=5 if name == 'concat_channels' else 0)
    if name == 'adapter_inputs':
        cfg.adapter_reps = 2
    elif name == 'wrap':
        cfg.tiling = 3
    elif name == 'regions':
        cfg.regions, cfg.context_len = 2, 154
    elif name == 'ip_tokens':
        cfg.ip_tokens = 4
    elif name == 'prompt_chunks':
        cfg.context_len = 154
    if name in ('model_channels_64', 'weight_quant'):    # a non-SD width (tests/test_engine_widths_gpu.py's w64): the sites come from the
        cfg.model_channels, cfg.num_heads, cfg.head_dim, cfg.context_dim = 64, 0, 64, 128      # channel rule, 256 | 256 and 128 | 128
        cfg.weight_quant = 1 if name == 'weight_quant' else 0                                   # ... and the same with uint8 weights
    return cfg, name == 'weight_quant'


@pytest.mark.parametrize('name', ['adapter_inputs', 'wrap', 'regions', 'ip_tokens', 'concat_channels', 'weight_quant', 'sd21', 'prompt_chunks',
                                  'model_channels_64'])
def test_the_switch_composes_with_every_other_unet_graph(name):
    """for each creation path and size rule: the identity has the unswitched graph's bits, STRONG moves the output and stays finite,
    eager equals the captured replay, and the parameter input sits behind every other input"""
    from sdod.amd import engine as E, weights as Wt
    cfg, quant = _variant(name)
    g0 = E.UNet(cfg, 2)
    sd = Wt.synthetic_state_dict(g0.param_table(), seed=1300)
    load = Wt.quantize_state_dict(sd) if quant else sd
    c1 = E.copy_config(cfg); c1.freeu = 1
    g1 = E.UNet(c1, 2)
    assert g1.param_table() == g0.param_table()
    for g in (g0, g1):
        g.load_state_dict(load); g.finalize()
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(tuple(g0.x.shape), generator=gen)
    temb = (0.5 * torch.randn(tuple(g0.temb.shape), generator=gen)).half()
    ctx = torch.randn(tuple(g0.ctx.shape), generator=gen).half()
    extra = {}
    if name == 'concat_channels':
        extra['cond'] = torch.randn(tuple(g0.cond.shape), generator=gen)
    if name == 'ip_tokens':
        extra['ip_ctx'] = torch.randn(tuple(g0.ip_ctx.shape), generator=gen).half()
    feats = [torch.randn(tuple(f.shape), generator=gen).half() for f in g0.adapter_feat] if name == 'adapter_inputs' else []

    def run(g):
        g.x.copy_(x); g.temb.copy_(temb); g.ctx.copy_(ctx)
        for k, v in extra.items():
            getattr(g, k).copy_(v)
        for slot, f in zip(getattr(g, 'adapter_feat', []), feats):
            slot.copy_(f)
        if name == 'ip_tokens':
            for w in g.ip_w:
                w[:, 1] = 0.5
        g.execute(); torch.cuda.synchronize()
        eager = g.eps.clone()
        g.execute(use_hip_graph=True); torch.cuda.synchronize()
        assert torch.equal(g.eps, eager)
        return eager
    n_inputs = g1.freeu_input()
    assert n_inputs >= 3 and g0.freeu_input() == -1
    with pytest.raises(Exception):
        g1._io(False, n_inputs + 1)                                           # nothing behind it
    labels = [l for l, _, _ in g1.op_table()]
    assert labels.count('freeu_filter') == 6 and labels.count('freeu_scale') == 6
    mc = cfg.model_channels
    assert [d.split()[2] for l, d in zip(labels, g1.op_details()) if l == 'freeu_filter'] == [f'c{4 * mc}'] * 5 + [f'c{2 * mc}']
    base = run(g0)
    assert torch.isfinite(base).all() and torch.equal(run(g1), base)
    _set(g1, *STRONG, 2)
    out = run(g1)
    away = rel_l2(out.float(), base.float())
    print(f'FreeU with {name}: STRONG v2 moves the output by {away:.3e}')
    assert torch.isfinite(out).all() and away > 1e-2
    _set(g1, 1.0, 1.0, 1.0, 1.0, 2)
    assert torch.equal(run(g1), base)


# ------------------------------------------------------------------ pipeline
CHAIN = (1.5, 1.6, 0.5, 0.2, 2)


@pytest.fixture(scope='module')
def rig(weights):
    from sdod.amd.pipeline import Txt2Img
    kw = dict(state_dicts=weights, images_per_gpu=1, latent_hw=16, with_text_encoder=False, with_vae_encoder=True)
    pipe, plain = Txt2Img(freeu=True, **kw), Txt2Img(**kw)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    return dict(pipe=pipe, plain=plain, ctx2=ctx2, x_T=x_T)


def test_pipeline_construction(rig):
    from sdod.amd import freeu as FU
    pipe, plain = rig['pipe'], rig['plain']
    assert pipe.freeu is True and pipe.unet.cfg.freeu == 1 and pipe.cfg.freeu == 0 and pipe.unet.freeu.tolist() == list(FU.IDENTITY)
    assert plain.freeu is False and not hasattr(plain.unet, 'freeu')
    assert (plain.unet.stats()['launches'], plain.unet.stats()['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES)
    for call in (lambda: plain.set_freeu(1.3, 1.4, 0.9, 0.2), plain.clear_freeu):
        with pytest.raises(RuntimeError, match='freeu=True'):
            call()
    for args in ((float('nan'), 1, 1, 1), (1, 11, 1, 1), (1, 1, 1, 1, 3)):
        with pytest.raises(ValueError):
            pipe.set_freeu(*args)
    assert pipe.unet.freeu.tolist() == list(FU.IDENTITY)
    pipe.set_freeu(1.3, 1.4, 0.9, 0.2)
    assert pipe.unet.freeu.tolist() == pytest.approx([1.3, 0.9, 1.4, 0.2, 2.0, 0, 0, 0])
    pipe.clear_freeu()
    assert pipe.unet.freeu.tolist() == list(FU.IDENTITY)


@pytest.mark.parametrize('sampler', ['plms', 'dpmpp_2m'])
def test_eager_and_captured_agree_and_new_values_need_no_capture(rig, sampler):
    from sdod.amd import freeu as FU
    pipe, plain, c, x_T = rig['pipe'], rig['plain'], rig['ctx2'].cuda(), rig['x_T']
    base = plain.generate(c, x_T, 4, 7.5, sampler)
    assert torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)         # as built: the plain pipeline bit for bit
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base)
    n_graphs = len(pipe._traj)
    pipe.set_freeu(*STRONG, 2)
    eager = pipe.generate(c, x_T, 4, 7.5, sampler)
    graphed = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert torch.equal(graphed, eager) and not torch.equal(eager, base) and len(pipe._traj) == n_graphs      # a replay of the same capture
    pipe.set_freeu(*FU.preset(1, 'sd14'), 1)
    graphed_b = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs and not torch.equal(graphed_b, graphed)
    assert torch.equal(graphed_b, pipe.generate(c, x_T, 4, 7.5, sampler))    # ... equals a fresh eager run with those values
    pipe.clear_freeu()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
    assert len(pipe._traj) == n_graphs


def test_latents_match_the_restatement_chain(rig, oracle):
    """20 PLMS steps at CHAIN against the sampler restatement (oracle/pipeline_oracle.py) on the fp32 UNet with FreeU"""
    from oracle import pipeline_oracle as PO
    pipe, x_T = rig['pipe'], rig['x_T']
    c16 = rig['ctx2'].float()
    model = FR.FreeUModel(oracle, *CHAIN)
    x2, t2 = x_T.repeat(2, 1, 1, 1), torch.tensor([981.0, 981.0])
    with torch.no_grad():
        moved = rel_l2(model(x2, t2, c16), oracle(x2, t2, c16))              # the restatement's first evaluation, with and without FreeU
    assert moved > 5e-2, moved                                               # on the CPU, before any GPU work
    z_ref = PO.plms_sample(model, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5)
    pipe.clear_freeu()
    z_plain = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
    pipe.set_freeu(*CHAIN)
    z = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5)
    pipe.clear_freeu()
    rl, away = rel_l2(z.cpu(), z_ref), rel_l2(z.cpu(), z_plain)
    print(f'FreeU plms final latent rel-L2 vs the restatement chain {rl:.3e}, vs the plain latent {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(z).all() and rl <= 2e-2 and away > 1e-2, (rl, away)


def test_rectangle_hires_and_loras_follow_the_switch(weights):
    """latent (8, 16) with a hires pass at (16, 16) on a pipeline that keeps its base weights: both UNets take the values, eager equals
    captured, cleared equals the same pipeline built without the flag"""
    from sdod.amd.pipeline import Txt2Img
    kw = dict(state_dicts=weights, images_per_gpu=1, latent_hw=(8, 16), with_text_encoder=False, hires_hw=(16, 16), loras=True)
    pipe, plain = Txt2Img(freeu=True, **kw), Txt2Img(**kw)
    assert pipe.hires.freeu is True and plain.hires.freeu is False
    g = torch.Generator().manual_seed(79)
    c = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, 8, 16, generator=g)
    run = lambda p, f: getattr(p, f)(c, x_T, 4, 7.5, 'dpmpp_2m', hires_steps=4)
    base = run(plain, 'generate_hires')
    assert torch.equal(run(pipe, 'generate_hires'), base)
    pipe.set_freeu(*STRONG, 2)
    assert pipe.hires.unet.freeu.tolist() == pipe.unet.freeu.tolist() == [2.0, 0.0, 2.0, 0.0, 2.0, 0, 0, 0]
    eager = run(pipe, 'generate_hires')
    assert not torch.equal(eager, base) and torch.equal(run(pipe, 'generate_hires_graphed'), eager)
    pipe.clear_freeu()
    assert torch.equal(run(pipe, 'generate_hires_graphed'), base)


def test_img2img_inpainting_and_the_pipelined_entry_point_follow_the_values(rig):
    pipe, plain, c, x_T = rig['pipe'], rig['plain'], rig['ctx2'].cuda(), rig['x_T']
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (1, 128, 128, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros(1, 128, 128, dtype=torch.uint8); mask[:, 32:96, 24:100] = 255

    def piped(p):
        img, ev = p.generate_pipelined(c, x_T, 4, 7.5, 'plms')
        ev.synchronize()                                                     # (the images are valid once the decode's event has completed)
        return img
    calls = {
        'img2img': (lambda p: p.img2img(c, u8, 0.5, 8, 7.5, seed=3), lambda p: p.img2img_graphed(c, u8, 0.5, 8, 7.5, seed=3)),
        'inpaint': (lambda p: p.inpaint(c, u8, mask, 0.5, 8, 7.5, seed=3), lambda p: p.inpaint_graphed(c, u8, mask, 0.5, 8, 7.5, seed=3)),
        'pipelined': (lambda p: p.generate(c, x_T, 4, 7.5, 'plms'), piped),
    }
    for name, (eager, other) in calls.items():
        pipe.clear_freeu()
        base = eager(plain).clone()
        assert torch.equal(eager(pipe), base) and torch.equal(other(pipe), base), name
        pipe.set_freeu(*STRONG, 2)
        out = eager(pipe).clone()
        assert not torch.equal(out, base) and torch.equal(other(pipe), out), name
    pipe.clear_freeu()


def test_panorama_windows_take_the_switch(weights):
    """a 16 x 24 canvas of two 16 x 16 windows in one evaluation: the version-2 statistics are per window"""
    from sdod.amd.pipeline import Txt2Img
    kw = dict(state_dicts=weights, images_per_gpu=2, latent_hw=16, with_text_encoder=False, canvas_hw=(16, 24))
    pipe, plain = Txt2Img(freeu=True, **kw), Txt2Img(**kw)
    g = torch.Generator().manual_seed(81)
    c = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, 16, 24, generator=g)
    args = dict(sampler='dpmpp_2m', steps=3, guidance=7.5, schedule='karras', stride=8)
    base = plain.generate_panorama(c, x_T, **args).clone()
    assert torch.equal(pipe.generate_panorama(c, x_T, **args), base)
    pipe.set_freeu(*STRONG, 2)
    out = pipe.generate_panorama(c, x_T, **args).clone()
    assert not torch.equal(out, base) and torch.equal(pipe.generate_panorama_graphed(c, x_T, **args), out)
    pipe.clear_freeu()
    assert torch.equal(pipe.generate_panorama_graphed(c, x_T, **args), base)
