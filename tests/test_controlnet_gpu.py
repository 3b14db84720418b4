"""ControlNet on the GPU: sdod_add_control_f16 bit for bit against its definition, the u / 255 input convolution on exact data, the
CONTROL_HINT and CONTROLNET graphs against the fp32 restatement (tests/controlnet_ref.py), the UNet's residual inputs against the
controlled oracle, and the pipeline (set_control_hint / clear_control_hint, eager and captured).

Stated tolerances, the project's own for the same kind of comparison: an fp16 graph against the fp32 restatement rel-L2 <= 1e-2; a
20-step PLMS chain's final latent <= 2e-2; everything else is bit-exact.  Where a test relies on the control signal mattering, the
fp32 restatement is first shown, on the CPU, to move by more than 5e-2, and the GPU result must lie farther than 1e-2 from the
uncontrolled one."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import controlnet_ref as CR

pytestmark = pytest.mark.gpu

# launch count and activation-arena bytes of the batch-2 16x16 UNet graph without control inputs, as tests/test_adapter_gpu.py records
# them from before either feature; and the arena of the same graph WITH control inputs (measured: the residual slots are inputs, not
# arena memory, and the one added launch allocates nothing)
PARENT_LAUNCHES = 321
PARENT_ARENA_BYTES = 4260096
CONTROL_ARENA_BYTES = 4260096

SIZES = [(16, 16), (8, 16)]          # the square the other feature tests use, and a rectangle whose deepest level is 1 x 2


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int16)


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ sdod_add_control_f16
COUNTS = [8, 40, 8192, 8200, 3 * 8192 + 24, 64]       # 8 elements .. more than three workgroups (8192 halves each), unequal
SCALES = [1.0, 0.37, -2.5, 0.0, 1.0 / 3.0, 0.0]
GUARD = 64


def _segments(seed=31):
    g = torch.Generator().manual_seed(seed)
    total = sum(c + GUARD for c in COUNTS)
    mk = lambda: (torch.randn(total, generator=g) * torch.exp2(torch.randint(-8, 9, (total,), generator=g).float())).half()
    h, r = mk(), mk()
    offs, o = [], 0
    for c in COUNTS:
        offs.append(o)
        o += c + GUARD
    return h, r, offs


def test_add_control_is_the_two_fp32_operations():
    """h = half(float(h) + s * float(r)) with the product and the sum rounded separately; guards between and behind the segments and
    every r unchanged; a zero-scale segment is not even read (its r is NaN) and keeps its bits"""
    from sdod.amd import ops
    h, r, offs = _segments()
    for k, (o, c) in enumerate(zip(offs, COUNTS)):
        if SCALES[k] == 0.0:
            r[o:o + c] = float('nan')
    hd, rd = h.cuda(), r.cuda()
    sd = torch.tensor(SCALES, dtype=torch.float32, device='cuda')
    ops.add_control([hd[o:o + c] for o, c in zip(offs, COUNTS)], [rd[o:o + c] for o, c in zip(offs, COUNTS)], sd)
    torch.cuda.synchronize()
    out = hd.cpu()
    ref = h.clone()
    fused_differs = 0
    for k, (o, c) in enumerate(zip(offs, COUNTS)):
        if SCALES[k] != 0.0:
            prod = torch.tensor(SCALES[k], dtype=torch.float32) * r[o:o + c].float()          # one fp32 rounding
            ref[o:o + c] = (h[o:o + c].float() + prod).half()                                 # a second one, then fp16
            fma = (h[o:o + c].double() + float(torch.tensor(SCALES[k], dtype=torch.float32)) * r[o:o + c].double()).float().half()
            fused_differs += int((bits(fma) != bits(ref[o:o + c])).sum())
    assert torch.equal(bits(out), bits(ref))           # segments, zero-scale segments and every guard in one comparison
    assert torch.equal(bits(rd.cpu()), bits(r))
    assert fused_differs > 0                             # the data can tell a fused multiply-add from the two operations
    assert bool(torch.isnan(r).any()) and not bool(torch.isnan(out).any())


def test_add_control_reads_its_scales_on_the_device():
    """the same launch arguments with other scale VALUES: what a captured graph relies on"""
    from sdod.amd import ops
    h = torch.ones(4096, dtype=torch.float16, device='cuda')
    r = torch.full((4096,), 2.0, dtype=torch.float16, device='cuda')
    s = torch.zeros(1, dtype=torch.float32, device='cuda')
    g = torch.cuda.CUDAGraph()
    ops.add_control([h], [r], s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        ops.add_control([h], [r], s)
    g.replay(); torch.cuda.synchronize()
    assert bool((h == 1.0).all())
    s.fill_(0.5)
    g.replay(); torch.cuda.synchronize()
    assert bool((h == 2.0).all())


def test_add_control_refuses_bad_arguments_and_leaves_the_destination_untouched():
    from sdod.amd import _lib
    lib = _lib.hip()
    h = torch.full((4096 + 16,), 7.0, dtype=torch.float16, device='cuda')
    r = torch.ones(4096 + 16, dtype=torch.float16, device='cuda')
    s = torch.ones(20, dtype=torch.float32, device='cuda')
    Seg = _lib.ControlSeg
    one = lambda hp, rp, n: (Seg * 1)(Seg(hp, rp, n))
    bad = [
        (one(h.data_ptr(), r.data_ptr(), 4096), 0, P(s)),                     # no segment
        ((Seg * 17)(*[Seg(h.data_ptr(), r.data_ptr(), 8)] * 17), 17, P(s)),  # more than 16
        (one(h.data_ptr(), r.data_ptr(), 4096), 1, None),                     # no scales
        (one(None, r.data_ptr(), 4096), 1, P(s)),
        (one(h.data_ptr(), None, 4096), 1, P(s)),
        (one(h.data_ptr(), r.data_ptr(), 0), 1, P(s)),
        (one(h.data_ptr(), r.data_ptr(), 4092), 1, P(s)),                     # count % 8
        (one(h[4:].data_ptr(), r.data_ptr(), 4096), 1, P(s)),                 # misaligned h
        (one(h.data_ptr(), r[4:].data_ptr(), 4096), 1, P(s)),                 # misaligned r
        ((Seg * 2)(Seg(h.data_ptr(), r.data_ptr(), 2048), Seg(h[2048:].data_ptr(), r.data_ptr(), 100)), 2, P(s)),  # a good one first
    ]
    for segs, n, sp in bad:
        assert lib.sdod_add_control_f16(segs, n, sp, None) != 0 and lib.sdod_hip_last_error()
    assert lib.sdod_add_control_f16(None, 1, P(s), None) != 0
    torch.cuda.synchronize()
    assert bool((h == 7.0).all()) and bool((r == 1.0).all())
    assert lib.sdod_add_control_f16(one(h.data_ptr(), r.data_ptr(), 4096), 1, P(s), None) == 0        # the good call writes its range only
    torch.cuda.synchronize()
    assert bool((h[:4096] == 8.0).all()) and bool((h[4096:] == 7.0).all())


# ------------------------------------------------------------------ the u / 255 input convolution
def test_unit_input_convolution_on_exact_data():
    """input_hint_block.0 runs on u / 255 with a border that is zero in THAT space.  Exact data (u in {0, 255}, weights k / 16, dyadic
    bias: every product and partial sum is exact in fp32) against the fp64 definition, bit for bit; a non-zero constant image shows a
    border padded in another space: with 2 u / 255 - 1 the border taps would contribute -w, not 0."""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(41)
    cout, n, h, w = 64, 2, 6, 10
    wt = (torch.randint(-16, 17, (cout, 3, 3, 3), generator=g).float() / 16).half()
    bias = torch.randint(-8, 9, (cout,), generator=g).float() / 4
    packed = torch.zeros(cout, 64, dtype=torch.float16)
    packed[:, :27] = wt.permute(0, 2, 3, 1).reshape(cout, 27)
    const = torch.full((n, h, w, 3), 255, dtype=torch.uint8)
    mixed = (torch.randint(0, 2, (n, h, w, 3), generator=g) * 255).to(torch.uint8)
    for img in (const, mixed):
        x = (img.double() / 255).permute(0, 3, 1, 2)
        ref = F.conv2d(x, wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
        assert torch.equal(ref.half().double(), ref)                                           # the data is exact in fp16
        y = ops.image_conv_in_unit(img.cuda(), packed.cuda(), bias.cuda()).cpu()
        assert torch.equal(bits(y), bits(ref.half()))
    ref = F.conv2d((const.double() / 255).permute(0, 3, 1, 2), wt.double(), bias.double(), padding=1)
    assert not torch.equal(ref[:, :, 0, 0], ref[:, :, 2, 2])                                   # the border is visible in this image


# ------------------------------------------------------------------ graphs
@pytest.fixture(scope='module')
def weights():
    """synthetic weights: the UNet and its TEMB, and ONE ControlNet dict in the checkpoint's shapes (prefix stripped) from which the
    control graph, the hint encoder and the control TEMB each take their own names"""
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    sds = {'unet': Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234),
           'temb': Wt.synthetic_state_dict(E.Temb(cfg, 1).param_table(), seed=1235),
           'vae': Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1236),
           'vae_enc': Wt.synthetic_state_dict(E.VaeEncoder(cfg, 1).param_table(), seed=1238),
           'controlnet': Wt.synthetic_state_dict(CR.param_table(), seed=1241)}
    return sds


@pytest.fixture(scope='module')
def control_ref(weights):
    return CR.ControlNet(weights['controlnet']).eval()


def hint_image(h, w, phase=0.0):
    """a smooth pattern with edges, uint8 [1, 8h, 8w, 3]"""
    yy, xx = torch.meshgrid(torch.arange(8.0 * h), torch.arange(8.0 * w), indexing='ij')
    img = torch.stack([128 + 100 * torch.sin(xx / 7 + k + phase) * torch.cos(yy / 5 - phase) for k in range(3)], -1)
    img[:, 40:44] = 255.0
    return img.clamp(0, 255).to(torch.uint8)[None]


def test_parameter_tables_are_the_checkpoints(weights):
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    want = dict(CR.param_table())
    ccfg = E.copy_config(cfg); ccfg.control_temb = 1
    cn, tb, hb = E.ControlNet(cfg, 2).param_table(), E.Temb(ccfg, 1).param_table(), E.ControlHint(cfg, 1).param_table()
    assert all(want[n] == s for n, s in cn + tb) and not {n for n, _ in cn} & {n for n, _ in tb}
    assert {n for n, _ in cn + tb + hb} == set(want)                         # together: every tensor of the checkpoint, nothing else
    pad = {16: 64, 32: 64, 96: 128}
    assert [s for _, s in hb] == [tuple(pad.get(d, d) if i < 2 else d for i, d in enumerate(s)) for _, s in E.control_hint_checkpoint_table()]
    assert E.Temb(ccfg, 1).param_table()[:4] == E.Temb(cfg, 1).param_table()[:4] and len(tb) == 4 + 2 * 10


@pytest.mark.parametrize('hw', SIZES)
def test_hint_graph_matches_the_restatement(weights, control_ref, hw):
    from sdod.amd import engine as E, ops
    g = E.ControlHint(E.sd14_config(*hw), 1)
    g.load_state_dict(weights['controlnet']); g.finalize()
    labels = [l for l, _, _ in g.op_table()]
    assert labels[:2] == ['image_conv_in_unit', 'silu'] and len(labels) >= 9
    hint = hint_image(*hw)
    g.hint.copy_(hint); g.execute(); torch.cuda.synchronize()
    out = g.out.clone()
    ref = control_ref.guided_hint(hint)
    rl = rel_l2(nchw(out), ref)
    print(f'hint graph {hw}: rel-L2 vs fp32 restatement {rl:.3e}')
    assert tuple(out.shape) == (1, hw[0], hw[1], 320) and torch.isfinite(out).all() and rl <= 1e-2, rl
    g.execute(use_hip_graph=True); torch.cuda.synchronize()
    assert torch.equal(g.out, out)
    g.hint.copy_(hint_image(*hw, phase=1.3)); g.execute(use_hip_graph=True); torch.cuda.synchronize()
    assert rel_l2(nchw(g.out), control_ref.guided_hint(hint_image(*hw, phase=1.3))) <= 1e-2 and rel_l2(g.out.float(), out.float()) > 1e-2
    # the padded channels: zero weights and zero bias where the checkpoint has none, so the first convolution's (and with SiLU(0) = 0
    # every later one's) padded outputs are exactly zero
    for j, (real, built) in enumerate(zip((16, 16, 32, 32, 96, 96, 256), (64, 64, 64, 64, 128, 128, 256))):
        b = g.packed_param(f'input_hint_block.{2 * j}.bias', torch.float32)
        assert b.numel() == built and not bool(b[real:].any())
        wpk = g.packed_param(f'input_hint_block.{2 * j}.weight').reshape(built, -1)
        assert not bool(wpk[real:].any())
    w0 = g.packed_param('input_hint_block.0.weight').reshape(64, 64)
    first = ops.activation(ops.image_conv_in_unit(hint.cuda(), w0, g.packed_param('input_hint_block.0.bias', torch.float32)), 'silu')
    assert bool(first[..., :16].any()) and not bool(first[..., 16:].any())


def _control_inputs(hw, seed=7):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 4, *hw, generator=gen)
    ctx = torch.randn(2, 77, 768, generator=gen).half()
    t = torch.tensor([999.0, 999.0])        # the pipeline's batch: one time for both guidance halves
    return x, ctx, t


@pytest.mark.parametrize('hw', SIZES)
def test_control_graph_matches_the_restatement_bound_or_not(weights, control_ref, hw):
    from sdod.amd import engine as E
    cfg = E.sd14_config(*hw)
    ccfg = E.copy_config(cfg); ccfg.control_temb = 1
    tg = E.Temb(ccfg, 2); tg.load_state_dict(weights['controlnet']); tg.finalize()
    assert tg.width == 30 * 320
    x, ctx, t = _control_inputs(hw)
    hint = hint_image(*hw)
    guided = control_ref.guided_hint(hint)
    with torch.no_grad():
        refs = control_ref(x, t, ctx.float(), guided)
    shapes = E.control_residual_shapes(cfg, 2)
    assert [tuple(r.permute(0, 2, 3, 1).shape) for r in refs] == shapes
    slots = [torch.full(s, float('nan'), dtype=torch.float16, device='cuda') for s in shapes]

    def run(bound):
        g = E.ControlNet(cfg, 2)
        g.load_state_dict(weights['controlnet'])
        if bound:
            for k, s in enumerate(slots):
                g.bind_output(k, s)
        g.finalize()
        assert g.temb_width == tg.width and not bool(g.hint.any())
        tg.t.copy_(t); tg.execute()
        g.x.copy_(x); g.temb.copy_(tg.out); g.ctx.copy_(ctx); g.hint.copy_(guided.permute(0, 2, 3, 1).half())
        g.execute(); torch.cuda.synchronize()
        outs = [o.clone() for o in g.out]
        g.execute(use_hip_graph=True, static_unchanged=True); torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, g.out))
        return g, outs

    g, outs = run(False)
    src = g.tune_source()
    print(f'control graph {hw}: {g.stats()["launches"]} launches, arena {g.stats()["arena_bytes"]} B, tiles {src}')
    assert src['shapes_tuned_in_process'] == 0, src            # every GEMM tile from the shipped table
    for k, (o, r) in enumerate(zip(outs, refs)):
        rl = rel_l2(nchw(o), r)
        print(f'  residual {k} {tuple(o.shape)}: rel-L2 vs fp32 restatement {rl:.3e}')
        assert torch.isfinite(o).all() and rl <= 1e-2, (k, rl)
    gb, outs_b = run(True)
    assert all(o.data_ptr() == s.data_ptr() for o, s in zip(gb.out, slots))                   # no copy: the graph writes the caller's memory
    assert all(torch.equal(a, b) for a, b in zip(outs, outs_b)) and all(torch.equal(a, s) for a, s in zip(outs, slots))
    assert gb.stats()['launches'] == g.stats()['launches'] and gb.stats()['arena_bytes'] == g.stats()['arena_bytes']
    # the hint matters, and so does its place: the residuals move when it is dropped
    g.hint.zero_(); g.execute(); torch.cuda.synchronize()
    assert rel_l2(g.out[0].float(), outs[0].float()) > 1e-2
    with pytest.raises(Exception, match='size mismatch'):
        E.ControlNet(cfg, 2).bind_output(0, slots[3])
    with pytest.raises(Exception, match='misaligned'):
        E.ControlNet(cfg, 2).bind_output(0, torch.zeros(slots[0].numel() + 8, dtype=torch.float16, device='cuda')[8:])
    with pytest.raises(Exception):
        g.bind_output(0, slots[0])                                                             # after finalize


@pytest.fixture(scope='module')
def unets(weights):
    """the UNet without and with control inputs on the same weights, the oracle, one set of inputs, residuals that differ between the
    two batch halves, and the oracle's plain output"""
    from oracle import sd_torch as S
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    tg = E.Temb(cfg, 2); tg.load_state_dict(weights['temb']); tg.finalize()
    g0 = E.UNet(cfg, 2); g0.load_state_dict(weights['unet']); g0.finalize()
    c1 = E.copy_config(cfg); c1.control_inputs = 1
    g1 = E.UNet(c1, 2); g1.load_state_dict(weights['unet']); g1.finalize()
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**weights['unet'], **weights['temb']}, assign=True)
    unet.eval()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 16, 16, generator=gen)
    ctx = torch.randn(2, 77, 768, generator=gen).half()
    t = torch.tensor([999.0, 501.0])
    with torch.no_grad():
        ref0 = unet(x, t, ctx.float())
    res = [(4.0 * torch.randn(b, c, h, w, generator=gen)).half() for b, h, w, c in E.control_residual_shapes(cfg, 2)]
    return dict(tg=tg, g0=g0, g1=g1, unet=unet, x=x, ctx=ctx, t=t, ref0=ref0, res=res)


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
    return nchw(eager)


def test_unet_with_control_inputs_is_the_plain_graph_plus_one_launch(unets):
    r = unets
    g0, g1 = r['g0'], r['g1']
    assert not hasattr(g0, 'control_res') and len(g1.control_res) == 13 and tuple(g1.control_scale.shape) == (13,)
    assert all(not bool(s.any()) for s in g1.control_res) and not bool(g1.control_scale.any())          # zeroed at finalize
    with pytest.raises(Exception):
        g0._io(False, 3)
    with pytest.raises(Exception):
        g1._io(False, 17)
    s0, s1 = g0.stats(), g1.stats()
    print(f'UNet b2 16x16: {s0["launches"]} launches, arena {s0["arena_bytes"]} B; with control inputs {s1["launches"]}, {s1["arena_bytes"]} B')
    assert (s0['launches'], s0['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES)
    assert s1['launches'] == s0['launches'] + 1 and s1['weight_bytes'] == s0['weight_bytes'] and s1['arena_bytes'] == CONTROL_ARENA_BYTES
    l0, l1 = [l for l, _, _ in g0.op_table()], [l for l, _, _ in g1.op_table()]
    assert l1.count('add_control') == 1 and 'add_control' not in l0 and [l for l in l1 if l != 'add_control'] == l0
    assert g1.tune_source()['shapes_tuned_in_process'] == 0
    out0 = _eval(g0, r)
    assert torch.equal(_eval(g1, r), out0)                                   # zero scales: the plain output, bit for bit
    for slot, res in zip(g1.control_res, r['res']):                          # ... whatever the slots hold
        slot.copy_(res.permute(0, 2, 3, 1))
    assert torch.equal(_eval(g1, r), out0)
    for slot in g1.control_res:
        slot.zero_()
    rl = rel_l2(out0, r['ref0'])
    print(f'plain graph vs fp32 oracle rel-L2 {rl:.3e}')
    assert rl <= 1e-2


@pytest.mark.parametrize('case', [0, 3, 11, 12, 'all'])
def test_unet_residuals_match_the_controlled_oracle(unets, case):
    """one residual at a time -- the first skip, the one behind the first stride-2 convolution, the last skip, the middle -- then all
    13 with unequal scales, different residuals in the two batch halves, against cldm's ControlledUnetModel on the fp32 oracle"""
    r = unets
    g1 = r['g1']
    scales = [0.0] * 13
    if case == 'all':
        scales = [0.5 + 0.1 * k for k in range(13)]
    else:
        scales[case] = 1.5
    with torch.no_grad():
        ref = CR.controlled_unet(r['unet'], r['x'], r['t'], r['ctx'].float(), [c.float() for c in r['res']], scales)
    moved = rel_l2(ref, r['ref0'])
    assert moved > 5e-2, moved                                               # on the CPU, before any GPU work
    assert not bool(g1.control_scale.any())                                  # every test leaves the scales zero
    if 'zero' not in r:
        r['zero'] = _eval(g1, r)
    for slot, res in zip(g1.control_res, r['res']):
        slot.copy_(res.permute(0, 2, 3, 1))
    g1.control_scale.copy_(torch.tensor(scales))
    out = _eval(g1, r)
    g1.control_scale.zero_()
    for slot in g1.control_res:
        slot.zero_()
    rl, away = rel_l2(out, ref), rel_l2(out, r['zero'])
    print(f'UNet with residual {case}: rel-L2 vs controlled oracle {rl:.3e}, vs the zero-scale output {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(out).all() and rl <= 1e-2 and away > 1e-2, (rl, away)


# ------------------------------------------------------------------ pipeline
class _Controlled:
    """the fp32 chain's model: control net, then the controlled UNet (what Txt2Img._unet_eps runs as two graphs)"""

    def __init__(self, unet, control, guided, scales):
        self.unet, self.control, self.guided, self.scales = unet, control, guided, scales

    def __call__(self, x, t, ctx):
        with torch.no_grad():
            res = self.control(x, t, ctx, self.guided)
            return CR.controlled_unet(self.unet, x, t, ctx, res, self.scales)


@pytest.fixture(scope='module')
def rig(weights):
    from oracle import sd_torch as S
    from sdod.amd.pipeline import Txt2Img
    kw = dict(state_dicts=weights, images_per_gpu=1, latent_hw=16, with_text_encoder=False, with_vae_encoder=True)
    pipe = Txt2Img(controlnet=True, **kw)
    plain = Txt2Img(**kw)
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict({**weights['unet'], **weights['temb']}, assign=True)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    u8 = torch.randint(0, 256, (1, 128, 128, 3), generator=g, dtype=torch.uint8)
    return dict(pipe=pipe, plain=plain, unet=unet.eval(), ctx2=ctx2, x_T=x_T, u8=u8, hint=hint_image(16, 16), hint_b=hint_image(16, 16, phase=1.3))


class _Count:
    """counts a graph's execute() calls"""

    def __init__(self, g):
        self.g, self.n, self.orig = g, 0, g.execute

    def __enter__(self):
        def execute(*a, **k):
            self.n += 1
            return self.orig(*a, **k)
        self.g.execute = execute
        return self

    def __exit__(self, *exc):
        del self.g.execute


def test_pipeline_construction(rig):
    pipe, plain = rig['pipe'], rig['plain']
    assert pipe.controlnet.batch == 2 and pipe.control_hint.batch == 1 and pipe.unet.cfg.control_inputs == 1 and pipe.cfg.control_inputs == 0
    assert tuple(pipe.control_hint.hint.shape) == (1, 128, 128, 3) and tuple(pipe.controlnet.hint.shape) == (1, 16, 16, 320)
    assert all(o.data_ptr() == s.data_ptr() for o, s in zip(pipe.controlnet.out, pipe.unet.control_res))   # bound: nothing to copy per step
    assert plain.controlnet is None and plain.control_hint is None and not hasattr(plain.unet, 'control_res')
    assert plain.unet.stats()['launches'] + 1 == pipe.unet.stats()['launches']
    assert (plain.unet.stats()['launches'], plain.unet.stats()['arena_bytes']) == (PARENT_LAUNCHES, PARENT_ARENA_BYTES)
    for call in (lambda: plain.set_control_hint(rig['hint']), plain.clear_control_hint):
        with pytest.raises(RuntimeError, match='controlnet=True'):
            call()
    for bad in (rig['hint'][..., :2], rig['hint'].float(), rig['hint'][:, :64]):
        with pytest.raises(ValueError):
            pipe.set_control_hint(bad)
    for bad in (float('inf'), float('nan'), [1.0] * 12, [1.0] * 12 + [float('nan')], 'strong'):
        with pytest.raises(ValueError):
            pipe.set_control_hint(rig['hint'], bad)
    assert not pipe._control_on and not bool(pipe.unet.control_scale.any())


def test_refused_combinations(weights):
    from sdod.amd.pipeline import Txt2Img
    for kw in (dict(cfg_split=True), dict(hires_hw=32), dict(inpaint_unet=True), dict(adapter=True), dict(tiling=True), dict(model='sd21')):
        with pytest.raises(ValueError, match='controlnet'):
            Txt2Img(state_dicts=weights, latent_hw=16, with_text_encoder=False, controlnet=True, **kw)


@pytest.mark.parametrize('sampler', ['plms', 'dpmpp_2m'])
def test_eager_and_captured_are_the_same_and_a_new_hint_needs_no_capture(rig, sampler):
    pipe, plain, c, x_T = rig['pipe'], rig['plain'], rig['ctx2'].cuda(), rig['x_T']
    base = plain.generate(c, x_T, 4, 7.5, sampler)
    # cleared (as built): the plain pipeline bit for bit, eager and captured, and the control graph is not executed at all
    with _Count(pipe.controlnet) as cnt:
        assert torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
        assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base)
        assert cnt.n == 0
    n_off = len(pipe._traj)
    pipe.set_control_hint(rig['hint'])
    with _Count(pipe.controlnet) as cnt:
        eager = pipe.generate(c, x_T, 4, 7.5, sampler)
        assert cnt.n >= 4                                               # once per evaluation
    graphed = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert torch.equal(graphed, eager) and not torch.equal(eager, base)
    assert len(pipe._traj) == n_off + 1                                 # on and off are two trajectories
    n_graphs = len(pipe._traj)
    # another hint: a replay of the same capture
    pipe.set_control_hint(rig['hint_b'])
    graphed_b = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs
    assert not torch.equal(graphed_b, graphed) and torch.equal(graphed_b, pipe.generate(c, x_T, 4, 7.5, sampler))
    # another weight, per-residual weights, a grey hint without the channel axis: the same
    pipe.set_control_hint(rig['hint_b'], 0.5)
    graphed_w = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs and not torch.equal(graphed_w, graphed_b)
    pipe.set_control_hint(rig['hint_b'], [0.5] * 12 + [0.25])
    graphed_p = pipe.generate_graphed(c, x_T, 4, 7.5, sampler).clone()
    assert len(pipe._traj) == n_graphs and not torch.equal(graphed_p, graphed_w)
    assert pipe.unet.control_scale.tolist() == [0.5] * 12 + [0.25]
    pipe.set_control_hint(rig['hint'][..., 0])
    grey = pipe.controlnet.hint.clone()
    pipe.set_control_hint(rig['hint'][..., :1].expand(-1, -1, -1, 3).contiguous())
    assert torch.equal(pipe.controlnet.hint, grey)
    # all 13 scales 0.0 with a hint set: the control graph still runs and adds nothing
    pipe.set_control_hint(rig['hint_b'], 0.0)
    with _Count(pipe.controlnet) as cnt:
        assert torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base) and cnt.n >= 4
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and len(pipe._traj) == n_graphs
    pipe.set_control_hint(rig['hint'])
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), graphed)
    pipe.clear_control_hint()
    assert not bool(pipe.unet.control_scale.any())
    with _Count(pipe.controlnet) as cnt:
        assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, sampler), base) and torch.equal(pipe.generate(c, x_T, 4, 7.5, sampler), base)
        assert cnt.n == 0
    assert len(pipe._traj) == n_graphs
    assert torch.equal(plain.generate_graphed(c, x_T, 4, 7.5, sampler), base)


def test_controlled_latents_match_the_restatement_chain(rig, control_ref):
    """20 PLMS steps with a hint at weight 1 against the sampler restatement (oracle/pipeline_oracle.py) on the fp32 control net and
    controlled UNet"""
    from oracle import pipeline_oracle as PO
    pipe, x_T = rig['pipe'], rig['x_T']
    c16 = rig['ctx2'].float()
    guided = control_ref.guided_hint(rig['hint'])
    model = _Controlled(rig['unet'], control_ref, guided, [1.0] * 13)
    x2, t2 = x_T.repeat(2, 1, 1, 1), torch.tensor([981.0, 981.0])
    with torch.no_grad():
        moved = rel_l2(model(x2, t2, c16), rig['unet'](x2, t2, c16))     # the restatement's first evaluation, with and without control
    assert moved > 5e-2, moved                                           # on the CPU, before any GPU work
    z_ref = PO.plms_sample(model, c16[0:1], c16[1:2], x_T, steps=20, scale=7.5)
    pipe.clear_control_hint()
    z_plain = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5).cpu()
    pipe.set_control_hint(rig['hint'])
    assert rel_l2(nchw(pipe.controlnet.hint), guided) <= 1e-2
    hint_before = pipe.controlnet.hint.clone()
    z = pipe.sample_plms(rig['ctx2'].cuda(), x_T, 20, 7.5)
    assert torch.equal(hint_before, pipe.controlnet.hint)                # static: no sampler launch writes there
    rl, away = rel_l2(z.cpu(), z_ref), rel_l2(z.cpu(), z_plain)
    print(f'controlled plms final latent rel-L2 vs the restatement chain {rl:.3e}, vs the uncontrolled latent {away:.3e} (oracle moved {moved:.3e})')
    assert torch.isfinite(z).all() and rl <= 2e-2 and away > 1e-2, (rl, away)
    pipe.clear_control_hint()


def test_img2img_runs_conditioned(rig):
    pipe, plain, c, u8 = rig['pipe'], rig['plain'], rig['ctx2'].cuda(), rig['u8']
    g = torch.Generator().manual_seed(5)
    noise = (torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g))
    pipe.clear_control_hint()
    cleared = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
    assert torch.equal(cleared, plain.img2img(c, u8, 0.5, 8, 7.5, noise=noise))
    pipe.set_control_hint(rig['hint'])
    hinted = pipe.img2img_graphed(c, u8, 0.5, 8, 7.5, noise=noise).clone()
    assert not torch.equal(hinted, cleared)
    assert torch.equal(hinted, pipe.img2img(c, u8, 0.5, 8, 7.5, noise=noise))
    pipe.clear_control_hint()


def test_rectangle_and_two_images(weights):
    """latent (8, 16), two images per GPU: the control graph at batch 4, one hint per image, eager equals captured"""
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img(state_dicts=weights, images_per_gpu=2, latent_hw=(8, 16), with_text_encoder=False, with_vae=False, controlnet=True)
    g = torch.Generator().manual_seed(78)
    c = (torch.randn(2, 77, 768, generator=g) * 0.5).half().cuda()
    x_T = torch.randn(2, 4, 8, 16, generator=g)
    base = pipe.sample_plms(c, x_T, 4, 7.5).clone()
    hints = torch.cat([hint_image(8, 16), hint_image(8, 16, phase=1.3)])
    pipe.set_control_hint(hints)
    assert not torch.equal(pipe.controlnet.hint[0], pipe.controlnet.hint[1])
    z = pipe.sample_plms(c, x_T, 4, 7.5).clone()
    assert torch.isfinite(z).all() and rel_l2(z, base) > 1e-2
    guided = pipe.controlnet.hint.clone()
    pipe.set_control_hint(hints.flip(0))
    assert torch.equal(pipe.controlnet.hint, guided.flip(0))             # image i is conditioned by hint i
    z2 = pipe.sample_plms(c, x_T.flip(0), 4, 7.5).clone()
    assert rel_l2(z2.flip(0), z) <= 1e-2
    pipe.clear_control_hint()
    assert torch.equal(pipe.sample_plms(c, x_T, 4, 7.5), base)


def test_long_prompts_and_loras_work(weights):
    """prompt_chunks = 2 (154 keys: the control graph's transformers take the three-launch cross-attention like the UNet's) on a
    pipeline that keeps its base weights for LoRA adapters: conditioned, eager equals captured, cleared equals the same pipeline
    built without the flag"""
    from sdod.amd.pipeline import Txt2Img
    kw = dict(state_dicts=weights, images_per_gpu=1, latent_hw=16, with_text_encoder=False, prompt_chunks=2, loras=True)
    pipe, plain = Txt2Img(controlnet=True, **kw), Txt2Img(**kw)
    assert pipe.controlnet.cfg.context_len == 154 and tuple(pipe.controlnet.ctx.shape) == (2, 154, 768)
    g = torch.Generator().manual_seed(79)
    c = (torch.randn(2, 154, 768, generator=g) * 0.5).half().cuda()
    x_T = torch.randn(1, 4, 16, 16, generator=g)
    base = plain.generate(c, x_T, 4, 7.5, 'plms')
    assert torch.equal(pipe.generate(c, x_T, 4, 7.5, 'plms'), base)
    pipe.set_control_hint(hint_image(16, 16))
    eager = pipe.generate(c, x_T, 4, 7.5, 'plms')
    assert not torch.equal(eager, base) and torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, 'plms'), eager)
    pipe.clear_control_hint()
    assert torch.equal(pipe.generate_graphed(c, x_T, 4, 7.5, 'plms'), base)
