"""LoRA adapters in the engine graphs: Graph.keep_base / set_loras / base_bytes on the 16x16 UNet (batch 2) and the text encoder,
synthetic weights, against the CPU oracle loaded with lora.merged_state_dict of the same factors.

Adapters: rank 4 on every supported UNet weight (256 of them), scale 0.05 of the weight's own spread (tests/lora_cases.py).  On the CPU
oracle that moves the UNet output by rel-L2 0.199 (two such adapters: 0.259) and, at scale 0.1 on six matrices of two layers, the text
encoder's by 0.182 -- measured once with the oracle alone, well above the 0.1 the comparison needs to mean something.
Tolerances are the project's for the same graphs without adapters: UNet evaluation rel-L2 <= 1e-2 (test_unet_graph_with_long_context),
text encoder rel-L2 <= 5e-3 (test_text_encoder_graph)."""
import pytest
import torch

import lora_cases as C

pytestmark = pytest.mark.gpu

UNET_SCALE, TEXT_SCALE, RANK = 0.05, 0.1, 4
# a LayerNorm-folded Linear, the composed proj_out (with ff.net.2 in front of it), a GEGLU matrix, a 3x3 convolution, a fused K/V member
WATCHED = ['input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight', 'input_blocks.1.1.transformer_blocks.0.ff.net.2.weight',
           'input_blocks.1.1.transformer_blocks.0.ff.net.0.proj.weight', 'input_blocks.1.0.in_layers.2.weight',
           'middle_block.1.transformer_blocks.0.attn2.to_k.weight', 'input_blocks.4.0.out_layers.3.weight']


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _oracle(sd):
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel()
    unet.load_state_dict(sd, assign=True)
    return unet.eval()


@pytest.fixture(scope='module')
def rig():
    """synthetic weights, two adapters over every supported UNet weight, the oracle outputs (base, one adapter, both) for 77 and 154
    keys, and the projected time embedding of t = 999"""
    from sdod.amd import engine as E, lora as L, weights as Wt
    cfg = E.sd14_config(16, 16)
    table = E.UNet(cfg, 2).param_table()
    sd = {**Wt.synthetic_state_dict(table, seed=1234), **Wt.synthetic_state_dict(E.Temb(cfg, 2).param_table(), seed=1235)}
    names = C.unet_targets(table)
    ent_a = C.make_entries(sd, names, RANK, UNET_SCALE, seed=5)
    ent_b = C.make_entries(sd, names, RANK, UNET_SCALE, seed=6)
    tg = E.Temb(cfg, 2)
    tg.load_state_dict(sd)
    tg.finalize()
    t = torch.tensor([999.0, 999.0])
    tg.t.copy_(t); tg.execute()
    torch.cuda.synchronize()
    inputs, refs = {}, {}
    for cl in (77, 154):
        gen = torch.Generator().manual_seed(cl)
        inputs[cl] = (torch.randn(2, 4, 16, 16, generator=gen), torch.randn(2, cl, 768, generator=gen).half())
    with torch.no_grad():
        for tag, ents in (('base', []), ('a', ent_a), ('ab', ent_a + ent_b)):
            unet = _oracle(L.merged_state_dict(sd, ents))
            for cl in ((77, 154) if tag == 'a' else (77,)):
                refs[tag, cl] = unet(inputs[cl][0], t, inputs[cl][1].float())
    assert rel_l2(refs['a', 77], refs['base', 77]) >= 0.1 and rel_l2(refs['ab', 77], refs['base', 77]) >= 0.1
    return dict(sd=sd, ent_a=ent_a, ent_b=ent_b, temb=tg.out.clone(), inputs=inputs, refs=refs, names=names)


def _graph(rig, context_len=77, keep=True, quant=0):
    from sdod.amd import engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    cfg.context_len = context_len
    cfg.weight_quant = quant
    g = E.UNet(cfg, 2)
    sd = rig['sd']
    if quant:
        sd = Wt.quantize_state_dict({k: v for k, v in sd.items() if k in dict(g.param_table())})
    g.load_state_dict(sd)
    if keep:
        g.keep_base()
    g.finalize()
    x, ctx = rig['inputs'][context_len]
    g.x.copy_(x); g.temb.copy_(rig['temb']); g.ctx.copy_(ctx)
    return g


def _run(g, **kw):
    g.execute(**kw)
    torch.cuda.synchronize()
    return g.eps.clone()


def _nchw(eps):
    return eps.float().cpu().permute(0, 3, 1, 2)


@pytest.fixture(scope='module')
def g77(rig):
    """the 77-key graph with a kept base, its base output and clones of the watched packed weights right after finalize()"""
    g = _graph(rig, 77)
    packed = {n: g.packed_param(n).clone() for n in WATCHED}
    base = _run(g)
    return g, base, packed


@pytest.mark.parametrize('context_len', [77, 154])
def test_unet_with_lora_matches_oracle_on_merged_weights(rig, g77, context_len):
    if context_len == 77:
        g, base = g77[0], g77[1]
    else:
        g = _graph(rig, context_len)
        base = _run(g)
    labels = [o[0] for o in g.op_table()]
    n_attn = sum(lab.startswith('attn_d') for lab in labels)
    # 16 self-attention launches; cross-attention is folded (no attention launch) up to 80 keys where the map has a multiple of 32
    # rows -- the ten blocks at 16 x 16 and 8 x 8 -- and the three-launch form in the six blocks at 4 x 4 and 2 x 2, and everywhere above 80 keys
    assert n_attn == (16 + 6 if context_len == 77 else 32)
    g.set_loras(rig['ent_a'])
    out = _run(g)
    r = rel_l2(_nchw(out), rig['refs']['a', context_len])
    moved = rel_l2(_nchw(out), _nchw(base))
    print(f'unet + lora, {context_len} keys ({n_attn} attention launches): rel-L2 vs merged oracle '
          f'{r:.3e}, moved from the base output by {moved:.3f}')
    assert torch.isfinite(out).all() and r <= 1e-2, r
    assert moved >= 0.05, moved
    g.set_loras([])
    assert torch.equal(_run(g), base)
    g.check()


def test_two_adapters_on_the_same_modules(rig, g77):
    g, base, _ = g77
    g.set_loras(rig['ent_a'] + rig['ent_b'])
    out = _run(g)
    r = rel_l2(_nchw(out), rig['refs']['ab', 77])
    print(f'two adapters: rel-L2 vs oracle with both merged {r:.3e}')
    assert r <= 1e-2, r
    g.set_loras(rig['ent_a'])
    one = _run(g)
    assert rel_l2(_nchw(one), rig['refs']['a', 77]) <= 1e-2 and not torch.equal(one, out)
    g.set_loras([])
    assert torch.equal(_run(g), base)


def test_clear_restores_the_packed_arena_bit_for_bit(rig, g77):
    g, base, packed = g77
    g.set_loras(rig['ent_a'])
    changed = [n for n in WATCHED if not torch.equal(g.packed_param(n), packed[n])]
    assert changed == WATCHED, changed
    _run(g)
    g.set_loras([])
    for n in WATCHED:
        assert torch.equal(g.packed_param(n), packed[n]), n
    assert torch.equal(_run(g), base)
    g.check()


def test_captured_replay_and_static_launches_follow_the_weights(rig):
    g = _graph(rig, 77)
    base = _run(g)
    assert torch.equal(_run(g, use_hip_graph=True), base)                    # captured before set_loras
    g.set_loras(rig['ent_a'])
    skipped = _run(g, static_unchanged=True)          # immediately after set_loras: the flag is ignored once
    full = _run(g, static_unchanged=False)
    assert torch.equal(skipped, full) and not torch.equal(full, base)
    assert torch.equal(_run(g, use_hip_graph=True), full)
    assert torch.equal(_run(g, use_hip_graph=True, static_unchanged=True), full)
    g.set_loras([])
    assert torch.equal(_run(g, use_hip_graph=True, static_unchanged=True), base)
    # ... and with the replay as the first execute after the change
    g.set_loras(rig['ent_a'])
    assert torch.equal(_run(g, use_hip_graph=True, static_unchanged=True), full)
    g.check()


def test_errors_leave_weights_and_output_unchanged(rig, g77):
    from sdod.amd._lib import SdodError
    g, base, packed = g77
    sd, name = rig['sd'], WATCHED[0]
    good = rig['ent_a'][:3]
    up, down = torch.zeros(320, 4), torch.zeros(4, 320)
    bad = [
        good + [('no.such.weight', up, down, 1.0)],
        good + [('input_blocks.1.1.proj_in.bias', up, down, 1.0)],                      # a vector
        good + [('input_blocks.0.0.weight', torch.zeros(320, 4, 1, 1), torch.zeros(4, 4, 3, 3), 1.0)],
        good + [(name, torch.zeros(320, 4), torch.zeros(4, 328), 1.0)],                 # wrong-shaped factor
        good + [(name, torch.zeros(321, 4), down, 1.0)],
        good + [(name, torch.zeros(320, 129), torch.zeros(129, 320), 1.0)],             # rank
        good + [(name, up, down, float('nan'))],
    ]
    for i, entries in enumerate(bad):
        with pytest.raises((SdodError, ValueError)):
            g.set_loras(entries)
        for n in WATCHED:
            assert torch.equal(g.packed_param(n), packed[n]), (i, n)
    assert torch.equal(_run(g, static_unchanged=True), base)
    # a graph without keep_base() and one with uint8 weights refuse as a whole
    plain = _graph(rig, 77, keep=False)
    assert plain.base_bytes() == 0
    w0 = plain.packed_param(name).clone()
    e0 = _run(plain)
    with pytest.raises(SdodError, match='keep_base'):
        plain.set_loras(good)
    with pytest.raises(SdodError, match='keep_base'):
        plain.set_loras([])
    with pytest.raises(SdodError, match='before finalize'):
        plain.keep_base()
    assert torch.equal(plain.packed_param(name), w0) and torch.equal(_run(plain, static_unchanged=True), e0)
    del plain
    q = _graph(rig, 77, keep=True, quant=1)
    wq = q.packed_param(name, torch.uint8).clone()
    eq = _run(q)
    with pytest.raises(SdodError, match='weight_quant'):
        q.set_loras(good)
    assert torch.equal(q.packed_param(name, torch.uint8), wq) and torch.equal(_run(q, static_unchanged=True), eq)


def test_base_bytes(rig, g77):
    g = g77[0]
    assert g.base_bytes() == g.stats()['weight_bytes'] > 0


def test_text_encoder_with_lora(rig):
    from oracle import sd_torch as S
    from sdod.amd import engine as E, lora as L, weights as Wt
    cfg = E.sd14_config()
    table = E.TextEncoder(cfg, 2).param_table()
    sd = Wt.synthetic_state_dict(table, seed=1236)
    names = C.text_targets(table, (0, 11))
    assert len(names) == 12
    ent = C.make_entries(sd, names, RANK, TEXT_SCALE, seed=7)
    g = E.TextEncoder(cfg, 2)
    g.load_state_dict(sd)
    g.keep_base()
    g.finalize()
    assert g.base_bytes() == g.stats()['weight_bytes']
    ids = torch.randint(0, 49408, (2, 77), generator=torch.Generator().manual_seed(5))
    ids[0, 10:] = 49407
    g.ids.copy_(ids.int())
    packed = {n: g.packed_param(n).clone() for n in names[:6]}
    g.execute(); torch.cuda.synchronize()
    base = g.out.clone()
    refs = []
    with torch.no_grad():
        for s in (sd, L.merged_state_dict(sd, ent)):
            with torch.device('meta'):
                clip = S.ClipTextModel()
            clip.load_state_dict(s, assign=True)
            refs.append(clip.eval()(ids))
    assert rel_l2(refs[1], refs[0]) >= 0.1
    g.set_loras(ent)
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True); torch.cuda.synchronize()
    r = rel_l2(g.out.float().cpu(), refs[1])
    print(f'clip + lora rel-L2 {r:.3e} (base {rel_l2(base.float().cpu(), refs[0]):.3e}), moved {rel_l2(g.out.float().cpu(), base.float().cpu()):.3f}')
    assert torch.isfinite(g.out).all() and r <= 5e-3, r
    g.set_loras([])
    for n, w in packed.items():
        assert torch.equal(g.packed_param(n), w), n
    g.execute(use_hip_graph=True); torch.cuda.synchronize()
    assert torch.equal(g.out, base)
