"""LyCORIS adapters in the engine graphs: Graph.set_networks on the 16x16 UNet (batch 2) and the text encoder, synthetic weights,
against the CPU oracle loaded with lycoris.merged_state_dict of the same factors (the rig of tests/test_lora_engine_gpu.py).

Adapters (tests/lycoris_cases.py): a LoHa set, rank 4, and a LoKr set, w1 cycling through 4 x 8, 2 x 64, 16 x 4 and 1 x 1 (a full
delta), each over every supported UNet weight (256 of them) at scale 0.05 of the weight's own spread.  On the CPU oracle the LoHa set
moves the UNet output by rel-L2 0.192, the LoKr set by 0.193, LoRA + LoHa + LoKr together by 0.329 -- measured once with the oracle
alone and asserted in the fixture to be at least 0.1, which the comparison needs to mean something; on six matrices of two
text-encoder layers at scale 0.1, LoHa + LoKr move the text encoder's output by 0.230.
Tolerances are the project's for the same graphs without adapters: UNet evaluation rel-L2 <= 1e-2, text encoder rel-L2 <= 5e-3."""
import pytest
import torch

import lora_cases as LC
import lycoris_cases as C

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


def unet_sets(sd, names):
    """the three entry lists over `names`: plain LoRA, LoHa, LoKr"""
    return dict(lora=LC.make_entries(sd, names, RANK, UNET_SCALE, seed=5), loha=C.make_loha_entries(sd, names, RANK, UNET_SCALE, seed=8),
                lokr=C.make_lokr_entries(sd, names, UNET_SCALE, seed=9))


@pytest.fixture(scope='module')
def rig():
    """synthetic weights, the three adapter sets, the oracle outputs (base, LoHa, LoKr, all three) and the projected time embedding"""
    from sdod.amd import engine as E, lycoris as L, weights as Wt
    cfg = E.sd14_config(16, 16)
    table = E.UNet(cfg, 2).param_table()
    sd = {**Wt.synthetic_state_dict(table, seed=1234), **Wt.synthetic_state_dict(E.Temb(cfg, 2).param_table(), seed=1235)}
    names = LC.unet_targets(table)
    sets = unet_sets(sd, names)
    sets['all'] = sets['lora'] + sets['loha'] + sets['lokr']
    tg = E.Temb(cfg, 2)
    tg.load_state_dict(sd)
    tg.finalize()
    t = torch.tensor([999.0, 999.0])
    tg.t.copy_(t); tg.execute()
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(77)
    x, ctx = torch.randn(2, 4, 16, 16, generator=gen), torch.randn(2, 77, 768, generator=gen).half()
    refs = {}
    with torch.no_grad():
        for tag in ('base', 'loha', 'lokr', 'all'):
            refs[tag] = _oracle(L.merged_state_dict(sd, sets.get(tag, [])))(x, t, ctx.float())
    for tag in ('loha', 'lokr', 'all'):
        assert rel_l2(refs[tag], refs['base']) >= 0.1, (tag, rel_l2(refs[tag], refs['base']))
    return dict(sd=sd, sets=sets, temb=tg.out.clone(), x=x, ctx=ctx, refs=refs, names=names)


def _graph(rig):
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    g = E.UNet(cfg, 2)
    g.load_state_dict(rig['sd'])
    g.keep_base()
    g.finalize()
    g.x.copy_(rig['x']); g.temb.copy_(rig['temb']); g.ctx.copy_(rig['ctx'])
    return g


def _run(g, **kw):
    g.execute(**kw)
    torch.cuda.synchronize()
    return g.eps.clone()


def _nchw(eps):
    return eps.float().cpu().permute(0, 3, 1, 2)


@pytest.fixture(scope='module')
def g77(rig):
    """the graph with a kept base, its base output and clones of the watched packed weights right after finalize()"""
    g = _graph(rig)
    packed = {n: g.packed_param(n).clone() for n in WATCHED}
    base = _run(g)
    return g, base, packed


@pytest.mark.parametrize('family', ['loha', 'lokr'])
def test_unet_with_one_family_matches_oracle_on_merged_weights(rig, g77, family):
    g, base, packed = g77
    g.set_networks(rig['sets'][family])
    changed = [n for n in WATCHED if not torch.equal(g.packed_param(n), packed[n])]
    assert changed == WATCHED, changed
    out = _run(g)
    r = rel_l2(_nchw(out), rig['refs'][family])
    moved = rel_l2(_nchw(out), _nchw(base))
    print(f'unet + {family}: rel-L2 vs merged oracle {r:.3e}, moved from the base output by {moved:.3f} '
          f'(oracle: {rel_l2(rig["refs"][family], rig["refs"]["base"]):.3f})')
    assert torch.isfinite(out).all() and r <= 1e-2, r
    assert moved >= 0.05, moved
    g.set_networks([])
    for n in WATCHED:
        assert torch.equal(g.packed_param(n), packed[n]), n
    assert torch.equal(_run(g), base)
    g.check()


def test_three_families_on_the_same_parameters_accumulate(rig, g77):
    g, base, _ = g77
    g.set_networks(rig['sets']['all'])
    out = _run(g)
    r = rel_l2(_nchw(out), rig['refs']['all'])
    print(f'LoRA + LoHa + LoKr on every weight: rel-L2 vs oracle with all merged {r:.3e} '
          f'(oracle moved {rel_l2(rig["refs"]["all"], rig["refs"]["base"]):.3f})')
    assert r <= 1e-2, r
    g.set_networks(rig['sets']['loha'])
    one = _run(g)
    assert rel_l2(_nchw(one), rig['refs']['loha']) <= 1e-2 and not torch.equal(one, out)
    g.set_networks([])
    assert torch.equal(_run(g), base)


def test_set_loras_and_set_networks_give_equal_arena_bits(rig, g77):
    g, base, packed = g77
    ent = rig['sets']['lora']
    g.set_loras(ent)
    via_loras = {n: g.packed_param(n).clone() for n in WATCHED}
    out_loras = _run(g)
    g.set_networks([])
    for n in WATCHED:
        assert torch.equal(g.packed_param(n), packed[n]), n
    g.set_networks(ent)
    for n in WATCHED:
        assert torch.equal(g.packed_param(n), via_loras[n]) and not torch.equal(via_loras[n], packed[n]), n
    assert torch.equal(_run(g), out_loras)
    g.set_loras([])
    assert torch.equal(_run(g), base)


def test_a_bad_entry_in_the_middle_leaves_the_arena_untouched(rig, g77):
    from sdod.amd._lib import SdodError
    g, base, packed = g77
    name = WATCHED[0]                                  # a 320 x 320 Linear
    good = rig['sets']['loha'][:2] + rig['sets']['lokr'][:2]
    z = torch.zeros
    bad = [
        ('loha', 'no.such.weight', z(320, 4), z(4, 320), z(320, 4), z(4, 320), 1.0),
        ('lokr', 'input_blocks.1.1.proj_in.bias', z(4, 4), z(80, 80), 1.0),                 # a vector
        ('loha', name, z(320, 4), z(4, 320), z(320, 4), z(4, 328), 1.0),                    # wrong-shaped factor
        ('loha', name, z(320, 4), z(4, 320), z(320, 5), z(5, 320), 1.0),                    # two ranks
        ('loha', name, z(320, 129), z(129, 320), z(320, 129), z(129, 320), 1.0),            # rank
        ('loha', name, z(320, 4), z(4, 320), z(320, 4), z(4, 320), float('nan')),
        ('lokr', name, z(3, 4), z(107, 80), 1.0),                                           # a does not divide 320
        ('lokr', name, z(4, 4), z(80, 79), 1.0),                                            # w2 of the wrong size
        ('lokr', name, z(4, 4), z(80, 80), float('inf')),
        ('loka', name, z(4, 4), z(80, 80), 1.0),                                            # no such kind
        (name, z(320, 4), z(4, 320)),                                                       # no such form
    ]
    for i, entry in enumerate(bad):
        with pytest.raises((SdodError, ValueError)):
            g.set_networks(good[:2] + [entry] + good[2:])
        for n in WATCHED:
            assert torch.equal(g.packed_param(n), packed[n]), (i, n)
    assert torch.equal(_run(g, static_unchanged=True), base)
    # the shape checks against param_table() are ValueErrors, as set_loras's are
    for i in (2, 3, 6, 7, 9, 10):
        with pytest.raises(ValueError):
            g.set_networks([bad[i]])


def test_captured_replay_follows_the_new_weights(rig):
    g = _graph(rig)
    base = _run(g)
    assert torch.equal(_run(g, use_hip_graph=True), base)                    # captured before set_networks
    g.set_networks(rig['sets']['loha'])
    skipped = _run(g, static_unchanged=True)          # immediately after set_networks: the flag is ignored once
    full = _run(g, static_unchanged=False)
    assert torch.equal(skipped, full) and not torch.equal(full, base)
    assert torch.equal(_run(g, use_hip_graph=True), full)
    g.set_networks(rig['sets']['lokr'])
    lokr = _run(g, use_hip_graph=True, static_unchanged=True)                # the replay as the first execute after the change
    assert not torch.equal(lokr, full) and torch.equal(_run(g), lokr)
    g.set_networks([])
    assert torch.equal(_run(g, use_hip_graph=True, static_unchanged=True), base)
    g.check()


def test_text_encoder_with_loha_and_lokr(rig):
    from oracle import sd_torch as S
    from sdod.amd import engine as E, lycoris as L, weights as Wt
    cfg = E.sd14_config()
    table = E.TextEncoder(cfg, 2).param_table()
    sd = Wt.synthetic_state_dict(table, seed=1236)
    names = LC.text_targets(table, (0, 11))
    assert len(names) == 12
    ent = C.make_loha_entries(sd, names, RANK, TEXT_SCALE, seed=7) + C.make_lokr_entries(sd, names, TEXT_SCALE, seed=8)
    g = E.TextEncoder(cfg, 2)
    g.load_state_dict(sd)
    g.keep_base()
    g.finalize()
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
    g.set_networks(ent)
    g.execute(use_hip_graph=True); g.execute(use_hip_graph=True); torch.cuda.synchronize()
    r = rel_l2(g.out.float().cpu(), refs[1])
    print(f'clip + loha + lokr rel-L2 {r:.3e} (base {rel_l2(base.float().cpu(), refs[0]):.3e}), oracle moved {rel_l2(refs[1], refs[0]):.3f}')
    assert torch.isfinite(g.out).all() and r <= 5e-3, r
    g.set_networks([])
    for n, w in packed.items():
        assert torch.equal(g.packed_param(n), w), n
    g.execute(use_hip_graph=True); torch.cuda.synchronize()
    assert torch.equal(g.out, base)
