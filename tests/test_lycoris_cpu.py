"""sdod/amd/lycoris.py on the CPU: reading every family and sub-form from synthetic dicts, the scale rules, the fp64 host merge against an
independent restatement, the host reductions against the unreduced definitions, what is refused, and the fp32 restatement of the LoHa
kernel's arithmetic against the bound its GPU test asserts."""
import pytest
import torch

import lycoris_cases as C

Q, K_, V = (f'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn1_to_{m}' for m in 'qkv')
Q2, K2 = (f'lora_unet_mid_block_attentions_0_transformer_blocks_0_attn2_to_{m}' for m in 'qk')
R0C1, R0C2, R1C1, R1C2 = (f'lora_unet_mid_block_resnets_{j}_conv{c}' for j in (0, 1) for c in (1, 2))
TE = 'lora_te_text_model_encoder_layers_0_mlp_fc1'
PARAM = {Q: 'middle_block.1.transformer_blocks.0.attn1.to_q.weight', K_: 'middle_block.1.transformer_blocks.0.attn1.to_k.weight',
         V: 'middle_block.1.transformer_blocks.0.attn1.to_v.weight', Q2: 'middle_block.1.transformer_blocks.0.attn2.to_q.weight',
         K2: 'middle_block.1.transformer_blocks.0.attn2.to_k.weight', R0C1: 'middle_block.0.in_layers.2.weight',
         R0C2: 'middle_block.0.out_layers.3.weight', R1C1: 'middle_block.2.in_layers.2.weight', R1C2: 'middle_block.2.out_layers.3.weight',
         TE: 'text_model.encoder.layers.0.mlp.fc1.weight'}
LIN, CONV = (24, 40), (12, 8, 3, 3)      # small stand-ins for the weights: the reader never sees the model's sizes
# module -> (family, alpha, the size alpha is divided by, scale)
EXPECT = {Q: ('lora', 1.5, 3, 0.5), R0C1: ('lora', 2.0, 4, 0.5), K_: ('loha', 2.5, 5, 0.5), R0C2: ('loha', None, 3, 1.0),
          V: ('lokr', 7.0, None, 1.0), Q2: ('lokr', 1.0, 2, 0.5), R1C1: ('lokr', 1.5, 3, 0.5), R1C2: ('lokr', 3.0, 3, 1.0),
          K2: ('full', 9.0, None, 1.0), TE: ('lora', None, 2, 1.0)}


def _file(seed=1):
    """every family and sub-form, fp16 tensors (so that a transposition or a pass-through is exact)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=gen) * 0.5).half()
    f = {f'{Q}.lora_up.weight': r(24, 3), f'{Q}.lora_down.weight': r(3, 40),                                   # plain LoRA
         f'{R0C1}.lora_up.weight': r(12, 4, 1, 1), f'{R0C1}.lora_mid.weight': r(4, 4, 3, 3), f'{R0C1}.lora_down.weight': r(4, 8, 1, 1),   # Tucker LoCon
         f'{K_}.hada_w1_a': r(24, 5), f'{K_}.hada_w1_b': r(5, 40), f'{K_}.hada_w2_a': r(24, 5), f'{K_}.hada_w2_b': r(5, 40),              # LoHa
         f'{R0C2}.hada_t1': r(3, 3, 3, 3), f'{R0C2}.hada_w1_a': r(3, 12), f'{R0C2}.hada_w1_b': r(3, 8),                                    # Tucker LoHa
         f'{R0C2}.hada_t2': r(3, 3, 3, 3), f'{R0C2}.hada_w2_a': r(3, 12), f'{R0C2}.hada_w2_b': r(3, 8),
         f'{V}.lokr_w1': r(4, 5), f'{V}.lokr_w2': r(6, 8),                                                       # LoKr, both sides full
         f'{Q2}.lokr_w1_a': r(4, 2), f'{Q2}.lokr_w1_b': r(2, 5), f'{Q2}.lokr_w2': r(6, 8),                       # LoKr, w1 factored
         f'{R1C1}.lokr_w1': r(2, 2), f'{R1C1}.lokr_w2_a': r(6, 3), f'{R1C1}.lokr_w2_b': r(3, 36),                # LoKr, w2 factored (conv, flat)
         f'{R1C2}.lokr_w1': r(2, 2), f'{R1C2}.lokr_t2': r(3, 3, 3, 3), f'{R1C2}.lokr_w2_a': r(3, 6), f'{R1C2}.lokr_w2_b': r(3, 4),   # Tucker LoKr
         f'{K2}.diff': r(24, 40),                                                                                # full
         f'{TE}.lora_up.weight': r(24, 2), f'{TE}.lora_down.weight': r(2, 40)}
    for m, (_, alpha, _, _) in EXPECT.items():
        if alpha is not None:
            f[f'{m}.alpha'] = torch.tensor(alpha)
    return f


def _sd(seed=2):
    gen = torch.Generator().manual_seed(seed)
    return {PARAM[m]: torch.randn(*(CONV if 'resnets' in m else LIN), generator=gen) for m in PARAM}


def _tucker(core, wa, wb):
    """out[o, i, k, l] = sum_r sum_s core[r, s, k, l] wa[r, o] wb[s, i], by two tensordots"""
    half = torch.tensordot(wa.double(), core.double(), dims=([0], [0]))            # [o, s, k, l]
    return torch.tensordot(half, wb.double(), dims=([1], [0])).permute(0, 3, 1, 2)  # [o, k, l, i] -> [o, i, k, l]


def _kron(w1, w2):
    """out[o, i, ...] = w1[o // c, i // d] * w2[o % c, i % d, ...], by index tensors"""
    (a, b), (c, d) = w1.shape, w2.shape[:2]
    o, i = torch.arange(a * c), torch.arange(b * d)
    left = w1.double()[(o // c)[:, None], (i // d)[None, :]]
    right = w2.double()[(o % c)[:, None], (i % d)[None, :]]
    return left.reshape(left.shape + (1,) * (w2.dim() - 2)) * right


def _restated_delta(m, f):
    """the unreduced definition of module m's difference, written out without torch.kron or einsum"""
    g = lambda n: f[f'{m}.{n}'].double()
    fam = EXPECT[m][0]
    if fam == 'lora':
        up, down = g('lora_up.weight').reshape(g('lora_up.weight').shape[0], -1), g('lora_down.weight')
        if f'{m}.lora_mid.weight' in f:
            return _tucker(g('lora_mid.weight'), up.t(), down.reshape(down.shape[0], -1))
        return up @ down.reshape(down.shape[0], -1)
    if fam == 'loha':
        if f'{m}.hada_t1' in f:
            return _tucker(g('hada_t1'), g('hada_w1_a'), g('hada_w1_b')) * _tucker(g('hada_t2'), g('hada_w2_a'), g('hada_w2_b'))
        return (g('hada_w1_a') @ g('hada_w1_b')) * (g('hada_w2_a') @ g('hada_w2_b'))
    if fam == 'lokr':
        w1 = g('lokr_w1') if f'{m}.lokr_w1' in f else g('lokr_w1_a') @ g('lokr_w1_b')
        if f'{m}.lokr_w2' in f:
            w2 = g('lokr_w2')
        elif f'{m}.lokr_t2' in f:
            w2 = _tucker(g('lokr_t2'), g('lokr_w2_a'), g('lokr_w2_b'))
        else:
            w2 = (g('lokr_w2_a') @ g('lokr_w2_b')).reshape(6, 4, 3, 3)
        return _kron(w1, w2)
    return g('diff')


def test_read_network_families_shapes_and_scales(tmp_path):
    from safetensors.torch import save_file
    from sdod.amd import lycoris as L
    f = _file()
    net = L.read_network(f)
    assert set(net) == set(EXPECT) and net.refused == {}
    for m, (fam, alpha, rank, scale) in EXPECT.items():
        mod = net[m]
        assert (mod['family'], mod['alpha'], mod['rank'], mod['scale']) == (fam, alpha, rank, scale), m
        assert set(mod['tensors']) == {k.partition('.')[2] for k in f if k.startswith(m + '.')} - {'alpha'}
    path = tmp_path / 'net.safetensors'
    save_file({k: v.contiguous() for k, v in f.items()}, str(path))
    again = L.read_network(str(path))
    assert {m: (d['family'], d['scale']) for m, d in again.items()} == {m: (d['family'], d['scale']) for m, d in net.items()}
    assert L.read_network(net) is net
    # the reduced forms: what the device is handed
    red = {m: L.reduce_module(net[m]) for m in net}
    assert [red[m][0] for m in (Q, R0C1, K_, R0C2, V, Q2, R1C1, R1C2, K2)] == ['lora', 'lora', 'loha', 'loha', 'lokr', 'lokr', 'lokr', 'lokr', 'lokr']
    assert red[Q][1] is f[f'{Q}.lora_up.weight'] and red[K_][2] is f[f'{K_}.hada_w1_b'] and red[V][2] is f[f'{V}.lokr_w2']   # pass-through
    assert tuple(red[R0C1][2].shape) == (4, 8, 3, 3) and red[R0C1][2].dtype == torch.float16
    assert [tuple(t.shape) for t in red[R0C2][1:]] == [(12, 3), (3, 8, 3, 3)] * 2
    assert torch.equal(red[R0C2][1], f[f'{R0C2}.hada_w1_a'].t())
    assert tuple(red[Q2][1].shape) == (4, 5) and tuple(red[R1C1][2].shape) == (6, 36) and tuple(red[R1C2][2].shape) == (6, 4, 3, 3)
    assert tuple(red[K2][1].shape) == (1, 1) and float(red[K2][1]) == 1.0 and red[K2][2] is f[f'{K2}.diff']
    # malformed modules are errors of the file, not refusals
    for bad in ({f'{Q}.hada_w1_a': f[f'{K_}.hada_w1_a']}, {f'{Q}.lokr_w1': f[f'{V}.lokr_w1']},
                {f'{Q}.lora_up.weight': f[f'{Q}.lora_up.weight'], f'{Q}.diff': f[f'{K2}.diff']}):
        with pytest.raises(ValueError, match=Q):
            L.read_network(bad)


def test_entries_for_a_mixed_file_gives_all_three_kinds():
    from sdod.amd import lycoris as L
    f = _file()
    ent, skipped = L.entries_for(f, 'sd14', 0.8, 0.25)
    assert skipped == [] and len(ent['unet']) == 9 and len(ent['text']) == 1
    by_name = {(e[0] if len(e) == 4 else e[1]): e for e in ent['unet'] + ent['text']}
    assert set(by_name) == set(PARAM.values())
    kinds = {m: ('lora' if len(by_name[PARAM[m]]) == 4 else by_name[PARAM[m]][0]) for m in PARAM}
    assert kinds == {Q: 'lora', R0C1: 'lora', TE: 'lora', K_: 'loha', R0C2: 'loha', V: 'lokr', Q2: 'lokr', R1C1: 'lokr', R1C2: 'lokr', K2: 'lokr'}
    for m, (_, _, _, scale) in EXPECT.items():
        e = by_name[PARAM[m]]
        assert e[-1] == (0.25 if m == TE else 0.8) * scale and isinstance(e, tuple) and e.raw['scale'] == e[-1], m
        assert {7: 4, 5: 2, 4: 2}[len(e)] == sum(torch.is_tensor(x) for x in e)
    # the plain reader's behaviour is unchanged: it refuses what is not plain LoRA
    from sdod.amd import lora
    with pytest.raises(ValueError) as err:
        lora.entries_for(f, 'sd14')
    for m in (K_, R0C2, V, K2, R0C1):
        assert m in str(err.value)
    assert 'not a plain LoRA module' in str(err.value)
    # ... and what it returns is accepted here
    plain = {k: v for k, v in f.items() if k.startswith(Q + '.') or k.startswith(TE + '.')}
    via_lora, _ = L.entries_for(lora.read_lora(plain), 'sd14', 0.8, 0.25)
    direct, _ = L.entries_for(plain, 'sd14', 0.8, 0.25)
    assert [tuple(e[:1]) + (e[3],) for e in via_lora['unet'] + via_lora['text']] == [tuple(e[:1]) + (e[3],) for e in direct['unet'] + direct['text']]


def test_merged_state_dict_matches_an_independent_restatement():
    from sdod.amd import lycoris as L
    f, sd = _file(), _sd()
    sd['some.bias'] = torch.zeros(3)
    ent, _ = L.entries_for(f, 'sd14', 0.8, 0.25)
    # a second adapter on one weight, as a bare tuple: evaluated on the factors it carries
    extra = ('lokr', PARAM[V], f[f'{V}.lokr_w1'], f[f'{V}.lokr_w2'], -0.3)
    out = L.merged_state_dict(sd, ent['unet'] + ent['text'] + [extra])
    assert out['some.bias'] is sd['some.bias']
    for m, (_, _, _, scale) in EXPECT.items():
        w = sd[PARAM[m]]
        want = w.double() + (0.25 if m == TE else 0.8) * scale * _restated_delta(m, f).reshape(w.shape)
        if m == V:
            want = want - 0.3 * _kron(f[f'{V}.lokr_w1'], f[f'{V}.lokr_w2'])
        got = out[PARAM[m]]
        assert got.dtype == w.dtype and got.shape == w.shape
        # both sides are fp64 sums of the same terms in another order: 1e-12 relative to the largest term, then one rounding to fp32
        assert float((got.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max()), m
    with pytest.raises(KeyError):
        L.merged_state_dict(sd, [('lokr', 'nope.weight', f[f'{V}.lokr_w1'], f[f'{V}.lokr_w2'], 1.0)])
    with pytest.raises(ValueError):
        L.merged_state_dict(sd, [('lokr', PARAM[V], f[f'{V}.lokr_w1'], f[f'{V}.lokr_w2'][:5], 1.0)])
    with pytest.raises(ValueError):
        L.merged_state_dict(sd, [('loha', PARAM[K_], f[f'{K_}.hada_w1_a'], f[f'{K_}.hada_w1_b'], 1.0)])


def test_host_reductions_against_the_unreduced_definitions():
    """The device is handed b' = fp16(b_exact) (a Tucker core contracted into the b factor) or w' = fp16(w_exact) (a factored LoKr side
    multiplied out); a transposed or passed-through fp16 factor is exact.  One rounding to fp16 moves a value x by at most
    E(x) = 2^-11 |x| + 2^-25 (half an ulp in the normal range, half the subnormal step below it; nothing here overflows).  So, elementwise,
        low-rank product   P = a b':          |P - P_exact| <= T,  T = |a| E(b_exact)             (LoCon: delta = P)
        LoHa               delta = P1 * P2:   |delta - exact| <= T1 |P2_exact| + T2 |P1_exact| + T1 T2
        LoKr               delta = w1' (x) w2':  |delta - exact| <= E1 (x) |w2| + |w1| (x) E2 + E1 (x) E2,  E = 0 for a side the file holds
    all evaluated in fp64, whose own error (2^-53 per operation) is covered by the factor 1 + 1e-6."""
    from sdod.amd import lycoris as L
    f = _file(seed=3)
    net = L.read_network(f)
    slack = 1 + 1e-6
    E = lambda x: 2.0 ** -11 * x.abs() + 2.0 ** -25
    for m in (R0C1, R0C2, Q2, R1C1, R1C2):
        mod = net[m]
        exact = L.delta(mod['family'], mod['tensors'])
        red = L.reduce_module(mod)
        assert all(t.dtype == torch.float16 for t in red[1:])
        plain_entry = (PARAM[m], red[1], red[2], 1.0) if red[0] == 'lora' else (red[0], PARAM[m], *red[1:], 1.0)
        _, fam, tensors, _ = L._plain(plain_entry)
        got = L.delta(fam, tensors).reshape(exact.shape)
        t = {k: v.double() for k, v in mod['tensors'].items()}
        if m == R0C1:
            b_exact = _tucker(t['lora_mid.weight'], torch.eye(4, dtype=torch.float64), t['lora_down.weight'].reshape(4, 8)).reshape(4, -1)
            bound = (t['lora_up.weight'].reshape(12, 4).abs() @ E(b_exact)).reshape(exact.shape)
        elif m == R0C2:
            p, tt = [], []
            for side in ('1', '2'):
                b_exact = _tucker(t[f'hada_t{side}'], torch.eye(3, dtype=torch.float64), t[f'hada_w{side}_b']).reshape(3, -1)
                a = t[f'hada_w{side}_a'].t()
                p.append((a @ b_exact).reshape(exact.shape))
                tt.append((a.abs() @ E(b_exact)).reshape(exact.shape))
            bound = tt[0] * p[1].abs() + tt[1] * p[0].abs() + tt[0] * tt[1]
        else:
            w1, w2 = L._lokr_sides(mod['tensors'])
            e1 = torch.zeros_like(w1) if 'lokr_w1' in t else E(w1)
            e2 = torch.zeros_like(w2) if 'lokr_w2' in t else E(w2)
            k4 = lambda x, y: torch.kron(x[:, :, None, None] if y.dim() == 4 else x, y.contiguous())
            bound = (k4(e1, w2.abs()) + k4(w1.abs(), e2) + k4(e1, e2)).reshape(exact.shape)
        err = (got - exact).abs()
        assert bool((err <= bound * slack).all()), (m, float((err / bound.clamp_min(1e-300)).max()))
        assert float(err.max()) > 0, m        # the reduction did round something: the bound is not vacuous
        print(f'{m}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')


def test_refusals_name_the_module_and_strict_false_skips_them():
    from sdod.amd import lycoris as L
    z = lambda *s: torch.zeros(*s)
    f = {k: v for k, v in _file().items() if k.startswith(Q + '.')}
    dora, diffb, norm, lokr, temb = K_, V, Q2, K2, 'lora_unet_down_blocks_0_resnets_0_time_emb_proj'
    f.update({f'{dora}.lora_up.weight': z(24, 4), f'{dora}.lora_down.weight': z(4, 40), f'{dora}.dora_scale': z(1, 40),
              f'{diffb}.diff': z(24, 40), f'{diffb}.diff_b': z(24),
              f'{norm}.w_norm': z(24), f'{norm}.b_norm': z(24),
              f'{lokr}.lokr_w1': z(5, 4), f'{lokr}.lokr_w2': z(4, 10),           # 5 x 4 rows = 20, not the weight's 24
              f'{temb}.hada_w1_a': z(320, 4), f'{temb}.hada_w1_b': z(4, 1280), f'{temb}.hada_w2_a': z(320, 4), f'{temb}.hada_w2_b': z(4, 1280)})
    shapes = {'unet': {p: LIN for p in PARAM.values()}, 'text': {}}
    with pytest.raises(ValueError) as e:
        L.entries_for(f, 'sd14', shapes=shapes)
    msg = str(e.value)
    for m, word in ((dora, 'dora_scale'), (diffb, 'diff_b'), (norm, 'w_norm'), (lokr, 'do not divide'), (temb, 'TEMB')):
        assert any(m in line and word in line for line in msg.splitlines()), (m, word, msg)
    assert Q + ':' not in msg
    ent, skipped = L.entries_for(f, 'sd14', strict=False, shapes=shapes)
    assert sorted(skipped) == sorted([dora, diffb, norm, lokr, temb])
    assert [e[0] for e in ent['unet']] == [PARAM[Q]] and ent['text'] == []
    # a LoKr whose w1 divides the weight but whose w2 has the wrong size is refused as well; with the right one it is taken
    f2 = {f'{lokr}.lokr_w1': z(4, 5), f'{lokr}.lokr_w2': z(6, 7)}
    assert L.entries_for(f2, 'sd14', strict=False, shapes=shapes)[1] == [lokr]
    f2[f'{lokr}.lokr_w2'] = z(6, 8)
    assert L.entries_for(f2, 'sd14', shapes=shapes)[1] == []
    # text-encoder modules on the OpenCLIP tower stay refused
    with pytest.raises(ValueError, match='OpenCLIP'):
        L.entries_for({f'{TE}.hada_w1_a': z(8, 2), f'{TE}.hada_w1_b': z(2, 8), f'{TE}.hada_w2_a': z(8, 2), f'{TE}.hada_w2_b': z(2, 8)}, 'sd21')


@pytest.mark.parametrize('case', list(C.LOHA_CASES))
def test_loha_fp32_restatement_is_within_one_ulp(case):
    """The bound of tests/test_lycoris_kernel_gpu.py -- 1 fp16 ulp of fp16(fp64 result) -- is one the kernel's arithmetic itself meets:
    sequential fp32 accumulation of each product, the fp32 product of the two, the scale and the add, on exactly the GPU test's inputs.
    Worst 1 ulp in every case; 202 of 245 760 elements (320 x 768, rank 128) and at most 3 of 2 880 (40 x 72) are not bit-equal."""
    inp = C.loha_inputs(case)
    d = C.ulp_diff(C.loha_fp32_restatement(*inp, C.SCALE), C.loha_expected(*inp, C.SCALE))
    print(f'loha fp32 restatement {case}: {int((d != 0).sum())} of {d.numel()} elements not bit-equal, worst {int(d.max())} ulp')
    assert int(d.max()) <= 1
