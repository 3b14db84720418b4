"""Canonical tensor -> weight-arena bytes, for every parameter of the smallest graphs that contain every packed form, bit for bit
against the plain packing reference of tests/weight_prep_ref.py (written from DESIGN.md 2 and include/sdod_engine.h, not from the
library's packer); then what finalize() makes of those bytes, against fp64.

Graphs (no evaluation is run; the widths are tests/test_engine_widths_gpu.py's):

  unet          model_channels 64, head_dim 64, context 128, 8x8 latent: KRSC convolutions, the 4-channel input convolution in rows
                of 64 halves, GEGLU weight and bias, out_layers.3 | skip_connection and ff.net.2 | proj_out (1x1 conv) column blocks
  unet_lin      the same with linear_proj: proj_in / proj_out packed as Linear
  unet_inpaint  the same with concat_channels 5: the 9-channel input convolution, rows of 128 halves
  temb          cond_proj_dim 48: time_embed.cond_proj.weight in rows padded to 64
  text0, text1  the text tower 128 wide in both dialects: embeddings, q | k | v groups, the fused in_proj
  vae_enc       vae_channels 64: the 3-channel input convolution, encoder.conv_out | quant_conv
  vae_dec       vae_channels 64: post_quant_conv kept in fp32

Every parameter param_table() lists is classified by weight_prep_ref.classify / column_blocks from its name and shape; one that has
no rule fails there.  Sources are fp32 and fp16 tensors with fp16 rounding ties, values next to 65504, subnormals, -0.0 and a value
below 2^-25 planted in every tensor (weight_prep_ref.F16_EDGES); round-to-nearest-even is the contract, torch's .half() the reference.

What finalize() changes, read from the builders (fold_jobs_ / compose_jobs_ in csrc/graphs.hip), and nothing else:

  * LayerNorm folds, W' = fp16(float(fp16(W)) * gamma) bit for bit: in every UNet transformer attn1.to_q / to_k / to_v by norm1,
    attn2.to_q by norm2, ff.net.0.proj by norm3; in every text layer q / k / v_proj (or attn.in_proj_weight) by layer_norm1 (ln_1) and
    mlp.fc1 (mlp.c_fc) by layer_norm2 (ln_2);
  * compositions, columns [0, k) of the owner's rows become P . W within the bound of tests/test_weight_prep_kernels_gpu.py against fp64
    of the fp16-rounded factors, P's own columns keep their bits: ff.net.2 | proj_out in every UNet transformer, encoder.conv_out |
    quant_conv in the VAE encoder;
  * every other parameter keeps the bits it had before finalize()."""
import pytest
import torch

import weight_prep_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def static_plan(monkeypatch):
    """finalize() times nothing: the static tile plan decides"""
    monkeypatch.setenv('SDOD_AUTOTUNE', '0')


def unet_config(**kw):
    from sdod.amd import engine as E
    cfg = E.sd14_config(8, 8, concat_channels=kw.pop('concat_channels', 0))
    cfg.model_channels, cfg.num_heads, cfg.head_dim, cfg.context_dim = 64, 0, 64, 128
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def make_graph(case, **kw):
    from sdod.amd import engine as E
    if case == 'unet':
        return E.UNet(unet_config(**kw), 1)
    if case == 'unet_lin':
        return E.UNet(unet_config(linear_proj=1), 1)
    if case == 'unet_inpaint':
        return E.UNet(unet_config(concat_channels=5), 1)
    if case == 'temb':
        return E.Temb(unet_config(), 1, cond_proj_dim=48)
    if case in ('text0', 'text1'):
        cfg = E.sd14_config(8, 8)
        cfg.context_dim, cfg.text_heads, cfg.text_layers, cfg.vocab_size, cfg.text_arch = 128, 2, 2, 1000, int(case[-1])
        return E.TextEncoder(cfg, 1)
    cfg = E.sd14_config(8, 8)
    cfg.vae_channels = 64
    return E.VaeEncoder(cfg, 1) if case == 'vae_enc' else E.VaeDecoder(cfg, 1)


CASES = ['unet', 'unet_lin', 'unet_inpaint', 'temb', 'text0', 'text1', 'vae_enc', 'vae_dec']
SEEDS = {c: 7000 + 10 * i for i, c in enumerate(CASES)}


def arena_of(g, name, dtype):
    """a set parameter's arena bytes on the host; a member of a column block (0 bytes) gives an empty tensor"""
    import ctypes
    n = ctypes.c_size_t()
    g._lib.sdod_graph_param_device(g._h, name.encode(), None, ctypes.byref(n))
    return g.packed_param(name, dtype).cpu() if n.value else torch.empty(0, dtype=dtype)


def compare_arena(g, table, ref, what, only=None):
    """every parameter's arena bytes against the reference image; returns how many were compared"""
    n = 0
    for name, _ in table:
        if only is not None and name not in only:
            continue
        want, dtype = ref[name]
        got = arena_of(g, name, dtype)
        assert got.numel() == want.numel(), f'{what}: {name} holds {got.numel()} elements of {dtype}, the reference {want.numel()}'
        if not torch.equal(R.bits(got), R.bits(want)):
            bad = (R.bits(got) != R.bits(want)).nonzero().flatten()
            i = int(bad[0])
            raise AssertionError(f'{what}: {name} differs from the packing reference in {bad.numel()} of {got.numel()} elements, first at flat '
                                 f'index {i}: arena {got[i].item()!r}, reference {want[i].item()!r}')
        n += 1
    return n


def check_block_shapes(g, table, quant=False):
    """the header's rules on sizes: a member of a column block reports 0 bytes, its owner rows of stride ld; tiny-Cin rows of 64 / 128"""
    blocks = R.column_blocks(table, quant)
    shapes = dict(table)
    for owner, (ld, members) in blocks.items():
        assert arena_of(g, owner, torch.float16).numel() == shapes[owner][0] * ld, owner
        for m, _, _ in members:
            if m != owner:
                assert arena_of(g, m, torch.float16).numel() == 0, m
    return blocks


# ------------------------------------------------------------------------------------------------ set_param -> arena
@pytest.mark.parametrize('case', CASES)
def test_arena_matches_packing_reference(case):
    """fp32 sources with every planted edge, then fp16 sources of other values over the same arena: every parameter, before finalize()"""
    g = make_graph(case)
    table = g.param_table()
    sd32 = R.planted_state_dict(table, SEEDS[case])
    g.load_state_dict(sd32)
    blocks = check_block_shapes(g, table)
    n = compare_arena(g, table, R.arena_ref(table, sd32), f'{case} fp32')
    sd16 = {k: v.half() for k, v in R.planted_state_dict(table, SEEDS[case] + 1).items()}
    g.load_state_dict(sd16)
    compare_arena(g, table, R.arena_ref(table, sd16), f'{case} fp16')
    kinds = sorted({R.classify(nm, sh) for nm, sh in table})
    print(f'arena {case}: {n} parameters, {len(blocks)} column blocks, forms {kinds}')
    assert n == len(table)
    want_kinds = {'unet': {'conv3', 'conv3_small', 'dense', 'geglu', 'vec', 'vec_geglu'}, 'vae_dec': {'mat_f32', 'conv3_small'}}.get(case, set())
    assert want_kinds <= set(kinds), kinds
    if case.startswith('unet'):
        row = R.small_conv_row(dict(table)['input_blocks.0.0.weight'][1])
        assert row == (128 if case == 'unet_inpaint' else 64) and g.packed_param('input_blocks.0.0.weight').numel() == 64 * row
        assert len(blocks) == 16 + 14        # every transformer's ff.net.2 | proj_out, every width-changing ResBlock's skip
        assert len(dict(table)['input_blocks.1.1.proj_out.weight']) == (2 if case == 'unet_lin' else 4)
    assert len(blocks) == {'temb': 1, 'vae_enc': 1}.get(case, len(blocks))


@pytest.mark.parametrize('case', ['unet', 'temb', 'vae_enc'])
def test_column_block_members_in_both_orders(case):
    """only the members of the column blocks are set: aliasing member first, then the owner; then each again with new values.  Neither
    disturbs the other, and the columns of the rows that nobody covers stay zero"""
    g = make_graph(case)
    table = g.param_table()
    blocks = R.column_blocks(table)
    assert blocks
    names = [m for _, (_, ms) in blocks.items() for m, _, _ in ms]
    sd_a = R.planted_state_dict(table, SEEDS[case] + 2)
    sd_b = R.planted_state_dict(table, SEEDS[case] + 3)
    for name in reversed(names):                       # members before owners
        g.set_param(name, sd_a[name])
    compare_arena(g, table, R.arena_ref(table, sd_a, only=set(blocks)), f'{case} members first', only=set(blocks))
    mixed = dict(sd_a)
    for owner in blocks:                                # new owners under the old members
        g.set_param(owner, sd_b[owner].half())
        mixed[owner] = sd_b[owner].half()
    compare_arena(g, table, R.arena_ref(table, mixed, only=set(blocks)), f'{case} owners again', only=set(blocks))
    for name in names:                                  # new members next to those owners
        if name not in blocks:
            g.set_param(name, sd_b[name])
            mixed[name] = sd_b[name]
    compare_arena(g, table, R.arena_ref(table, mixed, only=set(blocks)), f'{case} members again', only=set(blocks))
    if case == 'temb':                                  # 48 columns of 64: the padding is exactly zero
        rows = arena_of(g, 'time_embed.cond_proj.weight', torch.float16).view(64, 64)
        assert bool((R.bits(rows[:, 48:]) == 0).all())


# ------------------------------------------------------------------------------------------------ affine uint8 sources
U8_OFFSETS = [0, -128, -255]
U8_SCALES = [1e-4, 3e-3, 0.02, 0.4, (1 + 3 * 2.0 ** -11) * 2.0 ** -6]      # the last: (q + offset) = +-1 lands on an fp16 tie


def u8_state_dict(table, seed):
    from sdod.amd import weights as Wt
    gen = torch.Generator().manual_seed(seed)
    sd = R.planted_state_dict(table, seed)
    for i, (name, shape) in enumerate(table):
        if len(shape) < 2:
            continue
        q = torch.randint(0, 256, tuple(shape), generator=gen, dtype=torch.int32).to(torch.uint8)
        q.view(-1)[:6] = torch.tensor([1, 129, 254, 0, 255, 127], dtype=torch.uint8)[:q.numel()]
        sd[name] = Wt.QuantU8(q, U8_SCALES[i % len(U8_SCALES)], U8_OFFSETS[(i // len(U8_SCALES)) % len(U8_OFFSETS)])
    return sd


def test_u8q_sources_into_an_fp16_graph():
    """fp16(float32(float64(q + offset) * float64(scale))), in numpy: offsets 0, -128, -255, scales over four decades and one whose
    product with +-1 is an fp16 tie; all 15 (scale, offset) pairs occur"""
    g = make_graph('unet')
    table = g.param_table()
    sd = u8_state_dict(table, 7100)
    assert len({(v.scale, v.offset) for v in sd.values() if hasattr(v, 'payload')}) == 15
    tie = R.to_f16(sd[next(n for n, v in sd.items() if hasattr(v, 'payload') and v.scale == U8_SCALES[-1] and v.offset == 0)])
    assert tie.view(-1)[0].item() == (1 + 2.0 ** -9) * 2.0 ** -6        # q = 1: (1 + 3 * 2^-11) 2^-6 rounds to even, upwards
    g.load_state_dict(sd)
    assert compare_arena(g, table, R.arena_ref(table, sd), 'unet u8q -> fp16') == len(table)


def test_weight_quant_graph_keeps_repacked_codes():
    """weight_quant = 1: the codes in KRSC / GEGLU-interleaved / dense order, one byte each; vectors fp32 and the tiny-Cin input
    convolution fp16 as ever; no column blocks.  (Scale and offset rows: tests/test_engine_widths_gpu.py::test_w64_uint8_weights.)"""
    from sdod.amd import _lib, weights as Wt
    g = make_graph('unet', weight_quant=1)
    table = g.param_table()
    sd = Wt.quantize_state_dict(R.planted_state_dict(table, 7200, R.F16_EDGES_SMALL))
    g.load_state_dict(sd)
    assert check_block_shapes(g, table, quant=True) == {}
    ref = R.arena_ref(table, sd, quant=True)
    assert compare_arena(g, table, ref, 'unet weight_quant') == len(table)
    assert sum(dt == torch.uint8 for _, dt in ref.values()) > 200
    # refusals: the parameter keeps its bytes
    name = 'input_blocks.1.0.in_layers.2.weight'
    before = arena_of(g, name, torch.uint8).clone()
    for bad in (Wt.QuantU8(sd[name].q, sd[name].scale, -1025), Wt.QuantU8(sd[name].q, sd[name].scale, 1), sd[name].dequantize().half()):
        with pytest.raises(_lib.SdodError):
            g.set_param(name, bad)
        assert torch.equal(arena_of(g, name, torch.uint8), before), 'a refused set_param changed the arena'


# ------------------------------------------------------------------------------------------------ load_file against load_state_dict
@pytest.mark.parametrize('case', ['unet', 'temb', 'text0', 'vae_enc', 'vae_dec'])
def test_load_file_equals_load_state_dict(case, tmp_path):
    from sdod.amd import weights as Wt
    a, b = make_graph(case), make_graph(case)
    table = a.param_table()
    sd = R.planted_state_dict(table, SEEDS[case] + 4)
    for i, (name, shape) in enumerate(table):           # fp32, fp16 and affine-uint8 payloads mixed
        if i % 3 == 1:
            sd[name] = sd[name].half()
        elif i % 3 == 2 and len(shape) >= 2:
            sd[name] = Wt.quantize_u8(sd[name].clamp(-4, 4))
    path = str(tmp_path / f'{case}.sdodw')
    Wt.save(path, {'model.' + k: v for k, v in sd.items()})
    a.load_state_dict(sd)
    b.load_file(path, prefix='model.')
    ref = R.arena_ref(table, sd)
    for name, _ in table:
        dtype = ref[name][1]
        assert torch.equal(R.bits(arena_of(a, name, dtype)), R.bits(arena_of(b, name, dtype))), f'{case}: {name} differs between the two paths'
    compare_arena(b, table, ref, f'{case} load_file')


# ------------------------------------------------------------------------------------------------ finalize()
def fold_gamma(case, name):
    """the LayerNorm weight finalize() multiplies into parameter `name`, or None (the rule of the module docstring)"""
    if case.startswith('unet') and '.transformer_blocks.0.' in name:
        tb, leaf = name.split('.transformer_blocks.0.')
        norm = {'attn1.to_q.weight': 'norm1', 'attn1.to_k.weight': 'norm1', 'attn1.to_v.weight': 'norm1', 'attn2.to_q.weight': 'norm2',
                'ff.net.0.proj.weight': 'norm3'}.get(leaf)
        return None if norm is None else f'{tb}.transformer_blocks.0.{norm}.weight'
    if case == 'text0':
        for leaf, norm in (('.self_attn.q_proj.weight', 'layer_norm1'), ('.self_attn.k_proj.weight', 'layer_norm1'),
                           ('.self_attn.v_proj.weight', 'layer_norm1'), ('.mlp.fc1.weight', 'layer_norm2')):
            if name.endswith(leaf):
                return name[:-len(leaf)] + f'.{norm}.weight'
    if case == 'text1':
        for leaf, norm in (('.attn.in_proj_weight', 'ln_1'), ('.mlp.c_fc.weight', 'ln_2')):
            if name.endswith(leaf):
                return name[:-len(leaf)] + f'.{norm}.weight'
    return None


COMPOSED = {'unet': '.ff.net.2.weight', 'unet_lin': '.ff.net.2.weight', 'unet_inpaint': '.ff.net.2.weight', 'vae_enc': 'encoder.conv_out.weight'}


@pytest.mark.parametrize('case', ['unet', 'unet_lin', 'text0', 'text1', 'vae_enc', 'vae_dec', 'temb'])
def test_finalize_folds_composes_and_leaves_the_rest(case):
    from sdod.amd import _lib
    g = make_graph(case)
    table = g.param_table()
    sd = R.planted_state_dict(table, SEEDS[case] + 5, R.F16_EDGES_SMALL)
    sd = {k: (v.half() if i % 2 else v) for i, (k, v) in enumerate(sd.items())}
    g.load_state_dict(sd)
    pre = R.arena_ref(table, sd)
    compare_arena(g, table, pre, f'{case} before finalize')
    blocks = R.column_blocks(table)
    g.finalize()
    torch.cuda.synchronize()
    folded = composed = same = 0
    worst = 0.0
    for name, shape in table:
        want, dtype = pre[name]
        got = arena_of(g, name, dtype)
        gamma = fold_gamma(case, name)
        if gamma is not None:
            assert name not in blocks
            w = want.view(shape[0], -1)
            want = (w.float() * R.to_f32(sd[gamma])).half().reshape(-1)      # (the GEGLU interleave moves rows; gamma runs along a row)
            assert torch.equal(R.bits(got), R.bits(want)), f'{case}: {name} is not fp16(float(fp16(W)) * gamma) after finalize'
            folded += 1
        elif name in blocks and name.endswith(COMPOSED.get(case, '\0')):
            ld, ((_, _, k), (_, pcol, n_mid)) = blocks[name]
            rows, now = want.view(shape[0], ld), got.view(shape[0], ld)
            p, w = rows[:, pcol:pcol + n_mid], rows[:, :k]
            assert torch.equal(R.bits(now[:, k:]), R.bits(rows[:, k:])), f'{case}: {name}: the P block changed in finalize'
            ref, mag, _, _ = R.compose_ref(p, w)
            r = R.worst_ratio(now[:, :k], ref, R.compose_bound(ref, mag, n_mid))
            worst = max(worst, r)
            assert r <= 1, f'{case}: {name}: composed block {r:.3f} of the bound'
            composed += 1
        else:
            assert torch.equal(R.bits(got), R.bits(want)), f'{case}: {name} takes part in no fold and changed in finalize'
            same += 1
    print(f'finalize {case}: {folded} folded, {composed} composed (worst {worst:.3f} of the bound), {same} unchanged')
    assert (folded, composed) == {'unet': (80, 16), 'unet_lin': (80, 16), 'text0': (8, 0), 'text1': (4, 0), 'vae_enc': (0, 1)}.get(case, (0, 0))
    # parameters cannot change any more, and a refused set_param leaves the arena as it is
    name = table[0][0]
    before = arena_of(g, name, pre[name][1]).clone()
    with pytest.raises(_lib.SdodError, match='parameters cannot change after finalize'):
        g.set_param(name, torch.zeros(table[0][1]))
    assert torch.equal(R.bits(arena_of(g, name, pre[name][1])), R.bits(before))
