"""Plain references of the weight-preparation stage, for tests/test_weight_prep_kernels_gpu.py and tests/test_weight_arena_gpu.py:
what set_param leaves in a graph's weight arena (the packing maps of DESIGN.md 2 and of include/sdod_engine.h at
sdod_graph_param_device, written from those texts), and what finalize() turns it into (sdod_ln_fold_f16, sdod_compose_linear_f16).
Everything here is torch / numpy on the CPU; nothing reads the library.

The packed forms, canonical PyTorch tensor -> arena bytes:

  3x3 convolution [Cout][Cin][3][3]    fp16 [Cout][t * Cin + c], t = 3 r + s (KRSC)
  ... with 9 Cin <= 96 (tiny Cin)      the same order in rows of 64 halves (9 Cin <= 64) or 128, the rest of a row exactly zero
  1x1 convolution, Linear, embedding   fp16 [out][in], dense
  ff.net.0.proj (GEGLU) weight, bias   value row j -> (j // 16) * 32 + j % 16, gate row j -> the same + 16; weight fp16, bias fp32
  every other vector                   fp32
  post_quant_conv.weight               fp32, dense (the 4 x 4 matrix the latent-prep kernel reads)
  column blocks                        two parameters side by side in rows of stride ld (column_blocks() below); the second reports 0 bytes
  weight_quant graphs                  3x3 / 1x1 / Linear / GEGLU weights stay uint8 CODES in the same order, one byte each, no column blocks

fp32 -> fp16 is round-to-nearest-even (torch's .half()); an affine-uint8 tensor offered to an fp16 parameter becomes
fp16(float32(float64(q + offset) * float64(scale)))."""
import numpy as np
import torch

SENTINEL = 0x3A5D          # the suite's frame pattern (tests/gemm_cases.py): fp16 bits of 0.7955
SENTINEL32 = 0x7FC0BEEF    # fp32 frame pattern: a NaN with a payload no kernel produces


# ------------------------------------------------------------------------------------------------ the two finalize kernels
def compose_ref(p, w, bias_w=None, bias_p=None):
    """fp64 reference of sdod_compose_linear_f16 on fp16 factors p [n_out][n_mid], w [n_mid][k]: (c, sum_j |p w|, bias, its magnitude)"""
    P, W = p.double(), w.double()
    c, mag = P @ W, P.abs() @ W.abs()
    n_out = p.shape[0]
    bw = torch.zeros(p.shape[1], dtype=torch.float64) if bias_w is None else bias_w.double()
    bp = torch.zeros(n_out, dtype=torch.float64) if bias_p is None else bias_p.double()
    return c, mag, P @ bw + bp, P.abs() @ bw.abs() + bp.abs()


def compose_bound(ref, mag, n_mid):
    """one fp16 rounding (half an ulp of a normal value, or half the subnormal spacing) on top of sequential fp32 accumulation of
    n_mid terms (the standard bound, with a factor 2 of slack): the kernel's contract, not a measurement"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25 + n_mid * 2.0 ** -23 * mag


def compose_bias_bound(bias_mag, n_mid):
    return (n_mid + 1) * 2.0 ** -23 * bias_mag


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (<= 1 passes); a non-finite `got` is infinitely wrong"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(got.double()), err, torch.full_like(err, float('inf')))
    return float((err / bound).max())


def compose_wrong_fp16_accumulate(p, w):
    """a WRONG kernel: the running sum kept in fp16"""
    acc = torch.zeros(p.shape[0], w.shape[1], dtype=torch.float16)
    for j in range(p.shape[1]):
        acc = (acc.float() + p[:, j:j + 1].float() * w[j:j + 1].float()).half()
    return acc


def compose_wrong_fp16_products(p, w):
    """a WRONG kernel: fp32 accumulation of products that were each rounded to fp16"""
    acc = torch.zeros(p.shape[0], w.shape[1], dtype=torch.float32)
    for j in range(p.shape[1]):
        acc += (p[:, j:j + 1].float() * w[j:j + 1].float()).half().float()
    return acc.half()


def compose_like_kernel(p, w):
    """the contract itself on the CPU: sequential fp32 accumulation, one fp16 rounding"""
    acc = torch.zeros(p.shape[0], w.shape[1], dtype=torch.float32)
    for j in range(p.shape[1]):
        acc += p[:, j:j + 1].float() * w[j:j + 1].float()
    return acc.half()


def ln_fold_ref(w, gamma, beta, bias=None):
    """sdod_ln_fold_f16 on fp16 w [n][k]: W' bit for bit (one fp32 product, one rounding), then fp64 (s, its bound, t, its bound)"""
    k = w.shape[1]
    wf = (w.float() * gamma.float()).half()
    s, s_tol = wf.double().sum(1), k * 2.0 ** -23 * wf.double().abs().sum(1)
    bw = w.double() * beta.double()
    b = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    return wf, s, s_tol, bw.sum(1) + b, (k + 1) * 2.0 ** -23 * (bw.abs().sum(1) + b.abs())


# ------------------------------------------------------------------------------------------------ the packing maps
def geglu_rows(n):
    """destination row of canonical row r of a [2H] GEGLU projection: value j -> (j // 16) * 32 + j % 16, gate j -> that + 16"""
    h = n // 2
    assert n % 32 == 0
    j = torch.arange(n) % h
    return (j // 16) * 32 + j % 16 + 16 * (torch.arange(n) >= h)


def small_conv_row(cin):
    """halves per row of a tiny-Cin 3x3 convolution"""
    assert 9 * cin <= 96
    return 64 if 9 * cin <= 64 else 128


def classify(name, shape):
    """the packed form of a parameter, from its name and canonical shape alone; an unknown combination is an error, never a default"""
    shape = tuple(shape)
    if len(shape) == 1:
        return 'vec_geglu' if name.endswith('.ff.net.0.proj.bias') else 'vec'
    if len(shape) == 4 and shape[2:] == (3, 3):
        return 'conv3_small' if 9 * shape[1] <= 96 else 'conv3'
    if len(shape) == 4 and shape[2:] == (1, 1):
        return 'mat_f32' if name == 'post_quant_conv.weight' else 'dense'
    if len(shape) == 2:
        return 'geglu' if name.endswith('.ff.net.0.proj.weight') else 'dense'
    raise AssertionError(f'no packing rule for parameter {name} of shape {shape}')


CODE_KINDS = ('conv3', 'dense', 'geglu')      # what a weight_quant graph keeps as uint8 codes (embeddings: no such graph has one)


def pack_values(kind, t):
    """the DENSE packed image of canonical tensor `t` (any dtype: the map only moves elements), 2-D [rows][row length] or 1-D"""
    if kind in ('vec', 'mat_f32'):
        return t.reshape(-1)
    if kind == 'vec_geglu':
        out = torch.empty_like(t)
        out[geglu_rows(t.shape[0])] = t
        return out
    if kind == 'dense':
        return t.reshape(t.shape[0], -1)
    if kind == 'geglu':
        out = torch.empty_like(t)
        out[geglu_rows(t.shape[0])] = t
        return out
    co, ci = t.shape[:2]
    krsc = t.reshape(co, ci, 9).permute(0, 2, 1).reshape(co, 9 * ci)          # [o][t * ci + c]
    if kind == 'conv3':
        return krsc
    assert kind == 'conv3_small', kind
    out = torch.zeros(co, small_conv_row(ci), dtype=t.dtype)
    out[:, :9 * ci] = krsc
    return out


def to_f16(t):
    """what the arena holds of a canonical fp32 / fp16 tensor or of a weights.QuantU8: round to nearest even, once"""
    if hasattr(t, 'payload'):
        q = t.q.numpy().astype(np.float64) + np.float64(t.offset)
        real = (q * np.float64(np.float32(t.scale))).astype(np.float32)
        return torch.from_numpy(real.astype(np.float16))
    return t.half()


def to_f32(t):
    if hasattr(t, 'payload'):
        q = t.q.numpy().astype(np.float64) + np.float64(t.offset)
        return torch.from_numpy((q * np.float64(np.float32(t.scale))).astype(np.float32))
    return t.float()


def packed_ref(name, t, quant_codes=False):
    """(dense packed image, torch dtype of the arena) of the canonical tensor / QuantU8 `t` set into parameter `name`"""
    kind = classify(name, tuple(t.shape))
    if quant_codes and kind in CODE_KINDS:
        assert hasattr(t, 'payload'), name
        return pack_values(kind, t.q), torch.uint8
    if kind in ('vec', 'vec_geglu', 'mat_f32'):
        return pack_values(kind, to_f32(t)), torch.float32
    return pack_values(kind, to_f16(t)), torch.float16


def column_blocks(table, quant=False):
    """{owner: (ld, [(member, first column, columns)])} of a graph's parameter table: the parameters that share rows of a wider matrix.
      out_layers.3.weight | skip_connection.weight       ResBlocks that change width: [cout][9 cout + cin]
      ff.net.2.weight | proj_out.weight                  every transformer: [C][4C + C]
      encoder.conv_out.weight | quant_conv.weight        the VAE encoder: [8][9 ch + 8]
      time_embed.cond_proj.weight                        alone, rows padded to the next multiple of 64
    None of them in a weight_quant graph (a tensor's codes carry their own encoding)."""
    shapes = dict(table)
    out = {}
    if quant:
        return out
    for name, shape in table:
        if name.endswith('.skip_connection.weight'):
            owner = name[:-len('skip_connection.weight')] + 'out_layers.3.weight'
            cout, cin = shape[:2]
            assert shapes[owner] == (cout, cout, 3, 3), (owner, shapes[owner])
            out[owner] = (9 * cout + cin, [(owner, 0, 9 * cout), (name, 9 * cout, cin)])
        elif name.endswith('.transformer_blocks.0.ff.net.2.weight'):
            member = name[:-len('transformer_blocks.0.ff.net.2.weight')] + 'proj_out.weight'
            c = shape[0]
            assert shape == (c, 4 * c) and shapes[member][:2] == (c, c), (name, shape, shapes[member])
            out[name] = (5 * c, [(name, 0, 4 * c), (member, 4 * c, c)])
        elif name == 'quant_conv.weight':
            owner = 'encoder.conv_out.weight'
            zc, ch = shapes[owner][:2]
            out[owner] = (9 * ch + zc, [(owner, 0, 9 * ch), (name, 9 * ch, zc)])
        elif name == 'time_embed.cond_proj.weight' and shape[1] % 64:
            out[name] = ((shape[1] + 63) // 64 * 64, [(name, 0, shape[1])])
    return out


def arena_ref(table, sd, quant=False, only=None):
    """{name: (expected flat arena image, dtype)} for every parameter of `table` that reports bytes; members of a column block are laid
    into their owner's rows (zeros in the columns nobody covers, the arena being zeroed at allocation) and report an empty image"""
    blocks = column_blocks(table, quant)
    member_of = {m: o for o, (_, ms) in blocks.items() for m, _, _ in ms}
    out = {}
    for name, shape in table:
        if only is not None and name not in only:
            continue
        if name in member_of and member_of[name] != name:
            out[name] = (torch.empty(0, dtype=torch.float16), torch.float16)
            continue
        if name in blocks:
            ld, members = blocks[name]
            rows = torch.zeros(shape[0], ld, dtype=torch.float16)
            for m, col, width in members:
                img, dt = packed_ref(m, sd[m])
                assert dt == torch.float16 and tuple(img.shape) == (shape[0], width), (m, img.shape)
                rows[:, col:col + width] = img
            out[name] = (rows.reshape(-1), torch.float16)
            continue
        img, dt = packed_ref(name, sd[name], quant)
        out[name] = (img.reshape(-1), dt)
    return out


def bits(t):
    """integer view for bit-for-bit comparison (NaN, -0.0 and subnormals compare as they are stored)"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


# ------------------------------------------------------------------------------------------------ seeded tensors with planted edges
F16_EDGES = [
    1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,        # ties: to even is 1.0 and 1 + 2^-9; truncation gives 1.0 and 1 + 2^-10, half-up 1 + 2^-10 and 1 + 2^-9
    65503.0, 65519.0,                          # just under 65504 (-> 65504) and just over (below the tie at 65520: still 65504, never inf)
    2.0 ** -24 * 3, 2.0 ** -24 * 2.5,          # an fp16 subnormal, and a tie between two of them (-> 2 * 2^-24)
    -0.0, 2.0 ** -26,                          # keeps its sign bit; below half the smallest subnormal: +0
    -(1 + 2.0 ** -11), 2.0 ** -25 * 1.0001,    # the tie mirrored; just above half the smallest subnormal: 2^-24, not 0
]


F16_EDGES_SMALL = [e for e in F16_EDGES if abs(e) < 4]     # for what finalize multiplies: nothing that overflows fp16 afterwards


def planted_state_dict(table, seed, edges=F16_EDGES):
    """fp32 canonical tensors: weights.synthetic_state_dict's scales from one generator, with `edges` written over the first
    elements of every tensor and again at its end (rotated by the tensor's index, so tensors shorter than the list see all of them)"""
    gen = torch.Generator().manual_seed(seed)
    edges = torch.tensor(edges, dtype=torch.float32)
    sd = {}
    for i, (name, shape) in enumerate(table):
        shape = tuple(int(d) for d in shape)
        x = torch.randn(shape, generator=gen)
        if len(shape) >= 2:
            x.mul_(float(np.prod(shape[1:])) ** -0.5)
        elif name.endswith('weight'):
            x.mul_(0.1).add_(1.0)
        else:
            x.mul_(0.1)
        flat = x.view(-1)
        e = edges.roll(i)[:min(len(edges), flat.numel())]
        flat[:e.numel()] = e
        flat[flat.numel() - e.numel():] = e.flip(0)
        sd[name] = x
    return sd
