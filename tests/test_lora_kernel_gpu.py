"""sdod_lora_merge_f16 (ops.lora_merge) against fp64 on the same fp16 inputs.

Expected value: fp16(W + scale * up . down) evaluated in fp64 and rounded once.  Bound: every element within 1 fp16 ulp of it.  The
kernel accumulates at most 128 exact fp16 x fp16 products in fp32 and adds W with one fma, an error far below half an fp16 ulp, so
an element can differ from the expected value only where the fp64 sum lies next to a rounding tie; the count of elements that are not
bit-equal is printed.  Shapes: the smallest that reach every map (identity, column block, GEGLU row interleave, KRSC columns), the
tile remainders in both directions (64 x 64 tiles: 40 x 72), an odd rank, the maximum rank, and more than one workgroup."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _inputs(n, k, rank, seed, down_shape=None):
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(n, k, generator=gen) * 0.05).half()
    up = (torch.randn(n, rank, generator=gen) * 0.2).half()
    down = (torch.randn(*(down_shape or (rank, k)), generator=gen) * 0.2).half()
    return w, up, down


def _expected(w, up, down, scale):
    """canonical [n, k] result: fp64 on the fp16 values, one rounding to fp16"""
    return (w.double() + float(scale) * (up.double() @ down.double().reshape(down.shape[0], -1))).half()


def _ulp_diff(a, b):
    """distance in fp16 steps between two finite fp16 tensors (sign-magnitude bits mapped to a monotone integer line)"""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def _check(got, want, what):
    got = got.cpu()
    assert torch.isfinite(got).all()
    d = _ulp_diff(got, want)
    print(f'lora_merge {what}: {int((d != 0).sum())} of {d.numel()} elements not bit-equal, worst {int(d.max())} ulp')
    assert int(d.max()) <= 1, int(d.max())


def geglu_pack(m):
    """rows of a canonical [2H, k] matrix in the engine's PK_LINEAR_GEGLU order: 16 value rows, then the 16 gate rows of the same block"""
    h = m.shape[0] // 2
    return torch.stack([m[:h].reshape(h // 16, 16, -1), m[h:].reshape(h // 16, 16, -1)], 1).reshape(m.shape)


def krsc_pack(m, cin):
    """columns of a canonical [n, cin * 9] matrix (j = c * 9 + t) in KRSC order (t * cin + c)"""
    return m.reshape(m.shape[0], cin, 9).permute(0, 2, 1).reshape(m.shape[0], 9 * cin).contiguous()


@pytest.mark.parametrize('rank', [1, 7, 16, 128])
def test_plain_with_tile_remainders(rank):
    from sdod.amd import ops
    w, up, down = _inputs(40, 72, rank, seed=rank)
    scale = 0.37
    got = ops.lora_merge(w.cuda(), up.cuda(), down.cuda(), scale)
    _check(got, _expected(w, up, down, scale), f'40x72 rank {rank}')


def test_plain_cross_attention_to_k_shape():
    from sdod.amd import ops
    w, up, down = _inputs(320, 768, 4, seed=3)
    got = ops.lora_merge(w.cuda(), up.cuda(), down.cuda(), -1.25)
    _check(got, _expected(w, up, down, -1.25), '320x768 rank 4')


def test_column_block_leaves_the_other_columns_alone():
    from sdod.amd import ops
    w, up, down = _inputs(320, 320, 8, seed=4)
    wide = (torch.randn(320, 960, generator=torch.Generator().manual_seed(40)) * 0.05).half()
    wide[:, 320:640] = w
    dev = wide.cuda()
    ops.lora_merge(dev[:, 320:640], up.cuda(), down.cuda(), 0.5)                 # the view brings ld = 960
    out = dev.cpu()
    _check(out[:, 320:640], _expected(w, up, down, 0.5), 'column block 320 of 960')
    assert torch.equal(out[:, :320], wide[:, :320]) and torch.equal(out[:, 640:], wide[:, 640:])
    dev2 = wide.cuda()
    ops.lora_merge(dev2.view(-1)[320:], up.cuda(), down.cuda(), 0.5, ld=960)       # the same through a flat pointer + explicit ld
    assert torch.equal(dev2, dev)


def test_geglu_interleave():
    from sdod.amd import ops
    w, up, down = _inputs(2560, 320, 16, seed=5)
    got = ops.lora_merge(geglu_pack(w).cuda(), up.cuda(), down.cuda(), 0.8, geglu=True)
    _check(got, geglu_pack(_expected(w, up, down, 0.8)), 'GEGLU 2560x320 rank 16')


@pytest.mark.parametrize('n,cin,rank', [(64, 32, 8), (320, 320, 4)])
def test_conv3x3_krsc(n, cin, rank):
    from sdod.amd import ops
    w, up, down = _inputs(n, 9 * cin, rank, seed=n, down_shape=(rank, cin, 3, 3))
    got = ops.lora_merge(krsc_pack(w, cin).cuda(), up.cuda(), down.cuda(), 0.6, conv_cin=cin)
    want = krsc_pack(_expected(w, up, down, 0.6), cin)
    assert not torch.equal(want, _expected(w, up, down, 0.6))                       # the map is not the identity on this data
    _check(got, want, f'conv3x3 {n}x{cin}x3x3 rank {rank}')


def test_zero_scale_keeps_the_bits_and_two_runs_agree():
    from sdod.amd import ops
    w, up, down = _inputs(40, 72, 7, seed=9)
    w[0, :8] = torch.tensor([-0.0, 0.0, 6e-8, -6e-8, 65504.0, -65504.0, 1.0, -1.0]).half()   # signed zeros, subnormals, the largest
    dev = w.cuda()
    ops.lora_merge(dev, up.cuda(), down.cuda(), 0.0)
    assert torch.equal(dev.view(torch.int16).cpu(), w.view(torch.int16))
    a = ops.lora_merge(w.cuda(), up.cuda(), down.cuda(), 0.3)
    b = ops.lora_merge(w.cuda(), up.cuda(), down.cuda(), 0.3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a.cpu(), w)


def test_argument_errors_leave_w_unchanged():
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    w, up, down = _inputs(40, 72, 4, seed=11)
    dev, upd, downd = w.cuda(), up.cuda(), down.cuda()
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device='cuda')
    bad = [
        lambda: ops.lora_merge(dev, z(40, 0), z(0, 72), 1.0),                          # rank 0
        lambda: ops.lora_merge(dev, z(40, 129), z(129, 72), 1.0),                      # rank 129
        lambda: ops.lora_merge(z(40, 36), z(40, 4), z(4, 36), 1.0),                    # k = 36
        lambda: ops.lora_merge(dev, upd, downd, 1.0, ld=64),                           # ld < k
        lambda: ops.lora_merge(dev, upd, downd, float('inf')),                         # scale
        lambda: ops.lora_merge(dev, upd, downd, float('nan')),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(SdodError) as e:
            call()
        assert e.value.code == 2, (i, e.value)
    buf = torch.zeros(40 * 72 + 8, dtype=torch.float16, device='cuda')
    buf[1:1 + 40 * 72] = dev.view(-1)
    with pytest.raises(SdodError) as e:
        ops.lora_merge(buf[1:1 + 40 * 72].view(40, 72), upd, downd, 1.0)                # base misaligned by 2 bytes
    assert e.value.code == 2
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), w) and torch.equal(buf[1:1 + 40 * 72].cpu(), w.view(-1))
