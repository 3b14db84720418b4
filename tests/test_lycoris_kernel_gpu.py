"""sdod_loha_merge_f16 / sdod_lokr_merge_f16 (ops.loha_merge, ops.lokr_merge) against fp64 on the same fp16 inputs.

Expected value: the family's definition evaluated in fp64 and rounded to fp16 once.  Bound: every element within 1 fp16 ulp of it.
LoHa: tests/test_lycoris_cpu.py::test_loha_fp32_restatement_is_within_one_ulp shows on these very inputs that sequential fp32
accumulation, the fp32 product, the scale and the add stay within that bound (the MFMA sums the same exact products in fp32 in another
grouping).  LoKr: the fp16 x fp16 product is exact in fp32 and the update is one fma, so an element can differ only where the fp32
rounding of the sum in front of the fp16 one crosses a tie.  The count of elements that are not bit-equal is printed.
Shapes (tests/lycoris_cases.py): the smallest that reach every map -- identity, column block, GEGLU row interleave, KRSC columns --
with tile remainders in both directions (40 x 72 against 64 x 64 tiles), ranks 1 / odd / half a K step / the maximum, Kronecker splits
whose d is no multiple of 8 and whose c no multiple of 16, and more than one workgroup."""
import pytest
import torch

import lycoris_cases as C

pytestmark = pytest.mark.gpu


def _check(got, want, what):
    got = got.cpu()
    assert torch.isfinite(got).all()
    d = C.ulp_diff(got, want)
    print(f'{what}: {int((d != 0).sum())} of {d.numel()} elements not bit-equal, worst {int(d.max())} ulp')
    assert int(d.max()) <= 1, int(d.max())


def _cuda(*ts):
    return [t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------------------------------------------ LoHa
@pytest.mark.parametrize('case', ['plain_r1', 'plain_r7', 'plain_r16', 'plain_r128', 'wide_r128'])
def test_loha_plain_with_tile_remainders(case):
    from sdod.amd import ops
    w, *f = C.loha_inputs(case)
    got = ops.loha_merge(w.cuda(), *_cuda(*f), C.SCALE)
    _check(got, C.loha_expected(w, *f, C.SCALE), f'loha_merge {case} {tuple(w.shape)} rank {f[0].shape[1]}')


def test_loha_column_block_leaves_the_other_columns_alone():
    from sdod.amd import ops
    w, *f = C.loha_inputs('block')
    wide = (torch.randn(72, 960, generator=torch.Generator().manual_seed(40)) * 0.05).half()
    wide[:, 320:640] = w
    dev = wide.cuda()
    ops.loha_merge(dev[:, 320:640], *_cuda(*f), C.SCALE)                          # the view brings ld = 960
    out = dev.cpu()
    _check(out[:, 320:640], C.loha_expected(w, *f, C.SCALE), 'loha_merge column block 320 of 960')
    assert torch.equal(out[:, :320], wide[:, :320]) and torch.equal(out[:, 640:], wide[:, 640:])
    dev2 = wide.cuda()
    ops.loha_merge(dev2.view(-1)[320:], *_cuda(*f), C.SCALE, ld=960)                # the same through a flat pointer + explicit ld
    assert torch.equal(dev2, dev)


def test_loha_geglu_interleave():
    from sdod.amd import ops
    w, *f = C.loha_inputs('geglu')
    got = ops.loha_merge(C.geglu_pack(w).cuda(), *_cuda(*f), C.SCALE, geglu=True)
    want = C.loha_expected(w, *f, C.SCALE)
    assert not torch.equal(C.geglu_pack(want), want)
    _check(got, C.geglu_pack(want), 'loha_merge GEGLU 64x72 rank 16')


def test_loha_conv3x3_krsc():
    from sdod.amd import ops
    w, *f = C.loha_inputs('conv')
    got = ops.loha_merge(C.krsc_pack(w, 32).cuda(), *_cuda(*f), C.SCALE, conv_cin=32)
    want = C.loha_expected(w, *f, C.SCALE)
    assert not torch.equal(C.krsc_pack(want, 32), want)                            # the map is not the identity on this data
    _check(got, C.krsc_pack(want, 32), 'loha_merge conv3x3 64x32x3x3 rank 8')


# ------------------------------------------------------------------------------------------------------------------------------ LoKr
@pytest.mark.parametrize('a,b', [(1, 1), (5, 9), (8, 8), (40, 72)])
def test_lokr_plain(a, b):
    """(5, 9): d = 8, c = 8 (a wave's 16 rows straddle w1 rows); (8, 8): d = 9, a lane's 8 columns straddle a w1 column, c = 5;
    (40, 72): w2 is 1 x 1; (1, 1): a full delta"""
    from sdod.amd import ops
    w, w1, w2 = C.lokr_inputs(40, 72, a, b, seed=10 * a + b)
    got = ops.lokr_merge(w.cuda(), w1.cuda(), w2.cuda(), C.SCALE)
    _check(got, C.lokr_expected(w, w1, w2, C.SCALE), f'lokr_merge 40x72 w1 {a}x{b}')


@pytest.mark.parametrize('a,b', [(4, 4), (2, 8), (1, 1)])
def test_lokr_conv3x3_krsc(a, b):
    from sdod.amd import ops
    w, w1, w2 = C.lokr_inputs(64, 32, a, b, seed=100 + 10 * a + b, taps=9)
    got = ops.lokr_merge(C.krsc_pack(w, 32).cuda(), w1.cuda(), w2.cuda(), C.SCALE, conv_cin=32)
    want = C.lokr_expected(w, w1, w2, C.SCALE)
    assert not torch.equal(C.krsc_pack(want, 32), want)
    _check(got, C.krsc_pack(want, 32), f'lokr_merge conv3x3 64x32x3x3 w1 {a}x{b}')


def test_lokr_geglu_splits_the_canonical_row():
    """a = 4 over 64 rows: c = 16.  Packed rows 16 .. 31 are the canonical gate rows 32 .. 47: splitting the PACKED row would give them
    w1 row 1 where the definition has row 2, so the two results differ on this data and only the canonical one may pass."""
    from sdod.amd import ops
    w, w1, w2 = C.lokr_inputs(64, 72, 4, 3, seed=21)
    got = ops.lokr_merge(C.geglu_pack(w).cuda(), w1.cuda(), w2.cuda(), C.SCALE, geglu=True)
    want = C.geglu_pack(C.lokr_expected(w, w1, w2, C.SCALE))
    wrong = C.lokr_expected(C.geglu_pack(w), w1, w2, C.SCALE)                       # the Kronecker split applied to the packed row
    assert int(C.ulp_diff(wrong, want).max()) > 1
    _check(got, want, 'lokr_merge GEGLU 64x72 w1 4x3')


def test_lokr_column_block_leaves_the_other_columns_alone():
    from sdod.amd import ops
    w, w1, w2 = C.lokr_inputs(72, 320, 9, 64, seed=22)                              # d = 5
    wide = (torch.randn(72, 960, generator=torch.Generator().manual_seed(41)) * 0.05).half()
    wide[:, 320:640] = w
    dev = wide.cuda()
    ops.lokr_merge(dev[:, 320:640], w1.cuda(), w2.cuda(), C.SCALE)
    out = dev.cpu()
    _check(out[:, 320:640], C.lokr_expected(w, w1, w2, C.SCALE), 'lokr_merge column block 320 of 960')
    assert torch.equal(out[:, :320], wide[:, :320]) and torch.equal(out[:, 640:], wide[:, 640:])
    dev2 = wide.cuda()
    ops.lokr_merge(dev2.view(-1)[320:], w1.cuda(), w2.cuda(), C.SCALE, ld=960)
    assert torch.equal(dev2, dev)


# ------------------------------------------------------------------------------------------------------------------------------ both
SPECIALS = [-0.0, 0.0, 6e-8, -6e-8, 65504.0, -65504.0, 1.0, -1.0]                   # signed zeros, subnormals, the largest


def test_zero_scale_keeps_the_bits_and_two_runs_agree():
    from sdod.amd import ops
    w, *f = C.loha_inputs('plain_r7')
    w[0, :8] = torch.tensor(SPECIALS).half()
    dev = w.cuda()
    ops.loha_merge(dev, *_cuda(*f), 0.0)
    assert torch.equal(dev.view(torch.int16).cpu(), w.view(torch.int16))
    a = ops.loha_merge(w.cuda(), *_cuda(*f), 0.3)
    b = ops.loha_merge(w.cuda(), *_cuda(*f), 0.3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a.cpu(), w)
    w, w1, w2 = C.lokr_inputs(40, 72, 8, 8, seed=23)
    w[0, :8] = torch.tensor(SPECIALS).half()
    dev = w.cuda()
    ops.lokr_merge(dev, w1.cuda(), w2.cuda(), 0.0)
    assert torch.equal(dev.view(torch.int16).cpu(), w.view(torch.int16))
    a = ops.lokr_merge(w.cuda(), w1.cuda(), w2.cuda(), 0.3)
    b = ops.lokr_merge(w.cuda(), w1.cuda(), w2.cuda(), 0.3)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a.cpu(), w)


def test_argument_errors_leave_w_unchanged():
    from sdod.amd import _lib, ops
    from sdod.amd._lib import SdodError
    w, *f = C.loha_inputs('plain_r7')
    dev, fd = w.cuda(), _cuda(*f)
    _, w1, w2 = C.lokr_inputs(40, 72, 8, 8, seed=23)
    w1d, w2d = w1.cuda(), w2.cuda()
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device='cuda')
    lib, P = _lib.hip(), lambda t: t.data_ptr()
    raw = _lib.check                                                                                # status code -> SdodError
    bad = [
        lambda: ops.loha_merge(dev, z(40, 0), z(0, 72), z(40, 0), z(0, 72), 1.0),                  # rank 0
        lambda: ops.loha_merge(dev, z(40, 129), z(129, 72), z(40, 129), z(129, 72), 1.0),          # rank 129
        lambda: ops.loha_merge(z(40, 36), z(40, 4), z(4, 36), z(40, 4), z(4, 36), 1.0),            # k = 36
        lambda: ops.loha_merge(dev, *fd, 1.0, ld=64),                                              # ld < k
        lambda: ops.loha_merge(dev, *fd, 1.0, ld=76),                                              # ld % 8
        lambda: ops.loha_merge(dev, *fd, float('inf')),
        lambda: ops.loha_merge(dev, *fd, float('nan')),
        lambda: ops.loha_merge(dev, *fd, 1.0, conv_cin=16),                                        # k != 9 cin
        lambda: ops.loha_merge(dev, *fd, 1.0, geglu=True),                                         # n % 32
        lambda: raw(lib.sdod_loha_merge_f16(P(dev), 40, 72, 72, P(fd[0]), P(fd[1]), P(fd[2]), None, 7, 1.0, 0, 0, None)),   # null factor
        lambda: ops.lokr_merge(dev, w1d, w2d, 1.0, ld=64),
        lambda: ops.lokr_merge(dev, w1d, w2d, float('inf')),
        lambda: ops.lokr_merge(dev, w1d, w2d, float('nan')),
        lambda: ops.lokr_merge(dev, w1d, w2d, 1.0, conv_cin=16),
        lambda: ops.lokr_merge(dev, w1d, w2d, 1.0, geglu=True),
        lambda: ops.lokr_merge(z(40, 36), z(4, 4), z(10, 9), 1.0),                                 # k = 36
        lambda: raw(lib.sdod_lokr_merge_f16(P(dev), 40, 72, 72, P(w1d), 3, 8, P(w2d), 1.0, 0, 0, None)),    # a does not divide n
        lambda: raw(lib.sdod_lokr_merge_f16(P(dev), 40, 72, 72, P(w1d), 8, 7, P(w2d), 1.0, 0, 0, None)),    # b does not divide k
        lambda: raw(lib.sdod_lokr_merge_f16(P(dev), 40, 72, 72, P(w1d), 0, 8, P(w2d), 1.0, 0, 0, None)),    # a = 0
        lambda: raw(lib.sdod_lokr_merge_f16(P(dev), 40, 72, 72, None, 8, 8, P(w2d), 1.0, 0, 0, None)),      # null w1
    ]
    for i, call in enumerate(bad):
        with pytest.raises(SdodError) as e:
            call()
        assert e.value.code == 2, (i, e.value)
    buf = torch.zeros(40 * 72 + 8, dtype=torch.float16, device='cuda')
    buf[1:1 + 40 * 72] = dev.view(-1)
    for call in (lambda v: ops.loha_merge(v, *fd, 1.0), lambda v: ops.lokr_merge(v, w1d, w2d, 1.0)):
        with pytest.raises(SdodError) as e:
            call(buf[1:1 + 40 * 72].view(40, 72))                                                  # base misaligned by 2 bytes
        assert e.value.code == 2
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), w) and torch.equal(buf[1:1 + 40 * 72].cpu(), w.view(-1))
