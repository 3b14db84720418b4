"""The latent-resize launch on the GPU (sdod_latent_resize_f32, ops.latent_resize) against the fp64 restatement of its definition
(tests/resize_ref.py, itself checked against torch's float64 interpolate in test_latent_resize_cpu.py).

Stated tolerances.  nearest-exact: bit-equal.  bilinear / bicubic: max |error| <= 24 * 2^-24 * max|src| -- the weights carry one
rounding each, the sums are two 4-term fp32 sums, and sum |w| <= 1.375 per axis (bicubic's overshoot); measured on an MI355X:
<= 1.96 (bilinear) and <= 2.28 (bicubic) in units of 2^-24 * max|src| over these cases.  Same size: bit-equal to the source.  Fused
form a * R + b * nu: relative error <= 1e-6 against fp64 (test_encode_latent_noise_and_formula's bound).  In-kernel noise: bit-equal
to sdod_randn_f32 on the stated streams."""
import ctypes

import numpy as np
import pytest
import torch

import resize_ref as R

pytestmark = pytest.mark.gpu

CASES = [((8, 16), (16, 24)), ((16, 24), (8, 16)), ((5, 7), (13, 9)), ((64, 64), (96, 96))]


def _src(hw, seed=3):
    return 3.0 * torch.randn(2, 4, *hw, generator=torch.Generator().manual_seed(seed + hw[0] * 100 + hw[1]))


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('hw_in,hw_out', CASES)
def test_resize_matches_the_fp64_restatement(mode, hw_in, hw_out):
    from sdod.amd import ops
    src = _src(hw_in)
    got = ops.latent_resize(src.cuda(), hw_out, mode)
    assert got.shape == (2, 4) + hw_out and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = R.resize(src.numpy(), hw_out, mode)
    if mode == 'nearest-exact':
        assert np.array_equal(got, want.astype(np.float32))
        return
    unit = 2.0 ** -24 * float(src.abs().max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f'latent_resize {mode} {hw_in} -> {hw_out}: max abs error {err / unit:.2f} x 2^-24 max|src|')
    assert np.isfinite(got).all() and err <= 24 * unit, err / unit


@pytest.mark.parametrize('mode', R.MODES)
def test_same_size_is_bit_equal(mode):
    from sdod.amd import ops
    src = _src((16, 16)).cuda()
    src[0, 0, 0, :3] = torch.tensor([-0.0, 0.0, -3e38])                   # signed zeros, near the largest finite value
    got = ops.latent_resize(src, (16, 16), mode)
    assert torch.equal(got.view(torch.int32), src.view(torch.int32))


@pytest.mark.parametrize('mode', R.MODES)
def test_fused_start_latent_formula(mode):
    from sdod.amd import ops
    src = _src((8, 16)).cuda()
    r = ops.latent_resize(src, (16, 24), mode)
    nu = torch.randn(2, 4, 16, 24, generator=torch.Generator().manual_seed(9))
    for a, b in ((0.61, 0.79), (1.0, 14.6), (0.0, 1.0), (-2.5, 0.0)):
        got = ops.latent_resize(src, (16, 24), mode, a, b, noise=nu.cuda())
        af, bf = float(np.float32(a)), float(np.float32(b))
        want = af * r.cpu().double() + bf * nu.double()
        err = float(((got.cpu().double() - want).abs() / want.abs().clamp(min=1.0)).max())
        assert err <= 1e-6, (a, b, err)
    out = torch.full((2, 4, 16, 24), 7.0, device='cuda')
    assert ops.latent_resize(src, (16, 24), mode, out=out) is out and torch.equal(out, r)


def test_in_kernel_noise_is_sdod_randn_on_the_stated_streams():
    from sdod.amd import ops
    n, c = 2, 4
    for hw_in, hw_out in (((8, 16), (16, 24)), ((5, 7), (13, 9)), ((4, 4), (3, 5))):     # c * h * w = 60: the last Philox block is cut
        src = _src(hw_in).cuda()
        seed, idx0 = 123456789, 5
        got = ops.latent_resize(src, hw_out, 'bilinear', 0.61, 0.79, seed=seed, image_index=idx0)
        nu = torch.cat([ops.randn((1, c) + hw_out, seed, (2 << 32) | (idx0 + i), 'cuda') for i in range(n)])
        assert torch.equal(got, ops.latent_resize(src, hw_out, 'bilinear', 0.61, 0.79, noise=nu))
        assert not torch.equal(got, ops.latent_resize(src, hw_out, 'bilinear', 0.61, 0.79, seed=seed + 1, image_index=idx0))
        other = ops.latent_resize(src, hw_out, 'bilinear', 0.61, 0.79, seed=seed, image_index=idx0 + 1)
        assert not torch.equal(got, other)
        assert torch.isfinite(got).all()
        # image 1 at index0 draws the stream image 0 draws at index0 + 1
        same_src = src[1:2].expand(2, -1, -1, -1).contiguous()
        a = ops.latent_resize(same_src, hw_out, 'bilinear', 0.61, 0.79, seed=seed, image_index=idx0)
        b = ops.latent_resize(same_src, hw_out, 'bilinear', 0.61, 0.79, seed=seed, image_index=idx0 + 1)
        assert torch.equal(a[1], b[0])
    # b == 0: none is read or drawn -- seed and index play no part
    src = _src((8, 16)).cuda()
    assert torch.equal(ops.latent_resize(src, (16, 24), 'bicubic', 1.0, 0.0, seed=1), ops.latent_resize(src, (16, 24), 'bicubic', 1.0, 0.0, seed=2))


def test_refused_arguments_leave_dst_untouched():
    from sdod.amd import _lib
    lib = _lib.hip()
    n, c, hi, wi, ho, wo = 2, 4, 5, 7, 13, 9
    buf = torch.full((n * c * (hi * wi + ho * wo),), -77.0, device='cuda')
    src, dst = buf[:n * c * hi * wi], buf[n * c * hi * wi:]
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(s=src, d=dst, n=n, c=c, hi=hi, wi=wi, ho=ho, wo=wo, mode=1, a=1.0, b=0.0):
        return lib.sdod_latent_resize_f32(P(s), P(d), n, c, hi, wi, ho, wo, mode, a, b, None, 0, 0, st)

    bad = [dict(s=None), dict(d=None), dict(n=0), dict(c=0), dict(hi=0), dict(wi=-1), dict(ho=0), dict(wo=0), dict(mode=3), dict(mode=-1),
           dict(a=float('nan')), dict(a=float('inf')), dict(b=float('nan')), dict(b=float('-inf')),
           dict(d=src), dict(d=buf[4:]), dict(s=buf[n * c * hi * wi - 1:], d=buf)]
    for kw in bad:
        assert call(**kw) == 2, kw
        assert lib.sdod_hip_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -77.0).all())
    assert call() == 0                                                     # the same buffers, accepted: adjacent is not overlapping
    torch.cuda.synchronize()
    assert bool((src == -77.0).all()) and bool(((dst + 77.0).abs() <= 1e-4).all())   # (a constant resizes to itself, to rounding)
