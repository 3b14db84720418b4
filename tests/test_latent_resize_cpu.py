"""The latent resize's coordinate arithmetic on the CPU: sdod_latent_resize_taps -- the table the kernel computes with, filled by the
same function on the host -- against the fp64 restatement of its definition (tests/resize_ref.py) and against torch's float64
interpolate on an identity basis.

Stated tolerances: indices exact; a weight equals the fp64 value rounded to fp32 within 1 fp32 ulp (the library rounds t once in fp64,
evaluates in fp64 and rounds to fp32: a double rounding against the restatement's exact-rational t); the restatement equals torch's
float64 result to 1e-12 (measured: <= 8e-14 at these sizes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_ref as R

PAIRS = [(8, 16), (16, 24), (8, 24), (16, 16), (24, 16), (5, 13), (7, 9), (64, 96)]


@pytest.fixture(scope='module')
def lib():
    from sdod.amd import _lib
    return _lib.hip()


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('n_in,n_out', PAIRS)
def test_taps_match_the_fp64_restatement(lib, mode, n_in, n_out):
    from sdod.amd import ops
    idx, w = ops.latent_resize_taps(mode, n_in, n_out)
    idx, w = idx.numpy(), w.numpy()
    assert idx.shape == (n_out, 4) and w.shape == (n_out, 4) and w.dtype == np.float32
    ref_idx, ref_w = R.axis_taps(mode, n_in, n_out)
    assert np.array_equal(idx, ref_idx)
    want = ref_w.astype(np.float32)
    ulp = np.spacing(np.abs(want))                       # one fp32 ulp at each weight
    err = np.abs(w.astype(np.float64) - want.astype(np.float64))
    assert (err <= ulp).all(), float((err / ulp).max())
    assert (w[ref_w == 0.0] == 0.0).all()               # unused slots and exact zeros stay exact zeros


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('n_in,n_out', PAIRS)
def test_restatement_matches_torch_float64(mode, n_in, n_out):
    """each axis on an identity basis: interpolate applied to the n_in unit vectors gives the axis matrix"""
    eye = torch.eye(n_in, dtype=torch.float64)[:, None, :, None].expand(n_in, 1, n_in, 3).contiguous()   # [basis, 1, n_in, 3]
    kw = {} if mode == 'nearest-exact' else dict(align_corners=False)
    got = F.interpolate(eye, size=(n_out, 3), mode=mode, **kw)[:, 0, :, 0].T.numpy()                    # [n_out, n_in]
    ref = R.axis_matrix(mode, n_in, n_out)
    err = float(np.abs(got - ref).max())
    assert err <= 1e-12, err


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('n', [1, 5, 16, 96])
def test_same_size_is_the_identity(lib, mode, n):
    from sdod.amd import ops
    idx, w = ops.latent_resize_taps(mode, n, n)
    idx, w = idx.numpy(), w.numpy()
    m = np.zeros((n, n), np.float32)
    for d in range(n):
        for k in range(4):
            m[d, idx[d, k]] += w[d, k]
        assert sorted(w[d].tolist()) == [0.0, 0.0, 0.0, 1.0], (d, w[d])
    assert np.array_equal(m, np.eye(n, dtype=np.float32))


def test_taps_refuse_bad_arguments(lib):
    import ctypes
    idx = (ctypes.c_int32 * 16)()
    w = (ctypes.c_float * 16)()
    assert lib.sdod_latent_resize_taps(1, 4, 4, idx, w) == 0
    for args in ((3, 4, 4, idx, w), (-1, 4, 4, idx, w), (1, 0, 4, idx, w), (1, 4, 0, idx, w), (1, 4, 4, None, w), (1, 4, 4, idx, None)):
        assert lib.sdod_latent_resize_taps(*args) == 2, args
    with pytest.raises(ValueError):
        from sdod.amd import ops
        ops.latent_resize(torch.zeros(1, 4, 8, 8), (16, 16), mode='lanczos')


def test_symbols_are_exported_and_bound(lib):
    from sdod.amd import _lib
    for sym in ('sdod_latent_resize_f32', 'sdod_latent_resize_taps'):
        assert hasattr(lib, sym), sym
        assert sym in _lib.HIP_SYMBOLS, sym
