"""The exact-data recipes of tests/gemm_cases.py, checked without a GPU: the fp64 reference fits fp16 exactly, and fp32 sums
of the products give that reference in whatever order they are taken (whole K, 64-wide slabs, ragged split-K slices) -- and
what the launcher refuses before it launches anything (host-only: the descriptors carry fake pointers)."""
import ctypes

import pytest
import torch

import gemm_cases as gc


def _f32_orders(a, wf, k):
    """a . wf^T in fp32: at once, per 64-wide slab in both directions, and in three ragged split-K slices summed afterwards"""
    a32, w32 = a.float(), wf.float()
    yield a32 @ w32.t()
    slabs = [a32[:, s:s + 64] @ w32[:, s:s + 64].t() for s in range(0, k, 64)]
    acc = torch.zeros_like(slabs[0])
    for s in slabs:
        acc = acc + s
    yield acc
    acc = torch.zeros_like(slabs[0])
    for s in reversed(slabs):
        acc = acc + s
    yield acc
    cut = [0, (len(slabs) + 2) // 3, 2 * ((len(slabs) + 2) // 3), len(slabs)]
    parts = [sum(slabs[cut[i]:cut[i + 1]], torch.zeros_like(slabs[0])) for i in range(3)]
    yield parts[0] + parts[1] + parts[2]


@pytest.mark.parametrize('k', [64, 704, 1600])
def test_exact_fp16_recipe(k):
    m, n = 70, 72
    a, w, gen = gc.exact_f16(m, n, k, 7)
    bias = gc.small_ints((n,), gen, torch.float32); rb = gc.small_ints((3, n), gen); res = gc.small_ints((m, n), gen)
    ref = gc.ref_rows(a, w, bias, rb, 24, res)
    gc.assert_exact(ref)
    for y in _f32_orders(a, w, k):
        full = (y + bias + rb.float()[torch.arange(m) // 24]).half().float() + res.float()
        assert torch.equal(full.half().double(), ref)
    worst = torch.ones(1, 1600).half()                       # every product +1: the bound of the recipe itself
    gc.assert_exact(gc.ref_rows(worst, worst) + 24)
    for alpha in (0.5, 2.0 ** -4):
        ref = gc.ref_rows(a, w, alpha=alpha)
        gc.assert_exact(ref)
        assert torch.equal(((a.float() @ w.float().t()) * alpha).half().double(), ref)


@pytest.mark.parametrize('k', [64, 256, 1280])
def test_exact_uint8_recipe(k):
    m, n = 70, 72
    a, q, scale, off, wf, gen = gc.exact_u8(m, n, k, 9)
    assert int((a != 0).sum(1).max()) <= 8 and set(a.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert int(q.max()) > 250 and int(q.min()) < 5 and torch.equal(scale, torch.ones(n))
    assert torch.equal(wf, q.double() - 128 + off.double()[:, None]) and float(wf.abs().max()) <= 255
    ref = gc.ref_rows(a, wf)
    gc.assert_exact(ref)
    for y in _f32_orders(a, wf, k):
        assert torch.equal(y.half().double(), ref)
    # the form the kernel takes: codes recentred to q - 128 in fp16 (exact), the column's offset applied to the row sum of a
    y = a.float() @ (q.float() - 128).half().float().t() + a.float().sum(1, keepdim=True) * off[None, :]
    assert torch.equal(y.half().double(), ref)


def test_frames_and_sentinel():
    s = torch.tensor([gc.SENTINEL], dtype=torch.int16).view(torch.float16)
    assert torch.isfinite(s).all() and float(s) != round(float(s))
    f = gc.Framed(5, 24, 40, 8, device=torch.device('cpu'))
    assert f.view.shape == (5, 24) and f.view.stride() == (40, 1) and torch.isnan(f.view).all()
    f.view.fill_(1.0)
    f.frame_intact()
    for r, c in ((0, 9), (6, 0), (2, 7), (2, 32), (1, 39)):          # guard rows, columns left and right of the matrix
        g = gc.Framed(5, 24, 40, 8, device=torch.device('cpu'))
        g.buf[r, c] = 1.0
        with pytest.raises(AssertionError):
            g.frame_intact()
    a = gc.Framed(3, 64, 80, 0, fill='nan', device=torch.device('cpu'), data=torch.ones(3, 64).half())
    assert torch.isnan(a.buf[:, 64:]).all() and torch.isnan(a.buf[0]).all() and torch.isnan(a.buf[4]).all() and torch.isfinite(a.view).all()


def test_table_keys_decode():
    picks = gc.table_picks()
    assert len(picks) > 500
    assert 53 in gc.picked_tiles(a_mode=0, geglu=True, ln=True, strided=True) and 61 in gc.picked_tiles(a_mode=0, geglu=True, ln=True, strided=True)
    assert any(k['M'] == 8192 and k['N'] == 2560 and k['K'] == 320 and k['lda'] == 1600 and t == 53 for k, t, _ in picks)
    assert any(k['M'] == 512 and k['N'] == 10240 and k['K'] == 1280 and k['lda'] == 6400 and t == 61 for k, t, _ in picks)


def test_launcher_rejects_misaligned_out_and_residual_before_launching():
    """the 16-byte store paths (N, ldo, ldr multiples of 8) need 16-byte-aligned out / residual.  The descriptor is a split-K
    plan WITHOUT a workspace, which the launcher refuses further down anyway: whatever this test meets, nothing is launched"""
    from sdod.amd import _lib
    lib = _lib.hip()

    def message(**fields):
        d = gc.rows_desc(256, 128, 256, tile=8, split=2, **fields)
        assert lib.sdod_gemm_f16(ctypes.byref(d), None) != 0
        return lib.sdod_hip_last_error().decode()

    assert 'workspace' in message()
    assert '16-byte aligned' in message(out=0x1008) and 'out and residual' in message(out=0x1008)
    assert 'out and residual' in message(residual=0x1004, ldr=128)
    assert 'out and residual' in message(out=0x1002, ldo=136)
    # widths that take the scalar store path anyway carry no such demand
    assert 'workspace' in message(out=0x1002, ldo=132)
    assert 'workspace' in message(residual=0x1004, ldr=132)
    d = gc.rows_desc(256, 132, 256, tile=8, split=2, out=0x1002)
    assert lib.sdod_gemm_f16(ctypes.byref(d), None) != 0 and 'workspace' in lib.sdod_hip_last_error().decode()
