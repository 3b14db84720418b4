"""Regional prompts, the kernels: sdod_region_weights_f32 and sdod_region_blend_f16 bit for bit against their
definitions (tests/regions_ref.py), sdod_xattn_fold_regions_f16 bit for bit against the plain fold, and sdod_gemm_region_f16 -- the
region weight in the softmax epilogue of the folded cross-attention's score GEMM -- on every softmax tile.

Tolerances are those of test_kernels_gpu.py::test_folded_cross_attention_matches_linear_attention_linear for the same comparison: the
two-GEMM block against fp32 Linear -> attention -> Linear check(..., tol=4e-3), group sums within 5e-3 (here: of the region's weight;
weights in [0, 1] only scale the errors down).  Everything else is bit-exact."""
import ctypes

import pytest
import torch

import regions_ref as RR
from gemm_cases import check_close as check, run_gemm, tile_info

pytestmark = pytest.mark.gpu

SOFTMAX_TILES = (31, 48, 56, 57, 58, 59, 60)
GUARD = 16


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ sdod_region_weights_f32
def _mask_kinds(hw, k):
    ih, iw = 8 * hw[0], 8 * hw[1]
    split = RR.column_split(hw, 52, k)                                 # a hard split at pixel column 52: no multiple of 8
    over = torch.full((k, ih, iw), 255, dtype=torch.uint8)              # everything overlaps (and the largest sums there are) ...
    over[1, : ih // 2] = 128                                            # ... unevenly
    hole = RR.soft_masks(hw, k, seed=21)
    hole[:, 8:32, 16:48] = 0                                            # latent rows 1..3, columns 2..5: covered by no region
    return {'split52': split, 'overlap': over, 'hole': hole, 'soft': RR.soft_masks(hw, k, seed=22)}


@pytest.mark.parametrize('k', [2, 3, 4])
@pytest.mark.parametrize('hw', [(8, 8), (8, 16), (16, 24)])
def test_region_weights_bit_for_bit(hw, k):
    from sdod.amd import ops
    sizes = [(hw[0] // ds) * (hw[1] // ds) * k for ds in RR.LEVELS]
    for name, masks in _mask_kinds(hw, k).items():
        ref = RR.region_weights(masks)
        buf = torch.full((sum(sizes) + 5 * GUARD,), -7.0, dtype=torch.float32, device='cuda')
        outs, o = [], GUARD
        for n in sizes:
            outs.append(buf[o:o + n].view(-1, k))
            o += n + GUARD
        got = ops.region_weights(masks.cuda(), out=outs)
        torch.cuda.synchronize()
        for lvl, (g, r) in enumerate(zip(got, ref)):
            assert torch.equal(bits32(g.cpu()), bits32(r)), (name, hw, k, lvl, float((g.cpu() - r).abs().max()))
        host = buf.cpu()
        o = 0
        for n in sizes + [0]:                                           # the guard words in front of, between and behind the outputs
            assert bool((host[o:o + GUARD] == -7.0).all()), (name, o)
            o += GUARD + n
        if name == 'hole':
            assert got[0].view(hw[0], hw[1], k)[2, 3].tolist() == [1.0] + [0.0] * (k - 1)
    fresh = ops.region_weights(_mask_kinds(hw, k)['soft'].cuda())       # the allocating form
    assert all(torch.equal(a.cpu(), b) for a, b in zip(fresh, RR.region_weights(_mask_kinds(hw, k)['soft'])))


def test_region_weights_refuses_bad_arguments():
    from sdod.amd import _lib, ops
    lib = _lib.hip()
    m = torch.zeros(2, 64, 64, dtype=torch.uint8, device='cuda')
    w = [torch.full((64 * 2,), -7.0, device='cuda') for _ in range(4)]
    call = lambda mp, k, h, ww, ptrs: lib.sdod_region_weights_f32(mp, k, h, ww, *ptrs, None)
    ptrs = [P(t) for t in w]
    bad = [(None, 2, 8, 8, ptrs), (P(m), 0, 8, 8, ptrs), (P(m), 5, 8, 8, ptrs), (P(m), 2, 4, 8, ptrs), (P(m), 2, 8, 12, ptrs),
           (P(m), 2, 8, 8, ptrs[:3] + [None]), (ctypes.c_void_p(m.data_ptr() + 8), 2, 8, 8, ptrs)]
    for args in bad:
        assert call(*args) != 0 and lib.sdod_hip_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in w)
    with pytest.raises(ValueError):
        ops.region_weights(torch.zeros(2, 60, 64, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.region_weights(m.float())


# ------------------------------------------------------------------ sdod_region_blend_f16
@pytest.mark.parametrize('k', [2, 4])
@pytest.mark.parametrize('c', [320, 1280])
@pytest.mark.parametrize('rows,rpi', [(8, 8), (24, 8), (256, 64)])
def test_region_blend_bit_for_bit(rows, rpi, c, k):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(rows + c + k)
    a = (torch.randn(k, rows, c, generator=g) * torch.exp2(torch.randint(-8, 9, (k, rows, c), generator=g).float())).half()
    w = torch.rand(rpi, k, generator=g)
    w = w / w.sum(1, keepdim=True)
    w[0] = 0; w[0, k - 1] = 1                                          # a pixel wholly inside the last region
    ref = RR.region_blend(a, w)
    wr = w[torch.arange(rows) % rpi]
    fused = wr[:, 0:1] * a[0].float()                                   # what contracting every w_r a_r into its sum would give
    for r in range(1, k):
        fused = (fused.double() + wr[:, r:r + 1].double() * a[r].double()).float()
    differ = int((bits16(fused.half()) != bits16(ref)).sum())
    # the data can tell an FMA from the two roundings wherever there is enough of it for the fp16 rounding to show an fp32 ulp
    # (9 to 33 elements of the 256-row cases; the seeds are fixed)
    assert rows < 256 or differ > 0, differ
    buf = torch.full((rows * c + 2 * GUARD,), 3.0, dtype=torch.float16, device='cuda')
    ad, wd = a.cuda(), w.cuda()
    out = ops.region_blend(ad, wd, out=buf[GUARD:GUARD + rows * c].view(rows, c))
    torch.cuda.synchronize()
    assert torch.equal(bits16(out.cpu()), bits16(ref))
    host = buf.cpu()
    assert bool((host[:GUARD] == 3.0).all()) and bool((host[-GUARD:] == 3.0).all())
    assert torch.equal(bits16(ad.cpu()), bits16(a)) and torch.equal(wd.cpu(), w)
    assert torch.equal(bits16(ops.region_blend(ad, wd).cpu()), bits16(ref))
    first = ad.clone()
    ops.region_blend(first, wd, out=first[0])                           # in place on the first region's tensor, as the graph runs it
    assert torch.equal(bits16(first[0].cpu()), bits16(ref)) and torch.equal(bits16(first[1:].cpu()), bits16(a[1:]))


def test_region_blend_refuses_bad_arguments():
    from sdod.amd import _lib, ops
    lib = _lib.hip()
    a = torch.ones(2, 16, 64, dtype=torch.float16, device='cuda')
    w = torch.full((8, 2), 0.5, device='cuda')
    out = torch.full((16, 64), 9.0, dtype=torch.float16, device='cuda')
    call = lambda ap, stride, wp, op, rows, rpi, c, k: lib.sdod_region_blend_f16(ap, stride, wp, op, rows, rpi, c, k, None)
    good = (P(a), 16 * 64, P(w), P(out), 16, 8, 64, 2)
    bad = [(None,) + good[1:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:],
           good[:7] + (0,), good[:7] + (5,), good[:4] + (0, 8, 64, 2), good[:4] + (16, 0, 64, 2), good[:4] + (16, 6, 64, 2),
           good[:6] + (60, 2), good[:6] + (0, 2), (P(a), 16 * 64 - 8) + good[2:], (P(a), 16 * 64 + 4) + good[2:],
           (ctypes.c_void_p(a.data_ptr() + 8),) + good[1:], good[:3] + (ctypes.c_void_p(out.data_ptr() + 8),) + good[4:]]
    for args in bad:
        assert call(*args) != 0 and lib.sdod_hip_last_error(), args
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
    assert call(*good) == 0
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
    with pytest.raises(ValueError):
        ops.region_blend(a, torch.ones(8, 3, device='cuda'))
    with pytest.raises(ValueError):
        ops.region_blend(a, w, out=torch.zeros(8, 64, dtype=torch.float16, device='cuda'))


# ------------------------------------------------------------------ the fold and the region GEMM
CASES = [(rows, c, d, k) for rows in (32, 64, 96, 256) for c, d in ((320, 40), (1280, 160)) for k in (2, 3)]


def _block(rows, c, d, k, B=2, L=77, cd=768):
    """operands of one cross-attention block with k prompts per image; the fold in both forms"""
    from sdod.amd import ops
    heads = c // d
    g = torch.Generator().manual_seed(rows * 7 + c + d + k)
    t = dict(heads=heads, B=B, L=L, rows=rows, c=c, d=d, k=k, nk=heads * 80)
    t['x'] = (torch.randn(B * rows, c, generator=g) * 1.5 + 0.3).half().cuda()
    t['ctx'] = torch.randn(B * k * L, cd, generator=g).half().cuda()
    for n, shape, s in (('wq', (c, c), c), ('wo', (c, c), c), ('wk', (c, cd), cd), ('wv', (c, cd), cd)):
        t[n] = (torch.randn(*shape, generator=g) / s ** 0.5).half().cuda()
    t['gamma'] = (1 + 0.2 * torch.randn(c, generator=g)).cuda(); t['beta'] = (0.1 * torch.randn(c, generator=g)).cuda()
    t['bo'] = (0.1 * torch.randn(c, generator=g)).cuda()
    w = torch.rand(rows, k, generator=g)
    w = w / w.sum(1, keepdim=True)
    w[0] = 0; w[0, 0] = 1; w[1] = 0; w[1, k - 1] = 1                    # pixels wholly inside the first / the last region
    t['w'] = w.cuda()
    t['kv'] = ops.gemm(t['ctx'], torch.cat([t['wk'], t['wv']], 0))
    t['wq_f'], t['sq'], t['tq'] = ops.ln_fold(t['wq'].clone(), t['gamma'], t['beta'])
    t['fold'] = ops.xattn_fold(t['kv'], 0, c, B, L, t['wq_f'], t['sq'], t['tq'], t['wo'], heads, regions=k)
    t['plain_fold'] = ops.xattn_fold(t['kv'], 0, c, B * k, L, t['wq_f'], t['sq'], t['tq'], t['wo'], heads)
    return t


def _runs_on(tile, rows):
    """make_plan: a tile whose rows do not divide the image is replaced by 31 (64 rows) or 48 (32 rows)"""
    return tile if rows % tile_info(tile)['bm'] == 0 else (31 if rows % 64 == 0 else 48)


@pytest.mark.parametrize('rows,c,d,k', CASES)
def test_fold_with_regions_is_the_plain_fold_bit_for_bit(rows, c, d, k):
    t = _block(rows, c, d, k)
    B, nk = t['B'], t['nk']
    w1, s1, t1, w2 = t['fold']
    ow1, os1, ot1, ow2 = t['plain_fold']                                # n_img * k "images": one per (image, region) segment
    assert tuple(w1.shape) == (B, k * nk, c) and tuple(w2.shape) == (B, c, k * nk) and tuple(s1.shape) == tuple(t1.shape) == (B, k * nk)
    assert torch.equal(bits16(w1.view(B * k, nk, c)), bits16(ow1))
    assert torch.equal(bits32(s1.view(B * k, nk)), bits32(os1)) and torch.equal(bits32(t1.view(B * k, nk)), bits32(ot1))
    for b in range(B):
        for r in range(k):
            assert torch.equal(bits16(w2[b, :, r * nk:(r + 1) * nk]), bits16(ow2[b * k + r])), (b, r)
    from sdod.amd import ops
    one = ops.xattn_fold(t['kv'], 0, c, B * k, t['L'], t['wq_f'], t['sq'], t['tq'], t['wo'], t['heads'], regions=1)
    assert all(torch.equal(a.view(-1), b.view(-1)) for a, b in zip(one, t['plain_fold']))      # regions = 1 is the plain call


@pytest.mark.parametrize('rows,c,d,k', CASES)
def test_region_gemm_on_every_softmax_tile(rows, c, d, k):
    from sdod.amd import ops
    t = _block(rows, c, d, k)
    B, nk, heads, L, x = t['B'], t['nk'], t['heads'], t['L'], t['x']
    w1, s1, t1, w2 = t['fold']
    ow1, os1, ot1, _ = t['plain_fold']
    # region 0's operands of every image: what a plain one-prompt block would multiply
    p_w1 = ow1.view(B, k, nk, c)[:, 0].contiguous(); p_s1 = os1.view(B, k, nk)[:, 0].contiguous(); p_t1 = ot1.view(B, k, nk)[:, 0].contiguous()
    ones = torch.ones(rows, 1, device='cuda')
    first = torch.zeros(rows, k, device='cuda'); first[:, 0] = 1
    kw = dict(rows_per_img=rows, softmax_cols=80)
    for tile in SOFTMAX_TILES:
        on = _runs_on(tile, rows)
        plain = run_gemm(x, p_w1, p_t1, ln_s=p_s1, tile=tile, runs_on=on, tag='regions', **kw)[0]
        # (i) one region, weight 1.0: sdod_gemm_f16's bits
        got = run_gemm(x, p_w1, p_t1, ln_s=p_s1, tile=tile, runs_on=on, tag='regions', region_w=ones, regions=1, **kw)[0]
        assert torch.equal(bits16(got), bits16(plain)), (tile, 'regions=1')
        # (ii) weights (1, 0, ..): region 0's columns are the plain call's bits, every other column an exact zero
        got = run_gemm(x, w1, t1, ln_s=s1, tile=tile, runs_on=on, tag='regions', region_w=first, regions=k, **kw)[0]
        assert torch.equal(bits16(got[:, :nk]), bits16(plain)), (tile, 'weight 1')
        assert int((bits16(got[:, nk:]) != 0).sum()) == 0, (tile, 'weight 0')
        # (iii) soft weights: every 80-column group sums to its region's weight at the row's pixel; padding columns exact zeros
        p = run_gemm(x, w1, t1, ln_s=s1, tile=tile, runs_on=on, tag='regions', region_w=t['w'], regions=k, **kw)[0]
        pv = p.float().view(B, rows, k, heads, 80)
        assert float(pv[..., L:].abs().max()) == 0, tile
        err = float((pv.sum(-1) - t['w'].view(1, rows, k, 1)).abs().max())
        assert err < 5e-3, (tile, err)
        assert float(pv[:, 0, 1:].abs().max()) == 0 and float(pv[:, 1, :k - 1].abs().max()) == 0      # the rows with a zero weight
    # ... and behind the second GEMM the block is sum_r w_r attn(x, K_r, V_r) -> to_out + residual (fp32, same fp16 parameters)
    p = ops.gemm(x, w1, t1, ln_s=s1, region_w=t['w'], regions=k, **kw)
    out = ops.gemm(p, w2, t['bo'], residual=x, rows_per_img=rows)
    xf = x.float()
    ln = torch.nn.functional.layer_norm(xf, (c,), t['gamma'], t['beta'], 1e-5)
    q = (ln @ t['wq'].float().t()).view(B, rows, heads, d).transpose(1, 2)
    ctx = t['ctx'].float().view(B, k, L, -1)
    blend = torch.zeros(B, rows, c, device='cuda')
    for r in range(k):
        kk = (ctx[:, r] @ t['wk'].float().t()).view(B, L, heads, d).transpose(1, 2)
        vv = (ctx[:, r] @ t['wv'].float().t()).view(B, L, heads, d).transpose(1, 2)
        att = (torch.softmax(q @ kk.transpose(-1, -2) * d ** -0.5, -1) @ vv).transpose(1, 2).reshape(B, rows, c)
        blend = blend + t['w'][None, :, r:r + 1] * att
    ref = blend.reshape(B * rows, c) @ t['wo'].float().t() + t['bo'] + xf
    check(out, ref, tol=4e-3, name=f'regional folded cross-attention rows {rows} C{c} d{d} k{k}')


def test_region_gemm_reads_its_weights_in_the_launch():
    """(iv) the same captured launch with other weight VALUES gives the other result: what a captured UNet relies on"""
    from sdod.amd import ops
    t = _block(64, 320, 40, 2)
    w1, s1, t1, _ = t['fold']
    kw = dict(ln_s=s1, rows_per_img=64, softmax_cols=80, regions=2)
    wa, wb = t['w'].clone(), t['w'].flip(1).contiguous()
    ra = ops.gemm(t['x'], w1, t1, region_w=wa, **kw); rb = ops.gemm(t['x'], w1, t1, region_w=wb, **kw)
    assert not torch.equal(ra, rb)
    live = wa.clone()
    out = torch.empty_like(ra)
    ops.gemm(t['x'], w1, t1, region_w=live, out=out, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gemm(t['x'], w1, t1, region_w=live, out=out, **kw)
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(bits16(out), bits16(ra))
    live.copy_(wb)
    g.replay(); torch.cuda.synchronize()
    assert torch.equal(bits16(out), bits16(rb))


def test_region_gemm_refusals_write_nothing():
    """(v) null weights, a region count that does not divide N / 80, no softmax_cols, no per-image weights, rows_per_img = 24"""
    from sdod.amd import _lib, ops
    B, rows, c, nk = 2, 32, 320, 1280
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B * rows, c, generator=g).half().cuda()
    w1 = (torch.randn(B, nk, c, generator=g) / c ** 0.5).half().cuda()
    s1 = torch.ones(B, nk).cuda(); t1 = torch.zeros(B, nk).cuda()
    rw = torch.full((rows, 4), 0.25).cuda()
    p = torch.full((B * rows, nk), float('nan'), dtype=torch.float16).cuda()
    kw = dict(ln_s=s1, rows_per_img=rows, softmax_cols=80, out=p)
    with pytest.raises(_lib.SdodError, match='region_w'):
        ops.gemm(x, w1, t1, region_w=None, regions=2, **kw)
    with pytest.raises(_lib.SdodError, match='regions'):
        ops.gemm(x, w1, t1, region_w=rw, regions=3, **kw)                # 16 groups, 3 regions
    with pytest.raises(_lib.SdodError, match='regions'):
        ops.gemm(x, w1, t1, region_w=rw, regions=5, **kw)
    with pytest.raises(_lib.SdodError, match='regions'):
        ops.gemm(x, w1, t1, region_w=rw, regions=-1, **kw)
    with pytest.raises(_lib.SdodError, match='softmax_cols'):
        ops.gemm(x, w1, t1, region_w=rw, regions=2, ln_s=s1, rows_per_img=rows, out=p)
    with pytest.raises(_lib.SdodError, match='per-image weights'):      # one shared weight matrix: nothing says where an image ends
        ops.gemm(x, w1[0], t1[0], region_w=rw, regions=2, ln_s=s1[0], softmax_cols=80, out=p)
    x24 = x[:B * 24]
    p24 = torch.full((B * 24, nk), float('nan'), dtype=torch.float16).cuda()
    with pytest.raises(_lib.SdodError, match='rows_per_img a multiple of 32'):
        ops.gemm(x24, w1, t1, region_w=rw, regions=2, ln_s=s1, rows_per_img=24, softmax_cols=80, out=p24)
    torch.cuda.synchronize()
    assert torch.isnan(p).all() and torch.isnan(p24).all(), 'a refused GEMM wrote to its destination'
    ops.gemm(x, w1, t1, region_w=rw, regions=2, **kw)                   # the good call
    torch.cuda.synchronize()
    assert torch.isfinite(p).all()
