"""Image prompts, the kernels: sdod_xattn_fold_ip_f16 bit for bit against the plain fold run on each source alone
(and against an fp64 restatement), sdod_ip_weights_f32 and sdod_patch_embed_u8_f16 bit for bit against their definitions
(tests/ipadapter_ref.py), sdod_vit_tokens_f16 against fp64 within one fp16 ulp, and the score GEMM with weights (1, s) through
sdod_gemm_region_f16 on every softmax tile.

Tolerances.  The fold rounds an fp32 accumulation of fp16 products once to fp16: half an fp16 ulp of the value (2^-11 relative, 2^-25
absolute below the normal range) plus the fp32 accumulation's own error, at most K 2^-23 sum |a_k b_k| over the K <= 96 terms.  The
tokens kernel computes in fp32 and rounds once: one fp16 ulp of the fp64 value (2^-10 relative, 2^-24 absolute).  Everything else
is bit-exact."""
import ctypes

import pytest
import torch

import ipadapter_ref as IR
from gemm_cases import run_gemm, tile_info

pytestmark = pytest.mark.gpu

SOFTMAX_TILES = (31, 48, 56, 57, 58, 59, 60)                             # as tests/test_regions_kernel_gpu.py enumerates them
GUARD = 16


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------ sdod_xattn_fold_ip_f16
def _fold_operands(c, heads, T, B=2, L=77, cd=768, ld_ip_extra=0):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(c + heads + T)
    t = dict(B=B, L=L, T=T, c=c, heads=heads, d=c // heads, nk=heads * 80)
    ctx = torch.randn(B * L, cd, generator=g).half().cuda()
    tok = torch.randn(B * T, cd, generator=g).half().cuda()
    for n, shape, s in (('wq', (c, c), c), ('wo', (c, c), c), ('wk', (c, cd), cd), ('wv', (c, cd), cd), ('wk_ip', (c, cd), cd), ('wv_ip', (c, cd), cd)):
        t[n] = (torch.randn(*shape, generator=g) / s ** 0.5).half().cuda()
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).cuda(); beta = (0.1 * torch.randn(c, generator=g)).cuda()
    t['kv'] = ops.gemm(ctx, torch.cat([t['wk'], t['wv']], 0))
    # the image tokens' K | V behind 64 columns of something else, in rows of their own length: another stride, other offsets
    kv_ip = ops.gemm(tok, torch.cat([t['wk_ip'], t['wv_ip']], 0))
    t['kv_ip'] = torch.cat([torch.full((B * T, 64), 7.0, dtype=torch.float16, device='cuda'), kv_ip,
                            torch.full((B * T, ld_ip_extra), 7.0, dtype=torch.float16, device='cuda')], 1).contiguous()
    t['ip_off'] = 64
    t['wq_f'], t['sq'], t['tq'] = ops.ln_fold(t['wq'].clone(), gamma, beta)
    return t


@pytest.mark.parametrize('T', [1, 4, 16])
@pytest.mark.parametrize('c,heads', [(320, 8), (640, 8)])
def test_fold_on_two_sources_is_the_plain_fold_of_each_bit_for_bit(c, heads, T):
    from sdod.amd import ops
    t = _fold_operands(c, heads, T, ld_ip_extra=8)
    B, L, nk, d, off = t['B'], t['L'], t['nk'], t['d'], t['ip_off']
    args = (t['wq_f'], t['sq'], t['tq'], t['wo'], heads)
    w1, s1, t1, w2 = ops.xattn_fold_ip(t['kv'], 0, c, t['kv_ip'], off, off + c, B, L, T, *args)
    torch.cuda.synchronize()
    assert tuple(w1.shape) == (B, 2 * nk, c) and tuple(w2.shape) == (B, c, 2 * nk) and tuple(s1.shape) == tuple(t1.shape) == (B, 2 * nk)
    text = ops.xattn_fold(t['kv'], 0, c, B, L, *args)
    image = ops.xattn_fold(t['kv_ip'], off, off + c, B, T, *args)
    for seg, (pw1, ps1, pt1, pw2), n in ((0, text, L), (1, image, T)):
        assert torch.equal(bits16(w1.view(B, 2, nk, c)[:, seg]), bits16(pw1)), seg
        assert torch.equal(bits32(s1.view(B, 2, nk)[:, seg]), bits32(ps1)) and torch.equal(bits32(t1.view(B, 2, nk)[:, seg]), bits32(pt1)), seg
        assert torch.equal(bits16(w2.view(B, c, 2, nk)[:, :, seg]), bits16(pw2)), seg
        # the padding columns: zero rows / columns, s = 0, t = -30000
        assert float(w1.view(B, 2, heads, 80, c)[:, seg, :, n:].abs().max()) == 0
        assert float(w2.view(B, c, 2, heads, 80)[:, :, seg, :, n:].abs().max()) == 0
        assert bool((s1.view(B, 2, heads, 80)[:, seg, :, n:] == 0).all()) and bool((t1.view(B, 2, heads, 80)[:, seg, :, n:] == -30000.0).all())
    # against the definition in fp64, on the same fp16 operands
    alpha = d ** -0.5 * 1.4426950408889634
    wq64, wo64 = t['wq_f'].double().cpu(), t['wo'].double().cpu()
    for seg, kvsrc, koff, n in ((0, t['kv'], 0, L), (1, t['kv_ip'], off, T)):
        kv = kvsrc.double().cpu()
        K = kv[:, koff:koff + c].view(B, n, heads, d); V = kv[:, koff + c:koff + 2 * c].view(B, n, heads, d)
        wqh = wq64.view(heads, d, c)
        ref1 = alpha * torch.einsum('bjhk,hkc->bhjc', K, wqh)                                   # [B, heads, n, C]
        mag1 = alpha * torch.einsum('bjhk,hkc->bhjc', K.abs(), wqh.abs())
        got1 = w1.view(B, 2, heads, 80, c)[:, seg, :, :n].double().cpu()
        woh = wo64.view(c, heads, d)
        ref2 = torch.einsum('chk,bjhk->bchj', woh, V)                                           # [B, C, heads, n]
        mag2 = torch.einsum('chk,bjhk->bchj', woh.abs(), V.abs())
        got2 = w2.view(B, c, 2, heads, 80)[:, :, seg, :, :n].double().cpu()
        for got, ref, mag in ((got1, ref1, mag1), (got2, ref2, mag2)):
            bound = ref.abs() * 2.0 ** -11 * (1 + 2.0 ** -10) + 96 * 2.0 ** -23 * mag + 2.0 ** -25
            worst = float(((got - ref).abs() / bound).max())
            print(f'fold C{c} T{T} segment {seg}: worst error / bound {worst:.3f}')
            assert worst <= 1.0, (seg, worst)
        sq64, tq64 = t['sq'].double().cpu().view(heads, d), t['tq'].double().cpu().view(heads, d)
        for got, vec in ((s1, sq64), (t1, tq64)):
            ref = alpha * torch.einsum('bjhk,hk->bhj', K, vec)
            mag = alpha * torch.einsum('bjhk,hk->bhj', K.abs(), vec.abs())
            err = (got.view(B, 2, heads, 80)[:, seg, :, :n].double().cpu() - ref).abs()
            assert bool((err <= 96 * 2.0 ** -23 * mag + 1e-30).all())                           # fp32 throughout


def test_fold_on_two_sources_refuses_bad_arguments():
    from sdod.amd import _lib
    lib = _lib.hip()
    t = _fold_operands(320, 8, 4)
    B, L, c, nk = t['B'], t['L'], t['c'], t['nk']
    outs = [torch.full((B * 2 * nk * c,), 5.0, dtype=torch.float16, device='cuda'), torch.full((B * 2 * nk,), 5.0, device='cuda'),
            torch.full((B * 2 * nk,), 5.0, device='cuda'), torch.full((B * 2 * nk * c,), 5.0, dtype=torch.float16, device='cuda')]

    def call(kv_ip=P(t['kv_ip']), ld_ip=t['kv_ip'].shape[1], k_ip=64, v_ip=64 + c, T=4, L_=L):
        return lib.sdod_xattn_fold_ip_f16(P(t['kv']), 2 * c, 0, c, kv_ip, ld_ip, k_ip, v_ip, B, L_, T, P(t['wq_f']), c, P(t['sq']), P(t['tq']),
                                          P(t['wo']), c, 8, 40, 40 ** -0.5, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), None)
    for kw in (dict(kv_ip=None), dict(T=0), dict(T=17), dict(L_=81), dict(ld_ip=2 * c + 60), dict(k_ip=4), dict(v_ip=64 + c + 8),
               dict(k_ip=-8), dict(kv_ip=ctypes.c_void_p(t['kv_ip'].data_ptr() + 8))):
        assert call(**kw) != 0 and lib.sdod_hip_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((o == 5.0).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((outs[0] == 5.0).any())


# ------------------------------------------------------------------ sdod_ip_weights_f32
def _masks(hw):
    ih, iw = 8 * hw[0], 8 * hw[1]
    return {'none': None, 'zeros': torch.zeros(ih, iw, dtype=torch.uint8), 'full': torch.full((ih, iw), 255, dtype=torch.uint8),
            'soft': IR.soft_mask(hw, 31), 'left52': torch.cat([torch.full((ih, 52), 255, dtype=torch.uint8), torch.zeros(ih, iw - 52, dtype=torch.uint8)], 1)}


@pytest.mark.parametrize('scale', [0.0, 0.7, 1.0, 1.3])
@pytest.mark.parametrize('hw', [(8, 8), (8, 16), (16, 16)])
def test_ip_weights_bit_for_bit(hw, scale):
    from sdod.amd import ops
    sizes = [(hw[0] // ds) * (hw[1] // ds) * 2 for ds in IR.LEVELS]
    for name, mask in _masks(hw).items():
        ref = IR.ip_weights(scale, hw, mask)
        buf = torch.full((sum(sizes) + 5 * GUARD,), -7.0, dtype=torch.float32, device='cuda')
        outs, o = [], GUARD
        for n in sizes:
            outs.append(buf[o:o + n].view(-1, 2))
            o += n + GUARD
        got = ops.ip_weights(scale, hw[0], hw[1], None if mask is None else mask.cuda(), out=outs)
        torch.cuda.synchronize()
        for lvl, (g, r) in enumerate(zip(got, ref)):
            assert torch.equal(bits32(g.cpu()), bits32(r)), (name, hw, scale, lvl, float((g.cpu() - r).abs().max()))
        host = buf.cpu()
        o = 0
        for n in sizes + [0]:                                           # the guard words in front of, between and behind the outputs
            assert bool((host[o:o + GUARD] == -7.0).all()), (name, o)
            o += GUARD + n
        if name in ('none', 'full'):
            assert all(bool((g[:, 1] == torch.tensor(scale, dtype=torch.float32)).all()) for g in got)
        if name == 'zeros' or scale == 0.0:
            assert all(bits32(g[:, 1].cpu()).eq(0).all() for g in got)   # +0.0: the image segment then contributes exact zeros


def test_ip_weights_refuses_bad_arguments():
    from sdod.amd import _lib, ops
    lib = _lib.hip()
    m = torch.zeros(64, 64, dtype=torch.uint8, device='cuda')
    w = [torch.full((64 * 2,), -7.0, device='cuda') for _ in range(4)]
    ptrs = [P(t) for t in w]
    call = lambda mp, s, h, ww, pp: lib.sdod_ip_weights_f32(mp, ctypes.c_float(s), h, ww, *pp, None)
    for args in ((P(m), -0.5, 8, 8, ptrs), (P(m), float('nan'), 8, 8, ptrs), (P(m), float('inf'), 8, 8, ptrs), (P(m), 1.0, 4, 8, ptrs),
                 (P(m), 1.0, 8, 12, ptrs), (P(m), 1.0, 8, 8, ptrs[:3] + [None]), (ctypes.c_void_p(m.data_ptr() + 8), 1.0, 8, 8, ptrs)):
        assert call(*args) != 0 and lib.sdod_hip_last_error(), args[1:4]
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in w)
    with pytest.raises(ValueError):
        ops.ip_weights(1.0, 8, 8, torch.zeros(60, 64, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        ops.ip_weights(-1.0, 8, 8)


# ------------------------------------------------------------------ the vision tower's input side
@pytest.mark.parametrize('S', [28, 56])
def test_patch_embed_bit_for_bit(S):
    from sdod.amd import ops
    g = torch.Generator().manual_seed(S)
    img = torch.randint(0, 256, (2, S, S, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    img[0, 0, :8, 0] = torch.tensor([0, 1, 2, 127, 128, 253, 254, 255], dtype=torch.uint8)
    ref = IR.patch_rows(img, 14, kpad=640).half()
    got = ops.patch_embed(img.cuda(), 14)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2 * (S // 14) ** 2, 640)
    assert torch.equal(bits16(got.cpu()), bits16(ref))
    assert int((bits16(got[:, 588:].cpu()) != 0).sum()) == 0              # the padding columns: +0.0
    with pytest.raises(ValueError):
        ops.patch_embed(img[:, :, :14].cuda(), 14)


@pytest.mark.parametrize('NP', [4, 16])
def test_vit_tokens_against_fp64(NP):
    from sdod.amd import ops
    W, n = 320, 2
    g = torch.Generator().manual_seed(NP)
    patches = torch.randn(n, NP, W, generator=g).half()
    cls = (torch.randn(W, generator=g) * 0.5).half(); pos = (torch.randn(NP + 1, W, generator=g) * 0.5).half()
    w = 1 + 0.2 * torch.randn(W, generator=g); b = 0.1 * torch.randn(W, generator=g)
    ref = IR.vit_tokens(patches.double(), cls.double(), pos.double(), w.double(), b.double())
    got = ops.vit_tokens(patches.cuda(), cls.cuda(), pos.cuda(), w.cuda(), b.cuda())
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, NP + 1, W)
    err = (got.double().cpu() - ref).abs()
    bound = ref.abs() * 2.0 ** -10 + 2.0 ** -24
    worst = float((err / bound).max())
    print(f'vit_tokens P{NP}: worst error / one fp16 ulp {worst:.3f}')
    assert worst <= 1.0, worst


# ------------------------------------------------------------------ the score GEMM with weights (1, s)
@pytest.mark.parametrize('rows,c,heads,T', [(32, 320, 8, 4), (64, 640, 8, 16), (96, 320, 8, 1), (256, 640, 8, 4)])
def test_score_gemm_with_an_image_segment_on_every_softmax_tile(rows, c, heads, T):
    from sdod.amd import ops
    t = _fold_operands(c, heads, T)
    B, L, nk, off = t['B'], t['L'], t['nk'], t['ip_off']
    args = (t['wq_f'], t['sq'], t['tq'], t['wo'], heads)
    w1, s1, t1, _ = ops.xattn_fold_ip(t['kv'], 0, c, t['kv_ip'], off, off + c, B, L, T, *args)
    pw1, ps1, pt1, _ = ops.xattn_fold(t['kv'], 0, c, B, L, *args)
    g = torch.Generator().manual_seed(rows + T)
    x = (torch.randn(B * rows, c, generator=g) * 1.5 + 0.3).half().cuda()
    kw = dict(rows_per_img=rows, softmax_cols=80)
    for s in (0.0, 0.5, 1.0):
        wts = torch.stack([torch.ones(rows), torch.full((rows,), s)], 1).cuda()
        for tile in SOFTMAX_TILES:
            on = tile if rows % tile_info(tile)['bm'] == 0 else (31 if rows % 64 == 0 else 48)
            plain = run_gemm(x, pw1, pt1, ln_s=ps1, tile=tile, runs_on=on, tag='ipadapter', **kw)[0]
            got = run_gemm(x, w1, t1, ln_s=s1, tile=tile, runs_on=on, tag='ipadapter', region_w=wts, regions=2, **kw)[0]
            assert torch.equal(bits16(got[:, :nk]), bits16(plain)), (tile, s)       # the text half: sdod_gemm_f16's bits
            img = got[:, nk:].float().view(B * rows, heads, 80)
            assert float(img[..., T:].abs().max()) == 0, (tile, s)                   # padding columns
            if s == 0.0:
                assert int((bits16(got[:, nk:]) != 0).sum()) == 0, tile              # exact zeros
            else:
                err = float((img.sum(-1) - s).abs().max())
                assert err < 5e-3, (tile, s, err)                                   # each head's T probabilities sum to s
