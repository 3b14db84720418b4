"""The GEMM at the strides, aliasing and tile edges the engine runs it with (gemm.hip; helper: tests/gemm_cases.py).

a. The engine's forms, at C = 320 and a ragged 200 rows: attn2.to_out into columns 4C..5C of a [rows][5C] buffer (ldo = 5C,
   ldr = C), its per-image-weight variant (2 x 96 rows, K = 640), the GEGLU projection with the LayerNorm fold reading those
   columns and writing columns 0..4C of the SAME rows, the composed K = 5C Linear, the VAE's score GEMM over two column ranges
   of one buffer (lda = ldw = 2C, alpha = C^-1/2) and its V^T product (bias_on_m), weights inside a wider matrix, and the
   convolution with the time-embedding row bias at a column offset of a wider matrix and a weight with ldw > K.  Every form
   runs on the tiles the shipped tune table picks for that kind of key plus one tile per kernel family, and must give the bits
   of the dense contiguous call on the same tile, leave its frame untouched, and match fp64: exactly where the data can be
   exact, within this suite's tolerances (2e-3; 3e-3 with the LayerNorm fold) otherwise.
b. Edges of every register-staged, ring and A-panel tile of the table on exact data and framed operands: M and N around the
   tile, K around the ring depth, the full epilogue with a row bias whose image size divides nothing, bias_on_m, a ragged
   split-K, and the uint8 forms.  What a tile cannot run is asserted as a refusal (host-only calls), never skipped.
c. A ledger: every (tile, uint8?) the shipped table picks and every tuned non-halo tile has run with the plan confirming it.
   (Halo-patch tiles keep their own ledger in test_kernels_gpu.py; here they only run the two convolution forms.)"""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc
from gemm_cases import Framed, check_close, check_equal, dev, framed_in, framed_out, framed_res, run_gemm

pytestmark = pytest.mark.gpu

C = 320
ROWS = 200        # short of 2 x 128, no multiple of 32, 64 or 128
REPS = dict(reg=3, ring4=8, ring8=9, lean=23, ksub2=32, rows32=46, panel=53)   # one tile per kernel family


def tiles_for(reps=(), **key):
    """the table's picks for keys of that kind plus the named family representatives, halo tiles left out"""
    ts = set(gc.picked_tiles(a_mode=0, **key)) | {REPS[r] for r in reps}
    return sorted(t for t in ts if gc.tile_info(t)['family'] != 'halo')


def same_bits(strided, dense, name):
    assert torch.isfinite(strided).all(), f'{name}: non-finite output'
    assert torch.equal(strided.cpu(), dense.cpu()), f'{name}: differs from the dense call of the same tile'


# ------------------------------------------------------------------------------------------------ a. the engine's forms
@functools.lru_cache(None)
def _to_out_data():
    a, w, gen = gc.exact_f16(ROWS, C, C, 500)
    bias = gc.small_ints((C,), gen, torch.float32); res = gc.small_ints((ROWS, C), gen)
    ref = gc.ref_rows(a, w, bias, residual=res)
    gc.assert_exact(ref)
    return a, w, bias, res, ref


@pytest.mark.parametrize('tile', tiles_for(('reg', 'ring4', 'ring8', 'lean', 'ksub2', 'rows32', 'panel'), residual=True, u8=False, per_image=False))
def test_to_out_into_the_wide_buffer(tile):
    """attn2.to_out -> t2c: ldr = C, ldo = 5C at column 4C"""
    a, w, bias, res, ref = _to_out_data()
    d = dev()
    dense, _, _ = run_gemm(a.to(d), w.to(d), bias.to(d), residual=res.to(d), tile=tile, tag='form:to_out')
    check_equal(dense, ref, f'to_out dense tile{tile}')
    fa, fw, fr, fo = framed_in(a, C), framed_in(w, C), framed_res(res, C), framed_out(ROWS, C, 5 * C, 4 * C)
    run_gemm(fa.view, fw.view, bias.to(d), residual=fr.view, out=fo.view, tile=tile, tag='form:to_out')
    same_bits(fo.view, dense, f'to_out tile{tile}')
    fo.frame_intact(f'to_out tile{tile}'); fr.frame_intact('residual')


@functools.lru_cache(None)
def _per_image_data():
    k, rpi = 640, 96
    a, _, gen = gc.exact_f16(2 * rpi, 1, k, 510)
    w = gc.ternary((2, C, k), gen)
    bias = gc.small_ints((C,), gen, torch.float32); res = gc.small_ints((2 * rpi, C), gen)
    ref = torch.cat([gc.ref_rows(a[i * rpi:(i + 1) * rpi], w[i], bias, residual=res[i * rpi:(i + 1) * rpi]) for i in range(2)])
    gc.assert_exact(ref)
    return a, w, bias, res, ref


@pytest.mark.parametrize('tile', sorted(set(gc.picked_tiles(a_mode=0, per_image=True, softmax=False)) | {27, 46, 47, 48, 56, 59}))
def test_per_image_weights_into_the_wide_buffer(tile):
    """the folded cross-attention's second GEMM: per-image weights, K = 640, 2 images x 96 rows (a multiple of 32, not of 64)"""
    a, w, bias, res, ref = _per_image_data()
    d = dev()
    info = gc.tile_info(tile)
    # make_plan: a tile must not straddle two weight matrices -- ring tiles whose rows divide the image run, the rest go to 46
    runs_on = tile if info['family'] == 'ring' and 96 % info['bm'] == 0 else 46
    kw = dict(rows_per_img=96, tile=tile, runs_on=runs_on, tag='form:per_image')
    dense, _, _ = run_gemm(a.to(d), w.to(d), bias.to(d), residual=res.to(d), **kw)
    check_equal(dense, ref, f'per-image dense tile{tile}')
    fa, fr, fo = framed_in(a, 640), framed_res(res, C), framed_out(2 * 96, C, 5 * C, 4 * C)
    run_gemm(fa.view, w.to(d), bias.to(d), residual=fr.view, out=fo.view, **kw)
    same_bits(fo.view, dense, f'per-image tile{tile}')
    fo.frame_intact(f'per-image tile{tile}'); fr.frame_intact('residual')


@functools.lru_cache(None)
def _geglu_ln_data():
    from sdod.amd import ops
    g = torch.Generator().manual_seed(520)
    H = 4 * C
    x = (torch.randn(ROWS, C, generator=g) * 2 + torch.randn(ROWS, 1, generator=g) * 3).half()
    w = (torch.randn(2 * H, C, generator=g) * C ** -0.5).half(); b = torch.randn(2 * H, generator=g)
    gamma = 1 + 0.2 * torch.randn(C, generator=g); beta = 0.3 * torch.randn(C, generator=g)
    y = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5) @ w.double().t() + b.double()
    ref = y[:, :H] * F.gelu(y[:, H:])
    perm = gc.geglu_perm(H)
    d = dev()
    wf, s, t = ops.ln_fold(w[perm].contiguous().to(d), gamma.to(d), beta.to(d), b[perm].contiguous().to(d))
    return x, wf, s, t, ref


@pytest.mark.parametrize('tile', tiles_for(('reg', 'ring4', 'ring8', 'lean', 'ksub2', 'rows32', 'panel'), geglu=True, ln=True, u8=False, strided=True))
def test_geglu_with_ln_fold_in_place(tile):
    """ff.net.0.proj: A = columns 4C..5C (lda = 5C), out = columns 0..4C of the same rows (ldo = 5C), N = 8C, the LayerNorm
    statistics gathered over a strided row"""
    x, wf, s, t, ref = _geglu_ln_data()
    d = dev()
    runs_on = 14 if gc.tile_info(tile)['family'] == 'reg' else tile      # make_plan: fusions live in the LDS-DMA families
    kw = dict(ln_s=s, geglu=True, tile=tile, runs_on=runs_on, tag='form:geglu_ln')
    dense, _, _ = run_gemm(x.to(d), wf, t, **kw)
    check_close(dense, ref, 3e-3, f'geglu + ln dense tile{tile}')
    cat = Framed(ROWS, 5 * C, 5 * C)
    cat.view[:, 4 * C:] = x.to(d)
    a_view, out_view = cat.view[:, 4 * C:], cat.view[:, :4 * C]
    for i in range(3):
        out_view.fill_(float('nan'))
        run_gemm(a_view, wf, t, out=out_view, **kw)
        same_bits(out_view, dense, f'geglu + ln in place tile{tile} launch {i}')
        assert torch.equal(a_view.cpu().view(torch.int16), x.view(torch.int16)), 'the input columns 4C..5C changed'
        cat.frame_intact(f'geglu + ln tile{tile}')


@functools.lru_cache(None)
def _composed_data():
    a, w, gen = gc.exact_f16(ROWS, C, 5 * C, 530)
    bias = gc.small_ints((C,), gen, torch.float32); res = gc.small_ints((ROWS, C), gen)
    ref = gc.ref_rows(a, w, bias, residual=res)
    gc.assert_exact(ref)
    return a, w, bias, res, ref


@pytest.mark.parametrize('tile', tiles_for(('reg', 'ring4', 'ring8', 'lean', 'ksub2', 'rows32'), residual=True, u8=False, per_image=False))
def test_composed_linear_over_the_wide_buffer(tile):
    """ff.net.2 + proj_out composed: K = 5C over the [rows][5C] buffer, with a residual"""
    a, w, bias, res, ref = _composed_data()
    d = dev()
    dense, _, _ = run_gemm(a.to(d), w.to(d), bias.to(d), residual=res.to(d), tile=tile, tag='form:composed')
    check_equal(dense, ref, f'composed dense tile{tile}')
    fa, fw, fr, fo = framed_in(a, 5 * C), framed_in(w, 5 * C), framed_res(res, C), framed_out(ROWS, C, C)
    run_gemm(fa.view, fw.view, bias.to(d), residual=fr.view, out=fo.view, tile=tile, tag='form:composed')
    same_bits(fo.view, dense, f'composed tile{tile}')
    fo.frame_intact(f'composed tile{tile}'); fr.frame_intact('residual')


def test_composed_linear_is_refused_by_the_panel_tiles():
    """K = 5C: a 32-row panel is 100 KB next to a 64 KB ring"""
    d = gc.rows_desc(ROWS, C, 5 * C, residual=0x1000, ldr=C)
    assert not any(gc.panel_ok(d, t) for t in (53, 54, 55))
    assert gc.panel_ok(gc.rows_desc(ROWS, C, C, residual=0x1000, ldr=C), 53)


@functools.lru_cache(None)
def _scores_data():
    g = torch.Generator().manual_seed(540)
    qk = torch.randn(ROWS, 2 * C, generator=g).half()
    return qk, C ** -0.5 * (qk[:, :C].double() @ qk[:, C:].double().t())


@pytest.mark.parametrize('tile', tiles_for(('reg', 'ring4', 'ring8', 'lean', 'ksub2', 'rows32', 'panel'), residual=False, u8=False, per_image=False,
                                           geglu=False, ln=False, softmax=False))
def test_vae_scores_from_two_column_ranges_of_one_buffer(tile):
    """VAE attention scores: A = columns 0..C and W = columns C..2C of one qk buffer (lda = ldw = 2C), alpha = C^-1/2"""
    qk, ref = _scores_data()
    d = dev()
    alpha = C ** -0.5
    dense, _, _ = run_gemm(qk[:, :C].contiguous().to(d), qk[:, C:].contiguous().to(d), alpha=alpha, tile=tile, tag='form:vae_scores')
    check_close(dense, ref, 2e-3, f'vae scores dense tile{tile}')
    fq, fo = framed_in(qk, 2 * C), framed_out(ROWS, ROWS, ROWS + 8)
    run_gemm(fq.view[:, :C], fq.view[:, C:], alpha=alpha, out=fo.view, tile=tile, tag='form:vae_scores')
    same_bits(fo.view, dense, f'vae scores tile{tile}')
    fo.frame_intact(f'vae scores tile{tile}')


@functools.lru_cache(None)
def _vt_data():
    wv, g_b, gen = gc.exact_f16(C, ROWS, C, 550)       # "A" is the weight Wv [C][C], "W" the activations g_b [L][C]
    bias = gc.small_ints((C,), gen, torch.float32)
    ref = gc.ref_rows(wv, g_b, bias, bias_on_m=True)
    gc.assert_exact(ref)
    return wv, g_b, bias, ref


@pytest.mark.parametrize('tile', tiles_for(('reg', 'ring4', 'ring8', 'lean', 'ksub2', 'rows32'), residual=False, u8=False, per_image=False,
                                           geglu=False, ln=False, softmax=False))
def test_vae_v_transposed_product(tile):
    """V^T [C][L] = Wv . g_b^T + bv: bias indexed by the output row, an activation matrix as the weight operand"""
    wv, g_b, bias, ref = _vt_data()
    d = dev()
    dense, _, _ = run_gemm(wv.to(d), g_b.to(d), bias.to(d), bias_on_m=True, tile=tile, tag='form:vae_vt')
    check_equal(dense, ref, f'V^T dense tile{tile}')
    fa, fw, fo = framed_in(wv, C), framed_in(g_b, C), framed_out(C, ROWS, ROWS + 8)
    run_gemm(fa.view, fw.view, bias.to(d), bias_on_m=True, out=fo.view, tile=tile, tag='form:vae_vt')
    same_bits(fo.view, dense, f'V^T tile{tile}')
    fo.frame_intact(f'V^T tile{tile}')


def test_bias_on_m_is_refused_by_the_panel_tiles():
    from sdod.amd import _lib
    wv, g_b, bias, _ = _vt_data()
    d = dev()
    assert not gc.panel_ok(gc.rows_desc(C, ROWS, C, bias_on_m=1, bias=0x1000), 53)
    with pytest.raises(_lib.SdodError):
        run_gemm(wv.to(d), g_b.to(d), bias.to(d), bias_on_m=True, tile=53, tag='refused')


@functools.lru_cache(None)
def _wide_weight_data():
    a, wide, gen = gc.exact_f16(ROWS, C, 5 * C, 560)
    a = a[:, :C].contiguous()
    bias = gc.small_ints((C,), gen, torch.float32)
    ref = gc.ref_rows(a, wide[:, 4 * C:], bias)
    gc.assert_exact(ref)
    return a, wide, bias, ref


@pytest.mark.parametrize('tile', tiles_for(('reg', 'ring4', 'ring8', 'lean', 'ksub2', 'rows32', 'panel'), residual=False, u8=False, per_image=False,
                                           geglu=False, ln=False, softmax=False, strided=True))
def test_weight_inside_a_wider_matrix(tile):
    """Param::ld > 0: the weight is columns 4C..5C of a [C][5C] matrix (ldw = 5C), as the composed Linear's second block is"""
    a, wide, bias, ref = _wide_weight_data()
    d = dev()
    dense, _, _ = run_gemm(a.to(d), wide[:, 4 * C:].contiguous().to(d), bias.to(d), tile=tile, tag='form:wide_w')
    check_equal(dense, ref, f'wide weight dense tile{tile}')
    fa, fw, fo = framed_in(a, C + 8), framed_in(wide, 5 * C), framed_out(ROWS, C, C + 8)
    run_gemm(fa.view, fw.view[:, 4 * C:], bias.to(d), out=fo.view, tile=tile, tag='form:wide_w')
    same_bits(fo.view, dense, f'wide weight tile{tile}')
    fo.frame_intact(f'wide weight tile{tile}')


@functools.lru_cache(None)
def _conv_data():
    n, hw, cin, cout = 2, 16, 64, 136
    gen = torch.Generator().manual_seed(570)
    x = gc.ternary((n, hw, hw, cin), gen)
    wide = gc.ternary((cout, 9 * cin + 64), gen)                 # [cout][9 * cin + skip columns]: the conv-plus-skip matrix
    emb = gc.small_ints((n, 400), gen)                           # [B][sum of cout]: this layer's slice starts at column 128
    bias = gc.small_ints((cout,), gen, torch.float32); res = gc.small_ints((n, hw, hw, cout), gen)
    w = wide[:, :9 * cin]
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), bias.double(), padding=1).permute(0, 2, 3, 1)
    ref = (y + emb[:, 128:128 + cout].double()[:, None, None, :] + res.double()).reshape(n * hw * hw, cout)
    gc.assert_exact(ref)
    return x, wide, emb, bias, res, ref


@pytest.mark.parametrize('tile', [27, 28, 38, 44])
def test_conv_row_bias_and_weight_inside_wider_matrices(tile):
    """ResBlock in_layers conv: the time-embedding row bias at a column offset of the [B][sum cout] matrix (ld_row_bias > N) and
    the weight as the first 9 * cin columns of the conv-plus-skip matrix (ldw > K): an im2col ring tile and a halo-patch tile.
    The output [M][cout] and the residual sit in frames of their own, with ldr != ldo"""
    x, wide, emb, bias, res, ref = _conv_data()
    d = dev()
    cout, k = wide.shape[0], wide.shape[1] - 64
    kw = dict(conv=dict(stride=1), rows_per_img=256, tile=tile, split_k=1, tag='form:conv_row_bias')
    dense, _, _ = run_gemm(x.to(d), wide[:, :k].contiguous().to(d), bias.to(d), row_bias=emb[:, 128:128 + cout].contiguous().to(d),
                           residual=res.to(d), **kw)
    check_equal(dense.reshape(-1, cout), ref, f'conv dense tile{tile}')
    fw, fe = framed_in(wide, wide.shape[1]), framed_in(emb, 400)
    fr, fo = framed_res(res.reshape(-1, cout), cout + 24, 8), framed_out(ref.shape[0], cout, cout + 8)
    run_gemm(x.to(d), fw.view[:, :k], bias.to(d), row_bias=fe.view[:, 128:128 + cout], residual=fr.view, out=fo.view, **kw)
    same_bits(fo.view, dense.reshape(-1, cout), f'conv tile{tile}')
    fo.frame_intact(f'conv tile{tile}'); fr.frame_intact('residual')


# ---------------------------------------------------------------------------------------- b. edges of every runnable tile
EDGE_TILES = [t for t in range(1, gc.num_tiles() + 1) if gc.tile_info(t)['family'] != 'halo']
U8_TILES = [t for t in EDGE_TILES if gc.tile_info(t)['family'] == 'ring' and gc.u8_tile(t) == t]


def _edge(tile, m, n, k, tag, seed, *, u8=False, epilogue=False, bias_on_m=False, split=1, rows_per_img=24):
    """one exact, fully framed launch on `tile`; where the A-panel kernel cannot run the case, the refusal is asserted"""
    from sdod.amd import _lib
    d = dev()
    info = gc.tile_info(tile)
    name = f'{tag} tile{tile} M{m} N{n} K{k}'
    kw = dict(tile=tile, split_k=split, tag=tag)
    if u8:
        a, q, scale, off, wf, gen = gc.exact_u8(m, n, k, seed)
        fw = framed_in(q, k + 16)
        kw.update(w_scale=scale.to(d), w_off=off.to(d))
    else:
        a, wf, gen = gc.exact_f16(m, n, k, seed)
        fw = framed_in(wf, k + 8)
    bias = gc.small_ints((m if bias_on_m else n,), gen, torch.float32)
    rb = res = None
    if epilogue:
        rb = gc.small_ints(((m + rows_per_img - 1) // rows_per_img, n), gen); res = gc.small_ints((m, n), gen)
    ref = gc.ref_rows(a, wf, bias, rb, rows_per_img, res, bias_on_m=bias_on_m)
    gc.assert_exact(ref)
    ld_n = (n + 7) // 8 * 8 + 8
    fa, fo = framed_in(a, k + 8), framed_out(m, n, ld_n)
    kw.update(out=fo.view, bias_on_m=bias_on_m)
    if epilogue:
        fr, fb = framed_res(res, ld_n + 16, 8), framed_res(rb, ld_n + 24, 16)      # ldr != ldo, row bias at a column offset
        kw.update(residual=fr.view, row_bias=fb.view, rows_per_img=rows_per_img)
    if info['family'] == 'panel':
        desc = gc.rows_desc(m, n, k, tile, split, lda=k + 8, ldw=k + 8, ldo=ld_n, bias_on_m=int(bias_on_m), row_bias=0x1000 if epilogue else None)
        if not gc.panel_ok(desc, tile):
            with pytest.raises(_lib.SdodError, match='A-panel'):
                run_gemm(fa.view, fw.view, bias.to(d), **kw)
            fo.frame_intact(name + ' (refused)')
            return
    _, _, splits = run_gemm(fa.view, fw.view, bias.to(d), **kw)
    if split > 1:
        assert splits == split and (k // 64) % ((k // 64 + split - 1) // split) != 0, (name, splits)     # really ragged
    check_equal(fo.view, ref, name)
    fo.frame_intact(name)
    if epilogue:
        fr.frame_intact(name + ' residual'); fb.frame_intact(name + ' row bias')


def _n_edges(info):
    n_min = 16 if info['bn'] == 16 else 8
    return sorted({n for n in (n_min, info['bn'] - 8, info['bn'] + 8, info['bn'] + 4) if n >= n_min})


def _k_edges(info):
    s = max(info['stages'], 2)
    ks = {1, s - 1, s, s + 1}
    if info['ksub'] == 2:
        ks |= {2 * s, 2 * s + 1}
    return sorted(ks)


@pytest.mark.parametrize('tile', EDGE_TILES)
def test_edges_m_and_n(tile):
    info = gc.tile_info(tile)
    k = 64 * max(info['stages'], 3)
    for m in (1, info['bm'] - 1, info['bm'] + 1):
        for n in _n_edges(info):
            _edge(tile, m, n, k, 'edge:mn', 1000 * tile + m + n)


@pytest.mark.parametrize('tile', EDGE_TILES)
def test_edges_k_against_the_ring_depth(tile):
    info = gc.tile_info(tile)
    for kt in _k_edges(info):
        _edge(tile, info['bm'] + 1, info['bn'] + 8, 64 * kt, 'edge:k', 2000 * tile + kt)


@pytest.mark.parametrize('tile', EDGE_TILES)
def test_edges_full_epilogue(tile):
    """bias + row bias + residual; images of 24 rows divide neither the tile's rows nor the 40 rows of the last m-tile"""
    info = gc.tile_info(tile)
    assert info['bm'] % 24 and 40 % 24
    _edge(tile, info['bm'] + 40, info['bn'] + 8, 64 * (max(info['stages'], 2) + 1), 'edge:epilogue', 3000 + tile, epilogue=True)


@pytest.mark.parametrize('tile', EDGE_TILES)
def test_edges_bias_on_m(tile):
    info = gc.tile_info(tile)
    _edge(tile, info['bm'] + 1, info['bn'] + 8, 192, 'edge:bias_on_m', 4000 + tile, bias_on_m=True)


@pytest.mark.parametrize('tile', EDGE_TILES)
def test_edges_split_k_with_a_ragged_last_slice(tile):
    """seven slabs in three slices: 3 + 3 + 1"""
    info = gc.tile_info(tile)
    _edge(tile, info['bm'] + 1, info['bn'] + 8, 7 * 64, 'edge:split_k', 5000 + tile, split=3, epilogue=True)


@pytest.mark.parametrize('tile', U8_TILES)
def test_edges_uint8_n(tile):
    info = gc.tile_info(tile)
    for n in _n_edges(info):
        _edge(tile, info['bm'] + 1, n, 64 * info['stages'], 'edge:u8_n', 6000 * tile + n, u8=True)


@pytest.mark.parametrize('tile', U8_TILES)
def test_edges_uint8_k(tile):
    info = gc.tile_info(tile)
    for kt in _k_edges(info):
        _edge(tile, info['bm'] + 1, info['bn'] + 8, 64 * kt, 'edge:u8_k', 7000 * tile + kt, u8=True, epilogue=(kt == info['stages']))


def test_uint8_tiles_are_the_ones_the_table_of_forms_says():
    assert U8_TILES == [8, 13, 23, 24, 27, 28, 29, 30, 31]
    assert all(gc.u8_tile(t) == 23 for t in EDGE_TILES if t not in U8_TILES and gc.tile_info(t)['family'] != 'panel')


# ------------------------------------------------------------------------------------------------------------ c. the ledger
def test_every_picked_and_every_tuned_tile_ran_with_the_plan_confirming_it():
    """after the tests above (same session): every (tile, uint8?) pair the shipped table picks -- a uint8 pick on a tile
    without a uint8 form counts as the tile the plan substitutes -- and every tuned non-halo tile; the untuned rows (4, 15,
    16) at least the plain M / N edges.  Halo-patch tiles have their own ledger (test_kernels_gpu.py)."""
    # only this module's launches count (tags 'form:...' / 'edge:...'): the ledger is shared with test_kernels_gpu.py, whose
    # launches must not stand in for these whichever file runs first
    ran = {}
    for (t, _, u8), tags in gc.LEDGER.items():
        mine = {g for g in tags if g.startswith(('form:', 'edge:'))}
        if mine:
            ran[(t, u8)] = mine
    want = set()
    for key, tile, _ in gc.table_picks():
        if gc.tile_info(tile)['family'] == 'halo':
            continue
        want.add((gc.u8_tile(tile), True) if key['u8'] else (tile, False))
    want |= {(t, False) for t in EDGE_TILES if t not in gc.UNTUNED}
    assert (24, False) in want and (53, False) in want and (61, False) in want and (23, True) in want
    missing = sorted(p for p in want if p not in ran)
    assert not missing, f'(tile, uint8) pairs that never ran: {missing}'
    for t in gc.UNTUNED:
        assert 'edge:mn' in ran.get((t, False), ()), f'untuned tile {t} did not run the plain edge cases'
    assert (24, True) in ran and (15, False) in ran
