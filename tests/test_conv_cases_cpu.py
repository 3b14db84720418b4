"""The recipes and the geometry list of tests/conv_cases.py, checked without a GPU: the exact data really is exact (fp32 sums
of the taps in several orders and split-K slabs equal the fp64 reference, with an independent index-by-index restatement of the
convolution that tells h from w), halo_branch() / halo_takes() agree with the library's own planner (sdod_gemm_halo_ok, a
host-only call), and the geometry list reaches every (halo tile, branch) pair the GPU file's ledger demands."""
import itertools

import pytest
import torch

import conv_cases as cc
import gemm_cases as gc


def _bm(tile):
    return gc.tile_info(tile)['bm']


# ------------------------------------------------------------------------------------------------------------ the recipes
def _tap_partials(x, w3, cin, stride, pad_mode, ups):
    """fp32 partial products [9][chunks][n * ho * wo][cout] of a 3x3 convolution written out index by index: output pixel (y, x)
    and tap (ky, kx) read the (upsampled) input at row y * stride + ky - pad, column x * stride + kx - pad; rows are compared
    with h and columns with w, nothing is shared with F.conv2d"""
    n, h, w, _ = x.shape
    ho, wo = cc.out_size(h, w, stride, pad_mode, ups)
    hu, wu = h << int(ups), w << int(ups)
    pad = 0 if pad_mode else 1
    cout = w3.shape[0]
    parts = torch.zeros(9, cin // 64, n * ho * wo, cout)
    ys, xs = torch.arange(ho), torch.arange(wo)
    for ky, kx in itertools.product(range(3), range(3)):
        iy, ix = ys * stride + ky - pad, xs * stride + kx - pad
        ok = ((iy >= 0) & (iy < hu))[:, None] & ((ix >= 0) & (ix < wu))[None, :]
        sy, sx = iy.clamp(0, hu - 1) >> int(ups), ix.clamp(0, wu - 1) >> int(ups)
        g = x.float()[:, sy][:, :, sx] * ok[None, :, :, None]                     # [n][ho][wo][cin]
        for c in range(cin // 64):
            wt = w3[:, (ky * 3 + kx) * cin + c * 64:(ky * 3 + kx) * cin + (c + 1) * 64].float()
            parts[ky * 3 + kx, c] = g[..., c * 64:(c + 1) * 64].reshape(-1, 64) @ wt.t()
    return parts


def _sum_in_orders(parts, extra):
    """the same fp32 terms added tap-major, chunk-major, backwards, and as three split-K slabs reduced afterwards"""
    terms = [parts[t, c] for t in range(9) for c in range(parts.shape[1])]
    chunk_major = [parts[t, c] for c in range(parts.shape[1]) for t in range(9)]
    sums = []
    for seq in (terms, chunk_major, terms[::-1]):
        acc = torch.zeros_like(terms[0])
        for t in seq:
            acc = acc + t
        sums.append(acc + extra)
    per = (len(chunk_major) + 2) // 3
    slabs = [torch.stack(chunk_major[i:i + per]).sum(0) for i in range(0, len(chunk_major), per)]
    sums.append(slabs[2] + slabs[0] + slabs[1] + extra)
    return sums


@pytest.mark.parametrize('n,h,w,stride,pad_mode,ups', [(2, 8, 12, 1, 0, False), (2, 12, 8, 1, 0, False), (3, 5, 9, 1, 0, False), (1, 9, 5, 2, 0, False),
                                                       (2, 8, 12, 2, 0, False), (2, 8, 12, 2, 1, False), (1, 9, 5, 2, 1, False), (2, 12, 8, 2, 1, False),
                                                       (2, 4, 6, 1, 0, True), (2, 6, 4, 1, 0, True), (1, 5, 3, 1, 0, True), (3, 2, 24, 1, 0, False)])
def test_exact_conv_recipe_in_any_order(n, h, w, stride, pad_mode, ups):
    d, ref = cc.conv_case(n, h, w, 128, 0, 72, 7000 + 100 * h + w, 'plain', stride, pad_mode, ups)
    assert ref.shape[0] == n * int.__mul__(*cc.out_size(h, w, stride, pad_mode, ups))
    parts = _tap_partials(d['x0'], d['w'], 128, stride, pad_mode, ups)
    for s in _sum_in_orders(parts, d['bias'].float()):
        assert torch.equal(s.double(), ref)
    assert float(ref.abs().max()) > 30          # the data is not degenerate


@pytest.mark.parametrize('n,h,w', [(2, 8, 12), (2, 12, 8), (3, 4, 12)])
def test_exact_resblock_and_tail_recipes(n, h, w):
    d, ref = cc.conv_case(n, h, w, 64, 64, 72, 7100 + w, 'resblock')
    x = torch.cat([d['x0'], d['x1']], -1)
    extra = (d['bias'].float() + d['row_bias'].float().repeat_interleave(h * w, 0)) + d['residual'].float().reshape(-1, 72)
    for s in _sum_in_orders(_tap_partials(x, d['w'], 128, 1, 0, False), extra):
        assert torch.equal(s.double(), ref)
    rb = d['row_bias']
    assert all((rb[i] != rb[j]).all() for i in range(n) for j in range(i)), 'two images share a row-bias entry'
    d, ref = cc.conv_case(n, h, w, 64, 0, 72, 7200 + w, 'tail')
    t = torch.cat([d['t0'], d['t1']], -1).float().reshape(-1, 128)
    extra = d['bias'].float() + d['bias2'].float() + t @ d['w'][:, 576:].float().t()
    for s in _sum_in_orders(_tap_partials(d['x0'], d['w'], 64, 1, 0, False), extra):
        assert torch.equal(s.double(), ref)


@pytest.mark.parametrize('n,h,w,ups', [(2, 8, 12, False), (3, 5, 9, False), (3, 4, 8, True), (2, 6, 4, True), (1, 12, 16, False)])
def test_exact_u8_recipe(n, h, w, ups):
    d, ref = cc.conv_case_u8(n, h, w, 64, 64, 40, 7300 + w, ups=ups, row_bias=True)
    x = torch.cat([d['x0'], d['x1']], -1)
    # one nonzero per aligned 2x2 cell: any 3x3 window holds at most four
    nz = (x != 0).sum(-1).float()[:, None]
    assert float(torch.nn.functional.avg_pool2d(nz, 3, 1, 1, divisor_override=1).max()) <= 4
    assert int((x != 0).sum()) == n * ((h + 1) // 2) * ((w + 1) // 2)
    assert int(d['q'].min()) == 0 and int(d['q'].max()) == 255
    extra = d['bias'].float() + d['row_bias'].float().repeat_interleave((h << int(ups)) * (w << int(ups)), 0)
    for s in _sum_in_orders(_tap_partials(x, d['wf'].float(), 128, 1, 0, ups), extra):
        assert torch.equal(s.double(), ref)


def test_guarded_nhwc_layout():
    x = gc.ternary((2, 3, 5, 64), torch.Generator().manual_seed(1))
    v = cc.guarded_nhwc(x, device='cpu')
    assert torch.equal(v, x) and v.is_contiguous()
    buf = v._guard_buf
    assert buf.numel() == (2 * 7 + 30) * 64 and torch.isnan(buf[:7 * 64]).all() and torch.isnan(buf[-7 * 64:]).all()
    assert v.data_ptr() - buf.data_ptr() == 7 * 64 * 2
    cc.guards_intact(v)


# ------------------------------------------------------------------------------------------------------------ the planner
ALL_PLAIN = cc.RECTS + cc.RECTS_ENGINE + [g for g in cc.RECTS_RESBLOCK if g not in cc.RECTS]
ALL_UPS = cc.RECTS_UPS + cc.RECTS_ENGINE_UPS


def test_halo_branch_agrees_with_the_library_planner():
    """halo_takes (the three-way split + the patch's DMA rounds) == sdod_gemm_halo_ok for every listed geometry x halo tile,
    plain and upsampling; with thin channels nothing else of halo_geometry() can decline (the LDS total is below 160 KiB for
    every tile of the table once the patch fits its rounds)"""
    assert sorted({_bm(t) for t in cc.HALO_TILES}) == sorted(cc.HALO_NRMAX)
    for tile in cc.HALO_TILES:
        for ups, geoms in ((False, ALL_PLAIN), (True, ALL_UPS)):
            for n, h, w in geoms:
                want = cc.halo_takes(_bm(tile), h, w, ups) is not None
                assert cc.halo_ok(tile, n, h, w, ups) == want, (tile, n, h, w, ups, cc.halo_split(_bm(tile), h, w, ups))
    # the shapes for the implicit-GEMM tiles only: no halo tile takes them, in either role
    for tile in cc.HALO_TILES:
        for n, h, w in cc.RECTS_IMPLICIT_ONLY:
            assert not cc.halo_ok(tile, n, h, w) and not cc.halo_ok(tile, n, h, w, True)


def test_halo_split_on_known_geometries():
    assert cc.halo_split(192, 8, 12) == ('images', 12, 8, 2)          # the deepest level of a 64x96 latent on a 192-row tile
    assert cc.halo_split(96, 8, 12) == ('rows', 12, 8, 1)
    assert cc.halo_split(96, 64, 96) == ('segment', 96, 1, 1)
    assert cc.halo_split(64, 96, 64) == ('segment', 64, 1, 1) and cc.halo_split(128, 96, 64) == ('rows', 64, 2, 1)
    assert cc.halo_split(64, 5, 9) is None and cc.halo_split(96, 2, 6, True) == ('images', 12, 4, 2)
    assert cc.halo_split(64, 3, 16, True) == ('rows', 32, 2, 1) and cc.halo_split(64, 3, 4, True) is None   # 6 rows % 8


# (tile rows, branch) pairs no geometry can reach, with the reason.  Everything else must be covered below.
UNREACHABLE = {
    (128, 'segment'): 'a row segment is 128 pixels wide: its patch is 3 x 130 = 390 pixels, the tile has 9 DMA rounds = 288',
    (192, 'segment'): 'patch 3 x 194 = 582 pixels against 13 rounds = 416',
    (256, 'segment'): 'patch 3 x 258 = 774 pixels against 13 rounds = 416',
}


def test_unreachable_pairs_are_unreachable():
    """'segment' fixes the tile at one image row of BM pixels whatever the image: 3 * (BM + 2) patch pixels, which only the 64-
    and 96-row tiles hold.  Checked on the arithmetic and on the library, for widths BM and 2 BM and several heights"""
    for (bm, branch), reason in UNREACHABLE.items():
        assert branch == 'segment' and 3 * (bm + 2) > 32 * cc.HALO_NRMAX[bm], reason
        for tile in (t for t in cc.HALO_TILES if _bm(t) == bm):
            for h, w in itertools.product((1, 2, 3, 8, 24), (bm, 2 * bm)):
                assert cc.halo_branch(bm, h, w) == 'segment' and cc.halo_takes(bm, h, w) is None and not cc.halo_ok(tile, 1, h, w)
    for bm in (64, 96):
        assert 3 * (bm + 2) <= 32 * cc.HALO_NRMAX[bm]


def coverage(geoms, ups):
    """{(tile, branch): [(n, h, w), ...]} accepted with h != w"""
    cov = {}
    for tile in cc.HALO_TILES:
        for n, h, w in geoms:
            b = cc.halo_takes(_bm(tile), h, w, ups)
            if b and h != w and cc.halo_ok(tile, n, h, w, ups):
                cov.setdefault((tile, b), []).append((n, h, w))
    return cov


def test_geometry_list_reaches_every_tile_and_branch():
    """the coverage conditions (conditions on the list, not measurements): per halo tile and reachable branch at least two
    accepted plain geometries with h != w; in 'rows' both orientations; at least one accepted upsampling geometry with h != w
    in 'rows' and one in 'images'.  The GPU file's closing ledger test demands that each of these pairs RAN."""
    plain, ups = coverage(cc.RECTS, False), coverage(cc.RECTS_UPS, True)
    for tile in cc.HALO_TILES:
        for branch in cc.BRANCHES:
            got = plain.get((tile, branch), [])
            if (_bm(tile), branch) in UNREACHABLE:
                assert not got, (tile, branch, got)
                continue
            assert len(got) >= 2, (tile, branch, got)
        rows = plain[(tile, 'rows')]
        assert any(h < w for _, h, w in rows) and any(h > w for _, h, w in rows), (tile, rows)
        assert ups.get((tile, 'rows')) and ups.get((tile, 'images')), (tile, ups.get((tile, 'rows')), ups.get((tile, 'images')))
    # odd batches with parts > 1: the last tile holds more image slots than the batch has
    assert any(n % 2 and cc.halo_split(_bm(t), h, w)[3] > 1 for (t, b), gs in plain.items() if b == 'images' for n, h, w in gs)


def test_resblock_geometries_reach_both_row_bias_paths():
    """per halo tile that can reach 'images': a ResBlock geometry there (tiles that span images: the per-row row-bias fallback)
    and one in 'rows' or 'segment' (a tile inside one image: rb_lds, where the tile has that path)"""
    cov = coverage(cc.RECTS_RESBLOCK, False)
    for tile in cc.HALO_TILES:
        assert cov.get((tile, 'images')), tile
        assert cov.get((tile, 'rows')) or cov.get((tile, 'segment')), tile
    # the deepest level of a 64x96 latent: 8x12 = 96 rows per image, a 192-row tile holds two images
    assert (2, 8, 12) in cov[(51, 'images')] and (2, 8, 12) in cov[(52, 'images')] and (2, 8, 12) in cov[(49, 'rows')]
