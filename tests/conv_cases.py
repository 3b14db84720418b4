"""Shared pieces of the rectangular convolution tests (test_conv_cases_cpu.py, test_conv_rect_gpu.py): exact operands for the
3x3 convolution in every form the engine launches it, the fp64 reference, NaN-guarded NHWC inputs, a restatement of the halo
planner's three-way split, and the fixed geometry list.  The launch, the frames and the comparison are gemm_cases.py's.

Exact data   exact_conv(): ternary NHWC sources and ternary weights [cout][9 * (c0 + c1) (+ tail columns)] in the engine's KRSC
             order, bias / bias2 / row bias / residual integers in [-8, 8]: with 9 * (c0 + c1) + tail <= 1600 every partial sum
             in any tap order and any split-K slab is an integer below 2048, exact in fp16, so the kernel's output must EQUAL
             ref_conv (gemm_cases.check_equal) and one wrong, missing or doubled tap is a failure.
             exact_conv_u8(): codes over 0..255 with exact_u8's offsets and scale 1; the image holds one +-1 at a random channel
             of one random pixel per aligned 2x2 cell, so a 3x3 window sees at most four nonzeros (|sum| <= 1020; a nearest-2x
             window repeats a source pixel up to four times -- assert_exact on the reference is the arbiter there).
ref_conv     fp64 F.conv2d on the CPU: stride 1 / 2, pad_mode 1 (F.pad(x, (0, 1, 0, 1)) then pad 0), nearest-2x upsampling,
             the two-source concat, the row bias per image, the residual and the fused 1x1 tail with bias2.  It runs through
             gemm_cases.assert_exact before anything is launched.
guarded_nhwc the batch inside one allocation with at least W + 2 pixels of NaN in front of image 0 and behind the last image: a
             tap that reads above row 0 of image 0 or below the last row of the last image instead of the zero padding turns the
             output non-finite; neighbouring images are independent random data, so a tap that leaks across an image boundary
             breaks equality.
halo_branch  which of halo_geometry()'s branches (gemm.hip) a BM-row tile takes on an (h, w) image: 'segment' (W >= BM: a tile
             is a piece of one image row), 'rows' (BM / W <= H: whole image rows of one image), 'images' (BM / W > H: whole
             images, `parts` of them) or None (the arithmetic declines).  halo_takes() adds the patch's DMA rounds.
RECTS        the fixed geometry list (n, h, w); RECTS_UPS the upsampling sources; RECTS_ENGINE the engine's own rectangles."""
import functools

import torch
import torch.nn.functional as F

import gemm_cases as gc

HALO_TILES = list(range(37, 46)) + [49, 50, 51, 52]
# patch DMA rounds (256 lanes x 16 bytes = 32 pixels of 64 channels each) a tile of BM rows provides: gemm.hip, halo_nrmax
HALO_NRMAX = {64: 7, 96: 10, 128: 9, 192: 13, 256: 13}
BRANCHES = ('segment', 'rows', 'images')

# (a) the smallest shapes per branch.  The three of the fourth line are additions the coverage conditions of test_conv_cases_cpu.py demanded:
# no shape of the starting set puts a 64-row tile into 'images' (64 / W > H needs W in {8, 16} with H <= 4) and only one puts a
# 256-row tile there ((3, 4, 32)); (3, 2, 16), (3, 4, 8) and (3, 8, 16) do
RECTS = [(2, 8, 12), (2, 12, 8), (2, 16, 24), (2, 24, 16), (3, 5, 9), (1, 9, 5),
         (3, 4, 16), (3, 4, 12), (3, 2, 24), (3, 4, 24), (3, 4, 32), (2, 8, 32), (2, 32, 8),
         (2, 16, 32), (2, 8, 48), (1, 12, 16),
         (3, 2, 16), (3, 4, 8), (3, 8, 16),
         (1, 8, 64), (1, 4, 128), (1, 2, 256), (1, 4, 96), (1, 2, 192), (1, 72, 64)]
RECTS_SEGMENT = RECTS[-6:]                   # W >= 64: the row-segment shapes (the implicit-GEMM sweeps leave them out)
RECTS_IMPLICIT_ONLY = [(3, 5, 9), (1, 9, 5), (1, 5, 3)]      # no halo tile divides them
# upsampling sources (the output is 2h x 2w).  The last three are additions: the starting set gives the 64- and 128-row tiles
# no output whose width divides them (8x16: 'rows' on both; 4x8: 'images') and the 256-row tiles no 'rows' output (8x32)
RECTS_UPS = [(2, 4, 6), (2, 6, 4), (3, 2, 6), (1, 5, 3), (2, 8, 12), (2, 4, 48), (3, 4, 8), (3, 2, 4), (2, 4, 16)]
# (b) the engine's own rectangles, thin channels
RECTS_ENGINE = [(2, 64, 96), (2, 96, 64), (2, 32, 48), (2, 48, 32), (1, 128, 192)]
RECTS_ENGINE_UPS = [(2, 32, 48), (2, 48, 32)]
# everything a ResBlock asks: four shapes of the 96- / 192-row tiles, and three on which the 64- / 128- / 256-row tiles (which divide none of the
# four) reach 'images' ((3, 4, 8): 64 and 128 rows; (3, 4, 32): 256 rows) and 'rows' ((3, 4, 32); (2, 8, 32): 256 rows)
RECTS_RESBLOCK = [(2, 8, 12), (2, 12, 8), (3, 4, 12), (2, 16, 24), (3, 4, 8), (3, 4, 32), (2, 8, 32)]


# ----------------------------------------------------------------------------------------------------------- the planner
def halo_split(bm, h, w, ups=False):
    """(branch, tw, th, parts) of halo_geometry() on the OUTPUT size, or None where its arithmetic declines"""
    H, W = h << int(ups), w << int(ups)
    if W >= bm:
        if W % bm:
            return None
        branch, tw, th, parts = 'segment', bm, 1, 1
    else:
        if bm % W:
            return None
        tw, rows = W, bm // W
        if rows <= H:
            if H % rows:
                return None
            branch, th, parts = 'rows', rows, 1
        else:
            if rows % H:
                return None
            branch, th, parts = 'images', H, rows // H
    if ups and ((th > 1 and th % 2) or tw % 2):
        return None
    return branch, tw, th, parts


def halo_branch(bm, h, w, ups=False):
    s = halo_split(bm, h, w, ups)
    return s[0] if s else None


def halo_patch_pixels(bm, h, w, ups=False):
    """pixels of the LDS patch (zero halo included; cut from the SOURCE image under upsampling), or None"""
    s = halo_split(bm, h, w, ups)
    if s is None:
        return None
    _, tw, th, parts = s
    return parts * ((th // 2 if ups else th) + 2) * ((tw // 2 if ups else tw) + 2)


def halo_takes(bm, h, w, ups=False):
    """the branch if a BM-row tile takes the geometry (the split works out AND the patch fits the tile's DMA rounds), else None"""
    px = halo_patch_pixels(bm, h, w, ups)
    if px is None or (px * 8 + 255) // 256 > HALO_NRMAX[bm]:
        return None
    return halo_branch(bm, h, w, ups)


def conv_desc(n, h, w, c0, cout, c1=0, ups=False, stride=1, tile=0, split=0):
    """a convolution descriptor with fake (never dereferenced) pointers, for the host-only planning calls"""
    from sdod.amd._lib import GemmDesc
    d = GemmDesc()
    d.a = d.w = d.out = 0x1000
    d.a2 = 0x1000 if c1 else None
    d.a_mode = 1; d.ksize = 3; d.stride = stride; d.upsample = 1 if ups else 0
    d.n_img, d.h_in, d.w_in, d.c0, d.c1 = n, h, w, c0, c1
    ho, wo = (h << int(ups)) // stride, (w << int(ups)) // stride
    d.M, d.N, d.K = n * ho * wo, cout, 9 * (c0 + c1)
    d.ldw, d.ldo = d.K, cout
    d.tile, d.split_k = tile, split
    return d


def halo_ok(tile, n, h, w, ups=False, c0=64, cout=64):
    """the library's own answer (sdod_gemm_halo_ok: the predicate the launch uses; host-only)"""
    import ctypes
    from sdod.amd import _lib
    return _lib.hip().sdod_gemm_halo_ok(ctypes.byref(conv_desc(n, h, w, c0, cout, ups=ups)), tile) == 1


# ------------------------------------------------------------------------------------------------------------ exact data
def out_size(h, w, stride=1, pad_mode=0, ups=False):
    hu, wu = h << int(ups), w << int(ups)
    pad_sum = 1 if pad_mode else 2
    return (hu + pad_sum - 3) // stride + 1, (wu + pad_sum - 3) // stride + 1


def exact_conv(n, h, w, c0, c1, cout, seed, tail=None, stride=1, pad_mode=0, ups=False):
    """dict of CPU operands: x0 [n][h][w][c0], x1 (c1 > 0), w [cout][9 * (c0 + c1) + tail columns], bias, bias2 (tail), row_bias
    [n][cout] (every image its own row of distinct integers), residual [n][ho][wo][cout], t0 / t1 (tail = (tc0, tc1): the 1x1
    tail's NHWC sources at the OUTPUT size)"""
    tc0, tc1 = tail or (0, 0)
    k = 9 * (c0 + c1) + tc0 + tc1
    assert c0 + c1 <= 128 and tc0 + tc1 <= 128 and k <= 1600, (c0, c1, tail)
    gen = torch.Generator().manual_seed(seed)
    ho, wo = out_size(h, w, stride, pad_mode, ups)
    d = dict(x0=gc.ternary((n, h, w, c0), gen), x1=gc.ternary((n, h, w, c1), gen) if c1 else None, w=gc.ternary((cout, k), gen),
             bias=gc.small_ints((cout,), gen, torch.float32), bias2=gc.small_ints((cout,), gen, torch.float32) if tail else None,
             residual=gc.small_ints((n, ho, wo, cout), gen),
             t0=gc.ternary((n, ho, wo, tc0), gen) if tc0 else None, t1=gc.ternary((n, ho, wo, tc1), gen) if tc1 else None)
    # row bias: image i gets the integers (j + 5 * i) % 17 - 8 shuffled by one permutation of the columns: no two images agree
    # in any column, so a tile that applies image 0's row to image 1 differs everywhere
    perm = torch.randperm(cout, generator=gen)
    d['row_bias'] = torch.stack([((perm + 5 * i) % 17 - 8) for i in range(n)]).half()
    return d


def exact_conv_u8(n, h, w, c0, c1, cout, seed):
    """uint8-weight operands: x0 / x1 sparse (one +-1 per aligned 2x2 cell, over the concatenated channels), codes q
    [cout][9 * (c0 + c1)], w_scale = 1, w_off = offset + 128, wf the dequantised integer weights, bias, row_bias, residual"""
    gen = torch.Generator().manual_seed(seed)
    cin = c0 + c1
    x = torch.zeros(n, h, w, cin)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    dy = torch.randint(0, 2, (n, ch, cw), generator=gen); dx = torch.randint(0, 2, (n, ch, cw), generator=gen)
    chan = torch.randint(0, cin, (n, ch, cw), generator=gen); sign = torch.randint(0, 2, (n, ch, cw), generator=gen).float() * 2 - 1
    yy = (2 * torch.arange(ch)[None, :, None] + dy).clamp(max=h - 1); xx = (2 * torch.arange(cw)[None, None, :] + dx).clamp(max=w - 1)
    x[torch.arange(n)[:, None, None].expand_as(yy), yy, xx, chan] = sign
    k = 9 * cin
    q = torch.randint(0, 256, (cout, k), generator=gen, dtype=torch.uint8)
    r = torch.arange(cout) % 3
    offset = torch.where(r == 0, torch.tensor(-128.0), torch.where(r == 1, torch.tensor(-101.0), torch.tensor(0.0)))
    perm = torch.randperm(cout, generator=gen)
    return dict(x0=x[..., :c0].contiguous().half(), x1=x[..., c0:].contiguous().half() if c1 else None, q=q, w_scale=torch.ones(cout),
                w_off=(offset + 128).float(), wf=q.double() + offset.double()[:, None], bias=gc.small_ints((cout,), gen, torch.float32),
                row_bias=torch.stack([((perm + 5 * i) % 17 - 8) for i in range(n)]).half(), residual=None)


def ref_conv(x0, w, bias=None, *, x1=None, stride=1, pad_mode=0, ups=False, row_bias=None, residual=None, tail=None, bias2=None):
    """fp64 reference [n * ho * wo][cout]: conv3x3([x0 | x1]) + bias + row_bias[image] + residual + [t0 | t1] . w_tail^T + bias2;
    w = [cout][9 * cin (+ tail columns)] with the 3x3 part in (ky, kx, channel) order.  Checked for exactness before it returns."""
    x = (x0 if x1 is None else torch.cat([x0, x1], -1)).double().permute(0, 3, 1, 2)      # NCHW: dim 2 = h (rows), dim 3 = w
    cout, cin = w.shape[0], x.shape[1]
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode='nearest')
    if pad_mode:
        x = F.pad(x, (0, 1, 0, 1))           # one column on the right, one row at the bottom
    w3 = w[:, :9 * cin].double().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    y = F.conv2d(x, w3, None if bias is None else bias.double(), stride=stride, padding=0 if pad_mode else 1).permute(0, 2, 3, 1)
    if row_bias is not None:
        y = y + row_bias.double()[:, None, None, :]
    if residual is not None:
        y = y + residual.double()
    if tail is not None:
        t = torch.cat([s for s in tail if s is not None], -1).double()
        assert t.shape[:3] == y.shape[:3] and w.shape[1] == 9 * cin + t.shape[-1]
        y = y + t @ w[:, 9 * cin:].double().t()
        if bias2 is not None:
            y = y + bias2.double()
    y = y.reshape(-1, cout).contiguous()
    gc.assert_exact(y)
    return y


@functools.lru_cache(None)
def conv_case(n, h, w, c0, c1, cout, seed, form='plain', stride=1, pad_mode=0, ups=False):
    """(operands, fp64 reference) of one form, computed once and shared: 'plain' (bias only), 'resblock' (concat + row bias +
    residual), 'tail' (3x3 on x0, 1x1 tail on (c0, c1) sources of their own, bias2); callers must not modify what they get"""
    if form == 'tail':
        d = exact_conv(n, h, w, c0, 0, cout, seed, tail=(64, 64))
        return d, ref_conv(d['x0'], d['w'], d['bias'], tail=(d['t0'], d['t1']), bias2=d['bias2'])
    d = exact_conv(n, h, w, c0, c1, cout, seed, stride=stride, pad_mode=pad_mode, ups=ups)
    if form == 'resblock':
        return d, ref_conv(d['x0'], d['w'], d['bias'], x1=d['x1'], row_bias=d['row_bias'], residual=d['residual'])
    return d, ref_conv(d['x0'], d['w'], d['bias'], x1=d['x1'], stride=stride, pad_mode=pad_mode, ups=ups)


@functools.lru_cache(None)
def conv_case_u8(n, h, w, c0, c1, cout, seed, ups=False, row_bias=False):
    d = exact_conv_u8(n, h, w, c0, c1, cout, seed)
    return d, ref_conv(d['x0'], d['wf'], d['bias'], x1=d['x1'], ups=ups, row_bias=d['row_bias'] if row_bias else None)


# ---------------------------------------------------------------------------------------------------------------- guards
def guarded_nhwc(x, device=None):
    """x [n][h][w][c] on the device, inside one allocation with w + 2 pixels of NaN in front of and behind the batch"""
    n, h, w, c = x.shape
    guard = w + 2
    buf = torch.full(((2 * guard + n * h * w) * c,), float('nan'), dtype=torch.float16, device=device or gc.dev())
    view = buf[guard * c:(guard + n * h * w) * c].view(n, h, w, c)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    view._guard_buf = buf                    # (keeps the allocation's name for guards_intact)
    return view


def guards_intact(view):
    n, h, w, c = view.shape
    g = (w + 2) * c
    buf = view._guard_buf
    assert torch.isnan(buf[:g]).all() and torch.isnan(buf[-g:]).all(), 'the NaN guards around an input changed'
