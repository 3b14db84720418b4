"""The circular border of seamless tiling (sdod_gemm_desc::pad_mode 2 / 3 / 4, sdod_conv_in_wrap_f16, sdod_im2col3x3_small_wrap_f16) in
every kernel that can run a 3x3 convolution, on exact data: the output must EQUAL test_tiling_cpu.ref_conv_wrap.

Launches go through gemm_cases.run_gemm (the plan confirms the tile that ran), read NaN-guarded NHWC inputs (conv_cases.guarded_nhwc:
a tap that reads outside its image instead of wrapping meets NaN; the neighbouring image is independent data, so a tap that wraps
into it breaks equality) and write framed outputs.

a. halo-patch tiles: conv_cases.RECTS under modes 2, 3 and 4, RECTS_UPS with upsampling under mode 2; a declined shape must be one
   conv_cases.halo_takes predicts; split-K with both reduce forms, the ResBlock form, the fused tail and uint8 weights; the closing
   test reads the ledger.
b. implicit-GEMM tiles (ring and register-staged): stride 1 down to the 1 x 2 and 2 x 1 images of the deepest level, stride 2 on odd
   sizes, upsampling, split-K, and the 3-channel output convolution's shape class.
c. the shift property, with no reference: conv(roll(x)) == roll(conv(x)) bit for bit along wrapped axes.
d. the input convolutions."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import gemm_cases as gc
from gemm_cases import check_close, check_equal, dev, framed_in, framed_out, framed_res, run_gemm
from test_conv_rect_gpu import COUT, IMPLICIT_TILES, Failures, fused_runs_on, plain_runs_on
from test_tiling_cpu import WRAP_MODES, pad_wrap, ref_conv_wrap

pytestmark = pytest.mark.gpu

RAN = {}                   # (halo tile, branch, ups, mode) -> set of (n, h, w, detail) that ran and passed
DECLINED = {}


# ---------------------------------------------------------------------------------------------------------------- staging
@functools.lru_cache(None)
def _case(kind, n, h, w, c0, c1, cout, seed, form, stride, ups, mode):
    """(operands, wrapped fp64 reference) of one case, computed once; callers must not modify what they get"""
    if kind == 'u8':
        d = cc.exact_conv_u8(n, h, w, c0, c1, cout, seed)
        return d, ref_conv_wrap(d['x0'], d['wf'], d['bias'], mode=mode, x1=d['x1'], ups=ups, row_bias=d['row_bias'] if form == 'rowbias' else None)
    if form == 'tail':
        d = cc.exact_conv(n, h, w, c0, 0, cout, seed, tail=(64, 64))
        return d, ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=mode, tail=(d['t0'], d['t1']), bias2=d['bias2'])
    d = cc.exact_conv(n, h, w, c0, c1, cout, seed, stride=stride, pad_mode=0, ups=ups)
    if form == 'resblock':
        return d, ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=mode, x1=d['x1'], row_bias=d['row_bias'], residual=d['residual'])
    return d, ref_conv_wrap(d['x0'], d['w'], d['bias'], mode=mode, x1=d['x1'], stride=stride, ups=ups)


@functools.lru_cache(None)
def _staged(key):
    """device copies of one case's inputs, made once: NaN-guarded NHWC sources, the weight in a NaN (255) frame"""
    d, ref = _case(*key)
    dv = dev()
    s = dict(d=d, ref=ref, x0=cc.guarded_nhwc(d['x0']), x1=cc.guarded_nhwc(d['x1']) if d['x1'] is not None else None, bias=d['bias'].to(dv))
    if key[0] == 'u8':
        s['w'] = framed_in(d['q'], d['q'].shape[1] + 16)
        s['w_scale'], s['w_off'] = d['w_scale'].to(dv), d['w_off'].to(dv)
    else:
        s['w'] = framed_in(d['w'], d['w'].shape[1] + 8)
        s['t0'] = cc.guarded_nhwc(d['t0']) if d['t0'] is not None else None
        s['t1'] = cc.guarded_nhwc(d['t1']) if d['t1'] is not None else None
        s['bias2'] = d['bias2'].to(dv) if d['bias2'] is not None else None
    return s


def key_plain(n, h, w, mode, c0=128, stride=1, ups=False, cout=COUT):
    return ('f16', n, h, w, c0, 0, cout, 4000 + 131 * h + 7 * w + n + 1000 * stride + 250 * int(ups), 'plain', stride, ups, mode)


def key_form(n, h, w, mode, form):
    return ('f16', n, h, w, 64, 0 if form == 'tail' else 64, COUT, 4500 + 131 * h + 7 * w + n + (50 if form == 'tail' else 0), form, 1, False, mode)


def key_u8(n, h, w, mode, ups=False):
    return ('u8', n, h, w, 64, 64, 40, 4700 + 131 * h + 7 * w + n, 'plain' if ups else 'rowbias', 1, ups, mode)


def launch(key, *, tile, runs_on=None, tag, split=1, fixup=False, same_as=None):
    """one framed launch of a staged case on `tile` under the case's pad_mode; returns (output view, splits)"""
    import ctypes
    s = _staged(key)
    d, ref = s['d'], s['ref']
    kind, form, stride, ups, mode = key[0], key[8], key[9], key[10], key[11]
    m, cout = ref.shape
    ld = (cout + 7) // 8 * 8 + 8
    fo = framed_out(m, cout, ld)
    launch.last_out = fo
    kw = dict(out=fo.view, conv=dict(stride=stride, upsample=ups, pad_mode=mode), tile=tile, runs_on=runs_on, tag=tag, split_k=split, fixup=fixup)
    frames = [fo]
    if s['x1'] is not None:
        kw['a2'] = s['x1']
    if kind == 'u8':
        kw.update(w_scale=s['w_scale'], w_off=s['w_off'])
    if form in ('resblock', 'rowbias'):
        fb = framed_res(d['row_bias'], ld + 24, 16)
        kw.update(row_bias=fb.view, rows_per_img=m // d['row_bias'].shape[0])
        frames.append(fb)
    if form == 'resblock':
        fr = framed_res(d['residual'].reshape(m, cout), ld + 16, 8)
        kw.update(residual=fr.view)
        frames.append(fr)
    if form == 'tail':
        kw.update(tail=(s['t0'], s['t1']), bias2=s['bias2'])
    name = f'{tag} {key} tile{tile} split{split}' + (' fixup' if fixup else '')
    _, _, splits, desc = run_gemm(s['x0'], s['w'].view, s['bias'], want_desc=True, **kw)
    assert desc.pad_mode == mode
    if fixup:
        from sdod.amd import _lib
        assert splits > 1 and _lib.hip().sdod_gemm_fixup(ctypes.byref(desc)) == 1, f'{name}: the in-kernel reduce did not apply'
    check_equal(fo.view, ref, name)
    for f in frames:
        f.frame_intact(name)
    for g in ('x0', 'x1', 't0', 't1'):
        if s.get(g) is not None:
            cc.guards_intact(s[g])
    if same_as is not None:
        assert torch.equal(fo.view, same_as), f'{name}: bits differ from the unsplit launch'
    return fo.view, splits


# ------------------------------------------------------------------------------------------------------ a. halo-patch tiles
def halo_launch(key, geom, *, tile, detail='', **kw):
    """a halo tile may decline a geometry: exactly where conv_cases.halo_takes predicts (the answer of pad_mode 0), leaving nothing
    behind; what runs is compared exactly and counted in RAN"""
    from sdod.amd import _lib
    n, h, w = geom
    ups, mode = key[10], key[11]
    branch = cc.halo_takes(gc.tile_info(tile)['bm'], h, w, ups)
    try:
        out, splits = launch(key, tile=tile, tag=f'wrap:halo{mode}', **kw)
    except _lib.SdodError as ex:
        if 'halo-patch tile does not take' not in str(ex):
            raise
        assert branch is None, f'tile {tile} declined {geom} ups={ups} mode={mode}, which conv_cases.halo_takes places in {branch!r}'
        fo = launch.last_out
        assert torch.isnan(fo.view).all(), f'tile {tile} declined {geom} and still wrote'
        fo.frame_intact(f'tile {tile} declined {geom}')
        DECLINED[tile] = DECLINED.get(tile, 0) + 1
        return None
    assert branch is not None, f'tile {tile} ran {geom} ups={ups} mode={mode}, which conv_cases.halo_takes says it declines'
    RAN.setdefault((tile, branch, ups, mode), set()).add((n, h, w, detail))
    return out, splits


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_wrap_rectangles(tile):
    """mode 2 with the plan's own split (the reduce launch where it splits), modes 3 and 4 unsplit"""
    f = Failures()
    for g in cc.RECTS:
        for mode in WRAP_MODES:
            f.run(halo_launch, key_plain(*g, mode), g, tile=tile, split=0 if mode == 2 else 1)
    f.done()
    for mode in WRAP_MODES:
        assert any(k[0] == tile and k[3] == mode and not k[2] for k in RAN), f'tile {tile} ran nothing under mode {mode}'


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_wrap_upsampling_rectangles(tile):
    f = Failures()
    for g in cc.RECTS_UPS:
        f.run(halo_launch, key_plain(*g, 2, ups=True), g, tile=tile, split=1)
    f.done()
    assert any(k[0] == tile and k[2] for k in RAN), f'tile {tile} ran no upsampling shape'


def _taken(tile, geoms, ups=False, count=2):
    bm = gc.tile_info(tile)['bm']
    return [g for g in geoms if g[1] != g[2] and cc.halo_takes(bm, g[1], g[2], ups)][:count]


@pytest.mark.parametrize('tile', [37, 50])
def test_halo_wrap_split_k_gives_the_unsplit_bits(tile):
    """split-K 1 and 3, the reduce launch and the in-kernel reduce (fixup): the bits of the unsplit launch (128 channels are two
    64-channel chunks, so a request for three slices runs two)"""
    f = Failures()
    geoms = _taken(tile, cc.RECTS)
    assert len(geoms) == 2
    for g in geoms:
        key = key_plain(*g, 2)
        base = halo_launch(key, g, tile=tile, split=1, detail='split1')
        assert base is not None and base[1] == 1
        r = f.run(halo_launch, key, g, tile=tile, split=3, detail='split3', same_as=base[0])
        assert r is None or r[1] > 1
        for _ in range(2):
            f.run(halo_launch, key, g, tile=tile, split=3, fixup=True, detail='split3 fixup', same_as=base[0])
        f.run(halo_launch, key, g, tile=tile, split=1, fixup=False, detail='split1 again', same_as=base[0])
    f.done()


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_wrap_resblock_tail_and_uint8(tile):
    """per tile, on the first ResBlock geometry it takes: concat + per-image row bias + residual, the fused 1x1 tail (chained and as
    its own slice), and uint8 weights with the row bias (the WQ instantiation) -- each under a wrap mode"""
    f = Failures()
    geoms = _taken(tile, cc.RECTS_RESBLOCK, count=1)
    assert geoms
    g = geoms[0]
    f.run(halo_launch, key_form(*g, 2, 'resblock'), g, tile=tile, split=1, detail='resblock')
    f.run(halo_launch, key_form(*g, 3, 'resblock'), g, tile=tile, split=2, detail='resblock split2')
    f.run(halo_launch, key_form(*g, 2, 'tail'), g, tile=tile, split=1, detail='tail chained')
    f.run(halo_launch, key_form(*g, 4, 'tail'), g, tile=tile, split=2, detail='tail split2')
    f.run(halo_launch, key_u8(*g, 2), g, tile=tile, split=1, detail='u8')
    f.run(halo_launch, key_u8(*g, 3), g, tile=tile, split=0, detail='u8 split0')
    gu = _taken(tile, cc.RECTS_UPS, ups=True, count=1)
    assert gu
    f.run(halo_launch, key_u8(*gu[0], 2, ups=True), gu[0], tile=tile, split=1, detail='u8 ups')
    f.done()


def test_every_reachable_tile_and_branch_ran_wrapped():
    """after the tests above (same session), from what RAN on the GPU: every (tile, planner branch) that conv_cases.halo_takes makes
    reachable on RECTS and, with upsampling, on RECTS_UPS ran under mode 2, and every tile ran under modes 3 and 4"""
    missing = []
    for tile in cc.HALO_TILES:
        bm = gc.tile_info(tile)['bm']
        for ups, geoms in ((False, cc.RECTS), (True, cc.RECTS_UPS)):
            for branch in {cc.halo_takes(bm, h, w, ups) for _, h, w in geoms} - {None}:
                if not RAN.get((tile, branch, ups, 2)):
                    missing.append((tile, branch, ups, 2))
        for mode in (3, 4):
            if not any(k[0] == tile and k[3] == mode for k in RAN):
                missing.append((tile, mode))
        assert any(t.startswith('wrap:halo') for t in gc.LEDGER.get((tile, 'halo', False), ())), tile
        assert any(t.startswith('wrap:halo') for t in gc.LEDGER.get((tile, 'halo', True), ())), tile
    assert not missing, f'never ran: {missing}'
    reached = {k[1] for k in RAN if k[3] == 2}
    assert reached == set(cc.BRANCHES), reached


# -------------------------------------------------------------------------------------------------- b. implicit-GEMM tiles
@pytest.mark.parametrize('tile', IMPLICIT_TILES)
def test_implicit_wrap(tile):
    """(2, 1, 2) and (1, 2, 1) are the deepest-level shapes: all three taps of an axis land on one or two pixels.  The odd sizes
    under stride 2 make the bottom / right tap wrap too."""
    f = Failures()
    ro = plain_runs_on(tile)
    for n, h, w in [(2, 8, 12), (3, 5, 9), (1, 9, 5), (2, 1, 2), (1, 2, 1)]:
        for mode in WRAP_MODES:
            f.run(launch, key_plain(n, h, w, mode), tile=tile, runs_on=ro, tag='wrap:s1')
    for n, h, w in [(2, 8, 12), (1, 9, 5), (3, 5, 9)]:
        f.run(launch, key_plain(n, h, w, 2, stride=2), tile=tile, runs_on=ro, tag='wrap:s2')
    for n, h, w in [(2, 4, 6), (1, 5, 3)]:
        f.run(launch, key_plain(n, h, w, 2, ups=True), tile=tile, runs_on=ro, tag='wrap:ups')
    r = f.run(launch, key_plain(2, 8, 12, 2), tile=tile, runs_on=ro, tag='wrap:split', split=3)
    assert r is None or r[1] == 3, (tile, r[1])
    f.done()


@pytest.mark.parametrize('tile', [0, 7, 12, 14, 27, 46])
def test_implicit_wrap_resblock_forms(tile):
    f = Failures()
    for n, h, w in [(2, 8, 12), (3, 4, 12)]:
        if tile != 14:
            f.run(launch, key_form(n, h, w, 2, 'resblock'), tile=tile, runs_on=plain_runs_on(tile), tag='wrap:resblock')
        f.run(launch, key_form(n, h, w, 3, 'tail'), tile=tile, runs_on=fused_runs_on(tile), tag='wrap:tail')
    f.run(launch, key_u8(2, 8, 12, 4), tile=tile, runs_on=gc.u8_tile(fused_runs_on(tile)), tag='wrap:u8')
    f.done()


def test_output_convolution_shape_class():
    """Cout = 3 on the plan's own tile (N <= 16: the skinny register-staged tile 4): the VAE decoder's output convolution"""
    f = Failures()
    for n, h, w in [(2, 8, 12), (1, 9, 5), (2, 1, 2)]:
        for mode in WRAP_MODES:
            f.run(launch, key_plain(n, h, w, mode, c0=128, cout=3), tile=0, runs_on=4, tag='wrap:cout3')
    f.done()


# --------------------------------------------------------------------------------------------------------- c. shift property
def _conv_once(x, wt, bias, tile, runs_on, mode):
    out, _, _ = run_gemm(x, wt, bias, tile=tile, runs_on=runs_on, tag='wrap:shift', conv=dict(stride=1, pad_mode=mode), split_k=1)
    return out.view(*x.shape[:3], -1)


def _shift_case(tile, runs_on, n, h, w, sy, sx):
    gen = torch.Generator().manual_seed(97 + tile + h + w)
    x = gc.ternary((n, h, w, 64), gen)
    wt = gc.ternary((72, 9 * 64), gen).to(dev())
    bias = gc.small_ints((72,), gen, torch.float32).to(dev())
    y2 = _conv_once(x.to(dev()), wt, bias, tile, runs_on, 2)
    assert torch.isfinite(y2).all()
    assert torch.equal(_conv_once(torch.roll(x, (sy, sx), (1, 2)).to(dev()), wt, bias, tile, runs_on, 2), torch.roll(y2, (sy, sx), (1, 2))), \
        f'tile {tile} {(n, h, w)}: mode 2 does not commute with the shift {(sy, sx)}'
    y3 = _conv_once(x.to(dev()), wt, bias, tile, runs_on, 3)
    assert torch.equal(_conv_once(torch.roll(x, sx, 2).to(dev()), wt, bias, tile, runs_on, 3), torch.roll(y3, sx, 2)), \
        f'tile {tile} {(n, h, w)}: mode 3 does not commute with the x shift {sx}'
    assert not torch.equal(_conv_once(torch.roll(x, sy, 1).to(dev()), wt, bias, tile, runs_on, 3), torch.roll(y3, sy, 1)), \
        f'tile {tile} {(n, h, w)}: mode 3 commutes with a y shift'
    y0 = _conv_once(x.to(dev()), wt, bias, tile, runs_on, 0)
    assert not torch.equal(y0, y2) and not torch.equal(y0, y3) and not torch.equal(y2, y3)


@pytest.mark.parametrize('branch', cc.BRANCHES)
def test_shift_property_halo(branch):
    """the first (tile, geometry) of the lists in the branch; shifts that are no multiple of the tile's rows or row segment"""
    for tile in cc.HALO_TILES:
        bm = gc.tile_info(tile)['bm']
        for n, h, w in cc.RECTS:
            if h != w and cc.halo_takes(bm, h, w) == branch:
                _shift_case(tile, tile, n, h, w, 3 if h > 3 else 1, 5)
                return
    raise AssertionError(f'no tile reaches {branch}')


@pytest.mark.parametrize('tile', [27, 3])
def test_shift_property_implicit(tile):
    _shift_case(tile, tile, 2, 8, 12, 3, 5)
    _shift_case(tile, tile, 3, 5, 9, 2, 4)


# ------------------------------------------------------------------------------------------------------ d. input convolutions
WRAP_MODE = {1: 3, 2: 4, 3: 2}               # wrap bits (bit 0 = x, bit 1 = y) -> pad_mode


@pytest.mark.parametrize('n,c,h,w', [(2, 4, 8, 16), (1, 4, 1, 2)])
def test_input_convolutions_wrap(n, c, h, w):
    """sdod_conv_in_wrap_f16 against fp32 F.conv2d on the wrapped, fp16-rounded latent (the comparison of test_conv_in_equals_im2col_then_gemm)
    and, bit for bit, against sdod_im2col3x3_small_wrap_f16 + the K = 64 GEMM; the im2col matrix itself equals the one built in
    torch; wrap 0 through the new entry points gives the old entry points' bits"""
    from sdod.amd import ops
    g = torch.Generator().manual_seed(n * 1000 + h)
    cout = 320
    x = torch.randn(n, c, h, w, generator=g)
    wt = (torch.randn(cout, c, 3, 3, generator=g) / 6).half()
    bias = torch.randn(cout, generator=g)
    wk = torch.zeros(cout, 64, dtype=torch.float16)
    wk[:, :9 * c] = wt.permute(0, 2, 3, 1).reshape(cout, 9 * c)
    xd, wkd, bd = x.cuda(), wk.cuda(), bias.cuda()
    x16 = x.half()
    nhwc = x16.permute(0, 2, 3, 1).contiguous().cuda()
    outs = {}
    for wrap in (1, 2, 3):
        mode = WRAP_MODE[wrap]
        out = ops.conv_in(xd, wkd, bd, wrap=wrap)
        xp = pad_wrap(x16.float(), mode)
        ref = F.conv2d(xp, wt.float(), bias, padding=0).permute(0, 2, 3, 1)
        check_close(out, ref, name=f'conv_in wrap {wrap} {n}x{h}x{w}')
        cols = ops.im2col3x3_small(nhwc, 64, wrap=wrap)
        want = torch.zeros(n * h * w, 64, dtype=torch.float16)
        want[:, :9 * c] = F.unfold(xp, 3).view(n, c, 9, h * w).permute(0, 3, 2, 1).reshape(n * h * w, 9 * c).half()
        assert torch.equal(cols.cpu(), want), f'im2col wrap {wrap}'
        assert torch.equal(ops.gemm(cols, wkd, bd).view(n, h, w, cout), out), f'conv_in wrap {wrap} != im2col + GEMM'
        outs[wrap] = out
    plain = ops.conv_in(xd, wkd, bd)
    assert torch.equal(ops.conv_in(xd, wkd, bd, wrap=0), plain)
    assert torch.equal(ops.im2col3x3_small(nhwc, 64, wrap=0), ops.im2col3x3_small(nhwc, 64))
    assert not any(torch.equal(outs[a], b) for a, b in ((1, plain), (2, plain), (3, plain), (1, outs[2]), (1, outs[3]), (2, outs[3])))


def test_input_convolutions_refuse_a_bad_wrap():
    from sdod.amd import _lib, ops
    x = torch.zeros(1, 4, 8, 8, device='cuda')
    w = torch.zeros(320, 64, dtype=torch.float16, device='cuda'); b = torch.zeros(320, device='cuda')
    for wrap in (-1, 4):
        with pytest.raises(_lib.SdodError):
            ops.conv_in(x, w, b, wrap=wrap)
        with pytest.raises(_lib.SdodError):
            ops.im2col3x3_small(torch.zeros(1, 8, 8, 4, dtype=torch.float16, device='cuda'), 64, wrap=wrap)
