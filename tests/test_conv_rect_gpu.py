"""The 3x3 convolution at the rectangles the engine builds since (h, w) latents became public, on exact data (helpers:
tests/conv_cases.py, tests/gemm_cases.py).

Every launch goes through gemm_cases.run_gemm (the plan confirms the tile that ran), reads NaN-guarded NHWC inputs and a framed
weight matrix, writes into a framed output, and must EQUAL the fp64 reference: one wrong, missing or doubled tap, a row bias
taken from the neighbouring image or an h / w mix-up in the planner's arithmetic is a failure, not 1e-4 of rel-L2.

a. implicit-GEMM tiles (register-staged and ring: every tile id test_kernels_gpu.py::test_conv3x3 lists) take any geometry:
   stride 1 on every non-segment shape of the list, stride 2 with and without the VAE encoder's pad_mode, nearest-2x
   upsampling, split-K, everything a ResBlock asks, the engine's own rectangles.
b. halo-patch tiles take what halo_geometry() takes: each tile runs the whole list, a shape it declines must be one that
   conv_cases.halo_takes() predicts it declines (and the refusal leaves the output untouched), and everything that RAN is
   counted per (tile, branch of the planner): plain and upsampling at split 0 / 1 / 3 with the in-kernel split-K reduce giving
   the reduce kernel's bits twice in a row, uint8 weights, the ResBlock forms with a per-image row bias through both of the
   kernel's row-bias paths (rb_lds inside one image, the per-row fallback where a tile spans images).
c. the closing test reads the ledger: every (tile, branch) pair tests/test_conv_cases_cpu.py demands has run."""
import ctypes
import functools

import pytest
import torch

import conv_cases as cc
import gemm_cases as gc
from gemm_cases import check_equal, dev, framed_in, framed_out, framed_res, run_gemm

pytestmark = pytest.mark.gpu

# every tile id test_conv3x3 lists (0: the plan's own choice, which is tile 3 for these sizes)
IMPLICIT_TILES = [0, 6, 7, 8, 9, 10, 11, 12, 13, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 46, 47, 48]
# the implicit-GEMM tiles that carry the ResBlock fusions: test_conv3x3_concat_rowbias_residual / test_conv3x3_with_skip_tail_segment
CONCAT_TILES = [0, 6, 7, 8, 9, 10, 11, 12, 17, 18, 19, 20, 21, 22]
TAIL_TILES = [0, 7, 9, 12, 14, 23, 26, 27, 31, 32, 36, 46, 48]
COUT = 88                  # ragged against every BN (32 / 64 / 80 / 160), a multiple of 8
RAN = {}                   # (halo tile, branch, kind) -> set of (n, h, w, detail) that ran and passed
DECLINED = {}              # halo tile -> refusals (each one predicted by conv_cases.halo_takes)


class Failures:
    """the cases of one test run to the end and report together (only comparisons are collected: an error of the library or
    of the device ends the test where it happens)"""

    def __init__(self):
        self.msgs = []

    def run(self, fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except AssertionError as ex:
            self.msgs.append(str(ex).split('\n')[0][:400])
            return None

    def done(self):
        assert not self.msgs, f'{len(self.msgs)} failures:\n' + '\n'.join(self.msgs[:16])


def plain_runs_on(tile, key=None):
    """make_plan, tile 0: the largest register-staged tile (1, then 2) that still cuts M x N into 384 workgroups, else tile 3 --
    which is every small shape here; the engine's own rectangles reach the larger ones"""
    if tile or key is None:
        return tile or 3
    m, n = _staged(key)['ref'].shape
    for t in (1, 2):
        i = gc.tile_info(t)
        if -(-m // i['bm']) * -(-n // i['bn']) >= 384:
            return t
    return 3


def fused_runs_on(tile):
    """make_plan: fusions (tail, uint8) live in the LDS-DMA families -- the plan's own choice and the register-staged tiles go to 14"""
    return 14 if tile == 0 or gc.tile_info(tile)['family'] == 'reg' else tile


# ---------------------------------------------------------------------------------------------------------------- staging
@functools.lru_cache(None)
def _staged(key):
    """device copies of one case's inputs, made once: NaN-guarded NHWC sources, the weight in a NaN (255) frame"""
    kind, args = key[0], key[1:]
    d, ref = (cc.conv_case_u8 if kind == 'u8' else cc.conv_case)(*args)
    dv = dev()
    s = dict(ref=ref, x0=cc.guarded_nhwc(d['x0']), x1=cc.guarded_nhwc(d['x1']) if d['x1'] is not None else None, bias=d['bias'].to(dv))
    if kind == 'u8':
        s['w'] = framed_in(d['q'], d['q'].shape[1] + 16)
        s['w_scale'], s['w_off'] = d['w_scale'].to(dv), d['w_off'].to(dv)
    else:
        s['w'] = framed_in(d['w'], d['w'].shape[1] + 8)
        s['t0'] = cc.guarded_nhwc(d['t0']) if d['t0'] is not None else None
        s['t1'] = cc.guarded_nhwc(d['t1']) if d['t1'] is not None else None
        s['bias2'] = d['bias2'].to(dv) if d['bias2'] is not None else None
    s['d'] = d
    return s


def launch(key, *, tile, runs_on=None, tag, split=1, conv=None, form='plain', fixup=False, xcd=0, same_as=None):
    """one framed launch of a staged case on `tile`; returns (output view, splits).  form: 'plain' | 'resblock' | 'tail' | 'rowbias'"""
    s = _staged(key)
    d, ref = s['d'], s['ref']
    m, cout = ref.shape
    ld = (cout + 7) // 8 * 8 + 8
    fo = framed_out(m, cout, ld)
    kw = dict(out=fo.view, conv=conv or dict(stride=1), tile=tile, runs_on=runs_on, tag=tag, split_k=split, fixup=fixup, xcd=xcd)
    frames = [fo]
    launch.last_out = fo
    if s['x1'] is not None:
        kw['a2'] = s['x1']
    if key[0] == 'u8':
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
    name = f'{tag} {key} tile{tile} split{split}' + (' fixup' if fixup else '') + (f' xcd{xcd}' if xcd else '')
    _, _, splits, desc = run_gemm(s['x0'], s['w'].view, s['bias'], want_desc=True, **kw)
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
        assert torch.equal(fo.view, same_as), f'{name}: bits differ from the first launch'
    return fo.view, splits


def key_plain(n, h, w, c0=128, stride=1, pad_mode=0, ups=False, cout=COUT):
    return ('f16', n, h, w, c0, 0, cout, 9000 + 131 * h + 7 * w + n + 1000 * stride + 500 * pad_mode + 250 * int(ups), 'plain', stride, pad_mode, ups)


def key_form(n, h, w, form):
    return ('f16', n, h, w, 64, 0 if form == 'tail' else 64, COUT, 9500 + 131 * h + 7 * w + n + (50 if form == 'tail' else 0), form)


def key_u8(n, h, w, ups=False, row_bias=False):
    return ('u8', n, h, w, 64, 64, 40, 9700 + 131 * h + 7 * w + n, ups, row_bias)


# -------------------------------------------------------------------------------------------------- a. implicit-GEMM tiles
STRIDE1 = [g for g in cc.RECTS if g not in cc.RECTS_SEGMENT]


@pytest.mark.parametrize('tile', IMPLICIT_TILES)
def test_implicit_stride1_rectangles(tile):
    f = Failures()
    for n, h, w in STRIDE1:
        f.run(launch, key_plain(n, h, w), tile=tile, runs_on=plain_runs_on(tile), tag='rect:s1')
    f.done()


@pytest.mark.parametrize('tile', IMPLICIT_TILES)
def test_implicit_stride2_pad_mode_upsampling_and_split_k(tile):
    f = Failures()
    ro = plain_runs_on(tile)
    for n, h, w in [(2, 8, 12), (2, 12, 8), (1, 9, 5), (3, 5, 9)]:
        f.run(launch, key_plain(n, h, w, stride=2), tile=tile, runs_on=ro, tag='rect:s2', conv=dict(stride=2))
    for n, h, w in [(2, 8, 12), (1, 9, 5), (2, 12, 8)]:
        f.run(launch, key_plain(n, h, w, stride=2, pad_mode=1), tile=tile, runs_on=ro, tag='rect:s2pad', conv=dict(stride=2, pad_mode=1))
    for n, h, w in [(2, 4, 6), (2, 6, 4), (1, 5, 3)]:
        f.run(launch, key_plain(n, h, w, ups=True), tile=tile, runs_on=ro, tag='rect:ups', conv=dict(stride=1, upsample=True))
    for n, h, w in [(2, 8, 12), (2, 12, 8)]:
        for split in (1, 3):
            r = f.run(launch, key_plain(n, h, w), tile=tile, runs_on=ro, tag='rect:split', split=split)
            assert r is None or r[1] == split, (tile, split, r[1])       # 18 slabs: three slices of six
    f.done()


@pytest.mark.parametrize('tile', sorted(set(CONCAT_TILES) | set(TAIL_TILES)))
def test_implicit_resblock_forms_at_rectangles(tile):
    """two-source concat + per-image row bias + residual, then the 3x3 + 1x1-tail form; at 96 and 48 rows per image every tile
    of 64 / 128 / 256 rows straddles an image boundary"""
    f = Failures()
    for n, h, w in cc.RECTS_RESBLOCK[:4]:
        if tile in CONCAT_TILES:
            f.run(launch, key_form(n, h, w, 'resblock'), tile=tile, runs_on=plain_runs_on(tile), tag='rect:resblock', form='resblock')
        if tile in TAIL_TILES:
            f.run(launch, key_form(n, h, w, 'tail'), tile=tile, runs_on=fused_runs_on(tile), tag='rect:tail', form='tail')
    f.done()


# ------------------------------------------------------------------------------------------------------ b. halo-patch tiles
def halo_launch(key, geom, ups, *, tile, kind, detail='', **kw):
    """a halo tile may decline a geometry: the refusal must be the "does not take" error, predicted by conv_cases.halo_takes,
    and leaves nothing behind; what runs is compared exactly and counted in RAN[(tile, branch, kind)]"""
    from sdod.amd import _lib
    n, h, w = geom
    branch = cc.halo_takes(gc.tile_info(tile)['bm'], h, w, ups)
    try:
        out, splits = launch(key, tile=tile, tag=f'halo:{kind}', conv=dict(stride=1, upsample=True) if ups else None, **kw)
    except _lib.SdodError as ex:
        if 'halo-patch tile does not take' not in str(ex):
            raise
        assert branch is None, f'tile {tile} declined {geom} ups={ups}, which conv_cases.halo_takes places in {branch!r}'
        fo = launch.last_out
        assert torch.isnan(fo.view).all(), f'tile {tile} declined {geom} and still wrote'
        fo.frame_intact(f'tile {tile} declined {geom}')
        DECLINED[tile] = DECLINED.get(tile, 0) + 1
        return None
    assert branch is not None, f'tile {tile} ran {geom} ups={ups}, which conv_cases.halo_takes says it declines'
    RAN.setdefault((tile, branch, kind), set()).add((n, h, w, detail))
    return out, splits


def halo_sweep(f, key, geom, ups, tile, kind, splits=(0, 1, 3), **kw):
    """the splits of one geometry; a split plan runs again twice with the in-kernel reduce and must give the same bits"""
    for split in splits:
        r = f.run(halo_launch, key, geom, ups, tile=tile, kind=kind, detail=f'split{split}', split=split, **kw)
        if r is None:
            return                       # declined (or failed): the other splits answer the same
        if r[1] > 1:
            for _ in range(2):
                f.run(halo_launch, key, geom, ups, tile=tile, kind=kind, detail=f'split{split} fixup', split=split, fixup=True, same_as=r[0], **kw)


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_plain_rectangles(tile):
    f = Failures()
    for g in cc.RECTS:
        halo_sweep(f, key_plain(*g), g, False, tile, 'plain')
    f.done()
    assert any(k[0] == tile and k[2] == 'plain' for k in RAN), f'tile {tile} ran nothing'


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_upsampling_rectangles(tile):
    f = Failures()
    for g in cc.RECTS_UPS:
        halo_sweep(f, key_plain(*g, ups=True), g, True, tile, 'ups')
    f.done()
    assert any(k[0] == tile and k[2] == 'ups' for k in RAN), f'tile {tile} ran nothing'


def u8_subset(tile):
    """per branch the tile reaches: the first plain geometry with h != w, and the first upsampling source"""
    bm = gc.tile_info(tile)['bm']
    picks = {}
    for ups, geoms in ((False, cc.RECTS), (True, cc.RECTS_UPS)):
        for g in geoms:
            b = cc.halo_takes(bm, g[1], g[2], ups)
            if b and g[1] != g[2]:
                picks.setdefault((b, ups), g)
    return picks


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_uint8_weights_at_rectangles(tile):
    """affine-uint8 codes over 0..255 (scale 1, three offsets), two sources, a sparse +-1 image: exact; with the row bias on the
    plain geometries"""
    f = Failures()
    picks = u8_subset(tile)
    assert {b for b, ups in picks if not ups} == {b for b in cc.BRANCHES if b != 'segment' or gc.tile_info(tile)['bm'] in (64, 96)}
    for (b, ups), g in picks.items():
        halo_sweep(f, key_u8(*g, ups=ups, row_bias=not ups), g, ups, tile, 'u8', form='plain' if ups else 'rowbias')
    f.done()


@pytest.mark.parametrize('tile', cc.HALO_TILES)
def test_halo_resblock_forms_at_rectangles(tile):
    """everything a ResBlock asks of one launch.  Every image has its own row-bias row (no two agree in any column): where the
    tile spans images ('images': the per-row fallback) a row taken from the wrong image fails equality, where it lies inside one
    image the row rides in LDS (rb_lds)"""
    f = Failures()
    for g in cc.RECTS_RESBLOCK:
        halo_sweep(f, key_form(*g, 'resblock'), g, False, tile, 'rowbias', splits=(1, 2), form='resblock')
        halo_sweep(f, key_form(*g, 'tail'), g, False, tile, 'tail', splits=(1, 2), form='tail')
    f.done()


# ------------------------------------------------------------------------------------------------- the engine's rectangles
@pytest.mark.parametrize('tile', IMPLICIT_TILES + cc.HALO_TILES)
def test_engine_rectangles_thin_channels(tile):
    """64x96, 96x64, their half-size levels and 128x192 with cin = 64, plain and upsampling into 64x96 / 96x64"""
    f = Failures()
    halo = tile in cc.HALO_TILES
    for g in cc.RECTS_ENGINE:
        key = key_plain(*g, c0=64, cout=72)
        if halo:
            f.run(halo_launch, key, g, False, tile=tile, kind='engine', split=1)
        else:
            f.run(launch, key, tile=tile, runs_on=plain_runs_on(tile, key), tag='rect:engine')
    for g in cc.RECTS_ENGINE_UPS:
        key = key_plain(*g, c0=64, ups=True, cout=72)
        if halo:
            f.run(halo_launch, key, g, True, tile=tile, kind='engine_ups', split=1)
        else:
            f.run(launch, key, tile=tile, runs_on=plain_runs_on(tile, key), tag='rect:engine_ups', conv=dict(stride=1, upsample=True))
    f.done()
    if halo:
        assert any(k[0] == tile and k[2] == 'engine' for k in RAN), f'tile {tile} took none of the engine rectangles'


# ------------------------------------------------------------------------------------------------------------ c. the ledger
def test_every_demanded_tile_and_branch_ran():
    """after the tests above (same session), from what RAN on the GPU -- a refusal counts for nothing: per halo tile and branch
    it can reach, two plain geometries with h != w (in 'rows' both orientations), an upsampling geometry in 'rows' and one in
    'images', a uint8 launch per branch, and a row-bias launch in 'images' (the per-row fallback) and one inside a single image"""
    missing = []

    def geoms(tile, branch, kind):
        return {(n, h, w) for n, h, w, _ in RAN.get((tile, branch, kind), ()) if h != w}

    for tile in cc.HALO_TILES:
        bm = gc.tile_info(tile)['bm']
        for branch in cc.BRANCHES:
            if branch == 'segment' and bm not in (64, 96):     # unreachable: test_conv_cases_cpu.py::UNREACHABLE
                assert not any(k[0] == tile and k[1] == 'segment' for k in RAN)
                continue
            if len(geoms(tile, branch, 'plain')) < 2:
                missing.append((tile, branch, 'plain', sorted(geoms(tile, branch, 'plain'))))
            if not geoms(tile, branch, 'u8'):
                missing.append((tile, branch, 'u8'))
        rows = geoms(tile, 'rows', 'plain')
        if not (any(h < w for _, h, w in rows) and any(h > w for _, h, w in rows)):
            missing.append((tile, 'rows', 'both orientations', sorted(rows)))
        for branch in ('rows', 'images'):
            if not geoms(tile, branch, 'ups'):
                missing.append((tile, branch, 'ups'))
        if not geoms(tile, 'images', 'rowbias'):
            missing.append((tile, 'images', 'rowbias'))
        if not (geoms(tile, 'rows', 'rowbias') | geoms(tile, 'segment', 'rowbias')):
            missing.append((tile, 'single image', 'rowbias'))
    assert not missing, f'(tile, branch, kind) that never ran: {missing}'
    # every launch above went through run_gemm, which asserted the tile the plan ran: the shared ledger holds them
    for tile in cc.HALO_TILES:
        assert any(t.startswith('halo:') for t in gc.LEDGER.get((tile, 'halo', False), ())), tile
        assert 'halo:u8' in gc.LEDGER.get((tile, 'halo', True), ()), tile
