"""The kernels that reduce along a row, against fp64 on the data of tests/row_cases.py: the stand-alone LayerNorm, the LayerNorm
statistics gathered inside the GEMMs (every site that applies eps: the ring kernel with and without loader waves, the A-panel
kernel), sdod_ln_fold_f16, softmax_rows, the 80-column softmax of the score GEMM's epilogue (plain and with region weights), and
the fp32 activation functions over every finite fp16 input, stand-alone and inlined in the GEMM epilogues.

What the Gaussian rows of test_kernels_gpu.py cannot see and these can: eps (rows whose variance is at or below it), a row
maximum that misses a lane group (rows whose spread exceeds the exponent range: a lost maximum overflows), statistics stored
at another row (every row its own mean and scale), subnormal outputs flushed to zero, and one wrong activation coefficient.
tests/test_row_cases_cpu.py proves without a GPU that the references alone meet every bound used here with room.

The LayerNorm fold's contract (include/sdod_hip.h at `ln`): the 3e-3 tolerance holds for |row mean| / row std <= 100 (`offset`,
`nearconst`), beyond that the output is finite (the variance clamp)."""
import ctypes

import pytest
import torch

import gemm_cases as gc
import row_cases as rc
from gemm_cases import check_close as check, geglu_perm, run_gemm, tile_info

pytestmark = pytest.mark.gpu

TAG = 'rows-ln'


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def nan_like(shape):
    return torch.full(shape, float('nan'), dtype=torch.float16, device=dev())


# ------------------------------------------------------------------------------------------- a. stand-alone LayerNorm
LN_BASE_ROWS = 205          # M = 8200 is 40 repeats of 205 rows: one fp64 reference of 205 rows serves all of them


def _ln_inputs(kind, m, c):
    if m <= LN_BASE_ROWS:
        return rc.ln_rows(kind, m, c), 1
    assert m % LN_BASE_ROWS == 0
    return rc.ln_rows(kind, LN_BASE_ROWS, c), m // LN_BASE_ROWS


def _check_ln(out, ref, reps, kind, name):
    """the suite's check at 2e-3; a row of zeros (const rows without affine parameters) has no relative error: max-abs only"""
    assert torch.isfinite(out).all(), f'{name}: non-finite output'
    if reps > 1:
        out = out.view(reps, -1, out.shape[-1]); ref = ref.expand(reps, *ref.shape)
    if float(ref.abs().max()) == 0:
        mx = float(out.double().abs().max())
        assert mx <= 1e-3, f'{name}: max abs {mx:.3e} on rows that normalise to zero'
        return
    check(out, ref, tol=rc.LN_TOL, name=name)


# chunk counts 1, 8, 41, 49, 97, 193, 384: all four lanes-per-row variants, ragged lane groups, the maximum; M = 1 and 37 do
# not fill a wave, 8200 is more than one pass of the 2048-workgroup grid at 64 lanes per row
@pytest.mark.parametrize('m', [1, 37, 8200])
@pytest.mark.parametrize('c', [8, 64, 328, 392, 776, 1544, 3072])
def test_layer_norm_vs_fp64(c, m):
    from sdod.amd import ops
    d = dev()
    gamma, beta = rc.ln_params(c)
    for kind, eps in rc.LN_CASES:
        x, reps = _ln_inputs(kind, m, c)
        xd = x.to(d).repeat(reps, 1)
        out = ops.layer_norm(xd, gamma.to(d), beta.to(d), eps, out=nan_like((m, c)))
        _check_ln(out, rc.ln_ref(x, gamma, beta, eps), reps, kind, f'ln {kind} eps {eps} {m}x{c}')
    for kind in ('rowmix', 'const'):
        x, reps = _ln_inputs(kind, m, c)
        xd = x.to(d).repeat(reps, 1)
        ref = rc.ln_ref(x, None, None, 1e-5)
        out = ops.layer_norm(xd, None, None, 1e-5, out=nan_like((m, c)))           # weight = bias = None
        _check_ln(out, ref, reps, kind, f'ln no affine {kind} {m}x{c}')
        ops.layer_norm(xd, None, None, 1e-5, out=xd)                                # in place
        assert torch.equal(xd.view(torch.int16), out.view(torch.int16)), f'in place differs {kind} {m}x{c}'


@pytest.mark.parametrize('c', [3080, 12])
def test_layer_norm_refuses_without_writing(c):
    from sdod.amd import _lib, ops
    d = dev()
    x = rc.ln_rows('normal', 5, c).to(d)
    out = nan_like((5, c))
    with pytest.raises(_lib.SdodError):
        ops.layer_norm(x, None, None, 1e-5, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), 'a refused LayerNorm wrote to its destination'


# ------------------------------------------------------------------------------------ b. the LayerNorm fold in the GEMMs
FOLD_M, FOLD_N = 200, 160                    # ragged against 128-, 64- and 32-row tiles
FOLD_TILES = [0, 6, 8, 11, 14, 18, 20, 21, 22, 23, 25, 26, 27, 28, 30, 31, 32, 33, 35, 36, 46, 47, 48, 56, 57, 58, 59, 60, 61]   # test_gemm_with_folded_layer_norm's
PANEL_K = {53: 320, 54: 640, 55: 1280}       # the A-panel tiles and the K their panel is sized for
_fold_cache = {}


def _fold_case(k):
    """per K, computed once and left unchanged: the folded operands on the device and the fp64 reference of every (kind, eps)"""
    if k not in _fold_cache:
        from sdod.amd import ops
        d = dev()
        gamma, beta = rc.ln_params(k); w, bias = rc.linear_params(FOLD_N, k)
        wf, s, t = ops.ln_fold(w.clone().to(d), gamma.to(d), beta.to(d), bias.to(d))
        perm = geglu_perm(FOLD_N // 2)
        gwf, gs, gt = ops.ln_fold(w[perm].contiguous().to(d), gamma.to(d), beta.to(d), bias[perm].contiguous().to(d))
        c = dict(wf=wf, s=s, t=t, gwf=gwf, gs=gs, gt=gt, x={}, ref={})
        for kind, eps in rc.LN_CASES:
            x = rc.ln_rows(kind, FOLD_M, k)
            c['x'][kind] = x.to(d)
            c['ref'][kind, eps] = rc.fold_ref(x, w, gamma, beta, bias, eps)
        c['geglu_ref'] = rc.geglu_ref(c['ref']['rowmix', 1e-5])
        c['t_ref'] = w.double() @ beta.double() + bias.double()
        c['hot'] = torch.full((FOLD_M, k), 1000.0, dtype=torch.float16, device=d)
        _fold_cache[k] = c
    return _fold_cache[k]


def _even_tn(tile):
    """the GEGLU epilogue pairs value and gate blocks inside a wave: an even number of 16-column blocks per wave"""
    i = tile_info(tile)
    return (i['bn'] // i['wn']) % 32 == 0


@pytest.mark.parametrize('tile', FOLD_TILES + sorted(PANEL_K))
def test_gemm_ln_fold_vs_fp64(tile):
    ks = (PANEL_K[tile],) if tile in PANEL_K else (64, 320)
    on = tile or 14                                                  # 0: fusions live in the LDS-DMA families
    for k in ks:
        c = _fold_case(k)
        for kind, eps in rc.LN_CASES:
            out = run_gemm(c['x'][kind], c['wf'], c['t'], ln_s=c['s'], ln_eps=eps, tile=tile, runs_on=on, tag=TAG)[0]
            print(f'ln fold {kind} eps {eps} K {k} tile {tile}: rel-L2 {rc.rel_l2(out, c["ref"][kind, eps]):.2e}')
            check(out, c['ref'][kind, eps], tol=rc.FOLD_TOL, name=f'ln fold {kind} eps {eps} K {k} tile {tile}')
            if kind == 'const':                                      # variance 0: the row is t = beta . W^T + bias
                check(out, c['t_ref'].expand(FOLD_M, FOLD_N), tol=rc.FOLD_TOL, name=f'ln fold const rows = t, K {k} tile {tile}')
        if _even_tn(on):                                             # the two-fma form of the GEGLU epilogue
            out = run_gemm(c['x']['rowmix'], c['gwf'], c['gt'], ln_s=c['gs'], geglu=True, tile=tile, runs_on=on, tag=TAG)[0]
            check(out, c['geglu_ref'], tol=rc.FOLD_TOL, name=f'ln fold + geglu rowmix K {k} tile {tile}')
        # out of contract (|mean| / std unbounded): finite, nothing more -- the variance clamp
        out = run_gemm(c['hot'], c['wf'], c['t'], ln_s=c['s'], tile=tile, runs_on=on, tag=TAG)[0]
        assert torch.isfinite(out).all(), f'const rows of 1000.0: non-finite output, K {k} tile {tile}'


def test_every_statistics_site_ran():
    """the three places that turn the sums into (mean, rstd): the ring kernel's loader waves (spec 1), its unspecialised form
    (spec 0) and the A-panel kernel"""
    ran = {(tile_info(t)['family'], tile_info(t)['spec']) for (t, _, u8), tags in gc.LEDGER.items() if TAG in tags and not u8}
    assert {('ring', 0), ('ring', 1), ('panel', 0)} <= ran, ran


# ---------------------------------------------------------------------------------------------------- c. ops.ln_fold
@pytest.mark.parametrize('k', [64, 320, 1000])
def test_ln_fold_kernel_vs_fp64(k):
    from sdod.amd import _lib, ops
    lib = _lib.hip()
    d = dev()
    n, ldw = 5, k + 8
    gamma, beta = rc.ln_params(k); w, bias = rc.linear_params(n, k)
    for b in (bias, None):
        fw = gc.framed_in(w, ldw)                                    # NaN frame: one guard row above and below, 8 columns per row
        s = torch.full((n,), float('nan'), device=d); t = torch.full((n,), float('nan'), device=d)
        ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
        gd, bd, biasd = gamma.to(d), beta.to(d), None if b is None else b.to(d)
        _lib.check(lib.sdod_ln_fold_f16(ptr(fw.view), n, k, ldw, ptr(gd), ptr(bd), ptr(biasd), ptr(s), ptr(t), ops._stream()))
        torch.cuda.synchronize()
        got = fw.view.cpu()
        frame = fw.buf.clone(); frame[1:1 + n, :k] = float('nan')
        assert torch.isnan(frame).all(), 'ln_fold wrote outside its k columns'
        want = (w.float() * gamma).half()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), 'folded weight is not fp16(w * gamma)'
        s_ref = want.double().sum(1); s_tol = 1e-6 * want.double().abs().sum(1)
        assert bool(((s.cpu().double() - s_ref).abs() <= s_tol).all()), (s.cpu(), s_ref)
        t_ref = (w.double() * beta.double()).sum(1) + (0 if b is None else b.double())
        t_tol = 1e-6 * ((w.double() * beta.double()).abs().sum(1) + (0 if b is None else b.double().abs()))
        assert bool(((t.cpu().double() - t_ref).abs() <= t_tol).all()), (t.cpu(), t_ref)


# -------------------------------------------------------------------------------------------------- d. softmax_rows
@pytest.mark.parametrize('n', rc.SOFTMAX_NS)
def test_softmax_rows_vs_fp64(n):
    from sdod.amd import ops
    d = dev()
    for kind in rc.SOFTMAX_KINDS:
        x = rc.softmax_rows_kind(kind, n)
        assert x.shape[0] <= 64
        out = ops.softmax_rows(x.to(d), out=nan_like(tuple(x.shape))).cpu()
        name = f'softmax_rows N {n} {kind}'
        worst = rc.check_close16(out, rc.softmax_ref(x), rc.SOFTMAX_R, name=name)
        err = float((out.double().sum(1) - 1).abs().max())
        print(f'{name}: worst |err| / bound {worst:.3f}, row sums within {err:.2e}')
        assert err <= rc.row_sum_bound(n), f'{name}: a row sums to 1 +- {err:.3e}'


# ------------------------------------------------------------------------------- e. the score GEMM's softmax epilogue
SOFTMAX_TILES = [31, 48, 56, 57, 58, 59, 60]
EPI_M = 128                                   # rows 0..127: the peak visits each of the 77 key columns (r mod 77)
_epi_cache = {}


def _epi_case(kind, n):
    if (kind, n) not in _epi_cache:
        s = rc.epilogue_scores(kind, EPI_M, n)
        a, w, bias = rc.epilogue_operands(s, 192 if n == 160 else n)
        _epi_cache[kind, n] = (a.to(dev()), w.to(dev()), bias.to(dev()), rc.epilogue_ref(s))
    return _epi_cache[kind, n]


def _region_weights(rows, regions):
    """fp32 [rows][regions] of {1, 0, 0.25}, rotated from row to row so that a weight read at another row shows"""
    base = torch.tensor([1.0, 0.0, 0.25])
    return base[(torch.arange(rows)[:, None] + torch.arange(regions)[None]) % 3].contiguous()


@pytest.mark.parametrize('n', [160, 320])
@pytest.mark.parametrize('tile', SOFTMAX_TILES)
def test_gemm_softmax_epilogue_vs_fp64(tile, n):
    rows = tile_info(tile)['bm']              # per-image weights: a tile never straddles two images
    n_img = EPI_M // rows
    groups = n // 80
    for kind in rc.EPI_KINDS:
        a, w, bias, ref = _epi_case(kind, n)
        w_img = w[None].expand(n_img, *w.shape).contiguous()
        kw = dict(rows_per_img=rows, softmax_cols=80, tile=tile, tag='rows-softmax')
        name = f'softmax epilogue {kind} N {n} tile {tile}'
        plain = run_gemm(a, w_img, bias, **kw)[0].cpu()
        assert int((plain.view(EPI_M, groups, 80)[:, :, 77:].view(torch.int16) != 0).sum()) == 0, f'{name}: padding columns are not exact zeros'
        worst = rc.check_close16(plain, ref, rc.SOFTMAX_R, name=name)
        print(f'{name}: worst |err| / bound {worst:.3f}')
        # the REGION variant: weight 1 changes no bit, weight 0 gives exact zeros, 0.25 is an exact scaling of the reciprocal
        for regions in ((2,) if groups == 2 else (2, 4)):
            rw = _region_weights(rows, regions)
            got = run_gemm(a, w_img, bias, region_w=rw.to(dev()), regions=regions, **kw)[0].cpu()
            wt = rw.repeat(n_img, 1).repeat_interleave(groups // regions * 80, dim=1)      # [M][N]: the weight of every element
            assert wt.shape == got.shape
            one, zero = wt == 1.0, wt == 0.0
            assert torch.equal(got.view(torch.int16)[one], plain.view(torch.int16)[one]), f'{name} regions {regions}: weight 1 changed bits'
            assert int((got.view(torch.int16)[zero] != 0).sum()) == 0, f'{name} regions {regions}: weight 0 is not an exact zero'
            rc.check_close16(got, ref * wt.double(), rc.SOFTMAX_R, name=f'{name} regions {regions}')


# -------------------------------------------------------------------------------------- f. activations, exhaustively
def _sweep():
    return rc.all_finite_f16()


def _check_value_times_gelu(out, x, value, name):
    """value * gelu(gate) with the product in fp32: the GELU bound scaled by |value|, plus the product's own rounding.  Where the
    product leaves the fp16 range (|value| > 1, gates beyond 65504 / |value|) the output is the infinity of its sign."""
    ref = value * rc.gelu64(x)
    over = ref.abs() >= 65520                                  # halfway between the largest finite fp16 and 2^16 rounds up
    out = out.cpu()
    assert torch.equal(out[over].double(), torch.sign(ref[over]) * float('inf')), f'{name}: overflow is not an infinity'
    rc.check_close16(out[~over], ref[~over], rc.GELU_R + 2.0 ** -24, abs(value) * rc.GELU_A, name=name)


@pytest.mark.parametrize('act', ['silu', 'gelu', 'quick_gelu', 'relu'])
def test_activation_every_fp16_value(act):
    from sdod.amd import ops
    x = _sweep()
    out = ops.activation(x.to(dev()), act, out=nan_like(tuple(x.shape))).cpu()
    if act == 'relu':
        assert torch.equal(out.view(torch.int16), torch.where(x < 0, torch.zeros_like(x), x).view(torch.int16))
        return
    r, a = rc.ACT_BOUND[act]
    worst = rc.check_close16(out, rc.ACT_REF[act](x), r, a, name=f'activation {act}')
    print(f'activation {act}: worst |err| / bound {worst:.3f}')


@pytest.mark.parametrize('value', [1.0, -3.0, 2.0 ** -10])
def test_geglu_every_fp16_gate(value):
    from sdod.amd import ops
    g = _sweep().view(992, 64)
    x = torch.cat([torch.full_like(g, value), g], 1)
    _check_value_times_gelu(ops.geglu(x.to(dev())), g, value, f'geglu value {value}')


# one register-staged tile, one ring tile without and one with loader waves, a 32-row tile (all 64 x 64 or 32 x 64), and an A-panel
# tile (its epilogue is its own; the smallest K it takes is 192: the sweep sits in the first 64 columns, zeros behind)
ACT_TILES = [3, 8, 28, 46, 53]


def _sweep_operands(tile, h=64):
    """(a [992][k] = the sweep in the first 64 columns, identity [h][k])"""
    k = 192 if tile == 53 else h
    x = _sweep().view(992, h)
    a = torch.zeros(992, k, dtype=torch.float16); a[:, :h] = x
    eye = torch.zeros(h, k, dtype=torch.float16); eye[:, :h] = torch.eye(h).half()
    return x, a, eye


@pytest.mark.parametrize('act', ['silu', 'gelu', 'quick_gelu'])
@pytest.mark.parametrize('tile', ACT_TILES)
def test_gemm_epilogue_activation_every_fp16_value(tile, act):
    """A = the sweep as 992 x 64, W = the identity: every product and sum is exact, the output is act(a)"""
    x, a16, w = _sweep_operands(tile)
    out = run_gemm(a16.to(dev()), w.to(dev()), act=act, tile=tile, tag='rows-act')[0].cpu()
    r, a = rc.ACT_BOUND[act]
    rc.check_close16(out, rc.ACT_REF[act](x), r, a, name=f'gemm epilogue {act} tile {tile}')


@pytest.mark.parametrize('value', [1.0, -3.0, 2.0 ** -10])
@pytest.mark.parametrize('tile', [0, 8, 28, 46, 53])
def test_gemm_fused_geglu_every_fp16_gate(tile, value):
    """the fused GEGLU epilogue: the gate rows of W are the identity, the value rows zero with a bias of `value`"""
    h = 64
    x, a16, eye = _sweep_operands(tile, h)
    w = torch.cat([torch.zeros_like(eye), eye], 0)
    bias = torch.cat([torch.full((h,), value), torch.zeros(h)])
    perm = geglu_perm(h)
    out = run_gemm(a16.to(dev()), w[perm].contiguous().to(dev()), bias[perm].contiguous().to(dev()), geglu=True, tile=tile, runs_on=tile or 14,
                   tag='rows-act')[0].cpu()
    assert out.shape == (992, h)
    _check_value_times_gelu(out, x, value, f'fused geglu value {value} tile {tile}')
