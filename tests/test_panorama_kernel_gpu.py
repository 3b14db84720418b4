"""sdod_k_step_windows on the GPU against its float32 restatement (tests/panorama_ref.py), bit for bit: random fp16 predictions, no
UNet.  Every table shape (panorama_ref.SHAPES), the three samplers' coefficient patterns, both weight kinds, CFG modes 0 and 1, one
chunk and several; the noise injected and drawn in the kernel.  A negative control in the same test -- the restatement with "last
window wins" in the place of the average -- differs from the kernel in more than half of the multiply-covered elements, so the
equality cannot hold by accident."""
import numpy as np
import pytest
import torch

import panorama_ref as R

pytestmark = pytest.mark.gpu

SIGMA = 4.4998425189583315
COEF = {                                        # d0, d1 of an eps model at SIGMA; (a, b, cprev, u) as test_ksamplers_gpu.py's STEP_CASES
    'euler': dict(a=0.7699723632996166, b=0.2300276367003834, cprev=0.0, u=0.0),
    'euler_a': dict(a=0.5930, b=0.4070, cprev=0.0, u=2.1903),
    'euler_a_device': dict(a=0.5930, b=0.4070, cprev=0.0, u=2.1903),
    'dpmpp_2m': dict(a=0.7699723632996166, b=0.3493368915874824, cprev=-0.11930925488709897, u=0.0),
    'last': dict(a=0.0, b=1.0, cprev=0.0, u=0.0),
}
STAGE_SCALE = 0.27730186345778407
TEMB_W = 520
SEED, LEVEL, IDX0 = 987654321, 4, 5
FILL = -3.0                                     # the pattern the staging buffer holds before a launch


def bits(t):
    return t.contiguous().view(torch.int32)


def coef(case):
    return dict(COEF[case], d0=1.0, d1=-SIGMA, stage_scale=STAGE_SCALE)


def rows_per_eval(n_win, chunking):
    """'one': every window in one evaluation; 'several': two windows per evaluation where that gives more than one chunk (three windows:
    a partly filled last chunk), else one"""
    if chunking == 'one':
        return n_win
    return 2 if n_win > 2 else 1


def make(name, n, seed):
    s = R.SHAPES[name]
    (wh, ww), (H, W) = s['window'], s['canvas']
    n_win = len(s['oy']) * len(s['ox'])
    chunks = -(-n_win // n)
    g = torch.Generator().manual_seed(seed)
    d = dict(s, n=n, chunks=chunks, n_win=n_win,
             eps=torch.randn(chunks, 2 * n, wh, ww, 4, generator=g).half(), x=3.0 * torch.randn(1, 4, H, W, generator=g),
             den_prev=torch.randn(1, 4, H, W, generator=g), nu=torch.randn(1, 4, H, W, generator=g),
             temb_row=torch.randn(TEMB_W, generator=g).half())
    return d


def tables(d, kind):
    from sdod.amd import panorama as PN
    wgt = PN.window_weights(d['window'], kind)
    wsum = PN.weight_sum(d['canvas'], d['window'], d['oy'], d['ox'], wgt, d['wrap'])
    return torch.from_numpy(wgt), torch.from_numpy(wsum)


def launch(d, eps, cf, wgt, wsum, mode, x, den_prev, noise, stage, guidance=7.5):
    from sdod.amd import ops
    ops.k_step_windows(eps, x, cf, wgt, wsum, d['window'], d['oy'], d['ox'], d['n'], d['chunks'], d['wrap'], guidance=guidance,
                       den_prev=den_prev, noise=noise, seed=SEED, noise_level=LEVEL, image_index=IDX0, mode=mode, stage=stage)
    torch.cuda.synchronize()


@pytest.mark.parametrize('chunking', ['one', 'several'])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('kind', ['uniform', 'gaussian'])
@pytest.mark.parametrize('case', list(COEF))
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_step_equals_the_restatement_bit_for_bit(name, case, kind, mode, chunking):
    from sdod.amd import ops
    n = rows_per_eval(len(R.SHAPES[name]['oy']) * len(R.SHAPES[name]['ox']), chunking)
    d = make(name, n, seed=len(name) * 7 + n)
    cf = coef(case)
    wgt, wsum = tables(d, kind)
    H, W = d['canvas']
    nu = d['nu']
    if case == 'euler_a_device':      # drawn in the kernel == sdod_randn_f32 over the canvas on stream ((3 + level) << 32) | image_index
        nu = ops.randn((1, 4, H, W), SEED, ((3 + LEVEL) << 32) | IDX0, 'cuda').cpu()
    with_prev = case in ('dpmpp_2m', 'last')          # DPM++ 2M keeps den_prev through its last step, where cprev == 0
    kw = dict(den_prev=d['den_prev'], nu=nu, guidance=7.5, mode=mode)
    geom = (wgt, wsum, d['oy'], d['ox'], d['window'], d['wrap'], n)
    stage_ref = torch.full((d['chunks'], 2 * n, 4) + d['window'], FILL)
    want_x, want_den = R.step(d['eps'], d['x'], cf, *geom, x_stage=stage_ref, **kw)
    x, dp = d['x'].cuda(), d['den_prev'].cuda()
    stage = torch.full(stage_ref.shape, FILL, device='cuda')
    temb_dst = torch.zeros(2 * n, TEMB_W, dtype=torch.float16, device='cuda')
    launch(d, d['eps'].cuda(), cf, wgt.cuda(), wsum.cuda(), mode, x, dp if with_prev else None, nu.cuda() if case == 'euler_a' else None,
           (stage, d['temb_row'].cuda(), temb_dst))
    assert torch.equal(bits(x.cpu()), bits(want_x))
    assert torch.equal(bits(stage.cpu()), bits(stage_ref))              # the spare rows of a partly filled chunk keep FILL
    assert torch.equal(temb_dst.cpu(), d['temb_row'][None].expand(2 * n, -1))
    if with_prev:
        assert torch.equal(bits(dp.cpu()), bits(want_den))
    if case == 'last':
        assert torch.equal(x, dp)
    used = d['n_win']
    spare = stage.view(-1, 4, *d['window']).cpu()
    for w in range(d['chunks'] * n):
        rows = [(w // n) * 2 * n + w % n, (w // n) * 2 * n + n + w % n]
        assert bool((spare[rows] == FILL).all()) == (w >= used)
    # the negative control: "last window wins" is another function wherever more than one window covers an element
    multi = (R.cover_count(d['oy'], d['ox'], d['window'], d['canvas'], d['wrap']) > 1)[None, None].expand(1, 4, H, W)
    if int(multi.sum()):
        wrong, _ = R.step(d['eps'], d['x'], cf, *geom, last_wins=True, **kw)
        differs = (bits(wrong) != bits(x.cpu()))[multi].float().mean()
        assert float(differs) > 0.5, float(differs)
    else:
        assert name in ('rect_window', 'identity')


@pytest.mark.parametrize('case', list(COEF) + ['start'])
def test_one_window_equal_to_the_canvas_is_k_step(case):
    """16 x 16, weight 1: x, den_prev and x_stage bit-equal to ops.k_step on the same inputs"""
    from sdod.amd import ops
    d = make('identity', 1, seed=31)
    cf = dict(a=14.614641489691584, stage_scale=STAGE_SCALE) if case == 'start' else coef(case)
    one = torch.ones(16, 16, device='cuda')
    eps = None if case == 'start' else d['eps'].cuda()
    with_prev = case in ('dpmpp_2m', 'last')
    noise = d['nu'].cuda() if case == 'euler_a' else None
    got, want = {}, {}
    for out, fn in ((want, 'k_step'), (got, 'k_step_windows')):
        out['x'], out['dp'] = d['x'].cuda(), d['den_prev'].cuda()
        out['stage'] = torch.full((2, 4, 16, 16), FILL, device='cuda')
        out['temb'] = torch.zeros(2, TEMB_W, dtype=torch.float16, device='cuda')
        kw = dict(den_prev=out['dp'] if with_prev else None, noise=noise, seed=SEED, noise_level=LEVEL, image_index=IDX0, mode=1,
                  stage=(out['stage'], d['temb_row'].cuda(), out['temb']))
        if fn == 'k_step':
            ops.k_step(None if eps is None else eps[0], out['x'], cf, 7.5, **kw)
        else:
            ops.k_step_windows(eps, out['x'], cf, one, one, (16, 16), [0], [0], 1, 1, False, guidance=7.5, **kw)
    torch.cuda.synchronize()
    for key in want:
        assert torch.equal(bits(got[key].float()), bits(want[key].float())), key
    assert not torch.equal(got['x'], d['x'].cuda()) and not bool((got['stage'] == FILL).any())


@pytest.mark.parametrize('name', ['cover_1_2', 'wrap', 'grid_2x2'])
def test_start_form(name):
    d = make(name, 3, seed=11)                          # three rows per evaluation: four windows leave two spare rows
    wgt, wsum = tables(d, 'gaussian')
    cf = dict(a=14.614641489691584, stage_scale=STAGE_SCALE)
    stage_ref = torch.full((d['chunks'], 6, 4) + d['window'], FILL)
    want_x, _ = R.step(None, d['x'], cf, wgt, wsum, d['oy'], d['ox'], d['window'], d['wrap'], 3, x_stage=stage_ref)
    x, dp = d['x'].cuda(), d['den_prev'].cuda()
    stage = torch.full(stage_ref.shape, FILL, device='cuda')
    temb_dst = torch.zeros(6, TEMB_W, dtype=torch.float16, device='cuda')
    launch(d, None, cf, wgt.cuda(), wsum.cuda(), 1, x, dp, torch.full_like(x, float('nan')), (stage, d['temb_row'].cuda(), temb_dst))
    assert torch.equal(bits(x.cpu()), bits(want_x)) and torch.equal(bits(stage.cpu()), bits(stage_ref))
    assert torch.equal(dp.cpu(), d['den_prev'])                                       # the start form leaves the history alone
    assert bool((stage[1, 1] == FILL).all()) and bool((stage[1, 2] == FILL).all()) and bool((stage[1, 4:] == FILL).all())
    assert not bool((stage[1, 0] == FILL).any()) and not bool((stage[1, 3] == FILL).any())
    assert torch.equal(temb_dst.cpu(), d['temb_row'][None].expand(6, -1))


def test_noise_is_touched_only_when_u_is_not_zero():
    d = make('grid_2x2', 4, seed=3)
    wgt, wsum = tables(d, 'uniform')
    outs = []
    for noise in (None, torch.full((1, 4, 24, 24), float('nan'), device='cuda')):
        x = d['x'].cuda()
        launch(d, d['eps'].cuda(), coef('euler'), wgt.cuda(), wsum.cuda(), 1, x, None, noise, None)
        outs.append(x)
    assert torch.equal(bits(outs[0]), bits(outs[1])) and bool(torch.isfinite(outs[0]).all())


def test_refusals_leave_the_destinations_untouched():
    """every refusal of include/sdod_hip.h's list (panorama_ref.REFUSALS; the same cases test_panorama_cpu.py sends without a device):
    INVALID_ARGUMENT, and x, den_prev, x_stage, temb_dst keep their bytes; then the good call goes through"""
    from sdod.amd import _lib, ops
    lib = _lib.hip()
    b = R.BASE
    g = torch.Generator().manual_seed(2)
    t = dict(eps=torch.randn(b['chunks'], 2 * b['n'], b['wh'], b['ww'], b['c'], generator=g).half().cuda(),
             x=torch.randn(1, b['c'], b['H'], b['W'], generator=g).cuda(), den_prev=torch.randn(1, b['c'], b['H'], b['W'], generator=g).cuda(),
             noise=torch.randn(1, b['c'], b['H'], b['W'], generator=g).cuda(), wgt=torch.ones(b['wh'], b['ww'], device='cuda'),
             wsum=torch.ones(b['H'], b['W'], device='cuda'),
             x_stage=torch.full((b['chunks'], 2 * b['n'], b['c'], b['wh'], b['ww']), FILL, device='cuda'),
             temb_row=torch.randn(TEMB_W, generator=g).half().cuda(), temb_dst=torch.zeros(2 * b['n'], TEMB_W, dtype=torch.float16, device='cuda'))
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    keep = {k: t[k].clone() for k in ('x', 'den_prev', 'x_stage', 'temb_dst')}
    for label, over in R.REFUSALS:
        a = R.fill_args(ptrs, over, temb=(TEMB_W, 2 * b['n']))
        assert lib.sdod_k_step_windows(a, ops._stream()) == 2, label
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(bits(t[k].float()), bits(v.float())), k
    assert lib.sdod_k_step_windows(R.fill_args(ptrs, None, temb=(TEMB_W, 2 * b['n'])), ops._stream()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(t['x'], keep['x']) and not torch.equal(t['den_prev'], keep['den_prev'])
    assert bool((t['temb_dst'] == t['temb_row']).all())
    assert not bool((t['x_stage'][0] == FILL).any()) and not bool((t['x_stage'][1, 0] == FILL).any()) and bool((t['x_stage'][1, 1] == FILL).all())
    # ... and ops.k_step_windows raises SdodError for them
    with pytest.raises(_lib.SdodError):
        ops.k_step_windows(t['eps'], t['x'], coef('euler'), t['wgt'], t['wsum'], (16, 16), [0], [0, 6, 16], 2, 2)
    with pytest.raises(_lib.SdodError):
        ops.k_step_windows(t['eps'], t['x'], dict(coef('euler'), a=float('nan')), t['wgt'], t['wsum'], (16, 16), [0], [0, 8, 16], 2, 2)
