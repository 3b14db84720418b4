"""MultiDiffusion panoramas on the host: the window plan, the weights and their sum (sdod/amd/panorama.py), the float64 restatement's
partition of unity (tests/panorama_ref.py), and the argument contracts of Txt2Img(canvas_hw=...) and its entry points.  No device."""
import numpy as np
import pytest
import torch

import panorama_ref as R
from sdod.amd import panorama as PN
from sdod.amd._lib import PANO_MAX_AXIS


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_plan_windows_gives_the_listed_origins_and_covers_the_canvas(name):
    s = R.SHAPES[name]
    oy, ox = PN.plan_windows(s['canvas'], s['window'], s['stride'], s['wrap'])
    assert (list(oy), list(ox)) == (s['oy'], s['ox'])
    assert all(isinstance(v, int) and v % 8 == 0 for v in list(oy) + list(ox))
    cnt = R.cover_count(oy, ox, s['window'], s['canvas'], s['wrap'])
    assert int(cnt.min()) >= 1
    if s['wrap']:
        assert int(cnt.min()) == int(cnt.max()) == 2
    # the listed cover counts
    want = {'cover_1_2': (1, 2), 'clamped_last': (1, 2), 'grid_2x2': (1, 4), 'wrap': (2, 2), 'rect_window': (1, 1), 'identity': (1, 1)}[name]
    assert (int(cnt.min()), int(cnt.max())) == want
    if name == 'grid_2x2':
        assert int(cnt[12, 12]) == 4 and int(cnt[0, 0]) == 1
    if name == 'wrap':           # one window lies across the seam
        assert ox[-1] + s['window'][1] > s['canvas'][1]


def test_plan_windows_identity_for_any_stride_and_larger_canvases():
    for stride in (8, 16, (8, 16), (16, 8)):
        assert PN.plan_windows((16, 16), (16, 16), stride) == ([0], [0])
    assert PN.plan_windows((64, 256), (64, 64), 32) == ([0], [0, 32, 64, 96, 128, 160, 192])
    assert PN.plan_windows((64, 256), (64, 64), 32, True) == ([0], [0, 32, 64, 96, 128, 160, 192, 224])
    assert PN.plan_windows((16, 40), 16, 8) == ([0], [0, 8, 16, 24])            # an integer is a square window
    for wrap in (False, True):   # every pixel covered, every origin a multiple of 8, on a grid of shapes
        for W in (16, 32, 48, 64):
            for s in (8, 16):
                oy, ox = PN.plan_windows((24, W), (16, 16), s, wrap)
                cnt = R.cover_count(oy, ox, (16, 16), (24, W), wrap)
                assert int(cnt.min()) >= 1 and all(v % 8 == 0 for v in oy + ox)
                if wrap:
                    assert len(set(cnt[0].tolist())) == 1


@pytest.mark.parametrize('args', [
    ((16, 40), (16, 16), 4),               # a stride below 8
    ((16, 40), (16, 16), 12),              # no multiple of 8
    ((16, 40), (16, 16), 24),              # larger than the window side
    ((16, 40), (16, 16), (8, 24)),
    ((16, 40), (16, 16), 0),
    ((16, 40), (16, 16), 8.0),             # not an integer
    ((16, 40), (16, 16), (8, 8, 8)),
    ((16, 40), (16, 16), None),
    ((16, 40), (16, 48), 8),               # the window is larger than the canvas
    ((16, 40), (24, 16), 8),
    ((16, 36), (16, 16), 8),               # canvas no multiple of 8
    ((16, 40), (16, 12), 8),               # window no multiple of 8
    ((16, 40, 2), (16, 16), 8),
    ((16, 40), (16, 16), 16, True),        # wrap: W % stride != 0
    ((16, 8 * (PANO_MAX_AXIS + 2)), (16, 16), 8),          # 33 origins on the x axis
    ((16, 8 * (PANO_MAX_AXIS + 1)), (16, 16), 8, True),    # 33 with wrap
])
def test_plan_windows_refusals(args):
    with pytest.raises(ValueError):
        PN.plan_windows(*args)


def test_plan_windows_at_the_axis_limit():
    oy, ox = PN.plan_windows((16, 8 * (PANO_MAX_AXIS + 1)), (16, 16), 8)
    assert len(ox) == PANO_MAX_AXIS and ox[-1] == 8 * (PANO_MAX_AXIS + 1) - 16
    assert len(PN.plan_windows((16, 8 * PANO_MAX_AXIS), (16, 16), 8, True)[1]) == PANO_MAX_AXIS


def test_gaussian_weights():
    for hw in ((64, 64), (16, 16), (8, 16)):
        w = PN.window_weights(hw, 'gaussian')
        assert w.dtype == np.float32 and w.shape == hw
        assert np.array_equal(w, w[::-1]) and np.array_equal(w, w[:, ::-1])
        assert float(w.min()) > 0.0
        c = w[hw[0] // 2 - 1:hw[0] // 2 + 1, hw[1] // 2 - 1:hw[1] // 2 + 1]          # the four centre pixels share the maximum
        assert float(c.min()) == float(c.max()) == float(w.max()) and int((w == w.max()).sum()) == 4
    # the stated formula at one point, in float64, rounded once
    L, i, j = 64, 5, 40
    ax = lambda k: np.exp(-(k - (L - 1) / 2) ** 2 / (L * L) / (2 * 0.01)) / np.sqrt(2 * np.pi * 0.01)
    assert PN.window_weights((64, 64), 'gaussian')[i, j] == np.float32(ax(i) * ax(j))
    u = PN.window_weights((8, 16), 'uniform')
    assert u.dtype == np.float32 and u.shape == (8, 16) and bool((u == 1).all())
    with pytest.raises(ValueError):
        PN.window_weights((16, 16), 'cosine')


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_weight_sum_is_the_cover_count_and_the_average_is_a_partition_of_unity(name):
    s = R.SHAPES[name]
    win, can, wrap, oy, ox = s['window'], s['canvas'], s['wrap'], s['oy'], s['ox']
    ws = PN.weight_sum(can, win, oy, ox, PN.window_weights(win, 'uniform'), wrap)
    assert ws.dtype == np.float32 and ws.shape == can
    assert np.array_equal(ws, R.cover_count(oy, ox, win, can, wrap).numpy().astype(np.float32))
    g = PN.window_weights(win, 'gaussian')
    wsg = PN.weight_sum(can, win, oy, ox, g, wrap)
    cnt = R.cover_count(oy, ox, win, can, wrap).numpy()
    single = np.zeros(can, dtype=np.float32)                      # a pixel under one window of weight v has v exactly
    for _, rows, cols in R.windows(oy, ox, win, can, wrap):
        single[rows.numpy(), cols.numpy()] = g
    assert np.array_equal(wsg[cnt == 1], single[cnt == 1])
    # float64: equal predictions in every window come back exactly -- a constant (uniform weights: k v / k), and any canvas field
    # whose crops the windows predict (the windows agree where they overlap)
    n_win = len(oy) * len(ox)
    for n in (1, 2, n_win):
        chunks = -(-n_win // n)
        eps = torch.full((chunks, 2 * n) + win + (4,), 0.37109375, dtype=torch.float16)
        e = R.averaged(eps, torch.from_numpy(PN.window_weights(win, 'uniform')), torch.from_numpy(ws), oy, ox, win, can, wrap, n, 7.5, 1,
                       torch.float64)
        assert e.shape == (4,) + can and bool((e == 0.37109375).all())
    e = R.averaged(eps, torch.from_numpy(g).double(), torch.from_numpy(wsg.astype(np.float64)), oy, ox, win, can, wrap, n, 7.5, 1, torch.float64)
    # gaussian: sum(w v) / wsum with wsum summed in float32 -- at most 3 additions of 2^-24 relative each
    assert float((e - 0.37109375).abs().max()) <= 0.37109375 * 4 * 2.0 ** -24


def test_restatement_step_in_float64_is_the_linear_form():
    """the float64 step on one window equal to the canvas is den = d0 x + d1 CFG, x' = a x + b den + cprev den_prev + u nu"""
    g = torch.Generator().manual_seed(5)
    eps = torch.randn(1, 2, 16, 16, 4, generator=g).half()
    x, dp, nu = (torch.randn(1, 4, 16, 16, generator=g, dtype=torch.float64) for _ in range(3))
    coef = dict(d0=1.0, d1=-4.5, a=0.77, b=0.35, cprev=-0.12, u=0.5, stage_scale=0.25)
    one = torch.ones(16, 16)
    stage = torch.zeros(1, 2, 4, 16, 16, dtype=torch.float64)
    xn, den = R.step(eps, x, coef, one, one, [0], [0], (16, 16), False, 1, 7.5, 1, dp, nu, stage, torch.float64)
    eu, ec = eps[0, 0].double().permute(2, 0, 1), eps[0, 1].double().permute(2, 0, 1)
    e = eu + 7.5 * (ec - eu)
    want_den = x[0] - 4.5 * e
    assert torch.allclose(den[0], want_den, rtol=1e-14, atol=1e-14)
    assert torch.allclose(xn[0], 0.77 * x[0] + 0.35 * want_den - 0.12 * dp[0] + 0.5 * nu[0], rtol=1e-14, atol=1e-14)
    assert torch.equal(stage[0, 0], 0.25 * xn[0]) and torch.equal(stage[0, 1], stage[0, 0])


@pytest.mark.parametrize('label,over', R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_host_entry_refuses_before_any_launch(label, over):
    """sdod_k_step_windows checks its arguments on the host before it touches the device: every refusal comes back as
    INVALID_ARGUMENT (2) on a machine without one, with addresses nobody reads"""
    from sdod.amd import _lib
    lib = _lib.hip()
    fake = {p: 0x10000 * (i + 1) for i, p in enumerate(R.POINTERS)}
    a = R.fill_args(fake, over, temb=(520, 4))
    assert lib.sdod_k_step_windows(a, None) == 2, label
    assert lib.sdod_hip_last_error()


# ---------------------------------------------------------------------------------------------------------------- contracts
@pytest.mark.parametrize('kw,why', [
    (dict(cfg_split=True), 'cfg_split'), (dict(inpaint_unet=True), 'inpaint_unet'), (dict(hires_hw=(24, 32)), 'hires_hw'),
    (dict(adapter=True), 'adapter'), (dict(controlnet=True), 'controlnet'), (dict(regions=2), 'regions'),
    (dict(ip_adapter=True), 'ip_adapter'), (dict(tiling=True), 'tiling'), (dict(tiling='x'), 'tiling'), (dict(upscaler=True), 'upscaler'),
])
def test_constructor_refuses_the_options_that_need_canvas_sized_state(kw, why):
    from sdod.amd.pipeline import Txt2Img
    with pytest.raises(ValueError, match=f'canvas_hw cannot be combined with {why}: '):
        Txt2Img(state_dicts=None, latent_hw=16, canvas_hw=(16, 32), **kw)
    with pytest.raises(ValueError, match=f'canvas_hw cannot be combined with {why}: '):
        PN.panorama_check_build((16, 32), False, (16, 16), **kw)


@pytest.mark.parametrize('canvas_hw', [(16, 36), (12, 32), (16, 8), (8, 32), 8, (16,), (16, 32, 4), (16.0, 32), 'wide', (True, 32), (0, 32)])
def test_constructor_refuses_a_bad_canvas(canvas_hw):
    from sdod.amd.pipeline import Txt2Img
    with pytest.raises(ValueError, match='canvas_hw'):
        Txt2Img(state_dicts=None, latent_hw=16, canvas_hw=canvas_hw)


def test_check_build_passes_what_it_should():
    assert PN.panorama_check_build(None, False, (16, 16)) is None
    assert PN.panorama_check_build(None, False, (16, 16), tiling=True, hires_hw=(24, 24), regions=2) is None       # off: nobody's business
    assert PN.panorama_check_build((16, 32), True, (16, 16)) == (16, 32)
    assert PN.panorama_check_build(32, False, (16, 24)) == (32, 32)
    assert PN.panorama_check_build((16, 16), False, 16) == (16, 16)
    with pytest.raises(ValueError, match='canvas_wrap'):
        PN.panorama_check_build(None, True, (16, 16))
    with pytest.raises(ValueError, match='canvas_wrap'):
        PN.panorama_check_build((16, 32), 'x', (16, 16))


def bare(canvas_hw, wrap=False, n=2):
    """a Txt2Img without its constructor: what the argument checks read"""
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    p = Txt2Img.__new__(Txt2Img)
    p.cfg, p.n, p.device, p.canvas_hw, p.canvas_wrap = E.sd14_config(16, 16), n, torch.device('cpu'), canvas_hw, wrap
    return p


@pytest.mark.parametrize('entry', ['sample_panorama', 'generate_panorama', 'generate_panorama_graphed'])
def test_entry_points_refuse_bad_arguments_before_any_device_work(entry):
    ctx2 = torch.zeros(2, 77, 768, dtype=torch.float16)
    x_T = torch.zeros(1, 4, 16, 40)
    run = getattr(bare((16, 40)), entry)
    for sampler in ('plms', 'dpm', 'ddim', None):
        with pytest.raises(ValueError, match='sampler must be one of'):
            run(ctx2, x_T, sampler, 4)
    for stride in (4, 12, 24, (8, 32), 0, 8.5, (8,), 'half'):
        with pytest.raises(ValueError, match='stride'):
            run(ctx2, x_T, 'euler', 4, stride=stride)
    with pytest.raises(ValueError, match='weights must be one of'):
        run(ctx2, x_T, 'euler', 4, weights='cosine')
    for bad in (torch.zeros(1, 4, 16, 16), torch.zeros(2, 4, 16, 40), torch.zeros(4, 16, 40), torch.zeros(1, 4, 16, 40, dtype=torch.float64), None):
        with pytest.raises(ValueError, match='x_T must be'):
            run(ctx2, bad, 'euler', 4)
    with pytest.raises(ValueError, match='steps'):
        run(ctx2, x_T, 'euler', 0)
    with pytest.raises(ValueError, match='schedule'):
        run(ctx2, x_T, 'euler', 4, schedule='cosine')
    with pytest.raises(ValueError, match='eta'):
        run(ctx2, x_T, 'euler_a', 4, eta=-1.0)
    with pytest.raises(ValueError, match='step_noise'):
        run(ctx2, x_T, 'euler', 4, step_noise=torch.zeros(3, 1, 4, 16, 40))
    with pytest.raises(ValueError, match='step_noise'):
        run(ctx2, x_T, 'euler_a', 4, step_noise=torch.zeros(3, 1, 4, 16, 16))      # the window's shape, not the canvas's
    with pytest.raises(ValueError, match='built without canvas_hw'):
        getattr(bare(None), entry)(ctx2, x_T, 'euler', 4)
    # wrap: the stride must divide the canvas width -- the default (8) does at 40, 16 does not
    with pytest.raises(ValueError, match='stride'):
        getattr(bare((16, 40), wrap=True), entry)(ctx2, x_T, 'euler', 4, stride=16)


def test_check_args_returns_the_plan():
    x = torch.zeros(1, 4, 16, 40)
    assert PN.panorama_check_args((16, 40), (16, 16), False, 2, x, 'euler', None, 'uniform') == ([0], [0, 8, 16, 24], 2)
    assert PN.panorama_check_args((16, 40), (16, 16), False, 2, x, 'dpmpp_2m', 16, 'gaussian') == ([0], [0, 16, 24], 2)
    assert PN.panorama_check_args((16, 40), (16, 16), True, 4, x, 'euler_a', 8, 'uniform') == ([0], [0, 8, 16, 24, 32], 2)
    assert PN.panorama_check_args((16, 40), (16, 16), False, 4, x, 'euler', None, 'uniform')[2] == 1
    x64 = torch.zeros(1, 4, 64, 256)
    assert PN.panorama_check_args((64, 256), (64, 64), False, 1, x64, 'euler', None, 'uniform') == ([0], [0, 32, 64, 96, 128, 160, 192], 7)
