"""Regional prompts, host side (no GPU): the weight definition, the fp32 restatement on the oracle UNet, the mask helpers, the argument
checks, the host plan of the region score GEMM, and the exported symbols.  The GPU side is tests/test_regions_kernel_gpu.py (kernels)
and tests/test_regions_gpu.py (graph and pipeline)."""
import ctypes

import numpy as np
import pytest
import torch

import regions_ref as RR


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------ the weight definition
@pytest.mark.parametrize('hw,k', [((8, 8), 2), ((8, 16), 3), ((16, 24), 4)])
def test_weights_sum_to_one_and_are_the_box_sums(hw, k):
    masks = RR.soft_masks(hw, k, seed=5 + k)
    masks[:, 8:24, 16:40] = 0                                       # a hole no region covers: image rows 8..23, columns 16..39
    ws = RR.region_weights(masks)
    assert [tuple(w.shape) for w in ws] == [((hw[0] // ds) * (hw[1] // ds), k) for ds in RR.LEVELS]
    for ds, w in zip(RR.LEVELS, ws):
        assert w.dtype == torch.float32 and bool((w >= 0).all()) and float((w.sum(1) - 1).abs().max()) <= 2e-7 * k
        s = RR.region_sums(masks, ds)
        # exact integer sums, by another route: one pixel's box summed directly
        y, x = hw[0] // ds - 1, hw[1] // ds // 2
        b = 8 * ds
        assert [int(v) for v in s[:, y, x]] == [int(masks[r, y * b:(y + 1) * b, x * b:(x + 1) * b].to(torch.int64).sum()) for r in range(k)]
        tot = s.sum(0)
        wv = w.view(hw[0] // ds, hw[1] // ds, k)
        if ds == 1:                                                   # latent pixels (1, 2), (1, 3), (1, 4) and (2, 2..4) lie inside the hole
            assert int(tot[1, 2]) == 0 and int(tot[2, 4]) == 0
            assert wv[1, 2].tolist() == [1.0] + [0.0] * (k - 1) and wv[2, 4].tolist() == [1.0] + [0.0] * (k - 1)
        nz = tot > 0
        ref = (torch.from_numpy(s).double() / torch.from_numpy(np.where(nz, tot, 1)).double()[None]).permute(1, 2, 0)
        assert float((wv.double() - ref)[torch.from_numpy(nz)].abs().max()) <= 2.0 ** -24     # one fp32 rounding of the exact quotient


def test_a_hard_split_off_the_latent_grid_gives_fractional_weights_on_one_column():
    ws = RR.region_weights(RR.column_split((16, 16), 52))            # pixel column 52 = latent column 6.5
    w = ws[0].view(16, 16, 2)
    assert bool((w[:, :6, 0] == 1).all()) and bool((w[:, 7:, 1] == 1).all()) and bool((w[:, 6] == 0.5).all())
    assert bool((ws[3].view(2, 2, 2)[:, 0, 0] == np.float32(52) / np.float32(64)).all()) and bool((ws[3].view(2, 2, 2)[:, 1, 1] == 1).all())
    bg = RR.background_weights(2, (16, 16))
    only0 = torch.zeros(2, 128, 128, dtype=torch.uint8); only0[0] = 255
    assert all(torch.equal(a, b) for a, b in zip(RR.region_weights(only0), bg))
    assert all(torch.equal(a, b) for a, b in zip(RR.region_weights(torch.zeros(2, 128, 128, dtype=torch.uint8)), bg))   # nothing covered


def test_blend_definition_rounds_every_operation():
    g = torch.Generator().manual_seed(3)
    a = (torch.randn(3, 16, 8, generator=g) * torch.exp2(torch.randint(-6, 7, (3, 16, 8), generator=g).float())).half()
    w = torch.rand(8, 3, generator=g)
    out = RR.region_blend(a, w)
    wr = w[torch.arange(16) % 8]
    exact = sum(wr[:, r:r + 1].double() * a[r].double() for r in range(3))
    assert out.dtype == torch.float16 and float((out.double() - exact).abs().max()) <= float(exact.abs().max()) * 2.0 ** -10
    one = torch.zeros(8, 3); one[:, 1] = 1
    assert torch.equal(RR.region_blend(a, one), a[1])


# ------------------------------------------------------------------ the restatement on the fp32 oracle UNet
@pytest.fixture(scope='module')
def oracle_unet():
    from oracle import sd_torch as S
    unet = S.build(S.UNetModel, seed=1234)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 4, 16, 16, generator=g)
    t = torch.tensor([500.0, 500.0])
    ctx = torch.randn(2, 3 * 77, 768, generator=g) * 0.5
    return unet, x, t, ctx


def test_restatement_same_prompt_and_background(oracle_unet):
    unet, x, t, ctx = oracle_unet
    with torch.no_grad():
        plain = unet(x, t, ctx[:, :77])
    same = torch.cat([ctx[:, :77]] * 2, 1)
    out = RR.regional_unet(unet, RR.region_weights(RR.soft_masks((16, 16), 2, seed=1)))(x, t, same)
    r = rel_l2(out, plain)
    print(f'same prompt in both regions, random soft masks, vs the plain UNet: rel-L2 {r:.2e}')
    assert r <= 1e-5, r
    out0 = RR.regional_unet(unet, RR.background_weights(2, (16, 16)))(x, t, ctx[:, :154])
    assert torch.equal(out0, plain)                                   # region 0 everywhere: the plain UNet on the first 77 rows, exactly
    assert 'forward' not in vars(unet.middle_block[1].transformer_blocks[0].attn2)          # the wrapper leaves the model as it found it


def test_restatement_masks_matter(oracle_unet):
    unet, x, t, ctx = oracle_unet
    m = RR.column_split((16, 16), 52)
    a = RR.regional_unet(unet, RR.region_weights(m))(x, t, ctx[:, :154])
    b = RR.regional_unet(unet, RR.region_weights(m.flip(0)))(x, t, ctx[:, :154])
    r = rel_l2(a, b)
    print(f'two regions split at pixel column 52, then swapped: rel-L2 {r:.3f}')
    assert r > 5e-2, r


# ------------------------------------------------------------------ mask helpers
def test_column_row_masks_and_feather():
    from sdod.amd import regions as RG
    m = RG.column_masks([1, 1], 16)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (2, 128, 128)
    assert bool((m[0, :, :64] == 255).all()) and bool((m[0, :, 64:] == 0).all()) and bool((m.sum(0) == 255).all())
    m3 = RG.column_masks([1, 2, 1], (8, 16))
    assert tuple(m3.shape) == (3, 64, 128) and [int(m3[r, 0].sum()) // 255 for r in range(3)] == [32, 64, 32] and bool((m3.sum(0) == 255).all())
    r2 = RG.row_masks([3, 1], (8, 16))
    assert tuple(r2.shape) == (2, 64, 128) and bool((r2[0, :48] == 255).all()) and bool((r2[1, 48:] == 255).all()) and bool((r2.sum(0) == 255).all())
    assert torch.equal(RG.row_masks([1, 1], (16, 8)), RG.column_masks([1, 1], (8, 16)).transpose(1, 2))
    f = RG.feather(m, 4)
    assert f.dtype == torch.uint8 and f.shape == m.shape and torch.equal(RG.feather(m, 0), m)
    assert bool((f[0, :, :60] == 255).all()) and bool((f[0, :, 68:] == 0).all())                      # untouched 4 px from the border
    col = f[0, 5].to(torch.int64)
    assert bool((col[59:69].diff() < 0).all()) and int((f.to(torch.int64).sum(0) - 255).abs().max()) <= 1     # a ramp; still a partition
    assert torch.equal(f[0, 0], f[0, 77])                                                               # edges repeat: no darkening
    assert torch.equal(RG.feather(m.numpy(), 4), f)
    for bad in ([1], [1, 1, 1, 1, 1], [1, 0], [1, -1], [1, float('nan')], [1e-9, 1]):
        with pytest.raises(ValueError):
            RG.column_masks(bad, 16)
    for bad in (12, (8, 9), 0, (16,), 4):
        with pytest.raises((ValueError, TypeError)):
            RG.row_masks([1, 1], bad)
    for bad in (-1, 1.5, True, 1000):
        with pytest.raises(ValueError):
            RG.feather(m, bad)


# ------------------------------------------------------------------ argument checks
@pytest.mark.parametrize('kw', [dict(prompt_chunks=2), dict(cfg_split=True), dict(hires_hw=32), dict(controlnet=True), dict(adapter=True),
                                dict(tiling=True), dict(tiling='x'), dict(inpaint_unet=True), dict(model='sd21'), dict(weight_quant=True),
                                dict(weight_quant='auto')])
def test_regions_check_build_refuses_before_any_device_work(kw):
    from sdod.amd import pipeline as PL, regions as RG
    assert RG.regions_check_build(2) == 2 and RG.regions_check_build(4) == 4 and RG.regions_check_build(np.int64(3)) == 3
    assert RG.regions_check_build(False, **kw) == 0 and RG.regions_check_build(None, **kw) == 0      # without the flag nothing is checked
    with pytest.raises(ValueError, match='regions cannot be combined'):
        RG.regions_check_build(2, **kw)
    with pytest.raises(ValueError, match='regions'):                    # the constructor: before it touches the device
        PL.Txt2Img(state_dicts={}, latent_hw=16, regions=2, **kw)


@pytest.mark.parametrize('bad', [1, 5, 0, True, 2.0, '2', -2])
def test_regions_check_build_refuses_bad_counts(bad):
    from sdod.amd import pipeline as PL, regions as RG
    with pytest.raises(ValueError, match='regions must be'):
        RG.regions_check_build(bad)
    with pytest.raises(ValueError, match='regions must be'):
        PL.Txt2Img(state_dicts={}, latent_hw=16, regions=bad)


def test_uint8_weights_in_the_state_dict_are_refused():
    from sdod.amd import pipeline as PL

    class Codes:
        shape = (320, 320)

        def payload(self):
            return b''
    with pytest.raises(ValueError, match='regions cannot be combined with uint8 weights'):
        PL.Txt2Img(state_dicts={'unet': {'w': Codes()}}, latent_hw=16, regions=2)


def test_regions_check_args_and_the_setters_need_the_flag():
    from sdod.amd import engine as E, regions as RG
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    assert pipe.regions == 0
    for call in (lambda: pipe.set_regions(torch.zeros(2, 128, 128, dtype=torch.uint8)), pipe.clear_regions,
                 lambda: pipe.encode_regions(['a', 'b'])):
        with pytest.raises(RuntimeError, match='regions=k'):
            call()
    pipe.regions = 3
    pipe.cfg = E.sd14_config(8, 16)
    good = torch.zeros(3, 64, 128, dtype=torch.uint8)
    assert RG.regions_check_args(pipe, good) is good or torch.equal(RG.regions_check_args(pipe, good), good)
    out = RG.regions_check_args(pipe, good.numpy())
    assert torch.is_tensor(out) and out.dtype == torch.uint8 and tuple(out.shape) == (3, 64, 128)
    assert RG.regions_check_args(pipe, good.transpose(1, 2).contiguous().transpose(1, 2)).is_contiguous()
    bads = [good.float(), good.to(torch.int32), good.numpy().astype(np.float32), good[:2], torch.zeros(4, 64, 128, dtype=torch.uint8),
            good[:, :32], torch.zeros(3, 128, 64, dtype=torch.uint8), good[0], good[None], [[0]], None]
    for bad in bads:
        with pytest.raises(ValueError):
            RG.regions_check_args(pipe, bad)
        with pytest.raises(ValueError):
            pipe.set_regions(bad)                                     # raises before any device work (there is no device object here)
    for bad in (['a', 'b'], ['a', 'b', 'c', 'd'], 'abc', ['a', 'b', 3], None, ('a', 'b', None)):
        with pytest.raises(ValueError, match='exactly 3'):
            pipe.encode_regions(bad)
    with pytest.raises(ValueError, match='negative'):
        pipe.encode_regions(['a', 'b', 'c'], negative=['x'] * 3)


# ------------------------------------------------------------------ library, host side
def _score_desc(n, rows_per_img=256, k=320, batch=2):
    from sdod.amd import _lib
    d = _lib.GemmDesc()
    d.M, d.N, d.K = batch * rows_per_img, n, k
    d.lda, d.ldw, d.ldo = k, k, n
    d.ln, d.softmax_cols, d.rows_per_img = 1, 80, rows_per_img
    d.w_img_stride, d.vec_img_stride = n * k, n
    return d


@pytest.mark.parametrize('n', [1280, 1920])
@pytest.mark.parametrize('rows,k', [(256, 320), (64, 640), (4096, 320), (32, 1280), (96, 1280)])
def test_host_plan_names_a_wave80_ring_tile_for_the_region_score_gemm(n, rows, k):
    """N = regions * heads * 80 = 1280 (k = 2) and 1920 (k = 3): the plan must land on a tile whose waves own 80 columns (the softmax
    epilogue's group) in the LDS-DMA ring family, with rows that divide the image"""
    from sdod.amd import _lib
    lib = _lib.hip()
    d = _score_desc(n, rows, k)
    tile, splits = ctypes.c_int(), ctypes.c_int()
    assert lib.sdod_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(splits)) == 0
    info = (ctypes.c_int * 7)()
    assert lib.sdod_gemm_tile_info(tile.value, info) == 0
    bm, bn, wm, wn, stages, spec = info[0], info[1], info[2], info[3], info[4], info[5]
    assert bn // wn == 80 and stages > 0 and spec == 1 and rows % bm == 0 and splits.value == 1, (tile.value, list(info), splits.value)


def test_new_symbols_are_exported_and_bound():
    from sdod.amd import _lib, engine as E, ops
    lib = _lib.hip()
    for s in ('sdod_gemm_region_f16', 'sdod_xattn_fold_regions_f16', 'sdod_region_weights_f32', 'sdod_region_blend_f16'):
        assert s in _lib.HIP_SYMBOLS and getattr(lib, s).argtypes is not None
    E._engine()
    assert 'sdod_graph_create_regions' in E.ENGINE_SYMBOLS and lib.sdod_graph_create_regions.argtypes is not None
    assert all(hasattr(ops, n) for n in ('region_weights', 'region_blend'))
    assert E.RegionConfig._fields_ == [('regions', ctypes.c_int)] and ctypes.sizeof(E.RegionConfig) == 4
    # the public layouts did not move
    assert _lib.GemmDesc._fields_[-1][0] == 'pad_mode' and ctypes.sizeof(E.ModelConfig) == 16 * 4 and ctypes.sizeof(E.AdapterConfig) == 12


def test_region_config_travels_with_copies_and_changes_no_parameter():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    assert cfg.regions == 0 and E.copy_config(cfg).regions == 0
    c2 = E.copy_config(cfg); c2.context_len = 154; c2.regions = 2
    assert E.copy_config(c2).regions == 2 and E.copy_config(c2).context_len == 154 and cfg.regions == 0
    assert E.UNet(c2, 2).param_table() == E.UNet(cfg, 2).param_table()          # same checkpoint; the table is readable without a device
    c3 = E.copy_config(cfg); c3.regions = 2                                    # context_len must be 77 * regions
    with pytest.raises(Exception, match='context_len'):
        E.UNet(c3, 2)
    for bad in (1, 5):
        cb = E.copy_config(cfg); cb.regions = bad; cb.context_len = 77 * bad
        with pytest.raises(Exception, match='regions'):
            E.UNet(cb, 2)
    ca = E.copy_config(c2); ca.adapter_reps = 2
    with pytest.raises(ValueError, match='regions'):
        E.UNet(ca, 2)
