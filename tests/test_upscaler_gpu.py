"""The ESRGAN upscaler on the GPU: the UPSCALER graph against the fp32 restatement (tests/rrdb_ref.py), its structure (launch count,
hipGraph replay, nothing carried between images), the stand-alone class and the pipeline entry points."""
import functools

import pytest
import torch

import rrdb_ref as R

pytestmark = pytest.mark.gpu

# UNet (batch 2) and VAE decoder (batch 1) of Txt2Img(latent_hw=(8, 8)) on the synthetic weights below, as the parent commit builds
# them with SDOD_AUTOTUNE=0: (launches, arena bytes).  A pipeline built without `upscaler` must still report exactly these.  (The
# tune table has no 8 x 8 shapes; tiles timed in the process differ from run to run -- the parent's VAE reported 97 launches twice
# where this tree reported 95 -- so the rig is built with the tuner off: gemm.hip's static plan decides, the same in every process.)
PARENT_UNET = (357, 1065216)
PARENT_VAE = (108, 5767424)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(None)
def reference(nb, b, h, w):
    """(image, spread weights, fp32 float output, uint8 output) of one case, computed once and shared"""
    img = R.sample_image(b, h, w)
    sd = R.spread_weights(nb, img)
    y, u8 = R.upscale(sd, img)
    return img, sd, y, u8


@functools.lru_cache(None)
def graph(nb, b, h, w):
    from sdod.amd import engine as E
    g = E.Upscaler(nb, (h, w), b)
    g.load_state_dict(reference(nb, b, h, w)[1])
    return g.finalize()


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: f'nb{c[0]}')
def test_graph_matches_the_restatement(case):
    """float output within rel-L2 1e-2 of the fp32 restatement (the project's bound for an fp16 graph against its fp32 oracle); the
    uint8 image within 1 LSB at every byte.  The eager run and the hipGraph replay give the same bits."""
    from sdod.amd import ops, upscale as UP
    img, sd, y, u8 = reference(*case)
    g = graph(*case)
    g.img.copy_(img)
    g.execute()
    torch.cuda.synchronize()
    eager = g.out.clone()
    g.out.zero_()
    g.execute(use_hip_graph=True)
    g.execute(use_hip_graph=True)
    torch.cuda.synchronize()
    assert torch.equal(eager.view(torch.int16), g.out.view(torch.int16)), 'hipGraph replay differs from the eager run'
    r = rel_l2(eager, y)
    got = ops.image_to_u8(g.out, UP.U8_A, UP.U8_B, UP.U8_MODE).cpu()
    lsb = int((got.int() - u8.int()).abs().max())
    off = float((got != u8).float().mean())
    print(f'nb {case[0]} batch {case[1]} {case[2]}x{case[3]}: rel-L2 {r:.3e}; uint8 max |diff| {lsb} LSB, {off:.4f} of the bytes differ')
    assert torch.isfinite(eager).all() and r <= 1e-2, r
    assert lsb <= 1, lsb


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: f'nb{c[0]}')
def test_launch_list(case):
    nb = case[0]
    g = graph(*case)
    table = g.op_table()
    assert len(table) == 15 * nb + 6 == g.stats()['launches']
    labels = [t[0] for t in table]
    assert labels[0] == 'image_conv_in_unit' and labels[-1].startswith('gemm_t')
    assert all(l.startswith('dense_conv_n') for l in labels[1:-1]) and labels[1:1 + 15 * nb].count('dense_conv_n64') == 3 * nb
    st = g.stats()
    assert st['arena_bytes'] > 0 and st['weight_bytes'] > 0 and st['flops'] > 0
    b, h, w = case[1:]
    trunk = sum(t[1] for t in table[1:1 + 15 * nb])
    assert trunk == 2.0 * 239616 * 3 * nb * b * h * w          # 239,616 MAC per pixel per RDB


def test_nothing_is_carried_between_images():
    """A, then B, then A returns A's first result bit for bit (stale slices of the wide buffers included)"""
    case = R.CASES[1]
    g = graph(*case)
    a = reference(*case)[0]
    b = R.sample_image(case[1], case[2], case[3], seed=99).flip(1)
    outs = []
    for img in (a, b, a):
        g.img.copy_(img)
        g.execute(use_hip_graph=True)
        torch.cuda.synchronize()
        outs.append(g.out.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))
    assert not torch.equal(outs[0], outs[1])


def test_stand_alone_class_equals_the_graph():
    from sdod.amd import ops, upscale as UP
    nb, b, h, w = R.CASES[1]
    img, sd, y, u8 = reference(nb, b, h, w)
    up = UP.Upscaler(state_dict=sd, image_hw=(h, w))
    assert up.graph.num_blocks == nb and up.graph.batch == 1
    got = up.upscale(img.cuda())
    g = graph(nb, b, h, w)
    g.img.copy_(img)
    g.execute()
    want = ops.image_to_u8(g.out, UP.U8_A, UP.U8_B, UP.U8_MODE)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (b, 4 * h, 4 * w, 3) and torch.equal(got, want)
    assert torch.equal(up.upscale_float(img.cuda()).view(torch.int16), g.out.view(torch.int16))


def test_container_path(tmp_path):
    from sdod.amd import upscale as UP, weights as Wt
    nb, b, h, w = R.CASES[0]
    img, sd, y, u8 = reference(nb, b, h, w)
    path = str(tmp_path / 'upscaler.sdodw')
    Wt.save(path, {k: v.half() for k, v in sd.items()})
    a = UP.Upscaler(path=path, image_hw=(h, w)).upscale(img.cuda())
    bb = UP.Upscaler(state_dict={k: v.half() for k, v in sd.items()}, image_hw=(h, w)).upscale(img.cuda())
    assert torch.equal(a, bb)


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope='module')
def rig():
    mp = pytest.MonkeyPatch()
    mp.setenv('SDOD_AUTOTUNE', '0')
    try:
        yield _rig()
    finally:
        mp.undo()


def _rig():
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(8, 8)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    sds['upscaler'] = R.synthetic(2)
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=(8, 8), with_text_encoder=False)
    g = torch.Generator().manual_seed(77)
    ctx2 = (torch.randn(2, 77, 768, generator=g) * 0.5).half()
    x_T = torch.randn(1, 4, 8, 8, generator=g)
    x_T2 = torch.randn(1, 4, 8, 8, generator=g)
    return dict(pipe=Txt2Img(upscaler=True, **kw), plain=Txt2Img(**kw), ctx2=ctx2, x_T=x_T, x_T2=x_T2, sds=sds)


def test_pipeline_entry_points_agree(rig):
    pipe, ctx2 = rig['pipe'], rig['ctx2']
    kw = dict(steps=4, guidance=5.0, sampler='plms')
    small = pipe.generate_graphed(ctx2, rig['x_T'], **kw).clone()
    assert tuple(small.shape) == (1, 64, 64, 3)
    a = pipe.upscale(small).clone()
    b = pipe.generate_upscaled(ctx2, rig['x_T'], **kw).clone()
    c = pipe.generate_upscaled_graphed(ctx2, rig['x_T'], **kw).clone()
    assert a.dtype == torch.uint8 and tuple(a.shape) == (1, 256, 256, 3)
    assert torch.equal(a, b) and torch.equal(b, c)
    assert float(a.float().std()) > 1.0
    # a second replay, other noise: equals its eager twin, differs from the first
    c2 = pipe.generate_upscaled_graphed(ctx2, rig['x_T2'], **kw).clone()
    b2 = pipe.generate_upscaled(ctx2, rig['x_T2'], **kw)
    assert torch.equal(c2, b2) and not torch.equal(c2, c)
    # the stand-alone restatement sees the same image
    _, want = R.upscale(rig['sds']['upscaler'], small.cpu())
    assert int((a.cpu().int() - want.int()).abs().max()) <= 1


def test_pipeline_without_upscaler_is_the_parent_pipeline(rig):
    pipe, plain = rig['pipe'], rig['plain']
    assert plain.upscaler is None and pipe.upscaler is not None and pipe.upscaler.image_hw == (64, 64)
    with pytest.raises(ValueError, match='upscaler=True'):
        plain.upscale(torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
    for p in (plain, pipe):
        u, v = p.unet.stats(), p.vae.stats()
        print(f'UNet b2 8x8: {u["launches"]} launches, arena {u["arena_bytes"]} B; VAE 8x8: {v["launches"]} launches, arena {v["arena_bytes"]} B')
        assert (u['launches'], u['arena_bytes']) == PARENT_UNET
        assert (v['launches'], v['arena_bytes']) == PARENT_VAE
    st = pipe.upscaler.graph.stats()
    assert st['launches'] == 15 * 2 + 6 and st['arena_bytes'] > 0


def test_refused_combinations(rig):
    from sdod.amd.pipeline import Txt2Img
    with pytest.raises(ValueError, match='tiling'):
        Txt2Img(state_dicts=rig['sds'], latent_hw=(8, 8), with_text_encoder=False, upscaler=True, tiling=True)
    with pytest.raises(ValueError, match='upscaler'):
        Txt2Img(state_dicts={k: v for k, v in rig['sds'].items() if k != 'upscaler'}, latent_hw=(8, 8), with_text_encoder=False, upscaler=True)
