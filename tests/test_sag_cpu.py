"""Self-Attention Guidance's host side without a GPU: the blur taps and the build-time exclusions."""
import math

import pytest
import torch


def test_taps_are_diffusers_gaussian():
    """diffusers' gaussian_blur_2d(kernel_size=9, sigma=1.0): pdf = exp(-0.5 * (x / sigma) ** 2) on linspace(-4, 4, 9), normalised"""
    from sdod.amd import ops
    taps = ops.sag_taps()
    x = torch.linspace(-4, 4, steps=9, dtype=torch.float64)
    pdf = torch.exp(-0.5 * (x / 1.0).pow(2))
    assert len(taps) == 9 and math.isclose(math.fsum(taps), 1.0, rel_tol=0, abs_tol=1e-15)
    assert torch.allclose(torch.tensor(taps, dtype=torch.float64), pdf / pdf.sum(), rtol=1e-14, atol=0)
    assert [float(v) for v in ops._SAG_TAPS] == [float(torch.tensor(v, dtype=torch.float32)) for v in taps]


EXCLUDED = [dict(cfg_split=True), dict(unguided=True), dict(inpaint_unet=True), dict(hires_hw=(16, 16)), dict(canvas_hw=(8, 16)), dict(loras=True),
            dict(controlnet=True), dict(adapter=True), dict(regions=2), dict(ip_adapter=True), dict(tiling='x'), dict(model='sd21'),
            dict(weight_quant=True)]


@pytest.mark.parametrize('kw', EXCLUDED, ids=lambda kw: next(iter(kw)))
def test_build_exclusions(kw):
    """sag_check_build refuses each argument the second UNet graph does not follow, naming it, and Txt2Img does so before any device work"""
    from sdod.amd import sag as SG
    from sdod.amd.pipeline import Txt2Img
    name = next(iter(kw))
    word = {'weight_quant': 'uint8', 'model': 'sd21'}.get(name, name)
    with pytest.raises(ValueError, match=word):
        SG.sag_check_build(True, **kw)
    assert SG.sag_check_build(False, **kw) is False and SG.sag_check_build(True) is True
    with pytest.raises(ValueError, match='sag'):
        Txt2Img(state_dicts={}, sag=True, device='cpu', **kw)


def test_switch_and_scale_arguments():
    from sdod.amd import sag as SG
    from sdod.amd.pipeline import Txt2Img
    for bad in (1, 'on', 0.75):
        pytest.raises(ValueError, SG.sag_check_build, bad)
    for bad in (float('nan'), -0.1, 11, True, '1'):
        pytest.raises(ValueError, SG.sag_check_args, bad)
    assert SG.sag_check_args(0) == 0.0 and SG.sag_check_args(0.75) == 0.75
    plain = Txt2Img.__new__(Txt2Img)
    pytest.raises(RuntimeError, plain.set_sag)
    pytest.raises(RuntimeError, plain.clear_sag)
