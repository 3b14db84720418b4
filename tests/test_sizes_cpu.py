"""The size rule of the pipeline (check_latent_hw) and the argument contract of the hires pass (hires_check_args), on the host:
none of these needs a device."""
import pytest
import torch


def _pipe(latent=(8, 16), hires=(16, 24), model='sd14'):
    """a pipeline without its constructor (no device, no graphs), as the other argument-check tests build it"""
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    pipe.cfg = E.sd14_config(*latent)
    pipe.n = 1
    pipe.model = model
    if hires is not None:
        pipe.hires = Txt2Img.__new__(Txt2Img)
        pipe.hires.cfg = E.sd14_config(*hires)
        pipe.hires.n = 1
    return pipe


def test_check_latent_hw():
    from sdod.amd.pipeline import check_latent_hw
    assert check_latent_hw(16) == (16, 16)
    assert check_latent_hw((16, 24)) == (16, 24)
    assert check_latent_hw((8, 16)) == (8, 16)
    assert check_latent_hw([24, 8]) == (24, 8)
    for bad in ((16, 20), (0, 8), (16,), 12, (16, 24, 8), -8, 16.0, (16, 24.0), None, True, '16'):
        with pytest.raises(ValueError):
            check_latent_hw(bad)


def test_constructor_refuses_sizes_before_any_device_work():
    """ValueError from the first lines of the constructor: no device is selected, nothing is built"""
    from sdod.amd.pipeline import Txt2Img
    for kw in (dict(latent_hw=(16, 20)), dict(latent_hw=12), dict(latent_hw=(16,)), dict(latent_hw=16, hires_hw=(16, 20)),
               dict(latent_hw=16, hires_hw=4), dict(latent_hw=16, hires_hw=(24, 24), cfg_split=True),
               dict(latent_hw=16, hires_hw=(24, 24), inpaint_unet=True)):
        with pytest.raises(ValueError):
            Txt2Img(state_dicts={}, device='cuda:7', **kw)


def test_hires_check_args():
    from sdod.amd.pipeline import hires_check_args
    pipe = _pipe()
    hn = torch.zeros(1, 4, 16, 24)
    assert hires_check_args(pipe, 1, 'dpmpp_2m', 20, 0.5, 'bilinear', 'karras', 1.0, None, None) == 10
    assert hires_check_args(pipe, 1, 'plms', 20, 0.7, 'bicubic', 'discrete', 1.0, hn, None) == 14
    assert hires_check_args(pipe, 1, 'euler_a', 20, 0.5, 'nearest-exact', 'karras', 1.0, hn, torch.zeros(9, 1, 4, 16, 24)) == 10
    bad = [
        dict(upscaler='lanczos'), dict(upscaler='nearest'), dict(upscaler=None),
        dict(denoise=0.0), dict(denoise=1.0), dict(denoise=1.5), dict(denoise=-0.1), dict(denoise=0.04),     # t_enc 0 / steps / outside
        dict(hires_steps=0), dict(hires_steps=1),
        dict(sampler='heun'), dict(schedule='cosine'), dict(eta=-1.0),
        dict(hires_noise=torch.zeros(1, 4, 8, 16)), dict(hires_noise=torch.zeros(1, 4, 24, 16)), dict(hires_noise=torch.zeros(2, 4, 16, 24)),
        dict(hires_noise=torch.zeros(1, 4, 16, 24, dtype=torch.float64)), dict(hires_noise=[0.0]),
        dict(hires_step_noise=torch.zeros(9, 1, 4, 16, 24)),                                                  # dpmpp_2m draws none
        dict(sampler='euler_a', hires_step_noise=torch.zeros(10, 1, 4, 16, 24)),                              # t_enc - 1 = 9 rows
        dict(sampler='euler_a', hires_step_noise=torch.zeros(9, 1, 4, 8, 16)),
        dict(sampler='euler_a', hires_step_noise=torch.zeros(9, 1, 4, 16, 24, dtype=torch.float16)),
        dict(sampler='plms', hires_step_noise=torch.zeros(9, 1, 4, 16, 24)),
    ]
    for kw in bad:
        a = dict(sampler='dpmpp_2m', hires_steps=20, denoise=0.5, upscaler='bilinear', schedule='karras', eta=1.0, hires_noise=None,
                 hires_step_noise=None)
        a.update(kw)
        with pytest.raises(ValueError):
            hires_check_args(pipe, 1, **a)
    with pytest.raises(ValueError, match='hires_hw'):
        hires_check_args(_pipe(hires=None), 1, 'dpmpp_2m', 20, 0.5, 'bilinear', 'karras', 1.0, None, None)
    with pytest.raises(ValueError, match='v-conversion'):                                                     # DDIM img2img has none
        hires_check_args(_pipe(model='sd21'), 1, 'plms', 20, 0.5, 'bilinear', 'discrete', 1.0, None, None)
    assert hires_check_args(_pipe(model='sd21'), 1, 'euler', 20, 0.5, 'bilinear', 'karras', 1.0, None, None) == 10


def test_hires_entry_points_refuse_before_any_device_work():
    x_T = torch.zeros(1, 4, 8, 16)
    pipe = _pipe()
    for fn in (pipe.generate_hires, pipe.generate_hires_graphed):
        with pytest.raises(ValueError):
            fn(None, x_T, upscaler='lanczos')
        with pytest.raises(ValueError):
            fn(None, x_T, denoise=0.0)
        with pytest.raises(ValueError):
            fn(None, x_T, sampler='heun')
        with pytest.raises(ValueError):
            fn(None, x_T, hires_noise=torch.zeros(1, 4, 8, 16))
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'euler_a', step_noise=torch.zeros(3, 1, 4, 8, 16))
        with pytest.raises(ValueError):
            fn(None, x_T, 20, 7.5, 'euler_a', hires_step_noise=torch.zeros(3, 1, 4, 16, 24))
        with pytest.raises(TypeError):
            fn(None, x_T, 20, 7.5, 'euler', 20)                                          # hires_steps .. are keyword-only
    with pytest.raises(ValueError):
        pipe.hires_from_latent(None, torch.zeros(1, 4, 16, 24), hires_steps=20, hires_seed=1)                       # z_lo has the base size
    with pytest.raises(ValueError):
        pipe.hires_from_latent(None, x_T, hires_steps=20, hires_seed=1, upscaler='area')
    with pytest.raises(TypeError):
        pipe.hires_from_latent(None, x_T)                                                # hires_steps and hires_seed are generate_hires' to default
    bare = _pipe(hires=None)
    for fn in (bare.generate_hires, bare.generate_hires_graphed):
        with pytest.raises(ValueError, match='hires_hw'):
            fn(None, x_T)
    with pytest.raises(ValueError, match='hires_hw'):
        bare.hires_from_latent(None, x_T, hires_steps=20, hires_seed=1)


def test_rectangular_argument_checks_compare_against_the_rectangle():
    """the image / mask / noise checks of the existing entry points at (16, 24): the rectangle passes them, a square does not"""
    from sdod.amd.pipeline import inpaint_check_args, inpaint_concat_check_args, k_check_args
    lat = (4, 16, 24)
    img, mask = torch.zeros(1, 128, 192, 3, dtype=torch.uint8), torch.zeros(1, 128, 192, dtype=torch.uint8)
    assert inpaint_check_args(img, mask, 0.5, 20, None, lat, 1)[1] == 10
    inpaint_check_args(img, mask, 0.5, 20, torch.zeros(9, 1, 4, 16, 24), lat, 1)
    inpaint_concat_check_args(img, mask, torch.zeros(1, 4, 16, 24), 20, 'plms', None, lat, 1)
    k_check_args('euler_a', 20, 'karras', 1.0, torch.zeros(19, 1, 4, 16, 24), lat, 1)
    with pytest.raises(ValueError):
        inpaint_check_args(img, torch.zeros(1, 128, 128, dtype=torch.uint8), 0.5, 20, None, lat, 1)
    with pytest.raises(ValueError):
        inpaint_check_args(torch.zeros(1, 192, 128, 3, dtype=torch.uint8), torch.zeros(1, 192, 128, dtype=torch.uint8), 0.5, 20, None, lat, 1)
    with pytest.raises(ValueError):
        inpaint_concat_check_args(img, mask, torch.zeros(1, 4, 24, 16), 20, 'plms', None, lat, 1)
    with pytest.raises(ValueError):
        k_check_args('euler_a', 20, 'karras', 1.0, torch.zeros(19, 1, 4, 24, 16), lat, 1)


def test_unet_graph_refuses_sizes_the_levels_cannot_divide():
    """sdod_graph_create: INVALID_ARGUMENT with a message for a UNET graph whose latent is no multiple of 8; the VAE graphs keep
    accepting what they accept (their construction declares parameters only)"""
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    for hw in ((16, 20), (12, 16), (4, 8), (0, 8)):
        with pytest.raises(SdodError, match='multiples of 8') as e:
            E.UNet(E.sd14_config(*hw), 2)
        assert e.value.code == 2
    assert E.UNet(E.sd14_config(8, 16), 2).param_table() == E.UNet(E.sd14_config(16, 16), 2).param_table()
    assert E.VaeDecoder(E.sd14_config(12, 20), 1).param_table() == E.VaeDecoder(E.sd14_config(16, 16), 1).param_table()
