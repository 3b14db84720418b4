import pytest  # reference-only control's argument checks that need no GPU
import torch

EXCLUDED = dict(sag=True, hypertile=(8, 0), cfg_split=True, unguided=True, inpaint_unet=True, hires_hw=(24, 24), canvas_hw=(16, 32), controlnet=True,
                adapter=True, regions=2, ip_adapter=True, freeu=True, loras=True, tiling=True, model='sd21', weight_quant=True)


def test_sag_refuses_reference():
    from sdod.amd import sag as SG
    assert SG.sag_check_build(True) is True
    with pytest.raises(ValueError, match='reference'):
        SG.sag_check_build(True, reference=True)


@pytest.mark.parametrize('name', EXCLUDED)
def test_build_exclusions(name):
    from sdod.amd import reference as RF
    from sdod.amd.pipeline import Txt2Img
    assert RF.reference_check_build(True, with_vae_encoder=True) is True and RF.reference_check_build(False, **{name: EXCLUDED[name]}) is False
    with pytest.raises(ValueError, match='uint8' if name == 'weight_quant' else 'sd21' if name == 'model' else name):
        RF.reference_check_build(True, with_vae_encoder=True, **{name: EXCLUDED[name]})
    with pytest.raises(ValueError, match='reference'):            # ... and through the constructor, before any device work
        Txt2Img(state_dicts={}, device='cuda:7', with_vae_encoder=True, reference=True, **{name: EXCLUDED[name]})


def test_reference_needs_the_encoder_and_a_bool():
    from sdod.amd import reference as RF
    with pytest.raises(ValueError, match='with_vae_encoder'):
        RF.reference_check_build(True)
    with pytest.raises(ValueError, match='True or False'):
        RF.reference_check_build(0.5, with_vae_encoder=True)


BAD_ARGS = {'float picture': dict(image=torch.zeros(128, 128, 3)), 'wrong size': dict(image=torch.zeros(64, 128, 3, dtype=torch.uint8)),
            'two pictures': dict(image=torch.zeros(2, 128, 128, 3, dtype=torch.uint8)), 'fidelity above 1': dict(fidelity=1.5),
            'fidelity nan': dict(fidelity=float('nan')), 'fidelity bool': dict(fidelity=True), 'noise shape': dict(noise=torch.zeros(4, 8, 16)),
            'noise dtype': dict(noise=torch.zeros(4, 16, 16, dtype=torch.float16))}


@pytest.mark.parametrize('name', BAD_ARGS)
def test_set_reference_argument_errors(name):
    from sdod.amd import reference as RF
    a = {**dict(image=torch.zeros(128, 128, 3, dtype=torch.uint8), fidelity=0.5, noise=None), **BAD_ARGS[name]}
    img, f, nz = RF.reference_check_args(torch.zeros(1, 128, 128, 3, dtype=torch.uint8), 1, torch.zeros(4, 16, 16), (4, 16, 16))
    assert img.shape == (1, 128, 128, 3) and f == 1.0 and nz.shape == (1, 4, 16, 16)
    with pytest.raises(ValueError, match='reference'):
        RF.reference_check_args(a['image'], a['fidelity'], a['noise'], (4, 16, 16))
