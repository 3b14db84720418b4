"""Reference-only control (the reference_only preprocessor of A1111's ControlNet extension; diffusers' StableDiffusionReferencePipeline
with reference_attn=True; ComfyUI's ReferenceOnly node): the host side of Txt2Img(..., reference=True).

A reference picture, noised to the current step, rides through the UNet as the last two rows of a second graph of 2 n + 2 rows
(E.UNet(cfg, 2 n + 2, reference=2): [uncond x n ; cond x n ; ref_u ; ref_c]) whose every attn1 is the shared-key attention launch.
Nothing here touches the hot path: this module validates arguments.
"""
import math

NOISE_FAMILY = 1 << 20   # the Philox stream family of e_ref: (NOISE_FAMILY << 32) | 0 of set_reference's seed.  Families 0 (initial
#                          latents), 1 and 2 (the encoder's two draws) and 3 + step (step noise) are the ones in use (pipeline._replay)


def reference_check_build(reference, with_vae_encoder=False, sag=False, hypertile=None, cfg_split=False, unguided=False, inpaint_unet=False,
                          hires_hw=None, canvas_hw=None, controlnet=False, adapter=False, regions=False, ip_adapter=False, freeu=False,
                          loras=False, tiling=False, model='sd14', weight_quant=False):
    """Txt2Img's `reference` before any device work: False / None -> False, True -> True unless an argument the second UNet graph does
    not follow is set, anything else a ValueError.  freeu and loras write the pair graph alone and tiling excludes the VAE encoder, so
    they are refused too."""
    if reference is None or reference is False:
        return False
    if reference is not True:
        raise ValueError(f'reference must be True or False, got {reference!r} (the picture goes to set_reference)')
    given = dict(sag=sag, hypertile=hypertile is not None, cfg_split=cfg_split, unguided=unguided, inpaint_unet=inpaint_unet,
                 hires_hw=hires_hw is not None, canvas_hw=canvas_hw is not None, controlnet=controlnet, adapter=adapter, regions=regions,
                 ip_adapter=ip_adapter, freeu=freeu, loras=loras, tiling=tiling)
    bad = [name for name, v in given.items() if v]
    if model == 'sd21':
        bad.append("model='sd21' (v-prediction)")
    if weight_quant:
        bad.append('uint8 weights')
    if bad:
        raise ValueError(f'reference=True (reference-only control) cannot be combined with {", ".join(bad)}')
    if not with_vae_encoder:
        raise ValueError('reference=True needs with_vae_encoder=True: set_reference encodes the picture')
    return True


def reference_check_args(image_u8, fidelity, noise, latent_shape):
    """set_reference's arguments: one uint8 picture [1, 8 H, 8 W, 3] (or [8 H, 8 W, 3]), fidelity a finite number in [0, 1], noise None
    or fp32 [1, 4, H, W] / [4, H, W]; returns (image [1, 8 H, 8 W, 3], fidelity, noise [1, 4, H, W] or None).  ValueError otherwise."""
    import torch
    c, h, w = latent_shape
    if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8 or tuple(image_u8.shape[-3:]) != (8 * h, 8 * w, 3) \
            or image_u8.numel() != 8 * h * 8 * w * 3:
        raise ValueError(f'reference: image_u8 must be one uint8 picture [{8 * h}, {8 * w}, 3], got '
                         f'{tuple(image_u8.shape) if isinstance(image_u8, torch.Tensor) else image_u8!r}')
    if isinstance(fidelity, bool) or not isinstance(fidelity, (int, float)) or not math.isfinite(fidelity) or not 0.0 <= fidelity <= 1.0:
        raise ValueError(f'reference: fidelity must be a finite number in [0, 1], got {fidelity!r}')
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or noise.numel() != c * h * w or tuple(noise.shape[-3:]) != (c, h, w):
            raise ValueError(f'reference: noise must be fp32 [{c}, {h}, {w}], got {tuple(noise.shape) if isinstance(noise, torch.Tensor) else noise!r}')
        noise = noise.reshape(1, c, h, w)
    return image_u8.reshape(1, 8 * h, 8 * w, 3), float(fidelity), noise


def require(pipe):
    if getattr(pipe, 'ref_unet', None) is None:
        raise RuntimeError('this pipeline was built without reference=True: Txt2Img(..., reference=True, with_vae_encoder=True) is needed')
