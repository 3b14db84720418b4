"""Self-Attention Guidance (Hong et al., "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance", ICCV 2023;
DESIGN.md 6s): the host side of Txt2Img(..., sag=True).

Per UNet evaluation the pair graph (built with the switch) also gives the attention mass of middle_block.1's attn1; behind it the
pipeline runs ops.sag_degrade (blur the x0 prediction where the mass is above 1, renoise), a second UNet graph of one row per image on
the degraded latent under the uncond context, and ops.sag_fold, which puts s * (e_u - e_d) into the cond rows so that every step kernel
produces e_u + g (e_c - e_u) + s (e_u - e_d) unchanged.  Nothing here touches the hot path: this module validates arguments.
"""
import math

DEFAULT_SCALE = 0.75
MAX_SCALE = 10.0


def sag_check_build(sag, cfg_split=False, unguided=False, inpaint_unet=False, hires_hw=None, canvas_hw=None, loras=False, controlnet=False,
                    adapter=False, regions=False, ip_adapter=False, tiling=False, model='sd14', weight_quant=False, reference=False):
    """Txt2Img's `sag` before any device work: False / None -> False, True -> True unless one of the arguments the second UNet graph
    does not follow yet is set, anything else a ValueError.  freeu and hypertile compose: the second graph is built with the same
    switches and set_freeu() writes both."""
    if sag is None or sag is False:
        return False
    if sag is not True:
        raise ValueError(f'sag must be True or False, got {sag!r} (the scale goes to set_sag)')
    given = dict(cfg_split=cfg_split, unguided=unguided, inpaint_unet=inpaint_unet, hires_hw=hires_hw is not None, canvas_hw=canvas_hw is not None,
                 loras=loras, controlnet=controlnet, adapter=adapter, regions=regions, ip_adapter=ip_adapter, tiling=tiling,
                 reference=reference)   # (the engine refuses the two switches on one graph: sdod_graph_enable_reference)
    bad = [name for name, v in given.items() if v]
    if model == 'sd21':
        bad.append("model='sd21' (v-prediction)")
    if weight_quant:
        bad.append('uint8 weights')
    if bad:
        raise ValueError(f'sag=True (Self-Attention Guidance) cannot be combined with {", ".join(bad)}')
    return True


def sag_check_args(scale):
    """set_sag's scale: a finite number in [0, 10], else ValueError"""
    if isinstance(scale, bool) or not isinstance(scale, (int, float)):
        raise ValueError(f'sag: scale must be a number, got {scale!r}')
    scale = float(scale)
    if not math.isfinite(scale) or not 0.0 <= scale <= MAX_SCALE:
        raise ValueError(f'sag: scale must be a finite number in [0, {MAX_SCALE:g}], got {scale!r}')
    return scale


def require(pipe):
    if getattr(pipe, 'sag_unet', None) is None:
        raise RuntimeError('this pipeline was built without sag=True: Txt2Img(..., sag=True) is needed for Self-Attention Guidance')
