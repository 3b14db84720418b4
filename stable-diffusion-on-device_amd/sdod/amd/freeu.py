"""FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024): the host side of Txt2Img(..., freeu=True).

At the decoder sites where the backbone h and the popped skip tensor have the same width -- both 4 MC (stage 1) or both 2 MC (stage 2);
output_blocks 0 .. 4 and 7 of the SD 1.x / 2.x UNet -- the method multiplies channels [0, C / 2) of h by a factor made from b and
damps the lowest spatial frequencies of the skip tensor by s.  The engine does it in two launches per site (sdod_freeu_f16) that read
their four numbers and the version from one input of the UNet graph, `unet.freeu` = (b1, s1, b2, s2, version, 0, 0, 0): nothing here
touches the hot path, this module validates arguments and writes that block.

Presets: the values of the FreeU authors' README, keyed (version, model).  They were written down from memory, without the README at
hand to check them against: treat them as starting points, not as a citation.
"""
import math

import torch

# (b1, b2, s1, s2), the argument order of the published `register_free_upblock2d(pipe, b1, b2, s1, s2)` and of set_freeu()
PRESETS = {
    (2, 'sd14'): (1.3, 1.4, 0.9, 0.2),
    (2, 'sd21'): (1.4, 1.6, 0.9, 0.2),
    (1, 'sd14'): (1.2, 1.4, 0.9, 0.2),
    (1, 'sd21'): (1.1, 1.2, 0.9, 0.2),
}
IDENTITY = (1.0, 1.0, 1.0, 1.0, 2.0, 0.0, 0.0, 0.0)   # the block after finalize and after clear_freeu(): (b1, s1, b2, s2, version, ...)
MAX_VALUE = 10.0


def preset(version=2, model='sd14'):
    """(b1, b2, s1, s2) of the authors' README for `version` (1 or 2) and `model` ('sd14' covers SD 1.x, 'sd21' SD 2.x)"""
    try:
        return PRESETS[(version, model)]
    except KeyError:
        raise ValueError(f"no FreeU preset for version {version!r}, model {model!r} (versions 1 and 2, models 'sd14' and 'sd21')") from None


def freeu_check_build(freeu):
    """Txt2Img's `freeu` before any device work: False / None -> False, True -> True, anything else a ValueError.  The switch adds two
    launches per decoder site and one input to whichever UNet graph the other arguments select, so no combination is refused here."""
    if freeu is None or freeu is False:
        return False
    if freeu is True:
        return True
    raise ValueError(f'freeu must be True or False, got {freeu!r} (the values go to set_freeu)')


def freeu_check_args(b1, b2, s1, s2, version=2):
    """set_freeu's arguments: four finite numbers in [0, 10] and version 1 or 2, else ValueError.  Returns the parameter block as the
    graph holds it, a tuple of 8 floats (b1, s1, b2, s2, version, 0, 0, 0)."""
    if isinstance(version, bool) or version not in (1, 2):
        raise ValueError(f'freeu: version must be 1 or 2, got {version!r}')
    vals = []
    for name, v in (('b1', b1), ('s1', s1), ('b2', b2), ('s2', s2)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) and not (torch.is_tensor(v) and v.numel() == 1):
            raise ValueError(f'freeu: {name} must be a number, got {v!r}')
        v = float(v)
        if not math.isfinite(v) or not 0.0 <= v <= MAX_VALUE:
            raise ValueError(f'freeu: {name} must be a finite number in [0, {MAX_VALUE:g}], got {v!r}')
        vals.append(v)
    return (*vals, float(version), 0.0, 0.0, 0.0)


def require(pipe):
    if not getattr(pipe, 'freeu', False):
        raise RuntimeError('this pipeline was built without freeu=True: Txt2Img(..., freeu=True) is needed for FreeU')

