"""Regional prompts, the host side: masks for the common splits and the argument checks of Txt2Img(regions=k).

A region is a uint8 mask at image resolution, [8h, 8w] for an h x w latent, 255 = fully inside; k of them, [k, 8h, 8w], say where each
of k prompts applies.  Masks may be soft and may overlap: per UNet level the engine turns them into weights that sum to 1 at every
pixel (ops.region_weights), and a pixel no mask covers belongs to region 0, the background.  A base prompt at ratio b needs no more
than that: give region 0 a constant mask of b / (1 - b) times the other regions' value.

Everything here is numpy / torch on the CPU; nothing touches a device."""
import numpy as np
import torch

MIN_REGIONS, MAX_REGIONS = 2, 4


def _hw(hw):
    h, w = (hw, hw) if isinstance(hw, (int, np.integer)) and not isinstance(hw, bool) else tuple(hw)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 8 and v % 8 == 0 for v in (h, w)):
        raise ValueError(f'hw must be a latent size, multiples of 8 that are at least 8, got {hw!r}')
    return int(h), int(w)


def _cuts(ratios, n):
    """the k + 1 pixel boundaries of `n` pixels split in the proportions `ratios` (each part at least one pixel)"""
    r = np.asarray(ratios, dtype=np.float64).reshape(-1)
    if not MIN_REGIONS <= r.size <= MAX_REGIONS or not np.isfinite(r).all() or (r <= 0).any():
        raise ValueError(f'ratios must be {MIN_REGIONS} to {MAX_REGIONS} positive finite numbers, got {ratios!r}')
    edges = np.rint(np.concatenate([[0.0], np.cumsum(r)]) / r.sum() * n).astype(np.int64)
    if (np.diff(edges) < 1).any():
        raise ValueError(f'ratios {ratios!r} leave a region without a pixel at {n} pixels')
    return edges


def column_masks(ratios, hw):
    """k side-by-side regions, left to right, widths in the proportions `ratios`: uint8 [k, 8h, 8w], 255 inside, 0 outside"""
    h, w = _hw(hw)
    e = _cuts(ratios, 8 * w)
    m = torch.zeros(len(e) - 1, 8 * h, 8 * w, dtype=torch.uint8)
    for r in range(len(e) - 1):
        m[r, :, e[r]:e[r + 1]] = 255
    return m


def row_masks(ratios, hw):
    """k regions stacked top to bottom, heights in the proportions `ratios`: uint8 [k, 8h, 8w]"""
    h, w = _hw(hw)
    e = _cuts(ratios, 8 * h)
    m = torch.zeros(len(e) - 1, 8 * h, 8 * w, dtype=torch.uint8)
    for r in range(len(e) - 1):
        m[r, e[r]:e[r + 1], :] = 255
    return m


def feather(masks, px):
    """soften the borders: every mask is averaged over the (2 px + 1)^2 box around each pixel (the image's edge pixels repeated
    outside it), rounded to the nearest integer.  uint8 [k, H, W] -> uint8 [k, H, W]; px = 0 returns a copy.  Masks that summed to
    255 everywhere still do to within rounding, and the engine normalises anyway."""
    masks = check_masks(masks, None, None)
    if isinstance(px, bool) or not isinstance(px, (int, np.integer)) or px < 0 or px > 256:
        raise ValueError(f'px must be an integer in [0, 256], got {px!r}')
    if px == 0:
        return masks.clone()
    x = masks.to(torch.float64)[:, None]
    x = torch.nn.functional.pad(x, (px, px, px, px), mode='replicate')
    x = torch.nn.functional.avg_pool2d(x, 2 * px + 1, stride=1)
    return torch.clamp(torch.floor(x[:, 0] + 0.5), 0, 255).to(torch.uint8)


def check_masks(masks, k, latent):
    """masks as set_regions takes them: a uint8 torch tensor (or numpy array) [k, 8h, 8w] for `latent` = (h, w); None skips that
    check.  Returns a contiguous CPU/whatever-device torch tensor; raises ValueError."""
    if isinstance(masks, np.ndarray):
        if masks.dtype != np.uint8:
            raise ValueError(f'masks must be uint8, got {masks.dtype}')
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if not torch.is_tensor(masks):
        raise ValueError(f'masks must be a uint8 tensor [regions, 8h, 8w], got {type(masks).__name__}')
    if masks.dtype != torch.uint8:
        raise ValueError(f'masks must be uint8 (255 = inside the region), got {masks.dtype}')
    if masks.dim() != 3:
        raise ValueError(f'masks must be [regions, 8h, 8w], got {tuple(masks.shape)}')
    if k is not None and masks.shape[0] != k:
        raise ValueError(f'this pipeline was built with regions={k}: masks must hold {k} regions, got {masks.shape[0]}')
    if latent is not None and tuple(masks.shape[1:]) != (8 * latent[0], 8 * latent[1]):
        raise ValueError(f'masks must be at image resolution {(8 * latent[0], 8 * latent[1])}, got {tuple(masks.shape[1:])}')
    return masks.contiguous()


def regions_check_build(regions, prompt_chunks=1, cfg_split=False, hires_hw=None, controlnet=False, adapter=False, tiling=False,
                        inpaint_unet=False, model='sd14', weight_quant=None):
    """Txt2Img's `regions` against the rest of its arguments, before any device work: returns 0 (no regions) or k in [2, 4]; raises
    ValueError naming `regions` for a bad value and for every combination the regional UNet does not take."""
    if regions is False or regions is None:
        return 0
    if isinstance(regions, bool) or not isinstance(regions, (int, np.integer)) or not MIN_REGIONS <= regions <= MAX_REGIONS:
        raise ValueError(f'regions must be False or an integer in [{MIN_REGIONS}, {MAX_REGIONS}], got {regions!r}')
    refused = [('prompt_chunks > 1', prompt_chunks != 1), ('cfg_split', bool(cfg_split)), ('hires_hw', hires_hw is not None),
               ('controlnet', bool(controlnet)), ('adapter', bool(adapter)), ('tiling', bool(tiling)), ('inpaint_unet', bool(inpaint_unet)),
               ("model='sd21'", model == 'sd21'), ('uint8 weights (weight_quant)', bool(weight_quant))]
    bad = [name for name, on in refused if on]
    if bad:
        raise ValueError(f'regions cannot be combined with {", ".join(bad)}')
    return int(regions)


def regions_check_args(pipe, masks_u8):
    """set_regions' argument against the pipeline (callable on a Txt2Img.__new__ object that has `regions` and `_latent_shape`):
    returns the masks as a contiguous uint8 tensor; RuntimeError without regions, ValueError for a bad dtype, shape or region count"""
    k = int(getattr(pipe, 'regions', 0) or 0)
    if not k:
        raise RuntimeError('this pipeline was built without regions: Txt2Img(..., regions=k) is needed for regional prompts')
    return check_masks(masks_u8, k, tuple(pipe._latent_shape)[-2:])


def regions_check_prompts(pipe, prompts):
    """encode_regions' prompts: exactly k strings"""
    k = int(getattr(pipe, 'regions', 0) or 0)
    if not k:
        raise RuntimeError('this pipeline was built without regions: Txt2Img(..., regions=k) is needed for regional prompts')
    if isinstance(prompts, str) or not isinstance(prompts, (list, tuple)) or len(prompts) != k or not all(isinstance(p, str) for p in prompts):
        raise ValueError(f'prompts must be a list of exactly {k} strings (this pipeline was built with regions={k})')
    return list(prompts)
