"""MultiDiffusion panoramas on the host (numpy; no device): the window grid of a latent canvas, the per-window-pixel weights, their sum
per canvas pixel, and the argument contracts of Txt2Img(canvas_hw=...) and its panorama entry points.

MultiDiffusion (Bar-Tal et al. 2023; diffusers' StableDiffusionPanoramaPipeline, A1111's Tiled Diffusion) keeps the UNet at its native
size: it evaluates overlapping windows of a large canvas and fuses their predictions at every step.  Here the fused quantity is the
guided model output -- CFG and the three k-samplers are linear in it -- so one sampler step runs on the canvas, in one launch
(include/sdod_hip.h: sdod_k_step_windows), with one history and one noise stream."""
import numpy as np

from ._lib import PANO_MAX_AXIS
from .samplers import K_SAMPLERS

WEIGHT_KINDS = ('uniform', 'gaussian')


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _pair(v, name):
    hw = (v, v) if _is_int(v) else v
    if not isinstance(hw, (tuple, list)) or len(hw) != 2 or not all(_is_int(s) for s in hw):
        raise ValueError(f'{name} must be an integer or a pair of integers, got {v!r}')
    return int(hw[0]), int(hw[1])


def _axis_origins(size, window, stride, wrap, axis):
    if window < 8 or window % 8 or size < 8 or size % 8:
        raise ValueError(f'{axis}: canvas and window sides must be multiples of 8, at least 8, got canvas {size}, window {window}')
    if window > size:
        raise ValueError(f'{axis}: the window ({window}) is larger than the canvas ({size})')
    if stride < 8 or stride % 8 or stride > window:
        raise ValueError(f'{axis}: stride must be a multiple of 8 in [8, {window}] (the window side), got {stride}')
    if wrap:
        if size % stride:
            raise ValueError(f'{axis}: a wrapped canvas side ({size}) must be a multiple of the stride ({stride})')
        origins = list(range(0, size, stride))
    elif size == window:
        origins = [0]
    else:
        origins = list(range(0, size - window + 1, stride))
        if origins[-1] + window < size:          # the last window does not reach the border: one more, flush with it
            origins.append(size - window)
    if len(origins) > PANO_MAX_AXIS:
        raise ValueError(f'{axis}: {len(origins)} windows on one axis, at most {PANO_MAX_AXIS} (a larger stride has fewer)')
    return origins


def plan_windows(canvas_hw, window_hw, stride, wrap_x=False):
    """The window grid of a canvas: (oy, ox), the windows' origins per axis as lists of ints; window iy * len(ox) + ix covers rows
    oy[iy] .. + wh and columns ox[ix] .. + ww (modulo W with wrap_x).  Origins are 0, s, 2 s, ... while the window fits, plus -- where
    the last one does not reach the border -- one at size - window, as the front ends place it; an axis where the canvas equals the
    window has the single origin 0.  With wrap_x the x origins are 0, s, ... < W and W must be a multiple of the stride, so every
    column has the same cover count.  stride: an int or (sy, sx), each a multiple of 8 in [8, window side]; canvas and window sides
    multiples of 8.  More than PANO_MAX_AXIS origins on an axis, or anything else outside this contract: ValueError."""
    H, W = _pair(canvas_hw, 'canvas_hw')
    wh, ww = _pair(window_hw, 'window_hw')
    sy, sx = _pair(stride, 'stride')
    return _axis_origins(H, wh, sy, False, 'y'), _axis_origins(W, ww, sx, bool(wrap_x), 'x')


def window_weights(window_hw, kind='uniform'):
    """float32 [wh, ww], the weight of a window pixel's prediction.  'uniform': ones (MultiDiffusion).  'gaussian': the outer product of
    exp(-(i - (L - 1) / 2)^2 / L^2 / (2 * 0.01)) / sqrt(2 pi * 0.01) per axis of length L (Mixture of Diffusers' tile weights, as A1111's
    Tiled Diffusion uses them), computed in float64 and rounded once."""
    wh, ww = _pair(window_hw, 'window_hw')
    if kind not in WEIGHT_KINDS:
        raise ValueError(f'weights must be one of {WEIGHT_KINDS}, got {kind!r}')
    if kind == 'uniform':
        return np.ones((wh, ww), dtype=np.float32)
    var = 0.01

    def axis(L):
        i = np.arange(L, dtype=np.float64)
        return np.exp(-(i - (L - 1) / 2.0) ** 2 / float(L * L) / (2.0 * var)) / np.sqrt(2.0 * np.pi * var)
    return np.outer(axis(wh), axis(ww)).astype(np.float32)


def window_columns(ox, ww, W, wrap_x):
    """the canvas columns of a window at x origin ox, in window order (modulo W with wrap_x)"""
    cols = np.arange(ox, ox + ww)
    return cols % W if wrap_x else cols


def weight_sum(canvas_hw, window_hw, oy, ox, wgt, wrap_x=False):
    """float32 [H, W]: per canvas pixel the sum of wgt over the windows that cover it, accumulated in float32 in ascending window order
    -- the kernel's order, so a pixel under one window of weight v has v exactly and uniform weights give the exact cover count."""
    H, W = _pair(canvas_hw, 'canvas_hw')
    wh, ww = _pair(window_hw, 'window_hw')
    wgt = np.asarray(wgt, dtype=np.float32).reshape(wh, ww)
    out = np.zeros((H, W), dtype=np.float32)
    for y0 in oy:
        for x0 in ox:
            out[np.ix_(np.arange(y0, y0 + wh), window_columns(x0, ww, W, wrap_x))] += wgt
    return out


def panorama_check_build(canvas_hw, canvas_wrap, latent_hw, cfg_split=False, inpaint_unet=False, hires_hw=None, adapter=False,
                         controlnet=False, regions=False, ip_adapter=False, tiling=False, upscaler=False):
    """Txt2Img's canvas_hw: None (off; canvas_wrap must be off too), or an integer or (H, W) by check_latent_hw's rule -- multiples of 8,
    at least 8 -- with each side at least the window's (latent_hw), and none of the options whose state is sized by one UNet
    evaluation.  Returns (H, W) or None; raises ValueError.  Needs no device."""
    if canvas_hw is None:
        if canvas_wrap:
            raise ValueError('canvas_wrap needs canvas_hw')
        return None
    H, W = _pair(canvas_hw, 'canvas_hw')
    wh, ww = _pair(latent_hw, 'latent_hw')
    if any(v < 8 or v % 8 for v in (H, W)):
        raise ValueError(f'canvas_hw: height and width must be multiples of 8, at least 8 (64 px of image), got {canvas_hw!r}')
    if H < wh or W < ww:
        raise ValueError(f'canvas_hw {(H, W)} must be at least the window latent_hw {(wh, ww)} on each side')
    if not isinstance(canvas_wrap, (bool, np.bool_)):
        raise ValueError(f'canvas_wrap must be True or False, got {canvas_wrap!r}')
    for name, on, why in (
            ('cfg_split', cfg_split, 'the canvas step would have to run behind an exchange per chunk'),
            ('inpaint_unet', inpaint_unet, 'the conditioning channels would need a canvas-sized mask and masked latent'),
            ('hires_hw', hires_hw is not None, 'the second pass is a second place for the canvas state'),
            ('adapter', adapter, 'the adapter features would need a canvas-sized hint cut per window'),
            ('controlnet', controlnet, 'the control residuals would need a canvas-sized hint cut per window'),
            ('regions', regions, 'the region masks would need to be canvas-sized and cut per window'),
            ('ip_adapter', ip_adapter, 'the image-prompt mask would need to be canvas-sized and cut per window'),
            ('tiling', tiling not in (False, None, 0), 'a window is a crop of the canvas, its border must stay plain; canvas_wrap=True wraps the canvas'),
            ('upscaler', upscaler, 'the upscaler is built for the size of one UNet evaluation, not for the canvas')):
        if on:
            raise ValueError(f'canvas_hw cannot be combined with {name}: {why}')
    return H, W


def panorama_check_args(canvas_hw, window_hw, canvas_wrap, n, x_T, sampler, stride, weights):
    """the argument contract of Txt2Img.sample_panorama / generate_panorama / generate_panorama_graphed beyond k_check_args', checked on
    the host before any device work: a pipeline built with canvas_hw; a k-sampler ('plms' and 'dpm' keep histories of their own per
    evaluation and are refused); x_T fp32 [1, 4, H, W]; stride None (half the window, rounded down to a multiple of 8, at least 8) or
    plan_windows' rule; weights one of WEIGHT_KINDS.  Returns (oy, ox, chunks); raises ValueError."""
    if canvas_hw is None:
        raise ValueError('this pipeline was built without canvas_hw: Txt2Img(..., canvas_hw=(H, W)) is needed for panoramas')
    if sampler not in K_SAMPLERS:
        raise ValueError(f"sampler must be one of {K_SAMPLERS} (the window average needs a step that is linear in the model output with "
                         f"one history for the canvas; 'plms' and 'dpm' are not offered), got {sampler!r}")
    if weights not in WEIGHT_KINDS:
        raise ValueError(f'weights must be one of {WEIGHT_KINDS}, got {weights!r}')
    shape = tuple(getattr(x_T, 'shape', ()))
    if shape != (1, 4) + tuple(canvas_hw) or 'float32' not in str(getattr(x_T, 'dtype', '')):
        raise ValueError(f'x_T must be a float32 tensor {(1, 4) + tuple(canvas_hw)} (one canvas), got {shape} {getattr(x_T, "dtype", type(x_T))}')
    if stride is None:
        stride = tuple(max(8, (s // 2) // 8 * 8) for s in window_hw)
        if canvas_wrap and canvas_hw[1] % stride[1]:
            raise ValueError(f'the default x stride {stride[1]} does not divide the wrapped canvas width {canvas_hw[1]}: pass stride')
    oy, ox = plan_windows(canvas_hw, window_hw, stride, canvas_wrap)
    return oy, ox, -(-len(oy) * len(ox) // int(n))
