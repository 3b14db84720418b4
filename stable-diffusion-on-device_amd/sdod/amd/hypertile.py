"""HyperTile (tfernd/HyperTile; "Hypertile" in A1111's settings, the HyperTile node in ComfyUI): the host side of
Txt2Img(..., hypertile=T | (T, max_depth)).

The method runs a UNet's self-attention (attn1) inside rectangular tiles of the feature map, which cuts the score work by the number
of tiles; it is an opt-in approximation for large images.  Here it is a switch on the UNet / ControlNet graph
(sdod_graph_enable_hypertile): the tiled levels run sdod_attention_tiled_f16, one launch that walks the tiles in place.  The tile rule
is this project's and deterministic (HyperTile with swap_size = 1 and depth scaling; the random per-call swap is left out because a
captured trajectory needs a fixed grid); its one statement is sdod_hypertile_grid, which grid() wraps."""
import ctypes

from . import _lib

DEFAULT_TILE = 32       # latent pixels (256 image pixels)
DEFAULT_MAX_DEPTH = 0   # only the widest UNet level
MIN_TILE = 8
MAX_DEPTH = 3


def hypertile_check(hypertile):
    """Txt2Img's `hypertile` before any device work: None / False -> None, an int T -> (T, 0), a pair (T, max_depth) -> itself; T an int
    >= 8 (latent pixels), max_depth an int in [0, 3]; anything else a ValueError."""
    if hypertile is None or hypertile is False:
        return None
    pair = hypertile if isinstance(hypertile, (tuple, list)) else (hypertile, DEFAULT_MAX_DEPTH)
    if len(pair) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in pair):
        raise ValueError(f'hypertile must be None, a tile size T or a pair (T, max_depth) of ints, got {hypertile!r}')
    tile, max_depth = pair
    if tile < MIN_TILE:
        raise ValueError(f'hypertile: the tile size must be >= {MIN_TILE} latent pixels, got {tile}')
    if not 0 <= max_depth <= MAX_DEPTH:
        raise ValueError(f'hypertile: max_depth must be in [0, {MAX_DEPTH}], got {max_depth}')
    return (tile, max_depth)


def grid(h, w, tile=DEFAULT_TILE, level=0, max_depth=DEFAULT_MAX_DEPTH):
    """(th, tw): the tile sides at UNet level `level` of an h x w latent, or None where the rule leaves the level untiled
    (sdod_hypertile_grid: the tile count per axis is fixed at level 0 -- h / the smallest divisor of h that is >= min(tile, h) -- and
    kept at every level; untiled beyond max_depth, for a 1 x 1 grid and where the count does not divide the level's side)"""
    th, tw = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.hip().sdod_hypertile_grid(int(h), int(w), int(tile), int(level), int(max_depth), ctypes.byref(th), ctypes.byref(tw)))
    return (th.value, tw.value) if th.value > 0 else None
