"""ESRGAN x4 upscaling without any Stable Diffusion model (the front ends' "Extras" tab): RRDBNet as the engine's UPSCALER graph
(include/sdod_engine.h), from a state dict or an `upscaler.sdodw` container written by `python -m sdod.amd.convert --upscaler`.

    up = Upscaler(path='models/upscaler.sdodw', image_hw=(512, 512))
    big = up.upscale(img_u8)            # uint8 [n, 512, 512, 3] -> uint8 [n, 2048, 2048, 3]
"""
import re

import numpy as np
import torch

from . import engine as E
from . import ops
from . import weights

# sdod_image_to_u8 truncates: round(255 * clamp(y, 0, 1)) = clamp(floor(255 * (y + 1 / 510)), 0, 255), its mode 0 with a = 1, b = 1 / 510
U8_A, U8_B, U8_MODE = 1.0, 0.5 / 255.0, 0


def blocks_in(names):
    """number of RRDB blocks named by a collection of basicsr parameter names (body.N.*); ValueError when there is none"""
    found = {int(m.group(1)) for m in (re.match(r'body\.(\d+)\.', k) for k in names) if m}
    if not found or found != set(range(len(found))):
        raise ValueError('upscaler: the parameters name no consecutive body.N blocks (convert the checkpoint with sdod.amd.convert --upscaler)')
    return len(found)


def upscaler_check_build(state_dict, path, image_hw, num_blocks):
    """the argument contract of Upscaler(...) and of Txt2Img(upscaler=True), checked before any device work: exactly one source of
    parameters; image_hw a pair of multiples of 8 in [8, 1024]; num_blocks None (read from the parameter names) or the number the
    parameters have.  Returns (num_blocks, (h, w)); raises ValueError."""
    if (state_dict is None) == (path is None):
        raise ValueError('upscaler: give exactly one of state_dict and path')
    names = list(state_dict) if state_dict is not None else weights.names(path)
    found = blocks_in(names)
    if num_blocks is None:
        num_blocks = found
    if isinstance(num_blocks, (bool, float)) or not isinstance(num_blocks, (int, np.integer)) or int(num_blocks) != found:
        raise ValueError(f'upscaler: num_blocks={num_blocks!r} but the parameters have {found} blocks')
    return int(num_blocks), E.upscaler_check_config(int(num_blocks), image_hw)


def upscale_check_args(img_u8, image_hw):
    """img_u8: a uint8 tensor [n, H, W, 3] with (H, W) = image_hw, n >= 1; raises ValueError"""
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8:
        raise ValueError(f'img_u8 must be a uint8 tensor, got {getattr(img_u8, "dtype", type(img_u8))}')
    if img_u8.dim() != 4 or img_u8.shape[0] < 1 or tuple(img_u8.shape[1:]) != (image_hw[0], image_hw[1], 3):
        raise ValueError(f'img_u8 must be [n, {image_hw[0]}, {image_hw[1]}, 3], got {tuple(img_u8.shape)}')


class Upscaler:
    image_hw = (512, 512)
    graph = None

    def __init__(self, state_dict=None, path=None, image_hw=(512, 512), num_blocks=None, device='cuda:0', use_hip_graph=True):
        """state_dict: basicsr-named RRDBNet parameters (sdod.amd.convert.upscaler_parameters maps the other namings), or path: an
        upscaler.sdodw container.  image_hw: the input size the graph is built for, multiples of 8 in [8, 1024]; the output is 4x.
        Device memory: graph.stats() ('weight_bytes' + 'arena_bytes'), 33 MB + 1.2 GB at 512 x 512 with 23 blocks."""
        num_blocks, self.image_hw = upscaler_check_build(state_dict, path, image_hw, num_blocks)
        self.device = torch.device(device)
        self.use_hip_graph = use_hip_graph
        self.graph = E.Upscaler(num_blocks, self.image_hw, 1, device)
        if state_dict is not None:
            self.graph.load_state_dict(state_dict)
        else:
            self.graph.load_file(path)
        self.graph.finalize()

    def upscale_float(self, img_u8):
        """uint8 [n, H, W, 3] -> fp16 [n, 4H, 4W, 3], the network's output (nominally in [0, 1], not clamped)"""
        upscale_check_args(img_u8, self.image_hw)
        return torch.cat([self._run(img_u8[i:i + 1]).clone() for i in range(img_u8.shape[0])], 0)

    def upscale(self, img_u8):
        """uint8 [n, H, W, 3] -> uint8 [n, 4H, 4W, 3] = round(255 * clamp(y, 0, 1))"""
        upscale_check_args(img_u8, self.image_hw)
        return torch.cat([ops.image_to_u8(self._run(img_u8[i:i + 1]), U8_A, U8_B, U8_MODE) for i in range(img_u8.shape[0])], 0)

    def _run(self, one):
        with torch.cuda.device(self.device):
            self.graph.img.copy_(one)
            self.graph.execute(self.use_hip_graph)
        return self.graph.out
