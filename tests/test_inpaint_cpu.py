"""Inpainting on the host side (no GPU): the three new entry points resolve in the built library, the ctypes mirror of
sdod_ddim_inpaint_step_args has the C compiler's layout, the per-step noise levels of the loop against an independent numpy
restatement of ldm's schedule, and the argument contract of Txt2Img.inpaint (ValueError before any device work)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inpaint_symbols_resolve_and_are_bound():
    from sdod.amd import _lib
    lib = _lib.load('libsdod.so')
    for sym in ('sdod_ddim_inpaint_step', 'sdod_mask_to_latent_f32', 'sdod_image_composite_u8'):
        assert getattr(lib, sym) is not None
        assert sym in _lib.HIP_SYMBOLS
    typed = _lib.hip()
    assert typed.sdod_ddim_inpaint_step.argtypes[0] == ctypes.POINTER(_lib.DdimInpaintStepArgs)
    assert len(typed.sdod_mask_to_latent_f32.argtypes) == 7
    assert len(typed.sdod_image_composite_u8.argtypes) == 10


def test_ddim_inpaint_step_args_mirror_has_the_c_layout():
    """sizeof and the offsets of the first non-pointer field, of the first int, the first float and the last field, from a C build
    of the header (the method of test_gemm_desc_mirror_has_pad_mode_at_the_c_offset)"""
    from sdod.amd._lib import DdimInpaintStepArgs as A
    assert A._fields_[-1] == ('known_s1a', ctypes.c_float)
    probes = ('seed', 'n', 'noise_level', 'guidance', 'known_s1a')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sdod_hip.h"\nint main(void){printf("'
           + ' '.join(['%zu'] * (len(probes) + 1)) + '\\n", '
           + ', '.join(f'offsetof(sdod_ddim_inpaint_step_args, {p})' for p in probes)
           + ', sizeof(sdod_ddim_inpaint_step_args));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'o.c')
        with open(c, 'w') as f:
            f.write(src)
        exe = os.path.join(d, 'o')
        subprocess.check_call(['cc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe])
        vals = list(map(int, subprocess.check_output([exe]).split()))
    assert [getattr(A, p).offset for p in probes] == vals[:-1]
    assert ctypes.sizeof(A) == vals[-1]


@pytest.mark.parametrize('strength,steps', [(0.75, 20), (0.5, 20), (0.75, 50), (0.3, 50), (0.05, 20), (0.99, 50), (0.4, 8)])
def test_inpaint_levels_match_an_independent_restatement(strength, steps):
    """(index, j, sa, s1a) of every step: x' of ddim index `index` sits at alphas_prev[index] = alphas_cumprod[timesteps[index - 1]],
    so the known region is q_sample'd with sqrt(abar) / sqrt(1 - abar) of ddim index j = index - 1; the last step has no level"""
    from oracle.pipeline_oracle import _alphas_cumprod
    from sdod.amd.pipeline import img2img_schedule, inpaint_levels
    sch, t_enc = img2img_schedule(strength, steps)
    assert t_enc == int(strength * steps)
    ac = _alphas_cumprod().astype(np.float32)
    ddim_t = np.arange(0, 1000, 1000 // steps) + 1
    want = []
    for index in range(t_enc - 1, 0, -1):
        abar = ac[ddim_t[index - 1]]
        want.append((index, index - 1, np.float32(np.sqrt(abar)), np.float32(np.sqrt(np.float32(1.0) - abar))))
        # the level is the one the DDIM step of `index` reaches
        assert np.float32(sch.alphas_prev[index]) == abar
    got = inpaint_levels(sch, t_enc)
    assert len(got) == t_enc
    assert got[-1] == (0, None, None, None)                     # the last step: known = z0, no noise level
    assert [(i, j, np.float32(a), np.float32(b)) for i, j, a, b in got[:-1]] == want
    assert all(j is not None and 0 <= j <= t_enc - 2 for _, j, _, _ in got[:-1])    # rows of step_noise [t_enc - 1, ...]


def _args(n=1, hw=16):
    return torch.zeros(n, 8 * hw, 8 * hw, 3, dtype=torch.uint8), torch.zeros(n, 8 * hw, 8 * hw, dtype=torch.uint8)


def test_inpaint_check_args_accepts_the_contract():
    from sdod.amd.pipeline import inpaint_check_args
    init, mask = _args()
    sch, t_enc = inpaint_check_args(init, mask, 0.5, 20, None, (4, 16, 16), 1)
    assert t_enc == 10 and sch.steps == 20
    inpaint_check_args(init, mask, 0.5, 20, torch.zeros(9, 1, 4, 16, 16), (4, 16, 16), 1)
    inpaint_check_args(init, mask, 0.05, 20, torch.zeros(0, 1, 4, 16, 16), (4, 16, 16), 1)       # t_enc = 1: no noise level at all


@pytest.mark.parametrize('case', ['mask_shape', 'mask_rank', 'mask_dtype', 'init_dtype', 'init_rank', 'size', 'noise_len', 'noise_shape',
                                  'strength_hi', 'strength_lo', 'strength_neg'])
def test_inpaint_argument_errors_raise_before_device_work(case):
    """through Txt2Img.inpaint and inpaint_graphed themselves, on an object that has no device at all: any device work would fail
    with something other than ValueError"""
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)                               # no constructor: no graphs, no device
    pipe.cfg = E.sd14_config(16, 16)
    pipe.n = 1
    pipe.cfg_split = False
    init, mask = _args()
    kw = dict(strength=0.5, steps=20)
    if case == 'mask_shape':
        mask = mask[:, :-8]
    elif case == 'mask_rank':
        mask = mask[..., None]
    elif case == 'mask_dtype':
        mask = mask.float()
    elif case == 'init_dtype':
        init = init.float()
    elif case == 'init_rank':
        init = init[0]
    elif case == 'size':
        init, mask = _args(hw=24)
    elif case == 'noise_len':
        kw['step_noise'] = torch.zeros(10, 1, 4, 16, 16)
    elif case == 'noise_shape':
        kw['step_noise'] = torch.zeros(9, 1, 4, 16, 8)
    elif case == 'strength_hi':
        kw['strength'] = 1.0
    elif case == 'strength_lo':
        kw['strength'] = 0.01
    elif case == 'strength_neg':
        kw['strength'] = -0.5
    for fn in (pipe.inpaint, pipe.inpaint_graphed):
        with pytest.raises(ValueError):
            fn(None, init, mask, **kw)


def test_inpaint_refuses_another_batch_size():
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)
    pipe.cfg = E.sd14_config(16, 16)
    pipe.n = 1
    pipe.cfg_split = False
    init, mask = _args(n=2)
    for fn in (pipe.inpaint, pipe.inpaint_graphed):
        with pytest.raises(ValueError):
            fn(None, init, mask, strength=0.5, steps=20)
