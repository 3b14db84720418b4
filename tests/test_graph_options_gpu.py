"""The older create functions against the classes of sdod.amd.engine, which reach every graph through sdod_graph_create_opts: the same
launch list, the same memory and the same output bits.  Parameter tables (tests/test_graph_options_cpu.py) cannot see wrap, fused_attn
or control_inputs; the launch lists and the outputs can.  Same kernels on the same operands, so equality is exact."""
import ctypes

import pytest
import torch

from sdod.amd import engine as E, weights as Wt

pytestmark = pytest.mark.gpu

_STATE_DICTS = {}       # parameter table -> synthetic weights: the three UNet cases share one checkpoint


def state_dict(table):
    key = tuple(table)
    if key not in _STATE_DICTS:
        _STATE_DICTS[key] = Wt.synthetic_state_dict(table, 8100)
    return _STATE_DICTS[key]


def adopt(cls, handle, cfg, batch, **attrs):
    """a raw handle of the C ABI as an object of `cls`, without running its constructor (which would create a graph of its own)"""
    g = cls.__new__(cls)
    g._lib, g._h, g.cfg, g.batch, g.device, g.finalized = E._engine(), handle, cfg, batch, torch.device('cuda:0'), False
    for n, v in attrs.items():
        setattr(g, n, v)
    return g


def sd14(hw, **side):
    cfg = E.sd14_config(hw, hw)
    for n, v in side.items():
        setattr(cfg, n, v)
    return cfg


UNET_IO = (['x', 'temb', 'ctx'], ['eps'])
CASES = {
    # name: (class, cfg, batch, wrapper call on (lib, handle ref, cfg), constructor, attributes of an adopted object, inputs, outputs)
    'wrap': (E.UNet, sd14(16), 2,
             lambda lib, h, c: lib.sdod_graph_create_wrap(h, E.UNET, ctypes.byref(c), ctypes.byref(E.AdapterConfig(0, 0, 0)), 3, 2),
             lambda c: E.UNet(c, 2, wrap=3), {}) + UNET_IO,
    'control': (E.UNet, sd14(16, control_inputs=1), 2,
                lambda lib, h, c: lib.sdod_graph_create_control(h, E.UNET, ctypes.byref(c), ctypes.byref(E.ControlConfig(1, 0)), 2),
                lambda c: E.UNet(c, 2), {}, ['x', 'temb', 'ctx', 'control_res', 'control_scale'], ['eps']),
    'regions': (E.UNet, sd14(16, context_len=154, regions=2), 2,
                lambda lib, h, c: lib.sdod_graph_create_regions(h, E.UNET, ctypes.byref(c), ctypes.byref(E.RegionConfig(2)), 2),
                lambda c: E.UNet(c, 2), {}, ['x', 'temb', 'ctx', 'region_w'], ['eps']),
    'vae': (E.VaeDecoder, sd14(8), 1,
            lambda lib, h, c: lib.sdod_graph_create_vae(h, E.VAE_DECODER, ctypes.byref(c), 0, ctypes.byref(E.VaeConfig(1)), 1),
            lambda c: E.VaeDecoder(c, 1, fused_attn=True), {}, ['z'], ['img']),
    'lcm': (E.Temb, sd14(16), 2,
            lambda lib, h, c: lib.sdod_graph_create_lcm(h, E.TEMB, ctypes.byref(c), ctypes.byref(E.LcmConfig(256)), 2),
            lambda c: E.Temb(c, 2, cond_proj_dim=256), {'cond_proj_dim': 256}, ['t', 'w'], ['out']),
}


def tensors(g, names):
    out = []
    for n in names:
        v = getattr(g, n)
        out += list(v) if isinstance(v, (list, tuple)) else [v]
    return out


def fill(g, names, seed):
    gen = torch.Generator().manual_seed(seed)
    for t in tensors(g, names):
        if t.dim() == 1:        # timesteps, guidance scales, control scales: positive and of moderate size
            v = 0.25 + torch.rand(t.shape, generator=gen) * (900.0 if t.numel() == g.batch else 1.0)
        else:
            v = torch.randn(t.shape, generator=gen) * 0.5
        t.copy_(v.to(t.dtype))


@pytest.mark.parametrize('name', list(CASES))
def test_wrapper_and_class_build_the_same_graph(name):
    cls, cfg, batch, wrapper, make, attrs, ins, outs = CASES[name]
    lib = E._engine()
    h = ctypes.c_void_p()
    with torch.cuda.device(0):
        assert wrapper(lib, ctypes.byref(h), cfg) == 0 and h.value
    pair = [adopt(cls, h, cfg, batch, **attrs), make(cfg)]
    assert pair[0].param_table() == pair[1].param_table()
    sd = state_dict(pair[0].param_table())
    got = []
    for g in pair:
        g.load_state_dict(sd)
        g.finalize()
        fill(g, ins, 8200)
        g.execute()
        torch.cuda.synchronize()
        got.append([t.clone() for t in tensors(g, outs)])
    a, b = pair
    assert a.op_table() == b.op_table() and len(a.op_table()) > 0
    assert a.op_details() == b.op_details() and a.stats() == b.stats()
    for x, y in zip(*got):
        assert x.shape == y.shape and bool(torch.isfinite(x.float()).all()) and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
