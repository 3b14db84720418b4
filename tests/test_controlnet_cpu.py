"""ControlNet without a GPU: the fp32 restatement (tests/controlnet_ref.py) against the plain oracle, the parameter tables of the
three control graphs, the converter's key handling and refusals, and the host-side argument checks of the pipeline."""
import numpy as np
import pytest
import torch

import controlnet_ref as CR

MC = 64          # a narrow UNet keeps the oracle quick; the restatement is the same code at every width


def _sd(table, seed):
    from sdod.amd import weights as Wt
    return Wt.synthetic_state_dict(table, seed=seed)


@pytest.fixture(scope='module')
def small():
    from oracle import sd_torch as S
    with torch.device('meta'):
        unet = S.UNetModel(model_ch=MC)
    usd = _sd([(k, tuple(v.shape)) for k, v in unet.state_dict().items()], 3)
    unet.load_state_dict(usd, assign=True)
    csd = _sd(CR.param_table(MC), 4)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 8, 16, generator=g)
    ctx = torch.randn(2, 77, 768, generator=g)
    t = torch.tensor([801.0, 801.0])
    hint = torch.randint(0, 256, (1, 64, 128, 3), generator=g, dtype=torch.uint8)
    return dict(unet=unet.eval(), control=CR.ControlNet(csd, MC).eval(), x=x, ctx=ctx, t=t, hint=hint)


def test_restatement_with_zero_scales_is_the_plain_oracle(small):
    s = small
    with torch.no_grad():
        plain = s['unet'](s['x'], s['t'], s['ctx'])
        res = s['control'](s['x'], s['t'], s['ctx'], s['control'].guided_hint(s['hint']))
        zero = CR.controlled_unet(s['unet'], s['x'], s['t'], s['ctx'], res, [0.0] * 13)
        on = CR.controlled_unet(s['unet'], s['x'], s['t'], s['ctx'], res, [1.0] * 13)
    assert torch.equal(zero, plain)
    assert [tuple(r.shape) for r in res] == [(2, c, 8 // d, 16 // d) for c, d in zip(CR.residual_channels(MC), [1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8, 8])]
    assert float((on - plain).norm() / plain.norm()) > 5e-2
    # the guided hint is added behind input_blocks.0: without it the first residual changes
    with torch.no_grad():
        res0 = s['control'](s['x'], s['t'], s['ctx'], torch.zeros(1, MC, 8, 16))
    assert not torch.equal(res0[0], res[0])


def test_graph_tables_and_shapes():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 24)
    assert E.CONTROLNET == 8 and E.CONTROL_HINT == 9
    shapes = E.control_residual_shapes(cfg, 2)
    assert len(shapes) == 13 and shapes[0] == (2, 16, 24, 320) and shapes[3] == (2, 8, 12, 320) and shapes[6] == (2, 4, 6, 640)
    assert shapes[9] == shapes[12] == (2, 2, 3, 1280)
    want = dict(CR.param_table())
    tcfg = E.copy_config(cfg); tcfg.control_temb = 1
    cn, tb, hb = E.ControlNet(cfg, 2).param_table(), E.Temb(tcfg, 1).param_table(), E.ControlHint(cfg, 1).param_table()
    assert all(want[n] == s for n, s in cn + tb)
    assert {n for n, _ in cn + tb + hb} == set(want)
    assert sum(s[0] for n, s in tb if n.endswith('emb_layers.1.bias')) == 30 * 320
    assert dict(hb)['input_hint_block.0.weight'] == (64, 3, 3, 3) and dict(hb)['input_hint_block.8.weight'] == (128, 64, 3, 3)
    assert dict(hb)['input_hint_block.14.weight'] == (320, 256, 3, 3)
    # without the switches: the tables of the plain graphs, through the creation entry point they always used
    ucfg = E.copy_config(cfg); ucfg.control_inputs = 1
    assert E.UNet(ucfg, 2).param_table() == E.UNet(cfg, 2).param_table()
    assert len(E.Temb(cfg, 1).param_table()) == 4 + 2 * 22
    assert E.copy_config(ucfg).control_inputs == 1 and E.copy_config(cfg).control_inputs == 0


def test_engine_refusals():
    from sdod.amd import _lib, engine as E
    cfg = E.sd14_config(16, 16)
    with pytest.raises(_lib.SdodError, match='even batch'):
        E.ControlNet(cfg, 3)
    lib = E._engine()
    import ctypes
    for kind in (E.CONTROLNET, E.CONTROL_HINT):            # the new kinds only through their own entry point
        h = ctypes.c_void_p()
        assert lib.sdod_graph_create(ctypes.byref(h), kind, ctypes.byref(cfg), 2) != 0 and not h.value
    assert lib.sdod_graph_create(ctypes.byref(ctypes.c_void_p()), 10, ctypes.byref(cfg), 2) != 0
    bad = E.ControlConfig(1, 0)                            # control_inputs on a kind it does not apply to
    assert lib.sdod_graph_create_control(ctypes.byref(ctypes.c_void_p()), E.VAE_DECODER, ctypes.byref(cfg), ctypes.byref(bad), 1) != 0
    assert lib.sdod_graph_create_control(ctypes.byref(ctypes.c_void_p()), E.UNET, ctypes.byref(cfg), ctypes.byref(E.ControlConfig(2, 0)), 2) != 0
    qcfg = E.copy_config(cfg); qcfg.weight_quant = 1
    with pytest.raises(_lib.SdodError, match='weight_quant'):
        E.ControlNet(qcfg, 2)
    for extra in (dict(adapter_reps=2),):
        acfg = E.sd14_config(16, 16, **extra); acfg.control_inputs = 1
        with pytest.raises(ValueError, match='T2I-Adapter'):
            E.UNet(acfg, 2)
    g = E.ControlNet(cfg, 2)
    with pytest.raises(_lib.SdodError, match='out of range'):
        check = _lib.check
        check(lib.sdod_graph_bind_output(g._h, 13, ctypes.c_void_p(256), 2 * 16 * 16 * 320 * 2))
    with pytest.raises(_lib.SdodError, match='size mismatch'):
        _lib.check(lib.sdod_graph_bind_output(g._h, 0, ctypes.c_void_p(256), 16))
    with pytest.raises(_lib.SdodError, match='misaligned'):
        _lib.check(lib.sdod_graph_bind_output(g._h, 0, ctypes.c_void_p(264), 2 * 16 * 16 * 320 * 2))


def test_hint_parameters_are_padded_where_they_are_set():
    from sdod.amd import engine as E
    g = E.ControlHint(E.sd14_config(16, 16), 1)
    seen = {}
    g_set = E.Graph.set_param
    try:
        E.Graph.set_param = lambda self, name, tensor: seen.__setitem__(name, tensor)
        w = torch.arange(32 * 16 * 9, dtype=torch.float32).reshape(32, 16, 3, 3) + 1
        g.set_param('input_hint_block.4.weight', w)
        g.set_param('input_hint_block.4.bias', torch.ones(32))
        g.set_param('input_hint_block.14.bias', torch.ones(320))
    finally:
        E.Graph.set_param = g_set
    p = seen['input_hint_block.4.weight']
    assert tuple(p.shape) == (64, 64, 3, 3) and torch.equal(p[:32, :16], w) and not bool(p[32:].any()) and not bool(p[:, 16:].any())
    assert tuple(seen['input_hint_block.4.bias'].shape) == (64,) and float(seen['input_hint_block.4.bias'].sum()) == 32.0
    assert tuple(seen['input_hint_block.14.bias'].shape) == (320,)


# ------------------------------------------------------------------ converter
@pytest.fixture(scope='module')
def checkpoint():
    return {'control_model.' + k: v.half() for k, v in _sd(CR.param_table(), 6).items()}


def test_converter_strips_the_prefix_and_pads_the_hint_block(checkpoint, tmp_path):
    from sdod.amd import convert as C, engine as E, weights as Wt
    sd = dict(checkpoint)
    sd['model.diffusion_model.out.2.bias'] = torch.zeros(4)           # a full control_sd15_*.pth carries the base model too
    part = C.controlnet_parameters(sd)
    tables = C.controlnet_tables()
    for table in tables.values():
        for name, shape in table:
            assert tuple(part[name].shape) == tuple(shape) and part[name].dtype == torch.float16
    assert len(part) == sum(len(t) for t in tables.values()) == len(checkpoint)
    w = checkpoint['control_model.input_hint_block.8.weight']
    p = part['input_hint_block.8.weight']
    assert tuple(w.shape) == (96, 32, 3, 3) and tuple(p.shape) == (128, 64, 3, 3)
    assert torch.equal(p[:96, :32], w) and not bool(p[96:].any()) and not bool(p[:, 32:].any())
    assert torch.equal(part['zero_convs.3.0.weight'], checkpoint['control_model.zero_convs.3.0.weight'])
    # names already stripped are taken as they are; .pth through the file path
    bare = {k[len('control_model.'):]: v for k, v in checkpoint.items()}
    assert all(torch.equal(a, C.controlnet_parameters(bare)[k]) for k, a in part.items())
    path = tmp_path / 'control.pth'
    torch.save(checkpoint, path)
    out = C.convert_controlnet(str(path), str(tmp_path / 'models'))
    assert out.endswith('controlnet.sdodw')
    back = Wt.load(out)
    assert set(back) == set(part) and all(torch.equal(torch.as_tensor(np.asarray(back[k])).reshape(part[k].shape), part[k]) for k in list(part)[:8])
    C.main(['--controlnet', str(path), '--out', str(tmp_path / 'models2')])
    assert (tmp_path / 'models2' / 'controlnet.sdodw').exists()


def test_converter_refusals(checkpoint):
    from sdod.amd import convert as C
    with pytest.raises(ValueError, match='diffusers'):
        C.controlnet_state_dict({'controlnet_cond_embedding.conv_in.weight': torch.zeros(16, 3, 3, 3), 'down_blocks.0.resnets.0.conv1.weight': torch.zeros(1)})
    with pytest.raises(ValueError, match='diffusers'):
        C.controlnet_state_dict({'down_blocks.0.resnets.0.conv1.weight': torch.zeros(1)})
    sd21 = dict(checkpoint)
    sd21['control_model.input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight'] = torch.zeros(320, 1024)
    with pytest.raises(ValueError, match='1024'):
        C.controlnet_state_dict(sd21)
    grey = dict(checkpoint)
    grey['control_model.input_hint_block.0.weight'] = torch.zeros(16, 1, 3, 3)
    with pytest.raises(ValueError, match='3-channel'):
        C.controlnet_state_dict(grey)
    with pytest.raises(ValueError, match='not a ControlNet'):
        C.controlnet_state_dict({'model.diffusion_model.out.2.bias': torch.zeros(4)})
    short = {k: v for k, v in checkpoint.items() if 'zero_convs.7' not in k}
    with pytest.raises(KeyError, match='zero_convs.7'):
        C.controlnet_parameters(short)
    wrong = dict(checkpoint)
    wrong['control_model.input_hint_block.2.weight'] = torch.zeros(16, 8, 3, 3)
    with pytest.raises(ValueError, match='input_hint_block.2.weight'):
        C.controlnet_parameters(wrong)


# ------------------------------------------------------------------ pipeline, host side
@pytest.mark.parametrize('kw', [dict(cfg_split=True), dict(hires_hw=32), dict(inpaint_unet=True), dict(adapter=True), dict(tiling=True),
                                dict(tiling='x'), dict(model='sd21')])
def test_control_check_build_refuses_before_any_device_work(kw):
    from sdod.amd import pipeline as PL
    base = dict(cfg_split=False, hires_hw=None, inpaint_unet=False, adapter=False, tiling=False, model='sd14')
    PL.control_check_build(True, **base)
    PL.control_check_build(False, **dict(base, **kw))                    # without the flag nothing is checked
    with pytest.raises(ValueError, match='controlnet=True cannot be combined'):
        PL.control_check_build(True, **dict(base, **kw))
    with pytest.raises(ValueError, match='controlnet=True cannot be combined'):   # the constructor: before it touches the device
        PL.Txt2Img(state_dicts={}, latent_hw=16, controlnet=True, **kw)


def test_control_check_args():
    from sdod.amd import pipeline as PL
    lat = (4, 8, 16)
    hint = torch.zeros(2, 64, 128, 3, dtype=torch.uint8)
    h, s = PL.control_check_args(hint, 1.0, lat, 2)
    assert h is hint or torch.equal(h, hint)
    assert s == [1.0] * 13
    grey = torch.arange(2 * 64 * 128, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(2, 64, 128)
    h, s = PL.control_check_args(grey, np.float32(0.5), lat, 2)
    assert tuple(h.shape) == (2, 64, 128, 3) and h.is_contiguous() and all(torch.equal(h[..., k], grey) for k in range(3)) and s == [0.5] * 13
    _, s = PL.control_check_args(hint, [0.1 * k for k in range(13)], lat, 2)
    assert s == [0.1 * k for k in range(13)]
    _, s = PL.control_check_args(hint, torch.linspace(0, 1, 13), lat, 2)
    assert len(s) == 13 and s[-1] == 1.0
    for bad in (hint[:1], hint[..., :1], hint[:, :32], hint.float(), hint.numpy(), torch.zeros(2, 64, 128, 3, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            PL.control_check_args(bad, 1.0, lat, 2)
    for bad in (float('nan'), float('inf'), [1.0] * 12, [1.0] * 14, [1.0] * 12 + [float('inf')], 'one', None, True):
        with pytest.raises(ValueError):
            PL.control_check_args(hint, bad, lat, 2)


def test_setters_need_the_flag():
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)                                     # a pipeline object without the flag's graphs (class defaults)
    assert pipe.controlnet is None and pipe.control_hint is None and pipe._control_on is False
    with pytest.raises(RuntimeError, match='controlnet=True'):
        pipe.set_control_hint(torch.zeros(1, 128, 128, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='controlnet=True'):
        pipe.clear_control_hint()


def test_symbols_are_listed():
    from sdod.amd import _lib, engine as E
    assert 'sdod_add_control_f16' in _lib.HIP_SYMBOLS
    assert {'sdod_graph_create_control', 'sdod_graph_bind_output'} <= set(E.ENGINE_SYMBOLS)
    assert _lib.ControlSeg.h.offset == 0 and _lib.ControlSeg.r.offset == 8 and _lib.ControlSeg.count.offset == 16
