"""T2I-Adapter structural control without a GPU: the argument contract, the checkpoint converter, the ADAPTER graph's parameter table
and the torch restatement (tests/adapter_ref.py) the GPU tests compare against."""
import ctypes

import pytest
import torch

import adapter_ref as AR


# ------------------------------------------------------------------ pipeline.adapter_check_args
def _hint(n=1, hw=16, ch=3, dtype=torch.uint8):
    g = torch.Generator().manual_seed(3)
    shape = (n, 8 * hw, 8 * hw) + (() if ch is None else (ch,))
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dtype)


def test_adapter_check_args_accepts_the_contract():
    from sdod.amd.pipeline import adapter_check_args
    for ch in (1, 3):
        out = adapter_check_args(_hint(ch=ch), 1.0, (4, 16, 16), 1, ch)
        assert tuple(out.shape) == (1, 128, 128, ch) and out.dtype == torch.uint8
    out = adapter_check_args(_hint(ch=None), 0.37, (4, 16, 16), 1, 1)         # [n, 8h, 8w] for one channel
    assert tuple(out.shape) == (1, 128, 128, 1)
    out = adapter_check_args(torch.zeros(2, 128, 192, 3, dtype=torch.uint8), 0, (4, 16, 24), 2, 3)   # rectangular, batch 2, an integer weight
    assert tuple(out.shape) == (2, 128, 192, 3)
    adapter_check_args(_hint(), -1.5, (4, 16, 16), 1, 3)                      # any finite weight


@pytest.mark.parametrize('case', ['dtype', 'not_tensor', 'channels', 'missing_axis_3ch', 'size', 'batch', 'rank', 'w_nan', 'w_inf',
                                  'w_str', 'w_bool', 'w_none'])
def test_adapter_check_args_rejects(case):
    from sdod.amd.pipeline import adapter_check_args
    hint, weight, ch = _hint(), 1.0, 3
    if case == 'dtype':
        hint = hint.float()
    elif case == 'not_tensor':
        hint = hint.numpy()
    elif case == 'channels':
        hint = _hint(ch=1)
    elif case == 'missing_axis_3ch':
        hint = _hint(ch=None)
    elif case == 'size':
        hint = hint[:, :-8]
    elif case == 'batch':
        hint = _hint(n=2)
    elif case == 'rank':
        hint = hint[0]
    elif case == 'w_nan':
        weight = float('nan')
    elif case == 'w_inf':
        weight = float('inf')
    elif case == 'w_str':
        weight = '1.0'
    elif case == 'w_bool':
        weight = True
    elif case == 'w_none':
        weight = None
    with pytest.raises(ValueError):
        adapter_check_args(hint, weight, (4, 16, 16), 1, ch)


def _bare_pipe(adapter):
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    pipe = Txt2Img.__new__(Txt2Img)                               # no constructor: no graphs, no device
    pipe.cfg = E.sd14_config(16, 16)
    pipe.n = 1
    if adapter:
        pipe.adapter = object()                                    # anything but None: any use of it fails with another error
    return pipe


def test_hint_argument_errors_raise_before_device_work():
    """through Txt2Img.set_adapter_hint itself on an object without a device: any device work would fail with something else"""
    pipe = _bare_pipe(True)
    for hint, weight in ((_hint().float(), 1.0), (_hint(ch=1), 1.0), (_hint(), float('nan')), (_hint()[:, :64], 1.0)):
        with pytest.raises(ValueError):
            pipe.set_adapter_hint(hint, weight)


def test_a_pipeline_without_adapter_refuses_hints():
    pipe = _bare_pipe(False)
    with pytest.raises(RuntimeError, match='adapter=True'):
        pipe.set_adapter_hint(_hint())
    with pytest.raises(RuntimeError, match='adapter=True'):
        pipe.clear_adapter_hint()


@pytest.mark.parametrize('kw', [dict(cfg_split=True), dict(hires_hw=32), dict(inpaint_unet=True), dict(model='sd21'),
                                dict(adapter_channels=2), dict(adapter_channels=True)])
def test_refused_combinations_raise_before_device_work(kw, monkeypatch):
    from sdod.amd.pipeline import Txt2Img
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a, **k: pytest.fail('device work before the argument checks'))
    with pytest.raises(ValueError):
        Txt2Img(state_dicts={}, latent_hw=16, with_text_encoder=False, adapter=True, **kw)


# ------------------------------------------------------------------ convert.adapter_config
def _synthetic(hint_channels=3, nums_rb=2, meta=True):
    with torch.device('meta' if meta else 'cpu'):
        return {n: torch.zeros(s) for n, s in AR.param_table(hint_channels, nums_rb)}


@pytest.mark.parametrize('hc,nrb', [(1, 2), (3, 2), (3, 1), (1, 3)])
def test_adapter_config_infers_channels_and_blocks(hc, nrb):
    from sdod.amd import convert
    assert convert.adapter_config(_synthetic(hc, nrb)) == (hc, nrb)


@pytest.mark.parametrize('case,word', [('light', 'Adapter_light'), ('skep', 'sk=False'), ('down_opt', 'use_conv=True'),
                                       ('block2_3x3', 'block2'), ('diffusers', 'diffusers')])
def test_adapter_config_refuses_other_layouts_by_name(case, word):
    from sdod.amd import convert
    sd = _synthetic()
    with torch.device('meta'):
        if case == 'light':
            sd = {'conv_in.weight': sd['conv_in.weight'], 'body.0.in_conv.weight': torch.zeros(80, 192, 1, 1),
                  'body.0.body.0.block1.weight': torch.zeros(80, 80, 1, 1), 'body.0.out_conv.weight': torch.zeros(320, 80, 1, 1)}
        elif case == 'skep':
            sd['body.0.skep.weight'] = torch.zeros(320, 320, 1, 1)
        elif case == 'down_opt':
            sd['body.2.down_opt.op.weight'] = torch.zeros(320, 320, 3, 3)
        elif case == 'block2_3x3':
            sd['body.5.block2.weight'] = torch.zeros(1280, 1280, 3, 3)
        elif case == 'diffusers':
            sd = {'adapter.conv_in.weight': sd['conv_in.weight'], 'adapter.body.0.resnets.0.block1.weight': torch.zeros(320, 320, 3, 3)}
    with pytest.raises(ValueError, match=word):
        convert.adapter_config(sd)


def test_adapter_checkpoint_converts_and_round_trips(tmp_path, monkeypatch):
    """a miniature table (real names, small shapes) through convert_adapter and back through weights.load"""
    from sdod.amd import convert, weights as Wt
    table = [('conv_in.weight', (8, 64, 3, 3)), ('conv_in.bias', (8,))] + \
            [(f'body.{k}.{b}.{p}', s) for k in range(8) for b, p, s in (('block1', 'weight', (8, 8, 3, 3)), ('block1', 'bias', (8,)),
                                                                         ('block2', 'weight', (8, 8, 1, 1)), ('block2', 'bias', (8,)))]
    seen = []
    monkeypatch.setattr(convert, 'adapter_table', lambda hc, nrb=2, cfg=None: seen.append((hc, nrb)) or table)
    sd = Wt.synthetic_state_dict(table, seed=9)
    src = tmp_path / 'adapter.pth'
    torch.save(sd, src)
    out = convert.convert_adapter(str(src), str(tmp_path / 'models'))
    assert out.endswith('adapter.sdodw') and seen == [(1, 2)]
    back = Wt.load(out)
    assert list(back) == [n for n, _ in table]
    assert all(torch.equal(back[n], sd[n].half()) for n in back)
    convert.main(['--adapter', str(src), '--out', str(tmp_path / 'm2')])              # the command line writes the same file
    assert (tmp_path / 'm2' / 'adapter.sdodw').read_bytes() == open(out, 'rb').read()
    del sd['body.3.block2.bias']
    torch.save(sd, src)
    with pytest.raises(KeyError, match='body.3.block2.bias'):
        convert.convert_adapter(str(src), str(tmp_path / 'models'))


# ------------------------------------------------------------------ the graph's parameter table and configuration
@pytest.mark.parametrize('hc,nrb', [(3, 0), (1, 0), (3, 1)])
def test_adapter_param_table_is_the_checkpoints(hc, nrb):
    from sdod.amd import engine as E
    table = E.Adapter(E.sd14_config(16, 16, adapter_hint_channels=hc, adapter_res_blocks=nrb), 1).param_table()
    assert table == AR.param_table(hc, nrb or 2)
    d = dict(table)
    assert d['conv_in.weight'] == (320, 64 * hc, 3, 3)
    if not nrb:
        assert d['body.2.in_conv.weight'] == (640, 320, 1, 1) and d['body.4.in_conv.weight'] == (1280, 640, 1, 1)
        assert 'body.6.in_conv.weight' not in d and 'body.0.in_conv.weight' not in d and len(table) == 2 + 8 * 4 + 2 * 2
        assert d['body.7.block1.weight'] == (1280, 1280, 3, 3) and d['body.7.block2.weight'] == (1280, 1280, 1, 1)
    from sdod.amd import convert
    assert convert.adapter_table(hc, nrb or 2, E.sd14_config(16, 16)) == table


def test_adapter_graph_refuses_what_it_cannot_build():
    from sdod.amd import engine as E
    from sdod.amd._lib import SdodError
    for kw in (dict(adapter_hint_channels=0), dict(adapter_hint_channels=2), dict(adapter_hint_channels=3, adapter_res_blocks=9)):
        with pytest.raises(SdodError):
            E.Adapter(E.sd14_config(16, 16, **kw), 1)
    for h, w in ((12, 16), (16, 4)):                                   # the UNet's size rule
        with pytest.raises(SdodError):
            E.Adapter(E.sd14_config(h, w, adapter_hint_channels=3), 1)
    for reps, batch in ((3, 3), (2, 3), (-1, 2)):                      # adapter_reps 0, 1 or 2, dividing the batch
        with pytest.raises(SdodError):
            E.UNet(E.sd14_config(16, 16, adapter_reps=reps), batch)
    lib = E._engine()
    h = ctypes.c_void_p()
    cfg = E.sd14_config(16, 16)
    assert lib.sdod_graph_create(ctypes.byref(h), E.ADAPTER, ctypes.byref(cfg), 1) != 0 and not h.value   # no hint width: refused


def test_adapter_inputs_change_no_parameter_of_the_unet():
    """adapter_reps adds inputs and launches, never parameters; the model config mirror keeps its size"""
    from sdod.amd import engine as E
    plain = E.UNet(E.sd14_config(16, 16), 2).param_table()
    assert E.UNet(E.sd14_config(16, 16, adapter_reps=2), 2).param_table() == plain
    assert E.UNet(E.sd14_config(16, 16, adapter_reps=1), 2).param_table() == plain
    cfg = E.sd14_config(16, 24, adapter_reps=2, adapter_hint_channels=1)
    cp = E.copy_config(cfg)
    assert (cp.adapter_reps, cp.adapter_hint_channels, cp.adapter_res_blocks, cp.latent_h, cp.latent_w) == (2, 1, 0, 16, 24)
    cp.adapter_reps = 0
    assert cfg.adapter_reps == 2
    raw = E.ModelConfig.from_buffer_copy(cfg)                          # the ctypes copy carries them too; a raw buffer has none
    assert (raw.adapter_reps, raw.adapter_hint_channels, raw.latent_w) == (2, 1, 24)
    assert E.ModelConfig.from_buffer_copy(bytes(cfg)).adapter_reps == 0
    assert ctypes.sizeof(E.AdapterConfig) == 12 and [n for n, _ in E.AdapterConfig._fields_] == ['adapter_reps', 'adapter_hint_channels',
                                                                                              'adapter_res_blocks']
    assert E.adapter_feature_shapes(cfg, 1) == [(1, 16, 24, 320), (1, 8, 12, 640), (1, 4, 6, 1280), (1, 2, 3, 1280)]


def test_new_symbols_resolve_and_are_bound():
    from sdod.amd import _lib, engine as E
    lib = _lib.hip()
    for s in ('sdod_pixel_unshuffle_u8_f16', 'sdod_avg_pool2_f16', 'sdod_adapter_stage_f16', 'sdod_add_feature_f16'):
        assert s in _lib.HIP_SYMBOLS and getattr(lib, s).argtypes is not None
    assert 'sdod_graph_create_ex' in E.ENGINE_SYMBOLS and hasattr(lib, 'sdod_graph_create_ex')


# ------------------------------------------------------------------ the restatement
def test_restatement_returns_the_four_maps():
    from sdod.amd import weights as Wt
    sd = Wt.synthetic_state_dict(AR.param_table(3), seed=5)
    g = torch.Generator().manual_seed(6)
    hint = torch.randint(0, 256, (1, 128, 128, 3), generator=g, dtype=torch.uint8)     # a 3 x 128 x 128 input
    outs = AR.adapter_forward(sd, hint)
    assert [tuple(o.shape) for o in outs] == [(1, 320, 16, 16), (1, 640, 8, 8), (1, 1280, 4, 4), (1, 1280, 2, 2)]
    assert all(torch.isfinite(o).all() and float(o.abs().mean()) > 1e-3 for o in outs)
    other = AR.adapter_forward(sd, hint.flip(1))
    assert all(not torch.equal(a, b) for a, b in zip(outs, other))
    # the unshuffle's channel order: channel c * 64 + dy * 8 + dx of pixel (i, j) is image pixel (8 i + dy, 8 j + dx), channel c
    u = AR.unshuffle(hint)
    assert tuple(u.shape) == (1, 192, 16, 16)
    assert torch.equal(u[0, 2 * 64 + 3 * 8 + 5, 7, 9], hint[0, 8 * 7 + 3, 8 * 9 + 5, 2].float() / 255)


def test_hooks_add_behind_blocks_2_5_8_11():
    """the hooked oracle: feature k changes the output, and only through input_blocks[LEVELS[k]]"""
    seen = {}

    class Blk(torch.nn.Module):
        def forward(self, x, emb=None, context=None):
            return x + 1

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.input_blocks = torch.nn.ModuleList([Blk() for _ in range(12)])

        def forward(self, x):
            for i, m in enumerate(self.input_blocks):
                x = m(x, None, None)
                seen[i] = x.clone()
            return x

    toy = Toy()
    x = torch.zeros(2, 1, 1, 1)
    f = torch.full((1, 1, 1, 1), 10.0)
    with AR.hooked(toy, [None, f, None, None]) as m:
        out = m(x)
    assert float(out[0]) == 22.0 and float(out[1]) == 22.0 and float(seen[4][0]) == 5.0 and float(seen[5][0]) == 16.0
    assert float(toy(x)[0]) == 12.0                                        # hooks removed
