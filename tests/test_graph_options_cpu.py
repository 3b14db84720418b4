"""sdod_graph_create_opts and the one record behind the ten older create functions (include/sdod_engine.h at sdod_graph_options).
Graph construction only declares parameters, so nothing here needs a device."""
import ctypes
import itertools
import re

import pytest

from sdod.amd import _lib, engine as E

INVALID_ARGUMENT = 2
SMALL_VISION = (28, 14, 128, 2, 2, 256, 64, 1)
VISION_FIELDS = [n for n, _ in E.VisionConfig._fields_]


def options(**fields):
    return E.GraphOptions(size=ctypes.sizeof(E.GraphOptions), **fields)


def sd14(hw=16, **fields):
    cfg = E.sd14_config(hw, hw)
    for n, v in fields.items():
        setattr(cfg, n, v)
    return cfg


def ref(struct):
    return None if struct is None else ctypes.byref(struct)


def param_table(lib, h):
    name, nd, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    out = []
    for i in range(lib.sdod_graph_num_params(h)):
        assert lib.sdod_graph_param_info(h, i, ctypes.byref(name), ctypes.byref(nd), shape) == 0
        out.append((name.value.decode(), tuple(shape[:nd.value])))
    return out


def create_opts(lib, kind, cfg, opts, batch):
    """(return code, handle, message) of sdod_graph_create_opts"""
    h = ctypes.c_void_p()
    rc = lib.sdod_graph_create_opts(ctypes.byref(h), kind, ref(cfg), ref(opts), batch)
    return rc, h, (_lib.hip().sdod_hip_last_error() or b'').decode()


def test_record_mirror_and_symbol():
    lib = E._engine()
    assert 'sdod_graph_create_opts' in E.ENGINE_SYMBOLS and lib.sdod_graph_create_opts.argtypes is not None
    names = [n for n, _ in E.GraphOptions._fields_]
    assert names[0] == 'size' and ctypes.sizeof(E.GraphOptions) == 4 * len(names) == 88
    # everything the side structs hold, in the header's order
    side = [n for c in (E.AdapterConfig,) for n, _ in c._fields_] + ['wrap'] + [
        n for c in (E.UpscalerConfig, E.ControlConfig, E.RegionConfig, E.IpConfig, E.VisionConfig, E.LcmConfig, E.VaeConfig) for n, _ in c._fields_]
    assert names[1:] == side
    header = open(__file__.replace('tests/test_graph_options_cpu.py', 'include/sdod_engine.h')).read()
    struct = header[header.index('typedef struct sdod_graph_options {'):header.index('} sdod_graph_options;')]
    assert re.findall(r'\b(\w+)(?=[,;])', re.sub(r'/\*.*?\*/', '', struct)) == names and 'sdod_graph_create_opts(' in header


# ------------------------------------------------------------------ every older function is a translation into the record
def wrapper_cases():
    """(id, wrapper call on (lib, handle ref), kind, cfg, record fields, batch): accepted and refused calls of each of the ten functions.
    The refusals are those of the common rules; the kinds a function does not accept at all are its own business and are pinned where
    the function was introduced (test_controlnet_cpu, test_ipadapter_cpu, test_lcm_cpu, test_upscaler_cpu, test_vae_fused_attention_cpu)."""
    U, T, D, A = E.UNET, E.TEMB, E.VAE_DECODER, E.ADAPTER
    c16, c8 = sd14(16), sd14(8)
    out = []

    def add(name, call, kind, cfg, fields, batch=2):
        out.append(pytest.param(call, kind, cfg, fields, batch, id=f'{name}-{len(out)}'))

    for kind, batch in ((U, 2), (T, 2), (E.TEXT_ENCODER, 1), (D, 1), (E.VAE_ENCODER, 1), (E.UPSCALER, 1), (A, 1), (U, 0), (U, 65), (99, 1)):
        add('create', lambda lib, h, k=kind, b=batch: lib.sdod_graph_create(h, k, ref(c16), b), kind, c16, {}, batch)
    add('create', lambda lib, h: lib.sdod_graph_create(h, U, ref(sd14(16, num_heads=7)), 2), U, sd14(16, num_heads=7), {})
    for kind, ad, batch in ((U, (2, 0, 0), 2), (U, (1, 0, 0), 3), (A, (0, 3, 0), 1), (A, (0, 1, 4), 1), (T, (0, 3, 0), 2), (U, (3, 0, 0), 2),
                            (U, (2, 0, 0), 3), (A, (0, 2, 0), 1), (A, (0, 3, 9), 1), (U, None, 2)):
        a = None if ad is None else E.AdapterConfig(*ad)
        fields = {} if ad is None else dict(zip(('adapter_reps', 'adapter_hint_channels', 'adapter_res_blocks'), ad))
        add('ex', lambda lib, h, k=kind, a=a, b=batch: lib.sdod_graph_create_ex(h, k, ref(c16), ref(a), b), kind, c16, fields, batch)
    for kind, cfg, reps, wrap, batch in ((U, c16, 0, 3, 2), (U, c16, 2, 1, 2), (D, c8, 0, 2, 1), (U, c16, 0, 0, 2), (E.TEXT_ENCODER, c16, 0, 1, 1),
                                         (E.VAE_ENCODER, c8, 0, 1, 1), (U, c16, 0, 4, 2), (U, c16, 0, -1, 2), (U, sd14(16, concat_channels=5), 0, 1, 2)):
        a = E.AdapterConfig(reps, 0, 0)
        add('wrap', lambda lib, h, k=kind, c=cfg, a=a, w=wrap, b=batch: lib.sdod_graph_create_wrap(h, k, ref(c), ref(a), w, b), kind, cfg,
            dict(adapter_reps=reps, wrap=wrap), batch)
    for u in ((1, 16, 16), (2, 8, 24), (0, 8, 8), (24, 8, 8), (1, 4, 8), (1, 8, 1032)):
        uc = E.UpscalerConfig(*u)
        add('upscaler', lambda lib, h, uc=uc: lib.sdod_graph_create_upscaler(h, ref(uc), 1), E.UPSCALER, None, dict(zip(('num_blocks', 'in_h', 'in_w'), u)), 1)
    for kind, cc, cfg, batch in ((U, (1, 0), c16, 2), (T, (0, 1), c16, 2), (E.CONTROLNET, None, c16, 2), (E.CONTROLNET, (0, 0), c16, 4),
                                 (E.CONTROL_HINT, None, c16, 1), (U, None, c16, 2), (E.CONTROLNET, None, c16, 3), (D, (1, 0), c8, 1), (U, (0, 1), c16, 2),
                                 (U, (2, 0), c16, 2), (E.CONTROLNET, None, sd14(16, weight_quant=1), 2), (T, (0, 1), sd14(16, concat_channels=5), 2)):
        c = None if cc is None else E.ControlConfig(*cc)
        fields = {} if cc is None else dict(control_inputs=cc[0], control_temb=cc[1])
        add('control', lambda lib, h, k=kind, f=cfg, c=c, b=batch: lib.sdod_graph_create_control(h, k, ref(f), ref(c), b), kind, cfg, fields, batch)
    for kind, d, cfg in ((T, 256, c16), (T, 16, c16), (T, None, c16), (T, 0, c16), (T, 24, c16), (T, 4112, c16), (T, -16, c16), (U, 256, c16),
                         (T, 80, sd14(16, weight_quant=1)), (T, 128, sd14(16, weight_quant=1))):
        lc = None if d is None else E.LcmConfig(d)
        add('lcm', lambda lib, h, k=kind, f=cfg, lc=lc: lib.sdod_graph_create_lcm(h, k, ref(f), ref(lc), 2), kind, cfg, dict(time_cond_proj_dim=d or 0))
    for kind, wrap, fused, cfg in ((D, 0, 1, c8), (D, 3, 1, c8), (D, 1, None, c8), (E.VAE_ENCODER, 0, 1, c8), (E.VAE_ENCODER_MASKED, 0, 0, c8),
                                   (E.VAE_ENCODER, 1, 1, c8), (D, 0, 2, c8), (D, 0, 1, sd14(8, vae_channels=256)), (D, 4, 0, c8)):
        vc = None if fused is None else E.VaeConfig(fused)
        add('vae', lambda lib, h, k=kind, f=cfg, w=wrap, vc=vc: lib.sdod_graph_create_vae(h, k, ref(f), w, ref(vc), 1), kind, cfg,
            dict(wrap=wrap, fused_attn=fused or 0), 1)
    for r, cfg in ((2, sd14(16, context_len=154)), (3, sd14(16, context_len=231)), (4, sd14(16, context_len=308)), (2, c16), (5, sd14(16, context_len=385)),
                   (1, c16), (2, sd14(16, context_len=154, weight_quant=1)), (2, sd14(16, context_len=154, concat_channels=5))):
        rc = E.RegionConfig(r)
        add('regions', lambda lib, h, f=cfg, rc=rc: lib.sdod_graph_create_regions(h, U, ref(f), ref(rc), 2), U, cfg, dict(regions=r))
    for kind, t, cfg in ((U, 4, c16), (U, 16, c16), (U, None, c16), (T, 0, c16), (U, 17, c16), (U, -1, c16), (U, 4, sd14(16, weight_quant=1)),
                         (U, 4, sd14(16, concat_channels=5)), (U, 4, sd14(16, context_len=154)), (U, 4, sd14(16, context_len=80))):
        ic = None if t is None else E.IpConfig(t)
        add('ip', lambda lib, h, k=kind, f=cfg, ic=ic: lib.sdod_graph_create_ip(h, k, ref(f), ref(ic), 2), kind, cfg, dict(ip_tokens=t or 0))
    for kind, v, t, cfg in ((E.IMAGE_ENCODER, SMALL_VISION, None, None), (E.IMAGE_ENCODER, SMALL_VISION, 4, c16), (E.IMAGE_PROJ, SMALL_VISION, 4, c16),
                            (E.IMAGE_PROJ, (0, 0, 0, 0, 0, 0, 64, 0), 16, c16), (E.IMAGE_ENCODER, (28, 14, 128, 2, 3, 256, 64, 1), None, None),
                            (E.IMAGE_ENCODER, (30, 14, 128, 2, 2, 256, 64, 1), None, None), (E.IMAGE_ENCODER, (28, 14, 128, 2, 2, 256, 96, 1), None, None),
                            (E.IMAGE_PROJ, SMALL_VISION, 0, c16), (E.IMAGE_PROJ, SMALL_VISION, 17, c16)):
        vc, ic = E.VisionConfig(*v), None if t is None else E.IpConfig(t)
        fields = dict(zip(VISION_FIELDS, v), ip_tokens=t if kind == E.IMAGE_PROJ else 0)     # (the encoder's ip argument is not read)
        add('vision', lambda lib, h, k=kind, f=cfg, vc=vc, ic=ic: lib.sdod_graph_create_vision(h, k, ref(f), ref(vc), ref(ic), 2), kind, cfg, fields)
    return out


@pytest.mark.parametrize('call,kind,cfg,fields,batch', wrapper_cases())
def test_wrapper_is_a_translation(call, kind, cfg, fields, batch):
    lib = E._engine()
    h = ctypes.c_void_p()
    rc_w = call(lib, ctypes.byref(h))
    rc_o, g, _ = create_opts(lib, kind, cfg, options(**fields), batch)
    try:
        assert rc_w == rc_o and rc_w in (0, INVALID_ARGUMENT) and bool(h.value) == bool(g.value) == (rc_w == 0)
        if rc_w == 0:
            assert lib.sdod_graph_num_params(h) == lib.sdod_graph_num_params(g) > 0 and param_table(lib, h) == param_table(lib, g)
    finally:
        lib.sdod_graph_destroy(h)
        lib.sdod_graph_destroy(g)


def test_wrapper_cases_cover_all_ten_both_ways():
    lib = E._engine()
    seen = {}
    for p in wrapper_cases():
        call, kind, cfg, fields, batch = p.values
        h = ctypes.c_void_p()
        seen.setdefault(p.id.split('-')[0], set()).add(call(lib, ctypes.byref(h)) == 0)
        lib.sdod_graph_destroy(h)
    assert seen == {n: {True, False} for n in ('create', 'ex', 'wrap', 'upscaler', 'control', 'lcm', 'vae', 'regions', 'ip', 'vision')}


# ------------------------------------------------------------------ the exclusion matrix
# group -> {kind on which the group is valid on its own: its fields there}, the first kind being one on which it builds alone
ALL_KINDS = (E.UNET, E.VAE_DECODER, E.TEXT_ENCODER, E.TEMB, E.VAE_ENCODER, E.VAE_ENCODER_MASKED, E.UPSCALER, E.CONTROLNET, E.CONTROL_HINT,
             E.IMAGE_ENCODER, E.IMAGE_PROJ)
VISION = dict(zip(VISION_FIELDS, SMALL_VISION))
GROUPS = {
    'adapter': {**{k: dict(adapter_reps=2) for k in ALL_KINDS}, E.ADAPTER: dict(adapter_hint_channels=3)},   # (ignored where it is not read)
    'wrap': {E.UNET: dict(wrap=1), E.VAE_DECODER: dict(wrap=1)},
    'upscaler': {E.UPSCALER: dict(num_blocks=1, in_h=16, in_w=16)},
    'control': {E.UNET: dict(control_inputs=1), E.TEMB: dict(control_temb=1), E.CONTROLNET: {}, E.CONTROL_HINT: {}},
    'time_cond_proj_dim': {E.TEMB: dict(time_cond_proj_dim=256)},
    'fused_attn': {k: dict(fused_attn=1) for k in (E.VAE_DECODER, E.VAE_ENCODER, E.VAE_ENCODER_MASKED)},
    'regions': {E.UNET: dict(regions=2)},
    'ip_tokens': {E.UNET: dict(ip_tokens=4), E.IMAGE_PROJ: dict(ip_tokens=4)},
    'vision': {E.IMAGE_ENCODER: VISION, E.IMAGE_PROJ: VISION},
}
ALLOWED = {frozenset(('adapter', 'wrap')): E.UNET, frozenset(('wrap', 'fused_attn')): E.VAE_DECODER, frozenset(('ip_tokens', 'vision')): E.IMAGE_PROJ}


def config_for(fields):
    return sd14(16, context_len=77 * fields['regions']) if fields.get('regions') else sd14(16)


@pytest.mark.parametrize('name', list(GROUPS))
def test_each_option_builds_alone(name):
    kind, fields = next(iter(GROUPS[name].items()))
    lib = E._engine()
    rc, h, msg = create_opts(lib, kind, config_for(fields), options(**fields), 2)
    assert rc == 0 and h.value, msg
    lib.sdod_graph_destroy(h)


@pytest.mark.parametrize('a,b', list(itertools.combinations(GROUPS, 2)))
def test_exclusion_matrix(a, b):
    common = [k for k in GROUPS[a] if k in GROUPS[b]]
    kind = common[0] if common else E.UNET
    pick = lambda g: GROUPS[g].get(kind) if kind in GROUPS[g] else next(iter(GROUPS[g].values()))    # noqa: E731
    fields = {**pick(a), **pick(b)}
    lib = E._engine()
    rc, h, msg = create_opts(lib, kind, config_for(fields), options(**fields), 2)
    if frozenset((a, b)) in ALLOWED:
        assert kind == ALLOWED[frozenset((a, b))] and rc == 0 and h.value, msg
        lib.sdod_graph_destroy(h)
    else:
        assert rc == INVALID_ARGUMENT and not h.value
        m = re.search(r'the options (\w+) and (\w+) exclude each other', msg)
        assert m and set(m.groups()) == {a, b}, msg


def test_matrix_is_36_pairs_with_three_allowed():
    pairs = list(itertools.combinations(GROUPS, 2))
    assert len(GROUPS) == 9 and len(pairs) == 36 and sum(frozenset(p) in ALLOWED for p in pairs) == 3 == len(ALLOWED)


# ------------------------------------------------------------------ edge cases
def test_size_field_null_arguments_and_plain_equivalence():
    lib = E._engine()
    cfg = sd14(16)
    for size in (0, 4, ctypes.sizeof(E.GraphOptions) - 4, ctypes.sizeof(E.GraphOptions) + 4, -1):
        rc, h, msg = create_opts(lib, E.UNET, cfg, E.GraphOptions(size=size), 2)
        assert rc == INVALID_ARGUMENT and not h.value and 'size' in msg
    assert lib.sdod_graph_create_opts(None, E.UNET, ctypes.byref(cfg), ctypes.byref(options()), 2) == INVALID_ARGUMENT
    for kind in (E.UNET, E.TEMB, E.IMAGE_PROJ, E.CONTROLNET):                          # a model configuration is needed ...
        rc, h, _ = create_opts(lib, kind, None, options(**(dict(VISION, ip_tokens=4) if kind == E.IMAGE_PROJ else {})), 2)
        assert rc == INVALID_ARGUMENT and not h.value
    tables = {}
    for kind, fields in ((E.UPSCALER, GROUPS['upscaler'][E.UPSCALER]), (E.IMAGE_ENCODER, VISION)):   # ... except where no field of it is read
        for c in (None, E.sd14_config()):
            rc, h, msg = create_opts(lib, kind, c, options(**fields), 1)
            assert rc == 0, msg
            tables.setdefault(kind, []).append(param_table(lib, h))
            lib.sdod_graph_destroy(h)
    assert all(a == b and a for a, b in tables.values())
    for kind, batch in ((E.UNET, 2), (E.TEMB, 2), (E.TEXT_ENCODER, 1), (E.VAE_DECODER, 1), (E.VAE_ENCODER, 1), (E.VAE_ENCODER_MASKED, 1)):
        plain = ctypes.c_void_p()
        assert lib.sdod_graph_create(ctypes.byref(plain), kind, ctypes.byref(cfg), batch) == 0
        for opts in (None, options()):                                                # null options = all zero = sdod_graph_create
            rc, h, msg = create_opts(lib, kind, cfg, opts, batch)
            assert rc == 0 and param_table(lib, h) == param_table(lib, plain), msg
            lib.sdod_graph_destroy(h)
        lib.sdod_graph_destroy(plain)
    for kind in (E.UPSCALER, E.ADAPTER, E.IMAGE_ENCODER, E.IMAGE_PROJ):                # the kinds that need an option refuse its absence
        rc, h, _ = create_opts(lib, kind, cfg, None, 1)
        assert rc == INVALID_ARGUMENT and not h.value


def test_python_graph_fills_the_record():
    """what the classes of sdod.amd.engine build through the record is what the older functions build"""
    lib = E._engine()
    cfg = sd14(16, context_len=154)
    cfg.regions = 2
    h = ctypes.c_void_p()
    assert lib.sdod_graph_create_regions(ctypes.byref(h), E.UNET, ctypes.byref(cfg), ctypes.byref(E.RegionConfig(2)), 2) == 0
    assert E.UNet(cfg, 2).param_table() == param_table(lib, h)
    lib.sdod_graph_destroy(h)
    c = sd14(16)
    assert E.UNet(c, 2, wrap=None).param_table() == E.UNet(c, 2, wrap=0).param_table() == E.UNet(c, 2, wrap=3).param_table()
    assert set(E.Temb(c, 2, cond_proj_dim=256).param_table()) - set(E.Temb(c, 2).param_table()) == {('time_embed.cond_proj.weight', (320, 256))}
    side = E.copy_config(c)
    for n, v in (('adapter_reps', 2), ('tiling', 3), ('control_inputs', 1), ('control_temb', 1), ('regions', 2), ('ip_tokens', 4), ('freeu', 1),
                 ('hypertile', (8, 1))):
        assert getattr(c, n) == E.ModelConfig._SIDE[n] and not getattr(c, n)
        setattr(side, n, v)
    again = E.copy_config(side)
    assert all(getattr(again, n) == getattr(side, n) for n in E.ModelConfig._SIDE) and set(E.ModelConfig._SIDE) >= {
        'adapter_reps', 'adapter_hint_channels', 'adapter_res_blocks', 'tiling', 'control_inputs', 'control_temb', 'regions', 'ip_tokens', 'freeu', 'hypertile'}
    assert all(not getattr(E.copy_config(c), n) for n in E.ModelConfig._SIDE)
