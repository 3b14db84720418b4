"""LCM few-step sampling, the parts that need no GPU: the host tables (LcmSchedule, guidance_embedding) against the restatements of
tests/lcm_ref.py, the refusals of sdod_lcm_step and of the TEMB graph's guidance embedding on the host, the build-argument and
entry-point contracts, and the LoRA time modules' name mapping."""
import ctypes

import numpy as np
import pytest
import torch

import lcm_ref as R


# ---------------------------------------------------------------------------------------------------------------- host tables
@pytest.mark.parametrize('steps,strength', list(R.TIMESTEPS))
def test_timesteps(steps, strength):
    from sdod.amd.samplers import LcmSchedule
    sch = LcmSchedule(steps, strength=strength)
    assert sch.timesteps.tolist() == R.TIMESTEPS[(steps, strength)] == R.timesteps(steps, 50, strength)
    assert sch.steps == steps and np.array_equal(sch.alphas_cumprod, R.alphas_cumprod())


def test_timesteps_at_other_grids():
    from sdod.amd.samplers import LcmSchedule
    for steps, original, strength in ((3, 50, 1.0), (7, 50, 0.9), (50, 50, 1.0), (5, 100, 0.33), (6, 20, 0.75), (1, 1, 1.0)):
        assert LcmSchedule(steps, original, strength).timesteps.tolist() == R.timesteps(steps, original, strength)


@pytest.mark.parametrize('kw', [dict(steps=0), dict(steps=-1), dict(steps=51), dict(steps=26, strength=0.5), dict(steps=1, strength=0.01),
                                dict(strength=0.0), dict(strength=-0.5), dict(strength=1.5), dict(strength=float('nan')), dict(steps=True),
                                dict(steps=2.5), dict(original_steps=0), dict(original_steps=1001), dict(strength='full')])
def test_schedule_refuses(kw):
    from sdod.amd.samplers import LcmSchedule
    with pytest.raises(ValueError):
        LcmSchedule(**kw)


@pytest.mark.parametrize('v_prediction', [False, True])
@pytest.mark.parametrize('steps,strength', [(1, 1.0), (2, 1.0), (4, 1.0), (8, 1.0), (4, 0.5)])
def test_coef_is_the_published_step(steps, strength, v_prediction):
    """random scalars through the linear form with coef()'s floats against the published step, float64: 1e-12 relative"""
    from sdod.amd.samplers import LcmSchedule
    sch = LcmSchedule(steps, strength=strength)
    rng = np.random.default_rng(steps * 10 + int(v_prediction))
    for i in range(steps):
        cf = sch.coef(i, v_prediction)
        assert all(isinstance(v, float) for v in cf.values()) and set(cf) == {'d0', 'd1', 'a', 'b', 'u'}
        x, e, nu = rng.standard_normal(64) * 3, rng.standard_normal(64), rng.standard_normal(64)
        den = cf['d0'] * x + cf['d1'] * e
        got = cf['a'] * x + cf['b'] * den + cf['u'] * nu
        last = i == steps - 1
        t, t_next = int(sch.timesteps[i]), None if last else int(sch.timesteps[i + 1])
        want, x0 = R.published_step(x, e, t, t_next, nu, v_prediction)
        assert np.allclose(den, x0, rtol=1e-12, atol=0)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(x).max())
        assert (cf['u'] == 0.0) == last
        if last:         # the last step returns the consistency function's value
            c_skip, c_out = sch.scalings(i)
            assert cf['a'] == c_skip and cf['b'] == c_out
    with pytest.raises(ValueError):
        sch.coef(steps)
    with pytest.raises(ValueError):
        sch.coef(-1)


def test_start_coefficients():
    from sdod.amd.samplers import LcmSchedule
    ac = R.alphas_cumprod()
    for strength, t0 in ((1.0, 999), (0.5, 499), (0.3, 299)):
        a, b = LcmSchedule(4, strength=strength).start()
        assert (a, b) == (float(np.sqrt(ac[t0])), float(np.sqrt(1.0 - ac[t0]))) and abs(a * a + b * b - 1.0) < 1e-15


def test_guidance_embedding():
    from sdod.amd.samplers import guidance_embedding
    e = guidance_embedding(1.0)
    assert e.shape == (1, 256) and e.dtype == np.float64
    assert np.array_equal(e[0, :128], np.zeros(128)) and np.array_equal(e[0, 128:], np.ones(128))       # exactly [0 .. 0 | 1 .. 1]
    w = np.array([1.5, 8.0, 15.0])
    for dim in (256, 32):
        e = guidance_embedding(w, dim)
        assert np.allclose(e, R.guidance_features(torch.from_numpy(w), dim).numpy(), rtol=0, atol=1e-11)
        assert np.allclose(e[:, :dim // 2] ** 2 + e[:, dim // 2:] ** 2, 1.0, atol=1e-14)
        # the first frequency is 1, the last 1e-4: sine first, divisor dim/2 - 1
        assert np.allclose(e[:, 0], np.sin((w - 1) * 1000)) and np.allclose(e[:, dim // 2 - 1], np.sin((w - 1) * 0.1), atol=1e-12)
    for bad in (0, 2, 7):
        with pytest.raises(ValueError):
            guidance_embedding(1.0, bad)


# ---------------------------------------------------------------------------------------------------------------- sdod_lcm_step on the host
def test_symbols_are_bound():
    from sdod.amd import _lib, engine as E
    lib = _lib.hip()
    for s in ('sdod_lcm_step', 'sdod_guidance_features_f16'):
        assert s in _lib.HIP_SYMBOLS and getattr(lib, s).argtypes is not None
    E._engine()
    assert 'sdod_graph_create_lcm' in E.ENGINE_SYMBOLS and lib.sdod_graph_create_lcm.argtypes is not None
    hip_h = open(__file__.replace('tests/test_lcm_cpu.py', 'include/sdod_hip.h')).read()
    assert 'sdod_lcm_step(' in hip_h and 'sdod_guidance_features_f16(' in hip_h
    # the struct is the header's: 7 pointers, 2 x u64, 10 ints, 6 floats
    assert ctypes.sizeof(_lib.LcmStepArgs) == 7 * 8 + 2 * 8 + 10 * 4 + 6 * 4
    assert ctypes.sizeof(_lib.KStepArgs) == 7 * 8 + 2 * 8 + 9 * 4 + 8 * 4 + 4       # (sdod_k_step_args is untouched; 4: tail padding)


@pytest.mark.parametrize('label,over', R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_lcm_step_refuses_before_any_launch(label, over):
    """sdod_lcm_step checks its arguments on the host before it touches the device: every refusal comes back as INVALID_ARGUMENT (2)
    on a machine without one, with addresses nobody reads"""
    from sdod.amd import _lib
    lib = _lib.hip()
    fake = {p: 0x10000 * (i + 1) for i, p in enumerate(R.POINTERS)}
    a = R.fill_args(fake, over, temb=(520, 4))
    assert lib.sdod_lcm_step(ctypes.byref(a), None) == 2, label
    assert lib.sdod_hip_last_error()


def test_guidance_features_refuses_on_the_host():
    from sdod.amd import _lib
    lib = _lib.hip()
    for w, y, n, dim in ((None, 0x10000, 1, 256), (0x10000, None, 1, 256), (0x10000, 0x20000, 0, 256), (0x10000, 0x20000, 1, 2),
                         (0x10000, 0x20000, 1, 33), (0x10000, 0x20000, 1, 0), (0x10000, 0x20000, 1, -4)):
        assert lib.sdod_guidance_features_f16(w, y, n, dim, None) == 2


# ---------------------------------------------------------------------------------------------------------------- the TEMB graph's table
def test_temb_graph_declares_cond_proj():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    plain = E.Temb(cfg, 2).param_table()
    assert E.Temb(cfg, 2, cond_proj_dim=0).param_table() == plain and not [n for n, _ in plain if 'cond_proj' in n]
    for dim in (256, 32, 16, 320):
        table = E.Temb(cfg, 2, cond_proj_dim=dim).param_table()
        assert [e for e in table if e not in plain] == [('time_embed.cond_proj.weight', (320, dim))] and len(table) == len(plain) + 1
    assert dict(E.Temb(E.sd21_config(24, 24), 1, cond_proj_dim=256).param_table())['time_embed.cond_proj.weight'] == (320, 256)
    for bad in (8, 24, -16, 250, 4112):
        with pytest.raises(Exception, match='time_cond_proj_dim'):
            E.Temb(cfg, 2, cond_proj_dim=bad)
    ccfg = E.copy_config(cfg); ccfg.control_temb = 1
    with pytest.raises(ValueError, match='control_temb'):
        E.Temb(ccfg, 2, cond_proj_dim=256)
    with pytest.raises(ValueError, match='TEMB'):
        E.Graph(E.UNET, cfg, 2, cond_proj_dim=256)
    # the C entry point on its own: other kinds refuse the width, NULL and 0 build the plain graph
    lib = E._engine()
    h = ctypes.c_void_p()
    assert lib.sdod_graph_create_lcm(ctypes.byref(h), E.UNET, ctypes.byref(cfg), ctypes.byref(E.LcmConfig(256)), 2) == 2 and not h.value
    assert lib.sdod_graph_create_lcm(ctypes.byref(h), E.CONTROLNET, ctypes.byref(cfg), None, 2) == 2 and not h.value
    for lcm in (None, ctypes.byref(E.LcmConfig(0))):
        assert lib.sdod_graph_create_lcm(ctypes.byref(h), E.TEMB, ctypes.byref(cfg), lcm, 2) == 0
        assert lib.sdod_graph_num_params(h) == len(plain)
        lib.sdod_graph_destroy(h)


def test_converter_writes_cond_proj(tmp_path):
    from sdod.amd import convert as C, engine as E, weights as Wt
    cfg = E.sd14_config(16, 16)
    tables = C.parameter_tables(cfg)
    sd = {}
    for i, graph in enumerate(tables):
        for k, v in Wt.synthetic_state_dict(tables[graph], seed=50 + i).items():
            sd[C.GRAPHS[graph][0] + k] = v
    cond = torch.randn(320, 256, generator=torch.Generator().manual_seed(1))
    ckpt = str(tmp_path / 'lcm.ckpt')
    torch.save(dict(sd, **{'time_embedding.cond_proj.weight': cond}), ckpt)            # the one key under its diffusers name
    C.convert(ckpt, str(tmp_path / 'with'), cfg=cfg, guidance_embed=True)
    C.convert(ckpt, str(tmp_path / 'without'), cfg=cfg)
    got = Wt.load(str(tmp_path / 'with' / 'temb.sdodw'))
    assert torch.equal(got['time_embed.cond_proj.weight'].float(), cond.half().float())
    assert set(got) - set(Wt.load(str(tmp_path / 'without' / 'temb.sdodw'))) == {'time_embed.cond_proj.weight'}
    torch.save(sd, ckpt)
    with pytest.raises(KeyError, match='cond_proj'):
        C.convert(ckpt, str(tmp_path / 'missing'), cfg=cfg, guidance_embed=True)


# ---------------------------------------------------------------------------------------------------------------- contracts
@pytest.mark.parametrize('kw,why', [
    (dict(cfg_split=True), 'cfg_split'), (dict(inpaint_unet=True), 'inpaint_unet'), (dict(hires_hw=(24, 32)), 'hires_hw'),
    (dict(adapter=True), 'adapter'), (dict(controlnet=True), 'controlnet'), (dict(regions=2), 'regions'),
    (dict(ip_adapter=True), 'ip_adapter'), (dict(canvas_hw=(16, 32)), 'canvas_hw'),
])
def test_constructor_refuses_what_needs_the_pair(kw, why):
    from sdod.amd.pipeline import Txt2Img
    with pytest.raises(ValueError, match=f'unguided cannot be combined with {why}: '):
        Txt2Img(state_dicts=None, latent_hw=16, unguided=True, **kw)


def test_constructor_refuses_the_dependent_arguments():
    from sdod.amd.pipeline import Txt2Img, lcm_check_build
    with pytest.raises(ValueError, match='guidance_embed needs unguided'):
        Txt2Img(state_dicts=None, latent_hw=16, guidance_embed=True)
    with pytest.raises(ValueError, match='lora_time_modules needs loras'):
        Txt2Img(state_dicts=None, latent_hw=16, lora_time_modules=True)
    for name in ('unguided', 'guidance_embed', 'lora_time_modules'):
        with pytest.raises(ValueError, match=f'{name} must be True or False'):
            Txt2Img(state_dicts=None, latent_hw=16, loras=True, **{name: 1})
    off = dict(cfg_split=False, inpaint_unet=False, hires_hw=None, adapter=False, controlnet=False, regions=False, ip_adapter=False, canvas_hw=None)
    assert lcm_check_build(True, True, True, True, **off) is None
    assert lcm_check_build(False, False, False, False, **dict(off, cfg_split=True, hires_hw=(24, 24), regions=2)) is None     # off: nobody's business
    assert lcm_check_build(True, False, False, False, **off) is None


def bare(n=1, unguided=False, guidance_embed=False, encoder=None):
    """a Txt2Img without its constructor: what the argument checks read"""
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    p = Txt2Img.__new__(Txt2Img)
    p.cfg, p.n, p.device, p.unguided, p.guidance_embed, p.encoder = E.sd14_config(16, 16), n, torch.device('cpu'), unguided, guidance_embed, encoder
    return p


@pytest.mark.parametrize('entry', ['sample_lcm', 'generate_lcm', 'generate_lcm_graphed'])
def test_entry_points_refuse_bad_arguments_before_any_device_work(entry):
    ctx2 = torch.zeros(2, 77, 768, dtype=torch.float16)
    x = torch.zeros(1, 4, 16, 16)
    run = getattr(bare(), entry)
    for steps in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='steps must be a positive integer'):
            run(ctx2, x, steps)
    with pytest.raises(ValueError, match='steps = 51 is more than'):
        run(ctx2, x, 51)
    with pytest.raises(ValueError, match='original_steps must be'):
        run(ctx2, x, 4, original_steps=0)
    for strength in (0.0, 1.01, float('nan'), 'half'):
        with pytest.raises(ValueError, match='strength must be in'):
            run(ctx2, x, 4, strength=strength)
    for bad_x in (torch.zeros(2, 4, 16, 16), torch.zeros(1, 4, 16, 24), None):
        with pytest.raises(ValueError, match='x must be a tensor'):
            run(ctx2, bad_x, 4)
    for sn in (torch.zeros(4, 1, 4, 16, 16), torch.zeros(3, 1, 4, 16, 16, dtype=torch.float64), torch.zeros(3, 2, 4, 16, 16)):
        with pytest.raises(ValueError, match='step_noise must be a float32 tensor'):
            run(ctx2, x, 4, step_noise=sn)
    for g in (float('nan'), float('inf'), 'high', True):
        with pytest.raises(ValueError, match='guidance must be a finite number'):
            run(ctx2, x, 4, g)
    with pytest.raises(ValueError, match='guidance must be None'):
        getattr(bare(unguided=True), entry)(ctx2, x, 4, 8.0)
    with pytest.raises(ValueError, match='guidance is the scale w'):
        getattr(bare(unguided=True, guidance_embed=True), entry)(ctx2, x, 4)


def test_check_args_returns_the_scales():
    from sdod.amd.pipeline import lcm_check_args
    x = torch.zeros(2, 4, 16, 16)
    assert lcm_check_args(bare(2), x, 4, None, 50, 1.0, None) == (1.0, None)
    assert lcm_check_args(bare(2), x, 4, 1.5, 50, 1.0, torch.zeros(3, 2, 4, 16, 16)) == (1.5, None)
    assert lcm_check_args(bare(2, unguided=True), x, 1, None, 50, 0.5, None) == (None, None)
    assert lcm_check_args(bare(2, unguided=True, guidance_embed=True), x, 8, 8, 50, 1.0, None) == (None, 8.0)
    assert lcm_check_args(bare(2), None, 4, None, 50, 0.5, None, shape=(2, 4, 16, 16)) == (1.0, None)
    with pytest.raises(ValueError, match='at a time'):
        lcm_check_args(bare(2), None, 4, None, 50, 0.5, None, shape=(1, 4, 16, 16))


def test_img2img_lcm_needs_the_encoder_and_checks_first():
    ctx2 = torch.zeros(2, 77, 768, dtype=torch.float16)
    u8 = torch.zeros(1, 128, 128, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='with_vae_encoder'):
        bare().img2img_lcm(ctx2, u8)
    p = bare(encoder=object())
    with pytest.raises(ValueError, match='steps = 4 is more than'):
        p.img2img_lcm(ctx2, u8, strength=0.05)
    with pytest.raises(ValueError, match='at a time'):
        p.img2img_lcm(ctx2, torch.zeros(2, 128, 128, 3, dtype=torch.uint8))


ENTRY_CALLS = {
    'generate': 2, 'generate_graphed': 2, 'generate_pipelined': 2, 'generate_upscaled': 2, 'generate_upscaled_graphed': 2, 'sample_plms': 2,
    'sample_dpm': 2, 'sample_k': 3, 'sample_ddim_from': 3, 'img2img': 2, 'img2img_graphed': 2, 'inpaint': 3, 'inpaint_graphed': 3,
    'sample_ddim_inpaint': 5, 'inpaint_concat': 4, 'inpaint_concat_graphed': 4, 'generate_hires': 2, 'generate_hires_graphed': 2,
    'hires_from_latent': 2, 'sample_panorama': 2, 'generate_panorama': 2, 'generate_panorama_graphed': 2,
}


@pytest.mark.parametrize('entry', list(ENTRY_CALLS))
def test_the_pair_entry_points_refuse_an_unguided_pipeline(entry):
    """every entry point from before reads (uncond, cond) pairs: on an unguided pipeline it raises, naming the LCM ones, before it
    looks at an argument"""
    p = bare(unguided=True)
    with pytest.raises(ValueError, match='unguided=True.*sample_lcm / generate_lcm / generate_lcm_graphed / img2img_lcm'):
        getattr(p, entry)(*[None] * ENTRY_CALLS[entry], **(dict(hires_steps=4, hires_seed=1) if entry == 'hires_from_latent' else {}))
    with pytest.raises(ValueError, match='unguided=True'):
        p._set_context(torch.zeros(2, 77, 768))


# ---------------------------------------------------------------------------------------------------------------- LoRA time modules
def _time_file():
    g = torch.Generator().manual_seed(3)

    def mod(out, inp, rank=4):
        return {'lora_down.weight': torch.randn(rank, inp, generator=g), 'lora_up.weight': torch.randn(out, rank, generator=g),
                'alpha': torch.tensor(2.0)}
    mods = {'lora_unet_down_blocks_1_resnets_0_time_emb_proj': mod(640, 1280), 'lora_unet_mid_block_resnets_1_time_emb_proj': mod(1280, 1280),
            'lora_unet_up_blocks_3_resnets_2_time_emb_proj': mod(320, 1280), 'lora_unet_time_embedding_linear_1': mod(1280, 320),
            'lora_unet_time_embedding_linear_2': mod(1280, 1280),
            'lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q': mod(320, 320)}
    return {f'{m}.{k}': v for m, d in mods.items() for k, v in d.items()}


def test_time_modules_map_to_the_temb_graph():
    from sdod.amd import engine as E, lora, lycoris as L
    table = dict(E.Temb(E.sd14_config(16, 16), 1).param_table())
    want = {'lora_unet_down_blocks_1_resnets_0_time_emb_proj': 'input_blocks.4.0.emb_layers.1.weight',
            'lora_unet_mid_block_resnets_1_time_emb_proj': 'middle_block.2.emb_layers.1.weight',
            'lora_unet_up_blocks_3_resnets_2_time_emb_proj': 'output_blocks.11.0.emb_layers.1.weight',
            'lora_unet_time_embedding_linear_1': 'time_embed.0.weight', 'lora_unet_time_embedding_linear_2': 'time_embed.2.weight'}
    for module, name in want.items():
        assert lora.map_key(module, time_modules=True) == ('temb', name) and name in table
        with pytest.raises(ValueError, match='not a target'):        # without the keyword, and with it off: refused as ever
            lora.map_key(module)
        with pytest.raises(ValueError, match='not a target'):
            lora.map_key(module, 'sd14', False)
    # all 22 ResBlocks have a name in the table
    keys = [f'down_blocks_{i}_resnets_{j}' for i in range(4) for j in range(2)] + [f'mid_block_resnets_{j}' for j in range(2)] + \
        [f'up_blocks_{i}_resnets_{j}' for i in range(4) for j in range(3)]
    names = {lora.map_key(f'lora_unet_{k}_time_emb_proj', time_modules=True)[1] for k in keys}
    assert len(names) == 22 and names == {n for n in table if n.endswith('emb_layers.1.weight')}
    for bad in ('lora_unet_down_blocks_4_resnets_0_time_emb_proj', 'lora_unet_mid_block_resnets_2_time_emb_proj',
                'lora_unet_time_embedding_linear_3', 'lora_unet_conv_in'):
        with pytest.raises(ValueError):
            lora.map_key(bad, time_modules=True)
    assert lora.map_key('lora_unet_mid_block_attentions_0_proj_in', time_modules=True) == lora.map_key('lora_unet_mid_block_attentions_0_proj_in')
    f = _time_file()
    for entries_for in (L.entries_for, lora.entries_for):
        ent, skipped = entries_for(f, 'sd14', 0.5, 1.0, time_modules=True)
        assert skipped == [] and set(ent) == {'unet', 'text', 'temb'} and len(ent['unet']) == 1 and ent['text'] == []
        assert sorted(e[0] for e in ent['temb']) == sorted(want.values())
        assert all(e[3] == 0.5 * 2.0 / 4 for e in ent['temb'])                      # the UNet's strength x alpha / rank
        with pytest.raises(ValueError, match='time_emb_proj is not a target'):
            entries_for(f, 'sd14', 0.5, 1.0)
        ent, skipped = entries_for(f, 'sd14', 0.5, 1.0, strict=False)
        assert sorted(skipped) == sorted(want) and set(ent) == {'unet', 'text'} and len(ent['unet']) == 1
    # and the host merge takes the 'temb' entries on a TEMB state dict
    from sdod.amd import weights as Wt
    sd = Wt.synthetic_state_dict(E.Temb(E.sd14_config(16, 16), 1).param_table(), seed=5)
    ent, _ = L.entries_for(f, 'sd14', 0.5, 1.0, time_modules=True)
    merged = L.merged_state_dict(sd, ent['temb'])
    changed = {k for k in sd if not torch.equal(merged[k], sd[k])}
    assert changed == set(want.values())


def test_set_loras_without_the_switch_refuses_time_modules():
    """a pipeline built without lora_time_modules goes through entries_for exactly as before"""
    from sdod.amd import engine as E
    from sdod.amd.pipeline import Txt2Img
    p = Txt2Img.__new__(Txt2Img)
    p._loras, p.cfg, p.model = True, E.sd14_config(16, 16), 'sd14'
    p.unet, p.text = E.UNet(p.cfg, 2), None
    with pytest.raises(ValueError, match='time_emb_proj is not a target'):
        p.set_loras([(_time_file(), 1.0)])
