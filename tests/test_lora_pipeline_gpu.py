"""Txt2Img(loras=True): a kohya-named LoRA file handed to the pipeline (16x16 latent, synthetic weights) against the oracle loop on
lora.merged_state_dict weights, the graphed trajectory with an adapter set, and clear_loras().

Tolerances are test_plms_20_steps_matches_oracle's: final latent rel-L2 <= 2e-2, uint8 image within 2 LSB on >= 99 % of the pixels.
The adapter: rank 4, alpha 2, on every supported UNet weight and six matrices of two text-encoder layers, applied at strength 0.8 (scale
0.8 * 2 / 4 = 0.4 of factors sized 0.125 / 0.25 of the weights' spread: the 0.05 / 0.1 of tests/test_lora_engine_gpu.py)."""
import numpy as np
import pytest
import torch

import lora_cases as C

pytestmark = pytest.mark.gpu

RANK, ALPHA, STRENGTH = 4, 2.0, 0.8


def rel_l2(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _ids():
    ids_u = np.full(77, 49407, np.int64); ids_u[0] = 49406
    ids_c = ids_u.copy(); ids_c[1:9] = [320, 1125, 539, 550, 18376, 6765, 320, 4558]
    return ids_u, ids_c


@pytest.fixture(scope='module')
def rig(tmp_path_factory):
    from safetensors.torch import save_file
    from sdod.amd import engine as E, weights as Wt
    from sdod.amd.pipeline import Txt2Img
    cfg = E.sd14_config(16, 16)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'text': E.TextEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    # entries carry scale 1: the file route derives strength * alpha / rank itself; the factors hold the rest of the size
    ent_u = C.make_entries(sds['unet'], C.unet_targets(tables['unet']), RANK, 1.0, seed=5)
    ent_t = C.make_entries(sds['text'], C.text_targets(tables['text'], (0, 11)), RANK, 1.0, seed=7)
    ent_u = [(n, up, (down.float() * 0.125).half(), s) for n, up, down, s in ent_u]
    ent_t = [(n, up, (down.float() * 0.25).half(), s) for n, up, down, s in ent_t]
    path = str(tmp_path_factory.mktemp('lora') / 'adapter.safetensors')
    save_file(C.kohya_state_dict(ent_u + ent_t, ALPHA), path)
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, loras=True)
    return pipe, sds, path, ent_u, ent_t


def test_file_route_matches_the_oracle_on_merged_weights(rig):
    from oracle import pipeline_oracle as PO, sd_torch as S
    from sdod.amd import lora as L
    pipe, sds, path, ent_u, ent_t = rig
    scale = STRENGTH * ALPHA / RANK
    assert pipe.set_loras([(path, STRENGTH)]) == []
    try:
        with torch.device('meta'):
            unet, vae, clip = S.UNetModel(), S.AutoencoderKLDecode(), S.ClipTextModel()
        unet.load_state_dict({**L.merged_state_dict(sds['unet'], [(n, u, d, scale) for n, u, d, _ in ent_u]), **sds['temb']}, assign=True)
        clip.load_state_dict(L.merged_state_dict(sds['text'], [(n, u, d, scale) for n, u, d, _ in ent_t]), assign=True)
        vae.load_state_dict(sds['vae'], assign=True)
        ids_u, ids_c = _ids()
        ctx2 = pipe.encode_tokens(ids_u, ids_c)
        with torch.no_grad():
            ref_ctx = clip.eval()(torch.from_numpy(np.stack([ids_u, ids_c])))
        rc = rel_l2(ctx2.float().cpu(), ref_ctx)
        x_T = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(42))
        tr_gpu, tr_cpu = [], []
        z = pipe.sample_plms(ctx2, x_T, steps=20, guidance=7.5, trace=tr_gpu)
        c16 = ctx2.float().cpu()                      # the oracle consumes the SAME fp16 context the GPU used
        z_ref = PO.plms_sample(unet.eval(), c16[0:1], c16[1:2], x_T, steps=20, scale=7.5, trace=tr_cpu)
        assert tr_gpu == tr_cpu
        r = rel_l2(z.cpu(), z_ref)
        print(f'lora file route: context rel-L2 {rc:.3e}, plms final latent rel-L2 {r:.3e}')
        assert rc <= 5e-3, rc
        assert torch.isfinite(z).all() and r <= 2e-2, r
        img = pipe.decode(z, mode=1).cpu().numpy()
        img_ref = PO.decode_u8(vae.eval(), z_ref, mode=1)
        diff = np.abs(img.astype(np.int32) - img_ref.astype(np.int32))
        frac = float((diff <= 2).mean())
        print('uint8 image: max diff', int(diff.max()), 'within 2 LSB', frac)
        assert img.shape == (1, 128, 128, 3) and frac >= 0.99, frac
    finally:
        pipe.clear_loras()


def test_graphed_equals_eager_with_a_lora_and_clear_restores_the_image(rig):
    pipe, sds, path, ent_u, ent_t = rig
    ids_u, ids_c = _ids()
    x_T = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(7))
    kw = dict(steps=4, guidance=7.5, sampler='plms')
    ctx_base = pipe.encode_tokens(ids_u, ids_c)
    before = pipe.generate(ctx_base, x_T, **kw).clone()
    assert torch.equal(pipe.generate_graphed(ctx_base, x_T, **kw), before)         # the trajectory is captured BEFORE set_loras
    pipe.set_loras([(path, STRENGTH, 0.5)])
    ctx_lora = pipe.encode_tokens(ids_u, ids_c)                                     # the text encoder changed: encode again
    assert not torch.equal(ctx_lora, ctx_base)
    eager = pipe.generate(ctx_lora, x_T, **kw).clone()
    assert not torch.equal(eager, before)
    assert torch.equal(pipe.generate_graphed(ctx_lora, x_T, **kw), eager)          # ... and replayed after it
    kw2 = dict(steps=4, guidance=7.5, sampler='euler')
    assert torch.equal(pipe.generate_graphed(ctx_lora, x_T, **kw2), pipe.generate(ctx_lora, x_T, **kw2))   # captured with the adapter set
    pipe.clear_loras()
    assert torch.equal(pipe.encode_tokens(ids_u, ids_c), ctx_base)
    assert torch.equal(pipe.generate(ctx_base, x_T, **kw), before)
    assert torch.equal(pipe.generate_graphed(ctx_base, x_T, **kw), before)
    assert torch.equal(pipe.generate_graphed(ctx_base, x_T, **kw2), pipe.generate(ctx_base, x_T, **kw2))
    pipe.unet.check()


def test_not_built_with_the_flag(rig):
    from sdod.amd.pipeline import Txt2Img
    pipe, sds, path, _, _ = rig
    plain = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16)
    assert plain.unet.base_bytes() == 0 and plain.text.base_bytes() == 0
    assert plain.unet.stats() == pipe.unet.stats() and plain.text.stats() == pipe.text.stats()
    assert [o[0] for o in plain.unet.op_table()] == [o[0] for o in pipe.unet.op_table()]
    assert pipe.unet.base_bytes() == pipe.unet.stats()['weight_bytes'] and pipe.text.base_bytes() == pipe.text.stats()['weight_bytes']
    with pytest.raises(RuntimeError, match='loras=True'):
        plain.set_loras([(path, 0.8)])
    with pytest.raises(RuntimeError, match='loras=True'):
        plain.clear_loras()
    with pytest.raises(ValueError):
        pipe.set_loras([({'lora_unet_conv_in.lora_down.weight': torch.zeros(4, 4, 3, 3), 'lora_unet_conv_in.lora_up.weight': torch.zeros(320, 4, 1, 1)}, 1.0)])
    assert pipe.set_loras([({'lora_unet_conv_in.lora_down.weight': torch.zeros(4, 4, 3, 3), 'lora_unet_conv_in.lora_up.weight': torch.zeros(320, 4, 1, 1)}, 1.0)],
                          strict=False) == ['lora_unet_conv_in']
    pipe.clear_loras()
