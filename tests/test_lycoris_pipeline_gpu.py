"""Txt2Img(loras=True) with a LyCORIS file: one .safetensors with LoHa modules on the attention weights, LoKr modules (full diffs among
them) on the convolutions and plain LoRA on the text encoder, handed to set_loras (16x16 latent, synthetic weights), against the oracle
loop on lycoris.merged_state_dict weights; the graphed trajectory with the file set; clear_loras().

Tolerances are tests/test_lora_pipeline_gpu.py's: context rel-L2 <= 5e-3, final latent of 20 PLMS steps rel-L2 <= 2e-2, uint8 image within
2 LSB on >= 99 % of the pixels.  The adapter: alpha 2 at LoHa rank 4 and strength 0.8 (scale 0.4) on factors whose Hadamard product has
0.125 of the weight's spread -- the 0.05 of tests/test_lycoris_engine_gpu.py; the LoKr modules hold both sides in full, so their scale
is the strength alone and w2 carries 0.0625 of the weight's spread; the text modules are those of the LoRA pipeline test."""
import numpy as np
import pytest
import torch

import lora_cases as LC
import lycoris_cases as C

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
    shapes = dict(tables['unet'])
    targets = LC.unet_targets(tables['unet'])
    convs = [n for n in targets if len(shapes[n]) == 4]
    attn = [n for n in targets if len(shapes[n]) == 2]
    assert len(convs) > 50 and len(attn) > 100
    # entries carry scale 1: the file route derives strength * alpha / rank itself; the factors hold the rest of the size
    loha = [(k, n, a1, (b1.float() * 0.125 ** 0.5).half(), a2, (b2.float() * 0.125 ** 0.5).half(), s)
            for k, n, a1, b1, a2, b2, s in C.make_loha_entries(sds['unet'], attn, RANK, 1.0, seed=5)]
    lokr = [(k, n, w1, (w2.float() * 0.0625).half(), s) for k, n, w1, w2, s in C.make_lokr_entries(sds['unet'], convs, 1.0, seed=6)]
    ent_t = LC.make_entries(sds['text'], LC.text_targets(tables['text'], (0, 11)), RANK, 1.0, seed=7)
    ent_t = [(n, up, (down.float() * 0.25).half(), s) for n, up, down, s in ent_t]
    path = str(tmp_path_factory.mktemp('lycoris') / 'adapter.safetensors')
    save_file(C.file_dict(loha + lokr + ent_t, ALPHA), path)
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=16, loras=True)
    return pipe, sds, path


def test_a_mixed_file_is_read_as_three_kinds(rig):
    from sdod.amd import lora, lycoris as L
    pipe, sds, path = rig
    ent, skipped = L.entries_for(path, 'sd14', STRENGTH, STRENGTH)
    kinds = ['lora' if len(e) == 4 else e[0] for e in ent['unet']]
    assert skipped == [] and kinds.count('loha') > 100 and kinds.count('lokr') > 50 and kinds.count('lora') == 0
    assert len(ent['text']) == 12 and all(len(e) == 4 for e in ent['text'])
    assert any(e.raw['family'] == 'full' for e in ent['unet'])
    assert {e[-1] for e in ent['unet'] if e[0] == 'loha'} == {STRENGTH * ALPHA / RANK}
    assert {e[-1] for e in ent['unet'] if e[0] == 'lokr'} == {STRENGTH}                  # both sides in full: alpha is not used
    with pytest.raises(ValueError, match='not a plain LoRA module'):                  # the plain reader still refuses the file
        lora.entries_for(path, 'sd14', STRENGTH, STRENGTH)


def test_file_route_matches_the_oracle_on_merged_weights(rig):
    from oracle import pipeline_oracle as PO, sd_torch as S
    from sdod.amd import lycoris as L
    pipe, sds, path = rig
    ent, _ = L.entries_for(path, 'sd14', STRENGTH, STRENGTH)
    assert pipe.set_loras([(path, STRENGTH)]) == []
    try:
        with torch.device('meta'):
            unet, vae, clip = S.UNetModel(), S.AutoencoderKLDecode(), S.ClipTextModel()
        merged_unet = L.merged_state_dict(sds['unet'], ent['unet'])
        unet.load_state_dict({**merged_unet, **sds['temb']}, assign=True)
        clip.load_state_dict(L.merged_state_dict(sds['text'], ent['text']), assign=True)
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
        print(f'lycoris file route: context rel-L2 {rc:.3e}, plms final latent rel-L2 {r:.3e}')
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


def test_graphed_equals_eager_with_the_file_and_clear_restores_the_image(rig):
    pipe, sds, path = rig
    ids_u, ids_c = _ids()
    x_T = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(7))
    kw = dict(steps=4, guidance=7.5, sampler='plms')
    ctx_base = pipe.encode_tokens(ids_u, ids_c)
    before = pipe.generate(ctx_base, x_T, **kw).clone()
    assert torch.equal(pipe.generate_graphed(ctx_base, x_T, **kw), before)         # the trajectory is captured BEFORE set_loras
    pipe.set_loras([(path, STRENGTH, 0.5)])
    ctx_net = pipe.encode_tokens(ids_u, ids_c)                                      # the text encoder changed: encode again
    assert not torch.equal(ctx_net, ctx_base)
    eager = pipe.generate(ctx_net, x_T, **kw).clone()
    assert not torch.equal(eager, before)
    assert torch.equal(pipe.generate_graphed(ctx_net, x_T, **kw), eager)           # ... and replayed after it
    pipe.clear_loras()
    assert torch.equal(pipe.encode_tokens(ids_u, ids_c), ctx_base)
    assert torch.equal(pipe.generate(ctx_base, x_T, **kw), before)
    assert torch.equal(pipe.generate_graphed(ctx_base, x_T, **kw), before)
    pipe.unet.check()


def test_refused_modules_and_a_mix_of_files(rig):
    pipe, sds, path = rig
    k = 'lora_unet_mid_block_attentions_0_proj_in'
    dora = {f'{k}.lora_up.weight': torch.zeros(1280, 4), f'{k}.lora_down.weight': torch.zeros(4, 1280), f'{k}.dora_scale': torch.zeros(1, 1280)}
    lokr = {f'{k}.lokr_w1': torch.zeros(3, 4), f'{k}.lokr_w2': torch.zeros(427, 320)}         # 3 x 427 = 1281 rows
    with pytest.raises(ValueError, match='dora_scale'):
        pipe.set_loras([(dora, 1.0)])
    with pytest.raises(ValueError, match='do not divide'):
        pipe.set_loras([(lokr, 1.0)])
    assert pipe.set_loras([(dora, 1.0), (lokr, 1.0)], strict=False) == [k, k]
    # a plain LoRA dict next to the LyCORIS file in one list
    plain = {f'{k}.lora_up.weight': torch.full((1280, 4), 0.01), f'{k}.lora_down.weight': torch.full((4, 1280), 0.01)}
    assert pipe.set_loras([(path, STRENGTH), (plain, 1.0)]) == []
    pipe.clear_loras()
