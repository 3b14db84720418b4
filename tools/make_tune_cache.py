#!/usr/bin/env python3
"""Regenerate the shipped GEMM tile table (stable-diffusion-on-device_amd/tune/gfx950.tune) on an MI355X.

Builds every graph of the configurations the benches and the GPU tests use with the shipped table ignored
(SDOD_TUNE_DEFAULT=0) and SDOD_TUNE_CACHE pointing at a fresh file, so every distinct GEMM shape is timed cold-cache once
(engine.hip: emit_gemm) and its pick appended.  Copy the result over tune/gfx950.tune and commit it: from then on
every process builds the same launch lists without timing anything.

usage (GPU box):  python tools/make_tune_cache.py gpurun_out/gfx950.tune [--quick | --only-quant | --only-rows3 | --only-ln | --only-new]
                  python tools/make_tune_cache.py out/gfx950_regions.tune --only-regions    (-> tune/gfx950_regions.tune)
                  python tools/make_tune_cache.py out/gfx950_ip.tune --only-ip              (-> tune/gfx950_ip.tune)
NEVER run under a profiler (timing noise would be baked into the picks)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

out = os.path.abspath(sys.argv[1])
quick = '--quick' in sys.argv
only_quant = '--only-quant' in sys.argv   # keep the shipped picks of every fp16 shape, re-time the uint8-weight shapes only
only_rows3 = '--only-rows3' in sys.argv   # re-time only the 3x3 stride-1 convolutions on images whose rows are multiples of 3 (config 5)
only_ln = '--only-ln' in sys.argv         # keep every shipped pick but those of the LayerNorm-folded Linears (key flag bit 30): re-time those
only_n160 = '--only-n160' in sys.argv     # re-time the fp16 rows-mode shapes whose N is a multiple of 160 (candidates for the 160-wide tiles 56..58)
only_geglu = '--only-geglu' in sys.argv   # re-time the LayerNorm-folded GEGLU projections (key flags: bit 1 and bit 30)
only_softmax = '--only-softmax' in sys.argv # re-time the score GEMMs of the folded cross-attention (key flag bit 28)
only_tail = '--only-tail' in sys.argv     # re-time the 3x3 convolutions with a fused 1x1 skip (key flags: tc0 in bits 2..13)
only_new = '--only-new' in sys.argv       # keep EVERY shipped pick, time only the shapes the table does not have yet (a new fusion's GEMMs)
only_vae_enc = '--only-vae-encoder' in sys.argv  # keep EVERY shipped pick, time the VAE encoder's new shapes (img2img; key flag bit 26 = pad_mode)
only_rect = '--only-rect' in sys.argv      # keep EVERY shipped pick, time the sd14 shapes at 64 x 96, 96 x 64 and 96 x 96 (rectangular sizes, the hires pass)
only_regions = '--only-regions' in sys.argv  # keep EVERY pick of gfx950.tune and gfx950_control.tune, time the regional-prompt UNets' new shapes, write ONLY those
only_ip = '--only-ip' in sys.argv          # keep EVERY pick of the three shipped tables, time the new shapes of image prompts, write ONLY those
only_new = only_new or only_vae_enc or only_rect or only_regions or only_ip
if os.path.exists(out):
    os.remove(out)
os.makedirs(os.path.dirname(out), exist_ok=True)
if only_quant or only_rows3 or only_ln or only_new or only_n160 or only_geglu or only_softmax or only_tail:
    shipped = os.path.join(ROOT, 'stable-diffusion-on-device_amd', 'tune', 'gfx950.tune')
    with open(shipped) as f, open(out, 'w') as g:
        for line in f:
            v = line.split()
            if len(v) not in (13, 15):
                continue
            # key fields (engine.hip: key_of): 0 a_mode, 6 stride, 8 ksize, 9 h_in, 10 flags (bit 29 = uint8 weights, bit 30 = LayerNorm fold)
            if only_new:
                drop = False
            elif only_tail:
                drop = v[0] == '1' and ((int(v[10]) >> 2) & 4095) != 0 and not (int(v[10]) & (1 << 29))
            elif only_softmax:
                drop = int(v[10]) & (1 << 28)
            elif only_geglu:
                drop = (int(v[10]) & 2) and (int(v[10]) & (1 << 30))
            elif only_n160:
                drop = v[0] == '0' and int(v[2]) % 160 == 0 and not (int(v[10]) & ((1 << 29) | (1 << 28) | 2))   # (not uint8, not the score GEMMs, not GEGLU: those have their own switches)
            elif only_ln:
                drop = int(v[10]) & (1 << 30)
            else:
                drop = (int(v[10]) & (1 << 29)) if only_quant else (v[0] == '1' and v[6] == '1' and v[8] == '3' and int(v[9]) % 3 == 0)
            if not drop:
                g.write(line)
    if only_regions or only_ip:   # the later tables' picks too: the output is what NONE of them holds
        for suffix in ('_control.tune',) + (('_regions.tune',) if only_ip else ()):
            with open(shipped.replace('.tune', suffix)) as f, open(out, 'a') as g:
                g.writelines(line for line in f if len(line.split()) == 15)
        with open(out) as f:
            known = set(f.read().splitlines())
os.environ['SDOD_TUNE_CACHE'] = out
os.environ['SDOD_TUNE_DEFAULT'] = '0'

import torch  # noqa: E402
from sdod.amd import engine as E, weights as Wt  # noqa: E402

T0 = time.time()


def build(cls, cfg, batch, seed, label, quant=False):
    g = cls(cfg, batch)
    sd = Wt.synthetic_state_dict(g.param_table(), seed=seed)
    g.load_state_dict(Wt.quantize_state_dict(sd) if quant else sd)
    g.finalize()
    torch.cuda.synchronize()
    n = sum(1 for _ in open(out)) if os.path.exists(out) else 0
    print(f'[{time.time() - T0:6.1f}s] {label}: {g.stats()["launches"]} launches; table now {n} shapes', flush=True)
    del g


def vae_encoders():
    # img2img: 512 px (batch 1 and 2), 768 px, and the reduced size the GPU tests run
    for hw, b in ((64, 1), (64, 2), (96, 1), (16, 1)):
        build(E.VaeEncoder, E.sd14_config(hw, hw), b, 1238, f'vae encoder {hw}x{hw} b{b}')


if only_vae_enc:
    vae_encoders()
    print(f'done: {out}')
    sys.exit(0)

if only_regions:
    # the sizes tests/test_regions_gpu.py and tools/regions_bench.py build: 16 x 16, 8 x 16 and 64 x 64 at batch 2, 2 and 3 regions; the
    # text encoder at batch 2 k (Txt2Img(regions=k).encode_regions)
    for h, w in ((16, 16), (8, 16), (64, 64)):
        for k in (2, 3):
            c = E.sd14_config(h, w)
            c.context_len, c.regions = 77 * k, k
            build(E.UNet, c, 2, 1234, f'sd14 unet {h}x{w} b2, {k} regions')
    for k in (2, 3):
        build(E.TextEncoder, E.sd14_config(16, 16), 2 * k, 1237, f'clip-L b{2 * k}')
    with open(out) as f:
        new = [line for line in f.read().splitlines() if line not in known]
    with open(out, 'w') as f:
        f.write(''.join(line + '\n' for line in new))
    print(f'done: {out} ({len(new)} new shapes)')
    sys.exit(0)

if only_ip:
    # the sizes tests/test_ipadapter_gpu.py and tools/ipadapter_bench.py build: UNets with 4 and 16 image tokens at 16 x 16 and 8 x 16
    # (batch 2; batch 4 for two images per GPU), 64 x 64 with 4; the image projection and the image encoders, ViT-H/14 included
    def ip_unet(h, w, t, b):
        c = E.sd14_config(h, w)
        c.ip_tokens = t
        build(E.UNet, c, b, 1234, f'sd14 unet {h}x{w} b{b}, {t} image tokens')
    for h, w in ((16, 16), (8, 16)):
        for t in (4, 16):
            ip_unet(h, w, t, 2)
    ip_unet(16, 16, 4, 4)
    ip_unet(64, 64, 4, 2)
    c16 = E.sd14_config(16, 16)
    for proj, t, b in ((128, 4, 2), (128, 16, 2), (128, 4, 4), (1024, 4, 2)):
        build(lambda cfg, batch: E.ImageProj(cfg, proj, t, batch), c16, b, 1240, f'image projection {proj} -> {t} tokens b{b}')
    for v, b in (((28, 14, 320, 2, 4, 1280, 128, 0), 1), ((28, 14, 320, 2, 4, 1280, 128, 0), 2), ((56, 14, 128, 2, 2, 512, 64, 1), 2)):
        g = E.ImageEncoder(E.VisionConfig(*v), b)
        g.load_state_dict(Wt.synthetic_state_dict(g.checkpoint_table(), seed=1241)); g.finalize()
        print(f'[{time.time() - T0:6.1f}s] image encoder {v} b{b}: {g.stats()["launches"]} launches', flush=True)
        del g
    g = E.ImageEncoder(E.vit_h14_config(), 1)
    g.load_state_dict(Wt.synthetic_state_dict(g.checkpoint_table(), seed=1242, dtype=torch.float16)); g.finalize()
    print(f'[{time.time() - T0:6.1f}s] image encoder ViT-H/14 b1: {g.stats()["launches"]} launches', flush=True)
    del g
    with open(out) as f:
        new = [line for line in f.read().splitlines() if line not in known]
    with open(out, 'w') as f:
        f.write(''.join(line + '\n' for line in new))
    print(f'done: {out} ({len(new)} new shapes)')
    sys.exit(0)

if only_rect:
    for h, w in ((64, 96), (96, 64), (96, 96)):
        c = E.sd14_config(h, w)
        build(E.UNet, c, 2, 1234, f'sd14 unet {h}x{w} b2')
        build(E.VaeDecoder, c, 1, 1236, f'sd14 vae {h}x{w}')
    print(f'done: {out}')
    sys.exit(0)

if only_quant:
    for hw in (96, 24):
        cq = E.sd21_config(hw, hw)
        cq.weight_quant = 1
        build(E.UNet, cq, 2, 2100, f'sd21 unet {hw}x{hw} b2, uint8 weights', quant=True)
        build(E.Temb, cq, 1, 2101, 'sd21 temb b1, uint8 weights', quant=True)
        build(E.Temb, cq, 20, 2101, 'sd21 temb b20, uint8 weights', quant=True)
    print(f'done: {out}')
    sys.exit(0)

if only_ln:
    c64 = E.sd14_config(64, 64)
    for b in (2, 4, 1):
        build(E.UNet, c64, b, 1234, f'sd14 unet 64x64 b{b}')
    build(E.UNet, E.sd21_config(96, 96), 2, 2100, 'sd21 unet 96x96 b2')
    c16 = E.sd14_config(16, 16)
    for b in (2, 4, 1):
        build(E.UNet, c16, b, 1234, f'sd14 unet 16x16 b{b}')
    build(E.UNet, E.sd21_config(24, 24), 2, 2100, 'sd21 unet 24x24 b2')
    print(f'done: {out}')
    sys.exit(0)

if only_rows3:
    c96 = E.sd21_config(96, 96)
    build(E.UNet, c96, 2, 2100, 'sd21 unet 96x96 b2')
    for hw in (96, 24):
        cq = E.sd21_config(hw, hw)
        cq.weight_quant = 1
        build(E.UNet, cq, 2, 2100, f'sd21 unet {hw}x{hw} b2, uint8 weights', quant=True)
    build(E.VaeDecoder, c96, 1, 1236, 'vae 96x96')
    build(E.UNet, E.sd21_config(24, 24), 2, 2100, 'sd21 unet 24x24 b2')
    print(f'done: {out}')
    sys.exit(0)

# headline (configs 2/3), config 4's per-rank share (batch 4), latency mode (batch 1)
c64 = E.sd14_config(64, 64)
for b in (2, 4, 1):
    build(E.UNet, c64, b, 1234, f'sd14 unet 64x64 b{b}')
build(E.VaeDecoder, c64, 1, 1236, 'sd14 vae 64x64')
build(E.TextEncoder, c64, 2, 1237, 'clip-L b2')
build(E.TextEncoder, c64, 1, 1237, 'clip-L b1')
for b in (1, 2, 4):
    build(E.Temb, c64, b, 1235, f'temb b{b}')
build(E.Temb, c64, 20, 1235, 'temb b20')
build(E.Temb, c64, 50, 1235, 'temb b50')
if not quick:
    # config 5 (SD v2.1-768) and the reduced sizes the GPU tests run
    c96 = E.sd21_config(96, 96)
    build(E.UNet, c96, 2, 2100, 'sd21 unet 96x96 b2')
    for hw in (96, 24):      # config 5 with the weights kept uint8 in HBM (sdod_model_config.weight_quant)
        cq = E.sd21_config(hw, hw)
        cq.weight_quant = 1
        build(E.UNet, cq, 2, 2100, f'sd21 unet {hw}x{hw} b2, uint8 weights', quant=True)
        build(E.Temb, cq, 1, 2101, f'sd21 temb b1, uint8 weights', quant=True)
        build(E.Temb, cq, 20, 2101, f'sd21 temb b20, uint8 weights', quant=True)
    build(E.VaeDecoder, c96, 1, 1236, 'vae 96x96')
    build(E.TextEncoder, c96, 2, 2102, 'openclip-H b2')
    build(E.Temb, c96, 1, 2101, 'sd21 temb b1')
    build(E.Temb, c96, 20, 2101, 'sd21 temb b20')
    c16 = E.sd14_config(16, 16)
    for b in (2, 4, 1):
        build(E.UNet, c16, b, 1234, f'sd14 unet 16x16 b{b}')
    build(E.VaeDecoder, c16, 1, 1236, 'vae 16x16')
    c24 = E.sd21_config(24, 24)
    build(E.UNet, c24, 2, 2100, 'sd21 unet 24x24 b2')
    vae_encoders()
print(f'done: {out}')
