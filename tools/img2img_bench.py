#!/usr/bin/env python3
"""img2img on one MI355X, next to txt2img on the same box (synthetic weights, SD v1.4 shapes, 512 px, batch 1):

  * the VAE encoder graph alone: ms per encode (one hipGraph replay), launches, and TFLOP/s from the launch list's FLOPs;
  * img2img images/s at strength 0.75, 20 DDIM steps (15 guided UNet evaluations), Txt2Img.img2img_graphed;
  * txt2img images/s at 20 PLMS steps (21 guided UNet evaluations), Txt2Img.generate_graphed.

Not the benchmark (bench.py measures the flagship txt2img workload); a tool for DESIGN.md's img2img paragraph.

usage (GPU box):  python tools/img2img_bench.py [--iters 10] [--out profiles/img2img_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402


def timed(fn, iters):
    """ms per call: one warm-up, then `iters` back-to-back calls between two events"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--strength', type=float, default=0.75)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, with_vae_encoder=True)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    u8 = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()

    enc = pipe.encoder
    enc.img.copy_(u8)
    st = enc.stats()
    enc_ms = timed(lambda: enc.execute(use_hip_graph=True), a.iters)
    t_enc = int(a.strength * a.steps)
    i2i_ms = timed(lambda: pipe.img2img_graphed(ctx2, u8, a.strength, a.steps, 7.5, seed=1), a.iters)
    t2i_ms = timed(lambda: pipe.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms'), a.iters)
    res = {
        'device': torch.cuda.get_device_name(0),
        'vae_encoder_512px': {'ms': round(enc_ms, 3), 'launches': st['launches'], 'gflop': round(st['flops'] / 1e9, 1),
                              'tflops': round(st['flops'] / enc_ms / 1e9, 1)},
        'img2img': {'strength': a.strength, 'steps': a.steps, 'unet_evals': t_enc, 'ms_per_image': round(i2i_ms, 2),
                    'images_per_s': round(1000.0 / i2i_ms, 2)},
        'txt2img_plms': {'steps': a.steps, 'unet_evals': a.steps + 1, 'ms_per_image': round(t2i_ms, 2),
                         'images_per_s': round(1000.0 / t2i_ms, 2)},
        'wall_s': round(time.time() - t0, 1),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
