#!/usr/bin/env python3
"""The hires pass and the rectangular graphs on one MI355X (synthetic weights, SD v1.4 shapes, batch 1), ms per image:

  * generate_hires_graphed 64 x 64 -> 96 x 96 (512 px -> 768 px), 20 + 20 steps, denoise 0.5 (10 second-pass evaluations),
    dpmpp_2m on the Karras schedule, bilinear latent resize;
  * generate_graphed at 64 x 64 and at 64 x 96 (512 x 768 px), 20 steps of the same sampler;
  * where each UNet's GEMM tiles came from (Graph.tune_source: shipped table / timed in this process), its launches and bytes.

Not the benchmark (bench.py measures the flagship txt2img workload); the record behind INTEGRATION.md's "Image sizes and the hires
pass".  No threshold is attached to it.

usage (GPU box):  python tools/hires_bench.py [--iters 5] [--out profiles/hires_bench.json]"""
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


def unet_info(g):
    st = g.stats()
    return {'tune': g.tune_source(), 'launches': st['launches'], 'weight_bytes': st['weight_bytes'], 'arena_bytes': st['arena_bytes']}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--denoise', type=float, default=0.5)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    kw = dict(steps=a.steps, guidance=7.5, sampler='dpmpp_2m', schedule='karras')

    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, hires_hw=(96, 96), with_text_encoder=False)
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    hires_ms = timed(lambda: pipe.generate_hires_graphed(ctx2, x_T, hires_steps=a.steps, denoise=a.denoise, upscaler='bilinear', seed=1, **kw),
                     a.iters)
    base_ms = timed(lambda: pipe.generate_graphed(ctx2, x_T, **kw), a.iters)
    hi = pipe.hires
    extra = {k: sum(gr.stats()[k] for gr in (hi.unet, hi.vae)) for k in ('weight_bytes', 'arena_bytes')}
    info = {'unet_64x64': unet_info(pipe.unet), 'unet_96x96': unet_info(hi.unet)}
    del pipe, hi
    torch.cuda.empty_cache()

    rect = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=(64, 96), with_text_encoder=False)
    x_R = torch.randn(1, 4, 64, 96, generator=g).cuda()
    rect_ms = timed(lambda: rect.generate_graphed(ctx2, x_R, **kw), a.iters)
    info['unet_64x96'] = unet_info(rect.unet)

    res = {
        'device': torch.cuda.get_device_name(0),
        'sampler': 'dpmpp_2m', 'schedule': 'karras', 'iters': a.iters,
        'generate_hires_graphed_64x64_to_96x96': {'steps': a.steps, 'hires_steps': a.steps, 'denoise': a.denoise,
                                                  'unet_evals': [a.steps, int(a.denoise * a.steps)], 'ms_per_image': round(hires_ms, 2)},
        'generate_graphed_64x64': {'steps': a.steps, 'ms_per_image': round(base_ms, 2)},
        'generate_graphed_64x96': {'steps': a.steps, 'ms_per_image': round(rect_ms, 2)},
        'hires_extra_device_bytes': extra,
        'unets': info,
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
