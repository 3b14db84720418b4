#!/usr/bin/env python3
"""LCM few-step sampling on one MI355X next to 20-step PLMS on the same box, one process (synthetic weights, SD v1.4 shapes, 512 px):
ms per image and images/s of one graph replay -- input copies, the Philox fills of the step-noise input, context upload, every UNet
evaluation and fused step, VAE decode, uint8 -- for
  (a) plms20        Txt2Img.generate_graphed, 'plms', 20 steps, guidance 7.5, batch 1: the path bench.py measures, as the yardstick
  (b) lcm4_guided   generate_lcm_graphed on the same pipeline, 4 steps, CFG 1.5 (the LCM-LoRA form), batch 1
  (c) lcm4_unguided generate_lcm_graphed on Txt2Img(unguided=True, guidance_embed=True), 4 steps, w = 8, batch 1 (one UNet row)
  (d) lcm4_unguided_n2  the same with images_per_gpu = 2 (two UNet rows, two decodes per call; ms per image = ms per call / 2)
and the device time of one ops.lcm_step launch against one ops.k_step launch of the same batch (n = 1, guided, staged, no noise).

Each graphed result is checked against the eager call bit for bit first.  Every figure is the median of --iters (>= 20) single calls,
each between two device events, after warm-up; the variants alternate inside one loop so that they meet the same machine.  Not the
benchmark (bench.py measures the flagship txt2img workload); a tool for DESIGN.md 6p and the README's LCM sentence.

usage (GPU box):  python tools/lcm_bench.py [--iters 30] [--out profiles/lcm_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, ops, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402
from sdod.amd.samplers import KSchedule, LcmSchedule  # noqa: E402


def _summary(v, images=1):
    v = sorted(x / images for x in v)
    med = statistics.median(v)
    return {'ms_per_image': round(med, 3), 'images_per_s': round(1000.0 / med, 2), 'min': round(v[0], 3), 'p90': round(v[int(0.9 * (len(v) - 1))], 3)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    if a.iters < 20:
        ap.error('--iters must be at least 20 (the figures are medians)')
    if not torch.cuda.is_available():
        sys.exit('lcm_bench.py needs a GPU: nothing is measured without one')
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1, cond_proj_dim=256).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    plain = dict(sds, temb={k: v for k, v in sds['temb'].items() if 'cond_proj' not in k})
    pair = Txt2Img(state_dicts=plain, images_per_gpu=1, latent_hw=64, with_text_encoder=False)
    one = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, unguided=True, guidance_embed=True)
    two = Txt2Img(state_dicts=sds, images_per_gpu=2, latent_hw=64, with_text_encoder=False, unguided=True, guidance_embed=True)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x1 = torch.randn(1, 4, 64, 64, generator=g).cuda()
    x2 = torch.randn(2, 4, 64, 64, generator=g).cuda()

    calls = {
        'plms20': (1, lambda graphed: (pair.generate_graphed if graphed else pair.generate)(ctx2, x1, 20, 7.5, 'plms')),
        'lcm4_guided': (1, lambda graphed: (pair.generate_lcm_graphed if graphed else pair.generate_lcm)(ctx2, x1, 4, 1.5, seed=1)),
        'lcm4_unguided': (1, lambda graphed: (one.generate_lcm_graphed if graphed else one.generate_lcm)(ctx2, x1, 4, 8.0, seed=1)),
        'lcm4_unguided_n2': (2, lambda graphed: (two.generate_lcm_graphed if graphed else two.generate_lcm)(ctx2, x2, 4, 8.0, seed=1)),
    }
    equal = {name: bool(torch.equal(fn(True), fn(False))) for name, (_, fn) in calls.items()}
    times = {k: [] for k in calls}
    for it in range(a.warmup + a.iters):
        for name, (_, fn) in calls.items():
            ms = _timed(lambda: fn(True))
            if it >= a.warmup:
                times[name].append(ms)

    # one step launch of each kind behind the same prediction: n = 1, the guidance pair, staged inputs, no noise drawn
    eps = torch.randn(2, 64, 64, 4, generator=g).half().cuda()
    temb_row = torch.randn(pair.unet.temb_width, generator=g).half().cuda()
    stage = (pair.unet.x, temb_row, pair.unet.temb)
    lcf = LcmSchedule(4).coef(3)
    kcf = KSchedule(20).coef('euler', 5)
    xs = x1.clone()
    steps = {'lcm_step': lambda: ops.lcm_step(eps, xs, lcf, 1.5, stage=stage), 'k_step': lambda: ops.k_step(eps, xs, kcf, 1.5, stage=stage)}
    step_us = {k: [] for k in steps}
    for it in range(a.warmup + 10 * a.iters):
        for name, fn in steps.items():
            xs.copy_(x1)            # (outside the event pair: every timed launch updates the same finite latent)
            ms = _timed(fn)
            if it >= a.warmup:
                step_us[name].append(1000.0 * ms)

    res = {'device': torch.cuda.get_device_name(0), 'image': '512x512', 'iters': a.iters,
           'unet_evals': {'plms20': 21, 'lcm4_guided': 4, 'lcm4_unguided': 4, 'lcm4_unguided_n2': 4},
           'unet_rows': {'plms20': 2, 'lcm4_guided': 2, 'lcm4_unguided': 1, 'lcm4_unguided_n2': 2},
           'graphed_equals_eager_bit_for_bit': equal}
    res.update({k: _summary(v, calls[k][0]) for k, v in times.items()})
    res['speedup_over_plms20'] = {k: round(res['plms20']['ms_per_image'] / res[k]['ms_per_image'], 2) for k in calls if k != 'plms20'}
    # (an event pair around one eager launch includes the launch latency: the two figures compare with each other, not with a profiler's)
    res['one_launch_us'] = {k: {'median': round(statistics.median(v), 2), 'min': round(min(v), 2)} for k, v in step_us.items()}
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
