#!/usr/bin/env python3
"""The k-diffusion samplers on one MI355X next to PLMS on the same box, one process (synthetic weights, SD v1.4 shapes, 512 px, batch 1,
20 steps, guidance 7.5): ms per image of Txt2Img.generate_graphed -- input copies, euler_a's Philox fills of the graph's step-noise
input, one graph replay (context upload, every UNet evaluation and fused step, VAE decode, uint8) -- for 'plms' and for 'euler',
'euler_a', 'dpmpp_2m' on both schedules ('discrete', 'karras').

20-step PLMS makes 21 UNet evaluations (its first step is two), a 20-step k-sampler 20, and each of them one fused launch per step
behind the UNet, so a k-sampler should not take longer than PLMS in the same run.  Each graphed result is checked against the eager
call bit for bit first.

Every figure is the median of --iters (>= 20) single calls, each between two device events, after warm-up; the variants alternate
inside one loop so that they meet the same machine.  Not the benchmark (bench.py measures the flagship txt2img workload); a tool for
DESIGN.md's k-sampler paragraph.

usage (GPU box):  python tools/ksampler_bench.py [--iters 30] [--out profiles/ksampler_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402
from sdod.amd.samplers import K_SAMPLERS, K_SCHEDULES  # noqa: E402


def _summary(v):
    v = sorted(v)
    return {'ms_per_image': round(statistics.median(v), 3), 'min': round(v[0], 3), 'p90': round(v[int(0.9 * (len(v) - 1))], 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    if a.iters < 20:
        ap.error('--iters must be at least 20 (the figures are medians)')
    if not torch.cuda.is_available():
        sys.exit('ksampler_bench.py needs a GPU: nothing is measured without one')
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    st, gd, seed = a.steps, 7.5, 1

    calls = {'plms': dict(sampler='plms')}
    for sampler in K_SAMPLERS:
        for schedule in K_SCHEDULES:
            calls[f'{sampler}_{schedule}'] = dict(sampler=sampler, schedule=schedule, seed=seed)
    equal = {}
    for name, kw in calls.items():
        eager = pipe.generate(ctx2, x_T, st, gd, **kw)
        equal[name] = bool(torch.equal(pipe.generate_graphed(ctx2, x_T, st, gd, **kw), eager))
    variants = {name: (lambda kw=kw: pipe.generate_graphed(ctx2, x_T, st, gd, **kw)) for name, kw in calls.items()}
    times = {k: [] for k in variants}
    for it in range(a.warmup + a.iters):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))

    res = {'device': torch.cuda.get_device_name(0), 'steps': st, 'guidance': gd, 'image': '512x512', 'iters': a.iters,
           'unet_evals': {'plms': st + 1, 'k_samplers': st}, 'graphed_equals_eager_bit_for_bit': equal}
    res.update({k: _summary(v) for k, v in times.items()})
    # each k-sampler against PLMS, iteration by iteration (the calls of one iteration run back to back): k - plms
    res['minus_plms_ms'] = {}
    for name in calls:
        if name != 'plms':
            d = sorted(k - p for k, p in zip(times[name], times['plms']))
            res['minus_plms_ms'][name] = {'median': round(statistics.median(d), 3), 'p90': round(d[int(0.9 * (len(d) - 1))], 3),
                                          'not_slower_in': sum(1 for v in d if v <= 0), 'of': len(d)}
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
