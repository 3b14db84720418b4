#!/usr/bin/env python3
"""MultiDiffusion panoramas on one MI355X (synthetic weights, SD v1.4 shapes, guidance 7.5, dpmpp_2m): a 64 x 256 latent canvas
(512 x 2048 px) of 64 x 64 windows at stride 32 -- 7 windows, 8 with the canvas wrapped in x -- with n = every window in one UNet
evaluation, and with n = 2 (4 chunks).  Per configuration: ms per image of Txt2Img.generate_panorama_graphed (input copies, one graph
replay: every chunk's UNet evaluation and copies, the canvas steps, the canvas decode, uint8) and ms per step.

For comparison, on the same pipeline in the same loop: the ms per step of a plain k-sampler trajectory of n images
(generate_graphed: one UNet evaluation of batch 2n and one sdod_k_step launch per step), times the chunk count.  A panorama step is
`chunks` UNet evaluations of batch 2n and ONE sdod_k_step_windows launch, plus two device copies per chunk when there is more than
one; the difference to chunks x the plain step is what the averaging launch and the chunk copies add.

ms per step is the slope between two trajectory lengths, (T(steps) - T(steps / 2)) / (steps / 2), so the context upload and the decode
drop out.  Every figure is the median of --iters (>= 20) single calls, each between two device events, after warm-up; the variants
alternate inside one loop so that they meet the same machine.  Each graphed result is checked against the eager call bit for bit first.
Not the benchmark (bench.py measures the flagship txt2img workload); a tool for DESIGN.md's panorama paragraph.

usage (GPU box):  python tools/panorama_bench.py [--iters 20] [--configs wrap0_all,wrap1_all,wrap0_n2,wrap1_n2] [--out profiles/panorama_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, panorama as PN, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402

CANVAS, WINDOW, STRIDE = (64, 256), (64, 64), 32
CONFIGS = ('wrap0_all', 'wrap1_all', 'wrap0_n2', 'wrap1_n2')


def _median(v):
    return round(statistics.median(v), 3)


def measure(sds, name, steps, iters, warmup):
    wrap = name.startswith('wrap1')
    oy, ox = PN.plan_windows(CANVAS, WINDOW, STRIDE, wrap)
    windows = len(oy) * len(ox)
    n = windows if name.endswith('_all') else 2
    chunks = -(-windows // n)
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=n, latent_hw=WINDOW, with_text_encoder=False, canvas_hw=CANVAS, canvas_wrap=wrap)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_can = torch.randn(1, 4, *CANVAS, generator=g).cuda()
    x_win = torch.randn(n, 4, *WINDOW, generator=g).cuda()
    half = steps // 2
    kw = dict(sampler='dpmpp_2m', guidance=7.5)
    equal = bool(torch.equal(pipe.generate_panorama_graphed(ctx2, x_can, steps=steps, stride=STRIDE, **kw),
                             pipe.generate_panorama(ctx2, x_can, steps=steps, stride=STRIDE, **kw)))
    variants = {
        'pano': lambda: pipe.generate_panorama_graphed(ctx2, x_can, steps=steps, stride=STRIDE, **kw),
        'pano_half': lambda: pipe.generate_panorama_graphed(ctx2, x_can, steps=half, stride=STRIDE, **kw),
        'plain': lambda: pipe.generate_graphed(ctx2, x_win, steps=steps, **kw),
        'plain_half': lambda: pipe.generate_graphed(ctx2, x_win, steps=half, **kw),
    }
    times = {k: [] for k in variants}
    for it in range(warmup + iters):
        for key, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[key].append(e0.elapsed_time(e1))
    span = steps - half
    pano_step = [(a - b) / span for a, b in zip(times['pano'], times['pano_half'])]
    plain_step = [(a - b) / span for a, b in zip(times['plain'], times['plain_half'])]
    added = [p - chunks * q for p, q in zip(pano_step, plain_step)]
    return {'wrap': wrap, 'windows': windows, 'n': n, 'chunks': chunks, 'graphed_equals_eager_bit_for_bit': equal,
            'ms_per_image': _median(times['pano']), 'ms_per_image_min': round(min(times['pano']), 3), 'ms_per_step': _median(pano_step),
            'plain_k_step_ms_per_step': _median(plain_step), 'chunks_x_plain_ms_per_step': round(chunks * statistics.median(plain_step), 3),
            'added_ms_per_step': _median(added)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--configs', default=','.join(CONFIGS))
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    if a.iters < 20:
        ap.error('--iters must be at least 20 (the figures are medians)')
    if a.steps < 2 or a.steps % 2:
        ap.error('--steps must be even (the per-step figure is a slope between steps and steps / 2)')
    names = a.configs.split(',')
    if any(c not in CONFIGS for c in names):
        ap.error(f'--configs takes a comma-separated subset of {CONFIGS}')
    if not torch.cuda.is_available():
        sys.exit('panorama_bench.py needs a GPU: nothing is measured without one')
    t0 = time.time()
    cfg = E.sd14_config(*WINDOW)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    res = {'device': torch.cuda.get_device_name(0), 'canvas_latent': list(CANVAS), 'image': f'{8 * CANVAS[0]}x{8 * CANVAS[1]}',
           'window_latent': list(WINDOW), 'stride': STRIDE, 'sampler': 'dpmpp_2m', 'steps': a.steps, 'guidance': 7.5, 'iters': a.iters}
    for name in names:
        res[name] = measure(sds, name, a.steps, a.iters, a.warmup)
        print(f'{name}: {json.dumps(res[name])}', file=sys.stderr, flush=True)
        torch.cuda.empty_cache()         # the configuration's pipeline is gone: its arenas go back before the next one is built
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
