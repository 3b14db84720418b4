#!/usr/bin/env python3
"""What regional prompts cost on one MI355X (synthetic SD v1.4 weights, 64 x 64 latent, one image = a guidance batch of 2): a
pipeline built without the feature next to pipelines built with regions=2 and regions=3, in one process:

  * one guided evaluation (the captured launch lists, text context unchanged);
  * one set_regions call (the mask upload and the weights launch), host clock around a device synchronise;
  * generate_graphed, 20 PLMS steps.

The variants are timed alternately, `rounds` times; the medians and the spread of the rounds are reported.  At 64 x 64 every level
folds (L = 4096, 1024, 256, 64), so the only launches that differ are the two cross-attention GEMMs of each of the 16 transformer
blocks, `regions` times as wide.  Not the benchmark (bench.py measures the flagship txt2img workload); the record behind DESIGN.md
6k and INTEGRATION.md's "Regional prompts".  No threshold is attached to it.

usage (GPU box):  python tools/regions_bench.py [--rounds 7] [--iters 20] [--out profiles/regions_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, regions as RG, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402


def timed(fn, iters):
    """ms per call: `iters` back-to-back calls between two events (the caller has warmed fn up)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns, rounds, iters):
    """{name: [ms per call, one per round]}: every round times each function once, in turn"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, iters))
    return out


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20, help='evaluations per timed window (generate_graphed: a quarter of it)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False)
    pipes = {'without': Txt2Img(**kw), 'regions2': Txt2Img(regions=2, **kw), 'regions3': Txt2Img(regions=3, **kw)}
    ctx = {n: (0.5 * torch.randn(2, 77 * max(p.regions, 1), 768, generator=g)).half().cuda() for n, p in pipes.items()}
    masks = {n: RG.feather(RG.column_masks([1] * p.regions, 64), 16) for n, p in pipes.items() if p.regions}
    for n, p in pipes.items():
        if p.regions:
            p.set_regions(masks[n])
        p._set_context(ctx[n])
        p.unet.execute(True)
        p.unet.execute(True)

    ev = alternate({n: (lambda p=p: p.unet.execute(True, static_unchanged=True)) for n, p in pipes.items()}, a.rounds, a.iters)

    set_ms = {}
    for n, p in pipes.items():
        if not p.regions:
            continue
        ms = []
        for _ in range(a.rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            p.set_regions(masks[n])
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        set_ms[n] = summary(ms[1:])

    gi = max(1, a.iters // 4)
    gen = alternate({n: (lambda p=p, c=ctx[n]: p.generate_graphed(c, x_T, a.steps, 7.5, 'plms')) for n, p in pipes.items()}, a.rounds, gi)

    def graph(gr):
        s = gr.stats()
        return {'launches': s['launches'], 'arena_bytes': s['arena_bytes'], 'weight_bytes': s['weight_bytes'], 'tune': gr.tune_source()}

    res = {
        'device': torch.cuda.get_device_name(0), 'latent': [64, 64], 'unet_batch': 2, 'rounds': a.rounds, 'iters': a.iters,
        'guided_evaluation': {n: summary(v) for n, v in ev.items()},
        'set_regions': set_ms,
        'generate_graphed_plms': dict({'steps': a.steps}, **{n: summary(v) for n, v in gen.items()}),
        'graphs': {n: graph(p.unet) for n, p in pipes.items()},
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
