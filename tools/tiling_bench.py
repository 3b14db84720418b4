#!/usr/bin/env python3
"""What seamless tiling costs on one MI355X (synthetic weights, SD v1.4 shapes, 64 x 64 latent, batch 1):

  * generate_graphed, 20-step PLMS, with tiling=False, 'xy' and 'x' on one build: the three pipelines timed alternately over
    `--rounds` rounds of `--iters` images each; ms per image of every round, median / min / max, images per second;
  * the three UNets' launch lists (labels = kernel family and tile) compared, their launches and arena bytes, where their GEMM
    tiles came from (Graph.tune_source), and the per-label sum of the per-launch times of an eager profiled run
    (Graph.profile), so that a difference can be traced to a kernel.

From the code the expectation is no difference: same launches, same DMA counts in the halo-patch tiles; only the implicit-GEMM
gather (stride-2 and deepest-level convolutions) issues more loader instructions per DMA under a circular border.

Not the benchmark (bench.py measures the flagship txt2img workload); the record behind INTEGRATION.md's "Seamless tiling" and
DESIGN.md section 6h.  No threshold is attached to it.  --bench-runs FILE embeds a JSON file of recorded bench.py result lines
(the plain path of this build against its parent) under "bench_py_runs".

usage (GPU box):  python tools/tiling_bench.py [--rounds 5] [--iters 3] [--out profiles/tiling_bench.json]"""
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

MODES = (False, 'xy', 'x')


def timed(fn, iters):
    """ms per call: `iters` back-to-back calls between two events (the caller has warmed up)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def by_label(g, iters=3):
    """{label: [launches, ms summed over them]} of one eager, event-timed run of the graph"""
    out = {}
    for (label, _, _), ms in zip(g.op_table(), g.profile(iters)):
        e = out.setdefault(label, [0, 0.0])
        e[0] += 1
        e[1] += ms
    return {k: [n, round(ms, 4)] for k, (n, ms) in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--bench-runs', default=None, help='JSON file of recorded bench.py runs to embed')
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    kw = dict(steps=a.steps, guidance=7.5, sampler='plms')
    pipes = {m: Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, tiling=m) for m in MODES}
    runs = {m: (lambda p=p: p.generate_graphed(ctx2, x_T, **kw)) for m, p in pipes.items()}
    for fn in runs.values():                      # capture + warm-up
        fn(); fn()
    torch.cuda.synchronize()
    ms = {m: [] for m in MODES}
    for _ in range(a.rounds):                     # alternating: a drift of the clocks hits the three alike
        for m in MODES:
            ms[m].append(round(timed(runs[m], a.iters), 3))
    name = {False: 'tiling_off', 'xy': 'tiling_xy', 'x': 'tiling_x'}
    res = {'device': torch.cuda.get_device_name(0), 'workload': f'generate_graphed 64x64, {a.steps}-step plms, batch 1',
           'rounds': a.rounds, 'iters_per_round': a.iters}
    plain = pipes[False]
    for m in MODES:
        p = pipes[m]
        med = statistics.median(ms[m])
        st, sv = p.unet.stats(), p.vae.stats()
        res[name[m]] = {
            'ms_per_image_rounds': ms[m], 'ms_per_image_median': round(med, 3), 'ms_per_image_min': min(ms[m]), 'ms_per_image_max': max(ms[m]),
            'images_per_s': round(1000.0 / med, 3),
            'unet': {'launches': st['launches'], 'arena_bytes': st['arena_bytes'], 'tune': p.unet.tune_source(),
                     'launch_list_equals_plain': p.unet.op_table() == plain.unet.op_table() and p.unet.op_details() == plain.unet.op_details()},
            'vae': {'launches': sv['launches'], 'arena_bytes': sv['arena_bytes'], 'tune': p.vae.tune_source(),
                    'launch_list_equals_plain': p.vae.op_table() == plain.vae.op_table() and p.vae.op_details() == plain.vae.op_details()},
            'unet_ms_by_label': by_label(p.unet), 'vae_ms_by_label': by_label(p.vae),
        }
    base = res['tiling_off']
    for m in ('xy', 'x'):
        r = res[name[m]]
        r['ms_per_image_over_off'] = round(r['ms_per_image_median'] / base['ms_per_image_median'], 4)
        r['unet_label_ms_minus_off'] = {k: round(v[1] - base['unet_ms_by_label'].get(k, [0, 0.0])[1], 4) for k, v in r['unet_ms_by_label'].items()
                                        if abs(v[1] - base['unet_ms_by_label'].get(k, [0, 0.0])[1]) >= 0.002}
        r['vae_label_ms_minus_off'] = {k: round(v[1] - base['vae_ms_by_label'].get(k, [0, 0.0])[1], 4) for k, v in r['vae_ms_by_label'].items()
                                       if abs(v[1] - base['vae_ms_by_label'].get(k, [0, 0.0])[1]) >= 0.002}
    if a.bench_runs:
        with open(a.bench_runs) as f:
            res['bench_py_runs'] = json.load(f)
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
