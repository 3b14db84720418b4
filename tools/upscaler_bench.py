#!/usr/bin/env python3
"""What the ESRGAN upscaler costs on one MI355X (synthetic weights, 23 blocks, one 512 x 512 image -> 2048 x 2048):

  * the UPSCALER graph as a hipGraph replay against the yardstick -- PyTorch's own fp16 convolutions (MIOpen, channels-last) running
    tests/rrdb_ref.py's restatement on the same weights in the same process.  Both are warmed up, then timed alternately over
    `--rounds` rounds of `--iters` runs each, so the run-to-run spread of both is in the file;
  * the trunk's FLOP/s from the op table, and each kernel family's share of the graph from an eager profiled run (Graph.profile);
  * generate_upscaled_graphed next to generate_graphed (64 x 64 latent, 20-step PLMS): what the upscale adds to an image.

The aim is to be no slower than the yardstick beyond the spread measured in the same run; no ratio is asserted -- the numbers are
recorded as they come (DESIGN.md section 6i discusses them).  Not the benchmark (bench.py measures the flagship txt2img workload).

usage (GPU box):  python tools/upscaler_bench.py [--rounds 5] [--iters 3] [--size 512] [--skip-pipeline] [--out profiles/upscaler_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd')); sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

import rrdb_ref as R  # noqa: E402
from sdod.amd import engine as E, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402


def timed(fn, iters):
    """ms per call: `iters` back-to-back calls between two events (the caller has warmed up)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(ms):
    return {'ms_rounds': ms, 'ms_median': round(statistics.median(ms), 3), 'ms_min': min(ms), 'ms_max': max(ms),
            'spread_over_median': round((max(ms) - min(ms)) / statistics.median(ms), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--blocks', type=int, default=23)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--skip-pipeline', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    dev = torch.device('cuda:0')
    img = R.sample_image(1, a.size, a.size)
    sd = R.synthetic(a.blocks)
    g = E.Upscaler(a.blocks, (a.size, a.size), 1)
    g.load_state_dict(sd)
    g.finalize()
    g.img.copy_(img)
    sd16 = {k: v.to(dev, torch.float16) for k, v in sd.items()}
    sd16 = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd16.items()}
    x16 = (img.to(dev).permute(0, 3, 1, 2).float() / 255.0).half().contiguous(memory_format=torch.channels_last)

    def ours():
        g.execute(use_hip_graph=True)

    def yard():
        with torch.no_grad():
            return R.forward_float(sd16, x16)

    for _ in range(3):                            # capture / solver search + warm-up of both
        ours(); yard()
    torch.cuda.synchronize()
    y_ref = yard().permute(0, 2, 3, 1).float()
    agree = float((g.out.float() - y_ref).norm() / y_ref.norm())
    ms = {'graph': [], 'miopen': []}
    for _ in range(a.rounds):                     # alternating: a drift of the clocks hits both alike
        ms['graph'].append(round(timed(ours, a.iters), 3))
        ms['miopen'].append(round(timed(yard, a.iters), 3))
    table = g.op_table()
    prof = g.profile(2)
    by_label = {}
    for (label, fl, _), t in zip(table, prof):
        e = by_label.setdefault(label, [0, 0.0, 0.0])
        e[0] += 1; e[1] += t; e[2] += fl
    total = sum(prof)
    nb = a.blocks
    trunk_ms, trunk_fl = sum(prof[1:1 + 15 * nb]), sum(t[1] for t in table[1:1 + 15 * nb])
    st = g.stats()
    res = {'device': torch.cuda.get_device_name(0), 'workload': f'RRDBNet x4, {nb} blocks, one {a.size} x {a.size} image, fp16',
           'method': f'hipGraph replay of the UPSCALER graph vs tests/rrdb_ref.forward_float in fp16 channels_last (MIOpen) on the same weights, '
                     f'same process; 3 warm-up runs each, then {a.rounds} alternating rounds of {a.iters} back-to-back runs between two events',
           'rounds': a.rounds, 'iters_per_round': a.iters,
           'graph': dict(summary(ms['graph']), launches=st['launches'], arena_bytes=st['arena_bytes'], weight_bytes=st['weight_bytes'],
                         flops=st['flops'], tflops_at_median=round(st['flops'] / statistics.median(ms['graph']) / 1e9, 2)),
           'miopen': summary(ms['miopen']),
           'graph_over_miopen': round(statistics.median(ms['graph']) / statistics.median(ms['miopen']), 4),
           'rel_l2_graph_vs_miopen': agree,
           'profile_eager': {'ms_total': round(total, 3), 'trunk_ms': round(trunk_ms, 3), 'trunk_flops': trunk_fl,
                             'trunk_tflops': round(trunk_fl / trunk_ms / 1e9, 2),
                             'by_label': {k: {'launches': n, 'ms': round(t, 3), 'share': round(t / total, 4), 'tflops': round(fl / t / 1e9, 2) if t > 0 else 0}
                                          for k, (n, t, fl) in sorted(by_label.items())},
                             'dense_conv_share': round(sum(t for k, (n, t, fl) in by_label.items() if k.startswith('dense_conv')) / total, 4)}}
    del g, sd16, x16, y_ref
    torch.cuda.empty_cache()
    if not a.skip_pipeline:
        cfg = E.sd14_config(64, 64)
        tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
        sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
        sds['upscaler'] = sd
        gen = torch.Generator().manual_seed(5)
        ctx2 = (0.5 * torch.randn(2, 77, 768, generator=gen)).half().cuda()
        x_T = torch.randn(1, 4, 64, 64, generator=gen).cuda()
        kw = dict(steps=a.steps, guidance=7.5, sampler='plms')
        pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, upscaler=True)
        runs = {'generate_graphed': lambda: pipe.generate_graphed(ctx2, x_T, **kw),
                'generate_upscaled_graphed': lambda: pipe.generate_upscaled_graphed(ctx2, x_T, **kw)}
        for fn in runs.values():
            fn(); fn()
        torch.cuda.synchronize()
        pm = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                pm[k].append(round(timed(fn, a.iters), 3))
        res['pipeline'] = {'workload': f'64x64 latent, {a.steps}-step plms, batch 1; the upscaled image is 2048 x 2048',
                           **{k: summary(v) for k, v in pm.items()},
                           'upscale_adds_ms': round(statistics.median(pm['generate_upscaled_graphed']) - statistics.median(pm['generate_graphed']), 3)}
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
