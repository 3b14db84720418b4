#!/usr/bin/env python3
"""The VAE decoder's middle attention on one MI355X, four-launch form against fused form, one process, synthetic
weights, vae_channels 128 (d = 512): device time of the launches in which the two forms differ --
  four-launch: per image the V^T GEMM, the scores GEMM, sdod_softmax_rows_f16 and the P V GEMM;
  fused:       the V Linear over the batch and the attention_wide launch (with its merge pass where the keys are split)
-- from the graph's own per-launch timing (Graph.profile: an event pair stamped at each kernel's begin and end, eager), at latent
64x64, 96x96 and 128x128, batch 1 and 2, and for the fused form alone at 128x136 and 64x512, which the four-launch form cannot
build.  The launches around them (GroupNorm, the [q|k] projection, proj_out) are the same in both forms and are not counted.
Also: the arena size of both decoder graphs and the whole decode's summed launch time.  The two graphs of a size are profiled
alternately, --rounds times --iters launches each; the figure is the median over the rounds.  Before timing, the two forms'
images are compared (rel-L2).  Not the benchmark (bench.py measures the flagship txt2img workload).

usage (GPU box):  python tools/vae_attention_bench.py [--rounds 5] [--iters 5] [--out profiles/vae_attention_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, ops, weights as Wt  # noqa: E402

SIZES = [((64, 64), True), ((96, 96), True), ((128, 128), True), ((128, 136), False), ((64, 512), False)]


def block_ops(g, other=None):
    """indices of the launches in which the forms differ: what lies between the common head and the common tail of the two launch
    lists (label and shape detail); without a second form, the attention_wide launch and the V Linear in front of it"""
    mine = list(zip([lab for lab, _, _ in g.op_table()], g.op_details()))
    if other is None:
        a = [lab for lab, _ in mine].index('attention_wide')
        return [a - 1, a]
    theirs = list(zip([lab for lab, _, _ in other.op_table()], other.op_details()))
    head = next(i for i, (x, y) in enumerate(zip(mine, theirs)) if x != y)
    tail = next(i for i, (x, y) in enumerate(zip(reversed(mine), reversed(theirs))) if x != y)
    return list(range(head, len(mine) - tail))


def build(cfg, batch, fused, sd, z):
    g = E.VaeDecoder(cfg, batch, fused_attn=fused)
    g.load_state_dict(sd)
    g.finalize()
    g.z.copy_(z)
    g.execute()
    torch.cuda.synchronize()
    g.check()
    return g


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('vae_attention_bench.py needs a GPU: nothing is measured without one')
    rows = []
    for (h, w), both in SIZES:
        for batch in (1, 2) if both else (1,):
            cfg = E.sd14_config(h, w)
            sd = Wt.synthetic_state_dict(E.VaeDecoder(cfg, 1).param_table(), seed=1235)
            z = torch.randn(batch, 4, h, w, generator=torch.Generator().manual_seed(12)) * 0.18215 * 4
            forms = {'fused': build(cfg, batch, True, sd, z)}
            if both:
                forms['four_launch'] = build(cfg, batch, False, sd, z)
            row = {'latent_hw': [h, w], 'batch': batch, 'positions': h * w, 'key_splits': ops.attention_wide_splits(batch, h * w, h * w, 512)}
            if both:
                x, y = forms['fused'].img.float(), forms['four_launch'].img.float()
                row['rel_l2_fused_vs_four_launch'] = float((x - y).norm() / y.norm())
            ms = {k: {'block': [], 'decode': []} for k in forms}
            idx = {k: block_ops(g, next((o for j, o in forms.items() if j != k), None)) for k, g in forms.items()}
            for g in forms.values():
                g.profile(2)                                    # warm-up of the profiling path
            for _ in range(a.rounds):
                for k, g in forms.items():                      # alternating: both forms meet the same machine
                    t = g.profile(a.iters)
                    ms[k]['block'].append(sum(t[i] for i in idx[k]))
                    ms[k]['decode'].append(sum(t))
            for k, g in forms.items():
                fl = sum(g.op_table()[i][1] for i in idx[k])
                med = statistics.median(ms[k]['block'])
                row[k] = {'block_ms': round(med, 4), 'block_ms_min': round(min(ms[k]['block']), 4), 'block_ms_max': round(max(ms[k]['block']), 4),
                          'block_launches': len(idx[k]), 'block_labels': sorted({g.op_table()[i][0] for i in idx[k]}), 'block_tflops': round(fl / med / 1e9, 1),
                          'decode_launch_ms': round(statistics.median(ms[k]['decode']), 3),
                          'arena_mib': round(g.stats()['arena_bytes'] / 2 ** 20, 1), 'launches': g.stats()['launches']}
            if both:
                row['fused_over_four_launch'] = round(row['fused']['block_ms'] / row['four_launch']['block_ms'], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del forms
            torch.cuda.empty_cache()
    result = {'tool': 'tools/vae_attention_bench.py', 'device': torch.cuda.get_device_name(0), 'vae_channels': 128, 'rounds': a.rounds,
              'iters_per_round': a.iters, 'timing': 'Graph.profile: per-launch device time, eager, median over rounds', 'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
