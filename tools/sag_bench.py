#!/usr/bin/env python3
"""What Self-Attention Guidance costs on one MI355X, measured on one box in one process (synthetic weights, SD v1.4 shapes).

  (a) the attn_mass_d160 launch (sdod_attention_mass_f16: its two kernels) against the attn_d160 launch beside it in middle_block.1, in
      the 2-row pair graph built with the switch (heads = 8, d = 160, packed q|k|v rows) at the 8 x 8, 8 x 12 and 12 x 12 middle maps
      (512 x 512, 512 x 768 and 768 x 768 images).  DEVICE time from the graph's per-launch timer (Graph.profile: an event pair at
      each launch's begin and end, eager, mean of 5 executes), median / min / p90 over --iters rounds after warm-up.  Both launches
      are stamped in the same execute, so they meet the same machine state.
  (b) a UNet evaluation at 512 x 512 (64 x 64 latent), hipGraph replays between two device events, alternating:
        plain     the 2-row pair graph without the switch
        pair_sag  the 2-row pair graph with the switch (one attn_mass_d160 launch more)
        sag_eval  pair_sag, then what SAG adds behind it, as Txt2Img._unet_eps runs it: sag_degrade, the time-row copy, the 1-row
                  UNet graph, sag_fold.  The three small launches between the replays are eager, so their host gaps are in the figure.

usage (GPU box):  python tools/sag_bench.py [--iters 15] [--out profiles/sag_bench.json]"""
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


def _summary(v):
    v = sorted(v)
    return {'median': round(statistics.median(v), 4), 'min': round(v[0], 4), 'p90': round(v[int(0.9 * (len(v) - 1))], 4)}


def _timed(fn, reps):
    """mean time of one call in us, `reps` calls between two device events: whatever gaps the host leaves between launches are inside"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def launches(iters, warmup):
    """device time of the attn_mass_d160 launch and of the attn_d160 launch beside it, from the pair graph's own per-launch timer"""
    out = []
    sd = None
    for h, w in ((8, 8), (8, 12), (12, 12)):
        cfg = E.sd14_config(8 * h, 8 * w)
        if sd is None:
            sd = Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234)
        g = E.UNet(cfg, 2, sag=True)
        g.load_state_dict(sd)
        g.finalize()
        gen = torch.Generator().manual_seed(h * w)
        g.x.copy_(torch.randn(2, 4, 8 * h, 8 * w, generator=gen)); g.ctx.copy_((0.5 * torch.randn(2, 77, 768, generator=gen)).half()); g.temb.normal_(0, 0.1)
        g.execute()
        labels = [lab for lab, _, _ in g.op_table()]
        i_mass = labels.index('attn_mass_d160')
        i_attn = min((i for i, lab in enumerate(labels) if lab == 'attn_d160'), key=lambda i: abs(i - i_mass))   # middle_block.1's attn1
        t = {'attn_d160': [], 'attn_mass_d160': []}
        for it in range(warmup + iters):
            ms = g.profile(5)
            if it >= warmup:
                t['attn_d160'].append(1e3 * ms[i_attn]); t['attn_mass_d160'].append(1e3 * ms[i_mass])
        out.append({'middle_map': f'{h}x{w}', 'ops_apart': abs(i_attn - i_mass), 'us': {k2: _summary(v2) for k2, v2 in t.items()},
                    'ratio_of_medians': round(statistics.median(t['attn_mass_d160']) / statistics.median(t['attn_d160']), 4)})
        del g
    return out


def evaluation(iters, warmup):
    cfg = E.sd14_config(64, 64)
    sd = Wt.synthetic_state_dict(E.UNet(cfg, 2).param_table(), seed=1234)
    plain, pair, single = E.UNet(cfg, 2), E.UNet(cfg, 2, sag=True), E.UNet(cfg, 1)
    gen = torch.Generator().manual_seed(9)
    x, ctx = torch.randn(2, 4, 64, 64, generator=gen), (0.5 * torch.randn(2, 77, 768, generator=gen)).half()
    for g in (plain, pair, single):
        g.load_state_dict(sd)
        g.finalize()
        g.x.copy_(x[:g.batch]); g.ctx.copy_(ctx[:g.batch]); g.temb.normal_(0, 0.1)
        g.execute(); g.execute(use_hip_graph=True)
    a, b, ss = 0.6, 0.8, 1.0

    def sag_eval():
        pair.execute(use_hip_graph=True, static_unchanged=True)
        ops.sag_degrade(pair.x[:1], pair.eps[:1], pair.sag_mass[:1], a, b, ss, out=single.x)
        single.temb.copy_(pair.temb[:1])
        single.execute(use_hip_graph=True, static_unchanged=True)
        ops.sag_fold(pair.eps, single.eps, 0.75, 7.5)
    forms = {'plain': lambda: plain.execute(use_hip_graph=True, static_unchanged=True),
             'pair_sag': lambda: pair.execute(use_hip_graph=True, static_unchanged=True), 'sag_eval': sag_eval}
    t = {n: [] for n in forms}
    for it in range(warmup + iters):
        for n, fn in forms.items():
            us = _timed(fn, 10)
            if it >= warmup:
                t[n].append(us / 1e3)
    med = {n: statistics.median(v) for n, v in t.items()}
    return {'latent': '64x64', 'ms': {n: _summary(v) for n, v in t.items()}, 'launches': {'plain': plain.stats()['launches'], 'pair_sag': pair.stats()['launches'],
            'single': single.stats()['launches']}, 'pair_sag_over_plain': round(med['pair_sag'] / med['plain'], 4),
            'sag_eval_over_plain': round(med['sag_eval'] / med['plain'], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('sag_bench.py needs a GPU: nothing is measured without one')
    t0 = time.time()
    res = {'device': torch.cuda.get_device_name(0), 'iters': a.iters,
           'timing': {'launch': 'Graph.profile: per-launch device time, eager', 'evaluation': 'hipGraph replays between two device events, mean of 10'},
           'launch': launches(a.iters, a.warmup), 'evaluation': evaluation(a.iters, a.warmup)}
    res['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
