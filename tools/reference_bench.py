#!/usr/bin/env python3
"""What the shared-key attention launch costs on one MI355X, measured on one box in one process (SD v1.4 shapes).  The yardstick is
always the path WITHOUT the new kernel: ops.attention on concatenated K / V copies, and the UNet graph without the switch.

  (a) one sdod_attention_shared_f16 launch at batch 4, anchors 2, heads 8, on packed q|k|v rows as the UNet's four levels have them
      (64^2 d 40, 32^2 d 80, 16^2 d 160, 8^2 d 160).  shared_w0 (self_w = (0, 0)) against the SAME score work on ops.attention: two
      torch.cat copies [K_own ; K_anc], [V_own ; V_anc], one launch on the doubled keys for the two main rows and one for the two anchor
      rows; the yardstick's contiguous q / k / v operands are made outside the timed region.  shared_w_half_0 (self_w = (0.5, 0): the
      blend) against that plus the self-only launch the blend costs the yardstick, reported separately.  shared_w1 (self_w = (1, 1):
      one segment) against ops.attention on the four rows, which it equals bit for bit: what the SHARED instantiation's scratch and
      registers cost the workgroups that walk one segment.  Every side is 20 calls captured as one device graph; a figure is one replay
      between two device events / 20, the sides alternating, median / min / p90 over --iters rounds after warm-up.
  (b) one UNet evaluation at 64 x 64 as hipGraph replays (10 between two device events, static inputs unchanged): E.UNet(cfg, 2 n + 2,
      reference=2) at self_w = (0.5, 0) against E.UNet(cfg, 2 n) for n = 1, 2, alternating rounds.

usage (GPU box):  python tools/reference_bench.py [--iters 15] [--out profiles/reference_bench.json]"""
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
    """mean device time of one call in us: `reps` calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps


def _captured(fn, reps=20):
    """`reps` calls of fn as ONE device graph (warmed first): replaying it times the launches without the host's enqueue cost"""
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        for _ in range(reps):
            fn()
    return lambda: _timed(g.replay, 1) / reps


def launches(iters, warmup):
    out = []
    for hw, d in ((64, 40), (32, 80), (16, 160), (8, 160)):
        c, l = 8 * d, hw * hw
        g = torch.Generator().manual_seed(hw + d)
        qkv = torch.randn(4, l, 3 * c, generator=g).half().cuda()
        q, k, v = (qkv[:, :, i * c:(i + 1) * c] for i in range(3))
        o = torch.empty(4, l, c, dtype=torch.float16, device='cuda')
        # the yardstick's operands, made OUTSIDE the timed region: ops.attention takes contiguous tensors
        qm, qa, ka, va, q0, k0, v0 = (t.contiguous() for t in (q[:2], q[2:], k[2:], v[2:], q[:1], k[:1], v[:1]))
        qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
        o1 = torch.empty(1, l, c, dtype=torch.float16, device='cuda')
        w = {name: torch.tensor(ws, device='cuda') for name, ws in (('w0', (0.0, 0.0)), ('wblend', (0.5, 0.0)), ('w1', (1.0, 1.0)))}

        def concat():        # the same score work as self_w = (0, 0): 2 rows x 2 l keys + 2 rows x l keys; the concat copies counted
            ops.attention(qm, torch.cat([k[:2], k[2:]], 1), torch.cat([v[:2], v[2:]], 1), 8, out=o[:2])
            ops.attention(qa, ka, va, 8, out=o[2:])
        sides = {'shared_w0': lambda: ops.attention_shared(q, k, v, 8, 2, w['w0'], out=o),
                 'concat_and_attention': concat,
                 'shared_w_half_0': lambda: ops.attention_shared(q, k, v, 8, 2, w['wblend'], out=o),
                 'self_only_extra_launch': lambda: ops.attention(q0, k0, v0, 8, out=o1),   # what the blend costs the yardstick on top
                 'shared_w1': lambda: ops.attention_shared(q, k, v, 8, 2, w['w1'], out=o),
                 'attention_4_rows': lambda: ops.attention(qc, kc, vc, 8, out=o)}          # ... which shared_w1 equals bit for bit
        replay = {name: _captured(fn) for name, fn in sides.items()}
        t = {name: [] for name in sides}
        for it in range(warmup + iters):
            for name in sides:
                us = replay[name]()
                if it >= warmup:
                    t[name].append(us)
        med = {name: statistics.median(v2) for name, v2 in t.items()}
        out.append({'map': f'{hw}x{hw}', 'd': d, 'us': {k2: _summary(v2) for k2, v2 in t.items()},
                    'shared_w0_over_concat': round(med['shared_w0'] / med['concat_and_attention'], 4),
                    'shared_blend_over_concat_plus_self_only': round(med['shared_w_half_0'] / (med['concat_and_attention'] + med['self_only_extra_launch']), 4),
                    'shared_w1_over_attention': round(med['shared_w1'] / med['attention_4_rows'], 4)})
    return out


def graphs(sd, iters, warmup):
    out = []
    cfg = E.sd14_config(64, 64)
    for n in (1, 2):
        pair = {'plain': E.UNet(cfg, 2 * n), 'reference': E.UNet(cfg, 2 * n + 2, reference=2)}
        for g in pair.values():
            g.load_state_dict(sd)
            g.finalize()
            g.execute(use_hip_graph=True); g.execute(use_hip_graph=True)
        pair['reference'].reference_self_w.copy_(torch.tensor([0.5, 0.0]))
        t = {name: [] for name in pair}
        for it in range(warmup + iters):
            for name, g in pair.items():
                ms = _timed(lambda: g.execute(use_hip_graph=True, static_unchanged=True), 10) / 1e3
                if it >= warmup:
                    t[name].append(ms)
        out.append({'n': n, 'hipgraph_replay_ms': {name: _summary(v) for name, v in t.items()},
                    'ratio_of_medians': round(statistics.median(t['reference']) / statistics.median(t['plain']), 4),
                    'rows_ratio': round((2 * n + 2) / (2 * n), 4)})
        del pair
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('reference_bench.py needs a GPU: nothing is measured without one')
    t0 = time.time()
    sd = Wt.synthetic_state_dict(E.UNet(E.sd14_config(64, 64), 2).param_table(), seed=1234)
    res = {'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'launch': launches(a.iters, a.warmup),
           'graph_profile': graphs(sd, max(3, a.iters // 3), 1)}
    res['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
