#!/usr/bin/env python3
"""What T2I-Adapter structural control costs on one MI355X (synthetic SD v1.4 weights, 64 x 64 latent, one image = a guidance batch
of 2), a pipeline built with adapter=True next to one built without, in one process:

  * one guided UNet evaluation (the captured launch list, text context unchanged) without and with the four feature additions;
  * one set_adapter_hint call (adapter graph + four staging launches), host clock around a device synchronise;
  * generate_graphed, 20 PLMS steps, without the feature and with a hint set.

The two pipelines are timed alternately, `rounds` times; the medians and the spread of the rounds are reported.  Not the benchmark
(bench.py measures the flagship txt2img workload); the record behind INTEGRATION.md's "Structural control (T2I-Adapter)".  No
threshold is attached to it.

usage (GPU box):  python tools/adapter_bench.py [--rounds 7] [--iters 20] [--out profiles/adapter_bench.json]"""
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
    ap.add_argument('--iters', type=int, default=20, help='UNet evaluations per timed window (generate_graphed: a quarter of it)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table(),
              'adapter': E.Adapter(E.sd14_config(64, 64, adapter_hint_channels=3), 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    hint = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).cuda()
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False)
    plain, pipe = Txt2Img(**kw), Txt2Img(adapter=True, **kw)

    # one guided evaluation: the UNet graph's captured launch list on whatever its inputs hold, context projections not redone
    for p in (plain, pipe):
        p._set_context(ctx2)
        p.unet.execute(True)
        p.unet.execute(True)
    pipe.set_adapter_hint(hint)
    step = alternate({'without': lambda: plain.unet.execute(True, static_unchanged=True),
                      'with': lambda: pipe.unet.execute(True, static_unchanged=True)}, a.rounds, a.iters)

    # one hint: host clock, the device drained before and after
    set_ms = []
    for _ in range(a.rounds + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pipe.set_adapter_hint(hint)
        torch.cuda.synchronize()
        set_ms.append(1e3 * (time.perf_counter() - t))
    set_ms = set_ms[1:]          # the first call after the warm-up above still captures the adapter's graph

    gen = alternate({'without': lambda: plain.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms'),
                     'with_hint': lambda: pipe.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms')}, a.rounds, max(1, a.iters // 4))

    su, sa = plain.unet.stats(), pipe.unet.stats()
    ad = pipe.adapter.stats()
    res = {
        'device': torch.cuda.get_device_name(0), 'latent': [64, 64], 'unet_batch': 2, 'rounds': a.rounds, 'iters': a.iters,
        'unet_step': {'without': summary(step['without']), 'with_adapter_reps_2': summary(step['with']),
                      'launches': [su['launches'], sa['launches']], 'arena_bytes': [su['arena_bytes'], sa['arena_bytes']]},
        'set_adapter_hint': dict(summary(set_ms), adapter_launches=ad['launches'], adapter_weight_bytes=ad['weight_bytes'],
                                 adapter_arena_bytes=ad['arena_bytes'], adapter_tune=pipe.adapter.tune_source()),
        'generate_graphed_plms': {'steps': a.steps, 'without': summary(gen['without']), 'with_hint': summary(gen['with_hint'])},
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
