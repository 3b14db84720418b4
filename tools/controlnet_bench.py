#!/usr/bin/env python3
"""What ControlNet structural control costs on one MI355X (synthetic SD v1.4 weights, 64 x 64 latent, one image = a guidance batch of
2), a pipeline built with controlnet=True next to one built without, in one process:

  * one guided evaluation (the captured launch lists, text context unchanged): the plain UNet; the UNet with control inputs and
    every scale zero (what a cleared pipeline runs); the control graph followed by the UNet with control inputs (a set hint);
  * one set_control_hint call (hint encoder + the copy into the control graph's slot + the scales), host clock around a device
    synchronise;
  * generate_graphed, 20 PLMS steps, without the feature, with the flag but cleared, and with a hint set.

The variants are timed alternately, `rounds` times; the medians and the spread of the rounds are reported.  Not the benchmark
(bench.py measures the flagship txt2img workload); the record behind DESIGN.md 6j and INTEGRATION.md's "Structural control
(ControlNet)".  No threshold is attached to it.

usage (GPU box):  python tools/controlnet_bench.py [--rounds 7] [--iters 20] [--out profiles/controlnet_bench.json]"""
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


def control_table(cfg):
    """one table with every tensor of a ControlNet checkpoint (hint encoder in the checkpoint's own shapes)"""
    tcfg = E.copy_config(cfg)
    tcfg.control_temb = 1
    return E.ControlNet(cfg, 2).param_table() + E.Temb(tcfg, 1).param_table() + E.control_hint_checkpoint_table(cfg.model_channels)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20, help='evaluations per timed window (generate_graphed: a quarter of it)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table(),
              'controlnet': control_table(cfg)}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    hint = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).cuda()
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False)
    plain, pipe = Txt2Img(**kw), Txt2Img(controlnet=True, **kw)

    # one guided evaluation: the graphs' captured launch lists on whatever their inputs hold, context projections not redone
    for p in (plain, pipe):
        p._set_context(ctx2)
        p.unet.execute(True)
        p.unet.execute(True)
    pipe.controlnet.execute(True)
    pipe.controlnet.execute(True)

    def controlled():
        pipe.controlnet.execute(True, static_unchanged=True)
        pipe.unet.execute(True, static_unchanged=True)

    pipe.clear_control_hint()
    off = alternate({'without': lambda: plain.unet.execute(True, static_unchanged=True),
                     'cleared': lambda: pipe.unet.execute(True, static_unchanged=True)}, a.rounds, a.iters)
    pipe.set_control_hint(hint)
    on = alternate({'without': lambda: plain.unet.execute(True, static_unchanged=True), 'with_hint': controlled,
                    'control_graph_alone': lambda: pipe.controlnet.execute(True, static_unchanged=True)}, a.rounds, a.iters)

    # one hint: host clock, the device drained before and after
    set_ms = []
    for _ in range(a.rounds + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pipe.set_control_hint(hint)
        torch.cuda.synchronize()
        set_ms.append(1e3 * (time.perf_counter() - t))
    set_ms = set_ms[1:]          # (the first call may still capture the hint encoder's graph)

    gi = max(1, a.iters // 4)
    pipe.clear_control_hint()
    gen_off = alternate({'without': lambda: plain.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms'),
                         'cleared': lambda: pipe.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms')}, a.rounds, gi)
    pipe.set_control_hint(hint)
    gen_on = alternate({'without': lambda: plain.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms'),
                        'with_hint': lambda: pipe.generate_graphed(ctx2, x_T, a.steps, 7.5, 'plms')}, a.rounds, gi)

    def graph(gr):
        s = gr.stats()
        return {'launches': s['launches'], 'arena_bytes': s['arena_bytes'], 'weight_bytes': s['weight_bytes'], 'tune': gr.tune_source()}

    res = {
        'device': torch.cuda.get_device_name(0), 'latent': [64, 64], 'unet_batch': 2, 'rounds': a.rounds, 'iters': a.iters,
        'guided_evaluation': {'without': summary(off['without'] + on['without']), 'flag_cleared': summary(off['cleared']),
                              'with_hint': summary(on['with_hint']), 'control_graph_alone': summary(on['control_graph_alone'])},
        'set_control_hint': summary(set_ms),
        'generate_graphed_plms': {'steps': a.steps, 'without': summary(gen_off['without'] + gen_on['without']),
                                  'flag_cleared': summary(gen_off['cleared']), 'with_hint': summary(gen_on['with_hint'])},
        'graphs': {'unet': graph(plain.unet), 'unet_control_inputs': graph(pipe.unet), 'controlnet': graph(pipe.controlnet),
                   'control_hint': graph(pipe.control_hint)},
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
