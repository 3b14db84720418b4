#!/usr/bin/env python3
"""What FreeU costs on one MI355X, measured on one box in one process (synthetic weights, SD v1.4 shapes, 64 x 64 latent, batch 2 =
one guided evaluation):

  * bench.py's `unet_step_ms` (its --full definition, imported, not restated) on the plain UNet graph, on the graph with the FreeU
    switch at the identity (twelve launches that read their parameters and end), and on the same graph at the version-2 SD 1.4 preset;
    the three alternate inside one loop so that they meet the same machine;
  * the per-launch durations of the twelve new launches from Graph.profile (per-dispatch, no queue latency), at the identity and at
    the preset, and the whole launch list's sum for scale.

Every step figure is the median of --iters calls of bench.unet_step_time (each the mean of 10 steps between two device events), after
warm-up.  Not the benchmark (bench.py measures the flagship txt2img workload); a tool for DESIGN.md's FreeU section.

usage (GPU box):  python tools/freeu_bench.py [--iters 20] [--out profiles/freeu_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdod.amd import engine as E, freeu as FU, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402


def _summary(v):
    v = sorted(v)
    return {'median': round(statistics.median(v), 4), 'min': round(v[0], 4), 'p90': round(v[int(0.9 * (len(v) - 1))], 4)}


def _freeu_launches(unet, iters):
    """[{label, detail, us}] of the graph's FreeU launches and the launch list's total in ms, from Graph.profile"""
    ms = unet.profile(iters)
    rows = [{'label': l, 'detail': d, 'us': round(1e3 * t, 2)} for (l, _, _), d, t in zip(unet.op_table(), unet.op_details(), ms) if l.startswith('freeu')]
    return rows, round(sum(ms), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('freeu_bench.py needs a GPU: nothing is measured without one')
    import bench
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, with_vae=False)
    plain, pipe = Txt2Img(**kw), Txt2Img(freeu=True, **kw)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    temb_p, temb_f = (p.time_embeddings(np.asarray([951.0], np.float32)) for p in (plain, pipe))
    plain._set_context(ctx2); pipe._set_context(ctx2)
    preset = FU.preset(2, 'sd14')

    times = {'plain': [], 'freeu_identity': [], 'freeu_preset_v2_sd14': []}
    for it in range(a.warmup + a.iters):
        v0 = bench.unet_step_time(plain, temb_p, x_T)
        pipe.clear_freeu()
        v1 = bench.unet_step_time(pipe, temb_f, x_T)
        pipe.set_freeu(*preset, 2)
        v2 = bench.unet_step_time(pipe, temb_f, x_T)
        if it >= a.warmup:
            for k, v in zip(times, (v0, v1, v2)):
                times[k].append(v)
    res = {'device': torch.cuda.get_device_name(0), 'latent': '64x64', 'batch': 2, 'iters': a.iters, 'preset': list(preset),
           'unet_step_ms': {k: _summary(v) for k, v in times.items()}}
    med = {k: v['median'] for k, v in res['unet_step_ms'].items()}
    res['unet_step_ms']['identity_minus_plain'] = _summary([b - c for b, c in zip(times['freeu_identity'], times['plain'])])
    res['unet_step_ms']['preset_minus_plain'] = _summary([b - c for b, c in zip(times['freeu_preset_v2_sd14'], times['plain'])])
    res['relative_cost'] = {'identity': round(med['freeu_identity'] / med['plain'] - 1.0, 4), 'preset_v2_sd14': round(med['freeu_preset_v2_sd14'] / med['plain'] - 1.0, 4)}
    res['launches'] = {'plain': plain.unet.stats()['launches'], 'freeu': pipe.unet.stats()['launches']}
    res['arena_bytes'] = {'plain': plain.unet.stats()['arena_bytes'], 'freeu': pipe.unet.stats()['arena_bytes']}
    pipe.clear_freeu()
    rows_i, tot_i = _freeu_launches(pipe.unet, 5)
    pipe.set_freeu(*preset, 2)
    rows_p, tot_p = _freeu_launches(pipe.unet, 5)
    pipe.clear_freeu()
    _, tot_plain = _freeu_launches(plain.unet, 5)
    res['profile'] = {'unit': 'us per launch (Graph.profile: per-dispatch device time, median of 5 eager passes)',
                      'identity': rows_i, 'preset_v2_sd14': rows_p,
                      'freeu_launches_sum_us': {'identity': round(sum(r['us'] for r in rows_i), 2), 'preset_v2_sd14': round(sum(r['us'] for r in rows_p), 2)},
                      'launch_list_sum_ms': {'plain': tot_plain, 'freeu_identity': tot_i, 'freeu_preset_v2_sd14': tot_p}}
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
