#!/usr/bin/env python3
"""What HyperTile buys on one MI355X, measured on one box in one process (synthetic weights, SD v1.4 shapes).  The yardstick is always
the path WITHOUT the switch -- the untiled attention launch, the graph and the pipeline as they were -- never the tiled path itself.

  (a) one attn_tiled_d40 launch against one attn_d40 launch at B = 2, heads = 8, on packed q|k|v rows as the UNet's widest level has
      them: 64 x 64 with T = 32, 96 x 96 with T = 32 and T = 48.  The two alternate inside one loop; each figure is the mean of 20
      launches between two device events, median / min / p90 over --iters rounds after warm-up.
  (b) the UNet graph's launch list per evaluation (Graph.profile: per-dispatch device time, summed), at 64 x 64, 64 x 96 and 96 x 96,
      with and without the switch (tile 32, max_depth 0), alternating rounds; and the attention launches' share of it.
  (c) generate_hires_graphed 64^2 -> 96^2 (20 + 10 steps, the whole replay between two device events), with and without the switch.
  (d) for information: rel-L2 of generate()'s final image at 64 x 64 against the untiled run (the method is an approximation).

usage (GPU box):  python tools/hypertile_bench.py [--iters 15] [--out profiles/hypertile_bench.json] [--skip-hires]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, hypertile as HT, ops, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img  # noqa: E402


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


def launches(iters, warmup):
    out = []
    for hw, tile in ((64, 32), (96, 32), (96, 48)):
        th, tw = HT.grid(hw, hw, tile, 0, 0)
        g = torch.Generator().manual_seed(hw + tile)
        qkv = torch.randn(2, hw * hw, 3 * 320, generator=g).half().cuda()
        q, k, v = (qkv[:, :, i * 320:(i + 1) * 320] for i in range(3))
        o = torch.empty(2, hw * hw, 320, dtype=torch.float16, device='cuda')
        plain = lambda: ops._lib.check(ops._lib.hip().sdod_attention_f16(ops._p(q), ops._p(k), ops._p(v), ops._p(o), 2, 8, hw * hw, hw * hw, 40, 960,  # noqa: E731
                                                                         960, 960, 320, 40 ** -0.5, 0, ops._stream()))
        tiled = lambda: ops.attention_tiled(q, k, v, 8, (hw, hw), (th, tw), out=o)  # noqa: E731
        t = {'attn_d40': [], 'attn_tiled_d40': []}
        for it in range(warmup + iters):
            a, b = _timed(plain, 20), _timed(tiled, 20)
            if it >= warmup:
                t['attn_d40'].append(a); t['attn_tiled_d40'].append(b)
        out.append({'map': f'{hw}x{hw}', 'tile': tile, 'grid': f'{hw // th}x{hw // tw}', 'us': {k2: _summary(v2) for k2, v2 in t.items()},
                    'ratio_of_medians': round(statistics.median(t['attn_tiled_d40']) / statistics.median(t['attn_d40']), 4)})
    return out


def graphs(sd, iters, warmup):
    out = []
    for h, w in ((64, 64), (64, 96), (96, 96)):
        pair = {}
        for name, ht in (('plain', None), ('hypertile_32', (32, 0))):
            cfg = E.sd14_config(h, w)
            cfg.hypertile = ht
            g = E.UNet(cfg, 2)
            g.load_state_dict(sd)
            pair[name] = g.finalize()
        sums = {n: [] for n in pair}
        attn = {n: [] for n in pair}
        for it in range(warmup + iters):
            for n, g in pair.items():
                ms = g.profile(3)
                if it >= warmup:
                    sums[n].append(sum(ms))
                    attn[n].append(sum(t for (lab, _, _), t in zip(g.op_table(), ms) if lab.startswith('attn_')))
        out.append({'latent': f'{h}x{w}', 'launch_list_sum_ms': {n: _summary(v) for n, v in sums.items()},
                    'attention_launches_sum_ms': {n: _summary(v) for n, v in attn.items()},
                    'tiled_launches': sum(lab.startswith('attn_tiled') for lab, _, _ in pair['hypertile_32'].op_table()),
                    'ratio_of_medians': round(statistics.median(sums['hypertile_32']) / statistics.median(sums['plain']), 4)})
        del pair
        torch.cuda.empty_cache()
    return out


def pipelines(sds, iters, warmup, hires):
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g)
    kw = dict(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, hires_hw=96 if hires else None)
    plain, tiled = Txt2Img(**kw), Txt2Img(hypertile=32, **kw)
    a, b = plain.generate(ctx2, x_T, 20, 7.5, 'plms').float(), tiled.generate(ctx2, x_T, 20, 7.5, 'plms').float()
    res = {'rel_l2_final_image_64x64_vs_untiled': round(float((b - a).norm() / a.norm()), 5)}
    if hires:
        t = {'plain': [], 'hypertile_32': []}
        for it in range(warmup + iters):
            for n, p in (('plain', plain), ('hypertile_32', tiled)):
                us = _timed(lambda: p.generate_hires_graphed(ctx2, x_T, 20, 7.5, hires_steps=10), 1)
                if it >= warmup:
                    t[n].append(us / 1e3)
        res['generate_hires_graphed_64_to_96_ms'] = {n: _summary(v) for n, v in t.items()}
        res['hires_ratio_of_medians'] = round(statistics.median(t['hypertile_32']) / statistics.median(t['plain']), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-hires', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('hypertile_bench.py needs a GPU: nothing is measured without one')
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    res = {'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'launch': launches(a.iters, a.warmup),
           'graph_profile': graphs(sds['unet'], max(3, a.iters // 3), 1), 'pipeline': pipelines(sds, max(3, a.iters // 3), 1, not a.skip_hires)}
    res['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
