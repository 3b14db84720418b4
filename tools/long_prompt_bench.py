"""The guided UNet step against the number of cross-attention keys: the UNet graph at hw x hw latent, batch 2 (the classifier-free
guidance pair), context_len = 77 * chunks, as a hipGraph replay with unchanged static inputs -- what every sampler step after the
first replays.  Event-timed in WINDOWS x REPS replays after a warm-up; prints one JSON line (median / min / max ms per step, launch
counts, where the GEMM tiles came from) and with --op-table FILE writes the launch list (label, detail) for comparing two builds.

    python tools/long_prompt_bench.py --chunks 1      # 77 keys: the folded cross-attention
    python tools/long_prompt_bench.py --chunks 2      # 154 keys: Linear + attention + Linear per block
    SDOD_LIBSDOD=libsdod_prev.so python tools/long_prompt_bench.py --chunks 1 --tag parent      # another build in lib/, same box
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'stable-diffusion-on-device_amd')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdod.amd import engine as E, weights as Wt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chunks', type=int, default=1)
    ap.add_argument('--hw', type=int, default=64)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--tag', default='')
    ap.add_argument('--op-table', metavar='FILE')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    t0 = time.time()
    cfg = E.sd14_config(a.hw, a.hw)
    cfg.context_len = 77 * a.chunks
    g = E.UNet(cfg, 2)
    g.load_state_dict(Wt.synthetic_state_dict(g.param_table(), seed=1234))
    g.finalize()
    gen = torch.Generator().manual_seed(3)
    g.x.copy_(torch.randn(tuple(g.x.shape), generator=gen))
    g.temb.copy_((0.1 * torch.randn(tuple(g.temb.shape), generator=gen)).half())
    g.ctx.copy_(torch.randn(tuple(g.ctx.shape), generator=gen).half())
    g.execute(True)                                   # the static launches (K/V projection, the fold) run here, once per prompt
    for _ in range(20):
        g.execute(True, static_unchanged=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            g.execute(True, static_unchanged=True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.reps)
    g.check()
    assert torch.isfinite(g.eps).all()
    table, details = g.op_table(), g.op_details()
    labels = [t[0] for t in table]
    if a.op_table:
        with open(a.op_table, 'w') as f:
            for lab, det in zip(labels, details):
                f.write(f'{lab}\t{det}\n')
    print(json.dumps(dict(
        tag=a.tag, lib=os.environ.get('SDOD_LIBSDOD', 'libsdod.so'), latent=a.hw, batch=2, prompt_chunks=a.chunks, keys=77 * a.chunks,
        step_ms_median=round(float(np.median(ms)), 4), step_ms_min=round(min(ms), 4), step_ms_max=round(max(ms), 4),
        windows=a.windows, replays_per_window=a.reps, launches=g.stats()['launches'], launch_list=len(table),
        xattn_fold_launches=labels.count('xattn_fold'), attention_launches=sum(lab.startswith('attn_d') for lab in labels),
        gflop_per_step=round(g.stats()['flops'] / 1e9, 1), tune=g.tune_source(), setup_s=round(time.time() - t0, 1))), flush=True)


if __name__ == '__main__':
    main()
