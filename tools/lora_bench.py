"""Switching LoRA adapters on the full UNet (64 x 64 latent, batch 2, synthetic weights): Graph.set_loras against the only route that
existed before it -- merge on the host, build and finalize a new graph -- and the step time before, with and after an adapter.

For ranks 4, 16 and 128 on every supported weight of the UNet, medians over --repeats runs each, host clock around calls that end in a
device synchronise:
    set_loras_ms       Graph.set_loras(entries): fp16 image of the factors, upload, restore, one merge launch per weight, re-fold
    clear_ms           Graph.set_loras([]): restore + re-fold, nothing else
    restore_ms         a device-to-device copy of base_bytes() (what the restore is), timed on its own
    merges_ms          set_loras_ms - clear_ms: upload + merge launches;  refold_ms = clear_ms - restore_ms
    rebuild_ms         lora.merged_state_dict + UNet() + load_state_dict + finalize() of a fresh graph (--rebuild-repeats runs)
    unet_step_ms       hipGraph replay with unchanged static inputs, WINDOWS x REPS, before / with the adapter / after clearing it
Writes the result as JSON to --out (profiles/lora_switch.json) and prints it.

    python tools/lora_bench.py --out profiles/lora_switch.json

--family loha | lokr measures the same for the LyCORIS families through Graph.set_networks (sdod/amd/lycoris.py): LoHa at the given
ranks, LoKr at the --splits of w1 (a x b; 1x1 is a full delta), keyed 'AxB' where the LoRA result has the rank; the host route is then
lycoris.merged_state_dict.  --rebuild-repeats 0 leaves the host route out.  profiles/lycoris_switch.json holds these next to the
plain-LoRA figures of the commit before and after the families were added.
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

from sdod.amd import engine as E, lora as L, lycoris as Ly, weights as Wt  # noqa: E402

SKIP = ('input_blocks.0.0.weight', 'out.2.weight')


def entries(sd, names, rank, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in names:
        w = sd[n]
        up = torch.randn(w.shape[0], rank, generator=gen).half()
        down = (torch.randn(rank, *w.shape[1:], generator=gen) * (float(w.std()) / rank ** 0.5)).half()
        out.append((n, up.reshape(w.shape[0], rank, 1, 1) if w.dim() == 4 else up, down, 0.05))
    return out


def loha_entries(sd, names, rank, seed):
    """each low-rank product has the spread sqrt(std(W)): their Hadamard product has the weight's own"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in names:
        w = sd[n]
        f = []
        for _ in range(2):
            f.append(torch.randn(w.shape[0], rank, generator=gen).half())
            f.append((torch.randn(rank, *w.shape[1:], generator=gen) * (float(w.std()) ** 0.5 / rank ** 0.5)).half())
        out.append(('loha', n, *f, 0.05))
    return out


def lokr_entries(sd, names, a, b, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in names:
        w = sd[n]
        w1 = torch.randn(a, b, generator=gen).half()
        w2 = (torch.randn(w.shape[0] // a, w.shape[1] // b, *w.shape[2:], generator=gen) * float(w.std())).half()
        out.append(('lokr', n, w1, w2, 0.05))
    return out


def step_ms(g, windows, reps):
    g.execute(True)
    for _ in range(20):
        g.execute(True, static_unchanged=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.execute(True, static_unchanged=True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return dict(median=round(float(np.median(ms)), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=64)
    ap.add_argument('--ranks', type=int, nargs='+', default=[4, 16, 128])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--rebuild-repeats', type=int, default=3)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--family', choices=('lora', 'loha', 'lokr'), default='lora')
    ap.add_argument('--splits', nargs='+', default=['4x8', '16x64', '1x1'], metavar='AxB', help='--family lokr: the shapes of w1')
    ap.add_argument('--out', metavar='FILE')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    cfg = E.sd14_config(a.hw, a.hw)
    g = E.UNet(cfg, 2)
    table = g.param_table()
    sd = Wt.synthetic_state_dict(table, seed=1234)
    names = [n for n, s in table if len(s) >= 2 and n not in SKIP]
    g.load_state_dict(sd)
    g.keep_base()
    g.finalize()
    gen = torch.Generator().manual_seed(3)
    x, temb, ctx = (torch.randn(tuple(t.shape), generator=gen) for t in (g.x, g.temb, g.ctx))

    def stage(graph):
        graph.x.copy_(x); graph.temb.copy_((0.1 * temb).half()); graph.ctx.copy_(ctx.half())

    stage(g)
    res = dict(latent=a.hw, batch=2, adapted_weights=len(names), unet_weight_bytes=g.stats()['weight_bytes'], unet_base_bytes=g.base_bytes(),
               launches=g.stats()['launches'], tune=g.tune_source(), repeats=a.repeats, rebuild_repeats=a.rebuild_repeats,
               step_windows=a.windows, step_replays_per_window=a.reps, ranks={})
    if a.family != 'lora':
        res['family'] = a.family
    set_entries = g.set_loras if a.family == 'lora' else g.set_networks
    merged = L.merged_state_dict if a.family == 'lora' else Ly.merged_state_dict
    tcfg = E.sd14_config()
    tg = E.TextEncoder(tcfg, 2)
    tg.load_state_dict(Wt.synthetic_state_dict(tg.param_table(), seed=1236))
    tg.keep_base()
    tg.finalize()
    res['text_base_bytes'] = tg.base_bytes()
    del tg
    res['unet_step_ms_before'] = step_ms(g, a.windows, a.reps)
    base_eps = g.eps.clone()
    scratch = torch.empty(g.base_bytes(), dtype=torch.uint8, device='cuda')
    src = torch.empty_like(scratch)
    res['restore_ms'] = round(timed(lambda: scratch.copy_(src), a.repeats + 1)[0], 3)
    del scratch, src
    g.set_loras([])                                   # warm-up of the fold / compose launches' second use
    res['clear_ms'] = round(timed(lambda: g.set_loras([]), a.repeats)[0], 3)
    for rank in (a.splits if a.family == 'lokr' else a.ranks):
        if a.family == 'lokr':
            ka, kb = (int(v) for v in rank.split('x'))
            ent = lokr_entries(sd, names, ka, kb, seed=ka * 1000 + kb)
        else:
            ent = (entries if a.family == 'lora' else loha_entries)(sd, names, rank, seed=rank)
        set_entries(ent)                              # warm-up: the merge kernel's first launch
        total, runs = timed(lambda: set_entries(ent), a.repeats)
        with_lora = step_ms(g, a.windows, a.reps)
        moved = float((g.eps.float() - base_eps.float()).norm() / base_eps.float().norm())
        g.set_loras([])
        after = step_ms(g, a.windows, a.reps)
        same = bool(torch.equal(g.eps, base_eps))

        def rebuild():
            g2 = E.UNet(cfg, 2)
            g2.load_state_dict(merged(sd, ent))
            g2.finalize()
            return g2

        flop = sum(2.0 * sd[n].numel() * (1 if a.family == 'lokr' else rank * (2 if a.family == 'loha' else 1)) for n in names)
        res['ranks'][str(rank)] = dict(
            set_loras_ms=round(total, 3), set_loras_runs_ms=[round(v, 3) for v in runs], merges_ms=round(total - res['clear_ms'], 3),
            refold_ms=round(res['clear_ms'] - res['restore_ms'], 3), merge_gflop=round(flop / 1e9, 1),
            unet_step_ms_with_lora=with_lora, unet_step_ms_after_clear=after,
            output_moved_rel_l2=round(moved, 4), eps_after_clear_bit_equal=same)
        if a.rebuild_repeats > 0:
            t_merge = time.perf_counter()
            merged(sd, ent)
            t_merge = (time.perf_counter() - t_merge) * 1e3
            reb, reb_runs = timed(rebuild, a.rebuild_repeats)
            res['ranks'][str(rank)].update(rebuild_ms=round(reb, 1), rebuild_runs_ms=[round(v, 1) for v in reb_runs], host_merge_ms=round(t_merge, 1),
                                           rebuild_over_set_loras=round(reb / total, 1))
        print(f'rank {rank}:', json.dumps(res['ranks'][str(rank)]), flush=True)
    g.check()
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
