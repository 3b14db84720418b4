#!/usr/bin/env python3
"""Inpainting on one MI355X next to img2img on the same box, one process (synthetic weights, SD v1.4 shapes, 512 px, batch 1,
strength 0.75 of 20 DDIM steps = 15 guided UNet evaluations):

  * the like-for-like pair: two device graphs with the same static inputs (context, image, mask, n1, n2, step_noise) and no noise
    generation in either, `fused_graph_replay` = the graph of Txt2Img.inpaint_graphed (one launch per step behind the UNet) and
    `composed_graph_replay` = the same loop COMPOSED from separate launches -- stage_unet_inputs, cfg_combine, ddim_step, torch's
    elementwise blend -- captured the same way; its result is checked against inpaint() bit for bit first;
  * whole calls, host work included: Txt2Img.inpaint_graphed with device noise (16 Philox fills of the graph's noise inputs, input
    copies, replay), with injected noise (copies, replay), and Txt2Img.img2img_graphed with device noise.

Every figure is the median of --iters (>= 20) single calls, each between two device events, after warm-up; the variants alternate
inside one loop so that they meet the same machine.  Not the benchmark (bench.py measures the flagship txt2img workload); a tool for
DESIGN.md's inpainting paragraph.

--concat measures the 9-channel inpainting checkpoint path instead (Txt2Img(inpaint_unet=True)), at the same size:

  * the input convolution at 2 x 64 x 64 -> 320, per launch, each variant as a device graph of 100 launches: the 4-channel
    sdod_conv_in_f16, the 9-channel sdod_conv_in_cat_f16, and the two launches it replaces (sdod_latent_im2col_f16 to K = 128 on an already concatenated tensor + the K = 128 GEMM);
  * bench.py's `unet_step_ms` (its --full definition, imported, not restated) on the 4-channel and on the 9-channel UNet graph;
  * whole calls at 20-step PLMS: inpaint_concat_graphed beside generate_graphed (4-channel pipeline), inpaint_graphed and
    img2img_graphed (strength 0.75 of 20 DDIM steps = 15 evaluations, for scale).

usage (GPU box):  python tools/inpaint_bench.py [--iters 30] [--out profiles/inpaint_bench.json]
                  python tools/inpaint_bench.py --concat [--iters 30] [--out profiles/inpaint_concat_bench.json]"""
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

from sdod.amd import engine as E, ops, weights as Wt  # noqa: E402
from sdod.amd.pipeline import Txt2Img, img2img_schedule, inpaint_levels  # noqa: E402


def composed_inpaint(pipe, ctx2, u8, mask, strength, steps, guidance, noise, step_noise):
    """Txt2Img.inpaint() with injected noise, the per-step work as the separate launches the fused step replaces: the same inputs, the
    same launches in front of and behind the loop, no noise generation anywhere"""
    sch, t_enc = img2img_schedule(strength, steps)
    keep = ops.mask_to_latent(mask)[:, None]
    x, z0 = pipe.encode(u8, 0, 0, strength, steps, noise, return_z0=True)
    temb = pipe.time_embeddings(sch.timesteps.astype(np.float32))
    pipe._set_context(ctx2)
    for index, j, sa, s1a in inpaint_levels(sch, t_enc):
        e_t = pipe._eps(x, temb[index], guidance, mode=1)              # stage_unet_inputs, UNet, cfg_combine
        ops.ddim_step(x, e_t, **sch.coef(index))
        known = z0 if j is None else sa * z0 + s1a * step_noise[j]
        x = keep * known + (1 - keep) * x
    return pipe.decode(x, mode=1, composite=(u8, mask))


def _summary(v):
    v = sorted(v)
    return {'median': round(statistics.median(v), 3), 'min': round(v[0], 3), 'p90': round(v[int(0.9 * (len(v) - 1))], 3)}


def _alternate(variants, warmup, iters, scale=1.0):
    """every variant once per iteration, each between two device events; {name: [ms * scale]}"""
    times = {k: [] for k in variants}
    for it in range(warmup + iters):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1) * scale)
    return times


def concat_input_conv(a):
    """us per launch of the UNet's input convolution at 2 x 64 x 64 -> 320, every variant a device graph of `reps` launches"""
    reps = 100
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 64, 64, generator=g).cuda()
    cond = torch.randn(2, 5, 64, 64, generator=g).cuda()
    cat = torch.cat([x, cond], 1).contiguous()
    bias = torch.randn(320, generator=g).cuda()
    w4 = torch.zeros(320, 64, dtype=torch.float16); w4[:, :36] = (torch.randn(320, 36, generator=g) / 6).half()
    w9 = torch.zeros(320, 128, dtype=torch.float16); w9[:, :81] = (torch.randn(320, 81, generator=g) / 9).half()
    w4, w9 = w4.cuda(), w9.cuda()

    kernels = {'conv_in_4ch': lambda: ops.conv_in(x, w4, bias), 'conv_in_cat': lambda: ops.conv_in_cat(x, cond, w9, bias),
               'im2col128_gemm': lambda: ops.gemm(ops.latent_im2col(cat, 128, 1.0), w9, bias)}
    equal = bool(torch.equal(kernels['conv_in_cat'](), kernels['im2col128_gemm']().view(2, 64, 64, 320)))
    graphs = {}
    for name, fn in kernels.items():
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            for _ in range(reps):
                fn()
        graphs[name] = gr
    times = _alternate({k: v.replay for k, v in graphs.items()}, a.warmup, a.iters, scale=1e3 / reps)
    out = {k: _summary(v) for k, v in times.items()}
    med = {k: v['median'] for k, v in out.items()}
    out.update(unit='us per launch (device graph of %d launches, median of %d replays, variants alternating)' % (reps, a.iters),
               shape='2 x 64 x 64 -> 320', cat_equals_im2col128_gemm_bit_for_bit=equal,
               cat_over_4ch=round(med['conv_in_cat'] / med['conv_in_4ch'], 3),
               cat_over_two_launch=round(med['conv_in_cat'] / med['im2col128_gemm'], 3))
    return out


def main_concat(a):
    sys.path.insert(0, ROOT)
    import bench
    t0 = time.time()
    res = {'device': torch.cuda.get_device_name(0), 'image': '512x512', 'iters': a.iters, 'input_conv': concat_input_conv(a)}
    cfg9, cfg4 = E.sd14_config(64, 64, concat_channels=5), E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg9, 2).param_table(), 'temb': E.Temb(cfg9, 1).param_table(),
              'vae': E.VaeDecoder(cfg9, 1).param_table(), 'vae_enc': E.VaeEncoder(cfg9, 1).param_table()}
    sds9 = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    sds4 = dict(sds9, unet=dict(sds9['unet']))
    sds4['unet']['input_blocks.0.0.weight'] = sds9['unet']['input_blocks.0.0.weight'][:, :4].contiguous()
    assert dict(E.UNet(cfg4, 2).param_table()) == {k: tuple(v.shape) for k, v in sds4['unet'].items()}
    pipe9 = Txt2Img(state_dicts=sds9, images_per_gpu=1, latent_hw=64, with_text_encoder=False, inpaint_unet=True)
    pipe4 = Txt2Img(state_dicts=sds4, images_per_gpu=1, latent_hw=64, with_text_encoder=False, with_vae_encoder=True)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    u8 = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).cuda()
    yy, xx = torch.meshgrid(torch.arange(512.), torch.arange(512.), indexing='ij')
    mask = (255.0 * ((xx + 0.5 * yy - 250.0) / 100.0).clamp(0.0, 1.0)).round().to(torch.uint8)[None].cuda()
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    st, gd, seed = a.steps, 7.5, 1

    eager = pipe9.inpaint_concat(ctx2, u8, mask, x_T, st, gd, seed=seed)
    res['graphed_equals_eager'] = bool(torch.equal(pipe9.inpaint_concat_graphed(ctx2, u8, mask, x_T, st, gd, seed=seed), eager))
    # bench.py's unet_step_ms on both graphs, alternating
    temb4 = pipe4.time_embeddings(np.asarray([951.0], np.float32)); temb9 = pipe9.time_embeddings(np.asarray([951.0], np.float32))
    pipe4._set_context(ctx2); pipe9._set_context(ctx2)
    steps4, steps9 = [], []
    for it in range(a.warmup + a.iters):
        v4, v9 = bench.unet_step_time(pipe4, temb4, x_T), bench.unet_step_time(pipe9, temb9, x_T)
        if it >= a.warmup:
            steps4.append(v4); steps9.append(v9)
    res['unet_step_ms'] = {'unet_4ch': _summary(steps4), 'unet_9ch': _summary(steps9),
                           'diff_9ch_minus_4ch': _summary([b - c for b, c in zip(steps9, steps4)]),
                           'launches': {'unet_4ch': pipe4.unet.stats()['launches'], 'unet_9ch': pipe9.unet.stats()['launches']}}
    variants = {
        'generate_graphed': lambda: pipe4.generate_graphed(ctx2, x_T, st, gd, 'plms'),
        'inpaint_concat_graphed': lambda: pipe9.inpaint_concat_graphed(ctx2, u8, mask, x_T, st, gd, seed=seed),
        'inpaint_graphed_0.75': lambda: pipe4.inpaint_graphed(ctx2, u8, mask, 0.75, st, gd, seed=seed),
        'img2img_graphed_0.75': lambda: pipe4.img2img_graphed(ctx2, u8, 0.75, st, gd, seed=seed),
    }
    times = _alternate(variants, a.warmup, a.iters)
    res['ms_per_image'] = {k: _summary(v) for k, v in times.items()}
    res['ms_per_image']['inpaint_concat_minus_generate'] = _summary([b - c for b, c in zip(times['inpaint_concat_graphed'], times['generate_graphed'])])
    res['steps'] = st
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--concat', action='store_true', help='measure the 9-channel inpainting checkpoint path (see the module docstring)')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--strength', type=float, default=0.75)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    if a.iters < 20:
        ap.error('--iters must be at least 20 (the figures are medians)')
    if not torch.cuda.is_available():
        sys.exit('inpaint_bench.py needs a GPU: nothing is measured without one')
    if a.concat:
        return main_concat(a)
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
              'vae': E.VaeDecoder(cfg, 1).param_table(), 'vae_enc': E.VaeEncoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    pipe = Txt2Img(state_dicts=sds, images_per_gpu=1, latent_hw=64, with_text_encoder=False, with_vae_encoder=True)
    g = torch.Generator().manual_seed(5)
    ctx2 = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    u8 = torch.randint(0, 256, (1, 512, 512, 3), generator=g, dtype=torch.uint8).cuda()
    yy, xx = torch.meshgrid(torch.arange(512.), torch.arange(512.), indexing='ij')
    mask = (255.0 * ((xx + 0.5 * yy - 250.0) / 100.0).clamp(0.0, 1.0)).round().to(torch.uint8)[None].cuda()
    _, t_enc = img2img_schedule(a.strength, a.steps)
    n1, n2 = torch.randn(2, 1, 4, 64, 64, generator=g).cuda()
    sn = torch.randn(t_enc - 1, 1, 4, 64, 64, generator=g).cuda()
    s, st, gd, seed = a.strength, a.steps, 7.5, 1

    eager = pipe.inpaint(ctx2, u8, mask, s, st, gd, noise=(n1, n2), step_noise=sn)
    assert torch.equal(pipe.inpaint_graphed(ctx2, u8, mask, s, st, gd, noise=(n1, n2), step_noise=sn), eager)
    g_fused = pipe._traj[('inpaint', t_enc, int(st), float(gd), True, tuple(u8.shape))][0]
    # captured the way Txt2Img.*_graphed do it (warm-up, then capture with the engine graphs as launch lists), on the same inputs
    g_comp, _, out_comp = pipe._graphed(('composed', t_enc, int(st), float(gd)), [], lambda: composed_inpaint(pipe, ctx2, u8, mask, s, st, gd, (n1, n2), sn))
    g_comp.replay()
    torch.cuda.synchronize()
    composed_equal = bool(torch.equal(out_comp, eager))

    variants = {
        'fused_graph_replay': g_fused.replay,
        'composed_graph_replay': g_comp.replay,
        'inpaint_graphed': lambda: pipe.inpaint_graphed(ctx2, u8, mask, s, st, gd, seed=seed),
        'inpaint_graphed_injected_noise': lambda: pipe.inpaint_graphed(ctx2, u8, mask, s, st, gd, noise=(n1, n2), step_noise=sn),
        'img2img_graphed': lambda: pipe.img2img_graphed(ctx2, u8, s, st, gd, seed=seed),
    }
    times = {k: [] for k in variants}
    for it in range(a.warmup + a.iters):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))

    def summary(v):
        v = sorted(v)
        return {'ms_per_image': round(statistics.median(v), 3), 'min': round(v[0], 3), 'p90': round(v[int(0.9 * (len(v) - 1))], 3)}

    res = {'device': torch.cuda.get_device_name(0), 'strength': s, 'steps': st, 'unet_evals': t_enc, 'image': '512x512', 'iters': a.iters,
           'composed_equals_inpaint_bit_for_bit': composed_equal}
    res.update({k: summary(v) for k, v in times.items()})
    # the pair, iteration by iteration (the two replays of one iteration run back to back): composed - fused
    d = sorted(c - f for f, c in zip(times['fused_graph_replay'], times['composed_graph_replay']))
    res['composed_minus_fused_ms'] = {'median': round(statistics.median(d), 3), 'p10': round(d[int(0.1 * (len(d) - 1))], 3),
                                      'p90': round(d[int(0.9 * (len(d) - 1))], 3), 'fused_faster_in': sum(1 for v in d if v > 0), 'of': len(d)}
    res['wall_s'] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
