#!/usr/bin/env python3
"""What an image prompt (IP-Adapter) costs on one MI355X (synthetic SD v1.4 weights, 64 x 64 latent, one image = a guidance batch of
2): a pipeline built without the feature next to one built with ip_adapter=True, in one process:

  * one guided evaluation (the captured launch lists, static inputs unchanged) -- without / with an image prompt / built and cleared;
  * generate_graphed, 20 PLMS steps, the same three;
  * one set_image_prompt call at ViT-H/14 shapes (224 x 224, 32 layers, 1024-wide embeddings, 4 tokens), with the encoder
    (image_u8) and without it (embeds), host clock around a device synchronise;
  * launch counts, arena and weight bytes.

The variants are timed alternately, `rounds` times; the medians and the spread of the rounds are reported.  At 64 x 64 every level
folds (L = 4096, 1024, 256, 64), so the only launches that differ are the two cross-attention GEMMs of each of the 16 transformer
blocks, twice as wide -- the shapes of two regional prompts.  Not the benchmark (bench.py measures the flagship txt2img workload);
the record behind DESIGN.md 6l and INTEGRATION.md's "Image prompts".  No threshold is attached to it.

usage (GPU box):  python tools/ipadapter_bench.py [--rounds 7] [--iters 20] [--out profiles/ipadapter_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'stable-diffusion-on-device_amd'))

import torch  # noqa: E402

from sdod.amd import engine as E, ip_adapter as IP, weights as Wt  # noqa: E402
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
    ap.add_argument('--iters', type=int, default=20, help='evaluations per timed window (generate_graphed: a quarter of it)')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    a = ap.parse_args()
    t0 = time.time()
    cfg = E.sd14_config(64, 64)
    vision = E.vit_h14_config()
    tables = {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(), 'vae': E.VaeDecoder(cfg, 1).param_table()}
    sds = {k: Wt.synthetic_state_dict(t, seed=1234 + i) for i, (k, t) in enumerate(tables.items())}
    icfg = E.copy_config(cfg)
    icfg.ip_tokens = 4
    ip = Wt.synthetic_state_dict([p for p in E.UNet(icfg, 2).param_table() if '_ip.' in p[0]], seed=1240)
    ip.update(Wt.synthetic_state_dict(E.ImageProj(cfg, vision.proj_dim, 4, 2).param_table(), seed=1241))
    enc = Wt.synthetic_state_dict(E.ImageEncoder(vision, 1).checkpoint_table(), seed=1242, dtype=torch.float16)
    enc[IP.CONFIG_KEY] = torch.tensor([getattr(vision, n) for n, _ in E.VisionConfig._fields_], dtype=torch.float32)
    g = torch.Generator().manual_seed(5)
    x_T = torch.randn(1, 4, 64, 64, generator=g).cuda()
    ctx = (0.5 * torch.randn(2, 77, 768, generator=g)).half().cuda()
    image = torch.randint(0, 256, (1, 224, 224, 3), generator=g, dtype=torch.int32).to(torch.uint8)
    kw = dict(images_per_gpu=1, latent_hw=64, with_text_encoder=False)
    pipes = {'without': Txt2Img(state_dicts=sds, **kw),
             'image_prompt': Txt2Img(state_dicts=dict(sds, ip_adapter=ip, image_encoder=enc), ip_adapter=True, **kw),
             'cleared': Txt2Img(state_dicts=dict(sds, ip_adapter=ip), ip_adapter=True, **kw)}
    pipes['image_prompt'].set_image_prompt(image, weight=0.7)
    embeds = pipes['image_prompt'].image_embeds(image)
    pipes['cleared'].set_image_prompt(embeds=embeds, weight=0.7)
    pipes['cleared'].clear_image_prompt()
    for p in pipes.values():
        p._set_context(ctx)
        p.unet.execute(True)
        p.unet.execute(True)

    ev = alternate({n: (lambda p=p: p.unet.execute(True, static_unchanged=True)) for n, p in pipes.items()}, a.rounds, a.iters)

    set_ms = {}
    p = pipes['image_prompt']
    for name, call in (('image_u8', lambda: p.set_image_prompt(image, weight=0.7)), ('embeds', lambda: p.set_image_prompt(embeds=embeds, weight=0.7))):
        ms = []
        for _ in range(a.rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        set_ms[name] = summary(ms[1:])

    gi = max(1, a.iters // 4)
    gen = alternate({n: (lambda p=p: p.generate_graphed(ctx, x_T, a.steps, 7.5, 'plms')) for n, p in pipes.items()}, a.rounds, gi)

    def graph(gr):
        s = gr.stats()
        return {'launches': s['launches'], 'arena_bytes': s['arena_bytes'], 'weight_bytes': s['weight_bytes'], 'tune': gr.tune_source()}

    res = {
        'device': torch.cuda.get_device_name(0), 'latent': [64, 64], 'unet_batch': 2, 'rounds': a.rounds, 'iters': a.iters,
        'guided_evaluation': {n: summary(v) for n, v in ev.items()},
        'set_image_prompt_vit_h14': set_ms,
        'generate_graphed_plms': dict({'steps': a.steps}, **{n: summary(v) for n, v in gen.items()}),
        'graphs': dict({n: graph(p.unet) for n, p in pipes.items()}, image_encoder=graph(pipes['image_prompt'].image_encoder),
                       image_proj=graph(pipes['image_prompt'].image_proj)),
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
