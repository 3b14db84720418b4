"""Fingerprint of everything the graph builders (csrc/graphs.hip, the emitters of csrc/engine.hip) decide: for every graph kind, at
the smallest sizes that reach every branch of the builders, one JSON line with the ordered parameter table, the launch list (label,
flops, bytes, detail), stats() and a SHA-256 of every output after an eager execute() and after two hipGraph replays.  Two builds
whose lines are equal build the same graphs and compute the same bits: run it on both sides of a builder change and diff.

    python tools/graph_fingerprint.py --tree OTHER_CHECKOUT > a.jsonl ; python tools/graph_fingerprint.py > b.jsonl ; diff a.jsonl b.jsonl

--tree: the checkout (built) whose package is imported; default: the one this file is in.  --declare-only: parameter tables only, no
device.  SDOD_AUTOTUNE=0 is set: the static tile plan decides and nothing is timed, so the launch list is the same in every process.
SDOD_COMPOSE and SDOD_XATTN_FOLD are read once per process, so after its own graphs a full run starts this file three more times
(COMPOSE=0, XATTN_FOLD=0, both) on the two UNets that have both forms of cross-attention; the switches are part of every line."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

SWITCHES = ('SDOD_COMPOSE', 'SDOD_XATTN_FOLD')
SWITCHED = ['unet_sd14', 'unet_sd21']


def cases(E):
    """name -> (constructor, input attributes, output attributes).  sd14 UNet at 16x16: levels 0 and 1 take the folded cross-attention
    (L = 256, 64), levels 2, 3 and the middle the plain one with composition (L = 16, 4); sd21 at 32x32 folds at level 2 only."""
    def sd14(hw, wq=0, **kw):
        cfg = E.sd14_config(hw, hw, **kw)
        cfg.weight_quant = wq
        return cfg
    unet_io = (['x', 'temb', 'ctx'], ['eps'])
    out = {
        'unet_sd14': (lambda: E.UNet(sd14(16), 2),) + unet_io,
        'unet_sd14_wq1': (lambda: E.UNet(sd14(16, 1), 2),) + unet_io,
        'unet_sd14_wq2': (lambda: E.UNet(sd14(16, 2), 2),) + unet_io,
        'unet_sd14_concat5': (lambda: E.UNet(sd14(16, concat_channels=5), 2), ['x', 'temb', 'ctx', 'cond'], ['eps']),
        'unet_sd14_adapter2': (lambda: E.UNet(sd14(16, adapter_reps=2), 2), ['x', 'temb', 'ctx', 'adapter_feat'], ['eps']),
        'unet_sd14_wrap3': (lambda: E.UNet(sd14(16), 2, wrap=3),) + unet_io,
        'unet_sd21': (lambda: E.UNet(E.sd21_config(32, 32), 2),) + unet_io,
        'temb_sd14': (lambda: E.Temb(sd14(16), 2), ['t'], ['out']),
        'text_sd14': (lambda: E.TextEncoder(sd14(16), 2), ['ids'], ['out']),
        'text_sd21': (lambda: E.TextEncoder(E.sd21_config(32, 32), 2), ['ids'], ['out']),
        'vae_decoder': (lambda: E.VaeDecoder(sd14(8), 1, wrap=0), ['z'], ['img']),
        'vae_decoder_wrap3': (lambda: E.VaeDecoder(sd14(8), 1, wrap=3), ['z'], ['img']),
        'vae_encoder': (lambda: E.VaeEncoder(sd14(8), 1), ['img'], ['moments']),
        'vae_encoder_masked': (lambda: E.MaskedVaeEncoder(sd14(8), 1), ['img', 'mask'], ['moments']),
        'adapter_hint1': (lambda: E.Adapter(sd14(16, adapter_hint_channels=1), 1), ['hint'], ['out']),
        'adapter_hint3': (lambda: E.Adapter(sd14(16, adapter_hint_channels=3), 1), ['hint'], ['out']),
        'upscaler_nb1': (lambda: E.Upscaler(1, (16, 16), 1), ['img'], ['out']),
    }
    return out


def tensors(g, names):
    out = []
    for n in names:
        v = getattr(g, n)
        out += list(v) if isinstance(v, (list, tuple)) else [v]
    return out


def fill(g, names, torch, seed):
    gen = torch.Generator().manual_seed(seed)
    for t in tensors(g, names):
        if t.dtype == torch.uint8:
            v = torch.randint(0, 256, t.shape, generator=gen, dtype=torch.uint8)
        elif t.dtype == torch.int32:      # token ids
            v = torch.randint(0, g.cfg.vocab_size, t.shape, generator=gen, dtype=torch.int32)
        elif t.dim() == 1:                # timesteps
            v = torch.rand(t.shape, generator=gen) * 999.0
        else:
            v = torch.randn(t.shape, generator=gen) * 0.5
        t.copy_(v.to(t.dtype))


def digests(g, names, torch):
    torch.cuda.synchronize()
    return [hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for t in tensors(g, names)]


def fingerprint(name, case, declare_only, torch, Wt):
    make, ins, outs = case
    g = make()
    table = g.param_table()
    rec = {'graph': name, 'switches': {k: os.environ.get(k, '') for k in SWITCHES}, 'params': [[n, list(s)] for n, s in table]}
    if declare_only:
        return rec
    seed = 4000 + sum(name.encode())
    sd = Wt.synthetic_state_dict(table, seed)
    g.load_state_dict(Wt.quantize_state_dict(sd) if getattr(g.cfg, 'weight_quant', 0) else sd)
    g.finalize()
    fill(g, ins, torch, seed + 1)
    g.execute()
    rec['sha256_eager'] = digests(g, outs, torch)
    rec['finite'] = all(bool(torch.isfinite(t.float()).all()) for t in tensors(g, outs))    # (a hash of NaNs would compare equal too)
    for t in tensors(g, outs):
        t.zero_()
    g.execute(use_hip_graph=True)
    g.execute(use_hip_graph=True)
    rec['sha256_replay'] = digests(g, outs, torch)
    rec.update(ops=[list(o) for o in g.op_table()], details=g.op_details(), stats=g.stats())
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument('--tree', default=here, help='checkout to import the package from (default: this one)')
    ap.add_argument('--declare-only', action='store_true', help='parameter tables only; needs no device')
    ap.add_argument('--only', nargs='*', help='graph names; no switch runs are started')
    args = ap.parse_args()
    os.environ['SDOD_AUTOTUNE'] = '0'
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), 'stable-diffusion-on-device_amd'))
    import torch
    from sdod.amd import engine as E, weights as Wt
    print('# package under test:', os.path.dirname(E.__file__), file=sys.stderr)
    all_cases = cases(E)
    for name in args.only or all_cases:
        print(json.dumps(fingerprint(name, all_cases[name], args.declare_only, torch, Wt), sort_keys=True), flush=True)
    if args.only is None and not args.declare_only:
        for off in (SWITCHES[:1], SWITCHES[1:], SWITCHES):      # a fresh process each: the library reads the switches once
            env = dict(os.environ, **{k: '0' for k in off})
            subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', args.tree, '--only'] + SWITCHED, env=env, check=True, timeout=600)


if __name__ == '__main__':
    main()
