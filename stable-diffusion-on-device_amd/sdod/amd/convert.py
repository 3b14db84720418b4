"""Real-checkpoint loader: a CompVis Stable Diffusion v1.x checkpoint (`sd-v1-4.ckpt` or its
`.safetensors` twin) -> the four weight containers libsdod_setup / Txt2Img(models_dir=...) read.

The reference never touches a checkpoint at run time: its models arrive as serialized QNN graphs made offline by
`todlc.py` from ONNX exports of the ldm model (README.md:60-65, context.cpp:105-115).  This module is the same offline
step for the MI355X build.  It runs on a host without a GPU: the engine's parameter tables are host-side metadata.

    python -m sdod.amd.convert --ckpt sd-v1-4.ckpt --out models/          # + --tokenizer-vocab bpe_simple_vocab_16e6.txt.gz

    python -m sdod.amd.convert --adapter t2iadapter_canny_sd14v1.pth --out models/     # adapter.sdodw (Txt2Img(adapter=True))

Only loaders that execute nothing from the file are used: safetensors, or torch.load(weights_only=True).
"""
import argparse
import os

import torch

from . import engine as E
from . import weights

# graph -> (prefix inside an ldm checkpoint, container file stem in models_dir)
GRAPHS = {
    'unet': ('model.diffusion_model.', 'unet'),
    'temb': ('model.diffusion_model.', 'temb'),          # time MLP + every ResBlock's emb_layers projection (TEMB graph)
    'vae': ('first_stage_model.', 'vae_decoder'),
    'text': ('cond_stage_model.transformer.', 'text_encoder'),
}


def read_checkpoint(path):
    """-> flat {name: tensor}.  `.safetensors` through safetensors; anything else through torch.load(weights_only=True)
    (which refuses pickled code); a top-level 'state_dict' entry (ldm / lightning checkpoints) is unwrapped."""
    if path.endswith('.safetensors'):
        from safetensors.torch import load_file
        return load_file(path, device='cpu')
    sd = torch.load(path, map_location='cpu', weights_only=True, mmap=True)
    if isinstance(sd, dict) and 'state_dict' in sd and isinstance(sd['state_dict'], dict):
        sd = sd['state_dict']
    return sd


# opt-in graphs (convert --vae-encoder): not part of the txt2img containers, so the default tables, splits and files are unchanged
OPTIONAL_GRAPHS = {
    'vae_enc': ('first_stage_model.', 'vae_encoder'),    # encoder.* + quant_conv.*: the img2img path (Txt2Img(with_vae_encoder=True))
}

# SD v2.x (public ldm v2 checkpoints): same UNet / VAE prefixes, the text tower is open_clip's model under `.model.`
GRAPHS_SD21 = dict(GRAPHS, text=('cond_stage_model.model.', 'text_encoder'))


def parameter_tables(cfg=None):
    """{graph: [(name, shape), ...]} of the graphs for `cfg` (default SD v1.x; E.sd21_config() for SD v2.1); no device needed"""
    cfg = cfg or E.sd14_config()
    return {'unet': E.UNet(cfg, 2).param_table(), 'temb': E.Temb(cfg, 1).param_table(),
            'vae': E.VaeDecoder(cfg, 1).param_table(), 'text': E.TextEncoder(cfg, 1).param_table()}


def vae_encoder_table(cfg=None):
    """[(name, shape), ...] of the VAE encoder graph (img2img; opt-in, see OPTIONAL_GRAPHS); no device needed"""
    return E.VaeEncoder(cfg or E.sd14_config(), 1).param_table()


def split_state_dict(sd, tables=None, dtype=torch.float16):
    """Pick every graph's parameters out of a full checkpoint state dict.  Raises KeyError naming what is missing and
    ValueError on a shape mismatch; entries the graphs do not use (EMA copies, the VAE encoder, position_ids,
    loss / scheduler buffers) are ignored.  Returns ({graph: {name: tensor}}, [unused keys])."""
    tables = tables or parameter_tables()
    names = {n for n, _ in tables.get('text', [])}
    prefixes = dict(GRAPHS_SD21 if 'ln_final.weight' in names else GRAPHS, **OPTIONAL_GRAPHS)  # open_clip text tower => SD2.x
    out, used, missing = {}, set(), []
    for graph, table in tables.items():
        prefix = prefixes[graph][0]
        part = {}
        for name, shape in table:
            key = prefix + name
            if key not in sd and graph == 'text' and name.startswith('text_model.') and prefix + name[len('text_model.'):] in sd:
                key = prefix + name[len('text_model.'):]          # transformers >= 5 drops the text_model. level
            if key not in sd:
                missing.append(key)
                continue
            t = sd[key]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f'{key}: checkpoint shape {tuple(t.shape)} != graph shape {tuple(shape)}')
            part[name] = t.to(dtype) if t.is_floating_point() else t.float().to(dtype)
            used.add(key)
        out[graph] = part
    if missing:
        raise KeyError(f'{len(missing)} parameter(s) missing from the checkpoint, e.g. {missing[:5]}')
    return out, sorted(k for k in sd if k not in used)


def convert(ckpt_path, out_dir, dtype=torch.float16, cfg=None, vae_encoder=False):
    """checkpoint file -> out_dir/{unet,temb,vae_decoder,text_encoder}.sdodw (+ vae_encoder.sdodw with vae_encoder=True);
    returns the list of files written"""
    tables = parameter_tables(cfg)
    if vae_encoder:
        tables = dict(tables, vae_enc=vae_encoder_table(cfg))
    parts, _ = split_state_dict(read_checkpoint(ckpt_path), tables, dtype)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for graph, part in parts.items():
        path = os.path.join(out_dir, dict(GRAPHS, **OPTIONAL_GRAPHS)[graph][1] + '.sdodw')
        weights.save(path, part)
        written.append(path)
    return written


def adapter_config(sd):
    """(hint_channels, nums_rb) of a TencentARC T2I-Adapter state dict of the kind the engine builds -- the "full" SD 1.x adapters,
    Adapter(channels=[320, 640, 1280, 1280], nums_rb, ksize=1, sk=True, use_conv=False): hint_channels = conv_in.weight.shape[1] // 64,
    nums_rb = (highest body.K + 1) // 4.  Every other layout is refused by name with ValueError: diffusers-format keys
    (adapter.body.N.resnets.*), Adapter_light (body.N.body.M.*: the color adapter), sk=False (body.K.skep), use_conv=True
    (body.K.down_opt.op) and a block2 that is not 1x1 (ksize=3)."""
    import re
    keys = list(sd)
    if any(re.match(r'(adapter\.)?body\.\d+\.resnets\.', k) or k.startswith('adapter.') for k in keys):
        raise ValueError('diffusers-format adapter keys (adapter.body.N.resnets.*): convert the original TencentARC .pth checkpoint')
    if any(re.match(r'body\.\d+\.body\.\d+\.', k) for k in keys):
        raise ValueError('Adapter_light checkpoint (keys body.N.body.M.*: the color adapter) is not supported')
    if any(re.match(r'body\.\d+\.skep\.', k) for k in keys):
        raise ValueError('adapter built with sk=False (keys body.K.skep.*) is not supported')
    if any(re.match(r'body\.\d+\.down_opt\.op\.', k) for k in keys):
        raise ValueError('adapter built with use_conv=True (keys body.K.down_opt.op.*) is not supported')
    if 'conv_in.weight' not in sd:
        raise ValueError('not a T2I-Adapter state dict: conv_in.weight is missing')
    cin = int(sd['conv_in.weight'].shape[1])
    if cin not in (64, 192):
        raise ValueError(f'conv_in.weight takes {cin} channels: hints of 1 or 3 channels (64 or 192 after the unshuffle) are supported')
    blocks = sorted({int(m.group(1)) for m in (re.match(r'body\.(\d+)\.', k) for k in keys) if m})
    if not blocks or blocks != list(range(blocks[-1] + 1)) or (blocks[-1] + 1) % 4:
        raise ValueError(f'body.K blocks {blocks[:3]}..{blocks[-1:]} are not four stages of equally many blocks')
    for k in blocks:
        w = sd.get(f'body.{k}.block2.weight')
        if w is None or tuple(w.shape[2:]) != (1, 1):
            raise ValueError(f'body.{k}.block2.weight must be a 1x1 convolution (ksize=1), got {None if w is None else tuple(w.shape)}')
    return cin // 64, (blocks[-1] + 1) // 4


def adapter_table(hint_channels, nums_rb=2, cfg=None):
    """[(name, shape), ...] of the ADAPTER graph; no device needed"""
    cfg = E.copy_config(cfg or E.sd14_config())
    cfg.adapter_hint_channels, cfg.adapter_res_blocks = hint_channels, nums_rb
    return E.Adapter(cfg, 1).param_table()


def convert_adapter(path, out_dir, dtype=torch.float16):
    """a TencentARC t2iadapter_*_sd14v1 / sd15v2 .pth -> out_dir/adapter.sdodw; returns the file written"""
    sd = read_checkpoint(path)
    hint_channels, nums_rb = adapter_config(sd)
    part = {}
    for name, shape in adapter_table(hint_channels, nums_rb):
        if name not in sd:
            raise KeyError(f'{name} is missing from the adapter checkpoint')
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f'{name}: checkpoint shape {tuple(sd[name].shape)} != graph shape {tuple(shape)}')
        part[name] = sd[name].to(dtype)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, 'adapter.sdodw')
    weights.save(out, part)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--ckpt', help='sd-v1-x .ckpt / .safetensors (ldm key names)')
    ap.add_argument('--adapter', help='a TencentARC T2I-Adapter checkpoint (t2iadapter_{canny,depth,sketch,seg,openpose,keypose}_sd14v1.pth): '
                                      'write adapter.sdodw (Txt2Img(adapter=True)); with or without --ckpt')
    ap.add_argument('--out', required=True, help='models_dir to write')
    ap.add_argument('--fp32', action='store_true', help='keep fp32 payloads (the engine converts at load)')
    ap.add_argument('--model', default='sd14', choices=['sd14', 'sd21'], help='sd21: SD v2.x shapes and open_clip text-tower key names')
    ap.add_argument('--vae-encoder', action='store_true', help='also write vae_encoder.sdodw (first_stage_model.encoder + '
                                                                'quant_conv), the img2img path')
    ap.add_argument('--inpaint', action='store_true', help='an inpainting checkpoint (sd-v1-5-inpainting, 512-inpainting-ema): the UNet input '
                                                            'convolution is [320, 9, 3, 3]; implies --vae-encoder (Txt2Img(inpaint_unet=True))')
    ap.add_argument('--tokenizer-vocab', help='bpe_simple_vocab_16e6.txt.gz, or a directory with HF vocab.json + merges.txt: '
                                              'also write ctokenizer.txt')
    a = ap.parse_args(argv)
    if not a.ckpt and not a.adapter:
        ap.error('one of --ckpt and --adapter is required')
    cfg = E.sd21_config() if a.model == 'sd21' else None
    if a.inpaint:
        cfg = cfg or E.sd14_config()
        cfg.concat_channels = 5
    if a.ckpt:
        for p in convert(a.ckpt, a.out, torch.float32 if a.fp32 else torch.float16, cfg, vae_encoder=a.vae_encoder or a.inpaint):
            print('wrote', p)
    if a.adapter:
        print('wrote', convert_adapter(a.adapter, a.out, torch.float32 if a.fp32 else torch.float16))
    if a.tokenizer_vocab:
        from . import tokenizer_file
        print('wrote', tokenizer_file.generate(a.tokenizer_vocab, os.path.join(a.out, 'ctokenizer.txt')))


if __name__ == '__main__':
    main()
