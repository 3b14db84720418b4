"""Real-checkpoint loader: a CompVis Stable Diffusion v1.x checkpoint (`sd-v1-4.ckpt` or its
`.safetensors` twin) -> the four weight containers libsdod_setup / Txt2Img(models_dir=...) read.

The reference never touches a checkpoint at run time: its models arrive as serialized QNN graphs made offline by
`todlc.py` from ONNX exports of the ldm model (README.md:60-65, context.cpp:105-115).  This module is the same offline
step for the MI355X build.  It runs on a host without a GPU: the engine's parameter tables are host-side metadata.

    python -m sdod.amd.convert --ckpt sd-v1-4.ckpt --out models/          # + --tokenizer-vocab bpe_simple_vocab_16e6.txt.gz

    python -m sdod.amd.convert --adapter t2iadapter_canny_sd14v1.pth --out models/     # adapter.sdodw (Txt2Img(adapter=True))

    python -m sdod.amd.convert --upscaler RealESRGAN_x4plus.pth --out models/          # upscaler.sdodw (Txt2Img(upscaler=True))

    python -m sdod.amd.convert --controlnet control_v11p_sd15_canny.pth --out models/  # controlnet.sdodw (Txt2Img(controlnet=True))

    python -m sdod.amd.convert --ip-adapter ip-adapter_sd15.safetensors --out models/  # ip_adapter.sdodw (Txt2Img(ip_adapter=True))
    python -m sdod.amd.convert --image-encoder image_encoder/ --out models/            # image_encoder.sdodw (CLIP ViT-H/14, optional)

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


# the one key of a full LCM checkpoint that ldm's naming has no place for: diffusers' name (a UNet already translated to ldm names keeps
# it, or carries it under ours) -> the TEMB graph's parameter
LCM_COND_PROJ_KEYS = ('time_embedding.cond_proj.weight', 'model.diffusion_model.time_embedding.cond_proj.weight')


def convert(ckpt_path, out_dir, dtype=torch.float16, cfg=None, vae_encoder=False, guidance_embed=False):
    """checkpoint file -> out_dir/{unet,temb,vae_decoder,text_encoder}.sdodw (+ vae_encoder.sdodw with vae_encoder=True);
    returns the list of files written.  guidance_embed=True: a full LCM checkpoint -- temb.sdodw also gets
    time_embed.cond_proj.weight [model_channels, 256] (Txt2Img(unguided=True, guidance_embed=True)), read from
    model.diffusion_model.time_embed.cond_proj.weight or, renamed, from diffusers' time_embedding.cond_proj.weight."""
    tables = parameter_tables(cfg)
    if vae_encoder:
        tables = dict(tables, vae_enc=vae_encoder_table(cfg))
    sd = read_checkpoint(ckpt_path)
    if guidance_embed:
        tables = dict(tables, temb=E.Temb(cfg or E.sd14_config(), 1, cond_proj_dim=E.LCM_COND_PROJ_DIM).param_table())
        ours = GRAPHS['temb'][0] + 'time_embed.cond_proj.weight'
        for key in LCM_COND_PROJ_KEYS:
            if ours not in sd and key in sd:
                sd = dict(sd)
                sd[ours] = sd[key]
    parts, _ = split_state_dict(sd, tables, dtype)
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


UPSCALER_TOP = ('conv_first', 'conv_body', 'conv_up1', 'conv_up2', 'conv_hr', 'conv_last')
# the same network under the original ESRGAN repository's two namings -> basicsr's (the graph's)
_ESRGAN_NEW_ARCH = {'trunk_conv': 'conv_body', 'upconv1': 'conv_up1', 'upconv2': 'conv_up2', 'HRconv': 'conv_hr'}
_ESRGAN_OLD_ARCH = {'model.0': 'conv_first', 'model.3': 'conv_up1', 'model.6': 'conv_up2', 'model.8': 'conv_hr', 'model.10': 'conv_last'}


def upscaler_state_dict(sd):
    """An ESRGAN / Real-ESRGAN x4 RRDBNet state dict under any of its three namings -> (basicsr-named dict, num_blocks).  A
    `params_ema` or `params` wrapper is unwrapped.  Accepted: basicsr / Real-ESRGAN (conv_first, body.N.rdbK.convJ, conv_body, conv_up1,
    conv_up2, conv_hr, conv_last), the original ESRGAN "new arch" (RRDB_trunk.N.RDBk.convJ, trunk_conv, upconv1, upconv2, HRconv) and
    its "old arch" (model.0, model.1.sub.N.RDBk.convJ.0, model.1.sub.<nb> for the trunk convolution, model.3, model.6, model.8,
    model.10).  Refused by name with ValueError: x2 and x1 models, feature / growth widths other than 64 / 32, SRVGGNetCompact keys,
    anything without conv_first or model.0."""
    import re
    for wrap in ('params_ema', 'params'):
        if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    keys = list(sd)
    if any(re.match(r'body\.\d+\.(weight|bias)$', k) for k in keys):
        raise ValueError('SRVGGNetCompact keys (body.N.weight): the compact Real-ESRGAN networks are not supported, only RRDBNet')
    out = {}
    if 'conv_first.weight' in sd and any(k.startswith('body.') for k in keys):
        out = dict(sd)
    elif 'conv_first.weight' in sd and any(k.startswith('RRDB_trunk.') for k in keys):
        for k, v in sd.items():
            m = re.match(r'RRDB_trunk\.(\d+)\.RDB(\d)\.conv(\d)\.(weight|bias)$', k)
            if m:
                out[f'body.{m.group(1)}.rdb{m.group(2)}.conv{m.group(3)}.{m.group(4)}'] = v
                continue
            stem, _, leaf = k.rpartition('.')
            out[_ESRGAN_NEW_ARCH.get(stem, stem) + '.' + leaf] = v
    elif 'model.0.weight' in sd:
        subs = sorted({int(m.group(1)) for m in (re.match(r'model\.1\.sub\.(\d+)\.', k) for k in keys) if m})
        if not subs:
            raise ValueError('old-arch ESRGAN keys without model.1.sub.N: not an RRDBNet')
        nb = subs[-1]                                   # model.1.sub.<nb> is the trunk convolution behind blocks 0 .. nb - 1
        for k, v in sd.items():
            m = re.match(r'model\.1\.sub\.(\d+)\.RDB(\d)\.conv(\d)\.0\.(weight|bias)$', k)
            if m:
                out[f'body.{m.group(1)}.rdb{m.group(2)}.conv{m.group(3)}.{m.group(4)}'] = v
                continue
            stem, _, leaf = k.rpartition('.')
            if stem == f'model.1.sub.{nb}':
                out['conv_body.' + leaf] = v
            else:
                out[_ESRGAN_OLD_ARCH.get(stem, stem) + '.' + leaf] = v
    else:
        raise ValueError('not an ESRGAN RRDBNet state dict: neither conv_first.weight nor model.0.weight is present')
    cf = out['conv_first.weight']
    if cf.dim() == 4 and int(cf.shape[1]) == 12:
        raise ValueError('x2 model (conv_first takes 12 channels, the pixel-unshuffled input): only x4 models are supported')
    if cf.dim() == 4 and int(cf.shape[1]) == 48:
        raise ValueError('x1 model (conv_first takes 48 channels, the pixel-unshuffled input): only x4 models are supported')
    if 'conv_up2.weight' not in out:
        raise ValueError('x1 / x2 model (no conv_up2): only x4 models are supported')
    if cf.dim() != 4 or tuple(cf.shape[1:]) != (3, 3, 3):
        raise ValueError(f'conv_first.weight has shape {tuple(cf.shape)}, expected [64, 3, 3, 3]')
    g = out.get('body.0.rdb1.conv1.weight')
    if int(cf.shape[0]) != 64 or g is None or int(g.shape[0]) != 32:
        raise ValueError(f'feature / growth widths {int(cf.shape[0])} / {None if g is None else int(g.shape[0])}: only 64 / 32 is supported')
    blocks = sorted({int(m.group(1)) for m in (re.match(r'body\.(\d+)\.', k) for k in out) if m})
    if blocks != list(range(len(blocks))) or not 1 <= len(blocks) <= 23:
        raise ValueError(f'body.N blocks {blocks[:3]}..{blocks[-1:]}: 1 to 23 consecutive blocks are supported')
    return out, len(blocks)


def upscaler_table(num_blocks):
    """[(name, shape), ...] of the UPSCALER graph; no device needed"""
    return E.Upscaler(num_blocks, (8, 8), 1).param_table()


def upscaler_parameters(sd, dtype=torch.float16):
    """a state dict as upscaler_state_dict takes it -> ({graph name: tensor of `dtype`}, num_blocks), every shape checked"""
    sd, nb = upscaler_state_dict(sd)
    part = {}
    for name, shape in upscaler_table(nb):
        if name not in sd:
            raise KeyError(f'{name} is missing from the upscaler checkpoint')
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f'{name}: checkpoint shape {tuple(sd[name].shape)} != graph shape {tuple(shape)}')
        part[name] = sd[name].to(dtype)
    return part, nb


def convert_upscaler(path, out_dir, dtype=torch.float16):
    """an ESRGAN_4x / RealESRGAN_x4plus(.pth, .safetensors) checkpoint -> out_dir/upscaler.sdodw; returns the file written"""
    part, _ = upscaler_parameters(read_checkpoint(path), dtype)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, 'upscaler.sdodw')
    weights.save(out, part)
    return out


def controlnet_tables(cfg=None):
    """{'controlnet': ..., 'temb': ..., 'hint': ...}: the parameter tables of the three graphs a ControlNet checkpoint feeds (control
    graph, control TEMB, hint encoder -- the last with its PADDED shapes); no device needed"""
    cfg = E.copy_config(cfg or E.sd14_config())
    tcfg = E.copy_config(cfg)
    tcfg.control_temb = 1
    return {'controlnet': E.ControlNet(cfg, 2).param_table(), 'temb': E.Temb(tcfg, 1).param_table(), 'hint': E.ControlHint(cfg, 1).param_table()}


def controlnet_state_dict(sd):
    """A ControlNet 1.0 / 1.1 state dict for SD 1.x in ldm's (cldm's) naming -> the same tensors with `control_model.` stripped;
    entries outside that prefix (a full control_sd15_*.pth also carries the base model) are dropped.  Refused by name with ValueError:
    diffusers-format keys (controlnet_cond_embedding.*, down_blocks.*), a context width other than 768 (an SD 2.x ControlNet), a hint
    convolution that does not take 3 channels, anything without input_hint_block / zero_convs."""
    keys = list(sd)
    if any(k.startswith(('controlnet_cond_embedding.', 'down_blocks.', 'controlnet_down_blocks.', 'mid_block.')) for k in keys):
        raise ValueError('diffusers-format ControlNet keys (controlnet_cond_embedding.*, down_blocks.*): convert the original '
                         'lllyasviel .pth / .safetensors checkpoint (control_model.* names)')
    if any(k.startswith('control_model.') for k in keys):
        sd = {k[len('control_model.'):]: v for k, v in sd.items() if k.startswith('control_model.')}
    if 'input_hint_block.0.weight' not in sd or 'zero_convs.0.0.weight' not in sd:
        raise ValueError('not a ControlNet state dict: input_hint_block.0.weight / zero_convs.0.0.weight are missing')
    kw = sd.get('input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight')
    if kw is None or int(kw.shape[1]) != 768:
        raise ValueError(f'cross-attention context width {None if kw is None else int(kw.shape[1])}: only SD 1.x ControlNets (768) are supported')
    hw = sd['input_hint_block.0.weight']
    if hw.dim() != 4 or int(hw.shape[1]) != 3:
        raise ValueError(f'input_hint_block.0.weight has shape {tuple(hw.shape)}: only 3-channel hints are supported')
    return sd


def controlnet_parameters(sd, dtype=torch.float16):
    """a state dict as controlnet_state_dict takes it -> {name: tensor of `dtype`} for controlnet.sdodw: every tensor the three graphs
    name, shapes checked against the checkpoint's own, the hint encoder's 16 / 32 / 96 channel widths zero-padded to the graph's
    64 / 64 / 128"""
    sd = controlnet_state_dict(sd)
    tables = controlnet_tables()
    want = dict(E.control_hint_checkpoint_table())
    part = {}
    for graph, table in tables.items():
        for name, shape in table:
            if name not in sd:
                raise KeyError(f'{name} is missing from the ControlNet checkpoint')
            t = sd[name]
            ckpt_shape = want[name] if graph == 'hint' else tuple(shape)
            if tuple(t.shape) != tuple(ckpt_shape):
                raise ValueError(f'{name}: checkpoint shape {tuple(t.shape)} != expected {tuple(ckpt_shape)}')
            if tuple(t.shape) != tuple(shape):          # (hint encoder: zero weights and zero bias in the padded channels)
                padded = torch.zeros(tuple(shape), dtype=t.dtype)
                padded[tuple(slice(0, n) for n in t.shape)] = t
                t = padded
            part[name] = t.to(dtype)
    return part


def convert_controlnet(path, out_dir, dtype=torch.float16):
    """a ControlNet 1.0 / 1.1 SD 1.x checkpoint (.pth / .safetensors) -> out_dir/controlnet.sdodw; returns the file written"""
    part = controlnet_parameters(read_checkpoint(path), dtype)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, 'controlnet.sdodw')
    weights.save(out, part)
    return out


def read_ip_adapter(path):
    """an IP-Adapter file -> its state dict: `.safetensors` (flat image_proj.* / ip_adapter.* keys) through safetensors, `.bin` (the
    nested {'image_proj', 'ip_adapter'} dict) through torch.load(weights_only=True)"""
    if path.endswith('.safetensors'):
        from safetensors.torch import load_file
        return load_file(path, device='cpu')
    return torch.load(path, map_location='cpu', weights_only=True)


def convert_ip_adapter(path, out_dir, dtype=torch.float16):
    """ip-adapter_sd15.{bin,safetensors} -> out_dir/ip_adapter.sdodw (ip_adapter.adapter_parameters); returns the file written"""
    from . import ip_adapter as IP
    part = IP.adapter_parameters(read_ip_adapter(path), dtype)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, 'ip_adapter.sdodw')
    weights.save(out, part)
    return out


def convert_image_encoder(path, out_dir, dtype=torch.float16):
    """an HF CLIPVisionModelWithProjection checkpoint (model.safetensors / pytorch_model.bin, or the directory that holds one) ->
    out_dir/image_encoder.sdodw (ip_adapter.image_encoder_parameters); returns the file written"""
    from . import ip_adapter as IP
    if os.path.isdir(path):
        found = [os.path.join(path, n) for n in ('model.safetensors', 'pytorch_model.bin') if os.path.exists(os.path.join(path, n))]
        if not found:
            raise ValueError(f'{path} holds neither model.safetensors nor pytorch_model.bin')
        path = found[0]
    part = IP.image_encoder_parameters(read_checkpoint(path), dtype)
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, 'image_encoder.sdodw')
    weights.save(out, part)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--ckpt', help='sd-v1-x .ckpt / .safetensors (ldm key names)')
    ap.add_argument('--adapter', help='a TencentARC T2I-Adapter checkpoint (t2iadapter_{canny,depth,sketch,seg,openpose,keypose}_sd14v1.pth): '
                                      'write adapter.sdodw (Txt2Img(adapter=True)); with or without --ckpt')
    ap.add_argument('--upscaler', help='an ESRGAN x4 RRDBNet checkpoint (ESRGAN_4x, RealESRGAN_x4plus, the 6-block anime model; basicsr or '
                                       'original ESRGAN key names): write upscaler.sdodw (Txt2Img(upscaler=True)); with or without --ckpt')
    ap.add_argument('--controlnet', help='a ControlNet 1.0 / 1.1 checkpoint for SD 1.x (control_sd15_*.pth, control_v11*_sd15_*.pth / '
                                         '.safetensors; control_model.* names): write controlnet.sdodw (Txt2Img(controlnet=True)); with or '
                                         'without --ckpt')
    ap.add_argument('--ip-adapter', help='ip-adapter_sd15.bin / .safetensors (IP-Adapter for SD 1.x, not the "plus" or FaceID files): write '
                                         'ip_adapter.sdodw (Txt2Img(ip_adapter=True)); with or without --ckpt')
    ap.add_argument('--image-encoder', help='the IP-Adapter image encoder, an HF CLIPVisionModelWithProjection model.safetensors or its '
                                            'directory: write image_encoder.sdodw')
    ap.add_argument('--out', required=True, help='models_dir to write')
    ap.add_argument('--fp32', action='store_true', help='keep fp32 payloads (the engine converts at load)')
    ap.add_argument('--model', default='sd14', choices=['sd14', 'sd21'], help='sd21: SD v2.x shapes and open_clip text-tower key names')
    ap.add_argument('--vae-encoder', action='store_true', help='also write vae_encoder.sdodw (first_stage_model.encoder + '
                                                                'quant_conv), the img2img path')
    ap.add_argument('--inpaint', action='store_true', help='an inpainting checkpoint (sd-v1-5-inpainting, 512-inpainting-ema): the UNet input '
                                                            'convolution is [320, 9, 3, 3]; implies --vae-encoder (Txt2Img(inpaint_unet=True))')
    ap.add_argument('--guidance-embed', action='store_true', help='a full LCM checkpoint (LCM_Dreamshaper_v7): temb.sdodw also gets '
                                                                   'time_embed.cond_proj.weight, renamed from diffusers\' '
                                                                   'time_embedding.cond_proj.weight (Txt2Img(guidance_embed=True))')
    ap.add_argument('--tokenizer-vocab', help='bpe_simple_vocab_16e6.txt.gz, or a directory with HF vocab.json + merges.txt: '
                                              'also write ctokenizer.txt')
    a = ap.parse_args(argv)
    if not a.ckpt and not a.adapter and not a.upscaler and not a.controlnet and not a.ip_adapter and not a.image_encoder:
        ap.error('one of --ckpt, --adapter, --upscaler, --controlnet, --ip-adapter and --image-encoder is required')
    cfg = E.sd21_config() if a.model == 'sd21' else None
    if a.inpaint:
        cfg = cfg or E.sd14_config()
        cfg.concat_channels = 5
    if a.ckpt:
        for p in convert(a.ckpt, a.out, torch.float32 if a.fp32 else torch.float16, cfg, vae_encoder=a.vae_encoder or a.inpaint,
                         guidance_embed=a.guidance_embed):
            print('wrote', p)
    if a.adapter:
        print('wrote', convert_adapter(a.adapter, a.out, torch.float32 if a.fp32 else torch.float16))
    if a.upscaler:
        print('wrote', convert_upscaler(a.upscaler, a.out, torch.float32 if a.fp32 else torch.float16))
    if a.controlnet:
        print('wrote', convert_controlnet(a.controlnet, a.out, torch.float32 if a.fp32 else torch.float16))
    if a.ip_adapter:
        print('wrote', convert_ip_adapter(a.ip_adapter, a.out, torch.float32 if a.fp32 else torch.float16))
    if a.image_encoder:
        print('wrote', convert_image_encoder(a.image_encoder, a.out, torch.float32 if a.fp32 else torch.float16))
    if a.tokenizer_vocab:
        from . import tokenizer_file
        print('wrote', tokenizer_file.generate(a.tokenizer_vocab, os.path.join(a.out, 'ctokenizer.txt')))


if __name__ == '__main__':
    main()
