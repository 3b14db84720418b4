"""Image prompts (IP-Adapter for SD 1.x), the host side: the checkpoint's block table, its conversion, and the
argument checks of Txt2Img(ip_adapter=True).

IP-Adapter adds to every cross-attention a second attention on a few image tokens,
    out = to_out(attn(q, K_text, V_text) + s * attn(q, to_k_ip(tokens), to_v_ip(tokens))),
with tokens = ImageProjModel(CLIP image_embeds).  A checkpoint holds `image_proj.*` and `ip_adapter.{1, 3, .., 31}.to_{k,v}_ip.weight`,
the latter numbered by the position of the cross-attention in diffusers' `unet.attn_processors` (BLOCKS below).

Everything here is numpy / torch on the CPU; nothing touches a device."""
import os

import numpy as np
import torch

CTX_DIM = 768
MAX_TOKENS = 16
CONFIG_KEY = 'vision_config'     # image_encoder.sdodw: the eight integers of sdod_vision_config as an fp32 vector

# The ONE table: cross-attention j of the checkpoint (`ip_adapter.{2 j + 1}`) -> (ldm block, width).  diffusers lists the attention
# processors down blocks first, then up blocks, then the middle block; the ldm names follow from the usual diffusers <-> ldm layout.
BLOCKS = ([(f'input_blocks.{i}.1', c) for i, c in zip((1, 2, 4, 5, 7, 8), (320, 320, 640, 640, 1280, 1280))]
          + [(f'output_blocks.{i}.1', c) for i, c in zip(range(3, 12), (1280,) * 3 + (640,) * 3 + (320,) * 3)]
          + [('middle_block.1', 1280)])


def unet_key(j, which):
    """the UNet graph's parameter name for checkpoint index 2 j + 1; which = 'k' or 'v'"""
    return f'{BLOCKS[j][0]}.transformer_blocks.0.attn2.to_{which}_ip.weight'


def flatten(sd):
    """the nested {'image_proj': {...}, 'ip_adapter': {...}} dict of the .bin files -> flat `image_proj.*` / `ip_adapter.*` keys; a
    flat dict (the .safetensors files) passes through"""
    if isinstance(sd, dict) and 'image_proj' in sd and 'ip_adapter' in sd and all(isinstance(sd[k], dict) for k in ('image_proj', 'ip_adapter')):
        return {f'{top}.{k}': v for top in ('image_proj', 'ip_adapter') for k, v in sd[top].items()}
    return dict(sd)


def adapter_parameters(sd, dtype=torch.float16):
    """an ip-adapter_sd15 state dict (either key dialect) -> {name: tensor} for ip_adapter.sdodw: proj.* / norm.* of the IMAGE_PROJ
    graph and the UNet graph's `...attn2.to_{k,v}_ip.weight`.  Refused by name with ValueError: "plus" and FaceID checkpoints
    (image_proj.latents, image_proj.layers.*), SDXL widths, a context width other than 768, any width that does not fit the block
    the table assigns; KeyError for a missing tensor."""
    sd = flatten(sd)
    plus = sorted(k for k in sd if k == 'image_proj.latents' or k.startswith(('image_proj.layers.', 'image_proj.proj_in.', 'image_proj.proj_out.',
                                                                               'image_proj.perceiver_resampler.')))
    if plus:
        raise ValueError(f'an IP-Adapter "plus" / FaceID checkpoint ({plus[0]}): its Resampler image projection is not supported')
    if not any(k.startswith('ip_adapter.') for k in sd) or 'image_proj.proj.weight' not in sd:
        raise ValueError('not an IP-Adapter state dict: image_proj.proj.weight / ip_adapter.* are missing')
    idx = sorted({int(k.split('.')[1]) for k in sd if k.startswith('ip_adapter.')})
    if len(idx) > len(BLOCKS) or 'ip_adapter.1.to_k_ip.weight' in sd and int(sd['ip_adapter.1.to_k_ip.weight'].shape[1]) == 2048:
        raise ValueError(f'an SDXL IP-Adapter ({len(idx)} cross-attentions, context width '
                         f'{int(sd["ip_adapter.1.to_k_ip.weight"].shape[1]) if "ip_adapter.1.to_k_ip.weight" in sd else "?"}): only SD 1.x is supported')
    part = {}
    for j, (block, width) in enumerate(BLOCKS):
        for which in 'kv':
            key = f'ip_adapter.{2 * j + 1}.to_{which}_ip.weight'
            if key not in sd:
                raise KeyError(f'{key} is missing from the IP-Adapter checkpoint')
            t = sd[key]
            if t.dim() != 2 or int(t.shape[1]) != CTX_DIM:
                raise ValueError(f'{key}: context width {tuple(t.shape)[1:]}: only SD 1.x adapters ({CTX_DIM}) are supported')
            if int(t.shape[0]) != width:
                raise ValueError(f'{key}: {int(t.shape[0])} rows, but {block} (cross-attention {j}) is {width} wide')
            part[unet_key(j, which)] = t.to(dtype)
    pw = sd['image_proj.proj.weight']
    for key in ('image_proj.proj.bias', 'image_proj.norm.weight', 'image_proj.norm.bias'):
        if key not in sd:
            raise KeyError(f'{key} is missing from the IP-Adapter checkpoint')
    if int(sd['image_proj.norm.weight'].shape[0]) != CTX_DIM:
        raise ValueError(f'image_proj.norm.weight: context width {int(sd["image_proj.norm.weight"].shape[0])}: only {CTX_DIM} is supported')
    tokens = int(pw.shape[0]) // CTX_DIM
    if pw.dim() != 2 or tokens * CTX_DIM != int(pw.shape[0]) or not 1 <= tokens <= MAX_TOKENS or int(pw.shape[1]) % 64:
        raise ValueError(f'image_proj.proj.weight has shape {tuple(pw.shape)}: expected [T * {CTX_DIM}, E] with T in [1, {MAX_TOKENS}] and E a multiple of 64')
    if tuple(sd['image_proj.proj.bias'].shape) != (tokens * CTX_DIM,):
        raise ValueError(f'image_proj.proj.bias has shape {tuple(sd["image_proj.proj.bias"].shape)}, expected {(tokens * CTX_DIM,)}')
    for name in ('proj.weight', 'proj.bias', 'norm.weight', 'norm.bias'):
        part[name] = sd['image_proj.' + name].to(dtype)
    return part


def vision_config_of(sd):
    """the sdod_vision_config integers of an HF CLIPVisionModelWithProjection state dict: from the shapes, and the head width from the
    hidden size (64 per head, except OpenCLIP ViT-H/14's 1280 = 16 x 80); erf GELU for ViT-H, quick-GELU otherwise (the HF config's
    `hidden_act` is not in the state dict: pass quick_gelu to image_encoder_parameters to override)"""
    e = 'vision_model.embeddings.'
    pw = sd[e + 'patch_embedding.weight']
    width, patch = int(pw.shape[0]), int(pw.shape[-1])
    npos = int(sd[e + 'position_embedding.weight'].shape[0])
    grid = int(round((npos - 1) ** 0.5))
    if grid * grid != npos - 1:
        raise ValueError(f'{e}position_embedding.weight has {npos} rows: not a square grid plus the class token')
    layers = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('vision_model.encoder.layers.'))
    heads = width // 80 if width == 1280 else width // 64
    mlp = int(sd['vision_model.encoder.layers.0.mlp.fc1.weight'].shape[0])
    proj = int(sd['visual_projection.weight'].shape[0])
    return (grid * patch, patch, width, layers, heads, mlp, proj, 0 if width == 1280 else 1)


def image_encoder_parameters(sd, dtype=torch.float16, quick_gelu=None):
    """an HF CLIPVisionModelWithProjection state dict -> {name: tensor} for image_encoder.sdodw in the IMAGE_ENCODER graph's table
    shapes (patch embedding flattened and zero-padded, class embedding [1, W]) plus CONFIG_KEY"""
    from . import engine as E
    sd = {k: v for k, v in sd.items() if k.startswith(('vision_model.', 'visual_projection.'))}
    if 'visual_projection.weight' not in sd or 'vision_model.embeddings.patch_embedding.weight' not in sd:
        raise ValueError('not a CLIPVisionModelWithProjection state dict: vision_model.embeddings.* / visual_projection.weight are missing')
    vals = list(vision_config_of(sd))
    if quick_gelu is not None:
        vals[7] = 1 if quick_gelu else 0
    vision = E.VisionConfig(*vals)
    enc = E.ImageEncoder(vision, 1)
    want = dict(enc.checkpoint_table())
    part = {}
    for name, shape in enc.param_table():
        if name not in sd:
            raise KeyError(f'{name} is missing from the image encoder checkpoint')
        t = sd[name]
        if tuple(t.shape) != tuple(want[name]):
            raise ValueError(f'{name}: checkpoint shape {tuple(t.shape)} != expected {tuple(want[name])}')
        if tuple(t.shape) != tuple(shape):
            flat = t.reshape(shape[0], -1)
            padded = torch.zeros(tuple(shape), dtype=t.dtype)
            padded[:, :flat.shape[1]] = flat
            t = padded
        part[name] = t.to(dtype)
    part[CONFIG_KEY] = torch.tensor(vals, dtype=torch.float32)
    return part


# ------------------------------------------------------------------ Txt2Img(ip_adapter=True)
def ip_check_build(ip_adapter, regions=False, prompt_chunks=1, cfg_split=False, hires_hw=None, controlnet=False, adapter=False, tiling=False,
                   inpaint_unet=False, model='sd14', weight_quant=None):
    """Txt2Img's `ip_adapter` against the rest of its arguments, before any device work: returns False or True; raises ValueError naming
    `ip_adapter` for a bad value and for every combination the UNet with an image prompt does not take"""
    if ip_adapter is False or ip_adapter is None:
        return False
    if ip_adapter is not True:
        raise ValueError(f'ip_adapter must be False or True, got {ip_adapter!r}')
    refused = [('regions', bool(regions)), ('prompt_chunks > 1', prompt_chunks != 1), ('cfg_split', bool(cfg_split)), ('hires_hw', hires_hw is not None),
               ('controlnet', bool(controlnet)), ('adapter', bool(adapter)), ('tiling', bool(tiling)), ('inpaint_unet', bool(inpaint_unet)),
               ("model='sd21'", model == 'sd21'), ('uint8 weights (weight_quant)', bool(weight_quant))]
    bad = [name for name, on in refused if on]
    if bad:
        raise ValueError(f'ip_adapter cannot be combined with {", ".join(bad)}')
    return True


def ip_sources(state_dicts, models_dir):
    """what Txt2Img(ip_adapter=True) builds from: (ip_tokens, proj_dim, vision config tuple or None), read from
    state_dicts['ip_adapter'] (+ ['image_encoder'], with its CONFIG_KEY entry) or the headers of models_dir/ip_adapter.sdodw (+
    image_encoder.sdodw).  ValueError when the adapter is missing or malformed; no device work."""
    from . import weights
    vision = None
    if state_dicts is not None:
        if 'ip_adapter' not in state_dicts:
            raise ValueError("ip_adapter=True needs state_dicts['ip_adapter']")
        shape = tuple(state_dicts['ip_adapter']['proj.weight'].shape) if 'proj.weight' in state_dicts['ip_adapter'] else None
        if 'image_encoder' in state_dicts:
            cfgv = state_dicts['image_encoder'].get(CONFIG_KEY)
            if cfgv is None:
                raise ValueError(f"state_dicts['image_encoder'] needs the '{CONFIG_KEY}' entry (ip_adapter.image_encoder_parameters writes it)")
            vision = tuple(int(v) for v in cfgv.tolist())
    elif models_dir is not None:
        path = os.path.join(models_dir, 'ip_adapter.sdodw')
        if not os.path.exists(path):
            raise ValueError(f'ip_adapter=True needs {path} (python -m sdod.amd.convert --ip-adapter FILE --out DIR)')
        shape = weights.shapes(path).get('proj.weight')
        enc = os.path.join(models_dir, 'image_encoder.sdodw')
        if os.path.exists(enc):
            cfgv = weights.load(enc).get(CONFIG_KEY) if CONFIG_KEY in weights.shapes(enc) else None
            if cfgv is None:
                raise ValueError(f'{enc} holds no {CONFIG_KEY}: convert it again (python -m sdod.amd.convert --image-encoder FILE --out DIR)')
            vision = tuple(int(v) for v in cfgv.tolist())
    else:
        raise ValueError('ip_adapter=True needs state_dicts or models_dir')
    if shape is None or len(shape) != 2 or shape[0] % CTX_DIM or not 1 <= shape[0] // CTX_DIM <= MAX_TOKENS or shape[1] % 64:
        raise ValueError(f'ip_adapter: proj.weight has shape {shape}, expected [T * {CTX_DIM}, E] with T in [1, {MAX_TOKENS}] and E a multiple of 64')
    if vision is not None and (len(vision) != 8 or vision[6] != shape[1]):
        raise ValueError(f'ip_adapter: the image encoder gives {vision[6] if len(vision) == 8 else "?"}-wide embeddings, the adapter takes {shape[1]}')
    return int(shape[0]) // CTX_DIM, int(shape[1]), vision


def _as_tensor(x, name, dtypes):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError(f'{name} must be a tensor or a numpy array, got {type(x).__name__}')
    if x.dtype not in dtypes:
        raise ValueError(f'{name} must be {" or ".join(str(d).replace("torch.", "") for d in dtypes)}, got {x.dtype}')
    return x.contiguous()


def ip_check_args(pipe, image_u8, embeds, weight, mask_u8):
    """set_image_prompt's arguments against the pipeline (callable on a Txt2Img.__new__ object with `ip_tokens`, `n`, `_latent_shape`,
    `ip_proj_dim` and `ip_image_size`, the last None without an image encoder): returns (image or None, embeds or None, weight, mask
    or None) as contiguous tensors; RuntimeError without ip_adapter=True, ValueError for everything else; no device work"""
    if not int(getattr(pipe, 'ip_tokens', 0) or 0):
        raise RuntimeError('this pipeline was built without ip_adapter=True: Txt2Img(..., ip_adapter=True) is needed for image prompts')
    if (image_u8 is None) == (embeds is None):
        raise ValueError('give exactly one of image_u8 and embeds')
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or not np.isfinite(float(weight)) or float(weight) < 0:
        raise ValueError(f'weight must be a finite number >= 0, got {weight!r}')
    n = int(pipe.n)
    if image_u8 is not None:
        size = getattr(pipe, 'ip_image_size', None)
        if size is None:
            raise ValueError('this pipeline has no image encoder (no image_encoder weights were given): pass embeds, CLIP image_embeds '
                             f'[{n}, {pipe.ip_proj_dim}]')
        image_u8 = _as_tensor(image_u8, 'image_u8', (torch.uint8,))
        if tuple(image_u8.shape) != (n, size, size, 3):
            raise ValueError(f'image_u8 must be [{n}, {size}, {size}, 3] (resized and cropped by the caller), got {tuple(image_u8.shape)}')
    else:
        embeds = _as_tensor(embeds, 'embeds', (torch.float16, torch.float32))
        if tuple(embeds.shape) != (n, pipe.ip_proj_dim):
            raise ValueError(f'embeds must be [{n}, {pipe.ip_proj_dim}], got {tuple(embeds.shape)}')
        if not bool(torch.isfinite(embeds).all()):
            raise ValueError('embeds must be finite')
    if mask_u8 is not None:
        mask_u8 = _as_tensor(mask_u8, 'mask_u8', (torch.uint8,))
        h, w = tuple(pipe._latent_shape)[-2:]
        if tuple(mask_u8.shape) != (8 * h, 8 * w):
            raise ValueError(f'mask_u8 must be at image resolution {(8 * h, 8 * w)}, got {tuple(mask_u8.shape)}')
    return image_u8, embeds, float(weight), mask_u8
