"""LoRA adapters on the host: reading a kohya-style file, mapping its module names to graph parameters, and the plain host merge.

A kohya LoRA file holds, per adapted module, `<module>.lora_down.weight` [rank, in] (a convolution: [rank, cin, kh, kw]),
`<module>.lora_up.weight` [out, rank] ([out, rank, 1, 1]) and optionally `<module>.alpha`; the module computes with
W + strength * alpha / rank * up @ down.  `<module>` is the diffusers / HF module path with '.' written as '_' behind `lora_unet_` or
`lora_te_`.  The graphs name their parameters as the CompVis-ldm checkpoint does (include/sdod_engine.h), so map_key() translates:

    lora_unet_down_blocks_{i}_attentions_{j}_X      input_blocks.{1 + 3 i + j}.1.X          i = 0 .. 2, j = 0, 1
    lora_unet_mid_block_attentions_0_X              middle_block.1.X
    lora_unet_up_blocks_{i}_attentions_{j}_X        output_blocks.{3 i + j}.1.X             i = 1 .. 3, j = 0 .. 2
        X: proj_in, proj_out, transformer_blocks_0_{attn1,attn2}_{to_q,to_k,to_v,to_out_0}, transformer_blocks_0_ff_net_0_proj,
           transformer_blocks_0_ff_net_2  ->  the same path with dots
    lora_unet_down_blocks_{i}_resnets_{j}_Y         input_blocks.{1 + 3 i + j}.0.Z          i = 0 .. 3
    lora_unet_mid_block_resnets_{j}_Y               middle_block.{0, 2}.Z
    lora_unet_up_blocks_{i}_resnets_{j}_Y           output_blocks.{3 i + j}.0.Z             i = 0 .. 3
        Y -> Z: conv1 -> in_layers.2, conv2 -> out_layers.3, conv_shortcut -> skip_connection
    lora_unet_down_blocks_{i}_downsamplers_0_conv   input_blocks.{3 (i + 1)}.0.op           i = 0 .. 2
    lora_unet_up_blocks_{i}_upsamplers_0_conv       output_blocks.{3 i + 2}.{1 if i == 0 else 2}.conv      i = 0 .. 2
    lora_te_text_model_encoder_layers_{N}_{self_attn_{q,k,v,out}_proj, mlp_fc1, mlp_fc2}
                                                    text_model.encoder.layers.{N}.{self_attn.q_proj, .., mlp.fc2}   (sd14 only)

Refused, with the reason in the error: `time_emb_proj` (the time conditioning reaches the UNet graph already projected, by the TEMB
graph), `conv_in` / `conv_out` (the input convolution is packed for its own kernel, the output convolution is not a usual target),
`time_embedding`, the OpenCLIP text tower of sd21, and -- by THIS reader, which is the plain-LoRA one -- every module that holds
tensors of another family (LoHa `hada_*`, LoKr `lokr_*`, a Tucker core `lora_mid`, a full `diff`, DoRA `dora_scale`).  lycoris.py reads
those files, with the same module keys, and is what Txt2Img.set_loras uses; only `dora_scale`, `diff_b` and the norm-layer tensors stay
refused there.

With time_modules=True (a pipeline built with lora_time_modules=True, whose TEMB graphs keep their base weights) the time conditioning
is a target too, under a third graph name, 'temb' -- what LCM-LoRA adapts:

    lora_unet_{down_blocks_{i},mid_block,up_blocks_{i}}_resnets_{j}_time_emb_proj   <the ResBlock above>.emb_layers.1
    lora_unet_time_embedding_linear_1 / _2                                          time_embed.0 / time_embed.2"""
import math
import re

import torch

_ATTN_SUFFIX = {'proj_in': 'proj_in', 'proj_out': 'proj_out', 'transformer_blocks_0_ff_net_0_proj': 'transformer_blocks.0.ff.net.0.proj',
                'transformer_blocks_0_ff_net_2': 'transformer_blocks.0.ff.net.2'}
for _a in ('attn1', 'attn2'):
    for _m in ('to_q', 'to_k', 'to_v'):
        _ATTN_SUFFIX[f'transformer_blocks_0_{_a}_{_m}'] = f'transformer_blocks.0.{_a}.{_m}'
    _ATTN_SUFFIX[f'transformer_blocks_0_{_a}_to_out_0'] = f'transformer_blocks.0.{_a}.to_out.0'
_RES_SUFFIX = {'conv1': 'in_layers.2', 'conv2': 'out_layers.3', 'conv_shortcut': 'skip_connection'}
_TEXT_SUFFIX = {f'self_attn_{m}_proj': f'self_attn.{m}_proj' for m in ('q', 'k', 'v', 'out')}
_TEXT_SUFFIX.update({'mlp_fc1': 'mlp.fc1', 'mlp_fc2': 'mlp.fc2'})
_LORA_TENSORS = ('lora_down.weight', 'lora_up.weight', 'alpha')


class LoraFile(dict):
    """{module_key: (down, up, alpha)}; `other` lists the modules of the file that hold tensors of another adapter family"""
    other = ()


def read_lora(path):
    """A .safetensors file, a torch.save'd dict, or such a dict itself, in the kohya layout -> LoraFile {module_key: (down, up, alpha)}
    (alpha a float; a module without `.alpha` gets alpha = rank).  Modules with tensors that are not plain LoRA (LoHa, LoKr, DoRA, a
    `lora_mid` core) are not in the mapping; their names are in `.other`, for entries_for to refuse."""
    if isinstance(path, LoraFile):
        return path
    if isinstance(path, dict):
        raw = path
    elif str(path).endswith('.safetensors'):
        from safetensors.torch import load_file
        raw = load_file(str(path))
    else:
        raw = torch.load(str(path), map_location='cpu')
        if not isinstance(raw, dict):
            raise ValueError(f'{path}: not a dict of tensors')
    if raw and all(isinstance(v, tuple) and len(v) == 3 for v in raw.values()):
        out = LoraFile(raw)                          # already {module: (down, up, alpha)}
        return out
    mods, other = {}, set()
    for key, t in raw.items():
        module, _, rest = key.partition('.')
        if rest in _LORA_TENSORS:
            mods.setdefault(module, {})[rest] = t
        else:
            other.add(module)
    out = LoraFile()
    for module, d in mods.items():
        if module in other:
            continue
        if 'lora_down.weight' not in d or 'lora_up.weight' not in d:
            raise ValueError(f'{module}: lora_down.weight and lora_up.weight must both be present')
        down, up = d['lora_down.weight'], d['lora_up.weight']
        if down.dim() < 2 or up.dim() < 2 or up.shape[1] != down.shape[0] or up.numel() != up.shape[0] * up.shape[1]:
            raise ValueError(f'{module}: factors {tuple(up.shape)} x {tuple(down.shape)} are not a rank decomposition')
        out[module] = (down, up, float(d['alpha']) if 'alpha' in d else float(down.shape[0]))
    out.other = tuple(sorted(other))
    return out


def _unet_name(rest):
    m = re.fullmatch(r'(down_blocks_(\d+)|mid_block|up_blocks_(\d+))_attentions_(\d+)_(.+)', rest)
    if m and m.group(5) in _ATTN_SUFFIX:
        j = int(m.group(4))
        if m.group(2) is not None and int(m.group(2)) <= 2 and j <= 1:
            return f'input_blocks.{1 + 3 * int(m.group(2)) + j}.1.{_ATTN_SUFFIX[m.group(5)]}'
        if m.group(1) == 'mid_block' and j == 0:
            return f'middle_block.1.{_ATTN_SUFFIX[m.group(5)]}'
        if m.group(3) is not None and 1 <= int(m.group(3)) <= 3 and j <= 2:
            return f'output_blocks.{3 * int(m.group(3)) + j}.1.{_ATTN_SUFFIX[m.group(5)]}'
        return None
    m = re.fullmatch(r'(down_blocks_(\d+)|mid_block|up_blocks_(\d+))_resnets_(\d+)_(.+)', rest)
    if m:
        if m.group(5) == 'time_emb_proj':
            raise ValueError('time_emb_proj is not a target: the time conditioning reaches the UNet graph already projected (TEMB graph)')
        if m.group(5) not in _RES_SUFFIX:
            return None
        j, z = int(m.group(4)), _RES_SUFFIX[m.group(5)]
        if m.group(2) is not None and int(m.group(2)) <= 3 and j <= 1:
            return f'input_blocks.{1 + 3 * int(m.group(2)) + j}.0.{z}'
        if m.group(1) == 'mid_block' and j <= 1:
            return f'middle_block.{2 * j}.{z}'
        if m.group(3) is not None and int(m.group(3)) <= 3 and j <= 2:
            return f'output_blocks.{3 * int(m.group(3)) + j}.0.{z}'
        return None
    m = re.fullmatch(r'down_blocks_(\d+)_downsamplers_0_conv', rest)
    if m and int(m.group(1)) <= 2:
        return f'input_blocks.{3 * (int(m.group(1)) + 1)}.0.op'
    m = re.fullmatch(r'up_blocks_(\d+)_upsamplers_0_conv', rest)
    if m and int(m.group(1)) <= 2:
        i = int(m.group(1))
        return f'output_blocks.{3 * i + 2}.{1 if i == 0 else 2}.conv'     # behind the ResBlock, and the transformer where there is one
    if rest in ('conv_in', 'conv_out') or rest.startswith('time_embedding'):
        raise ValueError(f'{rest} is not a target (conv_in / conv_out / the time MLP are outside the adapted weights)')
    return None


_TIME_MLP = {'time_embedding_linear_1': 'time_embed.0', 'time_embedding_linear_2': 'time_embed.2'}


def _time_name(rest):
    """the TEMB graph's parameter (without .weight) of a module of the time conditioning -- a ResBlock's time_emb_proj, which is
    `<block>.emb_layers.1` (a row slice of the graph's one fused projection), or the time MLP's two Linears -- or None"""
    if rest in _TIME_MLP:
        return _TIME_MLP[rest]
    m = re.fullmatch(r'(down_blocks_(\d+)|mid_block|up_blocks_(\d+))_resnets_(\d+)_time_emb_proj', rest)
    if not m:
        return None
    j = int(m.group(4))
    if m.group(2) is not None and int(m.group(2)) <= 3 and j <= 1:
        return f'input_blocks.{1 + 3 * int(m.group(2)) + j}.0.emb_layers.1'
    if m.group(1) == 'mid_block' and j <= 1:
        return f'middle_block.{2 * j}.emb_layers.1'
    if m.group(3) is not None and int(m.group(3)) <= 3 and j <= 2:
        return f'output_blocks.{3 * int(m.group(3)) + j}.0.emb_layers.1'
    return None


def map_key(module_key, model='sd14', time_modules=False):
    """kohya module key -> ('unet' | 'text', graph parameter name).  ValueError, with the reason, for what is not supported.
    time_modules=True (a pipeline built with lora_time_modules: its TEMB graphs keep their base weights): the modules of the time
    conditioning -- lora_unet_*_resnets_*_time_emb_proj, lora_unet_time_embedding_linear_1 / _2, what LCM-LoRA adapts next to the
    usual ones -- map to ('temb', name) instead of being refused."""
    if time_modules and module_key.startswith('lora_unet_'):
        name = _time_name(module_key[len('lora_unet_'):])
        if name is not None:
            return 'temb', name + '.weight'
    if module_key.startswith('lora_unet_'):
        try:
            name = _unet_name(module_key[len('lora_unet_'):])
        except ValueError as e:
            raise ValueError(f'{module_key}: {e}') from None
        if name is None:
            raise ValueError(f'{module_key}: not a module of the SD UNet that takes an adapter')
        return 'unet', name + '.weight'
    for prefix in ('lora_te_', 'lora_te1_'):
        if module_key.startswith(prefix):
            if model != 'sd14':
                raise ValueError(f'{module_key}: text-encoder adapters are supported for the CLIP ViT-L/14 tower of sd14 only '
                                 f'(the OpenCLIP tower of {model} fuses q / k / v)')
            m = re.fullmatch(r'text_model_encoder_layers_(\d+)_(.+)', module_key[len(prefix):])
            if not m or m.group(2) not in _TEXT_SUFFIX:
                raise ValueError(f'{module_key}: not a module of the CLIP text encoder that takes an adapter')
            return 'text', f'text_model.encoder.layers.{int(m.group(1))}.{_TEXT_SUFFIX[m.group(2)]}.weight'
    raise ValueError(f'{module_key}: neither a lora_unet_ nor a lora_te_ module')


def entries_for(lora, model='sd14', scale_unet=1.0, scale_text=1.0, strict=True, time_modules=False):
    """lora: what read_lora takes or returns.  Returns ({'unet': [(param_name, up, down, scale)], 'text': [...]}, skipped): the entry
    lists Graph.set_loras takes, scale = strength * alpha / rank, and the module keys that were skipped.  strict=True raises ValueError
    listing every unsupported module instead of skipping it.  time_modules=True: the modules of the time conditioning (map_key) come
    back under a third list, 'temb', at the UNet's strength."""
    lora = read_lora(lora)
    out, skipped, why = {'unet': [], 'text': []}, [], []
    if time_modules:
        out['temb'] = []
    for module in lora.other:
        skipped.append(module)
        why.append(f'{module}: not a plain LoRA module (LoHa / LoKr / DoRA tensors)')
    for module, (down, up, alpha) in lora.items():
        try:
            graph, name = map_key(module, model, time_modules)
        except ValueError as e:
            skipped.append(module)
            why.append(str(e))
            continue
        rank = down.shape[0]
        strength = scale_text if graph == 'text' else scale_unet
        out[graph].append((name, up, down, float(strength) * float(alpha) / rank))
    if strict and skipped:
        raise ValueError('unsupported LoRA modules:\n  ' + '\n  '.join(why))
    return out, skipped


def merged_state_dict(sd, entries):
    """The plain host merge: a copy of `sd` with W + scale * up @ down (fp64, cast back to W's dtype, canonical layout, convolutions
    reshaped) for every (param_name, up, down, scale); entries naming the same weight are summed before the one cast.  The fallback for
    graphs built without keep_base() or with uint8 weights -- load the result into a new graph -- and what the tests feed the oracle."""
    acc = {}
    for name, up, down, scale in entries:
        if name not in sd:
            raise KeyError(name)
        w = sd[name]
        if not torch.is_tensor(w):
            raise ValueError(f'{name}: a quantised tensor cannot take a delta')
        rank = down.shape[0]
        delta = up.double().reshape(up.shape[0], rank) @ down.double().reshape(rank, -1)
        if delta.numel() != w.numel() or up.shape[0] != w.shape[0]:
            raise ValueError(f'{name}: factors {tuple(up.shape)} x {tuple(down.shape)} do not give a {tuple(w.shape)} weight')
        if not math.isfinite(scale):
            raise ValueError(f'{name}: scale must be finite')
        acc[name] = acc.get(name, w.double()) + float(scale) * delta.reshape(w.shape)
    out = dict(sd)
    for name, w in acc.items():
        out[name] = w.to(sd[name].dtype)
    return out
