"""Synthetic LoRA adapters shared by the LoRA GPU tests (not a test module).

Factors are fp16 -- the engine and the host merge then see the same numbers -- and sized against the weight they adapt:
up ~ N(0, 1), down ~ N(0, 1) * std(W) / sqrt(rank), so that scale * up @ down has `scale` times the weight's own spread."""
import re

import torch

UNET_SKIP = ('input_blocks.0.0.weight', 'out.2.weight')


def unet_targets(table):
    """every conv / Linear weight of the UNet table that takes an adapter"""
    return [n for n, shape in table if len(shape) >= 2 and n not in UNET_SKIP]


def text_targets(table, layers):
    """the six adapted matrices of the given text-encoder layers"""
    return [n for n, shape in table if len(shape) == 2 and (m := re.match(r'text_model\.encoder\.layers\.(\d+)\.', n)) and int(m.group(1)) in layers]


def make_entries(sd, names, rank, scale, seed):
    """[(param_name, up, down, scale)] in canonical kohya shapes: up [out, rank] or [out, rank, 1, 1], down [rank, in] or [rank, cin, kh, kw]"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in names:
        w = sd[n]
        std = float(w.float().std())
        up = torch.randn(w.shape[0], rank, generator=gen)
        down = torch.randn(rank, *w.shape[1:], generator=gen) * (std / rank ** 0.5)
        if w.dim() == 4:
            up = up.reshape(w.shape[0], rank, 1, 1)
        out.append((n, up.half(), down.half(), float(scale)))
    return out


def kohya_key(param_name):
    """the kohya module key of a graph parameter (the inverse of sdod.amd.lora.map_key, for the modules the tests write to files)"""
    n = param_name[:-len('.weight')]
    m = re.match(r'text_model\.encoder\.layers\.(\d+)\.(self_attn\.(?:q|k|v|out)_proj|mlp\.fc[12])$', n)
    if m:
        return f'lora_te_text_model_encoder_layers_{m.group(1)}_{m.group(2).replace(".", "_")}'
    m = re.match(r'(input_blocks|middle_block|output_blocks)\.(\d+)\.(?:(\d+)\.)?(.+)$', n)
    kind, a, b, rest = m.group(1), int(m.group(2)), m.group(3), m.group(4)
    if kind == 'middle_block':
        if a == 1:
            return 'lora_unet_mid_block_attentions_0_' + rest.replace('.', '_')
        return f'lora_unet_mid_block_resnets_{a // 2}_' + _res(rest)
    b = int(b)
    if kind == 'input_blocks':
        i, j = (a - 1) // 3, (a - 1) % 3
        if rest == 'op':
            return f'lora_unet_down_blocks_{i}_downsamplers_0_conv'
        return f'lora_unet_down_blocks_{i}_' + (f'attentions_{j}_' + rest.replace('.', '_') if b == 1 else f'resnets_{j}_' + _res(rest))
    i, j = a // 3, a % 3
    if rest == 'conv':
        return f'lora_unet_up_blocks_{i}_upsamplers_0_conv'
    return f'lora_unet_up_blocks_{i}_' + (f'attentions_{j}_' + rest.replace('.', '_') if b == 1 else f'resnets_{j}_' + _res(rest))


def _res(rest):
    return {'in_layers.2': 'conv1', 'out_layers.3': 'conv2', 'skip_connection': 'conv_shortcut'}[rest]


def kohya_state_dict(entries, alpha):
    """a kohya-named tensor dict of the entries' factors (their scale is dropped: the reader derives it from strength, alpha, rank)"""
    out = {}
    for name, up, down, _ in entries:
        k = kohya_key(name)
        out[f'{k}.lora_up.weight'] = up.contiguous()
        out[f'{k}.lora_down.weight'] = down.contiguous()
        out[f'{k}.alpha'] = torch.tensor(float(alpha))
    return out
