"""Reference-only control for the tests: the oracle UNet (oracle/sd_torch.py, unedited) with every attn1 wrapped from outside -- a main row of
group g attends to [own ; anchor g], mixed with its self-only result by self_w[g] (to_out is affine: blending behind it = in front of it)."""
import types

import torch


def wrap_oracle(unet, anchors, self_w):
    """unet with every SpatialTransformer's attn1 sharing the anchor rows' keys (in place on the modules; returns unet)"""
    from oracle import sd_torch as S
    for st in [m for m in unet.modules() if isinstance(m, S.SpatialTransformer)]:
        def attn1_forward(self, x, context=None, _fwd=st.transformer_blocks[0].attn1.forward):
            n = x.shape[0] - anchors
            group = [b // (n // anchors) for b in range(n)]
            own = _fwd(x)
            both = _fwd(x[:n], torch.cat([x[:n], x[[n + g for g in group]]], 1))
            w = torch.tensor([self_w[g] for g in group], dtype=x.dtype).reshape(n, 1, 1)
            return torch.cat([w * own[:n] + (1 - w) * both, own[n:]])
        st.transformer_blocks[0].attn1.forward = types.MethodType(attn1_forward, st.transformer_blocks[0].attn1)
    return unet
