"""HyperTile references for the tests: the tile rule restated, and the oracle UNet (oracle/sd_torch.py, unedited) with the method's
rearrangement -- b (nh h nw w) c -> (b nh nw) (h w) c around attn1 -- wrapped around its modules from outside."""
import types


def grid(H, W, T, level, max_depth):
    """(th, tw) at `level` of an H x W latent, or None where the level is untiled: the rule of include/sdod_hip.h, restated"""
    def count(n):
        return n // next(d for d in range(min(T, n), n + 1) if n % d == 0)
    nh, nw, h, w = count(H), count(W), H >> level, W >> level
    if level > max_depth or nh * nw == 1 or h == 0 or w == 0 or h % nh or w % nw:
        return None
    return h // nh, w // nw


def wrap_oracle(unet, latent_hw, tile, max_depth):
    """unet with every SpatialTransformer's attn1 run inside the rule's tiles (in place on the modules; returns unet)"""
    from oracle import sd_torch as S
    H, W = latent_hw
    for st in [m for m in unet.modules() if isinstance(m, S.SpatialTransformer)]:
        def st_forward(self, x, emb=None, context=None, _fwd=st.forward):
            self.map_hw = tuple(x.shape[2:])
            return _fwd(x, emb, context)

        def attn1_forward(self, x, context=None, _fwd=st.transformer_blocks[0].attn1.forward, _st=st):
            h, w = _st.map_hw
            t = grid(H, W, tile, (H // h).bit_length() - 1, max_depth)
            if t is None or (H >> ((H // h).bit_length() - 1), W >> ((H // h).bit_length() - 1)) != (h, w):
                return _fwd(x, context)
            (th, tw), b, c = t, x.shape[0], x.shape[-1]
            xt = x.reshape(b, h // th, th, w // tw, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, th * tw, c)
            y = _fwd(xt, context)
            return y.reshape(b, h // th, w // tw, th, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h * w, c)
        st.forward = types.MethodType(st_forward, st)
        st.transformer_blocks[0].attn1.forward = types.MethodType(attn1_forward, st.transformer_blocks[0].attn1)
    return unet
