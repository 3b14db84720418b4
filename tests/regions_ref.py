"""Regional prompts, the definitions the tests compare against (CPU, torch / numpy).

Weights.  k regions, masks uint8 [k, 8h, 8w] (255 = inside).  For each UNet level ds in (1, 2, 4, 8): s_r(y, x) = the integer sum of
mask r over the (8 ds)^2 image pixels of level pixel (y, x) -- at most 255 * 64^2 < 2^24, exact in int32 and in fp32; tot = sum_r
s_r; w_r = float32(s_r) / float32(tot), ONE fp32 division; where tot == 0, w_0 = 1 and the others 0 (region 0 is the background).
Per level an fp32 [h / ds * w / ds, k] array, row-major in pixels.

Cross-attention.  The context is [B, 77 k, D]; every attn2 computes sum_r w_r(pixel) attn2(x, ctx[:, 77 r : 77 r + 77]), blended in
front of to_out (which is affine, and the weights sum to 1, so behind it is the same).

Blend kernel.  out[m, c] = half(sum_r w[m % rows_per_img, r] float(a_r[m, c])): acc = w_0 a_0, then acc = acc + w_r a_r for r = 1 ..,
every product and every sum rounded on its own in fp32."""
import numpy as np
import torch

LEVELS = (1, 2, 4, 8)
L_PROMPT = 77


def region_sums(masks_u8, ds):
    """int64 [k, h / ds, w / ds]: box sums of the masks over (8 ds)^2 image pixels"""
    m = np.asarray(masks_u8.cpu() if torch.is_tensor(masks_u8) else masks_u8)
    assert m.dtype == np.uint8 and m.ndim == 3
    k, ih, iw = m.shape
    b = 8 * ds
    assert ih % b == 0 and iw % b == 0
    return m.astype(np.int64).reshape(k, ih // b, b, iw // b, b).sum(axis=(2, 4))


def region_weights(masks_u8):
    """the four levels' weights: a list of fp32 torch tensors [h / ds * w / ds, k]"""
    out = []
    for ds in LEVELS:
        s = region_sums(masks_u8, ds)                                  # [k, H, W]
        tot = s.sum(axis=0)
        assert s.max() < (1 << 24) and tot.max() < (1 << 24)            # exact in fp32
        w = np.float32(s) / np.float32(np.where(tot == 0, 1, tot))[None]        # one fp32 division per weight
        w = np.where(tot[None] == 0, np.float32(0), w)
        w[0][tot == 0] = np.float32(1)
        out.append(torch.from_numpy(np.ascontiguousarray(w.reshape(s.shape[0], -1).T.astype(np.float32))))
    return out


def background_weights(k, hw):
    """'region 0 everywhere' for an h x w latent"""
    out = []
    for ds in LEVELS:
        w = torch.zeros((hw[0] // ds) * (hw[1] // ds), k)
        w[:, 0] = 1.0
        out.append(w)
    return out


def regional_attn2(attn, x, context, w):
    """oracle.sd_torch.CrossAttention `attn` on k prompts: x [B, n, C], context [B, 77 k, D], w fp32 [n, k]"""
    b, n, _ = x.shape
    k = w.shape[1]
    assert context.shape[1] == L_PROMPT * k and w.shape[0] == n, (context.shape, w.shape, n)
    h = attn.heads
    q = attn.to_q(x).reshape(b, n, h, -1).transpose(1, 2)
    out = None
    for r in range(k):
        c = context[:, L_PROMPT * r:L_PROMPT * (r + 1)]
        kk = attn.to_k(c).reshape(b, L_PROMPT, h, -1).transpose(1, 2)
        vv = attn.to_v(c).reshape(b, L_PROMPT, h, -1).transpose(1, 2)
        sim = torch.einsum('bhid,bhjd->bhij', q, kk) * attn.scale
        o = torch.einsum('bhij,bhjd->bhid', sim.softmax(dim=-1), vv).transpose(1, 2).reshape(b, n, -1)
        o = w[None, :, r:r + 1].to(o.dtype) * o
        out = o if out is None else out + o
    return attn.to_out(out)


class regional_unet:
    """oracle UNetModel `unet` with every BasicTransformerBlock.attn2 blending per-region attention outputs by `weights` (the four
    levels' [pixels, k] tensors; the level is told by its pixel count).  Call it like the model: f(x, t, ctx) with ctx [B, 77 k, D]."""

    def __init__(self, unet, weights):
        self.unet = unet
        self.by_pixels = {int(w.shape[0]): w for w in weights}
        assert len(self.by_pixels) == len(weights)

    def __call__(self, x, t, ctx):
        from oracle import sd_torch as S
        patched = []
        try:
            for m in self.unet.modules():
                if isinstance(m, S.BasicTransformerBlock):
                    a = m.attn2
                    a.forward = (lambda xx, context=None, _a=a: regional_attn2(_a, xx, context, self.by_pixels[xx.shape[1]]))
                    patched.append(a)
            with torch.no_grad():
                return self.unet(x, t, ctx)
        finally:
            for a in patched:
                del a.forward


def region_blend(a, w):
    """a fp16 [k, rows, C], w fp32 [rows_per_img, k] -> fp16 [rows, C]; products and sums are separate fp32 operations"""
    k, rows, _ = a.shape
    rpi = w.shape[0]
    wr = w[torch.arange(rows) % rpi]                                    # [rows, k]
    acc = wr[:, 0:1] * a[0].float()
    for r in range(1, k):
        acc = acc + wr[:, r:r + 1] * a[r].float()
    return acc.half()


def column_split(hw, col, k=2):
    """hard split at image pixel column `col`: region 0 left of it, region 1 right of it, any further regions empty"""
    m = torch.zeros(k, 8 * hw[0], 8 * hw[1], dtype=torch.uint8)
    m[0, :, :col] = 255
    m[1, :, col:] = 255
    return m


def soft_masks(hw, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (k, 8 * hw[0], 8 * hw[1]), generator=g, dtype=torch.int32).to(torch.uint8)
