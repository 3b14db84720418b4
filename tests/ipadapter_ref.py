"""Image prompts (IP-Adapter), the definitions the tests compare against (CPU, torch / numpy).

Weights.  For each UNet level ds in (1, 2, 4, 8) an fp32 [h / ds * w / ds, 2] array, row-major in pixels: column 0 is 1, column 1 is
scale * (float32(S) / float32(255 (8 ds)^2)) with S the integer sum of the uint8 mask [8h, 8w] over the (8 ds)^2 image pixels of the
level pixel -- one fp32 division, one fp32 multiply.  No mask: S = 255 (8 ds)^2, i.e. scale everywhere.

Cross-attention.  out = to_out(w_0 attn(q, K_text, V_text) + w_1 attn(q, to_k_ip(tokens), to_v_ip(tokens))), the bias of to_out
added once; tokens [B, T, D] are the projected image tokens.

Image projection.  LayerNorm(Linear(e).reshape(T, D)) over D, eps 1e-5.

Vision tower.  HF CLIPVisionModelWithProjection: patch convolution (stride = kernel = p, no bias) on (u / 255 - mean) / std, class
token in front, + position embedding, pre_layrnorm, pre-LN blocks (full attention, quick or erf GELU), post_layernorm on the class
token, visual_projection (no bias).  `vision_forward` works in the dtype of its parameters (fp32 or fp64)."""
import numpy as np
import torch
import torch.nn.functional as F

LEVELS = (1, 2, 4, 8)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ------------------------------------------------------------------ weights
def ip_weights(scale, hw, mask_u8=None):
    """the four levels' weights: a list of fp32 torch tensors [h / ds * w / ds, 2]"""
    out = []
    for ds in LEVELS:
        b = 8 * ds
        full = 255 * b * b
        assert full < (1 << 24)                                          # exact in fp32
        if mask_u8 is None:
            s = np.full((hw[0] // ds, hw[1] // ds), full, dtype=np.int64)
        else:
            m = np.asarray(mask_u8.cpu() if torch.is_tensor(mask_u8) else mask_u8)
            assert m.dtype == np.uint8 and m.shape == (8 * hw[0], 8 * hw[1])
            s = m.astype(np.int64).reshape(m.shape[0] // b, b, m.shape[1] // b, b).sum(axis=(1, 3))
        frac = np.float32(s) / np.float32(full)                          # one fp32 division
        w1 = np.float32(scale) * frac                                    # one fp32 multiply
        assert frac.dtype == np.float32 and w1.dtype == np.float32
        w = np.stack([np.ones_like(w1), w1], axis=-1).reshape(-1, 2)
        out.append(torch.from_numpy(np.ascontiguousarray(w)))
    return out


def soft_mask(hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (8 * hw[0], 8 * hw[1]), generator=g, dtype=torch.int32).to(torch.uint8)


# ------------------------------------------------------------------ the adapter's synthetic weights
def ip_block_prefixes(table):
    """the transformer blocks of a UNet parameter table, in table order: '<block>.transformer_blocks.0'"""
    return [n[:-len('.attn2.to_q.weight')] for n, _ in table if n.endswith('.attn2.to_q.weight')]


def synthetic_ip_state_dict(table, seed, spread=1.0, ctx_dim=768):
    """to_k_ip / to_v_ip of every transformer block of `table`: N(0, spread^2 / fan_in), one generator, table order"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    shapes = dict(table)
    for pfx in ip_block_prefixes(table):
        c = int(shapes[pfx + '.attn2.to_q.weight'][0])
        for n in ('to_k_ip', 'to_v_ip'):
            sd[f'{pfx}.attn2.{n}.weight'] = torch.randn(c, ctx_dim, generator=g) * (spread * ctx_dim ** -0.5)
    return sd


# ------------------------------------------------------------------ decoupled cross-attention
def _attend(attn, q, k, v):
    b, n, _ = q.shape
    h = attn.heads
    q, k, v = (t.reshape(b, t.shape[1], h, -1).transpose(1, 2) for t in (q, k, v))
    sim = torch.einsum('bhid,bhjd->bhij', q, k) * attn.scale
    return torch.einsum('bhij,bhjd->bhid', sim.softmax(dim=-1), v).transpose(1, 2).reshape(b, n, -1)


def decoupled_attn2(attn, x, context, tokens, wk, wv, w):
    """oracle.sd_torch.CrossAttention `attn` with an image prompt: x [B, n, C], context [B, L, D], tokens [B, T, D], wk / wv [C, D],
    w fp32 [n, 2]"""
    assert w.shape == (x.shape[1], 2), (w.shape, x.shape)
    q = attn.to_q(x)
    text = _attend(attn, q, attn.to_k(context), attn.to_v(context))
    image = _attend(attn, q, tokens @ wk.to(x.dtype).T, tokens @ wv.to(x.dtype).T)
    mix = w[None, :, 0:1].to(x.dtype) * text + w[None, :, 1:2].to(x.dtype) * image
    return attn.to_out(mix)


class ip_unet:
    """oracle UNetModel `unet` with every BasicTransformerBlock.attn2 decoupled: ip_sd holds '<block>.attn2.to_{k,v}_ip.weight',
    tokens [B, T, D] the projected image tokens, weights the four levels' [pixels, 2] tensors (the level is told by its pixel
    count).  Call it like the model: f(x, t, ctx)."""

    def __init__(self, unet, ip_sd, tokens, weights):
        self.unet, self.ip_sd, self.tokens = unet, ip_sd, tokens
        self.by_pixels = {int(w.shape[0]): w for w in weights}
        assert len(self.by_pixels) == len(weights)

    def __call__(self, x, t, ctx):
        from oracle import sd_torch as S
        patched = []
        try:
            for name, m in self.unet.named_modules():
                if isinstance(m, S.BasicTransformerBlock):
                    a = m.attn2
                    wk, wv = self.ip_sd[name + '.attn2.to_k_ip.weight'], self.ip_sd[name + '.attn2.to_v_ip.weight']
                    a.forward = (lambda xx, context=None, _a=a, _k=wk, _v=wv:
                                 decoupled_attn2(_a, xx, context, self.tokens.to(xx.dtype)[:xx.shape[0]], _k, _v, self.by_pixels[xx.shape[1]]))
                    patched.append(a)
            with torch.no_grad():
                return self.unet(x, t, ctx)
        finally:
            for a in patched:
                del a.forward


# ------------------------------------------------------------------ image projection
def image_proj(sd, embeds, tokens, ctx_dim=768):
    """IP-Adapter's ImageProjModel: sd has proj.weight [T D, E], proj.bias, norm.weight, norm.bias [D]; embeds [B, E] -> [B, T, D]"""
    dt = sd['proj.weight'].dtype
    y = F.linear(embeds.to(dt), sd['proj.weight'], sd['proj.bias']).reshape(-1, tokens, ctx_dim)
    return F.layer_norm(y, (ctx_dim,), sd['norm.weight'], sd['norm.bias'], 1e-5)


# ------------------------------------------------------------------ vision tower
def patch_rows(img_u8, patch, kpad=None, dtype=torch.float32):
    """uint8 [n, S, S, 3] -> [n * (S / p)^2, 3 p p (or kpad)]: column c p p + dy p + dx = (u / 255 - mean_c) / std_c, every operation in
    `dtype`"""
    n, s = img_u8.shape[0], img_u8.shape[1]
    g = s // patch
    x = img_u8.to(dtype) / torch.tensor(255, dtype=dtype)
    x = (x - torch.tensor(CLIP_MEAN, dtype=torch.float32).to(dtype)) / torch.tensor(CLIP_STD, dtype=torch.float32).to(dtype)
    x = x.reshape(n, g, patch, g, patch, 3).permute(0, 1, 3, 5, 2, 4).reshape(n * g * g, 3 * patch * patch)
    if kpad is not None:
        x = F.pad(x, (0, kpad - x.shape[1]))
    return x


def vit_tokens(patches, cls, pos, w, b, eps=1e-5):
    """patches [n, P, W] -> LayerNorm([class | patches] + pos) [n, P + 1, W]"""
    n = patches.shape[0]
    x = torch.cat([cls.reshape(1, 1, -1).expand(n, 1, -1), patches], 1) + pos[None]
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def vision_forward(sd, img_u8, patch, heads, quick_gelu):
    """HF CLIPVisionModelWithProjection on a state dict with HF's names (checkpoint shapes): uint8 [n, S, S, 3] -> image_embeds"""
    dt = sd['visual_projection.weight'].dtype
    e = 'vision_model.embeddings.'
    pw = sd[e + 'patch_embedding.weight']
    width = pw.shape[0]
    n = img_u8.shape[0]
    rows = patch_rows(img_u8, patch, dtype=dt)
    patches = (rows @ pw.reshape(width, -1).T).reshape(n, -1, width)
    x = vit_tokens(patches, sd[e + 'class_embedding'], sd[e + 'position_embedding.weight'], sd['vision_model.pre_layrnorm.weight'],
                   sd['vision_model.pre_layrnorm.bias'])
    layer = 0
    while f'vision_model.encoder.layers.{layer}.layer_norm1.weight' in sd:
        p = f'vision_model.encoder.layers.{layer}.'
        h = F.layer_norm(x, (width,), sd[p + 'layer_norm1.weight'], sd[p + 'layer_norm1.bias'], 1e-5)
        q, k, v = (F.linear(h, sd[p + f'self_attn.{m}_proj.weight'], sd[p + f'self_attn.{m}_proj.bias']) for m in 'qkv')
        d = width // heads
        q, k, v = (t.reshape(n, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        a = (torch.einsum('bhid,bhjd->bhij', q, k) * d ** -0.5).softmax(-1)
        a = torch.einsum('bhij,bhjd->bhid', a, v).transpose(1, 2).reshape(n, -1, width)
        x = x + F.linear(a, sd[p + 'self_attn.out_proj.weight'], sd[p + 'self_attn.out_proj.bias'])
        h = F.layer_norm(x, (width,), sd[p + 'layer_norm2.weight'], sd[p + 'layer_norm2.bias'], 1e-5)
        h = F.linear(h, sd[p + 'mlp.fc1.weight'], sd[p + 'mlp.fc1.bias'])
        h = h * torch.sigmoid(1.702 * h) if quick_gelu else F.gelu(h)
        x = x + F.linear(h, sd[p + 'mlp.fc2.weight'], sd[p + 'mlp.fc2.bias'])
        layer += 1
    pooled = F.layer_norm(x[:, 0], (width,), sd['vision_model.post_layernorm.weight'], sd['vision_model.post_layernorm.bias'], 1e-5)
    return pooled @ sd['visual_projection.weight'].T
