"""fp32 torch restatement of the T2I-Adapter the engine builds (SDOD_GRAPH_ADAPTER), written from its definition -- TencentARC's "full"
adapter, Adapter(channels=[320, 640, 1280, 1280], nums_rb=2, ksize=1, sk=True, use_conv=False):

    x = conv_in(pixel_unshuffle8(hint / 255))                          conv_in.weight [MC, 64 * hint_channels, 3, 3]
    for stage i in 0..3, block j in 0..nums_rb-1, k = i * nums_rb + j:
        if i > 0 and j == 0:  x = avg_pool2(x)
                              if ch[i] != ch[i-1]:  x = in_conv(x)     body.k.in_conv.weight [ch[i], ch[i-1], 1, 1]
        x = block2(relu(block1(x))) + x                                body.k.block1.weight [c, c, 3, 3], body.k.block2.weight [c, c, 1, 1]
        behind the last block of stage i, x is output i

and of the place the UNet adds the four maps (TencentARC's openaimodel.py: `if (id + 1) % 3 == 0: h = h + features_adapter[k]`, i.e.
behind input_blocks.2, .5, .8 and .11, before the tensor is pushed as a skip).  Test infrastructure, not product."""
import torch
import torch.nn.functional as F

LEVELS = (2, 5, 8, 11)      # the input_blocks whose output takes feature 0..3


def channels(model_channels=320):
    return [model_channels, 2 * model_channels, 4 * model_channels, 4 * model_channels]


def param_table(hint_channels=3, nums_rb=2, model_channels=320):
    """[(name, shape)] in the order of the definition above"""
    ch = channels(model_channels)
    t = [('conv_in.weight', (ch[0], 64 * hint_channels, 3, 3)), ('conv_in.bias', (ch[0],))]
    for i in range(4):
        c = ch[i]
        for j in range(nums_rb):
            k = i * nums_rb + j
            if i > 0 and j == 0 and ch[i] != ch[i - 1]:
                t += [(f'body.{k}.in_conv.weight', (c, ch[i - 1], 1, 1)), (f'body.{k}.in_conv.bias', (c,))]
            t += [(f'body.{k}.block1.weight', (c, c, 3, 3)), (f'body.{k}.block1.bias', (c,)),
                  (f'body.{k}.block2.weight', (c, c, 1, 1)), (f'body.{k}.block2.bias', (c,))]
    return t


def unshuffle(hint_u8):
    """uint8 [n, 8h, 8w, ch] -> fp32 NCHW [n, 64 ch, h, w]"""
    return F.pixel_unshuffle(hint_u8.permute(0, 3, 1, 2).float() / 255, 8)


@torch.no_grad()
def adapter_forward(sd, hint_u8, nums_rb=2):
    """sd: {name: tensor} (param_table's names); hint_u8 uint8 [n, 8h, 8w, ch].  Returns the four fp32 NCHW feature maps."""
    w = {k: v.float() for k, v in sd.items()}
    x = F.conv2d(unshuffle(hint_u8), w['conv_in.weight'], w['conv_in.bias'], padding=1)
    outs = []
    for i in range(4):
        for j in range(nums_rb):
            k = i * nums_rb + j
            if i > 0 and j == 0:
                x = F.avg_pool2d(x, 2)
                if f'body.{k}.in_conv.weight' in w:
                    x = F.conv2d(x, w[f'body.{k}.in_conv.weight'], w[f'body.{k}.in_conv.bias'])
            h = F.relu(F.conv2d(x, w[f'body.{k}.block1.weight'], w[f'body.{k}.block1.bias'], padding=1))
            x = F.conv2d(h, w[f'body.{k}.block2.weight'], w[f'body.{k}.block2.bias']) + x
        outs.append(x)
    return outs


class hooked:
    """context manager: the oracle UNet (oracle.sd_torch.UNetModel) with forward hooks on input_blocks[2], [5], [8], [11] that return
    out + f.  feats: four NCHW tensors or None (level not set), each [n, C, h, w] with n dividing the batch: the same features for
    every guidance copy."""

    def __init__(self, unet, feats):
        self.unet, self.feats, self.handles = unet, feats, []

    def __enter__(self):
        for idx, f in zip(LEVELS, self.feats):
            if f is None:
                continue
            self.handles.append(self.unet.input_blocks[idx].register_forward_hook(
                lambda mod, args, out, f=f: out + f.repeat(out.shape[0] // f.shape[0], 1, 1, 1)))
        return self.unet

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        return False
