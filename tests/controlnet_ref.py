"""fp32 restatement of ControlNet (ldm's cldm.ControlNet and cldm.ControlledUnetModel for SD 1.x), built from the modules of
oracle.sd_torch.UNetModel.  Test infrastructure, not product.

  control net    input_blocks.0..11 and middle_block of a UNetModel on the CONTROL weights, the guided hint (input_hint_block on
                 hint / 255) added behind input_blocks.0, zero_convs.k.0 on the twelve skip tensors, middle_block_out.0 on the middle
  controlled     UNetModel.forward with h + scale[12] * control[12] behind the middle block and hs.pop() + scale[k] * control[k] where
  UNet           the decoder concatenates a skip

State-dict names are the checkpoint's with `control_model.` stripped, which is what sdod.amd.engine's ControlNet, ControlHint and
control Temb graphs take."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import sd_torch as S

HINT_WIDTHS = (3, 16, 16, 32, 32, 96, 96, 256)
HINT_STRIDES = (1, 1, 2, 1, 2, 1, 2, 1)


def residual_channels(mc=320):
    return [mc] * 4 + [2 * mc] * 3 + [4 * mc] * 6


def param_table(mc=320):
    """(name, shape) of everything a ControlNet checkpoint holds, in one table: the three engine graphs each take their own names"""
    with torch.device('meta'):
        unet = S.UNetModel(model_ch=mc)
    out = [(k, tuple(v.shape)) for k, v in unet.state_dict().items() if k.startswith(('time_embed.', 'input_blocks.', 'middle_block.'))]
    widths = HINT_WIDTHS + (mc,)
    for j in range(8):
        out += [(f'input_hint_block.{2 * j}.weight', (widths[j + 1], widths[j], 3, 3)), (f'input_hint_block.{2 * j}.bias', (widths[j + 1],))]
    for k, c in enumerate(residual_channels(mc)):
        pfx = f'zero_convs.{k}.0' if k < 12 else 'middle_block_out.0'
        out += [(pfx + '.weight', (c, c, 1, 1)), (pfx + '.bias', (c,))]
    return out


class ControlNet(nn.Module):
    def __init__(self, sd, mc=320):
        super().__init__()
        with torch.device('meta'):
            self.body = S.UNetModel(model_ch=mc)
        own = {k: v.float() for k, v in sd.items() if k.startswith(('time_embed.', 'input_blocks.', 'middle_block.'))}
        missing = self.body.load_state_dict(own, strict=False, assign=True)
        assert all(k.startswith(('output_blocks.', 'out.')) for k in missing.missing_keys) and not missing.unexpected_keys
        self.sd = {k: v.float() for k, v in sd.items()}
        self.mc = mc

    def guided_hint(self, hint_u8):
        """uint8 [n, 8h, 8w, 3] -> fp32 NCHW [n, mc, h, w]"""
        h = hint_u8.permute(0, 3, 1, 2).float() / 255
        for j in range(8):
            h = F.conv2d(h, self.sd[f'input_hint_block.{2 * j}.weight'], self.sd[f'input_hint_block.{2 * j}.bias'], stride=HINT_STRIDES[j], padding=1)
            if j < 7:
                h = F.silu(h)
        return h

    def forward(self, x, timesteps, context, guided_hint):
        """the 13 residuals, fp32 NCHW; guided_hint [n or B, mc, h, w] (n: repeated for the two guidance halves)"""
        b = self.body
        emb = b.time_embed(S.timestep_embedding(timesteps, self.mc))
        if guided_hint.shape[0] != x.shape[0]:
            guided_hint = guided_hint.repeat(x.shape[0] // guided_hint.shape[0], 1, 1, 1)
        outs = []
        h = x
        for k, m in enumerate(b.input_blocks):
            h = m(h, emb, context)
            if k == 0:
                h = h + guided_hint
            outs.append(F.conv2d(h, self.sd[f'zero_convs.{k}.0.weight'], self.sd[f'zero_convs.{k}.0.bias']))
        h = b.middle_block(h, emb, context)
        outs.append(F.conv2d(h, self.sd['middle_block_out.0.weight'], self.sd['middle_block_out.0.bias']))
        return outs


def controlled_unet(unet, x, timesteps, context, control, scales):
    """cldm.ControlledUnetModel.forward on an oracle UNetModel: control = 13 fp32 NCHW residuals, scales = 13 floats"""
    emb = unet.time_embed(S.timestep_embedding(timesteps, unet.model_ch))
    hs = []
    h = x
    for m in unet.input_blocks:
        h = m(h, emb, context)
        hs.append(h)
    h = unet.middle_block(h, emb, context)
    control = [float(s) * c for s, c in zip(scales, control)]
    h = h + control.pop()
    for m in unet.output_blocks:
        h = torch.cat([h, hs.pop() + control.pop()], dim=1)
        h = m(h, emb, context)
    return unet.out(h)
