"""fp32 PyTorch restatement of ESRGAN's RRDBNet (Wang et al., "ESRGAN: Enhanced Super-Resolution Generative Adversarial Networks", 2018;
the x4 network the front ends list as "ESRGAN_4x" and "R-ESRGAN 4x+"), written from the published architecture: 64 features, growth 32,
num_blocks residual-in-residual dense blocks, two nearest-2x upsampling convolutions.  Parameter names are basicsr's.

    f = conv_first(u / 255);  t = RRDB_nb(.. RRDB_1(f));  f = f + conv_body(t)
    f = lrelu(conv_up1(up2(f)));  f = lrelu(conv_up2(up2(f)));  y = conv_last(lrelu(conv_hr(f)))                 lrelu: slope 0.2
    RDB(x):  x_k = lrelu(conv_k(x | x_1 | .. | x_{k-1})), k = 1..4;  x_5 = conv_5(x | x_1 .. x_4);  0.2 x_5 + x
    RRDB(x): 0.2 RDB_3(RDB_2(RDB_1(x))) + x

Shared by the CPU tests, the GPU tests and tools/upscaler_bench.py (which runs it in fp16 on the GPU as the MIOpen yardstick)."""
import torch
import torch.nn.functional as F

NF, GC, SCALE = 64, 32, 4


def param_table(num_blocks):
    t = [('conv_first.weight', (NF, 3, 3, 3)), ('conv_first.bias', (NF,))]
    for b in range(num_blocks):
        for r in (1, 2, 3):
            for k in range(1, 6):
                cin, cout = NF + GC * (k - 1), GC if k < 5 else NF
                t += [(f'body.{b}.rdb{r}.conv{k}.weight', (cout, cin, 3, 3)), (f'body.{b}.rdb{r}.conv{k}.bias', (cout,))]
    for name, cout in (('conv_body', NF), ('conv_up1', NF), ('conv_up2', NF), ('conv_hr', NF), ('conv_last', 3)):
        t += [(f'{name}.weight', (cout, NF, 3, 3)), (f'{name}.bias', (cout,))]
    return t


def num_blocks_of(sd):
    return 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('body.'))


def _conv(sd, name, x):
    return F.conv2d(x, sd[name + '.weight'].to(x.dtype), sd[name + '.bias'].to(x.dtype), padding=1)


def forward_float(sd, x):
    """x: NCHW in [0, 1] (any float dtype / device; the parameters are cast to it) -> NCHW [n, 3, 4h, 4w], not clamped"""
    lrelu = lambda v: F.leaky_relu(v, 0.2)
    f = _conv(sd, 'conv_first', x)
    t = f
    for b in range(num_blocks_of(sd)):
        x0 = t
        for r in (1, 2, 3):
            xs = [t]
            for k in range(1, 5):
                xs.append(lrelu(_conv(sd, f'body.{b}.rdb{r}.conv{k}', torch.cat(xs, 1))))
            t = _conv(sd, f'body.{b}.rdb{r}.conv5', torch.cat(xs, 1)) * 0.2 + t
        t = t * 0.2 + x0
    f = f + _conv(sd, 'conv_body', t)
    f = lrelu(_conv(sd, 'conv_up1', F.interpolate(f, scale_factor=2, mode='nearest')))
    f = lrelu(_conv(sd, 'conv_up2', F.interpolate(f, scale_factor=2, mode='nearest')))
    return _conv(sd, 'conv_last', lrelu(_conv(sd, 'conv_hr', f)))


def to_u8(y):
    """NCHW float -> uint8 NHWC: round(255 * clamp(y, 0, 1))"""
    return torch.floor(255.0 * y.clamp(0, 1) + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def upscale(sd, img_u8):
    """img_u8 uint8 [n, h, w, 3] -> (float NHWC [n, 4h, 4w, 3], uint8 NHWC [n, 4h, 4w, 3])"""
    sd = {k: v.float() for k, v in sd.items()}
    with torch.no_grad():
        y = forward_float(sd, img_u8.permute(0, 3, 1, 2).float() / 255.0)
    return y.permute(0, 2, 3, 1).contiguous(), to_u8(y)


def upscale_signed_reparam(sd, img_u8):
    """What re-parametrising conv_first for the VAE encoder's input convolution would compute: x' = 2 u / 255 - 1 zero-padded in THAT
    space, weights w / 2 and bias b + sum(w) / 2.  Equal to upscale() in the interior, different on the border (a padded tap is worth
    0.5 in the [0, 1] space instead of 0): the tests use it to show that the border matters."""
    sd = {k: v.float() for k, v in sd.items()}
    w, b = sd['conv_first.weight'], sd['conv_first.bias']
    sd2 = dict(sd)
    sd2['conv_first.weight'] = w / 2
    sd2['conv_first.bias'] = b + w.sum(dim=(1, 2, 3)) / 2
    with torch.no_grad():
        y = forward_float(sd2, 2.0 * img_u8.permute(0, 3, 1, 2).float() / 255.0 - 1.0)
    return y.permute(0, 2, 3, 1).contiguous()


def synthetic(num_blocks, seed=77, last_gain=1.0, last_bias=0.0):
    """Kaiming-scaled synthetic parameters (weights.synthetic_state_dict) in fp16-representable values; conv_last scaled by last_gain
    with bias last_bias so that a test can spread the output over [0, 1] and beyond"""
    from sdod.amd import weights as Wt
    sd = Wt.synthetic_state_dict(param_table(num_blocks), seed=seed)
    sd['conv_last.weight'] = sd['conv_last.weight'] * last_gain
    sd['conv_last.bias'] = sd['conv_last.bias'] * last_gain + last_bias
    return {k: (v.half().float() if v.dim() == 4 else v) for k, v in sd.items()}


def spread_weights(num_blocks, img_u8, seed=77, sigma=0.35):
    """synthetic() with conv_last rescaled for the uint8 comparison: the fp32 output on img_u8 gets mean 0.5 and standard deviation
    `sigma`, so that a good part of the bytes saturates at 0 / 255 and most lie strictly inside (the CPU test asserts the shares)"""
    sd = synthetic(num_blocks, seed)
    y, _ = upscale(sd, img_u8)
    gain = sigma / float(y.std())
    sd['conv_last.weight'] = (sd['conv_last.weight'] * gain).half().float()
    sd['conv_last.bias'] = sd['conv_last.bias'] * gain + (0.5 - gain * float(y.mean()))
    return sd


def sample_image(n, h, w, seed=5):
    """uint8 [n, h, w, 3]: smooth colour waves with a hard edge and noise on top, every image its own"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(float(h)), torch.arange(float(w)), indexing='ij')
    img = torch.stack([torch.stack([128 + 90 * torch.sin(xx / 3 + k + i) * torch.cos(yy / 2 - k) for k in range(3)], -1) for i in range(n)])
    img[:, h // 2:, : w // 3] += 60
    img += torch.randn(img.shape, generator=g) * 12
    return img.clamp(0, 255).to(torch.uint8)


# the graph tests' cases: (num_blocks, batch, h, w)
CASES = [(1, 2, 8, 16), (2, 2, 16, 24), (23, 1, 16, 24)]


# ------------------------------------------------------------------------------------------------ the checkpoint namings
def to_new_arch(sd):
    """basicsr names -> the original ESRGAN repository's "new arch" names"""
    top = {'conv_body': 'trunk_conv', 'conv_up1': 'upconv1', 'conv_up2': 'upconv2', 'conv_hr': 'HRconv'}
    out = {}
    for k, v in sd.items():
        p = k.split('.')
        if p[0] == 'body':
            out[f'RRDB_trunk.{p[1]}.RDB{p[2][3:]}.{p[3]}.{p[4]}'] = v
        else:
            out[top.get(p[0], p[0]) + '.' + p[1]] = v
    return out


def to_old_arch(sd):
    """basicsr names -> the original ESRGAN repository's "old arch" (nn.Sequential) names"""
    nb = num_blocks_of(sd)
    top = {'conv_first': 'model.0', 'conv_body': f'model.1.sub.{nb}', 'conv_up1': 'model.3', 'conv_up2': 'model.6', 'conv_hr': 'model.8',
           'conv_last': 'model.10'}
    out = {}
    for k, v in sd.items():
        p = k.split('.')
        if p[0] == 'body':
            out[f'model.1.sub.{p[1]}.RDB{p[2][3:]}.{p[3]}.0.{p[4]}'] = v
        else:
            out[top[p[0]] + '.' + p[1]] = v
    return out
