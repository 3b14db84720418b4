"""Shared by the LyCORIS tests (not a test module): the kernel cases with their inputs and fp64 expectations, the packings, synthetic
LoHa / LoKr adapters sized against the weights they adapt, and the kohya-named file dicts of them.

Kernel inputs have the spreads of tests/test_lora_kernel_gpu.py: W ~ 0.05 N(0, 1), factors ~ 0.2 N(0, 1), scale 0.37.  (With a factor
spread of 0.5 at rank 128 the fp32 restatement of the LoHa arithmetic reaches 9 fp16 ulp: the product of two 128-term sums then
dwarfs W and one fp32 rounding of it is several fp16 steps of the result.  0.2 keeps the update of W's own size.)"""
import torch

import lora_cases as LC

SCALE = 0.37


def ulp_diff(a, b):
    """distance in fp16 steps between two finite fp16 tensors (sign-magnitude bits mapped to a monotone integer line)"""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def geglu_pack(m):
    """rows of a canonical [2H, k] matrix in the engine's PK_LINEAR_GEGLU order: 16 value rows, then the 16 gate rows of the same block"""
    h = m.shape[0] // 2
    return torch.stack([m[:h].reshape(h // 16, 16, -1), m[h:].reshape(h // 16, 16, -1)], 1).reshape(m.shape)


def krsc_pack(m, cin):
    """columns of a canonical [n, cin * 9] matrix (j = c * 9 + t) in KRSC order (t * cin + c)"""
    return m.reshape(m.shape[0], cin, 9).permute(0, 2, 1).reshape(m.shape[0], 9 * cin).contiguous()


# ---------------------------------------------------------------------------------------------------------------- LoHa kernel cases
# id -> (n, k, rank, seed, conv_cin): the shapes of the issue -- tile remainders in both directions at four ranks (1, an odd one, one
# below the MFMA K step, the maximum), a column block, the GEGLU interleave, a 3x3 convolution
LOHA_CASES = {
    'plain_r1': (40, 72, 1, 101, 0), 'plain_r7': (40, 72, 7, 107, 0), 'plain_r16': (40, 72, 16, 116, 0), 'plain_r128': (40, 72, 128, 228, 0),
    'block': (72, 320, 8, 31, 0), 'geglu': (64, 72, 16, 32, 0), 'conv': (64, 288, 8, 33, 32),
    'wide_r128': (320, 768, 128, 34, 0),
}


def loha_inputs(case):
    """canonical fp16 (w [n, k], w1a [n, r], w1b [r, k] or [r, cin, 3, 3], w2a, w2b) of a LOHA_CASES id"""
    n, k, rank, seed, cin = LOHA_CASES[case]
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(n, k, generator=gen) * 0.05).half()
    bshape = (rank, cin, 3, 3) if cin else (rank, k)
    f = [(torch.randn(*s, generator=gen) * 0.2).half() for s in ((n, rank), bshape, (n, rank), bshape)]
    return (w, *f)


def loha_expected(w, w1a, w1b, w2a, w2b, scale):
    """canonical [n, k]: the definition in fp64 on the fp16 values, one rounding to fp16"""
    r = w1b.shape[0]
    return (w.double() + float(scale) * (w1a.double() @ w1b.double().reshape(r, -1)) * (w2a.double() @ w2b.double().reshape(r, -1))).half()


def loha_fp32_restatement(w, w1a, w1b, w2a, w2b, scale):
    """the kernel's arithmetic on the CPU: each product accumulated sequentially in fp32 (r ascending; an fp16 x fp16 product is exact in
    fp32, so `acc + a * b` rounds once, as the fused multiply-add does), the two sums multiplied in fp32, fma(scale, p1 * p2, W) rounded
    to fp32 once (scale * had is exact in fp64) and then to fp16"""
    r = w1b.shape[0]

    def prod(a, b):
        a, b = a.float(), b.float().reshape(r, -1)
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
        for i in range(r):
            acc = acc + a[:, i:i + 1] * b[i:i + 1]
        return acc

    had = prod(w1a, w1b) * prod(w2a, w2b)
    s32 = torch.tensor(float(scale), dtype=torch.float32).double()
    return (s32 * had.double() + w.double()).float().half()


# ---------------------------------------------------------------------------------------------------------------- LoKr kernel cases
def lokr_inputs(n, cin, a, b, seed, taps=1):
    """canonical fp16 (w [n, cin * taps], w1 [a, b], w2 [n / a, cin / b] or [n / a, cin / b, 3, 3])"""
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(n, cin * taps, generator=gen) * 0.05).half()
    w1 = (torch.randn(a, b, generator=gen) * 0.2).half()
    w2 = (torch.randn(*((n // a, cin // b) + ((3, 3) if taps == 9 else ())), generator=gen) * 0.2).half()
    return w, w1, w2


def lokr_expected(w, w1, w2, scale):
    """canonical [n, k]: W + scale * kron(w1, w2) in fp64 (torch.kron; a 4-D w2 takes w1 as [a, b, 1, 1]), one rounding to fp16"""
    w1 = w1.double()
    kr = torch.kron(w1[:, :, None, None] if w2.dim() == 4 else w1, w2.double().contiguous())
    return (w.double() + float(scale) * kr.reshape(w.shape)).half()


# ---------------------------------------------------------------------------------------------------------------- adapters for graphs
LOKR_SPLITS = ((4, 8), (2, 64), (16, 4), (1, 1))   # b = 64 leaves d = 5, 10, 12, 15 .. on the SD widths: mostly no multiple of 8; (1, 1) is a full diff


def make_loha_entries(sd, names, rank, scale, seed):
    """[('loha', name, w1a, w1b, w2a, w2b, scale)]: each low-rank product has the spread sqrt(std(W)), so that their Hadamard product has
    the weight's own and `scale` is the update's size relative to it"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in names:
        w = sd[n]
        s = float(w.float().std()) ** 0.5
        f = []
        for _ in range(2):
            f.append(torch.randn(w.shape[0], rank, generator=gen).half())
            f.append((torch.randn(rank, *w.shape[1:], generator=gen) * (s / rank ** 0.5)).half())
        out.append(('loha', n, *f, float(scale)))
    return out


def make_lokr_entries(sd, names, scale, seed):
    """[('lokr', name, w1, w2, scale)] with w1 [a, b] ~ N(0, 1) and w2 ~ N(0, 1) * std(W), the split cycling through LOKR_SPLITS"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(names):
        w = sd[n]
        a, b = LOKR_SPLITS[i % len(LOKR_SPLITS)]
        w1 = torch.randn(a, b, generator=gen).half()
        w2 = (torch.randn(w.shape[0] // a, w.shape[1] // b, *w.shape[2:], generator=gen) * float(w.float().std())).half()
        out.append(('lokr', n, w1, w2, float(scale)))
    return out


def file_dict(entries, alpha=None):
    """a kohya / LyCORIS-named tensor dict of bare entries (plain 4-tuples, 'loha', 'lokr'); their scale is dropped: the reader derives
    it from alpha and the strength.  A 'lokr' entry with a 1 x 1 w1 is written as a full `diff` of w1 * w2."""
    out = {}
    for e in entries:
        if len(e) == 4:
            k = LC.kohya_key(e[0])
            out[f'{k}.lora_up.weight'], out[f'{k}.lora_down.weight'] = e[1].contiguous(), e[2].contiguous()
        elif e[0] == 'loha':
            k = LC.kohya_key(e[1])
            for nme, t in zip(('hada_w1_a', 'hada_w1_b', 'hada_w2_a', 'hada_w2_b'), e[2:6]):
                out[f'{k}.{nme}'] = t.reshape(t.shape[0], -1).contiguous()
        else:
            k = LC.kohya_key(e[1])
            if e[2].numel() == 1:
                out[f'{k}.diff'] = (e[2].double().reshape(()) * e[3].double()).to(e[3].dtype).contiguous()
                continue
            out[f'{k}.lokr_w1'], out[f'{k}.lokr_w2'] = e[2].contiguous(), e[3].contiguous()
        if alpha is not None:
            out[f'{k}.alpha'] = torch.tensor(float(alpha))
    return out
