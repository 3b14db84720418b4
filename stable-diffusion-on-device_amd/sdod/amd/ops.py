"""Thin torch-tensor wrappers over the kernel-level C ABI (include/sdod_hip.h).

torch supplies device memory and the current stream only; every computation below is a call into
lib/libsdod.so.  Activations are NHWC fp16; a torch NCHW tensor in channels_last memory format
IS that layout, so the conversions are views."""
import ctypes

import torch

from . import _lib
from ._lib import GemmDesc, check

ACT = {None: 0, 'none': 0, 'silu': 1, 'gelu': 2, 'quick_gelu': 3, 'relu': 4}   # 'relu': activation() only, not a GEMM epilogue


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _req(t, dtype=None, name='tensor'):
    if not t.is_cuda:
        raise ValueError(f'{name} must live on the GPU')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f'{name} must be {dtype}, got {t.dtype}')
    return t


def _req_out(out, like, numel, name='out'):
    """a caller's destination (or second operand) of a kernel that takes bare pointers: fp16, contiguous, of exactly `numel` elements
    and on the device of `like`, whose own _req follows and settles that this is the GPU.  Raises before the library is loaded."""
    if out.dtype != torch.float16:
        raise ValueError(f'{name} must be {torch.float16}, got {out.dtype}')
    if not out.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    if out.numel() != numel:
        raise ValueError(f'{name} must hold {numel} elements, got {out.numel()}')
    if out.device != like.device:
        raise ValueError(f'{name} must live on {like.device}, got {out.device}')
    return out


def _ld(t, dtype, name, width, mult=8):
    """Row stride (elements) of a GEMM matrix operand of `width` columns: a contiguous tensor is dense (the width, whatever its
    shape); a 2-D view with unit column stride (a column range of wider rows) gives its row stride, which must be a multiple
    of `mult` elements."""
    if t.is_contiguous():   # (also a ONE-row view into wider rows: torch calls it contiguous, and one row has no stride to honour)
        _req(t, dtype, name)
        return width
    if not t.is_cuda:
        raise ValueError(f'{name} must live on the GPU')
    if t.dtype != dtype:
        raise ValueError(f'{name} must be {dtype}, got {t.dtype}')
    if t.dim() != 2 or t.shape[1] != width or t.stride(1) != 1 or t.stride(0) < width or t.stride(0) % mult:
        raise ValueError(f'{name} must be contiguous or a 2-D view with unit column stride and a row stride that is a multiple of {mult}')
    return t.stride(0)


def _affine(weight, bias, c, device):
    """fp32 weight and bias for the kernels, which take both or neither: a missing one of the two becomes ones / zeros on the
    device (F.group_norm accepts either alone)."""
    if weight is None and bias is None:
        return None, None
    weight = torch.ones(c, dtype=torch.float32, device=device) if weight is None else weight.detach().to(torch.float32).contiguous()
    bias = torch.zeros(c, dtype=torch.float32, device=device) if bias is None else bias.detach().to(torch.float32).contiguous()
    return weight, bias


_ws = {}


def workspace(nbytes, device, tag='default'):
    """Grow-only fp32 scratch per (device, tag); reused across calls on the same stream."""
    key = (device, tag)
    buf = _ws.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        # zeroed: the one-launch GroupNorm keeps its grid-barrier words at the end of its workspace (include/sdod_hip.h)
        buf = torch.zeros((max(nbytes, 1) + 3) // 4, dtype=torch.float32, device=device)
        _ws[key] = buf
    return buf


def gemm(a, w, bias=None, *, residual=None, row_bias=None, rows_per_img=0, act=None, alpha=1.0, out=None,
         conv=None, a2=None, bias_on_m=False, split_k=0, tile=0, time_iters=0, geglu=False, tail=None, bias2=None,
         ln_s=None, ln_eps=1e-5, cold_scratch=None, phase=0, return_desc=False, w_scale=None, w_off=None, fixup=False,
         xcd=0, softmax_cols=0, region_w=None, regions=0):
    """out = act(alpha * A @ W^T + bias + row_bias) + residual.

    The matrix operands (a in rows mode, w, out, residual, row_bias) are contiguous or 2-D views with unit column stride into
    wider rows (row stride a multiple of 8 elements, 16 for uint8 w): lda / ldw / ldo / ldr / ld_row_bias are their row strides.
    a: fp16 [M, K] (rows mode) or NHWC [N, H, W, C0] with conv=dict(stride=1|2, upsample=bool) (3x3 pad 1);
    conv=dict(stride=2, pad_mode=1): ldm's VAE-encoder Downsample, F.pad(a, (0, 1, 0, 1)) then a 3x3 stride-2 pad-0 conv;
    conv=dict(pad_mode=2 | 3 | 4): seamless tiling, the 3x3 pad-1 border is circular on both axes / x only / y only;
    a2: optional second NHWC source concatenated on channels; w: fp16 [Nout, K] (conv: K = 9*(C0+C1), KRSC).
    region_w (fp32 [rows_per_img, regions]) with regions >= 1: sdod_gemm_region_f16, the softmax epilogue's 80-column groups are laid
    out [region][head][80] and group g's probabilities at row m are multiplied by region_w[m % rows_per_img, g // (Nout / 80 / regions)];
    the checks are the library's."""
    lib = _lib.hip()
    lda = _ld(a, torch.float16, 'a', a.shape[-1]) if conv is None else _req(a, torch.float16, 'a').shape[-1]
    d = GemmDesc()
    if w_scale is not None:   # affine-uint8 weight codes: real = (q + offset) * scale, w_off = offset + 128 per output column
        ldw = _ld(w, torch.uint8, 'w', w.shape[-1], 16); _req(w_scale, torch.float32, 'w_scale'); _req(w_off, torch.float32, 'w_off')
        d.wq = 1; d.w_scale = _p(w_scale); d.w_off = _p(w_off)
    else:
        ldw = _ld(w, torch.float16, 'w', w.shape[-1])
    per_image = w.dim() == 3   # [n_img, Nout, K]: the rows of image i (rows_per_img each) multiply w[i]; bias / ln_s may be [n_img, Nout]
    nout, k = w.shape[-2:]
    if per_image:
        assert conv is None and rows_per_img > 0 and w.is_contiguous()
        d.w_img_stride = nout * k
        d.rows_per_img = rows_per_img
        if (bias is not None and bias.dim() == 2) or (ln_s is not None and ln_s.dim() == 2):
            assert (bias is None or bias.dim() == 2) and (ln_s is None or ln_s.dim() == 2)
            d.vec_img_stride = nout
    d.softmax_cols = softmax_cols
    if conv is None:
        m = a.shape[0]
        assert a.shape[1] == k, (a.shape, w.shape)
        d.a_mode = 0
        d.lda = lda
        out_shape = (m, nout)
    else:
        n_img, h, wd, c0 = a.shape
        c1 = 0
        if a2 is not None:
            _req(a2, torch.float16, 'a2')
            assert a2.shape[:3] == a.shape[:3]
            c1 = a2.shape[3]
        stride = int(conv.get('stride', 1)); ups = 1 if conv.get('upsample', False) else 0
        ks = int(conv.get('ksize', 3))
        pad_mode = int(conv.get('pad_mode', 0))
        pad_sum = 1 if pad_mode == 1 else 2 * (ks // 2)   # (2 / 3 / 4: the circular borders, same output size as 0)
        hup, wup = h << ups, wd << ups
        ho, wo = (hup + pad_sum - ks) // stride + 1, (wup + pad_sum - ks) // stride + 1
        d.ksize = ks
        d.pad_mode = pad_mode
        m = n_img * ho * wo
        d.a_mode = 1
        d.n_img, d.h_in, d.w_in, d.c0, d.c1 = n_img, h, wd, c0, c1
        d.stride, d.upsample = stride, ups
        d.a2 = _p(a2)
        out_shape = (n_img, ho, wo, nout)
    nvis = nout // 2 if geglu else nout
    if geglu:
        out_shape = out_shape[:-1] + (nvis,)
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float16, device=a.device)
    else:
        assert out.numel() == m * nvis
    d.a, d.w, d.out = _p(a), _p(w), _p(out)
    d.M, d.N, d.K = m, nout, k
    d.ldw, d.ldo = ldw, _ld(out, torch.float16, 'out', nvis)
    d.geglu = 1 if geglu else 0
    if tail is not None:      # (t0, t1 or None): NHWC tensors read by the 1x1 tail segment; w holds [main K | tail K] columns
        t0, t1 = tail
        d.t0 = _p(t0); d.tc0 = t0.shape[-1]
        d.t1 = _p(t1); d.tc1 = t1.shape[-1] if t1 is not None else 0
        d.k_tail = k - d.tc0 - d.tc1
    if bias2 is not None:
        _req(bias2, torch.float32, 'bias2'); d.bias2 = _p(bias2)
    if ln_s is not None:      # LayerNorm folded into this Linear: w / bias / ln_s come from ln_fold()
        _req(ln_s, torch.float32, 'ln_s'); d.ln = 1; d.ln_s = _p(ln_s); d.ln_eps = ln_eps
    if bias is not None:
        _req(bias, torch.float32, 'bias'); d.bias = _p(bias)
    if row_bias is not None:
        d.ld_row_bias = _ld(row_bias, torch.float16, 'row_bias', row_bias.shape[-1]); d.row_bias = _p(row_bias); d.rows_per_img = rows_per_img
    if residual is not None:
        assert residual.numel() == m * nout
        d.residual = _p(residual); d.ldr = _ld(residual, torch.float16, 'residual', nout)
    d.act = ACT[act]
    d.alpha = alpha
    d.bias_on_m = 1 if bias_on_m else 0
    d.split_k = split_k
    d.tile = tile
    d.xcd_panels = xcd        # 0 = per-shape choice; 1 / 2 / 4 / 8 = n-tile panels of the XCD-aware tile order (speed only)
    need = lib.sdod_gemm_workspace_bytes(ctypes.byref(d))
    if need:
        ws = workspace(need, a.device, 'gemm')
        d.workspace = _p(ws); d.workspace_bytes = ws.numel() * 4
        if fixup:   # split-K reduced inside the GEMM launch where the tile supports it (zeroed counters, see include/sdod_hip.h)
            d.fix_counters = _p(workspace(lib.sdod_gemm_fixup_counters() * 4, a.device, 'gemm_fixup'))
    if time_iters:
        ms = ctypes.c_float()
        if cold_scratch is not None:   # cold weights, warm activations: what the launch meets inside a graph replay
            check(lib.sdod_gemm_time_cold(ctypes.byref(d), _stream(), min(time_iters, 16), _p(cold_scratch),
                                          cold_scratch.numel() * cold_scratch.element_size(), ctypes.byref(ms), None))
        else:
            check(lib.sdod_gemm_time(ctypes.byref(d), _stream(), time_iters, ctypes.byref(ms)))
        return ms.value
    d.phase = phase           # split-K only: 1 = partial slabs only (a GroupNorm may finish the job, group_norm_reduce)
    if region_w is not None or regions:
        check(lib.sdod_gemm_region_f16(ctypes.byref(d), _p(region_w), int(regions), _stream()))
    else:
        check(lib.sdod_gemm_f16(ctypes.byref(d), _stream()))
    if return_desc:
        d._keep = (a, w, bias, residual, row_bias, out, a2, bias2)   # the descriptor holds raw pointers
        return out, d
    return out


class GnReduce(ctypes.Structure):
    """mirror of `struct sdod_gn_reduce`"""
    _fields_ = [('partial', ctypes.c_void_p), ('splits', ctypes.c_int), ('slab_floats', ctypes.c_size_t), ('bias', ctypes.c_void_p),
                ('bias2', ctypes.c_void_p), ('row_bias', ctypes.c_void_p), ('ld_row_bias', ctypes.c_int), ('residual', ctypes.c_void_p),
                ('ldr', ctypes.c_int), ('x_out', ctypes.c_void_p), ('alpha', ctypes.c_float), ('act', ctypes.c_int),
                ('M', ctypes.c_int), ('N', ctypes.c_int)]


def group_norm_reduce(desc, n, hw, groups, weight=None, bias=None, eps=1e-5, silu=False, x2=None):
    """GroupNorm(+SiLU) of the output of a split-K GEMM launched with phase=1 (desc from gemm(..., return_desc=True)): the
    reduce + epilogue of that GEMM and the normalisation in one launch.  Returns y; x lands in the GEMM's `out`."""
    lib = _lib.hip()
    red = GnReduce()
    check(lib.sdod_gemm_reduce_info(ctypes.byref(desc), ctypes.byref(red)))
    c0 = desc.N
    c1 = x2.shape[-1] if x2 is not None else 0
    dev = desc._keep[0].device
    y = torch.empty((n, hw, c0 + c1), dtype=torch.float16, device=dev)
    weight, bias = _affine(weight, bias, c0 + c1, dev)
    check(lib.sdod_group_norm_reduce_nhwc(ctypes.byref(red), _p(x2), _p(y), _p(weight), _p(bias), n, hw, c0, c1, groups, eps,
                                          1 if silu else 0, _stream()))
    return y


def group_norm_nhwc(x, groups, weight=None, bias=None, eps=1e-5, silu=False, x2=None, out=None):
    """x: [N, ..., C] channels-last fp16/fp32 (optionally concatenated with x2 on C)."""
    lib = _lib.hip()
    _req(x, None, 'x')
    assert x.dtype in (torch.float16, torch.float32)
    n, c0 = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c0)
    c1 = 0
    if x2 is not None:
        _req(x2, x.dtype, 'x2'); c1 = x2.shape[-1]
    if out is None:
        out = torch.empty(x.shape[:-1] + (c0 + c1,), dtype=x.dtype, device=x.device)
    weight, bias = _affine(weight, bias, c0 + c1, x.device)
    ws = workspace(lib.sdod_group_norm_workspace_bytes(n, groups), x.device, 'gn')
    check(lib.sdod_group_norm_nhwc(_p(x), _p(x2), _p(out), _p(weight), _p(bias), n, hw, c0, c1, groups, eps,
                                   1 if silu else 0, 0 if x.dtype == torch.float16 else 1, _p(ws), _stream()))
    return out


_NCHW_DTYPES = {torch.float16: 0, torch.float32: 1, torch.bfloat16: 3}


def group_norm_nchw(x, groups, weight=None, bias=None, eps=1e-5, silu=False, out=None):
    """torch-semantics entry used by sdod.EfficientGN: x is [N, C, *] fp16 / bf16 / fp32; returns a tensor of the same shape
    and memory format.  No layout copy where it can be avoided: a channels_last tensor whose shape an NHWC kernel takes
    (sdod_group_norm_path >= 0) IS their layout (the permute is a view); anything else that is dense goes to the NCHW kernel,
    where a group is one contiguous slab (any channel count).  A tensor that is neither -- and a channels_last tensor that no
    NHWC kernel takes (too many channels for their LDS tables) -- is made contiguous first, and a channels_last result is
    given back in channels_last.  `out` (optional): a tensor of x's shape, dtype and memory format to write, which may be x."""
    if x.dtype not in _NCHW_DTYPES:
        raise TypeError('EfficientGN HIP kernels support float16, bfloat16 and float32')
    n, c = x.shape[0], x.shape[1]
    x = x.detach()
    lib = _lib.hip()
    if (x.dim() == 4 and c % 8 == 0 and x.dtype != torch.bfloat16 and not x.is_contiguous()
            and x.is_contiguous(memory_format=torch.channels_last)):
        hw = x.shape[2] * x.shape[3]
        if lib.sdod_group_norm_path(n, hw, c, 0, groups, 0 if x.dtype == torch.float16 else 1) >= 0:
            o = None
            if out is not None:
                if not (out.shape == x.shape and out.dtype == x.dtype and out.is_contiguous(memory_format=torch.channels_last)):
                    raise ValueError('out must match x in shape, dtype and memory format')
                o = out.permute(0, 2, 3, 1)
            y = group_norm_nhwc(x.permute(0, 2, 3, 1), groups, weight, bias, eps, silu, out=o)  # [N, H, W, C] view -> NHWC kernels
            return y.permute(0, 3, 1, 2)                                                      # logical NCHW, channels_last strides
    back_to_cl = False
    if not x.is_contiguous():
        back_to_cl = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
        x = x.contiguous()
    _req(x, None, 'x')
    dst = torch.empty_like(x)
    if out is not None:
        if out.shape != x.shape or out.dtype != x.dtype:
            raise ValueError('out must match x in shape and dtype')
        if out.is_contiguous():
            dst = out
        elif not (back_to_cl and out.is_contiguous(memory_format=torch.channels_last)):
            raise ValueError('out must have the memory format of x')
    weight, bias = _affine(weight, bias, c, x.device)
    spatial = x.numel() // (n * c)
    ws = workspace(lib.sdod_group_norm_nchw_workspace_bytes(n, groups), x.device, 'gn_nchw')
    check(lib.sdod_group_norm_nchw(_p(x), _p(dst), _p(weight), _p(bias), n, c, spatial, groups, eps, 1 if silu else 0,
                                   _NCHW_DTYPES[x.dtype], _p(ws), _stream()))
    if back_to_cl:
        if out is not None and dst is not out:
            return out.copy_(dst)
        return dst.contiguous(memory_format=torch.channels_last)
    return dst


def ln_fold(w, gamma, beta, bias=None):
    """fold LayerNorm(gamma, beta) into Linear(w, bias): returns (w_folded fp16, s fp32, t fp32); w is modified in place"""
    lib = _lib.hip()
    _req(w, torch.float16, 'w'); _req(gamma, torch.float32, 'gamma'); _req(beta, torch.float32, 'beta')
    n, k = w.shape
    s = torch.empty(n, dtype=torch.float32, device=w.device); t = torch.empty_like(s)
    check(lib.sdod_ln_fold_f16(_p(w), n, k, k, _p(gamma), _p(beta), _p(bias), _p(s), _p(t), _stream()))
    return w, s, t


def lora_merge(w, up, down, scale, *, ld=None, conv_cin=None, geglu=False):
    """w += scale * up @ down in place on a PACKED fp16 weight matrix (sdod_lora_merge_f16): w is [n][ld] fp16 on the device, of
    which k columns are updated (a 2-D view of a wider matrix brings its own row stride; ld overrides it); up [n, rank] and down
    [rank, k] (a 3x3 convolution: [rank, cin, 3, 3]) are fp16 device tensors in canonical order.  conv_cin: w's columns are in
    KRSC order (t * cin + c); geglu: w's rows carry the 16-row value / gate interleave.  Returns w."""
    lib = _lib.hip()
    for t, nme in ((w, 'w'), (up, 'up'), (down, 'down')):
        if not t.is_cuda or t.dtype != torch.float16:
            raise ValueError(f'{nme} must be an fp16 tensor on the GPU')
    _req(up, torch.float16, 'up'); _req(down, torch.float16, 'down')
    if up.dim() != 2 or w.stride(-1) != 1:
        raise ValueError('up must be [n, rank] and the columns of w contiguous')
    n, rank = up.shape
    k = down.numel() // rank if rank else (down.shape[-1] if down.dim() > 1 else 0)
    if ld is None:
        ld = w.stride(0) if w.dim() == 2 and w.shape[0] > 1 else k
    check(lib.sdod_lora_merge_f16(_p(w), n, k, int(ld), _p(up), _p(down), rank, float(scale), int(conv_cin or 0), 1 if geglu else 0,
                                  _stream()))
    return w


def _packed_ld(w, k, ld):
    if ld is not None:
        return int(ld)
    return w.stride(0) if w.dim() == 2 and w.shape[0] > 1 else k


def loha_merge(w, w1a, w1b, w2a, w2b, scale, *, ld=None, conv_cin=None, geglu=False):
    """w += scale * (w1a @ w1b) * (w2a @ w2b) (Hadamard product) in place on a PACKED fp16 weight matrix (sdod_loha_merge_f16): w, ld,
    conv_cin and geglu as in lora_merge; w1a, w2a [n, rank] and w1b, w2b [rank, k] ([rank, cin, 3, 3]) are fp16 device tensors in
    canonical order.  Returns w."""
    lib = _lib.hip()
    for t, nme in ((w, 'w'), (w1a, 'w1a'), (w1b, 'w1b'), (w2a, 'w2a'), (w2b, 'w2b')):
        if not t.is_cuda or t.dtype != torch.float16:
            raise ValueError(f'{nme} must be an fp16 tensor on the GPU')
        if t is not w:
            _req(t, torch.float16, nme)
    if w1a.dim() != 2 or w2a.shape != w1a.shape or w2b.shape != w1b.shape or w.stride(-1) != 1:
        raise ValueError('w1a and w2a must be [n, rank], w1b and w2b of one shape, and the columns of w contiguous')
    n, rank = w1a.shape
    k = w1b.numel() // rank if rank else (w1b.shape[-1] if w1b.dim() > 1 else 0)
    check(lib.sdod_loha_merge_f16(_p(w), n, k, _packed_ld(w, k, ld), _p(w1a), _p(w1b), _p(w2a), _p(w2b), rank, float(scale),
                                  int(conv_cin or 0), 1 if geglu else 0, _stream()))
    return w


def lokr_merge(w, w1, w2, scale, *, ld=None, conv_cin=None, geglu=False):
    """w += scale * kron(w1, w2) in place on a PACKED fp16 weight matrix (sdod_lokr_merge_f16): w, ld, conv_cin and geglu as in
    lora_merge; w1 [a, b] and w2 [c, d] ([c, d, 3, 3] with conv_cin = b * d) are fp16 device tensors in canonical order; the matrix
    has a * c rows.  Returns w."""
    lib = _lib.hip()
    for t, nme in ((w, 'w'), (w1, 'w1'), (w2, 'w2')):
        if not t.is_cuda or t.dtype != torch.float16:
            raise ValueError(f'{nme} must be an fp16 tensor on the GPU')
    _req(w1, torch.float16, 'w1'); _req(w2, torch.float16, 'w2')
    if w1.dim() != 2 or w2.dim() < 2 or w.stride(-1) != 1:
        raise ValueError('w1 must be [a, b], w2 [c, d] or [c, d, 3, 3], and the columns of w contiguous')
    a, b = w1.shape
    n, k = a * w2.shape[0], b * (w2.numel() // w2.shape[0])
    check(lib.sdod_lokr_merge_f16(_p(w), n, k, _packed_ld(w, k, ld), _p(w1), a, b, _p(w2), float(scale), int(conv_cin or 0),
                                  1 if geglu else 0, _stream()))
    return w


def layer_norm(x, weight, bias, eps=1e-5, out=None):
    lib = _lib.hip()
    _req(x, torch.float16, 'x')
    c = x.shape[-1]; m = x.numel() // c
    if out is None:
        out = torch.empty_like(x)
    check(lib.sdod_layer_norm_f16(_p(x), _p(out), _p(weight), _p(bias), m, c, eps, _stream()))
    return out


def attention(q, k, v, heads, scale=None, causal=False, out=None):
    """q: [B, Lq, heads*d], k/v: [B, Lk, heads*d] fp16 (row strides = last-dim size)."""
    lib = _lib.hip()
    for t, nme in ((q, 'q'), (k, 'k'), (v, 'v')):
        _req(t, torch.float16, nme)
    b, lq, c = q.shape
    lk = k.shape[1]
    d = c // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty_like(q)
    check(lib.sdod_attention_f16(_p(q), _p(k), _p(v), _p(out), b, heads, lq, lk, d, q.shape[2], k.shape[2], v.shape[2],
                                 out.shape[2], scale, 1 if causal else 0, _stream()))
    return out


def xattn_fold(kv, k_off, v_off, n_img, L, wq, sq, tq, wo, heads, scale=None, regions=None):
    """once-per-prompt part of the folded cross-attention (include/sdod_hip.h: sdod_xattn_fold_f16).  kv: fp16 [n_img * L, ld]
    holding K at column k_off and V at v_off; wq: LayerNorm-folded to_q weight with its fold vectors sq, tq (ln_fold); wo: to_out
    weight.  Returns (w1 [n_img, heads*80, C], s1, t1 [n_img, heads*80], w2 [n_img, C, heads*80]).
    regions=k (sdod_xattn_fold_regions_f16): kv is [n_img * k * L, ld], one segment per (image, region prompt); returns
    (w1 [n_img, k*heads*80, C], s1, t1 [n_img, k*heads*80], w2 [n_img, C, k*heads*80]), region-major."""
    lib = _lib.hip()
    _req(kv, torch.float16, 'kv'); _req(wq, torch.float16, 'wq'); _req(wo, torch.float16, 'wo')
    _req(sq, torch.float32, 'sq'); _req(tq, torch.float32, 'tq')
    c = wq.shape[0]; d = c // heads
    if scale is None:
        scale = d ** -0.5
    nk = heads * 80 * (1 if regions is None else int(regions))
    w1 = torch.empty(n_img, nk, c, dtype=torch.float16, device=kv.device)
    w2 = torch.empty(n_img, c, nk, dtype=torch.float16, device=kv.device)
    s1 = torch.empty(n_img, nk, dtype=torch.float32, device=kv.device); t1 = torch.empty_like(s1)
    if regions is not None:
        check(lib.sdod_xattn_fold_regions_f16(_p(kv), kv.shape[-1], k_off, v_off, n_img, int(regions), L, _p(wq), wq.shape[1], _p(sq), _p(tq),
                                              _p(wo), wo.shape[1], heads, d, scale, _p(w1), _p(s1), _p(t1), _p(w2), _stream()))
        return w1, s1, t1, w2
    check(lib.sdod_xattn_fold_f16(_p(kv), kv.shape[-1], k_off, v_off, n_img, L, _p(wq), wq.shape[1], _p(sq), _p(tq), _p(wo), wo.shape[1],
                                  heads, d, scale, _p(w1), _p(s1), _p(t1), _p(w2), _stream()))
    return w1, s1, t1, w2


def xattn_fold_ip(kv, k_off, v_off, kv_ip, k_off_ip, v_off_ip, n_img, L, T, wq, sq, tq, wo, heads, scale=None):
    """the fold on two sources per image (sdod_xattn_fold_ip_f16): text K/V [n_img * L, ld] and image-token K/V [n_img * T, ld_ip].
    Returns (w1 [n_img, 2*heads*80, C], s1, t1 [n_img, 2*heads*80], w2 [n_img, C, 2*heads*80]); segment 0 = text, 1 = image."""
    lib = _lib.hip()
    _req(kv, torch.float16, 'kv'); _req(kv_ip, torch.float16, 'kv_ip'); _req(wq, torch.float16, 'wq'); _req(wo, torch.float16, 'wo')
    _req(sq, torch.float32, 'sq'); _req(tq, torch.float32, 'tq')
    c = wq.shape[0]; d = c // heads
    if kv.shape[0] < n_img * L or kv_ip.shape[0] < n_img * T:
        raise ValueError(f'kv needs {n_img * L} rows and kv_ip {n_img * T}, got {kv.shape[0]} and {kv_ip.shape[0]}')
    if scale is None:
        scale = d ** -0.5
    nk = heads * 80 * 2
    w1 = torch.empty(n_img, nk, c, dtype=torch.float16, device=kv.device)
    w2 = torch.empty(n_img, c, nk, dtype=torch.float16, device=kv.device)
    s1 = torch.empty(n_img, nk, dtype=torch.float32, device=kv.device); t1 = torch.empty_like(s1)
    check(lib.sdod_xattn_fold_ip_f16(_p(kv), kv.shape[-1], k_off, v_off, _p(kv_ip), kv_ip.shape[-1], k_off_ip, v_off_ip, n_img, L, T,
                                     _p(wq), wq.shape[1], _p(sq), _p(tq), _p(wo), wo.shape[1], heads, d, scale, _p(w1), _p(s1), _p(t1), _p(w2),
                                     _stream()))
    return w1, s1, t1, w2


def attention_strided(q, k, v, out, batch, heads, lq, lk, d, ldq, ldk, ldv, ldo, scale, causal=False):
    """raw form for packed qkv buffers: pointers may be column offsets into wider rows"""
    lib = _lib.hip()
    check(lib.sdod_attention_f16(q, k, v, out, batch, heads, lq, lk, d, ldq, ldk, ldv, ldo, scale, 1 if causal else 0,
                                 _stream()))


def softmax_rows(x, out=None):
    if out is not None:
        _req_out(out, x, x.numel())
    _req(x, torch.float16, 'x')
    lib = _lib.hip()
    n = x.shape[-1]; m = x.numel() // n
    if out is None:
        out = torch.empty_like(x)
    check(lib.sdod_softmax_rows_f16(_p(x), _p(out), m, n, _stream()))
    return out


def geglu(x, out=None):
    if out is not None:
        _req_out(out, x, x.numel() // 2)
    _req(x, torch.float16, 'x')
    lib = _lib.hip()
    c = x.shape[-1] // 2; m = x.numel() // (2 * c)
    if out is None:
        out = torch.empty(x.shape[:-1] + (c,), dtype=torch.float16, device=x.device)
    check(lib.sdod_geglu_f16(_p(x), _p(out), m, c, _stream()))
    return out


def activation(x, act, out=None):
    if out is not None:
        _req_out(out, x, x.numel())
    _req(x, torch.float16, 'x')
    lib = _lib.hip()
    if out is None:
        out = torch.empty_like(x)
    check(lib.sdod_act_f16(_p(x), _p(out), x.numel(), ACT[act], _stream()))
    return out


def add(a, b, out=None):
    _req_out(b, a, a.numel(), 'b')
    if out is not None:
        _req_out(out, a, a.numel())
    _req(a, torch.float16, 'a')
    lib = _lib.hip()
    if out is None:
        out = torch.empty_like(a)
    check(lib.sdod_add_f16(_p(a), _p(b), _p(out), a.numel(), _stream()))
    return out


def pixel_unshuffle_u8(img_u8, factor=8, out=None):
    """the T2I-Adapter's input (sdod_pixel_unshuffle_u8_f16): uint8 HWC [n, 8h, 8w, ch] -> fp16 NHWC [n, h, w, 64 ch] = img / 255 in
    torch.nn.PixelUnshuffle(8)'s channel order (c * 64 + dy * 8 + dx); ch 1 or 3"""
    lib = _lib.hip()
    _req(img_u8, torch.uint8, 'img')
    n, ih, iw, ch = img_u8.shape
    h, w = ih // factor, iw // factor
    assert ih == h * factor and iw == w * factor, img_u8.shape
    if out is None:
        out = torch.empty((n, h, w, ch * factor * factor), dtype=torch.float16, device=img_u8.device)
    else:
        _req(out, torch.float16, 'out')
        assert out.numel() == img_u8.numel(), (out.shape, img_u8.shape)
    check(lib.sdod_pixel_unshuffle_u8_f16(_p(img_u8), _p(out), n, h, w, ch, factor, _stream()))
    return out


def avg_pool2(x, out=None):
    """AvgPool2d(2) on NHWC fp16 [n, h, w, c] (sdod_avg_pool2_f16): ((a + b) + (c + d)) * 0.25 in fp32; h, w even, c % 8 == 0"""
    lib = _lib.hip()
    _req(x, torch.float16, 'x')
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, h // 2, w // 2, c), dtype=torch.float16, device=x.device)
    else:
        _req(out, torch.float16, 'out')
        assert out.numel() * 4 == x.numel(), (out.shape, x.shape)
    check(lib.sdod_avg_pool2_f16(_p(x), _p(out), n, h, w, c, _stream()))
    return out


def adapter_stage(src, dst, weight=1.0):
    """dst = fp16(weight * src) (sdod_adapter_stage_f16): an adapter output into a feature slot of the UNet, the conditioning weight
    folded in"""
    lib = _lib.hip()
    _req(src, torch.float16, 'src'); _req(dst, torch.float16, 'dst')
    assert dst.numel() == src.numel(), (dst.shape, src.shape)
    check(lib.sdod_adapter_stage_f16(_p(src), _p(dst), src.numel(), float(weight), _stream()))
    return dst


def add_feature(h, f, reps):
    """h fp16 [reps * per_copy] += f fp16 [per_copy] for each of the reps (1 or 2) guidance copies, in place (sdod_add_feature_f16:
    the launch a UNet graph with adapter inputs makes at four places per evaluation)"""
    lib = _lib.hip()
    _req(h, torch.float16, 'h'); _req(f, torch.float16, 'f')
    assert h.numel() == reps * f.numel(), (h.shape, f.shape, reps)
    check(lib.sdod_add_feature_f16(_p(h), _p(f), f.numel(), reps, _stream()))
    return h


def add_control(hs, rs, scales):
    """hs[k] += scales[k] * rs[k] in place for up to 16 fp16 tensor pairs in ONE launch (sdod_add_control_f16: the launch a UNet
    graph with ControlNet inputs makes behind its middle block).  scales: fp32 device tensor [len(hs)], read by the kernel; a segment
    whose scale is exactly 0 is neither read nor written.  The pointer and size checks are the library's."""
    lib = _lib.hip()
    if len(hs) != len(rs):
        raise ValueError(f'{len(hs)} destinations but {len(rs)} residuals')
    for k, (h, r) in enumerate(zip(hs, rs)):
        _req(h, torch.float16, f'hs[{k}]'); _req(r, torch.float16, f'rs[{k}]')
        if h.numel() != r.numel():
            raise ValueError(f'segment {k}: {tuple(h.shape)} and {tuple(r.shape)} differ in size')
    _req(scales, torch.float32, 'scales')
    if scales.numel() != len(hs):
        raise ValueError(f'{len(hs)} segments need {len(hs)} scales, got {scales.numel()}')
    segs = (_lib.ControlSeg * max(len(hs), 1))(*[_lib.ControlSeg(h.data_ptr(), r.data_ptr(), h.numel()) for h, r in zip(hs, rs)])
    check(lib.sdod_add_control_f16(segs, len(hs), _p(scales), _stream()))
    return hs


def freeu(h, skip, params, stage, scratch=None, phases=3):
    """FreeU at one decoder site, in place on the fp16 NHWC tensors h and skip, both [n, H, W, C] (sdod_freeu_f16: the two launches a
    UNet graph with the FreeU switch makes there).  params: fp32 device tensor [8] = (b1, s1, b2, s2, version, 0, 0, 0), read by the
    kernels; stage 1 uses (b1, s1), stage 2 (b2, s2).  scratch: fp32 device tensor of n * H * W elements (the channel means version 2
    needs), allocated when None.  The pointer, size and alignment checks are the library's."""
    lib = _lib.hip()
    _req(h, torch.float16, 'h'); _req(skip, torch.float16, 'skip'); _req(params, torch.float32, 'params')
    if h.dim() != 4 or h.shape != skip.shape:
        raise ValueError(f'h and skip must be [n, H, W, C] tensors of one shape, not {tuple(h.shape)} and {tuple(skip.shape)}')
    if params.numel() != 8:
        raise ValueError(f'params must hold 8 floats (b1, s1, b2, s2, version, 0, 0, 0), not {params.numel()}')
    n, hh, ww, c = h.shape
    if scratch is None:
        scratch = torch.empty(max(n * hh * ww, 1), dtype=torch.float32, device=h.device)
    _req(scratch, torch.float32, 'scratch')
    if scratch.numel() < n * hh * ww:
        raise ValueError(f'scratch must hold n * H * W = {n * hh * ww} floats, not {scratch.numel()}')
    check(lib.sdod_freeu_f16(_p(h), _p(skip), n, hh, ww, c, _p(params), int(stage), _p(scratch), int(phases), _stream()))
    return h, skip


def region_weights(masks_u8, out=None):
    """region masks uint8 [k, 8h, 8w] -> the blend weights of the four UNet levels, fp32 [h/ds * w/ds, k] for ds = 1, 2, 4, 8
    (sdod_region_weights_f32: integer box sums, one division; region 0 where nothing covers a pixel).  out: the four destinations."""
    lib = _lib.hip()
    _req(masks_u8, torch.uint8, 'masks')
    if masks_u8.dim() != 3:
        raise ValueError(f'masks must be [regions, 8h, 8w], got {tuple(masks_u8.shape)}')
    k, ih, iw = masks_u8.shape
    h, w = ih // 8, iw // 8
    if ih != 8 * h or iw != 8 * w:
        raise ValueError(f'mask size {ih} x {iw} is not 8 x a latent size')
    if out is None:
        out = [torch.empty((h // ds) * (w // ds), k, dtype=torch.float32, device=masks_u8.device) for ds in (1, 2, 4, 8)]
    for lvl, o in enumerate(out):
        _req(o, torch.float32, f'out[{lvl}]')
        if o.numel() != (h >> lvl) * (w >> lvl) * k:
            raise ValueError(f'out[{lvl}] holds {o.numel()} floats, the level needs {(h >> lvl) * (w >> lvl) * k}')
    check(lib.sdod_region_weights_f32(_p(masks_u8), k, h, w, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _stream()))
    return out


def ip_weights(scale, h, w, mask_u8=None, out=None, device='cuda:0'):
    """the weights of the text and image-token segments at the four UNet levels, fp32 [h/ds * w/ds, 2] for ds = 1, 2, 4, 8
    (sdod_ip_weights_f32): column 0 is 1, column 1 scale * S / (255 (8 ds)^2) with S the sum of mask_u8 [8h, 8w] over the level
    pixel, or scale everywhere without a mask.  out: the four destinations (UNet.ip_w)."""
    lib = _lib.hip()
    scale = float(scale)
    if not (scale >= 0.0 and scale != float('inf')):
        raise ValueError(f'scale must be finite and >= 0, got {scale}')
    if mask_u8 is not None:
        _req(mask_u8, torch.uint8, 'mask')
        if tuple(mask_u8.shape) != (8 * h, 8 * w):
            raise ValueError(f'mask must be [{8 * h}, {8 * w}], got {tuple(mask_u8.shape)}')
        device = mask_u8.device
    if out is None:
        out = [torch.empty((h // ds) * (w // ds), 2, dtype=torch.float32, device=device) for ds in (1, 2, 4, 8)]
    for lvl, o in enumerate(out):
        _req(o, torch.float32, f'out[{lvl}]')
        if o.numel() != (h >> lvl) * (w >> lvl) * 2:
            raise ValueError(f'out[{lvl}] holds {o.numel()} floats, the level needs {(h >> lvl) * (w >> lvl) * 2}')
    check(lib.sdod_ip_weights_f32(None if mask_u8 is None else _p(mask_u8), scale, h, w, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _stream()))
    return out


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def patch_embed(img_u8, patch, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 [n, S, S, 3] -> fp16 [n * (S / patch)^2, kpad], the rows of a ViT's patch-embedding GEMM (sdod_patch_embed_u8_f16):
    column c p p + dy p + dx = fp16((u / 255 - mean_c) / std_c), zero from 3 p p up to kpad = the next multiple of 64"""
    lib = _lib.hip()
    _req(img_u8, torch.uint8, 'img')
    if img_u8.dim() != 4 or img_u8.shape[1] != img_u8.shape[2] or img_u8.shape[3] != 3:
        raise ValueError(f'img must be [n, S, S, 3], got {tuple(img_u8.shape)}')
    n, s = img_u8.shape[0], img_u8.shape[1]
    kpad = (3 * patch * patch + 63) // 64 * 64
    out = torch.empty(n * (s // patch) ** 2, kpad, dtype=torch.float16, device=img_u8.device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    check(lib.sdod_patch_embed_u8_f16(_p(img_u8), _p(out), n, s, int(patch), kpad, m3, s3, _stream()))
    return out


def vit_tokens(patches, class_embedding, position_embedding, ln_weight, ln_bias, eps=1e-5):
    """patches fp16 [n, P, W] -> fp16 [n, P + 1, W]: LayerNorm of (class token | patches) + positions (sdod_vit_tokens_f16)"""
    lib = _lib.hip()
    for t, dt, nm in ((patches, torch.float16, 'patches'), (class_embedding, torch.float16, 'class_embedding'),
                      (position_embedding, torch.float16, 'position_embedding'), (ln_weight, torch.float32, 'ln_weight'), (ln_bias, torch.float32, 'ln_bias')):
        _req(t, dt, nm)
    n, p, w = patches.shape
    if class_embedding.numel() != w or tuple(position_embedding.shape) != (p + 1, w) or ln_weight.numel() != w or ln_bias.numel() != w:
        raise ValueError('class_embedding [W], position_embedding [P + 1, W], ln_weight and ln_bias [W] must match patches [n, P, W]')
    out = torch.empty(n, p + 1, w, dtype=torch.float16, device=patches.device)
    check(lib.sdod_vit_tokens_f16(_p(patches), _p(class_embedding), _p(position_embedding), _p(ln_weight), _p(ln_bias), _p(out), n, p, w, float(eps), _stream()))
    return out


def region_blend(a, w, out=None):
    """out[m] = fp16(sum_r w[m % rows_per_img, r] * a[r, m]) (sdod_region_blend_f16): a fp16 [k, rows, C], w fp32 [rows_per_img, k];
    acc = w_0 a_0, then acc + w_r a_r, each product and sum rounded in fp32"""
    lib = _lib.hip()
    _req(a, torch.float16, 'a'); _req(w, torch.float32, 'w')
    if a.dim() != 3 or w.dim() != 2 or w.shape[1] != a.shape[0]:
        raise ValueError(f'a must be [k, rows, C] and w [rows_per_img, k], got {tuple(a.shape)} and {tuple(w.shape)}')
    k, rows, c = a.shape
    if out is None:
        out = torch.empty(rows, c, dtype=torch.float16, device=a.device)
    else:
        _req(out, torch.float16, 'out')
        if out.numel() != rows * c:
            raise ValueError(f'out holds {out.numel()} halves, need {rows * c}')
    check(lib.sdod_region_blend_f16(_p(a), rows * c, _p(w), _p(out), rows, w.shape[0], c, k, _stream()))
    return out


def concat_channels(a, b):
    lib = _lib.hip()
    _req(a, torch.float16, 'a'); _req(b, torch.float16, 'b')
    c0, c1 = a.shape[-1], b.shape[-1]
    rows = a.numel() // c0
    out = torch.empty(a.shape[:-1] + (c0 + c1,), dtype=torch.float16, device=a.device)
    check(lib.sdod_concat_channels_f16(_p(a), _p(b), _p(out), rows, c0, c1, _stream()))
    return out


def im2col3x3_small(x, kpad=64, wrap=None):
    """wrap (None = sdod_im2col3x3_small_f16; an int goes through sdod_im2col3x3_small_wrap_f16): circular border, bit 0 = x, bit 1 = y"""
    lib = _lib.hip()
    _req(x, torch.float16, 'x')
    n, h, w, c = x.shape
    out = torch.empty((n * h * w, kpad), dtype=torch.float16, device=x.device)
    if wrap is None:
        check(lib.sdod_im2col3x3_small_f16(_p(x), _p(out), n, h, w, c, kpad, _stream()))
    else:
        check(lib.sdod_im2col3x3_small_wrap_f16(_p(x), _p(out), n, h, w, c, kpad, int(wrap), _stream()))
    return out


def latent_im2col(x, kpad=64, scale=1.0):  # kpad=128: the 9-channel inpainting input (9 * 9 = 81 columns, zero beyond)
    """NCHW fp32 latent -> im2col matrix [n*h*w, kpad] fp16 of a 3x3 pad-1 convolution (the UNet's input conv as a K = 64 GEMM)"""
    lib = _lib.hip()
    _req(x, torch.float32, 'x')
    n, c, h, w = x.shape
    out = torch.empty((n * h * w, kpad), dtype=torch.float16, device=x.device)
    check(lib.sdod_latent_im2col_f16(_p(x), _p(out), n, h, w, c, kpad, scale, _stream()))
    return out


def conv_in(x, w, bias, scale=1.0, wrap=None):
    """the UNet's input convolution in one launch (include/sdod_hip.h: sdod_conv_in_f16): x NCHW fp32 [n, c, h, w], w fp16
    [cout, 64] (k = tap * c + channel, zero beyond 9 c), bias fp32 [cout] -> NHWC fp16 [n, h, w, cout].  wrap (None = that entry point;
    an int goes through sdod_conv_in_wrap_f16): circular border, bit 0 = x, bit 1 = y"""
    lib = _lib.hip()
    _req(x, torch.float32, 'x'); _req(w, torch.float16, 'w'); _req(bias, torch.float32, 'bias')
    n, c, h, wd = x.shape
    cout = w.shape[0]
    assert w.shape[1] == 64
    out = torch.empty((n, h, wd, cout), dtype=torch.float16, device=x.device)
    if wrap is None:
        check(lib.sdod_conv_in_f16(_p(x), _p(w), _p(bias), _p(out), n, h, wd, c, cout, scale, _stream()))
    else:
        check(lib.sdod_conv_in_wrap_f16(_p(x), _p(w), _p(bias), _p(out), n, h, wd, c, cout, scale, int(wrap), _stream()))
    return out


def image_conv_in(img_u8, w, bias):
    """the VAE encoder's input convolution in one launch (sdod_image_conv_in_f16): uint8 HWC RGB [n, h, w, 3] -> 2 u / 255 - 1 ->
    3x3 pad-1 conv with w fp16 [cout, 64] (PK_CONV3_SMALL packing) + bias fp32 [cout] -> NHWC fp16 [n, h, w, cout]"""
    lib = _lib.hip()
    _req(img_u8, torch.uint8, 'img'); _req(w, torch.float16, 'w'); _req(bias, torch.float32, 'bias')
    n, h, wd, c = img_u8.shape
    assert c == 3 and w.shape[1] == 64
    cout = w.shape[0]
    out = torch.empty((n, h, wd, cout), dtype=torch.float16, device=img_u8.device)
    check(lib.sdod_image_conv_in_f16(_p(img_u8), _p(w), _p(bias), _p(out), n, h, wd, cout, _stream()))
    return out


def image_conv_in_unit(img_u8, w, bias, out2=None):
    """RRDBNet's conv_first in one launch (sdod_image_conv_in_unit_f16): image_conv_in on u / 255, zero padding in that space.
    out2: optional fp16 [n, h, w, ld2] buffer (ld2 >= cout, a multiple of 8) whose first cout channels receive a second copy."""
    lib = _lib.hip()
    _req(img_u8, torch.uint8, 'img'); _req(w, torch.float16, 'w'); _req(bias, torch.float32, 'bias')
    n, h, wd, c = img_u8.shape
    assert c == 3 and w.shape[1] == 64
    cout = w.shape[0]
    out = torch.empty((n, h, wd, cout), dtype=torch.float16, device=img_u8.device)
    ld2 = 0
    if out2 is not None:
        _req(out2, torch.float16, 'out2')
        assert tuple(out2.shape[:3]) == (n, h, wd), out2.shape
        ld2 = out2.shape[3]
    check(lib.sdod_image_conv_in_unit_f16(_p(img_u8), _p(w), _p(bias), _p(out), _p(out2), ld2, n, h, wd, cout, _stream()))
    return out


def dense_conv_desc(inp, w, bias, out, *, n, h, wd, cin, cout, ld_in, ld_out, out_col=0, in_off=0, out_off=0, alpha=1.0, slope=0.0,
                    res1=None, res1_off=0, ld_res1=0, c1=0.0, res2=None, res2_off=0, ld_res2=0, upsample=0):
    """a sdod_dense_conv_desc over torch buffers: every operand is (tensor, element offset), so that a test can place an image inside
    a guarded buffer, alias operands or misalign a pointer; nothing is checked here -- the library's checks are what callers rely on"""
    def at(t, off):
        return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())
    return _lib.DenseConvDesc(at(inp, in_off), _p(w), _p(bias), at(out, out_off), at(res1, res1_off), at(res2, res2_off),
                              ld_in, ld_out, ld_res1, ld_res2, out_col, cin, cout, n, h, wd, upsample, alpha, slope, c1)


def dense_conv(inp, w, bias, out, **kw):
    """the ESRGAN dense-block convolution (sdod_dense_conv3x3_f16) on raw buffers; see dense_conv_desc for the arguments"""
    d = dense_conv_desc(inp, w, bias, out, **kw)
    check(_lib.hip().sdod_dense_conv3x3_f16(ctypes.byref(d), _stream()))
    return out


def dense_conv_ok(inp, w, bias, out, **kw):
    """1 when sdod_dense_conv3x3_f16 takes these arguments (host-only query)"""
    d = dense_conv_desc(inp, w, bias, out, **kw)
    return _lib.hip().sdod_dense_conv3x3_ok(ctypes.byref(d))


def conv_in_cat(x, cond, w, bias):
    """the 9-channel inpainting UNet's input convolution in one launch (sdod_conv_in_cat_f16): x NCHW fp32 [n, c, h, w] and cond NCHW
    fp32 [n, c_cond, h, w] read as their channel concatenation, w fp16 [cout, 128] (k = tap * (c + c_cond) + channel, zero from
    9 (c + c_cond); columns 96.. are not read), bias fp32 [cout] -> NHWC fp16 [n, h, w, cout]"""
    lib = _lib.hip()
    _req(x, torch.float32, 'x'); _req(cond, torch.float32, 'cond'); _req(w, torch.float16, 'w'); _req(bias, torch.float32, 'bias')
    n, c, h, wd = x.shape
    assert cond.shape[0] == n and tuple(cond.shape[2:]) == (h, wd) and w.shape[1] == 128, (x.shape, cond.shape, w.shape)
    cout = w.shape[0]
    out = torch.empty((n, h, wd, cout), dtype=torch.float16, device=x.device)
    check(lib.sdod_conv_in_cat_f16(_p(x), _p(cond), _p(w), _p(bias), _p(out), n, h, wd, c, cond.shape[1], cout, _stream()))
    return out


def masked_image_conv_in(img_u8, mask_u8, w, bias):
    """image_conv_in on inpainting's masked image (sdod_masked_image_conv_in_f16): a pixel is 0.0 where mask uint8 [n, h, w] >= 128 and
    2 u / 255 - 1 elsewhere"""
    lib = _lib.hip()
    _req(img_u8, torch.uint8, 'img'); _req(mask_u8, torch.uint8, 'mask'); _req(w, torch.float16, 'w'); _req(bias, torch.float32, 'bias')
    n, h, wd, c = img_u8.shape
    assert c == 3 and w.shape[1] == 64 and tuple(mask_u8.shape) == (n, h, wd)
    cout = w.shape[0]
    out = torch.empty((n, h, wd, cout), dtype=torch.float16, device=img_u8.device)
    check(lib.sdod_masked_image_conv_in_f16(_p(img_u8), _p(mask_u8), _p(w), _p(bias), _p(out), n, h, wd, cout, _stream()))
    return out


def inpaint_cond(moments, mask_u8, seed=0, image_index=0, n1=None, out=None, reps=1, factor=8):
    """the conditioning input of a 9-channel inpainting UNet in one launch (sdod_inpaint_cond_f32): moments fp32 [n, 2c, h, w] of the
    masked image and mask uint8 [n, 8h, 8w] -> fp32 [reps * n, 1 + c, h, w]: channel 0 = (mask[:, ::8, ::8] >= 128), channels 1.. =
    encode_latent's z0.  n1 None: Philox on the device, stream (1 << 32) | (image_index + i).  out: the destination (UNet.cond)."""
    lib = _lib.hip()
    _req(moments, torch.float32, 'moments'); _req(mask_u8, torch.uint8, 'mask')
    n, c2, h, w = moments.shape
    c = c2 // 2
    assert tuple(mask_u8.shape) == (n, factor * h, factor * w), (mask_u8.shape, moments.shape)
    if n1 is not None:
        _req(n1, torch.float32, 'n1')
        assert tuple(n1.shape) == (n, c, h, w), n1.shape
    if out is None:
        out = torch.empty((reps * n, 1 + c, h, w), dtype=torch.float32, device=moments.device)
    else:
        _req(out, torch.float32, 'out')
        assert out.numel() == reps * n * (1 + c) * h * w, (out.shape, reps, n, c, h, w)
    check(lib.sdod_inpaint_cond_f32(_p(moments), _p(mask_u8), _p(n1), _p(out), n, c, h, w, factor, reps, int(seed) & (2 ** 64 - 1),
                                    int(image_index) & (2 ** 64 - 1), _stream()))
    return out


def encode_latent(moments, sqrt_at, sqrt_one_minus_at, seed=0, image_index=0, n1=None, n2=None, z0=None):
    """ldm img2img's start latent from fp32 NCHW moments [n, 2c, h, w] (sdod_encode_latent_f32): posterior sample with n1,
    0.18215 scale, stochastic_encode with n2.  n1 / n2 None: Philox on the device, streams (1 << 32) | (image_index + i) and
    (2 << 32) | (image_index + i).  z0: optional fp32 [n, c, h, w] that receives 0.18215 * sample.  Returns x fp32 [n, c, h, w]."""
    lib = _lib.hip()
    _req(moments, torch.float32, 'moments')
    n, c2, h, w = moments.shape
    c = c2 // 2
    shape = (n, c, h, w)
    for t, name in ((n1, 'n1'), (n2, 'n2'), (z0, 'z0')):
        if t is not None:
            _req(t, torch.float32, name)
            assert tuple(t.shape) == shape, (name, t.shape, shape)
    x = torch.empty(shape, dtype=torch.float32, device=moments.device)
    check(lib.sdod_encode_latent_f32(_p(moments), _p(n1), _p(n2), _p(x), _p(z0), n, c, h * w, float(sqrt_at), float(sqrt_one_minus_at),
                                     int(seed), int(image_index), _stream()))
    return x


RESIZE_MODES = {'nearest-exact': 0, 'bilinear': 1, 'bicubic': 2}


def latent_resize(z, size, mode='bilinear', a=1.0, b=0.0, noise=None, seed=0, image_index=0, out=None):
    """a * R(z) + b * nu in one launch (sdod_latent_resize_f32): z fp32 [n, c, h, w] -> fp32 [n, c, h_out, w_out] with R =
    F.interpolate(size=size, mode=mode, align_corners=False, antialias=False), mode 'nearest-exact', 'bilinear' or 'bicubic'.  nu
    (b != 0 only): `noise` fp32 [n, c, h_out, w_out], or Philox on the device, stream (2 << 32) | (image_index + i) of `seed` for
    image i.  out: an existing fp32 destination that does not overlap z."""
    lib = _lib.hip()
    if mode not in RESIZE_MODES:
        raise ValueError(f'mode must be one of {tuple(RESIZE_MODES)}, got {mode!r}')
    _req(z, torch.float32, 'z')
    if z.dim() != 4:
        raise ValueError(f'z must be [n, c, h, w], got {tuple(z.shape)}')
    n, c, h, w = z.shape
    shape = (n, c, int(size[0]), int(size[1]))
    if noise is not None:
        _req(noise, torch.float32, 'noise')
        if tuple(noise.shape) != shape:
            raise ValueError(f'noise must be {shape}, got {tuple(noise.shape)}')
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=z.device)
    else:
        _req(out, torch.float32, 'out')
        if tuple(out.shape) != shape:
            raise ValueError(f'out must be {shape}, got {tuple(out.shape)}')
    check(lib.sdod_latent_resize_f32(_p(z), _p(out), n, c, h, w, shape[2], shape[3], RESIZE_MODES[mode], float(a), float(b), _p(noise),
                                     int(seed) & (2 ** 64 - 1), int(image_index) & (2 ** 64 - 1), _stream()))
    return out


def latent_resize_taps(mode, n_in, n_out):
    """the per-axis table of latent_resize, computed on the host by the function the kernel uses (sdod_latent_resize_taps): (idx int32
    [n_out, 4], w fp32 [n_out, 4]) as CPU tensors; unused slots hold index 0 and weight 0"""
    lib = _lib.hip()
    idx = torch.zeros((max(int(n_out), 0), 4), dtype=torch.int32)
    w = torch.zeros((max(int(n_out), 0), 4), dtype=torch.float32)
    check(lib.sdod_latent_resize_taps(RESIZE_MODES.get(mode, mode), int(n_in), int(n_out), _p(idx), _p(w)))
    return idx, w


def nchw_f32_to_nhwc_f16(x, scale=1.0):
    lib = _lib.hip()
    _req(x, torch.float32, 'x')
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    out = torch.empty((n,) + tuple(x.shape[2:]) + (c,), dtype=torch.float16, device=x.device)
    check(lib.sdod_nchw_f32_to_nhwc_f16(_p(x), _p(out), n, c, hw, scale, _stream()))
    return out


def nhwc_f16_to_nchw_f32(x):
    lib = _lib.hip()
    _req(x, torch.float16, 'x')
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    out = torch.empty((n, c) + tuple(x.shape[1:-1]), dtype=torch.float32, device=x.device)
    check(lib.sdod_nhwc_f16_to_nchw_f32(_p(x), _p(out), n, c, hw, _stream()))
    return out


def embedding(ids, table, pos):
    lib = _lib.hip()
    _req(ids, torch.int32, 'ids'); _req(table, torch.float16, 'table'); _req(pos, torch.float16, 'pos')
    rows = ids.numel(); seq = pos.shape[0]; c = table.shape[1]
    out = torch.empty(tuple(ids.shape) + (c,), dtype=torch.float16, device=ids.device)
    check(lib.sdod_embedding_f16(_p(ids), _p(table), _p(pos), _p(out), rows, seq, c, _stream()))
    return out


def context_assemble(enc, weights=None, out=None):
    """enc fp16 [P, K, T, D] (the text encoder's output per prompt and 75-token chunk), weights fp32 [P, K, T] or None -> the
    cross-attention context fp16 [P, K*T, D]: token rows scaled by their emphasis, each chunk's mean restored (include/sdod_hip.h:
    sdod_context_assemble_f16).  weights None: a copy."""
    lib = _lib.hip()
    _req(enc, torch.float16, 'enc')
    if enc.dim() != 4:
        raise ValueError(f'enc must be [P, K, T, D], got {tuple(enc.shape)}')
    p, k, t, d = enc.shape
    if weights is not None:
        _req(weights, torch.float32, 'weights')
        if tuple(weights.shape) != (p, k, t):
            raise ValueError(f'weights must be {(p, k, t)}, got {tuple(weights.shape)}')
    if out is None:
        out = torch.empty((p, k * t, d), dtype=torch.float16, device=enc.device)
    else:
        _req(out, torch.float16, 'out')
        if tuple(out.shape) != (p, k * t, d):
            raise ValueError(f'out must be {(p, k * t, d)}, got {tuple(out.shape)}')
    check(lib.sdod_context_assemble_f16(_p(enc), _p(weights), _p(out), p, k, t, d, _stream()))
    return out


def timestep_features(t, dim=320):
    lib = _lib.hip()
    _req(t, torch.float32, 't')
    out = torch.empty((t.numel(), dim), dtype=torch.float16, device=t.device)
    check(lib.sdod_timestep_features_f16(_p(t), _p(out), t.numel(), dim, _stream()))
    return out


def cfg_combine(eps_nhwc, guidance, uncond_first=True, mode=1):
    lib = _lib.hip()
    _req(eps_nhwc, torch.float16, 'eps')
    n2, c = eps_nhwc.shape[0], eps_nhwc.shape[-1]
    n = n2 // 2
    spatial = tuple(eps_nhwc.shape[1:-1])
    hw = eps_nhwc.numel() // (n2 * c)
    out = torch.empty((n, c) + spatial, dtype=torch.float32, device=eps_nhwc.device)
    check(lib.sdod_cfg_combine(_p(eps_nhwc), _p(out), n, c, hw, guidance, 1 if uncond_first else 0, mode, _stream()))
    return out


def _guided_dims(eps_nhwc, x):
    """(n, c, hw) of the fp32 latent x [n, c, ...] behind the fp16 NHWC prediction [2n, ..., c] of its (uncond, cond) batch"""
    _req(eps_nhwc, torch.float16, 'eps'); _req(x, torch.float32, 'x')
    n2, c = eps_nhwc.shape[0], eps_nhwc.shape[-1]
    n = n2 // 2
    hw = eps_nhwc.numel() // (n2 * c)
    assert x.numel() == n * c * hw
    return n, c, hw


def _fill_ddim(a, ddim):
    a.sqrt_one_minus_at, a.sqrt_at, a.sqrt_a_prev, a.dir_coef = ddim['sqrt_one_minus_at'], ddim['sqrt_at'], ddim['sqrt_a_prev'], ddim['dir_coef']


def _fill_v_pred(a, v_coef):
    if v_coef is not None:
        a.v_pred, a.vc0, a.vc1 = 1, v_coef[0], v_coef[1]


def _fill_stage(a, x, stage):
    """stage = (x_dst, temb_row, temb_dst) or None: the next evaluation's inputs, x repeated into x_dst and temb_row into every row of temb_dst"""
    if stage is None:
        return
    x_dst, temb_row, temb_dst = stage
    _req(x_dst, torch.float32, 'x_dst'); _req(temb_row, torch.float16, 'temb_row'); _req(temb_dst, torch.float16, 'temb_dst')
    a.x_stage, a.stage_reps = _p(x_dst), x_dst.numel() // x.numel()
    assert a.stage_reps * x.numel() == x_dst.numel() and temb_dst.numel() % temb_row.numel() == 0
    a.temb_row, a.temb_dst, a.temb_width, a.temb_reps = _p(temb_row), _p(temb_dst), temb_row.numel(), temb_dst.numel() // temb_row.numel()


def plms_update(eps_nhwc, x, old, coefs, div, ddim, guidance, mode=1, v_coef=None, stage=None):
    """one PLMS step in one launch (include/sdod_hip.h: sdod_plms_update): CFG of eps (+ v -> eps with v_coef = (c_e, c_x)),
    e' = (coefs[0] e_t + coefs[1:] . old) / div, DDIM update of x in place with ddim = schedule.coef(index), and -- with
    stage = (x_dst, temb_row, temb_dst) -- the next evaluation's inputs.  Returns e_t (fp32 [n, c, ...])."""
    lib = _lib.hip()
    n, c, hw = _guided_dims(eps_nhwc, x)
    assert len(old) <= 3 and len(coefs) == len(old) + 1
    e_out = torch.empty_like(x)
    a = _lib.PlmsUpdateArgs()
    a.eps_nhwc, a.e_out, a.x = _p(eps_nhwc), _p(e_out), _p(x)
    olds = list(old) + [None] * (3 - len(old)); cs = list(coefs) + [0.0] * (4 - len(coefs))
    for t in old:
        _req(t, torch.float32, 'old')
    a.old1, a.old2, a.old3 = _p(olds[0]), _p(olds[1]), _p(olds[2])
    a.n, a.c, a.hw, a.uncond_first, a.mode = n, c, hw, 1, mode
    a.guidance, a.c0, a.c1, a.c2, a.c3, a.div = guidance, cs[0], cs[1], cs[2], cs[3], div
    _fill_v_pred(a, v_coef)
    _fill_ddim(a, ddim)
    _fill_stage(a, x, stage)
    check(lib.sdod_plms_update(ctypes.byref(a), _stream()))
    return e_out


def dpm_step(eps_nhwc, x, y_prev, coef, guidance, mode=0, uncond_first=True, stage=None):
    """the reference driver's per-step arithmetic in one launch (include/sdod_hip.h: sdod_dpm_step): CFG of eps, the
    DPM-Solver++(2M) update of x / y_prev in place with coef = DpmSolver.coef(step), and -- with stage = (x_dst, temb_row,
    temb_dst) -- the next evaluation's inputs"""
    lib = _lib.hip()
    n, c, hw = _guided_dims(eps_nhwc, x)
    _req(y_prev, torch.float32, 'y_prev')
    assert x.numel() == y_prev.numel()
    a = _lib.DpmStepArgs()
    a.eps_nhwc, a.x, a.y_prev = _p(eps_nhwc), _p(x), _p(y_prev)
    a.n, a.c, a.hw, a.uncond_first, a.mode, a.order = n, c, hw, 1 if uncond_first else 0, mode, coef['order']
    a.guidance = guidance
    a.sigma_s, a.alpha_s, a.sigma_ratio, a.c_prev, a.c_cur = coef['sigma_s'], coef['alpha_s'], coef['sigma_ratio'], coef['c_prev'], coef['c_cur']
    _fill_stage(a, x, stage)
    check(lib.sdod_dpm_step(ctypes.byref(a), _stream()))


def ddim_inpaint_step(eps_nhwc, x, ddim, guidance, z0=None, keep=None, known=None, noise=None, seed=0, noise_level=0, image_index=0,
                      mode=1, v_coef=None, stage=None):
    """one DDIM step in one launch, with inpainting's latent blend (include/sdod_hip.h: sdod_ddim_inpaint_step): CFG of eps (+ v -> eps
    with v_coef = (c_e, c_x)), DDIM update of x in place with ddim = schedule.coef(index), then x = keep * known + (1 - keep) * x'
    with known = sa * z0 + s1a * nu for known = (sa, s1a), or z0 for known = None (the last step: no noise drawn or read), and -- with
    stage = (x_dst, temb_row, temb_dst) -- the next evaluation's inputs.  nu = noise (fp32, x's shape) or, when None, Philox on the
    device: stream ((3 + noise_level) << 32) | (image_index + i) of `seed` for image i.  keep (fp32 [n, H, W]) None: a plain fused
    DDIM step."""
    lib = _lib.hip()
    n, c, hw = _guided_dims(eps_nhwc, x)
    a = _lib.DdimInpaintStepArgs()
    a.eps_nhwc, a.x = _p(eps_nhwc), _p(x)
    if keep is not None:
        _req(keep, torch.float32, 'keep')
        assert keep.numel() == n * hw, (keep.shape, n, hw)
        if z0 is not None:
            _req(z0, torch.float32, 'z0')
            assert z0.numel() == x.numel()
        a.keep, a.z0 = _p(keep), _p(z0)
        if noise is not None:
            _req(noise, torch.float32, 'noise')
            assert noise.numel() == x.numel()
            a.noise = _p(noise)
        if known is None:
            a.last = 1                    # the kernel neither draws nor reads noise, whatever the pointer
        else:
            a.known_sa, a.known_s1a = known
            a.seed, a.noise_level, a.image_index0 = int(seed) & (2 ** 64 - 1), int(noise_level), int(image_index) & (2 ** 64 - 1)
    a.n, a.c, a.hw, a.uncond_first, a.mode = n, c, hw, 1, mode
    a.guidance = guidance
    _fill_v_pred(a, v_coef)
    _fill_ddim(a, ddim)
    _fill_stage(a, x, stage)
    check(lib.sdod_ddim_inpaint_step(ctypes.byref(a), _stream()))


def k_step(eps_nhwc, x, coef, guidance=1.0, den_prev=None, noise=None, seed=0, noise_level=0, image_index=0, mode=1, uncond_first=True,
           stage=None):
    """one k-diffusion sampler step in one launch (include/sdod_hip.h: sdod_k_step): CFG of eps, den = d0 x + d1 e, x <- a x + b den
    (+ cprev den_prev) (+ u nu) in place, den_prev <- den, and -- with stage = (x_dst, temb_row, temb_dst) -- the next evaluation's
    inputs, x_dst = stage_scale * x.  coef = KSchedule.coef(...): d0, d1, a, b, cprev, u, stage_scale (missing keys: d0 = 1, the rest 0).
    nu = noise (fp32, x's shape) or, when None, Philox on the device: stream ((3 + noise_level) << 32) | (image_index + i) of `seed`
    for image i; nothing is drawn or read when u == 0.  eps_nhwc None: the start form, x <- a x and the staging."""
    lib = _lib.hip()
    _req(x, torch.float32, 'x')
    a = _lib.KStepArgs()
    if eps_nhwc is None:
        n, c = x.shape[0], x.shape[1]
        hw = x.numel() // (n * c)
    else:
        n, c, hw = _guided_dims(eps_nhwc, x)
        a.eps_nhwc = _p(eps_nhwc)
    a.x = _p(x)
    for t, name in ((den_prev, 'den_prev'), (noise, 'noise')):
        if t is not None:
            _req(t, torch.float32, name)
            assert t.numel() == x.numel(), (name, t.shape, x.shape)
    a.den_prev, a.noise = _p(den_prev), _p(noise)
    a.seed, a.noise_level, a.image_index0 = int(seed) & (2 ** 64 - 1), int(noise_level), int(image_index) & (2 ** 64 - 1)
    a.n, a.c, a.hw, a.uncond_first, a.mode = n, c, hw, 1 if uncond_first else 0, mode
    a.guidance = guidance
    a.d0, a.d1, a.a, a.b = coef.get('d0', 1.0), coef.get('d1', 0.0), coef.get('a', 0.0), coef.get('b', 0.0)
    a.cprev, a.u, a.stage_scale = coef.get('cprev', 0.0), coef.get('u', 0.0), coef.get('stage_scale', 0.0)
    _fill_stage(a, x, stage)
    check(lib.sdod_k_step(ctypes.byref(a), _stream()))


def lcm_step(eps_nhwc, x, coef, guidance=None, den_out=None, noise=None, seed=0, noise_level=0, image_index=0, mode=1, uncond_first=True,
             stage=None):
    """one Latent Consistency Model step in one launch (include/sdod_hip.h: sdod_lcm_step): e = CFG of the pair eps_nhwc fp16 [2n, ..., c]
    with `guidance` (mode as cfg_combine), or -- guidance None -- the unguided form, e = eps_nhwc fp16 [n, ..., c] itself; den = d0 x + d1 e
    (the x0 prediction, written to den_out when given), x <- a x + b den (+ u nu) in place, and -- with stage = (x_dst, temb_row,
    temb_dst) -- the next evaluation's inputs, x_dst = x unscaled.  coef = LcmSchedule.coef(...): d0, d1, a, b, u.  nu = noise (fp32,
    x's shape) or, when None, Philox on the device: stream ((3 + noise_level) << 32) | (image_index + i) of `seed` for image i; nothing
    is drawn or read when u == 0."""
    lib = _lib.hip()
    _req(eps_nhwc, torch.float16, 'eps'); _req(x, torch.float32, 'x')
    a = _lib.LcmStepArgs()
    if guidance is None:
        n, c = eps_nhwc.shape[0], eps_nhwc.shape[-1]
        hw = eps_nhwc.numel() // (n * c)
        assert x.numel() == n * c * hw, (eps_nhwc.shape, x.shape)
    else:
        n, c, hw = _guided_dims(eps_nhwc, x)
        a.guided, a.guidance = 1, guidance
    a.eps_nhwc, a.x = _p(eps_nhwc), _p(x)
    for t, name in ((den_out, 'den_out'), (noise, 'noise')):
        if t is not None:
            _req(t, torch.float32, name)
            assert t.numel() == x.numel(), (name, t.shape, x.shape)
    a.den_out, a.noise = _p(den_out), _p(noise)
    a.seed, a.noise_level, a.image_index0 = int(seed) & (2 ** 64 - 1), int(noise_level), int(image_index) & (2 ** 64 - 1)
    a.n, a.c, a.hw, a.uncond_first, a.mode = n, c, hw, 1 if uncond_first else 0, mode
    a.d0, a.d1, a.a, a.b, a.u = coef['d0'], coef['d1'], coef['a'], coef['b'], coef['u']
    _fill_stage(a, x, stage)
    check(lib.sdod_lcm_step(ctypes.byref(a), _stream()))


def guidance_features(w, dim=256):
    """w fp32 [n] -> fp16 [n, dim]: the guidance-scale embedding of a full LCM checkpoint (include/sdod_hip.h: sdod_guidance_features_f16)"""
    lib = _lib.hip()
    _req(w, torch.float32, 'w')
    out = torch.empty((w.numel(), dim), dtype=torch.float16, device=w.device)
    check(lib.sdod_guidance_features_f16(_p(w), _p(out), w.numel(), dim, _stream()))
    return out


def k_step_windows(eps, x, coef, wgt, wsum, window_hw, oy, ox, n, chunks=1, wrap_x=False, guidance=1.0, den_prev=None, noise=None, seed=0,
                   noise_level=0, image_index=0, mode=1, stage=None):
    """k_step on a MultiDiffusion canvas in one launch (include/sdod_hip.h: sdod_k_step_windows).  x fp32 [1, c, H, W] (or [c, H, W]): the
    canvas, updated in place; eps fp16 [chunks, 2n, wh, ww, c] (one chunk: [2n, wh, ww, c], the UNet's own output): the predictions of
    the len(oy) * len(ox) windows of window_hw = (wh, ww) at origins oy x ox, window w = iy * len(ox) + ix in chunk w // n, rows w % n
    and n + w % n; wgt fp32 [wh, ww] and wsum fp32 [H, W] from sdod.amd.panorama (window_weights, weight_sum).  e = sum_w wgt CFG_w /
    wsum over the covering windows in ascending w, then k_step's update with coef = KSchedule.coef(...), den_prev and noise (canvas
    shaped; None: Philox stream ((3 + noise_level) << 32) | image_index of `seed`).  stage = (x_dst, temb_row, temb_dst): x_dst fp32
    [chunks, 2n, c, wh, ww] receives stage_scale * x' in both rows of every window, rows of no window keep their bytes.  eps None: the
    start form, x <- a x and the staging."""
    lib = _lib.hip()
    _req(x, torch.float32, 'x'); _req(wgt, torch.float32, 'wgt'); _req(wsum, torch.float32, 'wsum')
    c, H, W = (int(v) for v in x.shape[-3:])
    wh, ww = (int(v) for v in window_hw)
    assert x.numel() == c * H * W and wgt.numel() == wh * ww and wsum.numel() == H * W, (x.shape, wgt.shape, wsum.shape)
    a = _lib.KStepWindowsArgs()
    per_chunk = 2 * int(n) * c * wh * ww
    if eps is not None:
        _req(eps, torch.float16, 'eps')
        assert eps.numel() == int(chunks) * per_chunk, (eps.shape, chunks, n, c, wh, ww)
        a.eps = _p(eps)
    a.x, a.wgt, a.wsum = _p(x), _p(wgt), _p(wsum)
    for t, name in ((den_prev, 'den_prev'), (noise, 'noise')):
        if t is not None:
            _req(t, torch.float32, name)
            assert t.numel() == x.numel(), (name, t.shape, x.shape)
    a.den_prev, a.noise = _p(den_prev), _p(noise)
    a.seed, a.noise_level, a.image_index0 = int(seed) & (2 ** 64 - 1), int(noise_level), int(image_index) & (2 ** 64 - 1)
    a.c, a.H, a.W, a.wh, a.ww, a.n, a.chunks, a.mode, a.wrap_x = c, H, W, wh, ww, int(n), int(chunks), mode, 1 if wrap_x else 0
    a.ny, a.nx = len(oy), len(ox)                 # (the library refuses a count above the tables' size; the tables take what fits)
    for dst, src in ((a.oy, oy), (a.ox, ox)):
        for i, v in enumerate(list(src)[:_lib.PANO_MAX_AXIS]):
            dst[i] = int(v)
    a.guidance = guidance
    a.d0, a.d1, a.a, a.b = coef.get('d0', 1.0), coef.get('d1', 0.0), coef.get('a', 0.0), coef.get('b', 0.0)
    a.cprev, a.u, a.stage_scale = coef.get('cprev', 0.0), coef.get('u', 0.0), coef.get('stage_scale', 0.0)
    if stage is not None:
        x_dst, temb_row, temb_dst = stage
        _req(x_dst, torch.float32, 'x_dst'); _req(temb_row, torch.float16, 'temb_row'); _req(temb_dst, torch.float16, 'temb_dst')
        assert x_dst.numel() == int(chunks) * per_chunk and temb_dst.numel() % temb_row.numel() == 0, (x_dst.shape, chunks, n)
        a.x_stage = _p(x_dst)
        a.temb_row, a.temb_dst, a.temb_width, a.temb_reps = _p(temb_row), _p(temb_dst), temb_row.numel(), temb_dst.numel() // temb_row.numel()
    check(lib.sdod_k_step_windows(ctypes.byref(a), _stream()))


def mask_to_latent(mask_u8, factor=8):
    """inpainting's latent keep-mask (sdod_mask_to_latent_f32): uint8 [n, 8H, 8W] (255 = repaint, 0 = keep) -> fp32 [n, H, W],
    keep = (16320 - sum of the 8 x 8 block) / 16320"""
    lib = _lib.hip()
    _req(mask_u8, torch.uint8, 'mask')
    n, h, w = mask_u8.shape
    assert h % factor == 0 and w % factor == 0, (h, w, factor)
    out = torch.empty((n, h // factor, w // factor), dtype=torch.float32, device=mask_u8.device)
    check(lib.sdod_mask_to_latent_f32(_p(mask_u8), _p(out), n, h // factor, w // factor, factor, _stream()))
    return out


def image_composite(img_nhwc, init_u8, mask_u8, a=0.5, b=0.5, mode=1):
    """inpainting's pixel composite (sdod_image_composite_u8): img fp16 [n, h, w, 3], init uint8 [n, h, w, 3], mask uint8 [n, h, w] ->
    uint8 (d k + u (255 - k) + 127) / 255 with d = image_to_u8(img, a, b, mode)"""
    lib = _lib.hip()
    _req(img_nhwc, torch.float16, 'img'); _req(init_u8, torch.uint8, 'init'); _req(mask_u8, torch.uint8, 'mask')
    assert img_nhwc.shape[-1] == 3 and init_u8.numel() == img_nhwc.numel() and mask_u8.numel() * 3 == img_nhwc.numel()
    n = img_nhwc.shape[0]
    out = torch.empty(img_nhwc.shape, dtype=torch.uint8, device=img_nhwc.device)
    check(lib.sdod_image_composite_u8(_p(img_nhwc), _p(init_u8), _p(mask_u8), _p(out), n, mask_u8.numel() // n, a, b, mode, _stream()))
    return out


def stage_unet_inputs(x, x_dst, temb_row, temb_dst):
    """x fp32 [n,...] -> x_dst [reps*n,...] (repeated back to back); temb_row fp16 [w] -> every row of temb_dst [b, w]"""
    lib = _lib.hip()
    _req(x, torch.float32, 'x'); _req(x_dst, torch.float32, 'x_dst'); _req(temb_row, torch.float16, 'temb_row'); _req(temb_dst, torch.float16, 'temb_dst')
    reps = x_dst.numel() // x.numel()
    assert reps * x.numel() == x_dst.numel() and temb_dst.numel() % temb_row.numel() == 0
    check(lib.sdod_stage_unet_inputs(_p(x), _p(x_dst), x.numel(), reps, _p(temb_row), _p(temb_dst), temb_row.numel(),
                                     temb_dst.numel() // temb_row.numel(), _stream()))


def randn(shape, seed, stream_id, device, return_words=False, out=None):
    """N(0,1) fp32 tensor from the in-tree Philox4x32-10 generator: a pure function of (seed, stream_id, element index).
    out: an existing contiguous fp32 tensor of `shape` to fill (a row of a graph's static noise input) instead of a new one"""
    lib = _lib.hip()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    else:
        _req(out, torch.float32, 'out')
        assert tuple(out.shape) == tuple(shape), (out.shape, shape)
    words = torch.empty(out.numel(), dtype=torch.int32, device=device) if return_words else None
    with torch.cuda.device(out.device):
        check(lib.sdod_randn_f32(_p(out), _p(words), out.numel(), int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), _stream()))
    return (out, words) if return_words else out


def dpm_update(x, eps, y_prev, order, sigma_s, alpha_s, sigma_ratio, c_prev, c_cur):
    lib = _lib.hip()
    for t in (x, eps, y_prev):
        _req(t, torch.float32)
    check(lib.sdod_dpm_update(_p(x), _p(eps), _p(y_prev), x.numel(), order, sigma_s, alpha_s, sigma_ratio, c_prev, c_cur,
                              _stream()))


def ddim_step(x, e, sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef):
    lib = _lib.hip()
    _req(x, torch.float32); _req(e, torch.float32)
    check(lib.sdod_ddim_step_f32(_p(x), _p(e), x.numel(), sqrt_one_minus_at, sqrt_at, sqrt_a_prev, dir_coef, _stream()))


def lincomb4(es, coefs, div):
    lib = _lib.hip()
    es = list(es) + [None] * (4 - len(es)); coefs = list(coefs) + [0.0] * (4 - len(coefs))
    out = torch.empty_like(es[0])
    check(lib.sdod_lincomb4_f32(_p(out), _p(es[0]), _p(es[1]), _p(es[2]), _p(es[3]), coefs[0], coefs[1], coefs[2], coefs[3],
                                div, out.numel(), _stream()))
    return out


def image_to_u8(img_nhwc, a=0.5, b=0.5, mode=1):
    lib = _lib.hip()
    _req(img_nhwc, torch.float16, 'img')
    out = torch.empty(img_nhwc.shape, dtype=torch.uint8, device=img_nhwc.device)
    check(lib.sdod_image_to_u8(_p(img_nhwc), _p(out), img_nhwc.numel(), a, b, mode, _stream()))
    return out


def device_info():
    lib = _lib.hip()
    cu = ctypes.c_int(); mem = ctypes.c_size_t(); arch = ctypes.create_string_buffer(64)
    check(lib.sdod_hip_device_info(ctypes.byref(cu), ctypes.byref(mem), arch, 64))
    return {'cu_count': cu.value, 'hbm_bytes': mem.value, 'arch': arch.value.decode()}
