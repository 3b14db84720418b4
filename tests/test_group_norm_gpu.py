"""Every GroupNorm kernel path against float64 at its edges.

Reference: F.group_norm (and SiLU) in float64 on the CPU, on the same dtype-rounded inputs.  Tolerances are those of the
kernel suite's check(): rel-L2 <= 2e-3 (fp16), 2e-5 (fp32), 1e-2 (bf16), and max-abs <= 2e-2 * max|ref| + 1e-3.
Each NHWC case asserts the path it means to hit (sdod_group_norm_path); each NCHW case names the kernel form that
gn_nchw_launch_v picks for its slab length L = (C / G) * spatial: one launch with KMAX = ceil(L / (512 * W)) steps per
thread (W = 8 for whole, aligned vectors, 1 otherwise) up to 32 Ki elements, statistics + apply above."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 2e-3, torch.float32: 2e-5, torch.bfloat16: 1e-2}
DT = {torch.float16: 0, torch.float32: 1}


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def check(out, ref, tol, name, mask=None):
    """rel-L2 <= tol and max-abs <= 2e-2 * max|ref| + 1e-3 (tol None: the max-abs bound alone)"""
    out = out.detach().cpu().double(); ref = ref.detach().cpu().double()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    if mask is not None:
        out, ref = out[mask], ref[mask]
    assert torch.isfinite(out).all(), f'{name}: non-finite output'
    r = float((out - ref).norm() / (ref.norm() + 1e-30))
    mx = float((out - ref).abs().max()); scale = float(ref.abs().max())
    assert tol is None or r <= tol, f'{name}: rel-L2 {r:.3e} > {tol} (max abs {mx:.3e}, ref max {scale:.3e})'
    assert mx <= 2e-2 * scale + 1e-3, f'{name}: max abs {mx:.3e} vs ref max {scale:.3e}'


def ref_gn(x, groups, w, b, eps, silu, channels_last_dim=False):
    """float64 GroupNorm of x ([N, C, *], or [N, HW, C] with channels_last_dim)"""
    xd = x.detach().cpu().double()
    if channels_last_dim:
        xd = xd.permute(0, 2, 1)
    y = F.group_norm(xd, groups, None if w is None else w.cpu().double(), None if b is None else b.cpu().double(), eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1) if channels_last_dim else y


def make(kind, shape, dtype, gen, value=1000.0):
    """inputs of one edge case; `kind` in normal / pilot / control / nearconst / const / offset"""
    if kind == 'nearconst':
        return (3.0 + 1e-2 * torch.randn(shape, generator=gen)).to(dtype)
    if kind == 'const':
        return torch.full(shape, 3.0).to(dtype)
    if kind == 'offset':   # fp32 only.  (At 1000 the fp32 spacing, 6.1e-5, bounds the error of ANY fp32 mean: an exactly rounded
        # one already gives rel-L2 ~1.8e-5 of unit-variance outputs, at the 2e-5 tolerance; 100 keeps that bound 8x below it.)
        return (100.0 + torch.randn(shape, generator=gen)).to(dtype)
    return torch.randn(shape, generator=gen).to(dtype)


def affine(c, gen):
    return 1 + 0.2 * torch.randn(c, generator=gen), 0.3 * torch.randn(c, generator=gen)


# ------------------------------------------------------------------------------------------------------------ NHWC kernels
NHWC_CASES = [  # n, hw, c, groups, dtype, path
    (1, 16384, 512, 32, torch.float16, 0),    # grid-barrier kernel, KMAX 8, slab 256 Ki
    (1, 65536, 256, 32, torch.float16, 0),    # grid-barrier kernel, KMAX 16, slab 512 Ki (the VAE's 256^2 x 256 level)
    (2, 1024, 640, 32, torch.float16, 1),     # (image, group) kernel
    (1, 16, 4112, 2, torch.float16, 2),       # 2056 channels per group: too wide for the (image, group) kernel
    (1, 16384, 64, 4, torch.float16, 3),      # too many pixels per thread for the (image, group) kernel, < 5 MB
    (2, 256, 320, 32, torch.float32, 2),
    (1, 16384, 512, 32, torch.float32, 3),
    (1, 65536, 128, 32, torch.float32, 3),    # > 128 statistics chunks: the collapse launch, slab 256 Ki
    # fewer than 8 channels per group (model_channels 64 / 128 / 192, tests/test_engine_widths_gpu.py): a 16-byte piece of a pixel
    # row covers several groups, so the (image, group) kernel works on 2- or 4-channel vectors
    (2, 1024, 64, 32, torch.float16, 1),      # 2 channels per group: one 2-vector per pixel, 1024 threads
    (2, 1024, 128, 32, torch.float16, 1),     # 4 channels per group: one 4-vector per pixel
    (2, 256, 192, 32, torch.float16, 1),      # 6 channels per group: three 2-vectors per pixel, 341 pixels per pass
    (2, 16, 192, 32, torch.float16, 1),       # ... and on the 4x4 map: the 256-thread form
]


def _nhwc_pilots(x, groups, value, first=True):
    """the value at the first element of every (image, group) slab of x [N, HW, C] (first=False: in the slab's middle);
    returns the mask of the elements set"""
    n, hw, c = x.shape
    cg = c // groups
    mask = torch.zeros(x.shape, dtype=torch.bool)
    for g in range(groups):
        if first:
            mask[:, 0, g * cg] = True
        else:
            mask[:, hw // 2 + 3, g * cg + cg - 1] = True
    x[mask] = value
    return mask


@pytest.mark.parametrize('n,hw,c,groups,dtype,path,kind', [case + (kind,) for case in NHWC_CASES
                                                            for kind in ('pilot', 'control', 'nearconst', 'const', 'offset')
                                                            if kind != 'offset' or case[4] == torch.float32])
def test_group_norm_nhwc_edges(n, hw, c, groups, dtype, path, kind):
    from sdod.amd import ops, _lib
    assert _lib.hip().sdod_group_norm_path(n, hw, c, 0, groups, DT[dtype]) == path
    gen = torch.Generator().manual_seed(hw + c + groups)
    x = make(kind, (n, hw, c), dtype, gen)
    mask = None
    if kind in ('pilot', 'control'):
        value = 4000.0 if hw * c // groups >= 512 * 1024 else 1000.0
        mask = _nhwc_pilots(x, groups, value, first=kind == 'pilot')
    w, b = affine(c, gen)
    silu = kind != 'const'
    ref = ref_gn(x, groups, w, b, 1e-5, silu, channels_last_dim=True)
    d = dev()
    out = ops.group_norm_nhwc(x.to(d), groups, w.to(d), b.to(d), 1e-5, silu)
    name = f'nhwc path {path} {kind} {n}x{hw}x{c}/{groups} {dtype}'
    if kind == 'const':     # zero variance: the bias, within max-abs (the NHWC kernels apply x * scale + shift, and at
        # rstd = eps^-1/2 that form leaves ~1e-4 of rounding: above the fp32 rel-L2 bound, far inside max-abs)
        check(out, b.double().expand(n, hw, c), None, name + ' == bias')
        return
    check(out, ref, TOL[dtype], name)
    if mask is not None:    # the outlier must not skew the normalisation of every other element
        check(out, ref, TOL[dtype], name + ' (outliers excluded)', mask=~mask)


# ------------------------------------------------------------------------------------------------------------ NCHW kernels
NCHW_CASES = [  # shape, groups, form (what gn_nchw_launch_v runs for it)
    ((2, 64, 16, 16), 8, 'one vec KMAX 1'),          # L = 2,048
    ((2, 64, 32, 32), 8, 'one vec KMAX 2'),          # L = 8,192
    ((2, 128, 32, 32), 8, 'one vec KMAX 4'),         # L = 16,384
    ((1, 320, 32, 32), 10, 'one vec KMAX 8'),        # L = 32,768
    ((2, 45, 17, 19), 3, 'one scalar KMAX 16'),      # L = 4,845
    ((1, 30, 31, 23), 2, 'one scalar KMAX 32'),      # L = 10,695
    ((1, 50, 31, 37), 2, 'one scalar KMAX 64'),      # L = 28,675
    ((2, 320, 64, 64), 32, 'stats+apply vec'),       # L = 40,960, 2 chunks per slab
    ((1, 6, 211, 213), 2, 'stats+apply scalar'),     # L = 134,829, 8 chunks per slab
]
NCHW_DTYPES = [torch.float16, torch.float32, torch.bfloat16]


def _nchw_pilots(x, groups, value, first=True):
    n, c = x.shape[:2]
    cg = c // groups
    flat = x.view(n, groups, -1)
    mask = torch.zeros(flat.shape, dtype=torch.bool)
    if first:
        mask[:, :, 0] = True
    else:
        mask[:, :, flat.shape[2] // 2 + 5] = True
    flat[mask] = value
    return mask.view(x.shape)


@pytest.mark.parametrize('shape,groups,form', NCHW_CASES)
@pytest.mark.parametrize('dtype', NCHW_DTYPES)
def test_group_norm_nchw_edges_and_in_place(shape, groups, form, dtype):
    """outlier at every slab's first element (and, as a control, in its middle), near-constant and constant slabs, an fp32
    offset, and y is x bitwise equal to the out-of-place result, on every NCHW kernel form and dtype"""
    from sdod.amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(sum(shape) + groups)
    c = shape[1]
    w, b = affine(c, gen)
    kinds = ['pilot', 'control', 'nearconst', 'const'] + (['offset'] if dtype == torch.float32 else [])
    for kind in kinds:
        x = make(kind, shape, dtype, gen)
        mask = _nchw_pilots(x, groups, 1000.0, first=kind == 'pilot') if kind in ('pilot', 'control') else None
        silu = kind in ('pilot', 'nearconst')
        ref = ref_gn(x, groups, w, b, 1e-5, silu)
        xd = x.to(d)
        out = ops.group_norm_nchw(xd, groups, w.to(d), b.to(d), 1e-5, silu)
        name = f'nchw {form} {kind} {shape}/{groups} {dtype}'
        check(out, ref, TOL[dtype], name)
        if mask is not None:
            check(out, ref, TOL[dtype], name + ' (outliers excluded)', mask=~mask)
        if kind == 'const':
            check(out, b.double().view(1, c, 1, 1).expand(shape), TOL[dtype], name + ' == bias')
        if kind == 'pilot':   # in place: every workgroup of a slab must still see the slab as it was
            y = ops.group_norm_nchw(xd, groups, w.to(d), b.to(d), 1e-5, silu, out=xd)
            torch.cuda.synchronize()
            assert y.data_ptr() == xd.data_ptr()
            assert torch.equal(xd, out), f'{name}: in place differs from out of place'


@pytest.mark.parametrize('dtype', NCHW_DTYPES)
def test_group_norm_nchw_big_slab_outlier(dtype):
    """slabs of 512 Ki elements (statistics + apply) with 4000 at each slab's first element"""
    from sdod.amd import ops
    d = dev()
    shape, groups = (1, 256, 256, 256), 32
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(shape, generator=gen).to(dtype)
    mask = _nchw_pilots(x, groups, 4000.0)
    w, b = affine(256, gen)
    ref = ref_gn(x, groups, w, b, 1e-5, False)
    xd = x.to(d)
    out = ops.group_norm_nchw(xd, groups, w.to(d), b.to(d), 1e-5, False)
    check(out, ref, TOL[dtype], f'nchw 512 Ki slabs {dtype}')
    check(out, ref, TOL[dtype], f'nchw 512 Ki slabs {dtype} (outliers excluded)', mask=~mask)
    ops.group_norm_nchw(xd, groups, w.to(d), b.to(d), 1e-5, False, out=xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, out), 'in place differs from out of place'


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_group_norm_nchw_misaligned_view_takes_the_scalar_path(dtype):
    """storage_offset 1: L % 8 == 0, but the slabs are not 16-byte aligned, so the scalar form must run (one launch and the
    statistics + apply pair)"""
    from sdod.amd import ops
    d = dev()
    for shape, groups in (((2, 64, 32, 32), 8), ((2, 320, 64, 64), 32)):
        gen = torch.Generator().manual_seed(5)
        x = torch.randn(shape, generator=gen).to(dtype)
        _nchw_pilots(x, groups, 1000.0)
        w, b = affine(shape[1], gen)
        ref = ref_gn(x, groups, w, b, 1e-5, True)
        n = x.numel()
        buf = torch.empty(n + 1, dtype=dtype, device=d)
        xd = buf[1:].view(shape)
        xd.copy_(x.to(d))
        assert xd.storage_offset() == 1 and xd.is_contiguous()
        out = ops.group_norm_nchw(xd, groups, w.to(d), b.to(d), 1e-5, True)
        check(out, ref, TOL[dtype], f'misaligned {shape} {dtype}')
        ops.group_norm_nchw(xd, groups, w.to(d), b.to(d), 1e-5, True, out=xd)     # in place, misaligned
        torch.cuda.synchronize()
        assert torch.equal(xd, out)


def test_group_norm_nchw_more_than_65535_slabs():
    """n * groups = 65,540 slabs of 32,776 elements (the statistics + apply pair): slabs must not sit on grid.y"""
    from sdod.amd import ops
    d = dev()
    n, c, s = 1, 65540, 32776
    torch.manual_seed(11)
    x = torch.randn((n, c, s), dtype=torch.float16, device=d)
    w = (1 + 0.2 * torch.randn(c, device=d)); b = 0.3 * torch.randn(c, device=d)
    try:
        out = ops.group_norm_nchw(x, c, w, b, 1e-5, False)
        torch.cuda.synchronize()
        for g in [0, 1, 4097, 65535, 65536] + list(range(c - 5, c)):
            xs = x[:, g:g + 1].cpu()
            ref = ref_gn(xs, 1, w[g:g + 1], b[g:g + 1], 1e-5, False)
            check(out[:, g:g + 1], ref, TOL[torch.float16], f'slab {g}')
    finally:
        del x
        out = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ wide / odd channel counts, both layouts
WIDE = [  # n, hw, c, groups, dtype: the shapes the NHWC path 3 once reported but refused, and very wide maps
    (2, 16, 4104, 8, torch.float32), (1, 64, 2056, 8, torch.float16), (1, 64, 2056, 8, torch.float32),
    (1, 64, 8192, 2, torch.float16), (1, 2048, 4088, 8, torch.float32),
    (1, 64, 8192, 2, torch.float32), (1, 64, 8192, 32, torch.float16),
]


@pytest.mark.parametrize('n,hw,c,groups,dtype', WIDE)
def test_efficient_gn_wide_channels_both_layouts(n, hw, c, groups, dtype):
    import sdod
    d = dev()
    h = 8 if hw >= 64 else 4
    shape = (n, c, h, hw // h)
    gen = torch.Generator().manual_seed(c + groups)
    x = torch.randn(shape, generator=gen).to(dtype)
    _nchw_pilots(x, groups, 1000.0)
    m = sdod.EfficientGN(groups, c, impl='eff').to(d).to(dtype)
    w, b = affine(c, gen)
    with torch.no_grad():
        m.weight.copy_(w); m.bias.copy_(b)
        ref = ref_gn(x, groups, m.weight.float(), m.bias.float(), 1e-5, False)
        y0 = m(x.to(d))
        y1 = m(x.to(d).contiguous(memory_format=torch.channels_last))
    assert y0.is_contiguous() and y1.is_contiguous(memory_format=torch.channels_last)
    check(y0, ref, TOL[dtype], f'EfficientGN {shape}/{groups} {dtype} nchw')
    check(y1, ref, TOL[dtype], f'EfficientGN {shape}/{groups} {dtype} channels_last')


# ------------------------------------------------------------------------------------------------------------ partial affine
@pytest.mark.parametrize('which', ['weight', 'bias'])
def test_group_norm_partial_affine(which):
    """weight without bias / bias without weight: every wrapper equals F.group_norm with the same arguments"""
    from sdod.efficient_gn import efficient_group_norm
    from sdod.amd import ops
    d = dev()
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(2, 64, 16, 16, generator=gen) * 2 + 1).half()
    w, b = affine(64, gen)
    w = w if which == 'weight' else None
    b = b if which == 'bias' else None
    ref = ref_gn(x, 8, w, b, 1e-5, False)
    wd = None if w is None else w.to(d)
    bd = None if b is None else b.to(d)
    xd = x.to(d)
    check(efficient_group_norm(xd, 8, wd, bd, 1e-5), ref, 2e-3, f'efficient_group_norm {which} only')
    check(ops.group_norm_nchw(xd, 8, wd, bd, 1e-5), ref, 2e-3, f'group_norm_nchw {which} only')
    check(ops.group_norm_nchw(xd.contiguous(memory_format=torch.channels_last), 8, wd, bd, 1e-5), ref, 2e-3,
          f'group_norm_nchw channels_last {which} only')
    xh = xd.permute(0, 2, 3, 1).reshape(2, 256, 64).contiguous()
    out = ops.group_norm_nhwc(xh, 8, wd, bd, 1e-5)
    check(out.reshape(2, 16, 16, 64).permute(0, 3, 1, 2), ref, 2e-3, f'group_norm_nhwc {which} only')
