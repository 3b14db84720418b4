"""Shared pieces of the GEMM kernel tests (test_gemm_layouts_gpu.py, test_kernels_gpu.py): a launch that asks the plan which
tile really ran, operands framed inside larger allocations, and inputs whose product is exact in fp16.

run_gemm     launches through ops.gemm(..., return_desc=True), asks sdod_gemm_plan what the descriptor ran on and asserts it:
             the requested tile, or `runs_on=` where make_plan documents a substitute (so that a changed fallback is a visible
             test change).  Every launch is recorded in LEDGER[(tile that ran, family, uint8 weights?)] with the caller's tag.

Frames       A matrix [rows][width] sits in an allocation [rows + 2][ld] at column `col`: one guard row above, one below, and
             ld - width guard columns in every row.  ld and col are multiples of 8 elements (16 for uint8 codes), so every base
             pointer is 16-byte aligned as the launcher demands and as the engine's column offsets are.  Outputs and residuals
             carry the finite fp16 bit pattern SENTINEL in the frame (frame_intact: bit-unchanged after the launch; the interior
             of an output starts as NaN, so an element nobody wrote is seen too); a / w carry NaN there, so a K loop that
             strays past K, or a row loop past M, makes the output non-finite.  uint8 codes cannot hold NaN: their frame is
             the code 255, and the NaN frame of `a` next to it does the detecting.

Exact data   Every product, every partial sum in any order (split-K slabs included) and the result are integers (or integers
             times a power-of-two alpha) of magnitude <= 2048, which fp16, and fp32 a fortiori, hold exactly: the kernel's
             output must then EQUAL the fp64 reference (torch.equal), and a single wrong, missing or doubled term shows.
             fp16 weights (exact_f16): a and w ternary in {-1, 0, 1}, K <= 1600, so |a . w| <= 1600; bias, row bias and
             residual integers in [-8, 8]; |result| <= 1624.  alpha in {1, 2^-k}: alpha * sum is a multiple of 2^-k below 2^11.
             uint8 weights (exact_u8): codes over the whole 0..255, integer offsets in [-128, 0] (w_off = offset + 128),
             scale 1, and at most eight entries of +-1 per row of a: |sum| <= 8 * 255 = 2040.
             assert_exact() checks the bound and the fp16 round trip on the fp64 reference before a test launches anything;
             tests/test_gemm_cases_cpu.py checks both recipes without a GPU (fp32 sums in several orders, slab-wise too)."""
import ctypes
import os

import torch

SENTINEL = 0x3A5D          # fp16 bits of 0.7955: finite, and no integer (exact data never produces it)
LEDGER = {}                # (tile that ran, family, uint8?) -> set of tags
UNTUNED = (4, 15, 16)      # rows of gemm.hip's tile table with tuned = false (sdod_gemm_tile_info does not report the flag: the one copy)
TUNE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'stable-diffusion-on-device_amd', 'tune', 'gfx950.tune')


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _lib():
    from sdod.amd import _lib as L
    return L.hip()


def tile_info(tile):
    """{bm, bn, wm, wn, stages, family ('reg' | 'ring' | 'halo' | 'panel'), spec, ksub} of a tile id (host-only call)"""
    info = (ctypes.c_int * 7)()
    assert _lib().sdod_gemm_tile_info(tile, info) == 0, tile
    bm, bn, wm, wn, stages, spec, ksub = list(info)
    family = 'halo' if spec == 2 else 'panel' if spec == 3 else 'reg' if stages == 0 else 'ring'
    return dict(bm=bm, bn=bn, wm=wm, wn=wn, stages=stages, family=family, spec=spec if family == 'ring' else 0, ksub=ksub)


def num_tiles():
    return _lib().sdod_gemm_num_tiles()


def plan_of(desc):
    t, s = ctypes.c_int(), ctypes.c_int()
    assert _lib().sdod_gemm_plan(ctypes.byref(desc), ctypes.byref(t), ctypes.byref(s)) == 0
    return t.value, s.value


def rows_desc(m, n, k, tile=0, split=1, **fields):
    """a rows-mode descriptor with fake (never dereferenced) pointers, for the host-only planning calls"""
    from sdod.amd._lib import GemmDesc
    d = GemmDesc()
    d.a = d.w = d.out = 0x1000
    d.M, d.N, d.K, d.lda, d.ldw, d.ldo = m, n, k, k, k, n
    d.tile, d.split_k = tile, split
    for f, v in fields.items():
        setattr(d, f, v)
    return d


def u8_tile(tile):
    """the tile a uint8-weight GEMM planned on `tile` runs on (tiles without a uint8 form fall back)"""
    return plan_of(rows_desc(256, 256, 256, tile, wq=1))[0]


def panel_ok(desc, tile):
    return _lib().sdod_gemm_panel_ok(ctypes.byref(desc), tile) == 1


def run_gemm(a, w, bias=None, *, tile, runs_on=None, tag='', want_desc=False, **kw):
    """(out, tile that ran, splits[, descriptor]); asserts that the plan ran `tile` (or `runs_on`, a documented substitute)"""
    from sdod.amd import ops
    out, desc = ops.gemm(a, w, bias, tile=tile, return_desc=True, **kw)
    ran, splits = plan_of(desc)
    want = tile if runs_on is None else runs_on
    assert ran == want, f'{tag}: asked for tile {tile}, expected tile {want} to run, the plan ran tile {ran}'
    LEDGER.setdefault((ran, tile_info(ran)['family'], bool(desc.wq)), set()).add(tag)
    return (out, ran, splits, desc) if want_desc else (out, ran, splits)


def table_picks():
    """[(fields of the key as a dict, tile, split)] of the shipped tune table (one line: the 14 integers of the engine's shape
    key, then tile + 1000 * split_k)"""
    picks = []
    with open(TUNE_FILE) as f:
        for line in f:
            v = [int(x) for x in line.split()]
            if len(v) != 15:
                continue
            am, m, n, k, c0, c1, stride, ups, ks, h, flags, lda, w_in, n_img, val = v
            picks.append((dict(a_mode=am, M=m, N=n, K=k, ksize=ks, lda=lda, residual=bool(flags & 1), geglu=bool(flags & 2),
                               tail=bool((flags >> 2) & 0xffffff),   # 4 * tc0 + 16384 * tc1: bits 2..25
                               ln=bool(flags & (1 << 30)), u8=bool(flags & (1 << 29)), softmax=bool(flags & (1 << 28)),
                               per_image=bool(flags & (1 << 27))), val % 1000, val // 1000))
    return picks


def picked_tiles(**want):
    """sorted tile ids the shipped table picks for keys whose fields equal `want` (strided=True: rows mode with lda != K)"""
    strided = want.pop('strided', None)
    out = set()
    for key, tile, _ in table_picks():
        if strided is not None and (key['a_mode'] == 0 and key['lda'] != key['K']) != strided:
            continue
        if all(key[f] == v for f, v in want.items()):
            out.add(tile)
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- frames
class Framed:
    """a [rows][width] matrix at column `col` of a [rows + 2][ld] allocation (see the module docstring)"""

    def __init__(self, rows, width, ld, col=0, dtype=torch.float16, fill='sentinel', device=None, data=None):
        mult = 16 if dtype == torch.uint8 else 8
        assert ld % mult == 0 and col % mult == 0 and col + width <= ld, (width, ld, col)
        self.rows, self.width, self.ld, self.col, self.fill = rows, width, ld, col, fill
        device = device or dev()
        if dtype == torch.uint8:
            self.buf = torch.full((rows + 2, ld), 255, dtype=torch.uint8, device=device)
        elif fill == 'nan':
            self.buf = torch.full((rows + 2, ld), float('nan'), dtype=torch.float16, device=device)
        else:
            self.buf = torch.full((rows + 2, ld), SENTINEL, dtype=torch.int16, device=device).view(torch.float16)
        self.view = self.buf[1:1 + rows, col:col + width]
        if data is not None:
            self.view.copy_(data.to(device))
        elif dtype != torch.uint8:
            self.view.fill_(float('nan'))
        assert self.view.data_ptr() % 16 == 0

    def frame_intact(self, name=''):
        bits = self.buf.view(torch.int16).clone()
        bits[1:1 + self.rows, self.col:self.col + self.width] = SENTINEL
        bad = (bits != SENTINEL).nonzero()
        assert bad.numel() == 0, f'{name}: {bad.shape[0]} frame elements changed, first at (row, column) {bad[0].tolist()} of the allocation ' \
                                 f'(matrix rows 1..{self.rows}, columns {self.col}..{self.col + self.width - 1})'


def framed_in(data, ld, col=0):
    """an input (a / w) whose frame is NaN (255 for uint8 codes)"""
    return Framed(data.shape[0], data.shape[1], ld, col, dtype=data.dtype, fill='nan', data=data)


def framed_out(rows, width, ld, col=0):
    return Framed(rows, width, ld, col)


def framed_res(data, ld, col=0):
    return Framed(data.shape[0], data.shape[1], ld, col, data=data)


# ------------------------------------------------------------------------------------------------------------ exact data
def ternary(shape, gen):
    return torch.randint(-1, 2, shape, generator=gen).half()


def small_ints(shape, gen, dtype=torch.float16):
    return torch.randint(-8, 9, shape, generator=gen).to(dtype)


def exact_f16(m, n, k, seed):
    """(a [m][k], w [n][k]) ternary fp16"""
    assert k <= 1600
    gen = torch.Generator().manual_seed(seed)
    return ternary((m, k), gen), ternary((n, k), gen), gen


def exact_u8(m, n, k, seed):
    """(a with at most eight +-1 per row, codes q, w_scale = 1, w_off = offset + 128, the dequantised integer weights)"""
    gen = torch.Generator().manual_seed(seed)
    a = torch.zeros(m, k)
    cols = torch.randint(0, k, (m, 8), generator=gen)                  # (repeated columns: fewer than eight entries)
    a.scatter_(1, cols, torch.randint(0, 2, (m, 8), generator=gen).float() * 2 - 1)
    q = torch.randint(0, 256, (n, k), generator=gen, dtype=torch.uint8)
    offset = torch.where(torch.arange(n) % 3 == 0, torch.tensor(-128.0), torch.where(torch.arange(n) % 3 == 1, torch.tensor(-101.0), torch.tensor(0.0)))
    wf = q.double() + offset.double()[:, None]
    return a.half(), q, torch.ones(n), (offset + 128).float(), wf, gen


def ref_rows(a, wf, bias=None, row_bias=None, rows_per_img=0, residual=None, alpha=1.0, bias_on_m=False):
    """fp64 reference of the un-activated epilogue: alpha * a . wf^T + bias + row_bias + residual"""
    y = alpha * (a.double() @ wf.double().t())
    if bias is not None:
        y = y + (bias.double()[:, None] if bias_on_m else bias.double())
    if row_bias is not None:
        y = y + row_bias.double()[torch.arange(a.shape[0]) // rows_per_img]
    if residual is not None:
        y = y + residual.double()
    return y


def assert_exact(ref):
    """the exact-data bound, checked on the fp64 reference before anything is launched"""
    assert float(ref.abs().max()) <= 2048, float(ref.abs().max())
    assert torch.equal(ref.half().double(), ref), 'reference is not representable in fp16'


def check_equal(out, ref, name=''):
    out = out.detach().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f'{name}: non-finite output ({int((~torch.isfinite(out)).sum())} elements)'
    if not torch.equal(out.double(), ref):
        bad = (out.double() != ref).nonzero()
        i, j = bad[0].tolist()
        raise AssertionError(f'{name}: {bad.shape[0]} of {ref.numel()} elements differ from the exact result, first at ({i}, {j}): '
                             f'{float(out[i, j])} vs {float(ref[i, j])}; rows {sorted(set(bad[:, 0].tolist()))[:8]}, columns {sorted(set(bad[:, 1].tolist()))[:8]}')


def check_close(out, ref, tol=2e-3, name=''):
    """the kernel tests' tolerances (test_kernels_gpu.py imports this as `check`): rel-L2 <= tol, max-abs <= 2e-2 * max|ref| + 1e-3"""
    out = out.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f'{name}: non-finite output'
    r = float((out - ref).flatten().norm() / (ref.flatten().norm() + 1e-30))
    mx = float((out - ref).abs().max()); scale = float(ref.abs().max())
    assert r <= tol, f'{name}: rel-L2 {r:.3e} > {tol} (max abs {mx:.3e}, ref max {scale:.3e})'
    assert mx <= 2e-2 * scale + 1e-3, f'{name}: max abs {mx:.3e} vs ref max {scale:.3e}'


def geglu_perm(h):
    """row order of a [value | gate] weight for the fused GEGLU epilogue: 16-row blocks, value and gate interleaved"""
    perm = torch.empty(2 * h, dtype=torch.long)
    j = torch.arange(h)
    perm[(j // 16) * 32 + j % 16] = j
    perm[(j // 16) * 32 + 16 + j % 16] = h + j
    return perm
