"""The two device transforms finalize() runs in place on a graph's weights, each against fp64 (references: tests/weight_prep_ref.py).

sdod_compose_linear_f16 (ff.net.2 -> proj_out and encoder.conv_out -> quant_conv become one matrix).  Contract: fp32 accumulate,
rounded to fp16 ONCE; bias_out = P bw + bp in fp32.  Every element is held to

    |got - ref| <= 2^-11 |ref| + 2^-25 + n_mid 2^-23 sum_j |p_oj w_jk|        ref = P.double() @ W.double()
    |bias - ref| <= (n_mid + 1) 2^-23 (sum_j |p_oj bw_j| + |bp_o|)

which is one fp16 rounding (half an ulp, or half the subnormal spacing) plus the standard bound of sequential fp32 accumulation with a
factor 2 of slack: derived from the contract, not measured.  That the bound is tight enough to refuse a wrong kernel was checked on
the CPU and stays checked by test_compose_bound_refuses_wrong_kernels (no GPU): at every shape below, with weights
randn / sqrt(fan_in), a variant that keeps the running sum in fp16 exceeds the bound (worst element 63 to 150 times over where
k >= 255, 2.1 times at k = 1), so does one that rounds each product to fp16 before an fp32 sum (12 to 115 times, 1.7 at k = 1), while
the contract evaluated on the CPU reaches at most 0.98 of it (one rounding alone comes close to half an ulp somewhere).

Shapes: the UNet form as run_folds passes it (p = the column block at 4C of the rows c starts in, w a dense copy; C = 64, and 72 so
that k = 288 leaves a 32-lane remainder in the second 256-thread block), the VAE-encoder form (8 x 8 times 8 x 576 in rows of 584),
k at the block edge (1, 255, 256, 257), all eight combinations of NULL biases, and the refusals.  bias_out = NULL with the other two
set writes no bias and reads neither: compose_linear_kernel's bias branch is `if (blockIdx.x == 0 && threadIdx.x == 0 && bias_out)`,
and bias_w / bias_p are dereferenced only inside it (read in csrc/norms.hip before this test first ran).  The destination's
allocation is filled with a sentinel bit pattern first: every column outside [0, k) keeps its bits, the p block included.

sdod_ln_fold_f16: what tests/test_row_kernels_gpu.py::test_ln_fold_kernel_vs_fp64 (K = 64, 320, 1000 at ldw = K + 8) lacks: K = 8,
248, 264 (not multiples of 256, one below and one above a whole block) and 320, at ldw = K + 8 and K + 24, with and without
bias_in, sentinel-framed, W' bit for bit and s / t within K 2^-23 sum |W'| and (K + 1) 2^-23 (sum |beta W| + |bias|)."""
import ctypes

import pytest
import torch

import weight_prep_ref as R

gpu = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def factors(n_out, n_mid, k, seed):
    """fp16 (p, w) of the scale the engine's own tests use, fp32 (bias_w, bias_p)"""
    gen = torch.Generator().manual_seed(seed)
    p = (torch.randn(n_out, n_mid, generator=gen) * n_mid ** -0.5).half()
    w = (torch.randn(n_mid, k, generator=gen) * k ** -0.5).half()
    return p, w, 0.1 * torch.randn(n_mid, generator=gen), 0.1 * torch.randn(n_out, generator=gen)


# (name, n_out, n_mid, k, ldc, column of p inside c's rows or None = a matrix of its own, ldw)
COMPOSE_SHAPES = [
    ('unet_c64', 64, 64, 256, 320, 256, 256),
    ('unet_c72', 72, 72, 288, 360, 288, 288),
    ('vae_encoder', 8, 8, 576, 584, 576, 576),
    ('k1', 3, 5, 1, 4, None, 1),
    ('k255', 3, 5, 255, 258, None, 255),
    ('k256', 3, 5, 256, 259, None, 259),
    ('k257', 3, 5, 257, 260, None, 264),
]
SHAPE_IDS = [s[0] for s in COMPOSE_SHAPES]


def test_compose_bound_refuses_wrong_kernels():
    """no GPU: at every shape of this file the bound passes the contract and fails an fp16-accumulating and an fp16-product kernel"""
    for name, n_out, n_mid, k, _, _, _ in COMPOSE_SHAPES:
        p, w, _, _ = factors(n_out, n_mid, k, seed=len(name) + k)
        ref, mag, _, _ = R.compose_ref(p, w)
        bound = R.compose_bound(ref, mag, n_mid)
        good = R.worst_ratio(R.compose_like_kernel(p, w), ref, bound)
        acc16 = R.worst_ratio(R.compose_wrong_fp16_accumulate(p, w), ref, bound)
        prod16 = R.worst_ratio(R.compose_wrong_fp16_products(p, w), ref, bound)
        print(f'compose bound {name}: contract {good:.3f}, fp16 accumulate {acc16:.2f}, fp16 products {prod16:.2f} (of the bound)')
        assert good <= 1, (name, good)
        assert acc16 > 1 and prod16 > 1, (name, acc16, prod16)


class ComposeRun:
    """one launch on sentinel-framed memory: c = columns [0, k) of rows 1 .. n_out of a [n_out + 2][ldc] allocation"""

    def __init__(self, shape, p, w, bias_w, bias_p, with_out=True):
        _, self.n_out, self.n_mid, self.k, self.ldc, self.p_col, self.ldw = shape
        d = dev()
        self.cbuf = torch.full((self.n_out + 2, self.ldc), R.SENTINEL, dtype=torch.int16, device=d)
        self.c = self.cbuf[1:1 + self.n_out]
        if self.p_col is None:
            self.ldp = self.n_mid + 3
            self.pbuf = torch.full((self.n_out, self.ldp), R.SENTINEL, dtype=torch.int16, device=d)
            self.p = self.pbuf[:, :self.n_mid]
        else:
            self.ldp = self.ldc
            self.p = self.c[:, self.p_col:self.p_col + self.n_mid]
        self.p.copy_(p.view(torch.int16))
        self.wbuf = torch.full((self.n_mid, self.ldw), R.SENTINEL, dtype=torch.int16, device=d)
        self.wbuf[:, :self.k].copy_(w.view(torch.int16))
        self.bw = None if bias_w is None else bias_w.to(d)
        self.bp = None if bias_p is None else bias_p.to(d)
        self.bout = torch.full((self.n_out + 2,), R.SENTINEL32, dtype=torch.int32, device=d) if with_out else None
        self.before = self.cbuf.clone()

    def args(self, **kw):
        a = dict(p=self.p.data_ptr(), ldp=self.ldp, w=self.wbuf.data_ptr(), ldw=self.ldw, c=self.c.data_ptr(), ldc=self.ldc, n_out=self.n_out,
                 n_mid=self.n_mid, k=self.k)
        a.update(kw)
        return a

    def launch(self, **kw):
        from sdod.amd import _lib, ops
        a = self.args(**kw)
        vp = lambda v: ctypes.c_void_p(v) if v else None
        rc = _lib.hip().sdod_compose_linear_f16(vp(a['p']), a['ldp'], vp(a['w']), a['ldw'], vp(a['c']), a['ldc'], a['n_out'], a['n_mid'], a['k'],
                                                ptr(self.bw), ptr(self.bp), None if self.bout is None else ctypes.c_void_p(self.bout[1:].data_ptr()),
                                                ops._stream())
        try:
            _lib.check(rc)
        finally:
            torch.cuda.synchronize()

    def untouched(self, name):
        """everything of c's allocation but columns [0, k) of its rows kept its bits: the guard rows, the columns behind k, p"""
        now, want = self.cbuf.clone(), self.before.clone()
        now[1:1 + self.n_out, :self.k] = 0
        want[1:1 + self.n_out, :self.k] = 0
        bad = (now != want).nonzero()
        assert bad.numel() == 0, f'{name}: {bad.shape[0]} elements outside the k columns changed, first at (row, column) {bad[0].tolist()}'

    def intact(self, name):
        assert torch.equal(self.cbuf, self.before), f'{name}: a refused call wrote to the destination'
        if self.bout is not None:
            assert bool((self.bout == R.SENTINEL32).all()), f'{name}: a refused call wrote a bias'

    def got(self):
        return self.c[:, :self.k].contiguous().view(torch.float16).cpu()

    def bias(self):
        assert int(self.bout[0]) == R.SENTINEL32 and int(self.bout[-1]) == R.SENTINEL32, 'bias_out written outside its n_out elements'
        return self.bout[1:-1].view(torch.float32).cpu()


def check_compose(run, name, p, w, bias_w, bias_p):
    ref, mag, bref, bmag = R.compose_ref(p, w, bias_w, bias_p)
    worst = R.worst_ratio(run.got(), ref, R.compose_bound(ref, mag, run.n_mid))
    msg = f'compose {name}: worst |err| / bound {worst:.3f}'
    assert worst <= 1, msg
    run.untouched(name)
    if run.bout is not None:
        bound = R.compose_bias_bound(bmag, run.n_mid)
        got = run.bias()
        if float(bmag.max()) == 0:        # no bias at all: exactly zero
            assert bool((got == 0).all()), f'{name}: bias without terms is not zero'
        else:
            bworst = R.worst_ratio(got, bref, bound)
            msg += f', bias {bworst:.3f}'
            assert bworst <= 1, msg
    print(msg)


@gpu
@pytest.mark.parametrize('shape', COMPOSE_SHAPES, ids=SHAPE_IDS)
def test_compose_linear_vs_fp64(shape):
    name, n_out, n_mid, k = shape[:4]
    p, w, bw, bp = factors(n_out, n_mid, k, seed=len(name) + k)
    run = ComposeRun(shape, p, w, bw, bp)
    run.launch()
    check_compose(run, name, p, w, bw, bp)
    first, first_bias = run.cbuf.clone(), run.bout.clone()
    again = ComposeRun(shape, p, w, bw, bp)
    again.launch()
    assert torch.equal(first, again.cbuf) and torch.equal(first_bias, again.bout), f'{name}: two runs differ'


@gpu
@pytest.mark.parametrize('shape', [COMPOSE_SHAPES[0], COMPOSE_SHAPES[6]], ids=[SHAPE_IDS[0], SHAPE_IDS[6]])
def test_compose_linear_bias_combinations(shape):
    name, n_out, n_mid, k = shape[:4]
    p, w, bw, bp = factors(n_out, n_mid, k, seed=17)
    for has_w in (True, False):
        for has_p in (True, False):
            for has_out in (True, False):
                run = ComposeRun(shape, p, w, bw if has_w else None, bp if has_p else None, with_out=has_out)
                run.launch()
                check_compose(run, f'{name} bias_w {has_w} bias_p {has_p} bias_out {has_out}', p, w, bw if has_w else None, bp if has_p else None)


REFUSALS = [
    ('p null', dict(p=0)), ('w null', dict(w=0)), ('c null', dict(c=0)),
    ('n_out 0', dict(n_out=0)), ('n_mid 0', dict(n_mid=0)), ('k 0', dict(k=0)),
    ('n_out -1', dict(n_out=-1)), ('n_mid -1', dict(n_mid=-1)), ('k -1', dict(k=-1)),
    ('ldp < n_mid', 'ldp'), ('ldw < k', 'ldw'), ('ldc < k', 'ldc'),
    ('c == w', 'c_is_w'), ('c == p', 'c_is_p'), ('w = c + 8 halves', 'w_in_c'), ('w ends inside c', 'w_into_c'), ('w = the p block', 'w_is_p'),
]


@gpu
@pytest.mark.parametrize('shape', [COMPOSE_SHAPES[0], COMPOSE_SHAPES[5]], ids=[SHAPE_IDS[0], SHAPE_IDS[5]])
def test_compose_linear_refusals(shape):
    from sdod.amd import _lib
    name, n_out, n_mid, k = shape[:4]
    p, w, bw, bp = factors(n_out, n_mid, k, seed=23)
    run = ComposeRun(shape, p, w, bw, bp)
    a = run.args()
    for what, kw in REFUSALS:
        if kw == 'ldp':
            kw = dict(ldp=n_mid - 1)
        elif kw == 'ldw':
            kw = dict(ldw=k - 1)
        elif kw == 'ldc':
            kw = dict(ldc=k - 1)
        elif kw == 'c_is_w':
            kw = dict(w=a['c'], ldw=a['ldc'])
        elif kw == 'c_is_p':
            kw = dict(p=a['c'], ldp=a['ldc'])
        elif kw == 'w_in_c':        # the racy case: rows of w inside the span other workgroups store to
            kw = dict(w=a['c'] + 16, ldw=a['ldc'])
        elif kw == 'w_into_c':      # w starts in the guard row above c and runs into c's first rows
            kw = dict(w=a['c'] - 2 * a['ldc'], ldw=a['ldc'])
        elif kw == 'w_is_p':        # a w in c's own rows, even at columns >= k, lies inside the written span
            if run.p_col is None:
                continue
            kw = dict(w=a['p'], ldw=a['ldc'], k=min(k, n_mid))
        with pytest.raises(_lib.SdodError):
            run.launch(**kw)
        run.intact(f'{name}: {what}')
    run.launch()                    # ... and the same object still composes: p inside c's rows at columns >= k stays legal
    check_compose(run, name, p, w, bw, bp)


# ------------------------------------------------------------------------------------------------ ln_fold at a row stride above K
@gpu
@pytest.mark.parametrize('pad', [8, 24])
@pytest.mark.parametrize('k', [8, 248, 264, 320])
def test_ln_fold_strided_vs_fp64(k, pad):
    from sdod.amd import _lib, ops
    d = dev()
    n, ldw = 5, k + pad
    gen = torch.Generator().manual_seed(1000 * pad + k)
    w = (torch.randn(n, k, generator=gen) * k ** -0.5).half()
    w.view(-1)[:len(R.F16_EDGES_SMALL)] = torch.tensor(R.F16_EDGES_SMALL).half()[:w.numel()]
    gamma, beta, bias = 1 + 0.1 * torch.randn(k, generator=gen), 0.1 * torch.randn(k, generator=gen), 0.1 * torch.randn(n, generator=gen)
    gamma[:2] = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11])        # products on fp16 ties
    for b in (bias, None):
        buf = torch.full((n + 2, ldw), R.SENTINEL, dtype=torch.int16, device=d)
        buf[1:1 + n, :k].copy_(w.view(torch.int16))
        before = buf.clone()
        st = torch.full((2, n + 2), R.SENTINEL32, dtype=torch.int32, device=d)
        gd, bd, biasd = gamma.to(d), beta.to(d), None if b is None else b.to(d)
        _lib.check(_lib.hip().sdod_ln_fold_f16(ptr(buf[1:]), n, k, ldw, ptr(gd), ptr(bd), ptr(biasd), ptr(st[0, 1:]), ptr(st[1, 1:]), ops._stream()))
        torch.cuda.synchronize()
        name = f'ln_fold K {k} ldw {ldw} bias {b is not None}'
        got = buf[1:1 + n, :k].contiguous().view(torch.float16).cpu()
        now = buf.clone(); now[1:1 + n, :k] = 0; before[1:1 + n, :k] = 0
        assert torch.equal(now, before), f'{name}: wrote outside its K columns'
        assert bool((st[:, 0] == R.SENTINEL32).all()) and bool((st[:, -1] == R.SENTINEL32).all()), f'{name}: s / t written outside n elements'
        wf, s_ref, s_tol, t_ref, t_tol = R.ln_fold_ref(w, gamma, beta, b)
        assert torch.equal(R.bits(got), R.bits(wf)), f'{name}: folded weight is not fp16(float(w) * gamma)'
        s, t = st[0, 1:-1].view(torch.float32).cpu().double(), st[1, 1:-1].view(torch.float32).cpu().double()
        print(f'{name}: s within {float(((s - s_ref).abs() / s_tol).max()):.3f}, t within {float(((t - t_ref).abs() / t_tol).max()):.3f} of the bound')
        assert bool(((s - s_ref).abs() <= s_tol).all()), (name, s, s_ref)
        assert bool(((t - t_ref).abs() <= t_tol).all()), (name, t, t_ref)
