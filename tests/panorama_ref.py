"""A torch CPU restatement of sdod_k_step_windows (include/sdod_hip.h): the MultiDiffusion canvas step, one torch op per rounded
operation and in the kernel's order, so in float32 it gives the kernel's bits; in float64 it is the reference of the trajectories.
No device, no sdod import: the window geometry is restated here too."""
import torch

# the window / canvas / stride shapes at which the kernel can still go wrong, with the origins plan_windows must give
SHAPES = {
    'cover_1_2': dict(window=(16, 16), canvas=(16, 40), stride=8, wrap=False, oy=[0], ox=[0, 8, 16, 24]),
    'clamped_last': dict(window=(16, 16), canvas=(16, 40), stride=16, wrap=False, oy=[0], ox=[0, 16, 24]),
    'grid_2x2': dict(window=(16, 16), canvas=(24, 24), stride=8, wrap=False, oy=[0, 8], ox=[0, 8]),
    'wrap': dict(window=(16, 16), canvas=(16, 32), stride=8, wrap=True, oy=[0], ox=[0, 8, 16, 24]),
    'rect_window': dict(window=(8, 16), canvas=(16, 16), stride=(8, 16), wrap=False, oy=[0, 8], ox=[0]),
    'identity': dict(window=(16, 16), canvas=(16, 16), stride=8, wrap=False, oy=[0], ox=[0]),
}


# ---- the refusals of sdod_k_step_windows: a good call (BASE) and, per case, the struct fields that make it a bad one.  A pointer field
# takes ('null',) or ('offset', bytes); `oy` / `ox` are lists (ny / nx follow their length unless given).  Every case shrinks or keeps
# what a launch would touch, so one that were wrongly accepted would still stay inside BASE's buffers.
BASE = dict(c=4, H=16, W=32, wh=16, ww=16, oy=[0], ox=[0, 8, 16], wrap_x=0, n=2, chunks=2, mode=1, noise_level=1,
            guidance=7.5, d0=1.0, d1=-4.5, a=0.77, b=0.35, cprev=-0.12, u=0.5, stage_scale=0.25)
POINTERS = ('eps', 'x', 'den_prev', 'noise', 'wgt', 'wsum', 'x_stage', 'temb_row', 'temb_dst')
SCALARS = ('guidance', 'd0', 'd1', 'a', 'b', 'cprev', 'u', 'stage_scale')
REFUSALS = [(f'{p} NULL', {p: ('null',)}) for p in ('x', 'wgt', 'wsum')] + \
    [(f'{p} misaligned', {p: ('offset', 4)}) for p in ('x', 'den_prev', 'noise', 'x_stage')] + \
    [(f'{p} misaligned', {p: ('offset', 2)}) for p in ('wgt', 'wsum')] + [('eps misaligned', {'eps': ('offset', 1)})] + \
    [(f'{s} = {v}', {s: v}) for s in SCALARS for v in (float('nan'), float('inf'), -float('inf'))] + [
    ('W no multiple of 4', dict(W=30)), ('c H W no multiple of 4', dict(c=1, H=17, W=30)),
    ('wh no multiple of 4', dict(wh=6)), ('ww no multiple of 4', dict(ww=6)), ('c wh ww no multiple of 4', dict(c=1, wh=2, ww=1)),
    ('oy no multiple of 4', dict(wh=8, oy=[2])), ('ox no multiple of 4', dict(ox=[0, 6, 16])),
    ('oy negative', dict(oy=[-4])), ('ox negative', dict(ox=[-8, 8, 16])),
    ('ny = 0', dict(oy=[])), ('nx = 0', dict(ox=[])), ('ny = 33', dict(ny=33)), ('nx = 33', dict(nx=33)), ('ny = -1', dict(ny=-1)),
    ('oy + wh > H', dict(oy=[4])), ('oy + wh > H (H smaller)', dict(H=12)), ('ox + ww > W', dict(ox=[0, 8, 20])),
    ('wrap: ox >= W', dict(wrap_x=1, ox=[0, 8, 32])), ('wrap: ww > W', dict(wrap_x=1, W=8, ox=[0])), ('wrap_x = 2', dict(wrap_x=2)),
    ('ny nx > chunks n', dict(chunks=1)), ('ny nx > chunks n (n smaller)', dict(n=1)), ('n = 0', dict(n=0)), ('chunks = 0', dict(chunks=0)),
    ('c = 0', dict(c=0)), ('H = 0', dict(H=0)), ('wh = 0', dict(wh=0)),
    ('start form with b', dict(eps=('null',), cprev=0.0, u=0.0)), ('start form with cprev', dict(eps=('null',), b=0.0, u=0.0)),
    ('start form with u', dict(eps=('null',), b=0.0, cprev=0.0)),
    ('cprev without den_prev', dict(den_prev=('null',))), ('mode = 2', dict(mode=2)), ('mode = -1', dict(mode=-1)),
    ('temb_row without temb_dst', dict(temb_dst=('null',))), ('temb_width = 0', dict(temb_width=0)), ('temb_reps = 0', dict(temb_reps=0)),
]


def fill_args(pointers, over=None, temb=(0, 0)):
    """sdod_k_step_windows_args from BASE, the addresses `pointers` {field: int} and temb = (width, reps), with the fields of `over`
    replaced"""
    from sdod.amd import _lib
    v = dict(BASE, temb_width=temb[0], temb_reps=temb[1], **{p: pointers.get(p) for p in POINTERS})
    for key, val in (over or {}).items():
        if isinstance(val, tuple):
            v[key] = None if val[0] == 'null' else pointers[key] + val[1]
        else:
            v[key] = val
    a = _lib.KStepWindowsArgs()
    for key, val in v.items():
        if key in ('oy', 'ox'):
            for i, o in enumerate(val):
                getattr(a, key)[i] = o
        else:
            setattr(a, key, val)
    a.ny, a.nx = v.get('ny', len(v['oy'])), v.get('nx', len(v['ox']))
    return a


def windows(oy, ox, window, canvas, wrap):
    """[(w, rows [wh, 1], cols [1, ww])] in ascending w = iy * len(ox) + ix: the canvas rows and columns of window w, in window order"""
    wh, ww = window
    out = []
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            cols = torch.arange(x0, x0 + ww)
            if wrap:
                cols = cols % canvas[1]
            out.append((iy * len(ox) + ix, torch.arange(y0, y0 + wh)[:, None], cols[None, :]))
    return out


def cover_count(oy, ox, window, canvas, wrap):
    """int64 [H, W]: the number of windows over each canvas pixel"""
    cnt = torch.zeros(canvas, dtype=torch.int64)
    for _, rows, cols in windows(oy, ox, window, canvas, wrap):
        cnt[rows, cols] += 1
    return cnt


def crops(x, oy, ox, window, wrap):
    """x [1, c, H, W] -> [windows, c, wh, ww]: the windows' crops of the canvas, in window order"""
    return torch.stack([x[0][:, rows, cols] for _, rows, cols in windows(oy, ox, window, tuple(x.shape[-2:]), wrap)])


def guided(eps, w, n, g, mode, dtype):
    """CFG of window w from eps [chunks, 2n, wh, ww, c]: -> [c, wh, ww]; mode 1: e_u + g (e_c - e_u); mode 0: e_c g + e_u (1 - g)"""
    eu = eps[w // n, w % n].to(dtype).permute(2, 0, 1)
    ec = eps[w // n, n + w % n].to(dtype).permute(2, 0, 1)
    g = torch.tensor(g, dtype=dtype)
    if mode == 0:
        one_minus = torch.tensor(1.0, dtype=dtype) - g
        return ec * g + eu * one_minus
    diff = ec - eu
    scaled = g * diff
    return eu + scaled


def averaged(eps, wgt, wsum, oy, ox, window, canvas, wrap, n, g, mode, dtype, last_wins=False):
    """e [c, H, W]: acc = acc + wgt * CFG_w over the covering windows in ascending w, then acc / wsum.  last_wins (the negative
    control): the last covering window's prediction instead of the average."""
    c = eps.shape[-1]
    acc = torch.zeros((c,) + tuple(canvas), dtype=dtype)
    wgt = wgt.to(dtype)
    for w, rows, cols in windows(oy, ox, window, canvas, wrap):
        e_w = guided(eps, w, n, g, mode, dtype)
        if last_wins:
            acc[:, rows, cols] = e_w
        else:
            prod = wgt * e_w
            acc[:, rows, cols] = acc[:, rows, cols] + prod
    return acc if last_wins else acc / wsum.to(dtype)


def step(eps, x, coef, wgt, wsum, oy, ox, window, wrap, n, guidance=1.0, mode=1, den_prev=None, nu=None, x_stage=None,
         dtype=torch.float32, last_wins=False):
    """One canvas step.  x [1, c, H, W]; eps fp16 [chunks, 2n, wh, ww, c] or None (the start form); den_prev, nu like x or None; x_stage
    [chunks, 2n, c, wh, ww] (written in place: both rows of every window, nothing else) or None.  Returns (x', den or None) in `dtype`.
    float32: the scalars are rounded to float32 first, as the C struct holds them, and every product and sum is its own torch op."""
    canvas = tuple(x.shape[-2:])
    k = {key: torch.tensor(float(coef.get(key, 1.0 if key == 'd0' else 0.0)), dtype=dtype) for key in ('d0', 'd1', 'a', 'b', 'cprev', 'u', 'stage_scale')}
    one = torch.tensor(1.0, dtype=dtype)
    xv = x[0].to(dtype)
    den = None
    if eps is None:
        xn = (k['a'] * xv) / one
    else:
        e = averaged(eps, wgt, wsum, oy, ox, window, canvas, wrap, n, guidance, mode, dtype, last_wins)
        t0 = k['d0'] * xv
        t1 = k['d1'] * e
        den = (t0 + t1) / one
        t0 = k['a'] * xv
        t1 = k['b'] * den
        xn = t0 + t1
        if float(k['cprev']) != 0.0:
            t2 = k['cprev'] * den_prev[0].to(dtype)
            xn = xn + t2
        if float(k['u']) != 0.0:
            t3 = k['u'] * nu[0].to(dtype)
            xn = xn + t3
        xn = xn / one
    if x_stage is not None:
        st = k['stage_scale'] * xn
        for w, rows, cols in windows(oy, ox, window, canvas, wrap):
            x_stage[w // n, w % n] = st[:, rows, cols].to(x_stage.dtype)
            x_stage[w // n, n + w % n] = st[:, rows, cols].to(x_stage.dtype)
    return xn[None], (None if den is None else den[None])
