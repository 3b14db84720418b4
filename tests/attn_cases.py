"""Shared pieces of the attention kernel tests (test_attention_deferred_rescale_gpu.py, test_attention_paths_gpu.py): the fp64
reference on the same fp16-rounded inputs, the tolerance check, and inputs with planted rows.

Planted rows: row r's query is the unit vector of head dimension j, so its raw scores are column j of K, which the builder
writes key by key -- a jump of the running maximum at a chosen tile, scores near -300, scores spread over +-60, ...  The
remaining rows are random.  Tolerances are those of the attention kernel tests: rel-L2 <= 3e-3 and max-abs <= 2e-2 * max|ref|
+ 1e-3."""
import torch

LOG2E = 1.4426950408889634


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def check(out, ref, tol=3e-3, name=''):
    out = out.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f'{name}: non-finite output'
    r = float((out - ref).flatten().norm() / (ref.flatten().norm() + 1e-30))
    mx = float((out - ref).abs().max()); scale = float(ref.abs().max())
    assert r <= tol, f'{name}: rel-L2 {r:.3e} > {tol} (max abs {mx:.3e}, ref max {scale:.3e})'
    assert mx <= 2e-2 * scale + 1e-3, f'{name}: max abs {mx:.3e} vs ref max {scale:.3e}'


def ref_attention(q, k, v, heads, causal, scale=None):
    b, lq, c = q.shape
    d = c // heads
    qh = q.double().reshape(b, lq, heads, d).transpose(1, 2)
    kh = k.double().reshape(b, -1, heads, d).transpose(1, 2)
    vh = v.double().reshape(b, -1, heads, d).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * (d ** -0.5 if scale is None else scale)
    if causal:
        s = s.masked_fill(torch.ones(lq, kh.shape[2], dtype=torch.bool).triu(1), float('-inf'))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(b, lq, c)


def patterns(lk, d, gen, scale=None):
    """{name: raw (unscaled) scores of one row over the lk keys}; the threshold in raw units is THR / (scale * log2 e)"""
    thr_raw = 8.0 / ((d ** -0.5 if scale is None else scale) * LOG2E)
    nt = (lk + 63) // 64
    noise = lambda lo, hi: torch.rand(lk, generator=gen) * (hi - lo) + lo  # noqa: E731
    pats = {}

    def jump_at(key, height):
        p = noise(-1.0, 1.0)
        p[min(key, lk - 1)] = height
        return p
    if nt > 1:
        pats['jump_tile1'] = jump_at(64 + 5, 3 * thr_raw)
        pats['jump_middle'] = jump_at((nt // 2) * 64 + 17, 5 * thr_raw)
        pats['jump_last_full'] = jump_at((lk // 64 - 1) * 64 + 40, 2.5 * thr_raw)
        below = torch.zeros(lk)
        below[min(64 + 9, lk - 1)] = 0.985 * thr_raw  # the first tile sets m = 0 exactly; this key stays just under the threshold
        pats['just_below'] = below
        above = torch.zeros(lk)
        above[min(64 + 9, lk - 1)] = 1.02 * thr_raw
        pats['just_above'] = above
        steps = noise(-1.0, 1.0)
        for i, t in enumerate(range(1, nt, max(1, nt // 4))):
            steps[min(t * 64 + (7 * i) % 64, lk - 1)] = (i + 2) * 1.5 * thr_raw
        pats['several_jumps'] = steps
    if lk % 64:
        pats['jump_ragged'] = jump_at(lk - 1, 4 * thr_raw)
    pats['near_minus_300'] = noise(-303.0, -297.0)
    pats['pm60'] = noise(-60.0, 60.0)
    first = noise(-60.0, -40.0)
    first[0] = 60.0
    pats['max_at_key0'] = first
    pats['jump_tile0'] = jump_at(50, 3 * thr_raw)
    return pats


def build(b, heads, lq, lk, d, seed, scale=None):
    gen = torch.Generator().manual_seed(seed)
    c = heads * d
    q = torch.randn(b, lq, c, generator=gen)
    k = torch.randn(b, lk, c, generator=gen)
    v = torch.randn(b, lk, c, generator=gen)
    pats = patterns(lk, d, gen, scale)
    rows = []
    # planted rows spread over waves and query tiles; each pattern gets its own head dimension j, in every (batch, head)
    for i, (name, p) in enumerate(pats.items()):
        j = i % d
        row = (i * 37 + 3) % lq
        for bb in range(b):
            for hh in range(heads):
                q[bb, row, hh * d:(hh + 1) * d] = 0.0
                q[bb, row, hh * d + j] = 1.0
                k[bb, :, hh * d + j] = p
        rows.append(row)
    return q.half(), k.half(), v.half(), sorted(set(rows))
