"""sdod_attention_tiled_f16 (HyperTile): self-attention inside the th x tw tiles of an h x w token map, in place.

Every case: B = 2, heads = 2, q / k / v column offsets into one packed [B * h * w][3 * heads * d] buffer, the output a column slice of a
wider sentinel-filled buffer.  Asserted: (i) attn_cases.check against the fp64 reference (rearrange, ref_attention per tile, rearrange
back) at the attention kernel's tolerances; (ii) every tile equals ops.attention on the tile's rows gathered into contiguous tensors,
bit for bit (the dispatch is shared, so the form and the arithmetic are); (iii) every byte outside the written slice is unchanged.
The inputs are attn_cases.build's for the gathered problem (its planted rows sit in every tile), scattered onto the map."""
import ctypes
import functools

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu

B, HEADS, SENTINEL, PAD = 2, 2, -1234.0, 8
# (h, w, th, tw), each the smallest that reaches its hazard: 16-key tiles (shorter than a key tile and a query block); tw not dividing
# 64 and a ragged second key tile; 240 keys with a carry of the incremental map on every step; a 3 x 1 grid whose tiles span full
# rows; 256 keys (the d = 80 key/value split); a 1 x 1 grid (= ops.attention on the whole map)
GEOMS = [(8, 8, 4, 4), (16, 24, 8, 12), (24, 40, 12, 20), (24, 16, 8, 16), (32, 32, 16, 16), (16, 16, 16, 16)]


def gather(t, h, w, th, tw):
    """[B, h * w, C] -> [B * nh * nw, th * tw, C]"""
    return t.reshape(t.shape[0], h // th, th, w // tw, tw, -1).permute(0, 1, 3, 2, 4, 5).reshape(-1, th * tw, t.shape[-1])


def scatter(t, h, w, th, tw):
    """the inverse of gather"""
    return t.reshape(-1, h // th, w // tw, th, tw, t.shape[-1]).permute(0, 1, 3, 2, 4, 5).reshape(-1, h * w, t.shape[-1])


@functools.lru_cache(maxsize=None)
def case(d, geom):
    h, w, th, tw = geom
    tiles = B * (h // th) * (w // tw)
    q, k, v, _ = AC.build(tiles, HEADS, th * tw, th * tw, d, seed=1000 * d + h * w + tw)
    ref = scatter(AC.ref_attention(q, k, v, HEADS, False), h, w, th, tw)
    packed = torch.cat([scatter(t, h, w, th, tw) for t in (q, k, v)], dim=-1).contiguous()
    return packed, ref


def sentinel_out(h, w, c):
    wide = torch.full((B, h * w, c + 2 * PAD), SENTINEL, dtype=torch.float16, device=AC.dev())
    return wide, wide[:, :, PAD:PAD + c]


@pytest.mark.parametrize('qt', [None, '1', '2'])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'x'.join(map(str, g)))
@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_tiled_attention(monkeypatch, d, geom, qt):
    from sdod.amd import ops
    if qt is None:
        monkeypatch.delenv('SDOD_ATTN_QT', raising=False)
    else:
        monkeypatch.setenv('SDOD_ATTN_QT', qt)
    h, w, th, tw = geom
    c = HEADS * d
    packed, ref = case(d, geom)
    buf = packed.to(AC.dev())
    q, k, v = (buf[:, :, i * c:(i + 1) * c] for i in range(3))
    wide, out = sentinel_out(h, w, c)
    ops.attention_tiled(q, k, v, HEADS, (h, w), (th, tw), out=out)
    per_tile = ops.attention(*(gather(t, h, w, th, tw).contiguous() for t in (q, k, v)), HEADS)
    torch.cuda.synchronize()
    AC.check(out, ref, name=f'd{d} {geom} qt{qt}')
    assert torch.equal(gather(out, h, w, th, tw), per_tile), 'a tile differs from ops.attention on its gathered rows'
    assert (wide[:, :, :PAD] == SENTINEL).all() and (wide[:, :, PAD + c:] == SENTINEL).all(), 'wrote outside the output slice'


REFUSALS = {
    'th does not divide h': dict(th=5),
    'tw does not divide w': dict(tw=3),
    'zero height': dict(h=0),
    'negative batch': dict(batch=-1),
    'zero tile': dict(th=0),
    'head dim 48': dict(d=48),
    'stride below heads * d': dict(ldk=72),
    'misaligned pointer': dict(q_off=2),
    'zero scale': dict(scale=0.0),
    'negative scale': dict(scale=-0.1),
    'null pointer': dict(v_null=True),
}


@pytest.mark.parametrize('name', REFUSALS)
def test_tiled_attention_refuses(name):
    from sdod.amd import _lib
    a = dict(batch=B, heads=HEADS, h=8, w=8, th=4, tw=4, d=40, ldq=240, ldk=240, ldv=240, ldo=96, scale=40 ** -0.5, q_off=0, v_null=False)
    a.update(REFUSALS[name])
    buf = torch.zeros(B * 64 * 240 + 8, dtype=torch.float16, device=AC.dev())
    wide, out = sentinel_out(8, 8, 80)
    p = buf.data_ptr()
    rc = _lib.hip().sdod_attention_tiled_f16(ctypes.c_void_p(p + a['q_off']), ctypes.c_void_p(p + 160), None if a['v_null'] else ctypes.c_void_p(p + 320),
                                             ctypes.c_void_p(out.data_ptr()), a['batch'], a['heads'], a['h'], a['w'], a['th'], a['tw'], a['d'],
                                             a['ldq'], a['ldk'], a['ldv'], a['ldo'], a['scale'], None)
    torch.cuda.synchronize()
    assert rc == 2, (name, rc)                                    # INVALID_ARGUMENT
    assert (wide == SENTINEL).all(), 'a refused call wrote to its output'
