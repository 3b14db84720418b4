"""sdod_attention_shared_f16 (reference-only control): self-attention whose main sequences also attend to the keys of an
anchor sequence of the same batch, blended with the self-only result by a per-group weight read from device memory.

Every case: heads = 2, q / k / v column slices of one packed [batch * l][3 * heads * d] buffer, the output a column slice of a wider
sentinel-filled one.  Asserted: attn_cases.check at its default tolerance against fp64 -- w * ref_attention(own) + (1 - w) *
ref_attention(own ; anchor), plain for the anchors; no byte outside the slice written; w = 1 everywhere is ops.attention bit for bit."""
import ctypes
import functools

import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu

HEADS, SENTINEL, PAD = 2, -1234.0, 8
GROUPS = [(1, 3, (0.5,)), (2, 6, (0.0, 0.0)), (2, 6, (1.0, 0.25))]
# l: 16 -- both segments one ragged tile, a masked tile followed by more keys; 64 -- segments end on a tile; 80 -- a ragged second tile;
# 192 -- three tiles per segment; 256 -- the d = 80 key/value split; 320 -- five tiles, shared unevenly by the split's groups (d = 80 only)
SHAPES = [(d, l) for d in (40, 64, 80, 160) for l in (16, 64, 80, 192, 256)] + [(80, 320)]


@functools.lru_cache(maxsize=None)
def case(d, l, batch, anchors, boost):
    """(packed [batch, l, 3 c] fp16, {w tuple -> fp64 reference}): the two softmaxes once per shape, blended per weight set"""
    q, k, v, _ = AC.build(batch, HEADS, l, l, d, seed=7000 + 10 * d + l + batch)
    if boost:  # the anchors' scores grow fourfold: the running maximum moves by more than the deferred-shift threshold behind the snapshot
        k[batch - anchors:] *= boost
    n, per = batch - anchors, (batch - anchors) // anchors
    own = AC.ref_attention(q, k, v, HEADS, False)
    anc = [n + b // per for b in range(n)]
    both = AC.ref_attention(q[:n], torch.cat([k[:n], k[anc]], 1), torch.cat([v[:n], v[anc]], 1), HEADS, False)

    def ref(ws):
        w = torch.tensor([ws[b // per] for b in range(n)], dtype=torch.float64).reshape(n, 1, 1)
        return torch.cat([w * own[:n] + (1 - w) * both, own[n:]])
    return torch.cat([q, k, v], dim=-1).contiguous(), ref


def run(ops, packed, anchors, ws):
    buf = packed.to(AC.dev())
    (b, l, _), c = buf.shape, buf.shape[2] // 3
    q, k, v = (buf[:, :, i * c:(i + 1) * c] for i in range(3))
    wide = torch.full((b, l, c + 2 * PAD), SENTINEL, dtype=torch.float16, device=AC.dev())
    out = wide[:, :, PAD:PAD + c]
    ops.attention_shared(q, k, v, HEADS, anchors, torch.tensor(ws, dtype=torch.float32, device=AC.dev()), out=out)
    torch.cuda.synchronize()
    assert (wide[:, :, :PAD] == SENTINEL).all() and (wide[:, :, PAD + c:] == SENTINEL).all(), 'wrote outside the output slice'
    return out, (q, k, v)


@pytest.mark.parametrize('qt', [None, '1', '2'])
@pytest.mark.parametrize('anchors,batch,ws', GROUPS)
@pytest.mark.parametrize('d,l', SHAPES)
def test_shared_attention(monkeypatch, d, l, anchors, batch, ws, qt):
    from sdod.amd import ops
    monkeypatch.delenv('SDOD_ATTN_QT', raising=False) if qt is None else monkeypatch.setenv('SDOD_ATTN_QT', qt)
    packed, ref = case(d, l, batch, anchors, 0)
    out, _ = run(ops, packed, anchors, ws)
    AC.check(out, ref(ws), name=f'd{d} l{l} a{anchors} w{ws} qt{qt}')


@pytest.mark.parametrize('d', [40, 64, 80, 160])
def test_shared_attention_maximum_moves_behind_the_snapshot(d):
    from sdod.amd import ops
    packed, ref = case(d, 80, 6, 2, 4)
    out, _ = run(ops, packed, 2, (0.5, 0.25))
    AC.check(out, ref((0.5, 0.25)), name=f'd{d} boosted anchors')


@pytest.mark.parametrize('qt', [None, '1', '2'])
@pytest.mark.parametrize('d,l', [(d, l) for d in (40, 64, 80, 160) for l in (80, 256)] + [(80, 320)])
def test_self_weight_one_is_plain_attention(monkeypatch, d, l, qt):
    from sdod.amd import ops
    monkeypatch.delenv('SDOD_ATTN_QT', raising=False) if qt is None else monkeypatch.setenv('SDOD_ATTN_QT', qt)
    packed, _ = case(d, l, 6, 2, 0)
    out, (q, k, v) = run(ops, packed, 2, (1.0, 1.0))
    assert torch.equal(out, ops.attention(q.contiguous(), k.contiguous(), v.contiguous(), HEADS)), 'differs from ops.attention'


REFUSALS = {'no anchors': dict(anchors=0), 'three anchors': dict(anchors=3), 'indivisible batch': dict(batch=5), 'only anchors': dict(batch=2),
            'null self_w': dict(w_null=True), 'head dim 48': dict(d=48), 'misaligned pointer': dict(q_off=2), 'out inside the k / v range': dict(out_in_buf=True)}


@pytest.mark.parametrize('name', REFUSALS)
def test_shared_attention_refuses(name):
    from sdod.amd import _lib
    a = {**dict(batch=6, anchors=2, d=40, q_off=0, w_null=False, out_in_buf=False), **REFUSALS[name]}
    buf = torch.zeros(6 * 16 * 240 + 8, dtype=torch.float16, device=AC.dev())
    w = torch.zeros(2, dtype=torch.float32, device=AC.dev())
    wide = torch.full((6, 16, 96), SENTINEL, dtype=torch.float16, device=AC.dev())
    p = buf.data_ptr()
    rc = _lib.hip().sdod_attention_shared_f16(ctypes.c_void_p(p + a['q_off']), ctypes.c_void_p(p + 160), ctypes.c_void_p(p + 320),
                                              ctypes.c_void_p(p + 800 if a['out_in_buf'] else wide.data_ptr() + 16), a['batch'], HEADS, 16, a['d'], 240, 240, 240, 96,
                                              40 ** -0.5, a['anchors'], None if a['w_null'] else ctypes.c_void_p(w.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 2, (name, rc)                                    # INVALID_ARGUMENT
    assert (wide == SENTINEL).all(), 'a refused call wrote to its output'
