"""Host side of the wide attention kernel and of the VAE graphs' fused_attn switch: the width predicates, the argument checks of
sdod_attention_wide_f16 (an error code before any launch: the pointers here are never dereferenced) and the create-time refusals."""
import ctypes

import pytest

from sdod.amd import _lib, engine as E
from sdod.amd._lib import SdodError, check


def test_width_predicates():
    lib = _lib.hip()
    assert [d for d in (40, 64, 160, 256, 512, 1024) if lib.sdod_attention_wide_dim_ok(d)] == [256, 512]
    assert [d for d in range(-8, 513) if lib.sdod_attention_head_dim_ok(d)] == [40, 64, 80, 160]


def test_key_splits_by_grid():
    lib = _lib.hip()
    # one workgroup per 64 query rows in rounds of 256 (d = 512); the keys are split where that fills the rounds better: 64 -> 4 x 64,
    # 144 -> 7 x 144 = 1008 (4 rounds of a seventh), 256 and 512 fill theirs, 272 -> 7 x 272 = 1904 (8 rounds of a seventh)
    assert [lib.sdod_attention_wide_splits(1, n, n, 512) for n in (64 * 64, 96 * 96, 128 * 128, 128 * 136, 64 * 512)] == [4, 7, 1, 7, 1]
    assert lib.sdod_attention_wide_splits(2, 4096, 4096, 512) == 2 and lib.sdod_attention_wide_splits(2, 200, 200, 256) == 1
    assert lib.sdod_attention_wide_splits(1, 64, 64, 80) == 0
    assert lib.sdod_attention_wide_ws_bytes(1, 4096, 4096, 512) == 4 * 4096 * 514 * 4 and lib.sdod_attention_wide_ws_bytes(1, 16384, 16384, 512) == 0


@pytest.mark.parametrize('bad,word', [(dict(ldq=516), 'ldq'), (dict(ldo=500), 'ldo'), (dict(scale=0.0), 'scale'), (dict(scale=-1.0), 'scale'),
                                      (dict(d=160), 'd must'), (dict(lk=0), 'lk'), (dict(q=4104), 'aligned')])
def test_wide_attention_refuses(bad, word):
    a = dict(q=4096, k=8192, v=12288, out=16384, batch=1, lq=64, lk=64, d=512, ldq=1024, ldk=1024, ldv=512, ldo=512, scale=0.044)
    a.update(bad)
    with pytest.raises(SdodError, match=word) as e:
        check(_lib.hip().sdod_attention_wide_f16(a['q'], a['k'], a['v'], a['out'], a['batch'], a['lq'], a['lk'], a['d'], a['ldq'], a['ldk'],
                                                 a['ldv'], a['ldo'], a['scale'], None))
    assert e.value.code == 2


def test_fused_attn_refused_at_create():
    cfg = E.sd14_config(16, 16)
    cfg.vae_channels = 256
    with pytest.raises(SdodError, match='vae_channels'):
        E.VaeDecoder(cfg, 1, fused_attn=True)
    h = ctypes.c_void_p()
    cfg = E.sd14_config(16, 16)
    with pytest.raises(SdodError, match='kind'):
        check(E._engine().sdod_graph_create_vae(ctypes.byref(h), E.UNET, ctypes.byref(cfg), 0, ctypes.byref(E.VaeConfig(1)), 2))
    assert E.VaeDecoder(cfg, 1, fused_attn=True).param_table() == E.VaeDecoder(cfg, 1).param_table()
