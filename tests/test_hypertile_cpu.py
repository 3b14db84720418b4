"""HyperTile's host side without a GPU: the tile rule (sdod_hypertile_grid through hypertile.grid) against its restatement in
hypertile_ref.py, the switch's refusals that need no finalized graph (the after-finalize one is in test_hypertile_gpu.py: finalize
allocates device memory), and Txt2Img's argument check."""
import pytest

import hypertile_ref as HR

# (H, W, T, level, max_depth): 72 = 2 x 36 (no divisor at 32); a rectangle; 160 x 160 down to level 3 (20 = 5 x 4); a level whose
# side the tile count does not divide (72 >> 3 = 9 against nh = 2); T >= H (one tile on that axis, and on both: untiled)
TABLE = [(72, 72, 32, 0, 0), (72, 72, 32, 1, 3), (64, 96, 32, 0, 0), (64, 96, 32, 1, 1), (64, 96, 32, 1, 0), (160, 160, 32, 3, 3),
         (160, 160, 32, 2, 3), (72, 72, 32, 3, 3), (24, 96, 32, 0, 0), (24, 24, 32, 0, 0), (64, 64, 64, 0, 0), (16, 24, 8, 1, 1),
         (96, 96, 48, 0, 0), (40, 56, 8, 2, 3)]


@pytest.mark.parametrize('args', TABLE, ids=lambda a: '-'.join(map(str, a)))
def test_grid_follows_the_rule(args):
    from sdod.amd import hypertile
    assert hypertile.grid(*args) == HR.grid(*args)


def test_grid_known_values():
    from sdod.amd import hypertile
    assert hypertile.grid(72, 72, 32, 0, 0) == (36, 36)
    assert hypertile.grid(64, 96, 32, 0, 0) == (32, 32)
    assert hypertile.grid(160, 160, 32, 3, 3) == (4, 4)
    assert hypertile.grid(72, 72, 32, 3, 3) is None and hypertile.grid(24, 24, 32, 0, 0) is None
    with pytest.raises(Exception, match='tile must be >= 8'):
        hypertile.grid(64, 64, 4, 0, 0)


def test_switch_refusals():
    from sdod.amd import engine as E
    cfg = E.sd14_config(16, 16)
    E.UNet(cfg, 2).enable_hypertile(8, 1)
    for g in (E.Temb(cfg, 2), E.VaeDecoder(cfg, 1)):
        with pytest.raises(Exception, match='UNET and CONTROLNET'):
            g.enable_hypertile(8, 0)
    with pytest.raises(Exception, match='tile must be >= 8'):
        E.UNet(cfg, 2).enable_hypertile(7, 0)
    for depth in (-1, 4):
        with pytest.raises(Exception, match='max_depth'):
            E.UNet(cfg, 2).enable_hypertile(8, depth)


@pytest.mark.parametrize('bad', [4, 0, -8, 8.0, True, (8,), (8, 4), (8, -1), (8, 1, 1), 'auto', (8.0, 0)])
def test_argument_check_refuses(bad):
    from sdod.amd import hypertile
    with pytest.raises(ValueError, match='hypertile'):
        hypertile.hypertile_check(bad)


def test_argument_check_accepts():
    from sdod.amd import hypertile
    assert hypertile.hypertile_check(None) is None and hypertile.hypertile_check(False) is None
    assert hypertile.hypertile_check(32) == (32, 0) and hypertile.hypertile_check((8, 3)) == (8, 3) and hypertile.hypertile_check([16, 1]) == (16, 1)
