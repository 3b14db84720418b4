"""sdod_sag_degrade_f32 and sdod_sag_fold_f16 (Self-Attention Guidance).

sag_degrade against restate(): reflect pad, separable 9-tap blur, nearest mask from the middle map, renoise -- in fp64.  The masses are
0.5 / 1.0 / 1.5 in a checkerboard of 8 x 8 blocks that touches every border; 1.0 exactly must count as not salient.  The bound is four
times what the SAME restatement run in fp32 on the CPU loses against fp64 (fp32 arithmetic on the fp16-rounded e_u), taken per case.
sag_fold against fp64 rounded to fp16: one fp16 ulp; s = 0 leaves every bit; g = 0 is refused."""
import numpy as np
import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu


def restate(xs, eu, mass, a, b, ss, taps, dt):
    """xs [n, c, h, w], eu [n, h, w, c], mass [n, h / 8, w / 8] -> ss * (a * D + b * e_u), every operation in dtype dt"""
    xs, e, w = xs.astype(dt), eu.transpose(0, 3, 1, 2).astype(dt), np.asarray(taps, dtype=dt)
    a, b, ss = dt(a), dt(b), dt(ss)
    x0 = (xs / ss - b * e) / a
    pad = np.pad(x0, ((0, 0), (0, 0), (4, 4), (4, 4)), mode='reflect')
    H, W = x0.shape[2:]
    rows = sum(w[k] * pad[:, :, :, k:k + W] for k in range(9))
    blur = sum(w[k] * rows[:, :, k:k + H, :] for k in range(9))
    salient = np.repeat(np.repeat(mass > 1.0, 8, axis=1), 8, axis=2)[:, None]
    return ss * (a * np.where(salient, blur, x0) + b * e)


@pytest.mark.parametrize('abs_', [(1.0, 2.5, 0.37), (0.6, 0.8, 1.0)], ids=['k', 'ddim'])
@pytest.mark.parametrize('hw', [(8, 8), (16, 24), (64, 64)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_sag_degrade(hw, abs_):
    from sdod.amd import ops
    (h, w), (a, b, ss), n, c = hw, abs_, 2, 4
    rng = np.random.default_rng(h * 100 + w)
    xs = (ss * rng.standard_normal((n, c, h, w)) * (1 + b)).astype(np.float32)
    eu = rng.standard_normal((n, h, w, c)).astype(np.float16)
    iy, ix = np.mgrid[0:h // 8, 0:w // 8]
    mass = np.stack([np.array([1.5, 1.0, 0.5], dtype=np.float32)[(iy + ix + i) % 3] for i in range(n)])   # image 0 starts salient, image 1 at 1.0
    taps = ops.sag_taps()
    ref = restate(xs, eu, mass, a, b, ss, taps, np.float64)
    bound = 4 * float(np.abs(restate(xs, eu, mass, a, b, ss, taps, np.float32) - ref).max())
    dev = AC.dev()
    out = ops.sag_degrade(torch.from_numpy(xs).to(dev), torch.from_numpy(eu).to(dev), torch.from_numpy(mass).reshape(n, -1).to(dev), a, b, ss)
    err = float(np.abs(out.double().cpu().numpy() - ref).max())
    blurred = float(np.abs(ref - ss * (xs.astype(np.float64) / ss)).max())
    print(f'sag_degrade {h}x{w} a{a} b{b} ss{ss}: err {err:.3e}, bound {bound:.3e}, moved by the blur {blurred:.3e}')
    assert 0 < bound < 1e-5 and blurred > 0.1 and err <= bound, (err, bound)


@pytest.mark.parametrize('uncond_first', [True, False])
def test_sag_fold(uncond_first):
    from sdod.amd import ops
    from sdod.amd._lib import SdodError
    gen = torch.Generator().manual_seed(5)
    pair, ed = torch.randn(4, 16, 24, 4, generator=gen).half(), torch.randn(2, 16, 24, 4, generator=gen).half()
    s, g = 0.75, 7.5
    u, cnd = (pair[:2], pair[2:]) if uncond_first else (pair[2:], pair[:2])
    want = (cnd.double() + (s / g) * (u.double() - ed.double())).half()
    dev = AC.dev()
    out = ops.sag_fold(pair.to(dev), ed.to(dev), s, g, uncond_first=uncond_first).cpu()
    ou, oc = (out[:2], out[2:]) if uncond_first else (out[2:], out[:2])
    assert torch.equal(ou, u)
    ulps = (oc.view(torch.int16).int() - want.view(torch.int16).int()).abs().max()   # (same sign wherever they differ by a step)
    print(f'sag_fold uncond_first={uncond_first}: {int(ulps)} ulp')
    assert ulps <= 1 and not torch.equal(oc, cnd)
    assert torch.equal(ops.sag_fold(pair.to(dev), ed.to(dev), 0.0, g, uncond_first=uncond_first).cpu(), pair)
    with pytest.raises(SdodError) as e:
        ops.sag_fold(pair.to(dev), ed.to(dev), s, 0.0)
    assert e.value.code == 2
