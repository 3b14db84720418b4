"""fp64 restatement of the latent resize (include/sdod_hip.h: sdod_latent_resize_f32), shared by the resize tests (not a test
module): per axis, exact rational coordinates (fractions.Fraction), weights evaluated in float64."""
from fractions import Fraction

import numpy as np

MODES = ('nearest-exact', 'bilinear', 'bicubic')
A = -0.75


def _c1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _c2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def axis_taps(mode, n_in, n_out):
    """(idx int64 [n_out, 4], w float64 [n_out, 4]); unused slots: index 0, weight 0"""
    idx = np.zeros((n_out, 4), np.int64)
    w = np.zeros((n_out, 4), np.float64)
    for d in range(n_out):
        if mode == 'nearest-exact':
            idx[d, 0] = min(((2 * d + 1) * n_in) // (2 * n_out), n_in - 1)
            w[d, 0] = 1.0
            continue
        s = Fraction((2 * d + 1) * n_in - n_out, 2 * n_out)
        if mode == 'bilinear':
            s = max(s, Fraction(0))
            i0 = s.numerator // s.denominator
            t = float(s - i0)
            idx[d, :2] = i0, min(i0 + 1, n_in - 1)
            w[d, :2] = 1.0 - t, t
        else:
            i = s.numerator // s.denominator                     # floor, also below zero
            t = float(s - i)
            idx[d] = np.clip(np.arange(i - 1, i + 3), 0, n_in - 1)
            w[d] = _c2(t + 1.0), _c1(t), _c1(1.0 - t), _c2(2.0 - t)
    return idx, w


def axis_matrix(mode, n_in, n_out):
    """float64 [n_out, n_in]: the taps scattered (clamped taps that share an index add up)"""
    idx, w = axis_taps(mode, n_in, n_out)
    m = np.zeros((n_out, n_in), np.float64)
    for d in range(n_out):
        for k in range(4):
            m[d, idx[d, k]] += w[d, k]
    return m


def resize(src, size, mode):
    """src float array [n, c, h, w] -> float64 [n, c, size[0], size[1]]"""
    src = np.asarray(src, np.float64)
    my = axis_matrix(mode, src.shape[2], size[0])
    mx = axis_matrix(mode, src.shape[3], size[1])
    return np.einsum('yh,nchw,xw->ncyx', my, src, mx)
