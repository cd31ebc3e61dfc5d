"""Restatement of the speed perturbation's definition in numpy, independent of utils/audio.py and of the kernel:
the reduced ratio and the output length, the Hann-windowed sinc and its tap table in float64, the integer position arithmetic, the
resampled signal in float64, and a float32 form that adds in the kernel's order (one fused multiply-add per tap, ascending q, from
+0.0) for data on which every such step is exact."""
import math

import numpy as np

Z, ROLLOFF_NUM, ROLLOFF_DEN = 6, 99, 100


def ratio(p):
    g = math.gcd(int(p), 1000)
    return int(p) // g, 1000 // g


def length(n, p):
    num, den = ratio(p)
    return (2 * n * den + num) // (2 * num)


def half_width(num, den):
    """R = ceil(Z / c), c = 0.99 min(1, den / num), in integers."""
    a, b = Z * ROLLOFF_DEN * max(num, den), ROLLOFF_NUM * den
    return (a + b - 1) // b


def kernel(t, num, den):
    """h(t) = c sinc(c t) cos^2(pi c t / (2 Z)) inside |c t| < Z, float64."""
    c = (ROLLOFF_NUM / ROLLOFF_DEN) * min(1.0, den / num)
    t = np.asarray(t, dtype=np.float64)
    x = c * t
    s = np.ones_like(x)
    nz = x != 0
    s[nz] = np.sin(np.pi * x[nz]) / (np.pi * x[nz])
    h = c * s * np.cos(np.pi * x / (2.0 * Z)) ** 2
    return np.where(np.abs(x) < Z, h, 0.0)


def table64(p):
    """(R, H (den, 2R) float64): H[phi][q] = h(phi / den - (q - R + 1))."""
    num, den = ratio(p)
    R = half_width(num, den)
    numer = np.array([[phi - (q - R + 1) * den for q in range(2 * R)] for phi in range(den)], dtype=np.int64)
    return R, kernel(numer / float(den), num, den)


def positions(n_out, num, den):
    """(i_m, phi_m) of outputs 0 .. n_out - 1 in Python integers."""
    return [(m * num) // den for m in range(n_out)], [(m * num) % den for m in range(n_out)]


def _gather(x, i, R):
    """X[m][q] = x[i_m + q - R + 1], 0 outside [0, n)."""
    x = np.asarray(x)
    idx = np.asarray(i, dtype=np.int64)[:, None] + np.arange(2 * R, dtype=np.int64)[None, :] - R + 1
    ok = (idx >= 0) & (idx < x.size)
    X = np.zeros(idx.shape, dtype=x.dtype)
    X[ok] = x[idx[ok]]
    return X


def resample64(x, num, den, R, H, n_out):
    """The definition in float64 with table H (any dtype, taken as the values it holds): (y (n_out), sum_q |H x| per output)."""
    if n_out == 0:
        return np.zeros(0), np.zeros(0)
    i, phi = positions(n_out, num, den)
    prod = np.asarray(H, dtype=np.float64)[np.asarray(phi)] * _gather(np.asarray(x, dtype=np.float64), i, R)
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def resample32_exact(x, num, den, R, H, n_out):
    """float32 in the kernel's order: acc = fma(H[phi][q], x[..], acc) for q = 0 .. 2R - 1 from +0.0.  Each step is evaluated in
    float64 and rounded to float32: the fused result whenever the float64 product-and-sum is exact, which holds for the small dyadic
    tables and integer samples this is meant for (asserted)."""
    if n_out == 0:
        return np.zeros(0, dtype=np.float32)
    i, phi = positions(n_out, num, den)
    Hm = np.asarray(H, dtype=np.float32)[np.asarray(phi)].astype(np.float64)
    X = _gather(np.asarray(x, dtype=np.float32), i, R).astype(np.float64)
    acc = np.zeros(n_out, dtype=np.float32)
    for q in range(2 * R):
        s = Hm[:, q] * X[:, q] + acc.astype(np.float64)
        nxt = s.astype(np.float32)
        assert np.array_equal(nxt.astype(np.float64), s), "resample32_exact is for data whose partial sums are exact in float32"
        acc = nxt
    return acc
