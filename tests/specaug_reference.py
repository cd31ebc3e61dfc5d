"""SpecAugment as DESIGN.md section 7 defines it, in numpy float64: the reference of tests/test_specaug_host.py and
tests/test_gpu_specaug.py.  One row of parameters per utterance: {n, c, w, nF, nT, 0, 0, 0, 8 x (f0, fw), 8 x (t0, tw)}."""
import numpy as np

PARAMS, MAX_MASKS = 40, 8


def row(n, c=0, w=0, fmasks=(), tmasks=()):
    """A parameter row from python values: fmasks / tmasks are lists of (start, width)."""
    assert len(fmasks) <= MAX_MASKS and len(tmasks) <= MAX_MASKS
    r = [0] * PARAMS
    r[0], r[1], r[2], r[3], r[4] = n, c, w, len(fmasks), len(tmasks)
    for k, (a, b) in enumerate(fmasks):
        r[8 + 2 * k], r[9 + 2 * k] = a, b
    for k, (a, b) in enumerate(tmasks):
        r[8 + 2 * MAX_MASKS + 2 * k], r[9 + 2 * MAX_MASKS + 2 * k] = a, b
    return r


def warp_source(n, c, w):
    """(i0, i1, r, den) per output frame t < n, in python integers; the identity when the warp does not apply."""
    t = np.arange(n, dtype=np.int64)
    if not (0 < c < n and 0 <= w < n):
        return t, t.copy(), np.zeros(n, np.int64), np.ones(n, np.int64)
    left = t < w
    u = np.where(left, t, t - w)
    s = np.where(left, c, n - c)
    d = np.where(left, w, n - w)
    base = np.where(left, 0, c)
    num, den = (2 * u + 1) * s - d, 2 * d
    neg = num < 0
    i0 = np.where(neg, 0, num // den)
    r = np.where(neg, 0, num % den)
    i1 = np.minimum(i0 + 1, s - 1)
    return base + i0, base + i1, r, den


def warp(x, n, c, w):
    """x (F, >= n) -> float64 (F, n): the time warp c -> w of the first n frames."""
    x = np.asarray(x)[:, :n].astype(np.float64)
    i0, i1, r, den = warp_source(n, c, w)
    frac = r.astype(np.float64) / den.astype(np.float64)
    x0, x1 = x[:, i0], x[:, i1]
    return np.where(r == 0, x0, frac * (x1 - x0) + x0)


def spec_augment(x, params, t_out=None):
    """x (F, T) of one utterance, params its row -> float64 (F, t_out): warp, masks, zeros from frame n on."""
    x = np.asarray(x)
    F, T = x.shape
    t_out = T if t_out is None else t_out
    p = [int(v) for v in params]
    n = min(max(p[0], 0), t_out)
    y = np.zeros((F, t_out), np.float64)
    y[:, :n] = warp(x, n, p[1], p[2])
    for k in range(p[3]):
        f0, fw = p[8 + 2 * k], p[9 + 2 * k]
        y[max(f0, 0):max(f0 + fw, 0)] = 0.0
    for k in range(p[4]):
        t0, tw = p[8 + 2 * MAX_MASKS + 2 * k], p[9 + 2 * MAX_MASKS + 2 * k]
        y[:, max(t0, 0):max(t0 + tw, 0)] = 0.0
    return y


def spec_augment_batch(x, params, t_out=None):
    """x (B, F, T) -> float64 (B, F, t_out)."""
    return np.stack([spec_augment(x[b], params[b], t_out) for b in range(len(x))])
