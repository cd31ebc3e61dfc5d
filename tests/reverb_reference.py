"""Restatement of the reverberation's definition in numpy, independent of utils/audio.py and of the kernel:
  prepare(h, sample_rate, max_ms)   the taps of a recorded room impulse response, float64 (the caller casts to float32);
  reverb64(x, h, n)                 y[m] = sum_{k <= min(L - 1, m)} h[k] x[m - k] for m < n in float64 over the float32 inputs, and the
                                    magnitude sum_k |h[k] x[m - k]| the fp32 error bound is stated in;
  reverb32_exact(x, h, n)           the same as float32, asserting that the data make every fp32 partial sum exact (integers whose
                                    partial sums stay below 2^24), so that any summation order gives these bits;
  bound(L, mag)                     gamma_{L+1} mag + L 2^-126: an fp32 fmaf sum of L terms in any order."""
import numpy as np


def prepare(h, sample_rate, max_ms):
    h = [float(v) for v in np.asarray(h, dtype=np.float64).reshape(-1)]
    cap = (max_ms * sample_rate) // 1000 if isinstance(max_ms, int) else int(np.floor(max_ms * sample_rate / 1000.0))
    assert cap >= 1 and len(h) > 0 and any(v != 0.0 for v in h)
    peak = max(abs(v) for v in h)
    k0 = next(k for k, v in enumerate(h) if abs(v) == peak)          # the first of equal peaks
    kept = h[k0:k0 + cap]
    last = 0
    for k, v in enumerate(kept):
        if abs(v) >= 1e-3 * peak:
            last = k
    kept = np.array(kept[:last + 1], dtype=np.float64)
    return kept / np.sqrt(np.sum(kept ** 2))


def reverb64(x, h, n=None):
    x, h = np.asarray(x), np.asarray(h)
    assert x.dtype == np.float32 and h.dtype == np.float32
    n = x.size if n is None else n
    if n == 0:
        return np.zeros(0), np.zeros(0)
    x64, h64 = x[:n].astype(np.float64), h.astype(np.float64)
    return np.convolve(x64, h64)[:n], np.convolve(np.abs(x64), np.abs(h64))[:n]


def reverb32_exact(x, h, n=None):
    y, mag = reverb64(x, h, n)
    assert (mag < 2.0 ** 24).all() and np.array_equal(np.rint(x), x) and np.array_equal(np.rint(h), h), "not exact-integer data"
    return y.astype(np.float32)


def bound(L, mag):
    u = 2.0 ** -24
    j = L + 1
    return j * u / (1.0 - j * u) * mag + L * 2.0 ** -126
