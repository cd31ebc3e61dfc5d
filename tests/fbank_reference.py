"""Float64 restatement of the log-mel filterbank features, written from the definition with a dense (M, K) matrix
and sharing no code with utils/audio.py:

  spectrum  n_fft = win = sr * window_size, hop = sr * window_stride, symmetric window, centred reflect-padded frames;
            P[k] = re^2 + im^2 at the K = n_fft/2 + 1 bins f_k = k sr / n_fft;
  mel       HTK: mel(f) = 2595 log10(1 + f/700); M + 2 points equally spaced in mel between mel(f_min) and mel(f_max), mapped back to
            Hz as c_0 .. c_{M+1};
  weights   w[m][k] = max(0, min((f_k - c_m) / (c_{m+1} - c_m), (c_{m+2} - f_k) / (c_{m+2} - c_{m+1}))), no area normalisation, float64
            rounded to float32 (the stored precision is part of the definition);
  features  x[m][t] = log(max(sum_k w[m][k] P[k][t], 1e-10)), then (x - mean) / unbiased std over the utterance's M x n_frames values.
"""
import math

import numpy as np

FLOOR = 1e-10


def hz_to_mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


def centres(M, sample_rate, f_min, f_max=None):
    """c_0 .. c_{M+1} in Hz."""
    f_max = sample_rate / 2.0 if f_max is None else f_max
    lo, hi = hz_to_mel(f_min), hz_to_mel(f_max)
    c = [mel_to_hz(lo + (hi - lo) * i / (M + 1)) for i in range(M + 2)]
    c[0], c[-1] = float(f_min), float(f_max)          # mel_to_hz(hz_to_mel(f)) = f: the end points are f_min and f_max themselves
    return c


def dense_bank(M, n_fft, sample_rate, f_min, f_max=None):
    """(M, K) float64 array holding the float32-rounded weights."""
    K = n_fft // 2 + 1
    c = centres(M, sample_rate, f_min, f_max)
    w = np.zeros((M, K), dtype=np.float64)
    for m in range(M):
        for k in range(K):
            f = k * sample_rate / n_fft
            w[m, k] = max(0.0, min((f - c[m]) / (c[m + 1] - c[m]), (c[m + 2] - f) / (c[m + 2] - c[m + 1])))
    return w.astype(np.float32).astype(np.float64)


def densify(first, count, weights, K):
    """The dense (M, K) float64 matrix of a sparse bank."""
    w = np.zeros((len(first), K), dtype=np.float64)
    o = 0
    for m, (k0, n) in enumerate(zip(first, count)):
        w[m, k0:k0 + n] = np.asarray(weights[o:o + n], dtype=np.float64)
        o += n
    assert o == len(weights)
    return w


def symmetric_window(name, n):
    k = np.arange(n, dtype=np.float64)
    a = 2.0 * np.pi * k / (n - 1)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if name == "hann":
        return 0.5 - 0.5 * np.cos(a)
    raise ValueError(name)


def power_frames(y, n_fft, hop, window="hamming"):
    """(frames, K) float64 power spectrum of the float32 waveform y: a direct DFT as a matrix product, no FFT library.  The window is the
    float32-rounded one the front ends store."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    if y.size < 2:
        y = np.concatenate([y, np.zeros(2 - y.size)])
    pad = n_fft // 2
    if y.size > pad:
        left = y[1:pad + 1][::-1]
        right = y[-pad - 1:-1][::-1]
        yp = np.concatenate([left, y, right])
    else:
        yp = np.concatenate([np.zeros(pad), y, np.zeros(pad)])
    n_frames = 1 + (yp.size - n_fft) // hop
    win = symmetric_window(window, n_fft).astype(np.float32).astype(np.float64)
    frames = np.stack([yp[t * hop:t * hop + n_fft] * win for t in range(n_frames)])
    K = n_fft // 2 + 1
    ang = 2.0 * np.pi * np.outer(np.arange(n_fft), np.arange(K)) / n_fft
    re, im = frames @ np.cos(ang), -(frames @ np.sin(ang))
    return re * re + im * im


def log_mel(power, w, floor=FLOOR):
    """(M, frames) float64 raw features of a (frames, K) power spectrum through the dense bank w (M, K)."""
    return np.log(np.maximum(w @ power.T, floor))


def normalise(x):
    return (x - x.mean()) / x.std(ddof=1)


def features(y, sample_rate=16000, window_size=0.02, window_stride=0.01, M=80, f_min=20.0, normalize=True, window="hamming"):
    n_fft, hop = int(sample_rate * window_size), int(sample_rate * window_stride)
    x = log_mel(power_frames(y, n_fft, hop, window), dense_bank(M, n_fft, sample_rate, f_min))
    return normalise(x) if normalize else x


def finish(reim, lens, w, hop, Tmax, floor=FLOOR):
    """What asr_fbank_finish(normalize = 0) computes from (B * Tmax, ld) re | im rows: (raw (B, M, Tmax) float64, zero from each
    utterance's 1 + max(len, 2) // hop frames on; the frame counts; the per-utterance sums of the valid raw values)."""
    reim = np.asarray(reim, dtype=np.float64)
    M, K = w.shape
    B = len(lens)
    raw = np.zeros((B, M, Tmax))
    nfr = [min(1 + max(int(n), 2) // hop, Tmax) for n in lens]
    for b in range(B):
        rows = reim[b * Tmax:b * Tmax + nfr[b]]
        raw[b, :, :nfr[b]] = log_mel(rows[:, :K] ** 2 + rows[:, K:2 * K] ** 2, w, floor)
    return raw, nfr, [raw[b].sum() for b in range(B)]
