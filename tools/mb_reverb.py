"""asr_reverb alone at a training shape: 32 utterances of 8 s at 16 kHz (n = 128 000), responses of L = 1000 / 4000 / 8000 taps, once
with every row reverberated and once with every second row copied (--rir-prob 0.5).  Prints, per case, the median over repeated rounds
(HIP events around windows of about 0.1 s of back-to-back launches, after warm-up) of the launch with everything already on the device, and the achieved
fraction of the fp32 FMA peak: 2 sum_rows n L floating-point operations over the time, against 157.3 TF/s (the first L outputs of a
row have fewer terms, k <= m: 3 % of the count at L = 8000).
Recognition quality and a real corpus are not measured here.
usage: python tools/mb_reverb.py [rounds]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "end2end-asr-pytorch_amd"))
from asr_hip import lib as L  # noqa: E402
from asr_hip import ops  # noqa: E402
from utils.audio import RirBank  # noqa: E402

D = torch.device("cuda:0")
B, N = 32, 128000
PEAK = 157.3e12


def median_ms(fn, rounds):
    """Median, min and max over `rounds` windows of `inner` back-to-back launches; inner is sized from a first warm window so that a
    window lasts about 0.1 s."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    torch.cuda.synchronize()
    inner = int(min(max(100.0 / max(e0.elapsed_time(e1) / 3, 1e-3), 5), 1000))
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    wav = torch.from_numpy((rng.randn(B, N) * 0.1).astype(np.float32)).to(D)
    lens = torch.full((B,), N, dtype=torch.int32, device=D)
    out = torch.empty_like(wav)
    print("asr_reverb, B = %d rows of n = %d samples (tile %d, tap chunk %d); peak %.1f TF/s" % (B, N, ops.REVERB_TILE, ops.REVERB_CHUNK, PEAK / 1e12))
    print("%6s %12s %30s %10s %10s" % ("L", "rows", "ms: median (min .. max)", "TF/s", "of peak"))
    for taps in (1000, 4000, 8000):
        h = rng.randn(taps) * np.exp(-np.arange(taps) / (taps / 5.0))
        bank = RirBank.from_arrays([(h / np.sqrt(np.sum(h * h))).astype(np.float32)], D)
        for name, idx in (("all", [0] * B), ("every 2nd", [0 if b % 2 == 0 else -1 for b in range(B)])):
            rir = torch.tensor(idx, dtype=torch.int32, device=D)

            def launch():
                L.call("asr_reverb", L.ptr(wav), N, L.ptr(lens), L.ptr(rir), L.ptr(bank.data), bank.data.numel(), L.ptr(bank.offsets),
                       L.ptr(bank.lens), 1, L.ptr(out), N, N, B, L.stream())

            t = median_ms(launch, rounds)
            live = sum(1 for r in idx if r >= 0)
            terms = live * N * taps
            rate = 2.0 * terms / (t[0] * 1e-3)
            print("%6d %12s %30s %10.1f %9.1f%%" % (taps, name, "%.3f (%.3f .. %.3f)" % t, rate / 1e12, 100 * rate / PEAK))
    got = ops.reverb(wav[:2, :6000].contiguous(), [6000, 6000], [0, -1], bank)   # a last look that the launch computes something
    assert torch.isfinite(got).all() and torch.equal(got[1], wav[1, :6000])


if __name__ == "__main__":
    main()
