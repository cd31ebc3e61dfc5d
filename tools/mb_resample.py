"""asr_resample at a training shape: 32 utterances of 16 s at 16 kHz, speed factors cycling over {0.9, 1.0, 1.1} and once all 0.997 (the
1000-phase table).  Prints medians over repeated rounds (HIP events) of
  * the launch alone (plan, table and output already on the device), with the bytes it reads plus writes over that time as a share of
    the 6.3 TB/s a streaming kernel achieves on the MI355X -- the rounds rotate over enough copies of the batch to exceed the 256 MiB
    Infinity Cache, so the bytes come from HBM;
  * ops.resample as the front end calls it (host-side plan, two small uploads, the launch);
  * ops.augment_wave (asr_augment_wave) on the same batch, with tempo / gain drawn from the full ranges;
  * utils.audio.gpu_front_end on the same batch without and with the speed column.
Recognition quality and a real corpus are not measured here.
usage: python tools/mb_resample.py [rounds]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "end2end-asr-pytorch_amd"))
from asr_hip import lib as L  # noqa: E402
from asr_hip import ops  # noqa: E402
from utils.audio import device_resample_tables, gpu_front_end, speed_length, speed_ratio, tempo_length  # noqa: E402

D = torch.device("cuda:0")
SR, B, SECS = 16000, 32, 16
HBM_ACHIEVABLE = 6.3e12
COPIES = 6


def median_ms(fn, rounds, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
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


def fmt(t):
    return "%.4f ms (min %.4f max %.4f)" % t


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    n = SECS * SR
    wavs = [torch.from_numpy((rng.randn(B, n) * 0.1).astype(np.float32)).to(D) for _ in range(COPIES)]
    lens = torch.full((B,), n, dtype=torch.int32)
    lens_d = lens.to(D)
    for name, ps in (("factors cycling over 0.9 / 1.0 / 1.1", [(900, 1000, 1100)[b % 3] for b in range(B)]), ("all 0.997", [997] * B)):
        live = sorted(set(p for p in ps if p != 1000))
        table, index = device_resample_tables(live, D)
        n_out = [speed_length(n, p) for p in ps]
        plan = torch.tensor([(1, 1, 1, 0, n, 0, 0, 0) if p == 1000 else speed_ratio(p) + index[p] + (m, 0, 0, 0) for p, m in zip(ps, n_out)],
                            dtype=torch.int32).to(D)
        cols = max(n_out)
        outs = [torch.empty((B, cols), device=D, dtype=torch.float32) for _ in range(COPIES)]
        turn = [0]

        def launch():
            k = turn[0] = (turn[0] + 1) % COPIES
            L.call("asr_resample", L.ptr(wavs[k]), n, L.ptr(lens_d), L.ptr(plan), L.ptr(table), table.numel(), L.ptr(outs[k]), cols, cols, B,
                   L.stream())

        def whole():
            k = turn[0] = (turn[0] + 1) % COPIES
            return ops.resample(wavs[k], lens, ps)

        t = median_ms(launch, rounds)
        moved = 4 * (B * n + B * cols)                   # every input sample once, every output column once (zero tails included)
        print("B=%d x %d s, %s (table %.2f KB):" % (B, SECS, name, table.numel() * 4 / 1024.0))
        print("  asr_resample launch      %s; %.1f MB read + written = %.2f TB/s = %.0f %% of the achievable %.1f TB/s"
              % (fmt(t), moved / 1e6, moved / (t[0] * 1e-3) / 1e12, 100 * moved / (t[0] * 1e-3) / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12))
        print("  ops.resample (whole)     %s" % fmt(median_ms(whole, rounds)))
        tempos = [float("%.3f" % rng.uniform(0.85, 1.15)) for _ in range(B)]
        gains = [float("%.3f" % rng.uniform(-6, 8)) for _ in range(B)]
        params = torch.tensor([(t_, g, -1, 0.0, 0.0) for t_, g in zip(tempos, gains)], dtype=torch.float64)
        print("  ops.augment_wave         %s" % fmt(median_ms(lambda: ops.augment_wave(wavs[0], lens, params, None, sample_rate=SR), rounds)))
        six = torch.tensor([(n, t_, g, -1, 0.0, 0.0) for t_, g in zip(tempos, gains)], dtype=torch.float64)
        seven = torch.cat([six, torch.tensor(ps, dtype=torch.float64)[:, None]], dim=1)
        size6 = torch.tensor([tempo_length(n, t_) for t_ in tempos], dtype=torch.int32)
        size7 = torch.tensor([tempo_length(m, t_) for m, t_ in zip(n_out, tempos)], dtype=torch.int32)
        src = wavs[0][:, None, None, :]
        t6 = median_ms(lambda: gpu_front_end(src, size6, aug=six), rounds, inner=3)
        t7 = median_ms(lambda: gpu_front_end(src, size7, aug=seven), rounds, inner=3)
        print("  gpu_front_end, 6 columns %s" % fmt(t6))
        print("  gpu_front_end, 7 columns %s; the resample launch is %.1f %% of it" % (fmt(t7), 100 * t[0] / t7[0]))


if __name__ == "__main__":
    main()
