"""--features fbank at the training shape, 32 utterances of 8 s (800 frames), against the linear features in the same process:
  first   the first pass alone on one (32 * 800, 324) re | im buffer: fbank_logmel_kernel (asr_fbank_finish, normalize = 0: 80 x 800
          features per utterance) against spect_logmag_kernel (asr_spect_finish, normalize = 0: 161 x 800), device-event medians after
          warm-up, the two alternating; kernel times proper come from `rocprofv3 --kernel-trace --stats -- python tools/mb_fbank.py
          first 3`;
  step    the trainer's step body (tools/trainer_rate.py's loop, batch resident on the device, train.py's default --graph-buckets) on
          configs[1] with (32, 1, 80, 800) input against (32, 1, 161, 800), the two models alternating in rounds.
usage: python tools/mb_fbank.py first|step [reps]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
sys.path.insert(0, ROOT)
from asr_hip import lib as L  # noqa: E402
from asr_hip import ops  # noqa: E402

B, T, N_FFT, HOP, SR = 32, 800, 320, 160, 16000


def median_ms(fn, reps, inner=20):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def first_pass(reps):
    from utils.audio import mel_filterbank
    K = N_FFT // 2 + 1
    ld = (2 * K + 3) // 4 * 4
    reim = torch.randn(B * T, ld, device="cuda") * 3
    lengths = torch.full((B,), T * HOP - 1, dtype=torch.int32, device="cuda")
    bank = ops.fbank_upload(mel_filterbank(80, N_FFT, SR, 20.0), "cuda")
    spect = torch.empty((B, 1, K, T), device="cuda")
    feat = torch.empty((B, 1, 80, T), device="cuda")
    sc = torch.zeros((2, B), device="cuda")

    def linear():
        L.call("asr_spect_finish", L.ptr(reim), ld, L.ptr(lengths), L.ptr(spect), L.ptr(sc[0]), L.ptr(sc[1]), B, K, T, HOP, 0, L.stream())

    def mel():
        L.call("asr_fbank_finish", L.ptr(reim), ld, L.ptr(lengths), L.ptr(feat), L.ptr(sc[0]), L.ptr(sc[1]), B, K, 80, T, HOP, 0,
               L.ptr(bank.first), L.ptr(bank.count), L.ptr(bank.weights), bank.weights.numel(), ops.FBANK_FLOOR, L.stream())

    for _ in range(10):
        linear()
        mel()
    torch.cuda.synchronize()
    read, w_lin, w_mel = B * T * 2 * K * 4, B * T * K * 4, B * T * 80 * 4
    for rnd in range(3):
        for name, fn, wr in (("spect_logmag_kernel", linear, w_lin), ("fbank_logmel_kernel", mel, w_mel)):
            m = median_ms(fn, reps)
            print("round %d %-20s %.1f us per launch (min %.1f max %.1f): %.1f MB read + %.1f MB written = %.0f GB/s"
                  % (rnd, name, m[0] * 1e3, m[1] * 1e3, m[2] * 1e3, read / 1e6, wr / 1e6, (read + wr) / m[0] / 1e6))


def step_pair(steps):
    import bench as Bn
    from trainer.asr.trainer import Trainer
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    import train
    l2i, i2l = Bn.labels(Bn.V)
    base = Bn.MODEL_FLAGS + ["--dropout", "0.1", "--precision", "bf16", "--cuda", "--batch-size", str(B)]
    runs = {}
    for name, extra, bins in (("161 linear bins", [], 161), ("80 mel bins", ["--features", "fbank"], 80)):
        args = constant.parse(base + extra)
        train.resolve_graph_buckets(args, constant.explicit)
        model = init_transformer_model(args, l2i, i2l).cuda().train()
        opt = init_optimizer(args, model, "noam")
        _, src_len, tgt = Bn.synthetic_batch(B, torch)
        src = torch.randn(B, 1, bins, Bn.T_SRC, generator=torch.Generator().manual_seed(1))
        batch = (src.cuda(), tgt.cuda(), torch.ones(B), src_len, torch.full((B,), tgt.shape[1], dtype=torch.int32))
        runs[name] = (args, model, opt, batch, Trainer())

    def run(name, n):
        args, model, opt, batch, tr = runs[name]
        constant.set_args(args)
        torch.cuda.synchronize()
        t0 = time.time()
        pending = None
        for _ in range(n):
            r = tr._run_batch(model, batch, 0.1, "ce", i2l, opt)
            if pending is not None:
                last = pending.result()
            pending = r if hasattr(r, "result") else None
            if pending is None:
                last = r
        if pending is not None:
            last = pending.result()
        torch.cuda.synchronize()
        return (time.time() - t0) / n * 1e3, last[0]

    for name in runs:
        run(name, 8)
    times = {name: [] for name in runs}
    for rnd in range(5):
        for name in runs:
            ms, loss = run(name, steps)
            times[name].append(ms)
            print("round %d %-16s dim_input %d graph-buckets %d: %.3f ms/step (loss %.4f)"
                  % (rnd, name, runs[name][0].dim_input, runs[name][0].graph_buckets, ms, loss))
    for name, v in times.items():
        print("%-16s median %.3f ms/step (min %.3f max %.3f)" % (name, np.median(v), min(v), max(v)))


if __name__ == "__main__":
    torch.cuda.set_device(0)
    what = sys.argv[1] if len(sys.argv) > 1 else "first"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else None
    if what == "first":
        first_pass(n or 20)
    else:
        step_pair(n or 40)
