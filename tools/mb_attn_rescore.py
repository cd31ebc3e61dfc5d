"""Attention rescoring of the CTC n-best at the benchmark vocabulary: what the scorer, the decoder pass and the
decoding mode cost.  B 32, T' 75, V 4364, the benchmark model in bf16 with a randomly initialised CTC head.

1. ops.seq_logprob alone (csrc/seq_logprob.hip, both launches), in one process: the B W (n + 1) scored rows of W 8 / 16 hypotheses of
   n 20 / 60 labels, V 4364 in the 4416-wide buffer the vocabulary projection writes.  HIP events, medians of 7 rounds of 200 calls after
   warm-up; bytes per second = M V 4 bytes over the time, beside the 6.29 TB/s a float4 copy reaches on this chip.
2. Decoder.score_hypotheses in the same process, same W and n: the folded pass (cross-attention K | V on the B utterances) against the
   same method on the repeat_interleave'd encoder output with one hypothesis per row (K | V on B W copies).  A call ends in its
   device-to-host copy: wall-clock medians of 20 calls after 3 warm-up calls, the two alternating.
3. Transformer.evaluate on ONE batch (300 input frames = T' 75), each mode in a fresh process of its own, the modes alternating, wall-clock
   medians of 3 calls after a warm-up call, two processes per mode: ctc_beam with W 8 and lambda 0 (the plain CTC search), lambda 0.3 (rescored), W 16 with
   lambda 0.3, the 300-step greedy decoder, and --beam-search at W 8.  A random head's hypotheses are as long as the frames allow.
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_attn_rescore.py [rounds] [--no-evaluate]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, LD, WIDTHS, LABELS = 32, 4364, 4416, (8, 16), (20, 60)
CALLS, LIMIT_S = 200, 240
EVAL_T_SRC, EVAL_PROCESSES = 300, 2
EVAL_MODES = ("ctc_w8", "rescore_w8", "rescore_w16", "greedy", "beam_w8")
HBM_COPY_TBS = 6.29          # float4 copy, MI355X


def _paths():
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)


def timed(torch, fn, rounds):
    """Microseconds per call: `rounds` HIP-event brackets around CALLS calls each, after 10 warm-up calls."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return times


def _model(torch, precision="bf16"):
    import bench
    from utils import constant
    from utils.functions import init_transformer_model
    flags = bench.MODEL_FLAGS + ["--dropout", "0", "--precision", precision, "--cuda", "--batch-size", str(B), "--ctc-weight", "0.3",
                                 "--tgt-max-len", "301", "--src-max-len", str(EVAL_T_SRC)]
    args = constant.parse(flags)
    l2i, i2l = bench.labels(V)
    torch.manual_seed(123456)
    return bench, init_transformer_model(args, l2i, i2l).cuda().eval()


def measure(rounds):
    import numpy as np
    import torch
    _paths()
    from asr_hip import ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    for W in WIDTHS:
        for n in LABELS:
            R, M = B * W, B * W * (n + 1)
            g = torch.Generator().manual_seed(W * 100 + n)
            wide = torch.randn(M, LD, generator=g).to(dev)
            tgt = torch.randint(0, V, (M,), generator=g).to(dev)
            off = torch.arange(0, M + 1, n + 1, dtype=torch.int32).to(dev)
            logits = wide[:, :V]
            out = ops.seq_logprob(logits, tgt, off)
            assert torch.isfinite(out["score"]).all() and out["score"].numel() == R
            times = timed(torch, lambda: ops.seq_logprob(logits, tgt, off), rounds)
            med = float(np.median(times))
            tbs = M * V * 4 / (med * 1e-6) / 1e12
            print("seq_logprob W %2d n %2d: M %6d rows, R %3d  median %7.1f us per call (min %.1f max %.1f, %d x %d calls)  %.2f TB/s of logits "
                  "= %.0f%% of the %.2f TB/s float4 copy" % (W, n, M, R, med, min(times), max(times), rounds, CALLS, tbs,
                                                              100 * tbs / HBM_COPY_TBS, HBM_COPY_TBS))
    _, model = _model(torch)
    dec = model.decoder
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(B, EVAL_T_SRC // 4, 512, generator=g).to(dev).to(ops.compute_dtype())
    for W in WIDTHS:
        enc_rep = enc.repeat_interleave(W, dim=0).contiguous()
        for n in LABELS:
            hyps = [[torch.randint(3, V, (n,), generator=g).tolist() for _ in range(W)] for _ in range(B)]
            flat = [[y] for hs in hyps for y in hs]
            folded = lambda: dec.score_hypotheses(enc, hyps)
            repeated = lambda: dec.score_hypotheses(enc_rep, flat)
            a, b = folded(), repeated()
            worst = max(abs(x - y) for xs, ys in zip(a, [[s[0] for s in b[i * W:(i + 1) * W]] for i in range(B)]) for x, y in zip(xs, ys))
            t = {"folded": [], "repeated": []}
            for i in range(23):
                for name, fn in (("folded", folded), ("repeated", repeated)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if i >= 3:
                        t[name].append((time.perf_counter() - t0) * 1e3)
            print("score_hypotheses W %2d n %2d (%5d scored rows): folded median %6.2f ms (min %.2f), on the repeated encoder output %6.2f ms "
                  "(min %.2f); largest score difference between the two %.3f of scores about %.0f"
                  % (W, n, B * W * (n + 1), float(np.median(t["folded"])), min(t["folded"]), float(np.median(t["repeated"])),
                     min(t["repeated"]), worst, abs(a[0][0])))


def evaluate_once(mode):
    import numpy as np
    import torch
    _paths()
    torch.cuda.set_device(0)
    bench, model = _model(torch)
    src, src_len, tgt = bench.synthetic_batch(B, torch, EVAL_T_SRC, 100, V)
    src, tgt = src.cuda(), tgt.cuda()
    kw = {"ctc_w8": dict(ctc_beam=True, beam_width=8), "rescore_w8": dict(ctc_beam=True, beam_width=8, attention_rescoring_weight=0.3),
          "rescore_w16": dict(ctc_beam=True, beam_width=16, attention_rescoring_weight=0.3), "greedy": {},
          "beam_w8": dict(beam_search=True, beam_width=8, beam_nbest=1)}[mode]
    times = []
    with torch.no_grad():
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, hyps, _ = model.evaluate(src, src_len, tgt, **kw)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    assert len(hyps) == B
    print("evaluate %-11s B %d T' %d: median %8.1f ms per batch over 3 calls after a warm-up call of %.1f ms (%s); hypotheses of %d..%d labels"
          % (mode, B, EVAL_T_SRC // 4, float(np.median(times[1:])), times[0], ", ".join("%.1f" % t for t in times[1:]),
             min(len(h) for h in hyps), max(len(h) for h in hyps)))


def _child(*argv):
    # (a fresh child: this process never touches the device)
    return subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__)] + list(argv)).returncode


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
    elif len(sys.argv) > 2 and sys.argv[1] == "--child-evaluate":
        evaluate_once(sys.argv[2])
    else:
        argv = [a for a in sys.argv[1:] if a != "--no-evaluate"]
        rc = _child("--child", argv[0] if argv else "7")
        if rc == 0 and "--no-evaluate" not in sys.argv:
            for _ in range(EVAL_PROCESSES):
                for mode in EVAL_MODES:
                    rc = _child("--child-evaluate", mode)
                    if rc != 0:              # a fault, a hang or a failure: nothing more is started on the device
                        sys.exit(rc)
        sys.exit(rc)
