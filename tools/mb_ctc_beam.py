"""asr_ctc_beam_search (csrc/ctc_beam.hip) at the benchmark vocabulary, and what decoding with it costs beside the attention decoder.

1. The entry point alone, in one process: B 32, V 4364, C 16, W 8 and 16, at T' 75 and T' 400, on peaked random logits (standard
   normal plus 10 on one winner per frame: a label every fourth frame, the blank elsewhere -- a trained head's shape; full lengths).
   All three launches (row log-sum-exp, top-C, search), and beside them asr_logsoftmax_topk alone on the same B * T' rows with k = C:
   the entry point's second launch, timed through its own public entry point, so that the search's share can be told from the
   candidates'.  HIP events, medians of 7 rounds of 200 calls after warm-up.
2. Transformer.evaluate on ONE batch (B 32, 300 input frames = T' 75, the benchmark model in bf16 with a randomly initialised CTC head):
   ctc_beam=True (W 8) against the default, the 300-step greedy attention decoder -- code this feature does not touch --, each in a
   fresh process of its own, the two alternating, wall-clock medians of 3 calls after a warm-up call (evaluate ends in a device-to-host
   copy).  A random head's flat posteriors take the kernel's dependent-read path more often than a trained head's would.
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_ctc_beam.py [rounds] [--no-evaluate]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, C, WIDTHS, LENGTHS = 32, 4364, 16, (8, 16), (75, 400)
CALLS, LIMIT_S = 200, 240
EVAL_W, EVAL_T_SRC, EVAL_PROCESSES = 8, 300, 3


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


def measure(rounds):
    import numpy as np
    import torch
    _paths()
    from asr_hip import lib as Lb
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    h = Lb.load()
    for T in LENGTHS:
        g = torch.Generator().manual_seed(T)
        logits = torch.randn(B, T, V, generator=g)
        win = torch.zeros(B, T, dtype=torch.int64)
        win[:, ::4] = torch.randint(3, V, (B, (T + 3) // 4), generator=g)
        logits.scatter_add_(2, win.unsqueeze(2), torch.full((B, T, 1), 10.0))
        logits = logits.to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        vals, idx = torch.empty((B * T, C), device=dev), torch.empty((B * T, C), dtype=torch.int64, device=dev)

        def topk():
            Lb.call("asr_logsoftmax_topk", Lb.ptr(logits), V, B * T, V, C, Lb.ptr(vals), Lb.ptr(idx), Lb.stream())

        print("B %d V %d C %d      T' %3d asr_logsoftmax_topk (%d rows) median %7.1f us per call"
              % (B, V, C, T, B * T, float(np.median(timed(torch, topk, rounds)))))
        for W in WIDTHS:
            n = h.asr_ctc_beam_workspace(B, T, W, C)
            ws = torch.empty(n, device=dev)
            ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
            lens, scores = torch.empty((B, W), dtype=torch.int32, device=dev), torch.empty((B, W), device=dev)

            def run():
                Lb.call("asr_ctc_beam_search", Lb.ptr(logits), V, Lb.ptr(il), B, T, V, W, C, W, 0, Lb.ptr(ws), n, Lb.ptr(ids), Lb.ptr(lens),
                        Lb.ptr(scores), Lb.stream())

            times = timed(torch, run, rounds)
            assert torch.isfinite(scores[:, 0]).all() and int(lens[:, 0].min()) > 0
            print("B %d V %d C %d W %2d T' %3d asr_ctc_beam_search median %7.1f us per call (min %.1f max %.1f, %d x %d calls); best "
                  "hypothesis %d..%d labels" % (B, V, C, W, T, float(np.median(times)), min(times), max(times), rounds, CALLS,
                                                int(lens[:, 0].min()), int(lens[:, 0].max())))


def evaluate_once(mode):
    import numpy as np
    import torch
    _paths()
    import bench
    from utils import constant
    from utils.functions import init_transformer_model
    torch.cuda.set_device(0)
    flags = bench.MODEL_FLAGS + ["--dropout", "0", "--precision", "bf16", "--cuda", "--batch-size", str(B), "--ctc-weight", "0.3",
                                 "--tgt-max-len", "301", "--src-max-len", str(EVAL_T_SRC)]
    args = constant.parse(flags)
    l2i, i2l = bench.labels(V)
    torch.manual_seed(123456)
    model = init_transformer_model(args, l2i, i2l).cuda().eval()
    src, src_len, tgt = bench.synthetic_batch(B, torch, EVAL_T_SRC, 100, V)
    src, tgt = src.cuda(), tgt.cuda()
    kw = dict(ctc_beam=True, beam_width=EVAL_W) if mode == "beam" else {}
    times = []
    with torch.no_grad():
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, hyps, _ = model.evaluate(src, src_len, tgt, **kw)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    assert len(hyps) == B
    print("evaluate %-6s B %d T' %d: median %8.1f ms per batch over 3 calls after a warm-up call of %.1f ms (%s)"
          % (mode, B, EVAL_T_SRC // 4, float(np.median(times[1:])), times[0], ", ".join("%.1f" % t for t in times[1:])))


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
                for mode in ("beam", "greedy"):
                    rc = _child("--child-evaluate", mode)
                    if rc != 0:              # a fault, a hang or a failure: nothing more is started on the device
                        sys.exit(rc)
        sys.exit(rc)
