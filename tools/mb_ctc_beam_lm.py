"""The fused arm of the CTC prefix beam search (asr_ctc_beam_search_lm, csrc/ctc_beam.hip) against the plain search, in the same call.

B 32, T' 75, V 4364, C 16, W 8 and 16, full lengths, on the peaked random logits of tools/mb_ctc_beam.py (standard normal plus 10 on one
winner per frame: a label every fourth frame, the blank elsewhere).  The LM: a Witten-Bell trigram (utils/ngram.py) of a synthetic corpus
of 40000 sentences of 20 labels drawn from a Zipf-like distribution over the labels -- 1.17e6 stored n-grams, a table of 2^22 slots
(64 MiB: keys and values, far beyond the 4 MiB L2 of an XCD).  alpha 0.3, beta 0.5, SOS / EOS as the sentence marks.  Both entries run all three launches (row log-sum-exp,
top-C, search); they alternate round by round.  HIP events, medians of 7 rounds of 200 calls after warm-up.  asr_ngram_logp alone on
B * W * C queries (one step's worth of extension slots) is printed beside them.
The measurement runs in a child process under a time limit, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_ctc_beam_lm.py [rounds]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, V, C, WIDTHS, ORDER = 32, 75, 4364, 16, (8, 16), 3
SENTENCES, SENT_LEN = 40000, 20
ALPHA, BETA, BOS, EOS = 0.3, 0.5, 1, 2
CALLS, LIMIT_S = 200, 400


def corpus(np):
    rng = np.random.default_rng(0)
    p = 1.0 / np.arange(1, V - 2) ** 0.9
    ids = 3 + rng.choice(V - 3, size=(SENTENCES, SENT_LEN), p=p / p.sum())
    return ids.tolist()


def bracket(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


def measure(rounds):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    from asr_hip import lib as Lb
    from asr_hip import ops
    from utils.ngram import NgramLM
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    lm = NgramLM.estimate(corpus(np), V, ORDER, BOS, EOS)
    t = lm.device_table(dev)
    print("trigram LM: %d stored n-grams, table of %d slots (%.1f MiB), longest probe run %d" % (
        len(lm.keys), t["capacity"], t["capacity"] * 16 / 2 ** 20, t["max_probe"]))
    g = torch.Generator().manual_seed(T)
    logits = torch.randn(B, T, V, generator=g)
    win = torch.zeros(B, T, dtype=torch.int64)
    win[:, ::4] = torch.randint(3, V, (B, (T + 3) // 4), generator=g)
    logits.scatter_add_(2, win.unsqueeze(2), torch.full((B, T, 1), 10.0))
    logits = logits.to(dev)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    h = Lb.load()
    for W in WIDTHS:
        n = h.asr_ctc_beam_workspace(B, T, W, C)
        ws = torch.empty(n, device=dev)
        ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
        lens, scores, lmv = torch.empty((B, W), dtype=torch.int32, device=dev), torch.empty((B, W), device=dev), torch.empty((B, W), device=dev)
        head = (Lb.ptr(logits), V, Lb.ptr(il), B, T, V, W, C, W, 0, Lb.ptr(ws), n, Lb.ptr(ids), Lb.ptr(lens), Lb.ptr(scores))

        def plain():
            Lb.call("asr_ctc_beam_search", *head, Lb.stream())

        def fused():
            Lb.call("asr_ctc_beam_search_lm", *head, Lb.ptr(t["keys"]), Lb.ptr(t["vals"]), t["capacity"], t["max_probe"], ORDER, BOS, EOS,
                    ALPHA, BETA, Lb.ptr(lmv), Lb.stream())

        q = B * W * C
        ctx = torch.randint(3, V, (q, ORDER - 1), generator=g).to(torch.int32).to(dev)
        sym = torch.randint(3, V, (q,), generator=g).to(torch.int32).to(dev)

        def lookup():
            ops.ngram_logp(t, ctx, sym)

        for fn in (plain, fused, lookup):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {"plain": [], "fused": [], "lookup": []}
        for _ in range(rounds):
            for name, fn in (("plain", plain), ("fused", fused), ("lookup", lookup)):
                times[name].append(bracket(torch, fn))
        fused()
        torch.cuda.synchronize()
        assert torch.isfinite(scores[:, 0]).all() and torch.isfinite(lmv[:, 0]).all() and int(lens[:, 0].min()) > 0
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("B %d V %d C %d W %2d T' %d: plain %7.1f us per call (min %.1f max %.1f), fused %7.1f us (min %.1f max %.1f) = %.2f x plain, "
              "+%.2f us per frame; asr_ngram_logp on %d random queries %.1f us; %d x %d calls each; best fused hypothesis %d..%d labels"
              % (B, V, C, W, T, med["plain"], min(times["plain"]), max(times["plain"]), med["fused"], min(times["fused"]),
                 max(times["fused"]), med["fused"] / med["plain"], (med["fused"] - med["plain"]) / T, q, med["lookup"], rounds, CALLS,
                 int(lens[:, 0].min()), int(lens[:, 0].max())))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
    else:
        # (a fresh child: this process never touches the device)
        sys.exit(subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child",
                                 sys.argv[1] if len(sys.argv) > 1 else "7"]).returncode)
