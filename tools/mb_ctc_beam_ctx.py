"""The phrase arms of the CTC prefix beam search (asr_ctc_beam_search_ctx, csrc/ctc_beam.hip) against the plain search and the LM arm, in
the same call.

B 32, T' 75, V 4364, C 16, W 8 and 16, full lengths, on the peaked random logits and under the trigram LM of tools/mb_ctc_beam_lm.py
(1.17e6 stored n-grams, a table of 2^22 slots).  The phrase list: 1000 phrases of 2 to 6 labels, half of them cut from the label
sequences the logits spell (so that matches advance, complete and break off), half random; gamma 3.  Four entries -- plain, LM, phrases
only, phrases + LM -- run all three launches (row log-sum-exp, top-C, search) and alternate round by round.  HIP events, medians of 7
rounds of 200 calls after warm-up.  asr_ctx_step alone on B * W * C transitions (one step's worth of extension slots) is printed beside them.
The measurement runs in a child process under a time limit, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_ctc_beam_ctx.py [rounds]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mb_ctc_beam_lm as lm_tool  # noqa: E402

B, T, V, C, WIDTHS, ORDER = lm_tool.B, lm_tool.T, lm_tool.V, lm_tool.C, lm_tool.WIDTHS, lm_tool.ORDER
ALPHA, BETA, BOS, EOS = lm_tool.ALPHA, lm_tool.BETA, lm_tool.BOS, lm_tool.EOS
PHRASES, GAMMA = 1000, 3.0
CALLS, LIMIT_S = lm_tool.CALLS, 500


def phrases(np, win):
    """Half cut from the spelled sequences (win: (B,T) winners, 0 = blank), half random; 2 to 6 labels each."""
    rng = np.random.default_rng(1)
    spelled = [[int(c) for c in row if c] for row in win.tolist()]
    out = set()
    for i in range(100 * PHRASES):
        if len(out) == PHRASES:
            break
        n = int(rng.integers(2, 7))
        if i % 2:
            out.add(tuple(rng.integers(3, V, size=n).tolist()))
        else:
            s = spelled[int(rng.integers(len(spelled)))]
            j = int(rng.integers(0, len(s) - n + 1))
            out.add(tuple(s[j:j + n]))
    return sorted(out)


def measure(rounds):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    from asr_hip import lib as Lb
    from asr_hip import ops
    from utils.context import ContextGraph
    from utils.ngram import NgramLM
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    lm = NgramLM.estimate(lm_tool.corpus(np), V, ORDER, BOS, EOS)
    t = lm.device_table(dev)
    g = torch.Generator().manual_seed(T)
    logits = torch.randn(B, T, V, generator=g)
    win = torch.zeros(B, T, dtype=torch.int64)
    win[:, ::4] = torch.randint(3, V, (B, (T + 3) // 4), generator=g)
    logits.scatter_add_(2, win.unsqueeze(2), torch.full((B, T, 1), 10.0))
    logits = logits.to(dev)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    graph = ContextGraph.from_phrases(phrases(np, win.numpy()), V)
    c = graph.device_table(dev)
    print("trigram LM: %d stored n-grams, table of %d slots; phrase list: %d phrases, %d states, %d stored transitions, table of %d slots "
          "(%.2f MiB with hold), longest probe run %d" % (len(lm.keys), t["capacity"], len(graph.phrases), graph.states,
                                                          len(graph.transitions()[0]), c["capacity"],
                                                          (c["capacity"] * 16 + graph.states * 4) / 2 ** 20, c["max_probe"]))
    h = Lb.load()
    for W in WIDTHS:
        n = h.asr_ctc_beam_workspace(B, T, W, C)
        ws = torch.empty(n, device=dev)
        ids = torch.empty((B, W, T), dtype=torch.int32, device=dev)
        lens, credit = torch.empty((B, W), dtype=torch.int32, device=dev), torch.empty((B, W), dtype=torch.int32, device=dev)
        scores, lmv = torch.empty((B, W), device=dev), torch.empty((B, W), device=dev)
        head = (Lb.ptr(logits), V, Lb.ptr(il), B, T, V, W, C, W, 0, Lb.ptr(ws), n, Lb.ptr(ids), Lb.ptr(lens), Lb.ptr(scores))
        ng = (Lb.ptr(t["keys"]), Lb.ptr(t["vals"]), t["capacity"], t["max_probe"], ORDER, BOS, EOS, ALPHA, BETA, Lb.ptr(lmv))
        cx = (Lb.ptr(c["keys"]), Lb.ptr(c["vals"]), c["capacity"], c["max_probe"], Lb.ptr(c["hold"]), c["states"], GAMMA, Lb.ptr(credit))

        def plain():
            Lb.call("asr_ctc_beam_search", *head, Lb.stream())

        def fused():
            Lb.call("asr_ctc_beam_search_lm", *head, *ng, Lb.stream())

        def biased():
            Lb.call("asr_ctc_beam_search_ctx", *head, None, None, 0, 0, 0, BOS, EOS, 0.0, BETA, Lb.ptr(lmv), *cx, Lb.stream())

        def both():
            Lb.call("asr_ctc_beam_search_ctx", *head, *ng, *cx, Lb.stream())

        q = B * W * C
        state = torch.randint(0, graph.states, (q,), generator=g).to(torch.int32).to(dev)
        sym = torch.randint(3, V, (q,), generator=g).to(torch.int32).to(dev)

        def lookup():
            ops.context_step(c, state, sym)

        arms = (("plain", plain), ("lm", fused), ("phrases", biased), ("phrases+lm", both), ("lookup", lookup))
        for _, fn in arms:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in arms}
        for _ in range(rounds):
            for name, fn in arms:
                times[name].append(lm_tool.bracket(torch, fn))
        found = {}
        for name, fn in arms[2:4]:
            fn()
            torch.cuda.synchronize()
            assert torch.isfinite(scores[:, 0]).all() and int(lens[:, 0].min()) > 0 and int(credit[:, 0].min()) >= 0
            found[name] = (float(credit[:, 0].float().mean()), int(credit[:, 0].max()))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("B %d V %d C %d W %2d T' %d, us per call (min .. max) and us per frame over plain:" % (B, V, C, W, T))
        for name, _ in arms[:4]:
            print("  %-11s %7.1f (%.1f .. %.1f)  %+.2f" % (name, med[name], min(times[name]), max(times[name]),
                                                           (med[name] - med["plain"]) / T))
        print("  increments per frame: lm %.2f, phrases %.2f, their sum %.2f, phrases+lm %.2f; asr_ctx_step on %d random transitions "
              "%.1f us; %d x %d calls each; best hypothesis earns %.1f labels on average (most %d) with phrases, %.1f (%d) with both"
              % ((med["lm"] - med["plain"]) / T, (med["phrases"] - med["plain"]) / T,
                 (med["lm"] + med["phrases"] - 2 * med["plain"]) / T, (med["phrases+lm"] - med["plain"]) / T, q, med["lookup"], rounds,
                 CALLS, *found["phrases"], *found["phrases+lm"]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
    else:
        # (a fresh child: this process never touches the device)
        sys.exit(subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child",
                                 sys.argv[1] if len(sys.argv) > 1 else "7"]).returncode)
