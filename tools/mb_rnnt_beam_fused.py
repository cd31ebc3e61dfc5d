"""The fused arms of the transducer beam search (asr_rnnt_beam_search_lm / _ctx, csrc/rnnt_beam.hip) against the
plain search, in ONE call: what a step's n-gram and phrase lookups cost.

The shape of tools/mb_rnnt_beam.py -- B 32, T' 75, V 4364, J 256, bf16, K 16, full lengths, bench.py's model with a transducer head -- at
W 8 and 16, S 2 and 5.  The trigram table is tools/mb_ctc_beam_lm.py's (1.17e6 stored n-grams, 2^22 slots), the phrase list
tools/mb_ctc_beam_ctx.py's 1000 phrases; alpha 0.3, beta 0.5, gamma 3, bos SOS, eos EOS.  Four entries -- plain, LM only, phrases only,
both -- alternate round by round; HIP events, medians of `rounds` brackets of 10 calls after warm-up, as ms per batch and us per search
step (a batch is T' (S + 1) steps: no early exit).  The last line of a shape says whether the two increments add.

--parent-lib PATH: a libasr_hip.so built from the commit before the fused arms.  Its asr_rnnt_beam_search joins the rotation TWICE
(parent, parent again): the distance between the two medians and the range of the parent's brackets are the call's own spread, and
the plain arm of this tree is held against both.
The measurement runs in a child process under a time limit, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_rnnt_beam_fused.py [rounds] [--parent-lib PATH]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mb_ctc_beam_ctx as ctx_tool  # noqa: E402
import mb_ctc_beam_lm as lm_tool  # noqa: E402
import mb_rnnt_beam as plain_tool  # noqa: E402

B, V, J = plain_tool.B, plain_tool.V, plain_tool.J
K, SHAPES = 16, ((8, 2), (16, 2), (8, 5), (16, 5))
ALPHA, BETA, GAMMA, BOS, EOS, ORDER = lm_tool.ALPHA, lm_tool.BETA, ctx_tool.GAMMA, lm_tool.BOS, lm_tool.EOS, lm_tool.ORDER
CALLS, LIMIT_S = 10, 900


def tables(np, torch):
    """The trigram LM of tools/mb_ctc_beam_lm.py and the phrase list of tools/mb_ctc_beam_ctx.py (its generator, draw for draw)."""
    from utils.context import ContextGraph
    from utils.ngram import NgramLM
    lm = NgramLM.estimate(lm_tool.corpus(np), V, ORDER, BOS, EOS)
    T = lm_tool.T
    g = torch.Generator().manual_seed(T)
    torch.randn(lm_tool.B, T, V, generator=g)                   # (the logits that tool draws first)
    win = torch.zeros(lm_tool.B, T, dtype=torch.int64)
    win[:, ::4] = torch.randint(3, V, (lm_tool.B, (T + 3) // 4), generator=g)
    return lm, ContextGraph.from_phrases(ctx_tool.phrases(np, win.numpy()), V)


def bracket(torch, fn):
    """ms per call over CALLS calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


def measure(rounds, parent_path):
    import ctypes

    import numpy as np
    import torch
    plain_tool._paths()
    from asr_hip import functions as F_, lib as Lb, params as P
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    model, enc, frames = plain_tool._setup(torch)
    T = enc.shape[1]
    with torch.no_grad():
        e = F_.linear(enc, model.rnnt_enc.weight, model.rnnt_enc.bias, False, True).contiguous()
    tabs = [P.linear_weight(m.weight, e.dtype) for m in model.rnnt_embed]
    w_out, b_out = P.linear_weight(model.rnnt_out.weight, e.dtype), model.rnnt_out.bias.data
    fl = torch.tensor(frames, dtype=torch.int32, device=dev)
    lm, graph = tables(np, torch)
    t, c = lm.device_table(dev), graph.device_table(dev)
    print("B %d T' %d V %d J %d %s K %d; trigram LM: %d stored n-grams, table of %d slots, longest probe run %d; phrase list: %d phrases, "
          "%d states, table of %d slots, longest probe run %d" % (B, T, V, J, e.dtype, K, len(lm.keys), t["capacity"], t["max_probe"],
                                                                 len(graph.phrases), graph.states, c["capacity"], c["max_probe"]))
    h = Lb.load()
    parent = None
    if parent_path:
        parent = ctypes.CDLL(parent_path)
        for name in ("asr_rnnt_beam_workspace", "asr_rnnt_beam_search"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = Lb._SIGS[name]
    for W, S in SHAPES:
        n = h.asr_rnnt_beam_workspace(B, T, V, W, K, S)
        ws = torch.empty(n, device=dev)
        ids = torch.empty((B, W, T * S), dtype=torch.int32, device=dev)
        lens, credit = torch.empty((B, W), dtype=torch.int32, device=dev), torch.empty((B, W), dtype=torch.int32, device=dev)
        scores, lmv = torch.empty((B, W), device=dev), torch.empty((B, W), device=dev)
        head = (Lb.ptr(e), Lb.ptr(tabs[0]), Lb.ptr(tabs[1]) if len(tabs) == 2 else None, Lb.ptr(w_out), Lb.ptr(b_out), Lb.ptr(fl), B, T, J, V,
                W, K, S, W, 0, BOS, Lb.dt(e), Lb.ptr(ws), n, Lb.ptr(ids), Lb.ptr(lens), Lb.ptr(scores))
        ng = (Lb.ptr(t["keys"]), Lb.ptr(t["vals"]), t["capacity"], t["max_probe"], ORDER, BOS, EOS, ALPHA, BETA)
        cx = (Lb.ptr(c["keys"]), Lb.ptr(c["vals"]), c["capacity"], c["max_probe"], Lb.ptr(c["hold"]), c["states"], GAMMA)

        def plain():
            Lb.call("asr_rnnt_beam_search", *head, Lb.stream())

        def fused():
            Lb.call("asr_rnnt_beam_search_lm", *head, *ng, Lb.ptr(lmv), Lb.stream())

        def biased():
            Lb.call("asr_rnnt_beam_search_ctx", *head, None, None, 0, 0, 0, BOS, EOS, 0.0, BETA, *cx, Lb.ptr(lmv), Lb.ptr(credit), Lb.stream())

        def both():
            Lb.call("asr_rnnt_beam_search_ctx", *head, *ng, *cx, Lb.ptr(lmv), Lb.ptr(credit), Lb.stream())

        def old():
            rc = parent.asr_rnnt_beam_search(*head, Lb.stream())
            assert rc == 0, rc

        arms = [("plain", plain), ("lm", fused), ("phrases", biased), ("phrases+lm", both)]
        if parent is not None:
            arms = [("parent", old)] + arms + [("parent again", old)]
        for _, fn in arms:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in arms}
        for _ in range(rounds):
            for name, fn in arms:
                times[name].append(bracket(torch, fn))
        both()
        torch.cuda.synchronize()
        assert torch.isfinite(scores[:, 0]).all() and torch.isfinite(lmv[:, 0]).all() and int(credit[:, 0].min()) >= 0
        med = {k: float(np.median(v)) for k, v in times.items()}
        steps = T * (S + 1)
        print("W %2d S %d (%d steps), ms per batch (min .. max), us per search step, us per step over plain:" % (W, S, steps))
        for name, _ in arms:
            print("  %-12s %8.3f (%.3f .. %.3f)  %7.2f  %+.2f" % (name, med[name], min(times[name]), max(times[name]), med[name] * 1e3 / steps,
                                                                  (med[name] - med["plain"]) * 1e3 / steps))
        d_lm, d_cx, d_both = ((med[k] - med["plain"]) * 1e3 / steps for k in ("lm", "phrases", "phrases+lm"))
        print("  increments per step: lm %.2f us, phrases %.2f us, their sum %.2f us, phrases+lm %.2f us (%s); best hypothesis earns %.1f "
              "labels on average with both; %d x %d calls each" % (d_lm, d_cx, d_lm + d_cx, d_both,
                                                                    "above the sum" if d_both > d_lm + d_cx else "within the sum",
                                                                    float(credit[:, 0].float().mean()), rounds, CALLS))
        if parent is not None:
            lo, hi = sorted((med["parent"], med["parent again"]))
            every = times["parent"] + times["parent again"]
            if lo <= med["plain"] <= hi:
                verdict = "between the two"
            else:
                d = med["plain"] - (hi if med["plain"] > hi else lo)
                verdict = "%+.3f ms (%+.3f %%) outside the two, %s the range of the parent's %d brackets" % (
                    d, 100.0 * d / hi, "inside" if min(every) <= med["plain"] <= max(every) else "OUTSIDE", len(every))
            print("  plain %.3f ms against the parent build's %.3f and %.3f ms (%.3f ms apart; its brackets %.3f .. %.3f): %s" % (
                med["plain"], med["parent"], med["parent again"], hi - lo, min(every), max(every), verdict))


if __name__ == "__main__":
    argv = sys.argv[1:]
    parent_lib = ""
    if "--parent-lib" in argv:
        i = argv.index("--parent-lib")
        parent_lib = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    if argv and argv[0] == "--child":
        measure(int(argv[1]), parent_lib)
    else:
        # (a fresh child: this process never touches the device)
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", argv[0] if argv else "5"]
        sys.exit(subprocess.run(cmd + (["--parent-lib", parent_lib] if parent_lib else [])).returncode)
