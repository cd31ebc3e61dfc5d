"""MWER training over the CTC n-best: what the new backward kernel and the step cost on one MI355X.

1. ops.seq_logprob_bwd (csrc/mwer.hip) against ops.ce_bwd (csrc/ce.hip) at the same M, V and output form, alternating in one process:
   the rows of B 32 utterances x (N + 1) sequences x 21 rows for N 4 / 8, V 4364, bf16 and fp32 output padded to 64 columns.  Both read
   M V 4 bytes and write M ldd {2,4}; ce_bwd is handed its log-sum-exp, seq_logprob_bwd recomputes it (the second read of a row comes
   from cache).  HIP events, medians of `rounds` brackets of 200 calls after warm-up.
2. The training step on the shape the neighbouring tools use (B 32, 300 input frames = T' 75, V 4364, bf16, the benchmark model with a CTC
   head, targets of 20 labels): the joint --ctc-weight 0.3 eager step (forward, joint loss, backward, optimiser) against the MWER step
   with N 4 and N 8 (--mwer-weight 0.5), the three alternating in one process; wall-clock medians of 15 steps after 3 warm-up steps, each
   step ended by a device synchronise.  What the decoder pass costs depends on how long the hypotheses are, so the steps run in three
   regimes: the randomly initialised head as it is (it emits almost only blanks: hypotheses of 0..1 labels, the fewest rows), "given"
   (N random hypotheses of 20 labels, the gold's length, handed to the step in place of the search: what a trained model's rows look
   like), and the blank's bias lowered to -10 (every frame emits a label: hypotheses as long as the 75 frames allow, the most rows).
3. The split of the MWER step's extra time at N 4 and N 8, each part by itself between synchronises (medians of 15): the search (CTC
   prefix beam search + its device-to-host copy), the host errors (edit_distance_batch), the decoder rows (Decoder._score_rows forward over
   gold + N hypotheses, against Decoder.forward over the gold alone), the loss (ops.mwer_loss).
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_mwer.py [rounds]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, T_SRC_STEP, LABELS, NBEST = 32, 4364, 300, 20, (4, 8)
CALLS, LIMIT_S, STEPS, WARM = 200, 420, 15, 3


def _paths():
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)


def timed_pair(torch, fns, rounds):
    """Microseconds per call of each fn: `rounds` HIP-event brackets of CALLS calls each, the fns alternating bracket by bracket."""
    for fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / CALLS * 1e3)
    return times


def kernels(rounds):
    import numpy as np
    import torch
    _paths()
    from asr_hip import ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    for N in NBEST:
        R = B * (N + 1)
        M = R * (LABELS + 1)
        g = torch.Generator().manual_seed(N)
        logits = torch.randn(M, V, generator=g).to(dev)
        tgt = torch.randint(3, V, (M,), generator=g).to(dev)
        off = torch.arange(0, M + 1, LABELS + 1, dtype=torch.int32).to(dev)
        coef = torch.randn(R, generator=g).to(dev)
        lse, _, sums, _ = ops.ce_fwd_det(logits, tgt, 0.0, 0)
        go, count = torch.ones(1, device=dev), sums[1:2].clone()
        for dt, name, width in ((torch.bfloat16, "bf16", 2), (torch.float32, "fp32", 4)):
            ours = lambda: ops.seq_logprob_bwd(logits, tgt, off, coef, out_dtype=dt, pad=64)
            ce = lambda: ops.ce_bwd(logits, tgt, lse, 0.0, 0, go, count, out_dtype=dt, pad=64)
            a, b = ours(), ce()
            assert a.shape == b.shape and torch.isfinite(a.float()).all()
            t_ours, t_ce = timed_pair(torch, (ours, ce), rounds)
            m_ours, m_ce = float(np.median(t_ours)), float(np.median(t_ce))
            byts = M * V * 4 + M * a.shape[1] * width
            print("N %d M %5d V %d %s out (ldd %d): seq_logprob_bwd median %6.1f us (min %.1f max %.1f)  ce_bwd %6.1f us (min %.1f max %.1f)  "
                  "ratio %.2f  [%.2f vs %.2f TB/s of %d bytes; %d x %d calls each, alternating]"
                  % (N, M, V, name, a.shape[1], m_ours, min(t_ours), max(t_ours), m_ce, min(t_ce), max(t_ce), m_ours / m_ce,
                     byts / (m_ours * 1e-6) / 1e12, byts / (m_ce * 1e-6) / 1e12, byts, rounds, CALLS))


def _model(torch):
    import bench
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    flags = bench.MODEL_FLAGS + ["--dropout", "0.1", "--precision", "bf16", "--cuda", "--batch-size", str(B), "--ctc-weight", "0.3",
                                 "--tgt-max-len", "101", "--src-max-len", str(T_SRC_STEP)]
    args = constant.parse(flags)
    l2i, i2l = bench.labels(V)
    torch.manual_seed(123456)
    model = init_transformer_model(args, l2i, i2l).cuda().train()
    return bench, args, model, init_optimizer(args, model, "noam")


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def steps():
    import numpy as np
    import torch
    _paths()
    from asr_hip import ops
    from utils import constant
    from utils.metrics import calculate_joint_loss
    torch.cuda.set_device(0)
    bench, args, model, opt = _model(torch)
    src, src_len, tgt = bench.synthetic_batch(B, torch, T_SRC_STEP, LABELS + 1, V)
    src, tgt = src.cuda(), tgt.cuda()
    tl = torch.full((B,), LABELS, dtype=torch.int32)

    def joint():
        opt.zero_grad()
        pred, gold, _, _, ctc = model(src, src_len, tgt, return_ctc=True)
        loss, _, _ = calculate_joint_loss(model, pred, gold, ctc, tgt, src_len, tl, 0.1, 0.3)
        ops.backward_from(loss)
        opt.step()
        return loss

    def mwer(N):
        def run():
            opt.zero_grad()
            loss = model.mwer_step(src, src_len, tgt, tl, 0.5, 0.3, nbest=N)[0]
            ops.backward_from(loss)
            opt.step()
            return loss
        return run

    g = torch.Generator().manual_seed(7)
    given = {N: [[torch.randint(3, V, (LABELS,), generator=g).tolist() for _ in range(N)] for _ in range(B)] for N in NBEST}

    def mwer_given(N):
        def run():
            opt.zero_grad()
            loss = model.mwer_step(src, src_len, tgt, tl, 0.5, 0.3, nbest=N, hyps=given[N])[0]
            ops.backward_from(loss)
            opt.step()
            return loss
        return run

    def regime(name, with_given):
        fns = [("joint", joint)] + [("mwer N %d" % N, mwer(N)) for N in NBEST]
        if with_given:
            fns += [("given N %d" % N, mwer_given(N)) for N in NBEST]
        t = {k: [] for k, _ in fns}
        for i in range(WARM + STEPS):
            for k, fn in fns:
                ms = _wall(torch, fn)
                if i >= WARM:
                    t[k].append(ms)
        base = float(np.median(t["joint"]))
        for k, _ in fns:
            med = float(np.median(t[k]))
            print("[" + name + "] step %-9s B %d T' %d V %d bf16: median %7.2f ms (min %.2f max %.2f, %d steps after %d warm-up, alternating)  %.2f x the joint step"
                  % (k, B, T_SRC_STEP // 4, V, med, min(t[k]), max(t[k]), STEPS, WARM, med / base))
        # ---- the split of the extra time, each part alone
        with torch.no_grad():
            enc = model.encoder(model._features(src), src_len)[0]
            ctc = model.ctc_logits(enc)
        frames = model.ctc_frame_lengths(src_len, ctc.shape[1])
        lens = torch.tensor(frames, dtype=torch.int32).cuda()
        golds = [row[:LABELS] for row in tgt.cpu().tolist()]
        T = ctc.shape[1]

        def med(fn, n=STEPS):
            for _ in range(WARM):
                fn()
            return float(np.median([_wall(torch, fn) for _ in range(n)]))

        def gold_only():
            with torch.no_grad():
                model.decoder(tgt, enc, src_len)

        t_gold = med(gold_only)
        for N in NBEST:
            box = {}

            def search():
                out = ops.ctc_beam_search(ctc, lens, N, 0, N, constant.PAD_TOKEN)
                flat = torch.cat([out["ids"].reshape(-1), out["lengths"].reshape(-1)]).cpu()
                ids, ln = torch.split(flat, [B * N * T, B * N])
                ids, ln = ids.view(B, N, T).tolist(), ln.view(B, N).tolist()
                box["hyps"] = [[ids[b][n][:ln[b][n]] for n in range(N) if ln[b][n] >= 0] for b in range(B)]

            t_search = med(search)
            hyps = box["hyps"]
            t_err = med(lambda: model.mwer_errors(hyps, golds, "label"))
            both = [[g] + hs for g, hs in zip(golds, hyps)]
            rows = sum(len(y) + 1 for hs in both for y in hs)

            def rows_fwd():
                with torch.no_grad():
                    box["out"] = model.decoder._score_rows(enc, both)

            t_rows = med(rows_fwd)
            score = box["out"][0]["score"]
            err = torch.rand(score.numel()).cuda()
            utt = torch.tensor([0] + list(np.cumsum([len(hs) for hs in both])), dtype=torch.int32).cuda()
            t_loss = med(lambda: ops.mwer_loss(score, err, utt, 0.5 / B, 0.35 / (B * (LABELS + 1))))
            print("[" + name + "] split N %d: search + copy %6.2f ms, host errors %5.2f ms, decoder forward over %d rows of gold + hypotheses %6.2f ms (gold alone, "
                  "Decoder.forward: %.2f ms), mwer_loss %5.3f ms; hypotheses of %d..%d labels, %d in all"
                  % (N, t_search, t_err, rows, t_rows, t_gold, t_loss, min(len(y) for hs in hyps for y in hs),
                     max(len(y) for hs in hyps for y in hs), sum(len(hs) for hs in hyps)))

    # a randomly initialised head emits almost only blanks (hypotheses of 0..1 labels: the fewest decoder rows a step can have); with the
    # blank's bias lowered every frame emits a label (hypotheses as long as the frames allow: the most); a trained model lies between,
    # near the gold length, which the "given" steps have (N random hypotheses of 20 labels, no search)
    regime("random head", True)
    with torch.no_grad():
        model.ctc_linear.bias[constant.PAD_TOKEN] = -10.0
    regime("blank bias -10", False)


def _child(*argv):
    # (a fresh child: this process never touches the device)
    return subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__)] + list(argv)).returncode


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child-kernels":
        kernels(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-steps":
        steps()
    else:
        rc = _child("--child-kernels", sys.argv[1] if len(sys.argv) > 1 else "7")
        if rc == 0:                  # after a fault, a hang or a failure nothing more is started on the device
            rc = _child("--child-steps")
        sys.exit(rc)
