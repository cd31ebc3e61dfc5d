"""asr_ctc_align beside asr_ctc_fwd on the same inputs, in one process: B 32, V 4364, L 60, at T' 75 and T' 400 (random logits, random
labels, full lengths).  asr_ctc_fwd walks the lattice twice (alpha and beta) with a log-add per state and writes both to memory; the
alignment walks it once with a compare and an add, then walks its back-pointers.  Both include the row log-sum-exp kernel.  HIP events,
medians of 7 rounds of 200 calls after warm-up, the two alternating.  The measurement runs in a child process under a time limit of its
own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_ctc_align.py [rounds]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, L, LENGTHS = 32, 4364, 60, (75, 400)
CALLS, LIMIT_S = 200, 240


def measure(rounds):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)
    from asr_hip import lib as Lb
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    h = Lb.load()
    for T in LENGTHS:
        g = torch.Generator().manual_seed(T)
        logits = (torch.randn(B, T, V, generator=g) * 2.0).to(dev)
        targets = torch.randint(3, V, (B, L), generator=g).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), L, dtype=torch.int32, device=dev)
        n_fwd, n_ali = h.asr_ctc_workspace(B, T, L), h.asr_ctc_align_workspace(B, T, L)
        ws_fwd = torch.empty(n_fwd, device=dev)
        ws_ali = torch.empty(n_ali, device=dev)
        loss = torch.empty(1, device=dev)
        path = torch.empty((B, T), dtype=torch.int32, device=dev)
        start, end = torch.empty((B, L), dtype=torch.int32, device=dev), torch.empty((B, L), dtype=torch.int32, device=dev)
        lab, score = torch.empty((B, L), device=dev), torch.empty(B, device=dev)

        def fwd():
            Lb.call("asr_ctc_fwd", Lb.ptr(logits), V, Lb.ptr(targets), Lb.ptr(il), Lb.ptr(tl), B, T, V, L, 0, Lb.ptr(ws_fwd), n_fwd,
                    Lb.ptr(loss), Lb.stream())

        def ali():
            Lb.call("asr_ctc_align", Lb.ptr(logits), V, Lb.ptr(targets), Lb.ptr(il), Lb.ptr(tl), B, T, V, L, 0, Lb.ptr(ws_ali), n_ali,
                    Lb.ptr(path), Lb.ptr(start), Lb.ptr(end), Lb.ptr(lab), Lb.ptr(score), Lb.stream())

        for _ in range(10):
            fwd()
            ali()
        torch.cuda.synchronize()
        times = {"asr_ctc_fwd": [], "asr_ctc_align": []}
        for _ in range(rounds):
            for name, fn in (("asr_ctc_fwd", fwd), ("asr_ctc_align", ali)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / CALLS * 1e3)
        assert torch.isfinite(score).all() and torch.isfinite(loss).all() and int(path.min()) >= 0
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k, v in times.items():
            print("B %d V %d L %d T' %3d %-14s median %7.1f us per call (min %.1f max %.1f, %d x %d calls)"
                  % (B, V, L, T, k, med[k], min(v), max(v), rounds, CALLS))
        print("T' %3d: asr_ctc_align / asr_ctc_fwd = %.2f" % (T, med["asr_ctc_align"] / med["asr_ctc_fwd"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
    else:
        rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # (a fresh child: this process never touches the device)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(rounds)])
        sys.exit(r.returncode)
