"""Pruned transducer training: what its launches and its step cost on one MI355X, V 4364, joint width 256, bf16,
band S 5.

1. Every new entry point alone, HIP events, medians of `rounds` brackets of 20 calls after warm-up, at B 32, T' 75, U 20 / 40 and at
   B 16, T' 400, U 200: asr_rnnt_simple_fwd (its six launches together; the contraction dot = Ea El^T alone is 2 B T' (U+1) V flop),
   asr_rnnt_simple_bwd (two contractions of the same size and the one-hot launch), asr_rnnt_prune_ranges, asr_rnnt_joint_pruned_fwd /
   _bwd, asr_rnnt_pruned_fwd (fill, row pass, lattice, finish) and asr_rnnt_pruned_bwd (bf16 out, 4416 columns).
2. The training step (forward, loss, backward, optimiser; bench.py's model, dropout 0.1) at B 32, T' 75, U 20 / 40: --ctc-weight 0.3
   eager, + --transducer-weight 0.3 (the full lattice) and + --transducer-prune-range 5, alternating in one process; wall-clock medians
   of 10 steps after 3 warm-up steps, each ended by a device synchronise; the peak memory of each mode's last step.
3. The pruned step at B 16, 1600 input frames (T' 400), U 100 and 200, which the full lattice refuses (its joint logits would take 2^31
   bytes or more): medians of 5 steps after 2 warm-up steps, and the peak memory.
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_rnnt_pruned.py [rounds]"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mb_rnnt import B, J, SMOOTHING, STEPS, T_ENC, T_SRC, V, WARM, _model, _paths, _wall  # noqa: E402

CALLS, LIMIT_S, S = 20, 420, 5


def timed(torch, fn, rounds):
    import numpy as np
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return float(np.median(out))


def kernels(rounds):
    import torch
    _paths()
    from asr_hip import ops
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    for Bn, T, U in ((B, T_ENC, 20), (B, T_ENC, 40), (16, 400, 200)):
        U1 = U + 1

        def line(name, us, note=""):
            print("%-28s B %2d T' %3d U %3d S %d: median %9.1f us%s" % (name, Bn, T, U, S, us, note))
        am = torch.randn(Bn, T, V, generator=g).to(dev)
        lm = torch.randn(Bn, U1, V, generator=g).to(dev)
        tg = torch.randint(3, V, (Bn, U), generator=g).to(dev)
        fr = torch.full((Bn,), T, dtype=torch.int32, device=dev)
        tl = torch.full((Bn,), U, dtype=torch.int32, device=dev)
        loss, ws, gb, gl = ops.rnnt_simple_fwd(am, lm, tg, fr, tl)
        assert torch.isfinite(loss).all()
        flop = 2.0 * Bn * T * U1 * V
        us = timed(torch, lambda: ops.rnnt_simple_fwd(am, lm, tg, fr, tl), rounds)
        line("asr_rnnt_simple_fwd", us, "   (one contraction of %.2f GFLOP inside: %.1f TF/s if it were all of the time)" % (flop / 1e9, flop / us / 1e6))
        go = torch.ones(1, device=dev)
        us = timed(torch, lambda: ops.rnnt_simple_bwd(am.shape, lm.shape, tg, fr, tl, ws, go), rounds)
        line("asr_rnnt_simple_bwd", us, "   (two contractions: %.1f TF/s if they were all of the time)" % (2 * flop / us / 1e6))
        s = ops.rnnt_prune_ranges(gb, gl, fr, tl, S)
        line("asr_rnnt_prune_ranges", timed(torch, lambda: ops.rnnt_prune_ranges(gb, gl, fr, tl, S), rounds))
        del am, lm, ws, gb, gl
        e = torch.randn(Bn, T, J, generator=g).to(dev, torch.bfloat16)
        p = torch.randn(Bn, U1, J, generator=g).to(dev, torch.bfloat16)
        z = ops.rnnt_joint_pruned(e, p, s, S)
        dz = torch.randn(z.shape, generator=g).to(dev, torch.bfloat16)
        line("asr_rnnt_joint_pruned_fwd", timed(torch, lambda: ops.rnnt_joint_pruned(e, p, s, S), rounds))
        line("asr_rnnt_joint_pruned_bwd", timed(torch, lambda: ops.rnnt_joint_pruned_bwd(dz, z, s, U1), rounds))
        del z, dz
        logits = torch.empty(Bn * T * S, V, device=dev).normal_().mul_(3.0).view(Bn, T, S, V)
        loss, pws = ops.rnnt_pruned_fwd(logits, tg, fr, tl, s, U)
        assert torch.isfinite(loss).all()
        nb = logits.numel() * 4
        us = timed(torch, lambda: ops.rnnt_pruned_fwd(logits, tg, fr, tl, s, U), rounds)
        line("asr_rnnt_pruned_fwd", us, "   (%d bytes of logits: %.2f TB/s; %d diagonals)" % (nb, nb / us / 1e6, T + U))
        d = ops.rnnt_pruned_bwd(logits, tg, fr, tl, s, U, pws, go, out_dtype=torch.bfloat16, pad=64)
        assert torch.isfinite(d.float()).all()
        nb += d.numel() * 2
        del d
        us = timed(torch, lambda: ops.rnnt_pruned_bwd(logits, tg, fr, tl, s, U, pws, go, out_dtype=torch.bfloat16, pad=64), rounds)
        line("asr_rnnt_pruned_bwd (bf16)", us, "   (%d bytes: %.2f TB/s)" % (nb, nb / us / 1e6))
        del logits, pws
        torch.cuda.empty_cache()


def _batch(torch, Bn, t_src, U):
    import bench
    src, _, tgt = bench.synthetic_batch(Bn, torch, t_src=t_src, t_tgt=U + 1)
    return src.cuda(), torch.full((Bn,), t_src, dtype=torch.int64), tgt.cuda(), torch.full((Bn,), U, dtype=torch.int32)


def steps():
    import numpy as np
    import torch
    _paths()
    from asr_hip import ops
    from utils.metrics import calculate_joint_loss
    torch.cuda.set_device(0)
    head = ["--transducer-weight", "0.3", "--transducer-dim-joint", str(J)]
    joint, jopt = _model(torch, [])
    full, fopt = _model(torch, head)
    pruned, popt = _model(torch, head + ["--transducer-prune-range", str(S)])
    for U in (20, 40):
        src, src_len, tgt, tl = _batch(torch, B, T_SRC, U)

        def ctc_step():
            jopt.zero_grad()
            pred, gold, _, _, ctc = joint(src, src_len, tgt, return_ctc=True)
            loss = calculate_joint_loss(joint, pred, gold, ctc, tgt, src_len, tl, SMOOTHING, 0.3)[0]
            ops.backward_from(loss)
            jopt.step()

        def step_of(model, opt):
            def fn():
                opt.zero_grad()
                loss = model.transducer_step(src, src_len, tgt, tl, 0.3, SMOOTHING, ctc_weight=0.3, simple_scale=0.5)[0]
                ops.backward_from(loss)
                opt.step()
            return fn
        fns = (("--ctc-weight 0.3 eager", ctc_step), ("+ --transducer-weight 0.3", step_of(full, fopt)),
               ("+ --transducer-prune-range %d" % S, step_of(pruned, popt)))
        t, peak = {k: [] for k, _ in fns}, {}
        for i in range(WARM + STEPS):
            for k, fn in fns:
                torch.cuda.reset_peak_memory_stats()
                ms = _wall(torch, fn)
                peak[k] = torch.cuda.max_memory_allocated() / 2 ** 30
                if i >= WARM:
                    t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, _ in fns:
            print("step %-30s B %d T' %d U %d V %d bf16: median %7.2f ms (min %.2f max %.2f, %d steps after %d warm-up, alternating); "
                  "peak memory of a step %.2f GB (all three models resident)" % (k, B, T_ENC, U, V, med[k], min(t[k]), max(t[k]), STEPS, WARM, peak[k]))
        a, f, p = (med[k] for k, _ in fns)
        print("U %d: full-lattice head +%.2f ms, pruned head +%.2f ms over the joint step; pruned / full = %.2f" % (U, f - a, p - a, p / f))


def big():
    import numpy as np
    import torch
    _paths()
    from asr_hip import functions as F_
    from asr_hip import ops
    torch.cuda.set_device(0)
    Bn, t_src = 16, 1600
    model, opt = _model(torch, ["--transducer-weight", "0.3", "--transducer-dim-joint", str(J), "--transducer-prune-range", str(S),
                                "--batch-size", str(Bn), "--src-max-len", str(t_src), "--tgt-max-len", "256"])
    for U in (100, 200):
        src, src_len, tgt, tl = _batch(torch, Bn, t_src, U)
        try:
            F_.check_rnnt_shape(Bn, t_src // 4, U + 1, V)
            refused = "accepted"
        except ValueError:
            refused = "refused"

        def fn():
            opt.zero_grad()
            loss = model.transducer_step(src, src_len, tgt, tl, 0.3, SMOOTHING, ctc_weight=0.3, simple_scale=0.5)[0]
            ops.backward_from(loss)
            opt.step()
            return loss
        ms = []
        for i in range(2 + 5):
            torch.cuda.reset_peak_memory_stats()
            v = _wall(torch, fn)
            if i >= 2:
                ms.append(v)
        print("step + --transducer-prune-range %d   B %d T' %d U %d V %d bf16: median %7.2f ms (min %.2f max %.2f, 5 steps after 2 warm-up); "
              "peak memory %.2f GB; the full lattice at this shape is %s (%.1f GB of fp32 joint logits); loss %.4f"
              % (S, Bn, t_src // 4, U, V, float(np.median(ms)), min(ms), max(ms), torch.cuda.max_memory_allocated() / 2 ** 30, refused,
                 Bn * (t_src // 4) * (U + 1) * 4416 * 4 / 1e9, float(fn().detach())))


def _child(*argv):
    # (a fresh child: this process never touches the device)
    return subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__)] + list(argv)).returncode


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child-kernels":
        kernels(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-steps":
        steps()
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-big":
        big()
    else:
        rc = _child("--child-kernels", sys.argv[1] if len(sys.argv) > 1 else "5")
        for mode in ("--child-steps", "--child-big"):
            if rc == 0:              # after a fault, a hang or a failure nothing more is started on the device
                rc = _child(mode)
        sys.exit(rc)
