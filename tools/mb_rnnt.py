"""Transducer head: what the new launches, the step and the greedy search cost on one MI355X, at B 32, T' 75
encoder frames (300 input frames), U 20 and 40 labels, V 4364, joint width 256, bf16.

1. Every new entry point alone, HIP events, medians of `rounds` brackets of 50 calls after warm-up, with the bytes it has to move over
   its time (the streaming rate the other mb_ tools quote): asr_rnnt_joint_fwd (reads e and p, writes z), asr_rnnt_joint_bwd (reads dz
   and z, writes de and dp), asr_rnnt_fwd (its three launches together -- row pass, lattice, finish: the fp32 logits read once) and
   asr_rnnt_bwd (the logits read once, the bf16 gradient, 4416 columns wide, written once).  The lattice alone is the same entry with
   V 8: its rows are then a hundredth of the bytes.
2. The training step (forward, loss, backward, optimiser; bench.py's model at this shape, dropout 0.1): --ctc-weight 0.3 eager against
   --ctc-weight 0.3 --transducer-weight 0.3, alternating in one process; wall-clock medians of 10 steps after 3 warm-up steps, each ended
   by a device synchronise.
3. transducer_greedy (--transducer-max-symbols 5) against ctc_greedy on the same encoder output; wall-clock medians of 5 calls.
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_rnnt.py [rounds]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, T_ENC, T_SRC, J, SMOOTHING = 32, 4364, 75, 300, 256, 0.1
CALLS, LIMIT_S, STEPS, WARM = 50, 420, 10, 3


def _paths():
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)


def timed(torch, fn, rounds):
    """Median microseconds per call of fn: `rounds` HIP-event brackets of CALLS calls each."""
    import numpy as np
    for _ in range(5):
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

    def line(name, U, us, nbytes, note=""):
        print("%-22s U %2d: median %8.1f us  %12d bytes  %.2f TB/s%s" % (name, U, us, nbytes, nbytes / (us * 1e-6) / 1e12, note))
    for U in (20, 40):
        U1, M = U + 1, B * T_ENC * (U + 1)
        e = torch.randn(B, T_ENC, J, generator=g).to(dev, torch.bfloat16)
        p = torch.randn(B, U1, J, generator=g).to(dev, torch.bfloat16)
        z = ops.rnnt_joint(e, p)
        dz = torch.randn(M * J, generator=g).to(dev, torch.bfloat16).view(B, T_ENC, U1, J)
        line("asr_rnnt_joint_fwd", U, timed(torch, lambda: ops.rnnt_joint(e, p), rounds), (e.numel() + p.numel() + z.numel()) * 2)
        line("asr_rnnt_joint_bwd", U, timed(torch, lambda: ops.rnnt_joint_bwd(dz, z), rounds), (2 * z.numel() + e.numel() + p.numel()) * 2)
        del dz, z
        tg = torch.randint(3, V, (B, U), generator=g).to(dev)
        fr = torch.full((B,), T_ENC, dtype=torch.int32, device=dev)
        tl = torch.full((B,), U, dtype=torch.int32, device=dev)
        small, tg8 = torch.randn(M, 8, generator=g).to(dev).view(B, T_ENC, U1, 8), tg.clamp(max=7)
        line("asr_rnnt_fwd, V 8", U, timed(torch, lambda: ops.rnnt_fwd(small, tg8, fr, tl), rounds), M * 8 * 4,
             "   (the lattice: %d diagonals)" % (T_ENC + U))
        del small
        logits = torch.empty(M, V, device=dev).normal_().mul_(3.0).view(B, T_ENC, U1, V)
        loss, ws = ops.rnnt_fwd(logits, tg, fr, tl)
        assert torch.isfinite(loss).all()
        line("asr_rnnt_fwd", U, timed(torch, lambda: ops.rnnt_fwd(logits, tg, fr, tl), rounds), M * V * 4)
        go = torch.ones(1, device=dev)
        d = ops.rnnt_bwd(logits, tg, fr, tl, ws, go, out_dtype=torch.bfloat16, pad=64)
        assert torch.isfinite(d.float()).all()
        ldd = d.shape[1]
        del d
        line("asr_rnnt_bwd (bf16 out)", U, timed(torch, lambda: ops.rnnt_bwd(logits, tg, fr, tl, ws, go, out_dtype=torch.bfloat16, pad=64), rounds),
             M * V * 4 + M * ldd * 2, "   (ldd %d)" % ldd)
        del logits, ws
        torch.cuda.empty_cache()


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _model(torch, extra):
    import bench
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    flags = bench.MODEL_FLAGS + ["--dropout", "0.1", "--precision", "bf16", "--cuda", "--batch-size", str(B), "--ctc-weight", "0.3"] + extra
    l2i, i2l = bench.labels(V)
    torch.manual_seed(123456)
    args = constant.parse(flags)
    model = init_transformer_model(args, l2i, i2l).cuda().train()
    return model, init_optimizer(args, model, "noam")


def steps():
    import numpy as np
    import torch
    _paths()
    import bench
    from asr_hip import ops
    from utils.metrics import calculate_joint_loss
    torch.cuda.set_device(0)
    joint, jopt = _model(torch, [])
    rnnt, ropt = _model(torch, ["--transducer-weight", "0.3", "--transducer-dim-joint", str(J)])
    for U in (20, 40):
        src, src_len, tgt = bench.synthetic_batch(B, torch, t_src=T_SRC, t_tgt=U + 1)
        src, tgt = src.cuda(), tgt.cuda()
        src_len = torch.full((B,), T_SRC, dtype=torch.int64)
        tl = torch.full((B,), U, dtype=torch.int32)

        def ctc_step():
            jopt.zero_grad()
            pred, gold, _, _, ctc = joint(src, src_len, tgt, return_ctc=True)
            loss = calculate_joint_loss(joint, pred, gold, ctc, tgt, src_len, tl, SMOOTHING, 0.3)[0]
            ops.backward_from(loss)
            jopt.step()

        def rnnt_step():
            ropt.zero_grad()
            loss = rnnt.transducer_step(src, src_len, tgt, tl, 0.3, SMOOTHING, ctc_weight=0.3)[0]
            ops.backward_from(loss)
            ropt.step()

        fns = (("--ctc-weight 0.3 eager", ctc_step), ("+ --transducer-weight 0.3", rnnt_step))
        t = {k: [] for k, _ in fns}
        for i in range(WARM + STEPS):
            for k, fn in fns:
                ms = _wall(torch, fn)
                if i >= WARM:
                    t[k].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, _ in fns:
            print("step %-26s B %d T' %d U %d V %d bf16: median %7.2f ms (min %.2f max %.2f, %d steps after %d warm-up, alternating)"
                  % (k, B, T_ENC, U, V, med[k], min(t[k]), max(t[k]), STEPS, WARM))
        print("U %d: transducer step / joint step = %.2f (+%.2f ms); peak memory %.2f GB"
              % (U, med[fns[1][0]] / med[fns[0][0]], med[fns[1][0]] - med[fns[0][0]], torch.cuda.max_memory_allocated() / 2 ** 30))


def greedy():
    import numpy as np
    import torch
    _paths()
    import bench
    torch.cuda.set_device(0)
    model, _ = _model(torch, ["--transducer-weight", "0.3", "--transducer-dim-joint", str(J)])
    model.eval()
    src, _, _ = bench.synthetic_batch(B, torch, t_src=T_SRC, t_tgt=21)
    lengths = torch.full((B,), T_SRC, dtype=torch.int64)
    with torch.no_grad():
        enc = model.encoder(model._features(src.cuda()), lengths)[0]
    frames = model.ctc_frame_lengths(lengths, enc.shape[1])
    fns = (("ctc_greedy", lambda: model.ctc_greedy(enc, frames)), ("transducer_greedy (5)", lambda: model.transducer_greedy(enc, frames, 5)))
    for k, fn in fns:
        fn()
        ms = [_wall(torch, fn) for _ in range(5)]
        print("decode %-22s B %d T' %d V %d bf16: median %8.2f ms (min %.2f max %.2f, 5 calls)"
              % (k, B, enc.shape[1], V, float(np.median(ms)), min(ms), max(ms)))


def _child(*argv):
    # (a fresh child: this process never touches the device)
    return subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__)] + list(argv)).returncode


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child-kernels":
        kernels(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-steps":
        steps()
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-greedy":
        greedy()
    else:
        rc = _child("--child-kernels", sys.argv[1] if len(sys.argv) > 1 else "5")
        for mode in ("--child-steps", "--child-greedy"):
            if rc == 0:              # after a fault, a hang or a failure nothing more is started on the device
                rc = _child(mode)
        sys.exit(rc)
