"""Knowledge distillation: what the fused row kernels and the step cost on one MI355X.

1. asr_distill_fwd + asr_distill_finish (ops.distill_fwd) against asr_ce_fwd_partials + asr_ce_finish (ops.ce_fwd_det), and
   asr_distill_bwd (ops.distill_bwd) against asr_ce_bwd (ops.ce_bwd), alternating in one process: M = B 32 x 100 decoder rows (the
   benchmark's), V 4364, smoothing 0.1, tau 2, bf16 output padded to 64 columns (the hand-over form) and, for the backward, the fp32
   output too (its arm sums the three distributions first).  The distill pair reads student AND teacher: twice the bytes of the CE pair,
   and three log-sum-exps per row instead of one.  HIP events, medians of `rounds` brackets of 200 calls after warm-up.
2. The training step at the configs[1] shape (B 32, 800 input frames, 100 decoder rows, V 4364, bf16, dropout 0.1): the eager CE step
   (forward, loss, backward, optimiser), the distillation step with --distill-weight 0.5 under a teacher of the same architecture, and
   the teacher's forward alone under no_grad, the three alternating; wall-clock medians of 15 steps after 3 warm-up steps, each ended by a
   device synchronise.
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_distill.py [rounds]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, T_TGT, SMOOTHING, TAU = 32, 4364, 100, 0.1, 2.0
CALLS, LIMIT_S, STEPS, WARM = 200, 420, 15, 3


def _paths():
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)


def timed(torch, fns, rounds):
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
    M = B * T_TGT
    g = torch.Generator().manual_seed(0)
    s = (torch.randn(M, V, generator=g) * 3.0).to(dev)
    t = (s.cpu() + torch.randn(M, V, generator=g) * 2.0).to(dev)
    gold = torch.randint(3, V, (M,), generator=g)
    gold[::5] = 0
    gold = gold.to(dev)
    lse, _, sums, _ = ops.ce_fwd_det(s, gold, SMOOTHING, 0)
    stats, _, dsums, _ = ops.distill_fwd(s, t, gold, SMOOTHING, 0, TAU, 0.5, 0.5)
    go, count = torch.ones(1, device=dev), sums[1:2].clone()
    assert torch.equal(sums[1], dsums[1]) and torch.isfinite(stats).all()
    fwd = (lambda: ops.distill_fwd(s, t, gold, SMOOTHING, 0, TAU, 0.5, 0.5), lambda: ops.ce_fwd_det(s, gold, SMOOTHING, 0))
    tf = [float(np.median(x)) for x in timed(torch, fwd, rounds)]
    print("forward  M %d V %d: distill_fwd + finish median %6.1f us  ce_fwd_partials + finish %6.1f us  ratio %.2f  [reads %d vs %d bytes: "
          "%.2f vs %.2f TB/s; %d x %d calls each, alternating]"
          % (M, V, tf[0], tf[1], tf[0] / tf[1], 2 * M * V * 4, M * V * 4, 2 * M * V * 4 / (tf[0] * 1e-6) / 1e12,
             M * V * 4 / (tf[1] * 1e-6) / 1e12, rounds, CALLS))
    for dt, name, width in ((torch.bfloat16, "bf16", 2), (torch.float32, "fp32", 4)):
        bwd = (lambda: ops.distill_bwd(s, t, gold, stats, SMOOTHING, 0, TAU, 0.5, 0.5, go, count, out_dtype=dt, pad=64),
               lambda: ops.ce_bwd(s, gold, lse, SMOOTHING, 0, go, count, out_dtype=dt, pad=64))
        a = bwd[0]()
        assert torch.isfinite(a.float()).all()
        tb = [float(np.median(x)) for x in timed(torch, bwd, rounds)]
        wr = M * a.shape[1] * width
        print("backward M %d V %d %s out (ldd %d): distill_bwd median %6.1f us  ce_bwd %6.1f us  ratio %.2f  [%d + %d vs %d + %d bytes: "
              "%.2f vs %.2f TB/s]" % (M, V, name, a.shape[1], tb[0], tb[1], tb[0] / tb[1], 2 * M * V * 4, wr, M * V * 4, wr,
                                      (2 * M * V * 4 + wr) / (tb[0] * 1e-6) / 1e12, (M * V * 4 + wr) / (tb[1] * 1e-6) / 1e12))
        if name == "bf16":
            print("pair     bf16: distill fwd + finish + bwd %6.1f us  CE fwd + finish + bwd %6.1f us  ratio %.2f"
                  % (tf[0] + tb[0], tf[1] + tb[1], (tf[0] + tb[0]) / (tf[1] + tb[1])))


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
    import bench
    from asr_hip import ops
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    from utils.metrics import calculate_metrics
    torch.cuda.set_device(0)
    flags = bench.MODEL_FLAGS + ["--dropout", "0.1", "--precision", "bf16", "--cuda", "--batch-size", str(B)]
    l2i, i2l = bench.labels(V)
    torch.manual_seed(1)
    teacher = init_transformer_model(constant.parse(flags), l2i, i2l).cuda().eval().requires_grad_(False)
    torch.manual_seed(123456)
    args = constant.parse(flags)
    model = init_transformer_model(args, l2i, i2l).cuda().train()
    opt = init_optimizer(args, model, "noam")
    src, src_len, tgt = bench.synthetic_batch(B, torch)
    src, tgt = src.cuda(), tgt.cuda()
    tl = torch.full((B,), tgt.shape[1], dtype=torch.int32)

    def ce():
        opt.zero_grad()
        pred, gold, _, _ = model(src, src_len, tgt)
        loss, _ = calculate_metrics(pred, gold, smoothing=SMOOTHING, loss_type="ce", sync=False)
        ops.backward_from(loss)
        opt.step()

    def distill():
        opt.zero_grad()
        loss = model.distill_step(src, src_len, tgt, tl, teacher, 0.5, TAU, SMOOTHING)[0]
        ops.backward_from(loss)
        opt.step()

    def teacher_fwd():
        with torch.no_grad():
            teacher(src, src_len, tgt)

    fns = (("eager CE step", ce), ("distill step", distill), ("teacher forward", teacher_fwd))
    t = {k: [] for k, _ in fns}
    for i in range(WARM + STEPS):
        for k, fn in fns:
            ms = _wall(torch, fn)
            if i >= WARM:
                t[k].append(ms)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k, _ in fns:
        print("step %-15s B %d T %d rows %d V %d bf16: median %7.2f ms (min %.2f max %.2f, %d steps after %d warm-up, alternating)"
              % (k, B, bench.T_SRC, T_TGT, V, med[k], min(t[k]), max(t[k]), STEPS, WARM))
    print("distill step - (eager CE step + teacher forward) = %.2f ms; distill step / eager CE step = %.2f"
          % (med["distill step"] - med["eager CE step"] - med["teacher forward"], med["distill step"] / med["eager CE step"]))


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
