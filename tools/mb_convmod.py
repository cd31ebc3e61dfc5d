"""The convolution module's three kernels (csrc/convmod.hip) beside the module's own two pointwise GEMMs and its add + LayerNorm epilogue,
in one process, at the encoder shape of BASELINE.json configs[1] (B 32, T' = T_src / 4 = 200, D 512; bf16) for K = 15 and 31; then the
eager training step of that model with and without --conv-module-kernel.  HIP events, medians of 7 rounds of 200 calls after warm-up,
the launches alternating.  Forward side: pointwise_1 (D -> 2D), pointwise_2 (D -> D), add_ln; backward side: the two data-gradient
GEMMs, the two weight-gradient GEMMs, add_ln's backward.  Lengths are full, so no tile is skipped.  The measurement runs in a child
process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_convmod.py [rounds]"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, LIMIT_S, STEP_CALLS = 200, 420, 20


def baseline_shape():
    """(B, T', D, layers, heads, inner, T_src, T_tgt) of BASELINE.json configs[1]."""
    text = json.load(open(os.path.join(ROOT, "BASELINE.json")))["configs"][1]
    num = lambda pat: int(re.search(pat, text).group(1))
    assert "vgg_cnn" in text
    t_src = num(r"T_src=(\d+)")
    return (num(r"bs=(\d+)"), t_src // 4, num(r"d_model=(\d+)"), num(r"(\d+)-layer"), num(r"heads=(\d+)"), num(r"dim-inner=(\d+)"), t_src,
            num(r"T_tgt=(\d+)"))


def _time(fns, rounds, calls):
    import numpy as np
    import torch
    times = {k: [] for k, _ in fns}
    for _ in range(rounds):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / calls * 1e3)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def measure(rounds):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)
    from asr_hip import ops
    B, T, D, layers, heads, inner, t_src, t_tgt = baseline_shape()
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    cd = torch.bfloat16
    ops.set_compute_dtype(cd)
    M = B * T
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, u, dv = rnd(M, D).to(dev, cd), rnd(M, 2 * D).to(dev, cd), rnd(M, D).to(dev, cd)
    W1, W2 = (rnd(2 * D, D) * D ** -0.5).to(dev, cd), (rnd(D, D) * D ** -0.5).to(dev, cd)
    b1, b2, gamma, beta = rnd(2 * D).to(dev), rnd(D).to(dev), torch.ones(D, device=dev), torch.zeros(D, device=dev)
    dW1, dW2, db1, db2 = torch.zeros(2 * D, D, device=dev), torch.zeros(D, D, device=dev), torch.zeros(2 * D, device=dev), torch.zeros(D, device=dev)
    dgamma, dbeta = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    y = rnd(M, D).to(dev, cd)
    zz = y.clone()
    _, mean, rstd = ops.add_ln_fwd(zz, x, gamma, beta)
    gemm = [("pointwise_1 fwd", lambda: ops.gemm_nt(x, W1, bias=b1)), ("pointwise_2 fwd", lambda: ops.gemm_nt(x, W2, bias=b2)),
            ("add_ln fwd", lambda: ops.add_ln_fwd(y, x, gamma, beta)),
            ("pointwise_1 dgrad", lambda: ops.gemm_nn(u, W1)), ("pointwise_2 dgrad", lambda: ops.gemm_nn(dv, W2)),
            ("pointwise_1 wgrad", lambda: ops.gemm_tn(u, x, dW1, colsum_acc=db1)), ("pointwise_2 wgrad", lambda: ops.gemm_tn(dv, x, dW2, colsum_acc=db2)),
            ("add_ln bwd", lambda: ops.add_ln_bwd(dv, zz, mean, rstd, gamma, None, dgamma, dbeta))]
    print("BASELINE configs[1] encoder shape: B %d T' %d D %d, bf16; %d x %d calls" % (B, T, D, rounds, CALLS))
    for K in (15, 31):
        wd, bd = (rnd(D, 1, K) * K ** -0.5).to(dev), rnd(D).to(dev)
        dwd, dbd = torch.zeros(D * K, device=dev), torch.zeros(D, device=dev)
        s, v = ops.convmod_fwd(u, wd, bd, lens, B, T, D, K)
        new = [("asr_convmod_fwd", lambda: ops.convmod_fwd(u, wd, bd, lens, B, T, D, K)),
               ("asr_convmod_bwd_data", lambda: ops.convmod_bwd_data(dv, s, u, wd, lens, B, T, D, K)),
               ("asr_convmod_bwd_weight", lambda: ops.convmod_bwd_weight(dv, s, u, lens, B, T, D, K, dwd, dbd))]
        fns = new + gemm
        for _, fn in fns:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        res = _time(fns, rounds, CALLS)
        assert torch.isfinite(v.float()).all() and torch.isfinite(dwd).all()
        for k, _ in fns:
            print("K %2d %-24s median %7.1f us per call (min %.1f max %.1f)" % ((K, k) + res[k]))
        t_new = sum(res[k][0] for k, _ in new)
        t_gemm = sum(res[k][0] for k, _ in gemm if k.startswith("pointwise"))
        t_ln = sum(res[k][0] for k, _ in gemm if k.startswith("add_ln"))
        # bytes each new kernel must move at least once (bf16): fwd reads u, writes s and v; bwd_data reads dv, s, u, writes du;
        # bwd_weight reads dv, s, u
        mb = [M * D * 2 * x_ / 1e6 for x_ in (4, 6, 4)]
        print("K %2d the three new launches %.1f us; the module's pointwise GEMMs (2 fwd, 2 dgrad, 2 wgrad) %.1f us; add_ln fwd + bwd %.1f us; "
              "new / GEMMs = %.2f; share of the module %.0f %%" % (K, t_new, t_gemm, t_ln, t_new / t_gemm, 100 * t_new / (t_new + t_gemm + t_ln)))
        print("K %2d minimum traffic %.1f / %.1f / %.1f MB -> %s TB/s" % ((K,) + tuple(mb) + (
            " / ".join("%.2f" % (b_ / res[k][0]) for b_, (k, _) in zip(mb, new)),)))

    # the eager training step of the configs[1] model, with and without the module
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    from utils.metrics import calculate_loss
    V = 4364
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x4E00 + i) for i in range(V - 3)]
    l2i = {c: i for i, c in enumerate(chars)}
    i2l = {i: c for c, i in l2i.items()}
    src = torch.randn(B, 1, 161, t_src, generator=g).to(dev)
    tgt = torch.randint(3, V, (B, t_tgt - 1), generator=g).to(dev)
    src_len = torch.full((B,), t_src, dtype=torch.int32)
    steps = {}
    for K in (0, 15, 31):
        flags = ["--num-layers", str(layers), "--num-heads", str(heads), "--dim-model", str(D), "--dim-key", "64", "--dim-value", "64",
                 "--dim-inner", str(inner), "--dim-emb", str(D), "--feat_extractor", "vgg_cnn", "--tgt-max-len", str(t_tgt), "--src-max-len",
                 str(t_src), "--label-smoothing", "0.1", "--dropout", "0.1", "--precision", "bf16", "--cuda", "--conv-module-kernel", str(K)]
        args = constant.parse(flags)
        torch.manual_seed(123456)
        model = init_transformer_model(args, l2i, i2l).cuda().train()
        opt = init_optimizer(args, model, "noam")

        def step():
            opt.zero_grad()
            pred, gold, _, _ = model(src, src_len, tgt)
            ops.backward_from(calculate_loss(pred, gold, smoothing=0.1, loss_type="ce"))
            opt.step()

        for _ in range(5):
            step()
        torch.cuda.synchronize()
        steps[K] = _time([("step", step)], rounds, STEP_CALLS)["step"]
        print("eager training step, --conv-module-kernel %2d: median %8.1f us (min %.1f max %.1f, %d x %d steps)"
              % ((K,) + steps[K] + (rounds, STEP_CALLS)))
        del model, opt
    for K in (15, 31):
        print("K %2d adds %.1f us per step (%.1f %%), %.1f us per encoder layer" % (K, steps[K][0] - steps[0][0],
                                                                                   100 * (steps[K][0] / steps[0][0] - 1), (steps[K][0] - steps[0][0]) / layers))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
    else:
        rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # (a fresh child: this process never touches the device)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(rounds)])
        sys.exit(r.returncode)
