"""Transducer beam search (csrc/rnnt_beam.hip): what one batch costs on one MI355X at B 32, T' 75 encoder frames
(300 input frames), V 4364, joint width 256, bf16 -- bench.py's model with a transducer head.

1. The search kernel alone (ops.rnnt_beam_search on the model's own tensors), HIP events, medians of `rounds` brackets of 10 calls
   after warm-up, for W 1 / 4 / 8 / 16 with S 2 and S 5 at the default K = 16, as time per batch and per search step (a batch is T' (S + 1)
   steps: no early exit).  The MFMA projection computes all 16 rows whatever W is, the row pass (log-sum-exp, one candidate pass and K selection rounds per
   live row) grows with W and K, so three more lines split a step: (W 1, K 1) is the projection plus the fixed part of a step,
   (W 16, K 1) adds the other rows' log-sum-exp and candidate pass, (W 16, K 16) fifteen more selection rounds.  The same steps at V 64
   leave a step's fixed part: the z rows, the barriers, the beam bookkeeping.
2. Transformer.transducer_beam_search (rnnt_enc GEMM + search + copy + host ranking) for the same W and S, against transducer_greedy
   (5 symbols per frame) and ctc_beam_search at W 8 on the same encoder output: wall-clock medians of 5 calls.
3. bench.py's step with the flag off (`bench.py --gpus 1`), as a child process: its JSON line.
Every measurement runs in a child process under a time limit of its own, so a hung kernel ends the run instead of holding the device.
usage: python tools/mb_rnnt_beam.py [rounds]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, T_SRC, J = 32, 4364, 300, 256
CALLS, LIMIT_S = 10, 420


def _paths():
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)


def _setup(torch):
    import bench
    from utils import constant
    from utils.functions import init_transformer_model
    flags = bench.MODEL_FLAGS + ["--dropout", "0.1", "--precision", "bf16", "--cuda", "--batch-size", str(B), "--ctc-weight", "0.3",
                                 "--transducer-weight", "0.3", "--transducer-dim-joint", str(J)]
    l2i, i2l = bench.labels(V)
    torch.manual_seed(123456)
    model = init_transformer_model(constant.parse(flags), l2i, i2l).cuda().eval()
    src, _, _ = bench.synthetic_batch(B, torch, t_src=T_SRC, t_tgt=21)
    lengths = torch.full((B,), T_SRC, dtype=torch.int64)
    with torch.no_grad():
        enc = model.encoder(model._features(src.cuda()), lengths)[0]
    return model, enc, model.ctc_frame_lengths(lengths, enc.shape[1])


def kernel(rounds):
    import numpy as np
    import torch
    _paths()
    from asr_hip import functions as F_, ops, params as P
    torch.cuda.set_device(0)
    model, enc, frames = _setup(torch)
    T = enc.shape[1]
    with torch.no_grad():
        e = F_.linear(enc, model.rnnt_enc.weight, model.rnnt_enc.bias, False, True).contiguous()
    tables = [P.linear_weight(m.weight, e.dtype) for m in model.rnnt_embed]
    w_out, b_out = P.linear_weight(model.rnnt_out.weight, e.dtype), model.rnnt_out.bias.data
    fl = torch.tensor(frames, dtype=torch.int32, device="cuda")

    def timed(W, K, S, tables=tables, w_out=w_out, b_out=b_out):
        fn = lambda: ops.rnnt_beam_search(e, tables, w_out, b_out, fl, W, K, S, W)      # noqa: E731
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
            out.append(e0.elapsed_time(e1) / CALLS)
        return float(np.median(out))
    print("search kernel alone, B %d T' %d V %d J %d %s, weights %.2f MB per step" % (B, T, V, J, e.dtype, V * J * 2 / 1e6))
    for S in (2, 5):
        for W, K in ((1, 16), (4, 16), (8, 16), (16, 16), (1, 1), (16, 1)):
            ms = timed(W, K, S)
            steps = T * (S + 1)
            print("asr_rnnt_beam_search W %2d K %2d S %d: median %8.3f ms per batch, %7.2f us per search step (%d steps)"
                  % (W, K, S, ms, ms * 1e3 / steps, steps))
    # the same e and steps with a vocabulary of 64 (random parameters): projection and row pass shrink to a sixty-eighth, what is left
    # is a step's fixed part -- the z rows, five barriers, the beam bookkeeping
    g = torch.Generator().manual_seed(1)
    Vs = 64
    small = dict(tables=[torch.randn(Vs, J, generator=g).to("cuda", e.dtype) for _ in tables],
                 w_out=(torch.randn(Vs, J, generator=g) / 16).to("cuda", e.dtype), b_out=torch.randn(Vs, generator=g).cuda())
    for S in (2, 5):
        for W, K in ((1, 1), (16, 16)):
            ms = timed(W, K, S, **small)
            print("asr_rnnt_beam_search W %2d K %2d S %d, V %d: median %8.3f ms per batch, %7.2f us per search step"
                  % (W, K, S, Vs, ms, ms * 1e3 / (T * (S + 1))))


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def decode():
    import numpy as np
    import torch
    _paths()
    torch.cuda.set_device(0)
    model, enc, frames = _setup(torch)
    fns = [("transducer_greedy (5)", lambda: model.transducer_greedy(enc, frames, 5)),
           ("ctc_beam_search W 8", lambda: model.ctc_beam_search(enc, frames, 8)),
           ("ctc_greedy", lambda: model.ctc_greedy(enc, frames))]
    for S in (2, 5):
        for W in (1, 4, 8, 16):
            fns.append(("transducer_beam_search W %2d S %d" % (W, S),
                        lambda W=W, S=S: model.transducer_beam_search(enc, frames, W, nbest=1, max_symbols=S)))
    for k, fn in fns:
        fn()
        ms = [_wall(torch, fn) for _ in range(5)]
        print("decode %-32s B %d T' %d V %d bf16: median %8.2f ms (min %.2f max %.2f, 5 calls)"
              % (k, B, enc.shape[1], V, float(np.median(ms)), min(ms), max(ms)))


def _child(*argv):
    # (a fresh child: this process never touches the device)
    return subprocess.run(["timeout", "-k", "10", str(LIMIT_S)] + list(argv)).returncode


if __name__ == "__main__":
    me = [sys.executable, os.path.abspath(__file__)]
    if len(sys.argv) > 2 and sys.argv[1] == "--child-kernel":
        kernel(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-decode":
        decode()
    else:
        rc = _child(*me, "--child-kernel", sys.argv[1] if len(sys.argv) > 1 else "5")
        if rc == 0:                  # after a fault, a hang or a failure nothing more is started on the device
            rc = _child(*me, "--child-decode")
        if rc == 0:
            print("bench.py --gpus 1 --steps 20 --warmup 5 (the flag-off training step):", flush=True)
            rc = _child(sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5")
        sys.exit(rc)
