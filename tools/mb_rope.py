"""asr_rope (csrc/rope.hip) on the Q|K columns of the fused Q|K|V projection at the encoder shape of BASELINE.json configs[1]
(B 32, T' = T_src / 4 = 200, H heads of 64; bf16), forward and inverse, beside a strided device-to-device copy_ of the same view into
another Q|K|V buffer, which moves the same bytes (reads the view once, writes it once); then the eager training step of that model with
--pos-encoding abs and rope.  HIP events, medians of 7 rounds of 200 calls after warm-up, the launches alternating.  No threshold: the
figures go into DESIGN.md section 7.  The measurement runs in a child process under a time limit of its own, so a hung kernel ends
the run instead of holding the device.
usage: python tools/mb_rope.py [rounds]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mb_convmod import _time, baseline_shape  # noqa: E402

CALLS, LIMIT_S, STEP_CALLS = 200, 300, 20


def measure(rounds):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
    sys.path.insert(0, ROOT)
    from asr_hip import ops
    B, T, D, layers, heads, inner, t_src, t_tgt = baseline_shape()
    dk = 64
    HD = heads * dk
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    cd = torch.bfloat16
    ops.set_compute_dtype(cd)
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, T, 3 * HD, generator=g).to(dev, cd)
    other = torch.empty_like(qkv)
    qk, qk_other = qkv[:, :, :2 * HD], other[:, :, :2 * HD]
    cs = ops.rope_table(T, dk, device=dev)
    fns = [("asr_rope forward", lambda: ops.rope_(qk, cs, 2 * heads, dk)), ("asr_rope inverse", lambda: ops.rope_(qk, cs, 2 * heads, dk, inverse=True)),
           ("copy_ of the view", lambda: qk_other.copy_(qk))]
    for _, fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    res = _time(fns, rounds, CALLS)
    assert torch.isfinite(qkv.float()).all()
    mb = 2 * B * T * 2 * HD * 2 / 1e6                   # the view read once and written once, bf16
    print("BASELINE configs[1] encoder shape: B %d T' %d, Q|K = %d heads of %d in rows of %d, bf16; %d x %d calls" % (B, T, 2 * heads, dk, 3 * HD, rounds, CALLS))
    for k, _ in fns:
        print("%-20s median %6.1f us per call (min %.1f max %.1f)  %.1f MB -> %.2f TB/s" % ((k,) + res[k] + (mb, mb / res[k][0])))
    print("asr_rope / copy_: forward %.2f, inverse %.2f; per encoder layer and step (one forward, one inverse) %.1f us"
          % (res["asr_rope forward"][0] / res["copy_ of the view"][0], res["asr_rope inverse"][0] / res["copy_ of the view"][0],
             res["asr_rope forward"][0] + res["asr_rope inverse"][0]))

    # the eager training step of the configs[1] model under both position signals
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
    for pos in ("abs", "rope"):
        flags = ["--num-layers", str(layers), "--num-heads", str(heads), "--dim-model", str(D), "--dim-key", str(dk), "--dim-value", str(dk),
                 "--dim-inner", str(inner), "--dim-emb", str(D), "--feat_extractor", "vgg_cnn", "--tgt-max-len", str(t_tgt), "--src-max-len",
                 str(t_src), "--label-smoothing", "0.1", "--dropout", "0.1", "--precision", "bf16", "--cuda", "--pos-encoding", pos]
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
        steps[pos] = _time([("step", step)], rounds, STEP_CALLS)["step"]
        print("eager training step, --pos-encoding %-4s: median %8.1f us (min %.1f max %.1f, %d x %d steps)"
              % ((pos,) + steps[pos] + (rounds, STEP_CALLS)))
        del model, opt
    print("rope adds %.1f us per step (%.1f %%), %.1f us per encoder layer" % (steps["rope"][0] - steps["abs"][0],
                                                                              100 * (steps["rope"][0] / steps["abs"][0] - 1),
                                                                              (steps["rope"][0] - steps["abs"][0]) / layers))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        measure(int(sys.argv[2]))
    else:
        rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
        # (a fresh child: this process never touches the device)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(rounds)])
        sys.exit(r.returncode)
