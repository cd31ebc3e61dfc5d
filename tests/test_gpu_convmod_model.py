"""--conv-module-kernel through the model on the MI355X: the tiny vgg model of tests/test_gpu_model.py with a ConvolutionModule in
every encoder layer (seeded random module weights), against the same model whose ConvolutionModule.forward is the plain-torch autograd
composition of tests/convmod_reference.py -- everything else runs the same kernels; then the captured step, the data-parallel ready
marks, evaluation and the checkpoint round trip, and the flag switched off."""
import os

import numpy as np
import pytest
import torch

import convmod_reference as R

pytestmark = pytest.mark.gpu

K = 7


def _labels(V):
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x4E00 + i) for i in range(V - 3)]
    return {c: i for i, c in enumerate(chars)}, {i: c for i, c in enumerate(chars)}


def build(golden_dir, precision, kernel=K, extra=()):
    """vgg_tiny's reference weights and batch; the modules' parameters (absent from the golden file) drawn from a seeded generator."""
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    z = np.load(os.path.join(golden_dir, "vgg_tiny.npz"))
    flags = str(z["flags"]).split()
    for k, v in zip(extra[::2], extra[1::2]):
        flags[flags.index(k) + 1] = v
    args = constant.parse(flags + ["--precision", precision, "--cuda"] + (["--conv-module-kernel", str(kernel)] if kernel is not None else []))
    l2i, i2l = _labels(int(z["V"]))
    model = init_transformer_model(args, l2i, i2l)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w0/")}
    if "decoder.positional_encoding.pe" in sd and sd["decoder.positional_encoding.pe"].shape != model.decoder.positional_encoding.pe.shape:
        del sd["decoder.positional_encoding.pe"]                     # (a longer --tgt-max-len: the sinusoid table is the model's own)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all("conv_module" in k or k.endswith(".pe") for k in res.missing_keys)
    g = torch.Generator().manual_seed(2020)
    for name, p in model.named_parameters():
        if "conv_module" in name:
            scale = 0.3 if p.dim() > 1 else 0.1
            with torch.no_grad():
                p.copy_((1.0 if name.endswith("layer_norm.weight") else 0.0) + scale * torch.randn(p.shape, generator=g))
    model = model.cuda().train()
    return z, args, model, init_optimizer(args, model, "noam")


def _batch(z):
    return torch.from_numpy(z["src"]).cuda(), torch.from_numpy(z["src_len"]), torch.from_numpy(z["tgt"]).cuda()


def _step(model, opt, z):
    from utils.metrics import calculate_metrics
    src, src_len, tgt = _batch(z)
    opt.zero_grad()
    pred, gold, hyp, _ = model(src, src_len, tgt)
    loss, _ = calculate_metrics(pred, gold, smoothing=float(z["smoothing"]), loss_type="ce")
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {k: p.grad.detach().double().cpu().numpy().copy() for k, p in model.named_parameters()}


def _torch_arm(monkeypatch):
    from models.common_layers import ConvolutionModule
    monkeypatch.setattr(ConvolutionModule, "forward", lambda self, x, key_len=None, row_keep=None: R.torch_module_forward(self, x, key_len, row_keep))


def test_model_parity_fp32_against_the_torch_composition(golden_dir, monkeypatch):
    z, _, model, opt = build(golden_dir, "fp32")
    loss, grads = _step(model, opt, z)
    _torch_arm(monkeypatch)
    z, _, model_t, opt_t = build(golden_dir, "fp32")
    loss_t, grads_t = _step(model_t, opt_t, z)
    print("loss %.7f  torch arm %.7f" % (loss, loss_t))
    assert abs(loss - loss_t) < 2e-5
    assert sum("conv_module" in k for k in grads) == 16
    worst = 0.0
    for k, g in grads.items():
        if k.endswith("key_linear.bias"):
            continue
        tol = 1e-6 + 2e-4 * np.abs(grads_t[k]).max()
        worst = max(worst, float(np.abs(g - grads_t[k]).max() / tol))
        np.testing.assert_allclose(g, grads_t[k], rtol=0, atol=tol, err_msg=k)
        if "conv_module" in k:
            assert np.abs(grads_t[k]).max() > 1e-6, k                # the module is live: no gradient of it is trivially zero
    print("worst |g - g_torch| / (2e-4 max|g| + 1e-6) = %.3f" % worst)


def test_model_parity_bf16_against_the_torch_composition(golden_dir, monkeypatch):
    z, _, model, opt = build(golden_dir, "bf16")
    loss, grads = _step(model, opt, z)
    _torch_arm(monkeypatch)
    z, _, model_t, opt_t = build(golden_dir, "bf16")
    loss_t, grads_t = _step(model_t, opt_t, z)
    print("loss %.5f  torch arm %.5f" % (loss, loss_t))
    assert abs(loss - loss_t) < 3e-2
    bad, low = [], 1.0
    for k, g in grads.items():
        g, r = g.ravel(), grads_t[k].ravel()
        if np.linalg.norm(r) < 1e-6 or k.endswith("key_linear.bias"):
            continue
        cos = float(g @ r / (np.linalg.norm(g) * np.linalg.norm(r) + 1e-30))
        low = min(low, cos)
        if cos < 0.98:
            bad.append((k, cos))
    print("lowest gradient cosine %.5f" % low)
    assert not bad, bad


def test_graph_replay_equals_eager_steps(golden_dir):
    from asr_hip.graph import GraphedTrainStep
    from utils.metrics import calculate_loss
    z, _, m1, o1 = build(golden_dir, "fp32")
    src, src_len, tgt = _batch(z)
    sm = float(z["smoothing"])
    losses = []
    for _ in range(4):
        o1.zero_grad()
        pred, gold, _, _ = m1(src, src_len, tgt)
        loss = calculate_loss(pred, gold, smoothing=sm)
        loss.backward()
        o1.step()
        losses.append(loss.item())
    z, _, m2, o2 = build(golden_dir, "fp32")
    gs = GraphedTrainStep(m2, o2, sm, src, src_len, tgt, warmup_steps=1)       # 1 eager + 1 replayed step
    assert o2._step == 2 and abs(gs.loss.item() - losses[1]) < 2e-5
    for k in (2, 3):
        loss, _ = gs(src, src_len, tgt)
        assert abs(loss.item() - losses[k]) < 5e-5, (k, loss.item(), losses[k])
    assert o2._step == 4
    moved = 0.0
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if k.endswith("key_linear.bias"):
            continue
        assert torch.allclose(a, b, atol=1e-5), k
    w0 = build(golden_dir, "fp32")[2].state_dict()
    for k, a in m2.state_dict().items():
        if "conv_module" in k:
            moved = max(moved, (a - w0[k]).abs().max().item())
    assert moved > 1e-5                                              # the replayed steps trained the modules


def test_trainer_takes_the_graph_path(golden_dir, monkeypatch):
    from trainer.asr.trainer import Trainer
    from utils import constant
    z, _, m, o = build(golden_dir, "fp32")
    monkeypatch.setattr(constant.args, "graph_buckets", 16, raising=False)
    monkeypatch.setattr(constant, "USE_CUDA", True, raising=False)
    i2l = {i: chr(0x61 + i % 26) for i in range(int(z["V"]))}
    src, tgt = torch.from_numpy(z["src"]), torch.from_numpy(z["tgt"])
    data = (src, tgt, torch.ones(src.shape[0]), torch.from_numpy(z["src_len"]), torch.full((src.shape[0],), tgt.shape[1], dtype=torch.int32))
    tr = Trainer()
    out = []
    for _ in range(3):
        r = tr._run_batch(m, data, float(z["smoothing"]), "ce", i2l, o)
        out.append(r.result() if hasattr(r, "result") else r)
    assert len(tr._graphs) == 1 and o._step == 3
    assert all(r[0] == r[0] for r in out) and out[-1][0] < out[0][0]


def test_every_module_parameter_is_marked_ready_once_per_backward(golden_dir):
    from asr_hip import params as P
    from models.common_layers import ConvolutionModule
    z, _, model, opt = build(golden_dir, "bf16")

    class Recorder:
        active = False            # (no exchange: the step keeps its single-GPU launch sequence, only the ready marks are recorded)

        def __init__(self):
            self.seen = []

        def mark_ready(self, p):
            self.seen.append(id(p))

    rec = Recorder()
    P.set_reducer(rec)
    try:
        _step(model, opt, z)
    finally:
        P.set_reducer(None)
    mods = [m for m in model.modules() if isinstance(m, ConvolutionModule)]
    assert len(mods) == 2
    for m in mods:
        ps = list(m.parameters())
        assert len(ps) == 8
        for p in ps:
            assert rec.seen.count(id(p)) == 1


def test_evaluation_and_checkpoint_round_trip(golden_dir, tmp_path):
    from utils import constant
    from utils.functions import load_model, save_model
    z, args, model, opt = build(golden_dir, "fp32", extra=("--tgt-max-len", "301"))
    src, src_len, tgt = _batch(z)
    model.eval()
    _, hyps, gold = model.evaluate(src, src_len, tgt)
    assert len(hyps) == len(gold) == 3 and all(isinstance(h, str) for h in hyps)
    with torch.no_grad():
        logits = model(src, src_len, tgt)[0]
    args.save_folder, args.name = str(tmp_path), "ck"
    l2i, i2l = _labels(int(z["V"]))
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l, best_model=False)
    flags = str(z["flags"]).split()
    flags[flags.index("--tgt-max-len") + 1] = "301"
    constant.parse(flags + ["--precision", "fp32", "--cuda"])        # the resumed run types no --conv-module-kernel
    m2, _, _, _, a2, _, _ = load_model(os.path.join(str(tmp_path), "ck", "epoch_1.th"))
    assert a2.conv_module_kernel == K and hasattr(m2.encoder.layers[1], "conv_module")
    m2.eval()
    with torch.no_grad():
        logits2 = m2(src, src_len, tgt)[0]
    assert torch.equal(logits, logits2)


def test_flag_off_is_the_parent_model_and_launches_nothing_new(golden_dir, monkeypatch):
    from asr_hip import ops
    z, _, plain, _ = build(golden_dir, "fp32", kernel=None)
    keys = list(plain.state_dict().keys())
    assert set(keys) == {k[3:] for k in z.files if k.startswith("w0/")}        # the reference's own key set
    z, _, off, opt = build(golden_dir, "fp32", kernel=0)
    assert list(off.state_dict().keys()) == keys and not any("conv_module" in k for k in keys)
    calls = [0]
    for name in ("convmod_fwd", "convmod_bwd_data", "convmod_bwd_weight"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, **k: (calls.__setitem__(0, calls[0] + 1), _real(*a, **k))[1])
    loss, _ = _step(off, opt, z)
    assert calls[0] == 0 and abs(loss - float(z["loss"])) < 2e-5      # the parent's golden loss
    z, _, on, opt_on = build(golden_dir, "fp32")
    _step(on, opt_on, z)
    assert calls[0] == 3 * 2                                          # three launches per module, two encoder layers
