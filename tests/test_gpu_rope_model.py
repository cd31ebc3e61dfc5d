"""--pos-encoding rope through the model on the MI355X: the self-attention sub-layer against the float64 restatement of
tests/rope_reference.py on both arms of MHAFn (one fused Q|K|V GEMM, three GEMMs), the tiny vgg model of tests/test_gpu_model.py against
the same model whose asr_hip.ops.rope_ is the fp32 torch restatement, batch invariance of the encoder, the captured step, the joint
CTC step, the convolution module, the data-parallel ready marks, decoding, the checkpoint round trip, and the flag switched off.

The bound of the fp32 comparisons, per tensor: four times the error of the SAME composition in plain fp32 torch on the GPU against the
float64 one, and at least one fp32 rounding (2^-24) of the tensor's largest magnitude."""
import os

import numpy as np
import pytest
import torch

import rope_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore():
    from asr_hip import ops
    from utils import constant
    keep = (constant.args, constant.explicit, constant.USE_CUDA, ops.compute_dtype())
    yield
    constant.args, constant.explicit, constant.USE_CUDA = keep[:3]
    ops.set_compute_dtype(keep[3])


def _bound(e32, ref):
    return max(4.0 * e32, 2.0 ** -24 * ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ the sub-layer
def _block(H, dk, D, fused, seed):
    """A MultiHeadAttention in fp32 mode with seeded weights.  fused: its parameters re-homed into one flat buffer with Q, K, V weights
    and biases adjacent, the layout the optimiser gives a model and the one GEMM for Q|K|V needs."""
    from asr_hip import ops
    from asr_hip import params as P
    from models.common_layers import MultiHeadAttention
    ops.set_compute_dtype(torch.float32)
    mha = MultiHeadAttention(H, D, dk, dk, dropout=0.1)
    g = torch.Generator().manual_seed(seed)
    sd = mha.state_dict()
    for name in R.PARAMS:
        p = sd[name]
        p.copy_((1.0 if name == "layer_norm.weight" else 0.0) + (0.3 if p.dim() > 1 else 0.1) * torch.randn(p.shape, generator=g))
    mha = mha.cuda().eval()
    named = dict(mha.named_parameters())
    flat = None
    if fused:
        order = [named[n] for n in ("query_linear.weight", "key_linear.weight", "value_linear.weight", "query_linear.bias", "key_linear.bias",
                                    "value_linear.bias", "output_linear.weight", "output_linear.bias", "layer_norm.weight", "layer_norm.bias")]
        flat = P.FlatParams(order, order=order)
    return mha, [named[n] for n in R.PARAMS], flat


# (B, T, H, dk, D, the arm a flat layout gives): H dk = 32 does not fill a 64-element slot of the flat buffer, so its biases are not
# adjacent and no fused arm exists at that shape; H 4 is there to have the fused arm at head width 16 as well
BLOCK_SHAPES = [(2, 19, 2, 16, 32, "unfused"), (2, 19, 4, 16, 32, "fused"), (2, 40, 5, 64, 64, "fused")]


@pytest.mark.parametrize("start", [0, 37])
@pytest.mark.parametrize("flat_layout", [False, True])
@pytest.mark.parametrize("B,T,H,dk,D,flat_arm", BLOCK_SHAPES)
def test_block_parity_fp32_against_float64(B, T, H, dk, D, flat_arm, flat_layout, start, monkeypatch):
    from asr_hip import ops
    mha, params, flat = _block(H, dk, D, flat_layout, seed=100 + H)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, D, generator=gen)
    dout = torch.randn(B, T, D, generator=gen)
    lens = torch.tensor([T, T - 8], dtype=torch.int32)
    cs = ops.rope_table(start + T, dk)[start:]
    calls = []
    real = ops.rope_
    monkeypatch.setattr(ops, "rope_", lambda t, c, nheads, d, inverse=False: (calls.append((nheads, inverse)), real(t, c, nheads, d, inverse))[1])

    xd = x.cuda().requires_grad_(True)
    for p in params:
        p.grad = None if flat is None else p.grad.zero_()
    out, _ = mha(xd, xd, xd, key_len=lens.cuda(), row_keep=ops.length_mask(lens.cuda(), T), need_attn=False, rope=cs.cuda())
    out.backward(dout.cuda())
    ops.join_deferred()
    torch.cuda.synchronize()
    arm = flat_arm if flat_layout else "unfused"
    want = [(2 * H, False), (2 * H, True)] if arm == "fused" else [(H, False), (H, False), (H, True), (H, True)]
    assert calls == want, (arm, calls)                                  # the arm under test is the arm that ran; V is never rotated
    got = [out.detach(), xd.grad] + [p.grad for p in params]

    def compose(dtype, device):
        xs = x.to(device, dtype).requires_grad_(True)
        ws = [p.detach().to(device, dtype).requires_grad_(True) for p in params]
        o = R.mha_block(xs, ws, cs.to(device, dtype), H, dk, lens)
        o.backward(dout.to(device, dtype))
        return [t.double().cpu() for t in [o.detach(), xs.grad] + [w.grad for w in ws]]

    ref, t32 = compose(torch.float64, "cpu"), compose(torch.float32, "cuda")
    worst = 0.0
    for name, g, r, t in zip(("out", "dx") + R.PARAMS, got, ref, t32):
        if name == "key_linear.bias":                                   # its true gradient is zero (softmax is shift invariant)
            continue
        e, e32 = (g.double().cpu() - r).abs().max().item(), (t - r).abs().max().item()
        bound = _bound(e32, r)
        worst = max(worst, e / bound)
        print("%-22s e %.3e  e_torch32 %.3e  bound %.3e  ratio %.3f" % (name, e, e32, bound, e / bound))
        assert e <= bound, (name, e, e32, bound)
        assert r.abs().max().item() > 1e-3, name
    assert not out[1, T - 8:].any()
    print("%s start %d %s: worst ratio %.3f" % ((B, T, H, dk), start, arm, worst))


# ------------------------------------------------------------------------------------------------ the model
def _labels(V):
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x4E00 + i) for i in range(V - 3)]
    return {c: i for i, c in enumerate(chars)}, {i: c for i, c in enumerate(chars)}


def build(golden_dir, precision, pos="rope", extra=(), more=()):
    """vgg_tiny's reference weights and batch under --pos-encoding `pos`; parameters the golden file does not have (a convolution module,
    the CTC head) are drawn from a seeded generator."""
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    z = np.load(os.path.join(golden_dir, "vgg_tiny.npz"))
    flags = str(z["flags"]).split()
    for k, v in zip(extra[::2], extra[1::2]):
        flags[flags.index(k) + 1] = v
    args = constant.parse(flags + ["--precision", precision, "--cuda"] + (["--pos-encoding", pos] if pos is not None else []) + list(more))
    l2i, i2l = _labels(int(z["V"]))
    model = init_transformer_model(args, l2i, i2l)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w0/")}
    if "decoder.positional_encoding.pe" in sd and sd["decoder.positional_encoding.pe"].shape != model.decoder.positional_encoding.pe.shape:
        del sd["decoder.positional_encoding.pe"]
    res = model.load_state_dict(sd, strict=False)
    new = lambda k: "conv_module" in k or k.startswith("ctc_linear")
    assert not res.unexpected_keys and all(new(k) or k.endswith(".pe") for k in res.missing_keys)
    g = torch.Generator().manual_seed(2021)
    for name, p in model.named_parameters():
        if new(name):
            with torch.no_grad():
                p.copy_((1.0 if name.endswith("layer_norm.weight") else 0.0) + (0.3 if p.dim() > 1 else 0.1) * torch.randn(p.shape, generator=g))
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


def _count_rope(monkeypatch):
    from asr_hip import ops
    calls = []
    real = ops.rope_
    monkeypatch.setattr(ops, "rope_", lambda t, c, nheads, d, inverse=False: (calls.append(inverse), real(t, c, nheads, d, inverse))[1])
    return calls


def _torch_arm(monkeypatch):
    from asr_hip import ops
    monkeypatch.setattr(ops, "rope_", R.torch_rope_)


def test_model_parity_fp32_against_the_torch_arm(golden_dir, monkeypatch):
    with monkeypatch.context() as mp:
        calls = _count_rope(mp)
        z, _, model, opt = build(golden_dir, "fp32")
        loss, grads = _step(model, opt, z)
    assert len(calls) == 2 * 4 and sum(calls) == 4         # two encoder layers on the unfused arm (H dk = 32): Q and K, forward and inverse
    _torch_arm(monkeypatch)
    z, _, model_t, opt_t = build(golden_dir, "fp32")
    loss_t, grads_t = _step(model_t, opt_t, z)
    print("loss %.7f  torch arm %.7f  (abs model: %.7f)" % (loss, loss_t, float(z["loss"])))
    assert abs(loss - loss_t) < 2e-5
    assert abs(loss - float(z["loss"])) > 1e-4                           # the position signal is another one: not the golden loss
    worst = 0.0
    for k, g in grads.items():
        if k.endswith("key_linear.bias"):
            continue
        tol = 1e-6 + 2e-4 * np.abs(grads_t[k]).max()
        worst = max(worst, float(np.abs(g - grads_t[k]).max() / tol))
        np.testing.assert_allclose(g, grads_t[k], rtol=0, atol=tol, err_msg=k)
    assert np.abs(grads["encoder.layers.0.self_attn.query_linear.weight"]).max() > 1e-6
    print("worst |g - g_torch| / (2e-4 max|g| + 1e-6) = %.3f" % worst)


def test_model_parity_bf16_against_the_torch_arm(golden_dir, monkeypatch):
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


def _encoder_rows(enc, x, lens, dtype, device):
    """The rope encoder in eval mode as a plain-torch composition in `dtype`: input projection + LayerNorm (no sinusoid), then per layer the
    block of tests/rope_reference.py and the feed-forward sub-layer, rows at and behind an utterance's length zeroed after each."""
    F = torch.nn.functional
    c = lambda t: t.detach().to(device, dtype)
    B, T, _ = x.shape
    keep = (torch.arange(T)[None, :] < lens.long()[:, None])[:, :, None].to(device, dtype)
    h = F.layer_norm(c(x) @ c(enc.input_linear.weight).t() + c(enc.input_linear.bias), (enc.dim_model,), c(enc.layer_norm_input.weight),
                     c(enc.layer_norm_input.bias), 1e-5)
    cs = c(enc.rope_cs[:T])
    for layer in enc.layers:
        sa = dict(layer.self_attn.named_parameters())
        h = R.mha_block(h, [c(sa[n]) for n in R.PARAMS], cs, enc.num_heads, enc.dim_key, lens)
        ff = layer.pos_ffn
        y = torch.relu(h @ c(ff.conv_1.weight)[:, :, 0].t() + c(ff.conv_1.bias)) @ c(ff.conv_2.weight)[:, :, 0].t() + c(ff.conv_2.bias)
        h = F.layer_norm(y + h, (enc.dim_model,), c(ff.layer_norm.weight), c(ff.layer_norm.bias), 1e-5) * keep
    return h.double().cpu()


def test_encoder_rows_do_not_depend_on_the_batch_around_them(golden_dir):
    """An utterance of 11 frames alone and padded to 19 beside a longer one: the same rows, within the bound of the fp32 comparisons taken
    over the whole encoder (two blocks and their feed-forward sub-layers), and both within it of the float64 composition."""
    z, _, model, _ = build(golden_dir, "fp32")
    enc = model.encoder.eval()
    x = torch.randn(2, 19, enc.dim_input, generator=torch.Generator().manual_seed(9))
    x[1, 11:] = 1e3                                                      # padding frames must not matter, whatever they hold
    lens = torch.tensor([19, 11])
    with torch.no_grad():
        pair = enc(x.cuda(), lens)[0].double().cpu()
        alone = enc(x[1:, :11].contiguous().cuda(), lens[1:])[0].double().cpu()
        ref = _encoder_rows(enc, x, lens, torch.float64, "cpu")
        e32 = (_encoder_rows(enc, x, lens, torch.float32, "cuda") - ref).abs().max().item()
    bound = _bound(e32, ref)
    e_pair, e_alone, diff = (pair - ref).abs().max().item(), (alone[0] - ref[1, :11]).abs().max().item(), (alone[0] - pair[1, :11]).abs().max().item()
    print("e_torch32 %.3e bound %.3e: pair %.3f alone %.3f alone-vs-pair %.3f of it" % (e32, bound, e_pair / bound, e_alone / bound, diff / bound))
    assert diff <= bound and e_pair <= bound and e_alone <= bound
    assert not pair[1, 11:].any() and pair[1, :11].abs().max().item() > 0.1


def test_graph_replay_equals_eager_steps(golden_dir, monkeypatch):
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
    calls = _count_rope(monkeypatch)
    gs = GraphedTrainStep(m2, o2, sm, src, src_len, tgt, warmup_steps=1)       # 1 eager + 1 replayed step
    assert len(calls) >= 8                                              # the rotation is in what was captured
    assert o2._step == 2 and abs(gs.loss.item() - losses[1]) < 2e-5
    for k in (2, 3):
        loss, _ = gs(src, src_len, tgt)
        assert abs(loss.item() - losses[k]) < 5e-5, (k, loss.item(), losses[k])
    assert o2._step == 4
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if k.endswith("key_linear.bias"):
            continue
        assert torch.allclose(a, b, atol=1e-5), k


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


def _wide(golden_dir, precision, seed=77):
    """vgg_tiny's batch on a model of its shape with FOUR heads of 16: H dk = 64 fills a slot of the flat parameter buffer, so every encoder
    self-attention runs the one-GEMM Q|K|V arm and the rotation gets the strided Q|K view.  The golden weights do not fit: seeded."""
    from utils import constant
    from utils.functions import init_optimizer, init_transformer_model
    z = np.load(os.path.join(golden_dir, "vgg_tiny.npz"))
    flags = str(z["flags"]).split()
    flags[flags.index("--num-heads") + 1] = "4"
    args = constant.parse(flags + ["--precision", precision, "--cuda", "--pos-encoding", "rope"])
    torch.manual_seed(seed)
    model = init_transformer_model(args, *_labels(int(z["V"]))).cuda().train()
    return z, model, init_optimizer(args, model, "noam")


def test_fused_arm_in_the_model_against_the_torch_arm_and_under_capture(golden_dir, monkeypatch):
    from asr_hip.graph import GraphedTrainStep
    from utils.metrics import calculate_loss
    with monkeypatch.context() as mp:
        calls = _count_rope(mp)
        z, model, opt = _wide(golden_dir, "fp32")
        loss, grads = _step(model, opt, z)
    assert len(calls) == 2 * 2 and sum(calls) == 2                      # two encoder layers, one call forward and one inverse each
    with monkeypatch.context() as mp:
        _torch_arm(mp)
        z, model_t, opt_t = _wide(golden_dir, "fp32")
        loss_t, grads_t = _step(model_t, opt_t, z)
    assert abs(loss - loss_t) < 2e-5
    for k, g in grads.items():
        if not k.endswith("key_linear.bias"):
            np.testing.assert_allclose(g, grads_t[k], rtol=0, atol=1e-6 + 2e-4 * np.abs(grads_t[k]).max(), err_msg=k)
    src, src_len, tgt = _batch(z)
    sm = float(z["smoothing"])
    losses = []
    for _ in range(4):                                                  # (model_t, now on the kernel again: the patch is undone)
        opt_t.zero_grad()
        pred, gold, _, _ = model_t(src, src_len, tgt)
        l = calculate_loss(pred, gold, smoothing=sm)
        l.backward()
        opt_t.step()
        losses.append(l.item())
    gs = GraphedTrainStep(model, opt, sm, src, src_len, tgt, warmup_steps=1)
    assert abs(gs.loss.item() - losses[1]) < 2e-5
    for k in (2, 3):
        l, _ = gs(src, src_len, tgt)
        assert abs(l.item() - losses[k]) < 5e-5, (k, l.item(), losses[k])


def test_joint_ctc_step(golden_dir, monkeypatch):
    from utils.metrics import calculate_joint_loss
    z, _, model, opt = build(golden_dir, "fp32", more=["--ctc-weight", "0.3"])
    calls = _count_rope(monkeypatch)
    src, src_len, tgt = _batch(z)
    tl = torch.tensor([5, 4, 1], dtype=torch.int32)                     # within the 16, 10 and 2 encoder frames of the three utterances
    opt.zero_grad()
    pred, gold, _, _, ctc_logits = model(src, src_len, tgt, return_ctc=True)
    loss, ce, ctc = calculate_joint_loss(model, pred, gold, ctc_logits, tgt, src_len, tl, float(z["smoothing"]), 0.3)
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(loss.item()) and np.isfinite(ctc.item()) and abs(loss.item() - (0.7 * ce.item() + 0.3 * ctc.item())) < 1e-5
    assert len(calls) == 8 and sum(calls) == 4
    assert model.ctc_linear.weight.grad.abs().max().item() > 0
    assert model.encoder.layers[0].self_attn.query_linear.weight.grad.abs().max().item() > 0
    before = model.encoder.layers[0].self_attn.key_linear.weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, model.encoder.layers[0].self_attn.key_linear.weight.detach())


def test_step_with_the_convolution_module(golden_dir, monkeypatch):
    with monkeypatch.context() as mp:
        calls = _count_rope(mp)
        z, _, model, opt = build(golden_dir, "fp32", more=["--conv-module-kernel", "7"])
        loss, grads = _step(model, opt, z)
    assert len(calls) == 8 and hasattr(model.encoder.layers[0], "conv_module")
    _torch_arm(monkeypatch)
    z, _, model_t, opt_t = build(golden_dir, "fp32", more=["--conv-module-kernel", "7"])
    loss_t, grads_t = _step(model_t, opt_t, z)
    assert np.isfinite(loss) and abs(loss - loss_t) < 2e-5
    for k, g in grads.items():
        if not k.endswith("key_linear.bias"):
            np.testing.assert_allclose(g, grads_t[k], rtol=0, atol=1e-6 + 2e-4 * np.abs(grads_t[k]).max(), err_msg=k)
    assert np.abs(grads["encoder.layers.1.conv_module.depthwise.weight"]).max() > 1e-6


def test_every_attention_parameter_is_marked_ready_once_per_backward(golden_dir):
    """--parallel: the reducer hears of each parameter once, after the rotation's backward as before it (no new parameter, no new mark)."""
    from asr_hip import params as P
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
    for layer in model.encoder.layers:
        ps = list(layer.self_attn.parameters())
        assert len(ps) == 10
        for p in ps:
            assert rec.seen.count(id(p)) == 1


def test_evaluation_and_checkpoint_round_trip(golden_dir, tmp_path):
    from utils import constant
    from utils.functions import load_model, save_model
    z, args, model, opt = build(golden_dir, "fp32", extra=("--tgt-max-len", "301"), more=["--ctc-weight", "0.3"])
    src, src_len, tgt = _batch(z)
    model.eval()
    _, hyps, gold = model.evaluate(src, src_len, tgt)                                           # greedy
    assert len(hyps) == len(gold) == 3 and all(isinstance(h, str) for h in hyps)
    _, hyps_b, _ = model.evaluate(src, src_len, tgt, ctc_beam=True, beam_width=4, beam_nbest=1)  # --ctc-beam-search
    assert len(hyps_b) == 3 and all(isinstance(h, str) for h in hyps_b)
    with torch.no_grad():
        logits = model(src, src_len, tgt)[0]
    args.save_folder, args.name = str(tmp_path), "ck"
    l2i, i2l = _labels(int(z["V"]))
    save_model(model, 1, opt, {"valid_loss": 1.0}, l2i, i2l, best_model=False)
    flags = str(z["flags"]).split()
    flags[flags.index("--tgt-max-len") + 1] = "301"
    constant.parse(flags + ["--precision", "fp32", "--cuda"])            # the resumed run types no --pos-encoding
    m2, _, _, _, a2, _, _ = load_model(os.path.join(str(tmp_path), "ck", "epoch_1.th"))
    assert a2.pos_encoding == "rope" and m2.encoder.pos_encoding == "rope" and m2.encoder.rope_cs.is_cuda
    m2.eval()
    with torch.no_grad():
        logits2 = m2(src, src_len, tgt)[0]
    assert torch.equal(logits, logits2)


def test_flag_off_is_the_parent_model_and_launches_nothing_new(golden_dir, monkeypatch):
    from asr_hip import ops
    z, _, rope, _ = build(golden_dir, "fp32")
    keys = list(rope.state_dict().keys())

    def boom(*a, **k):
        raise AssertionError("ops.rope_ called under --pos-encoding abs")

    monkeypatch.setattr(ops, "rope_", boom)
    for pos in (None, "abs"):
        z, _, plain, opt = build(golden_dir, "fp32", pos=pos)
        assert list(plain.state_dict().keys()) == keys and not hasattr(plain.encoder, "rope_cs")
        loss, _ = _step(plain, opt, z)
        assert abs(loss - float(z["loss"])) < 2e-5                       # the parent's golden loss
    with pytest.raises(AssertionError):
        z, _, rope, opt = build(golden_dir, "fp32")
        _step(rope, opt, z)
