"""Pruned transducer training at the model, trainer, train.py and test.py levels, on the tiny model of
tests/test_gpu_rnnt_model.py: D 32, 2 + 2 layers, V 11, J 16, B 3, a dozen encoder frames, U 4, --transducer-prune-range 3.

Gradients: the same step with F_.RnntSimpleFn, F_.RnntJointPrunedFn and F_.RnntPrunedFn swapped for plain torch arithmetic on the same
tensors (the materialised am + lm and the scattered band under a cell-by-cell torch.logaddexp lattice, autograd through an index
gather), in float64 and in fp32, with the band the GPU chose handed to both (a band from float64 occupancies may differ at a tie and is
never compared); per tensor |g - g64| <= 4 max(max |g32 - g64|, one fp32 rounding of the largest entry)."""
import math

import numpy as np
import pytest
import torch

import rnnt_pruned_reference as P
import rnnt_reference as R
from test_gpu_mwer_model import CHARS, GOLD, _batch, _corpus, cli, process_wide_random_state_is_left_as_found  # noqa: F401  (fixtures)
from test_gpu_rnnt_model import HEAD, TINY, _model

pytestmark = pytest.mark.gpu

PRUNED = HEAD + ["--transducer-prune-range", "3"]
SIMPLE_KEYS = ["rnnt_simple_am.weight", "rnnt_simple_am.bias", "rnnt_simple_lm.weight", "rnnt_simple_lm.bias"]
C = 0.5


class _Simple:
    def __init__(self, dt):
        self.dt = dt

    def apply(self, am, lm, gold, frames, lengths, blank):
        a, l = am.to(self.dt), lm.to(self.dt)
        total = 0.0
        for b in range(a.shape[0]):
            Tb, Ub = int(frames[b]), int(lengths[b])
            x = a[b, :Tb, None, :] + l[b, None, :Ub + 1, :]
            total = total + R.nll_autograd(x, [int(v) for v in gold[b, :Ub]], blank) / max(Ub, 1)
        none = torch.zeros((a.shape[0], a.shape[1], l.shape[1]), device=am.device)
        return (total / a.shape[0]).float(), none, none


class _JointPruned:
    def __init__(self, dt):
        self.dt = dt

    def apply(self, e, p, s_begin, W):
        idx = s_begin.long()[:, :, None] + torch.arange(W, device=e.device)[None, None, :]
        rows = torch.arange(e.shape[0], device=e.device)[:, None, None].expand_as(idx)
        return torch.tanh(e.to(self.dt)[:, :, None, :] + p.to(self.dt)[rows, idx]).to(e.dtype)


class _PrunedLoss:
    def __init__(self, dt):
        self.dt = dt

    def apply(self, pred, gold, frames, lengths, s_begin, umax, blank):
        x = pred.to(self.dt)
        s = s_begin.cpu()
        total = 0.0
        for b in range(x.shape[0]):
            Tb, Ub = int(frames[b]), int(lengths[b])
            total = total + P.nll_autograd_band(x[b, :Tb], [int(v) for v in gold[b, :Ub]], s[b], Ub, blank) / max(Ub, 1)
        return (total / x.shape[0]).float()


def _grads(model, batch, r, band=None, swap=None, monkeypatch=None):
    from asr_hip import functions as F_
    from asr_hip import ops
    src, lengths, tgt, tl = batch
    for p in model.parameters():
        p.grad = None
    kept = {}
    hook = model.encoder.register_forward_hook(lambda mod, args, out: (out[0].retain_grad(), kept.__setitem__("enc", out[0]))[0])
    prune = ops.rnnt_prune_ranges

    def spy(*a, **k):
        kept["s"] = prune(*a, **k) if band is None else band
        return kept["s"]
    monkeypatch.setattr(ops, "rnnt_prune_ranges", spy)
    if swap is not None:
        monkeypatch.setattr(F_, "RnntSimpleFn", _Simple(swap))
        monkeypatch.setattr(F_, "RnntJointPrunedFn", _JointPruned(swap))
        monkeypatch.setattr(F_, "RnntPrunedFn", _PrunedLoss(swap))
    try:
        loss, gold_seq, hyp_seq, stats = model.transducer_step(src, lengths, tgt, tl, r, 0.1, simple_scale=C)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hook.remove()
        monkeypatch.undo()
    out = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    out["enc_out"] = kept["enc"].grad.detach().double().cpu()
    return float(loss.detach()), stats, out, kept["s"]


def test_fp32_step_gradients_against_plain_torch_arithmetic_with_the_gpu_s_band(cli, monkeypatch):
    model = _model(cli, PRUNED + ["--precision", "fp32"]).train()
    batch = _batch()
    r = 0.4
    loss, stats, g, s = _grads(model, batch, r, monkeypatch=monkeypatch)
    assert s.dtype == torch.int32 and tuple(s.shape) == (3, 12)
    for b, (Tb, Ub) in enumerate(zip((12, 10, 8), (3, 4, 2))):
        assert Ub + 1 <= 3 or P.band_properties(s[b].cpu(), Tb, Ub, 3), s[b]
    loss64, _, g64, _ = _grads(model, batch, r, s, torch.float64, monkeypatch)
    loss32, _, g32, _ = _grads(model, batch, r, s, torch.float32, monkeypatch)
    assert math.isfinite(loss) and abs(loss - loss64) <= 4 * max(abs(loss32 - loss64), R.EPS32 * abs(loss64)), (loss, loss64, loss32)
    new = ["rnnt_enc.weight", "rnnt_enc.bias", "rnnt_embed.0.weight", "rnnt_embed.1.weight", "rnnt_out.weight", "rnnt_out.bias"] + SIMPLE_KEYS
    assert set(g) == set(g64) == set(g32) and all(k in g for k in new + ["decoder.output_linear.weight", "conv.0.weight"])
    worst = ("", 0.0)
    for k in sorted(g):
        x = R.excess(g[k], g64[k], R.bound32(g64[k], g32[k]))
        worst = max(worst, (k, x), key=lambda t: t[1])
        assert x <= 1.0, (k, x, float(g64[k].abs().max()))
    print("worst gradient error / bound %.3f (%s); loss %.6f (float64 arithmetic %.6f)" % (worst[1], worst[0], loss, loss64))
    assert all(float(g64[k].abs().max()) > 0 for k in new) and float(g64["enc_out"].abs().max()) > 0
    # the loss is the definition's: (1 - r) L_existing + r (L_pruned + c L_simple) from the step's own terms
    rnnt = float(stats["rnnt_pruned"]) + C * float(stats["rnnt_simple"])
    assert abs(float(stats["rnnt"]) - rnnt) <= 1e-6 * rnnt and float(stats["rnnt_simple"]) > 0 and float(stats["rnnt_pruned"]) > 0
    want = (1 - r) * float(stats["ce"]) + r * float(stats["rnnt"])
    assert abs(loss - want) <= 1e-5 * abs(want)


def test_bf16_step_hands_the_band_gradient_through_the_logit_slot(cli, monkeypatch):
    """bf16: RnntPrunedFn claims the slot of rnnt_out and CEFn the decoder's, so both gradients leave as bf16, 64-column padded; the
    simple joiner's two projections get formal fp32 gradients (RnntSimpleFn claims nothing)."""
    from asr_hip import ops
    seen = []
    for name in ("rnnt_pruned_bwd", "ce_bwd", "rnnt_simple_bwd", "rnnt_bwd"):
        orig = getattr(ops, name)

        def spy(*a, _orig=orig, _name=name, **k):
            out = _orig(*a, **k)
            seen.append((_name, k.get("out_dtype"), k.get("pad")) if _name != "rnnt_simple_bwd" else (_name, out[0].dtype, out[1].dtype))
            return out
        monkeypatch.setattr(ops, name, spy)
    batch = _batch()
    model = _model(cli, PRUNED + ["--precision", "bf16"]).train()
    loss, stats, g, _ = _grads(model, batch, 0.4, monkeypatch=monkeypatch)
    assert sorted(seen, key=str) == sorted([("ce_bwd", torch.bfloat16, 64), ("rnnt_pruned_bwd", torch.bfloat16, 64),
                                            ("rnnt_simple_bwd", torch.float32, torch.float32)], key=str), seen
    assert all(bool(torch.isfinite(v).all()) for v in g.values())
    for k in ["rnnt_out.weight", "rnnt_embed.1.weight", "decoder.output_linear.weight"] + SIMPLE_KEYS:
        assert float(g[k].abs().max()) > 0, k
    ref = _model(cli, PRUNED + ["--precision", "fp32"]).train()
    loss32, _, _, _ = _grads(ref, batch, 0.4, monkeypatch=monkeypatch)
    assert abs(loss - loss32) <= 3e-2 * abs(loss32), (loss, loss32)


def _terms64(model, batch):
    """float64 (L_pruned, L_simple) of the model as it stands, on its own fp32 am / lm / band logits, with the band the GPU chooses."""
    from asr_hip import functions as F_
    from asr_hip import ops
    src, lengths, tgt, tl = batch
    with torch.no_grad():
        enc = model.encoder(model._features(src), lengths)[0]
        _, s, W, U, p, (tg, frames, _) = model.transducer_band(enc, lengths, tgt, tl)
        am = F_.linear(enc, model.rnnt_simple_am.weight, model.rnnt_simple_am.bias, True, True)
        lm = F_.linear(p, model.rnnt_simple_lm.weight, model.rnnt_simple_lm.bias, True, True)
        e = F_.linear(enc, model.rnnt_enc.weight, model.rnnt_enc.bias, False, True)
        logits = F_.linear(ops.rnnt_joint_pruned(e.contiguous(), p.contiguous(), s, W), model.rnnt_out.weight, model.rnnt_out.bias, True, True)
    fr = frames.cpu()
    simple = P.simple_loss_and_grad(am.cpu(), lm.cpu(), tg.cpu(), fr, tl)["loss"]
    pruned = P.pruned_loss_and_grad(logits.cpu(), tg.cpu(), fr, tl, s.cpu(), U)["loss"]
    return float(pruned), float(simple)


def test_a_few_adam_steps_lower_the_float64_pruned_loss_of_a_fixed_batch(cli):
    from utils import constant
    from utils.functions import init_optimizer
    model = _model(cli, PRUNED + ["--precision", "fp32", "--k-lr", "2"]).train()
    opt = init_optimizer(constant.args, model, "noam")
    batch = _batch()
    before = _terms64(model, batch)
    for _ in range(4):
        opt.zero_grad()
        loss, _, _, _ = model.transducer_step(batch[0], batch[1], batch[2], batch[3], 0.9, 0.0, simple_scale=C)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    after = _terms64(model, batch)
    print("float64 L_pruned %.6f -> %.6f, L_simple %.6f -> %.6f after 4 Adam steps" % (before[0], after[0], before[1], after[1]))
    assert all(math.isfinite(v) for v in before + after) and after[0] + C * after[1] < before[0] + C * before[1]


def test_a_shape_the_full_lattice_refuses_runs_on_a_band_of_5():
    """B 32, T' 75, U 60 at V 4364: 2.6e9 bytes of joint logits in full (refused), 0.21e9 on the band.  The head's three Functions on
    random e / p and projections, forward and backward."""
    from asr_hip import functions as F_
    from asr_hip import ops
    B, T, U, V, J, S = 32, 75, 60, 4364, 64, 5
    with pytest.raises(ValueError, match="2\\^31"):
        F_.check_rnnt_shape(B, T, U + 1, V)
    g = torch.Generator().manual_seed(0)
    dev = "cuda"
    lengths = torch.randint(40, U + 1, (B,), generator=g, dtype=torch.int32)
    lengths[0] = U
    frames = torch.randint(62, T + 1, (B,), generator=g, dtype=torch.int32)
    tgt = torch.randint(1, V, (B, U), generator=g).to(dev)
    am = (torch.randn((B, T, V), generator=g) * 0.5).to(dev).requires_grad_(True)
    lm = (torch.randn((B, U + 1, V), generator=g) * 0.5).to(dev).requires_grad_(True)
    e = torch.randn((B, T, J), generator=g).to(dev).requires_grad_(True)
    p = torch.randn((B, U + 1, J), generator=g).to(dev).requires_grad_(True)
    w_out = (torch.randn((V, J), generator=g) * 0.1).to(dev).requires_grad_(True)
    simple, gb, gl = F_.RnntSimpleFn.apply(am, lm, tgt, frames, lengths, 0)
    s = ops.rnnt_prune_ranges(gb, gl, frames.to(dev), lengths.to(dev), S)
    z = F_.RnntJointPrunedFn.apply(e, p, s, S)
    logits = z.float() @ w_out.t()
    assert tuple(logits.shape) == (B, T, S, V)
    pruned = F_.RnntPrunedFn.apply(logits, tgt, frames, lengths, s, U, 0)
    (pruned + 0.5 * simple).backward()
    torch.cuda.synchronize()
    sc = s.cpu()
    for b in range(B):
        assert P.band_properties(sc[b], int(frames[b]), int(lengths[b]), S), b
    assert math.isfinite(float(simple.detach())) and math.isfinite(float(pruned.detach())) and float(pruned.detach()) > 0
    for name, t in (("am", am), ("lm", lm), ("e", e), ("p", p), ("w_out", w_out)):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, name


def test_with_the_range_0_the_step_has_the_bits_and_the_keys_of_the_full_lattice_head(cli, monkeypatch):
    from asr_hip import ops

    def never(*a, **k):
        raise AssertionError("a pruned-transducer kernel was launched with --transducer-prune-range 0")
    for name in ("rnnt_simple_fwd", "rnnt_simple_bwd", "rnnt_prune_ranges", "rnnt_joint_pruned", "rnnt_joint_pruned_bwd", "rnnt_pruned_fwd",
                 "rnnt_pruned_bwd"):
        monkeypatch.setattr(ops, name, never)
    batch = _batch()
    out = []
    for extra in ([], ["--transducer-prune-range", "0", "--transducer-simple-scale", "0.3"]):
        model = _model(cli, HEAD + ["--precision", "fp32"] + extra).train()
        loss, _, _, stats = model.transducer_step(batch[0], batch[1], batch[2], batch[3], 0.4, 0.1)
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.detach().cpu(), list(model.state_dict().keys()), stats))
    # (the loss, not the weight gradients: the weight-gradient GEMM of csrc/gemm_tn.hip adds its K slices with atomics, so two runs of the
    # SAME model need not give the same gradient bits)
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert not any(k.startswith("rnnt_simple") for k in out[0][1]) and float(out[0][2]["rnnt_simple"]) == 0.0


def test_train_py_with_prune_range_and_test_py_transducer_greedy(cli, tmp_path, monkeypatch, caplog):
    """train.py --transducer-weight 0.3 --transducer-prune-range 3 for two epochs on the three-utterance manifest (bf16, eager steps,
    finite losses, the simple layers move and come back from the checkpoint); test.py's evaluate() with --transducer-greedy then
    decodes from the head, which ignores the two simple layers."""
    import logging
    import test as test_mod
    import train as train_mod
    import utils.functions as UF
    from models.asr.transformer import Transformer
    from trainer.asr.trainer import Trainer
    from utils import constant
    caplog.set_level(logging.INFO)
    man, lab = _corpus(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--train-manifest-list", man, "--valid-manifest-list", man, "--test-manifest-list", man, "--labels-path", lab, "--cuda",
            "--batch-size", "3", "--num-workers", "0", "--epochs", "2", "--save-every", "1", "--name", "tinypruned", "--save-folder",
            str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key", "16", "--dim-value", "16",
            "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64", "--label-smoothing", "0.1", "--dropout",
            "0.1", "--k-lr", "20", "--warmup", "5", "--transducer-weight", "0.3", "--transducer-dim-joint", "16", "--transducer-context", "1",
            "--transducer-prune-range", "3", "--transducer-simple-scale", "0.25"]
    first, calls = {}, []
    init, step = UF.init_transformer_model, Transformer.transducer_step

    def recording_init(*a, **k):
        m = init(*a, **k)
        first["w"] = m.rnnt_simple_am.weight.detach().cpu().clone()
        return m

    def spy(self, *a, **k):
        out = step(self, *a, **k)
        calls.append((self.training, float(out[0].detach()), float(out[3]["rnnt_pruned"]), float(out[3]["rnnt_simple"]), k.get("simple_scale")))
        return out

    def no_graph(*a, **k):
        raise AssertionError("the pruned transducer step must run eagerly")
    monkeypatch.setattr(UF, "init_transformer_model", recording_init)
    monkeypatch.setattr(Transformer, "transducer_step", spy)
    monkeypatch.setattr(Trainer, "_graph_step", no_graph)
    cli(argv)
    train_mod.main()
    monkeypatch.setattr(UF, "init_transformer_model", init)
    monkeypatch.setattr(Transformer, "transducer_step", step)
    assert constant.args.graph_buckets == 0 and constant.args.precision == "bf16"
    assert len([c for c in calls if c[0]]) == 2 and all(math.isfinite(v) and v > 0 for c in calls for v in c[1:4]), calls
    assert all(c[4] == 0.25 for c in calls)
    assert "the pruned transducer step (--transducer-prune-range 3) runs as eager launches" in caplog.text
    assert "--transducer-prune-range 3: pruned transducer training" in caplog.text
    path = str(tmp_path / "save" / "tinypruned" / "best_model.th")
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert np.isfinite(state["metrics"]["train_loss"]) and np.isfinite(state["metrics"]["valid_loss"])
    a = state["args"]
    assert (a.transducer_weight, a.transducer_prune_range, a.transducer_simple_scale) == (0.3, 3, 0.25)
    assert not torch.equal(state["model_state_dict"]["rnnt_simple_am.weight"], first["w"]) and "rnnt_simple_lm.bias" in state["model_state_dict"]
    # test.py: no flag but the decoding mode -- the head and the simple layers come back from the checkpoint's own settings
    cli(["--cuda", "--continue-from", path, "--tgt-max-len", "301", "--batch-size", "3", "--num-workers", "0", "--transducer-greedy",
         "--transducer-max-symbols", "2"])
    model, _, _, _, largs, l2i, _ = UF.load_model(path)
    assert torch.equal(model.rnnt_simple_am.weight.detach().cpu(), state["model_state_dict"]["rnnt_simple_am.weight"])
    assert largs.transducer_prune_range == 3
    test_mod.check_transducer_decoding(constant.args, model)
    from asr_hip import ops
    from models.common_layers import PositionalEncoding
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset

    def never(*a, **k):
        raise AssertionError("decoding touched the simple joiner")
    for name in ("rnnt_simple_fwd", "rnnt_prune_ranges", "rnnt_joint_pruned", "rnnt_pruned_fwd"):
        monkeypatch.setattr(ops, name, never)
    model.decoder.positional_encoding = PositionalEncoding(model.decoder.dim_model, 301).cuda()
    ds = SpectrogramDataset(test_mod.feature_conf(largs), [man], l2i, normalize=True)
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    cer, wer = test_mod.evaluate(model, loader)
    assert np.isfinite(cer) and cer >= 0 and np.isfinite(wer)
