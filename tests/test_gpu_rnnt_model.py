"""The transducer head at the model, trainer, train.py and test.py levels, on a tiny model: D 32, 2 + 2 layers,
V 11, J 16, B 3, a dozen encoder frames.

Gradients: the same step with F_.RnntJointFn and F_.RnntFn swapped for plain torch arithmetic on the same tensors (tanh of a broadcast
sum; a cell-by-cell torch.logaddexp lattice under autograd, tests/rnnt_reference.py), in float64 (the reference) and in fp32 (torch's
own fp32); per tensor |g - g64| <= 4 max(max |g32 - g64|, one fp32 rounding of the largest entry): the rule and the bounds of
tests/test_gpu_mwer_model.py and tests/test_gpu_distill_model.py."""
import math

import numpy as np
import pytest
import torch

import rnnt_reference as R
from test_gpu_mwer_model import CHARS, GOLD, _batch, _corpus, cli, process_wide_random_state_is_left_as_found  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TINY = ("--num-layers 2 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 16 "
        "--src-max-len 64 --dropout 0 --k-lr 20 --warmup 5 --cuda").split()
HEAD = ["--transducer-weight", "0.4", "--transducer-dim-joint", "16"]


def _model(cli, extra, seed=0):
    from utils import constant
    from utils.functions import init_transformer_model
    torch.manual_seed(seed)
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(CHARS)
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(TINY + list(extra)), l2i, {i: c for c, i in l2i.items()}).cuda()


class _Joint:
    def __init__(self, dt):
        self.dt = dt

    def apply(self, e, p):
        return torch.tanh(e.to(self.dt)[:, :, None, :] + p.to(self.dt)[:, None, :, :]).to(e.dtype)


class _Loss:
    def __init__(self, dt):
        self.dt = dt

    def apply(self, pred, gold, frames, lengths, blank):
        x = pred.to(self.dt)
        total = 0.0
        for b in range(x.shape[0]):
            Tb, Ub = int(frames[b]), int(lengths[b])
            total = total + R.nll_autograd(x[b, :Tb, :Ub + 1], [int(v) for v in gold[b, :Ub]], blank) / max(Ub, 1)
        return (total / x.shape[0]).float()


def _grads(model, batch, r, w, swap=None, monkeypatch=None):
    from asr_hip import functions as F_
    src, lengths, tgt, tl = batch
    for p in model.parameters():
        p.grad = None
    kept = {}
    hook = model.encoder.register_forward_hook(lambda mod, args, out: (out[0].retain_grad(), kept.__setitem__("enc", out[0]))[0])
    if swap is not None:
        monkeypatch.setattr(F_, "RnntJointFn", _Joint(swap))
        monkeypatch.setattr(F_, "RnntFn", _Loss(swap))
    try:
        loss, gold_seq, hyp_seq, stats = model.transducer_step(src, lengths, tgt, tl, r, 0.1, ctc_weight=w)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hook.remove()
        if swap is not None:
            monkeypatch.undo()
    out = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    out["enc_out"] = kept["enc"].grad.detach().double().cpu()
    return float(loss.detach()), stats, out, gold_seq, hyp_seq


@pytest.mark.parametrize("w", [0.0, 0.3], ids=["ce", "ce+ctc"])
def test_fp32_step_gradients_against_plain_torch_arithmetic(cli, monkeypatch, w):
    model = _model(cli, HEAD + ["--precision", "fp32"] + (["--ctc-weight", str(w)] if w else [])).train()
    batch = _batch()
    r = 0.4
    loss, stats, g, gold_seq, hyp_seq = _grads(model, batch, r, w)
    loss64, _, g64, _, _ = _grads(model, batch, r, w, torch.float64, monkeypatch)
    loss32, _, g32, _, _ = _grads(model, batch, r, w, torch.float32, monkeypatch)
    assert math.isfinite(loss) and abs(loss - loss64) <= 4 * max(abs(loss32 - loss64), R.EPS32 * abs(loss64)), (loss, loss64, loss32)
    new = ["rnnt_enc.weight", "rnnt_enc.bias", "rnnt_embed.0.weight", "rnnt_embed.1.weight", "rnnt_out.weight", "rnnt_out.bias"]
    assert set(g) == set(g64) == set(g32) and all(k in g for k in new + ["decoder.output_linear.weight", "conv.0.weight"])
    assert ("ctc_linear.weight" in g) == (w > 0)
    worst = ("", 0.0)
    for k in sorted(g):
        b32 = R.bound32(g64[k], g32[k])
        x = R.excess(g[k], g64[k], b32)
        worst = max(worst, (k, x), key=lambda t: t[1])
        assert x <= 1.0, (k, x, b32, float(g64[k].abs().max()))
    print("ctc weight %g: worst gradient error / bound %.3f (%s); loss %.6f (float64 arithmetic %.6f)" % (w, worst[1], worst[0], loss, loss64))
    assert all(float(g64[k].abs().max()) > 0 for k in new) and float(g64["enc_out"].abs().max()) > 0
    # the loss is the definition's: (1 - r) L_existing + r L_rnnt from the step's own terms
    existing = float(stats["ce"]) if not w else (1 - w) * float(stats["ce"]) + w * float(stats["ctc"])
    want = (1 - r) * existing + r * float(stats["rnnt"])
    assert abs(loss - want) <= 1e-5 * abs(want) and float(stats["rnnt"]) > 0
    # ... and the transducer term is the restatement's on the head's own logits
    with torch.no_grad():
        enc = model.encoder(model._features(batch[0]), batch[1])[0]
        logits = model.transducer_logits(enc, batch[2], batch[3]).cpu()
    frames = model.ctc_frame_lengths(batch[1], enc.shape[1])
    assert tuple(logits.shape) == (3, enc.shape[1], 5, 11) and frames == [12, 10, 8]
    r64 = R.loss_and_grad(logits, batch[2].cpu(), frames, batch[3])
    r32 = R.loss_and_grad(logits, batch[2].cpu(), frames, batch[3], dtype=torch.float32)
    assert abs(float(stats["rnnt"]) - float(r64["loss"])) <= 4 * max(abs(float(r32["loss"]) - float(r64["loss"])), R.EPS32 * float(r64["loss"]))
    # what the trainer's metrics get, as from forward(): the gold targets with EOS, PAD up to --tgt-max-len, and an arg-max per position
    want_gold = [y + [2] + [0] * (15 - len(y)) for y in GOLD]
    assert gold_seq.cpu().tolist() == want_gold and hyp_seq.shape == gold_seq.shape


def test_bf16_step_hands_both_gradients_through_the_logit_slot(cli, monkeypatch):
    """bf16: RnntFn claims the slot of the joint's projection and CEFn the decoder's, so both gradients leave as bf16, 64-column padded
    (no fp32 copy); the loss is the fp32 model's within bf16's resolution on this model (the 3e-2 smoke() allows its bf16 step)."""
    from asr_hip import ops
    seen = []
    for name in ("rnnt_bwd", "ce_bwd"):
        orig = getattr(ops, name)

        def spy(*a, _orig=orig, _name=name, **k):
            seen.append((_name, k.get("out_dtype"), k.get("pad")))
            return _orig(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    batch = _batch()
    model = _model(cli, HEAD + ["--precision", "bf16"]).train()
    loss, stats, g, _, _ = _grads(model, batch, 0.4, 0.0)
    assert sorted(seen) == [("ce_bwd", torch.bfloat16, 64), ("rnnt_bwd", torch.bfloat16, 64)], seen
    assert all(bool(torch.isfinite(v).all()) for v in g.values()) and float(g["rnnt_out.weight"].abs().max()) > 0
    assert float(g["rnnt_embed.1.weight"].abs().max()) > 0 and float(g["decoder.output_linear.weight"].abs().max()) > 0
    ref = _model(cli, HEAD + ["--precision", "fp32"]).train()
    loss32, _, _, _, _ = _grads(ref, batch, 0.4, 0.0)
    assert abs(loss - loss32) <= 3e-2 * abs(loss32), (loss, loss32)


def test_a_few_adam_steps_lower_the_float64_transducer_loss_of_a_fixed_batch(cli):
    from utils import constant
    from utils.functions import init_optimizer
    model = _model(cli, HEAD + ["--precision", "fp32", "--k-lr", "2"]).train()
    opt = init_optimizer(constant.args, model, "noam")
    batch = _batch()

    def loss64():
        with torch.no_grad():
            enc = model.encoder(model._features(batch[0]), batch[1])[0]
            logits = model.transducer_logits(enc, batch[2], batch[3]).cpu()
        return float(R.loss_and_grad(logits, batch[2].cpu(), model.ctc_frame_lengths(batch[1], enc.shape[1]), batch[3])["loss"])
    before = loss64()
    for _ in range(4):
        opt.zero_grad()
        loss, _, _, _ = model.transducer_step(batch[0], batch[1], batch[2], batch[3], 0.9, 0.0)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    after = loss64()
    print("float64 transducer loss %.6f -> %.6f after 4 Adam steps" % (before, after))
    assert math.isfinite(before) and after < before


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_greedy_search_on_a_joint_table_set_by_hand(cli, precision):
    """Hand-set parameters: joint dimension 0 carries a frame signal, 1 the last label, 2 the label before it, saturated to +-1 by the
    tanh, so the logits are a table known by hand (tests/test_rnnt_host.py walks it); every margin is 1 or more, which decides in fp32
    and in bf16 alike.  Utterance 0 runs into the max_symbols cut, utterance 1 ends before a frame that would emit, utterance 2 has no
    frame at all."""
    model = _model(cli, ["--transducer-weight", "0.4", "--transducer-dim-joint", "8", "--precision", precision]).eval()
    big = 20.0
    with torch.no_grad():
        for p in (model.rnnt_enc.weight, model.rnnt_enc.bias, model.rnnt_out.weight, model.rnnt_out.bias, model.rnnt_embed[0].weight,
                  model.rnnt_embed[1].weight):
            p.zero_()
        model.rnnt_enc.weight[0, 0] = 1.0
        model.rnnt_embed[0].weight[:, 1] = -big
        model.rnnt_embed[0].weight[3, 1] = big                  # one back is label 3
        model.rnnt_embed[1].weight[:, 2] = -big
        model.rnnt_embed[1].weight[4, 2] = big                  # two back is label 4
        model.rnnt_out.bias.copy_(torch.tensor([1.0, -9, -9, -3, 0, -4] + [-9.0] * 5))
        model.rnnt_out.weight[3, :3] = torch.tensor([3.0, -3.0, 0.0])     # label 3: on frame signal +1 unless it was just emitted
        model.rnnt_out.weight[4, :3] = torch.tensor([-4.0, 0.0, 0.0])     # label 4: on frame signal -1, whatever the history
        model.rnnt_out.weight[5, :3] = torch.tensor([0.0, 0.0, 6.0])      # label 5: when label 4 stands two back (and the frame is quiet)
    enc = torch.zeros(3, 5, 32, device="cuda")
    enc[:, :, 0] = torch.tensor([big, -big, 0.0, big, -big])
    lengths = [5, 3, 0]
    e64 = enc.cpu().double() @ model.rnnt_enc.weight.detach().cpu().double().t() + model.rnnt_enc.bias.detach().cpu().double()
    tables = [m.weight.detach().cpu() for m in model.rnnt_embed]
    w_out, b_out = model.rnnt_out.weight.detach().cpu(), model.rnnt_out.bias.detach().cpu()
    cut = False
    for S in (1, 2, 4):
        want, dec = R.greedy(e64, tables, w_out, b_out, lengths, S)
        assert all(m >= 0.99 for d in dec for _, _, m in d), [min(m for _, _, m in d) for d in dec if d]
        strs, ids = model.transducer_greedy(enc, lengths, max_symbols=S, return_ids=True)
        assert ids == want, (S, ids, want)
        assert strs == ["".join(model.id2label[x] for x in row) for row in want] and ids[2] == [] and len(ids[1]) < len(ids[0])
        for d in dec:
            per_frame = {}
            for t, k, _ in d:
                per_frame[t] = per_frame.get(t, 0) + (k != 0)
            cut |= any(n == S for n in per_frame.values())
            assert all(n <= S for n in per_frame.values())
    assert cut and want[0] != R.greedy(e64, tables, w_out, b_out, lengths, 1)[0][0]
    assert model.transducer_greedy(enc, [0, 0, 0]) == ["", "", ""]


def test_with_weight_0_the_loss_has_the_bits_of_the_model_built_without_the_argument(cli, monkeypatch):
    from asr_hip import ops
    from models.asr.transformer import Transformer
    from utils.metrics import calculate_metrics

    def never(*a, **k):
        raise AssertionError("a transducer kernel was launched with --transducer-weight 0")
    for name in ("rnnt_joint", "rnnt_joint_bwd", "rnnt_fwd", "rnnt_bwd"):
        monkeypatch.setattr(ops, name, never)
    src, lengths, tgt, _ = _batch()
    losses, keys = [], []
    for how in ("flag", "none", "argument"):
        model = _model(cli, ["--precision", "fp32"] + (["--transducer-weight", "0"] if how == "flag" else []))
        if how == "argument":                       # the constructor itself, without the new argument
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            model = Transformer(model.encoder, model.decoder, feat_extractor=model.feat_extractor).cuda()
            model.load_state_dict(sd)
        model.train()
        pred, gold, *_ = model(src, lengths, tgt)
        loss, _ = calculate_metrics(pred, gold, smoothing=0.1, loss_type="ce", sync=False)
        losses.append(loss.detach().cpu())
        keys.append(list(model.state_dict().keys()))
        assert not hasattr(model, "rnnt_out")
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2]) and keys[0] == keys[1] == keys[2]
    assert not any(k.startswith("rnnt") for k in keys[0])


def test_train_py_with_transducer_weight_and_test_py_transducer_greedy(cli, tmp_path, monkeypatch, caplog):
    """train.py --transducer-weight 0.3 for two epochs on the three-utterance manifest (bf16, eager steps, finite losses, the head moves
    and comes back from the checkpoint); test.py's evaluate() with --transducer-greedy then decodes from it."""
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
            "--batch-size", "3", "--num-workers", "0", "--epochs", "2", "--save-every", "1", "--name", "tinyrnnt", "--save-folder",
            str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key", "16", "--dim-value", "16",
            "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64", "--label-smoothing", "0.1", "--dropout",
            "0.1", "--k-lr", "20", "--warmup", "5", "--transducer-weight", "0.3", "--transducer-dim-joint", "16", "--transducer-context", "1"]
    first, calls = {}, []
    init, step = UF.init_transformer_model, Transformer.transducer_step

    def recording_init(*a, **k):
        m = init(*a, **k)
        first["w"] = m.rnnt_out.weight.detach().cpu().clone()
        return m

    def spy(self, *a, **k):
        out = step(self, *a, **k)
        calls.append((self.training, float(out[0].detach()), float(out[3]["rnnt"])))
        return out

    def no_graph(*a, **k):
        raise AssertionError("the transducer step must run eagerly")
    monkeypatch.setattr(UF, "init_transformer_model", recording_init)
    monkeypatch.setattr(Transformer, "transducer_step", spy)
    monkeypatch.setattr(Trainer, "_graph_step", no_graph)
    cli(argv)
    train_mod.main()
    monkeypatch.setattr(UF, "init_transformer_model", init)
    assert constant.args.graph_buckets == 0 and constant.args.precision == "bf16"
    assert len([c for c in calls if c[0]]) == 2 and all(math.isfinite(c[1]) and math.isfinite(c[2]) and c[2] > 0 for c in calls), calls
    assert "the transducer step runs as eager launches" in caplog.text
    path = str(tmp_path / "save" / "tinyrnnt" / "best_model.th")
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert np.isfinite(state["metrics"]["train_loss"]) and np.isfinite(state["metrics"]["valid_loss"])
    a = state["args"]
    assert (a.transducer_weight, a.transducer_dim_joint, a.transducer_context) == (0.3, 16, 1)
    assert not torch.equal(state["model_state_dict"]["rnnt_out.weight"], first["w"]) and "rnnt_embed.1.weight" not in state["model_state_dict"]
    # test.py: no flag but the decoding mode -- the head comes back from the checkpoint's own settings
    cli(["--cuda", "--continue-from", path, "--tgt-max-len", "301", "--batch-size", "3", "--num-workers", "0", "--transducer-greedy",
         "--transducer-max-symbols", "2"])
    model, _, _, _, largs, l2i, _ = UF.load_model(path)
    assert torch.equal(model.rnnt_out.weight.detach().cpu(), state["model_state_dict"]["rnnt_out.weight"])
    test_mod.check_transducer_decoding(constant.args, model)
    test_mod.check_ctc_decoding(constant.args, model)
    from models.common_layers import PositionalEncoding
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    model.decoder.positional_encoding = PositionalEncoding(model.decoder.dim_model, 301).cuda()
    ds = SpectrogramDataset(test_mod.feature_conf(largs), [man], l2i, normalize=True)
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    seen = []
    greedy = Transformer.transducer_greedy

    def recording(self, enc_out, lengths, max_symbols=5, return_ids=False):
        out = greedy(self, enc_out, lengths, max_symbols=max_symbols, return_ids=True)
        seen.append((list(lengths), max_symbols, out[1]))
        return out if return_ids else out[0]
    monkeypatch.setattr(Transformer, "transducer_greedy", recording)
    cer, wer = test_mod.evaluate(model, loader)
    assert np.isfinite(cer) and cer >= 0 and np.isfinite(wer)
    assert len(seen) == 1 and seen[0][1] == 2 and len(seen[0][2]) == 3
    assert all(len(ids) <= 2 * n and all(0 < x < len(l2i) for x in ids) for n, ids in zip(seen[0][0], seen[0][2]))
