"""MWER training over the CTC n-best at the model, trainer and train.py levels, on a tiny model: D 32, 2 + 2 layers,
V 11, B 3, N 3, a dozen encoder frames, fp32 and bf16.

Scores: Decoder._score_rows(differentiable=True) issues the launches of score_hypotheses in the same order (the factoring moved the host
conversion out and nothing else; SeqLogProbFn.forward IS ops.seq_logprob), so the differentiable scores are demanded torch.equal to
score_hypotheses' in eval mode.
Gradients: the same step with the two new Functions swapped for plain torch log_softmax / softmax arithmetic on the same logits, in
float64 (the reference) and in fp32 (torch's own fp32); per tensor |g - g64| <= 4 max(max |g32 - g64|, one fp32 rounding of the largest
entry), the rule of tests/test_gpu_mwer.py.  In bf16 both sides round dlogits to bf16 once, which the fp32-against-float64 term
measures on this very input."""
import json
import math
import os
import wave

import numpy as np
import pytest
import torch

import mwer_reference as R

pytestmark = pytest.mark.gpu

CHARS = "abcdefg "                       # + PAD, SOS, EOS: V = 11
TINY = ("--num-layers 2 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 16 "
        "--src-max-len 64 --dropout 0 --ctc-weight 0.3 --cuda").split()
HYPS = [[[3, 4, 5], [3, 5], [6, 4, 5, 7]], [[8, 9], [8]], [[4], [], [4, 10, 4]]]          # N = 3: 3, 2 and 3 distinct hypotheses
GOLD = [[3, 4, 5], [8, 9, 3, 4], [4, 10]]


@pytest.fixture(autouse=True)
def process_wide_random_state_is_left_as_found():
    """The random generators and the dropout seed counters (asr_hip.params._state, ops.step_state) are process-wide, and the training
    runs of later test files start from them: every test here puts them back."""
    import random
    from asr_hip import ops
    from asr_hip import params as P
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
    seeds = (P._state["seed_ctr"], P._state["base_seed"])
    counters = ops._cfg["state"]
    kept = None if counters is None else counters.clone()
    yield
    torch.cuda.synchronize()
    torch.set_rng_state(rng[0])
    torch.cuda.set_rng_state_all(rng[1])
    np.random.set_state(rng[2])
    random.setstate(rng[3])
    P._state["seed_ctr"], P._state["base_seed"] = seeds
    if counters is None:
        ops._cfg["state"] = None
    else:
        counters.copy_(kept)
        ops._cfg["state"] = counters


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _model(cli, precision, seed=0):
    from utils import constant
    from utils.functions import init_transformer_model
    torch.manual_seed(seed)
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(CHARS)
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(TINY + ["--precision", precision]), l2i, {i: c for c, i in l2i.items()}).cuda()


def _batch():
    g = torch.Generator().manual_seed(3)
    src = torch.randn(3, 1, 161, 48, generator=g)              # 48 input frames: 12 encoder frames
    tgt = torch.zeros(3, 4, dtype=torch.int64)
    for b, y in enumerate(GOLD):
        tgt[b, :len(y)] = torch.tensor(y)
    return src.cuda(), torch.tensor([48, 40, 32]), tgt.cuda(), torch.tensor([len(y) for y in GOLD], dtype=torch.int32)


def _enc(model, src, lengths):
    with torch.no_grad():
        return model.encoder(model._features(src), lengths)[0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_differentiable_scores_equal_score_hypotheses(cli, precision):
    model = _model(cli, precision).eval()
    src, lengths, _, _ = _batch()
    enc = _enc(model, src, lengths)
    both = [[g] + hs for g, hs in zip(GOLD, HYPS)]
    want = model.decoder.score_hypotheses(enc, both)
    out, seg_off, logits, tgt_d = model.decoder._score_rows(enc.detach().clone().requires_grad_(), both, differentiable=True)
    assert out["score"].requires_grad and not out["tok"].requires_grad and logits.shape[0] == seg_off[-1] == tgt_d.numel()
    assert out["score"].detach().cpu().tolist() == [s for row in want for s in row]          # the same bits
    assert all(math.isfinite(s) and s < 0 for row in want for s in row)


def _grads(model, src, lengths, tgt, tl, m, w, swap=None, monkeypatch=None):
    """One mwer_step + backward on fixed hypotheses -> (loss, stats, {name: gradient}) with 'enc_out' among the names."""
    from asr_hip import functions as F_
    for p in model.parameters():
        p.grad = None
    kept = {}
    hook = model.encoder.register_forward_hook(lambda mod, args, out: (out[0].retain_grad(), kept.__setitem__("enc", out[0]))[0])
    if swap is not None:
        class Seq:
            @staticmethod
            def apply(logits, tgt_d, seg_d):
                return R.seq_scores(logits.to(swap), tgt_d, seg_d.tolist()).float(), None

        class Loss:
            @staticmethod
            def apply(score, err, utt_off, rs, gs):
                return (R.mwer_loss_of(score.to(swap), err, utt_off.tolist(), rs, gs).float(), torch.zeros_like(score),
                        torch.zeros(utt_off.numel() - 1, device=score.device), torch.zeros(2, device=score.device))
        monkeypatch.setattr(F_, "SeqLogProbFn", Seq)
        monkeypatch.setattr(F_, "MwerLossFn", Loss)
    try:
        loss, gold_seq, hyp_seq, stats = model.mwer_step(src, lengths, tgt, tl, m, w, nbest=3, hyps=HYPS)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hook.remove()
        if swap is not None:
            monkeypatch.undo()
    out = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    out["enc_out"] = kept["enc"].grad.detach().double().cpu()
    return float(loss.detach()), stats, out, gold_seq, hyp_seq


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradients_against_plain_torch_arithmetic_on_the_same_logits(cli, monkeypatch, precision):
    model = _model(cli, precision).train()
    src, lengths, tgt, tl = _batch()
    m, w = 0.5, 0.3
    loss, stats, g, gold_seq, hyp_seq = _grads(model, src, lengths, tgt, tl, m, w)
    loss64, _, g64, _, _ = _grads(model, src, lengths, tgt, tl, m, w, torch.float64, monkeypatch)
    loss32, _, g32, _, _ = _grads(model, src, lengths, tgt, tl, m, w, torch.float32, monkeypatch)
    assert math.isfinite(loss) and abs(loss - loss64) <= 4 * max(abs(loss32 - loss64), R.EPS32 * abs(loss64)), (loss, loss64, loss32)
    assert set(g) == set(g64) == set(g32) and "decoder.output_linear.weight" in g and "ctc_linear.weight" in g and "conv.0.weight" in g
    worst = ("", 0.0)
    for k in sorted(g):
        b32 = R.bound32(g64[k], g32[k])
        x = R.excess(g[k], g64[k], b32)
        worst = max(worst, (k, x), key=lambda t: t[1])
        assert x <= 1.0, (k, x, b32, float(g64[k].abs().max()))
    print("%s: worst gradient error / bound %.3f (%s); loss %.6f (float64 arithmetic %.6f)" % (precision, worst[1], worst[0], loss, loss64))
    assert float(g64["decoder.output_linear.weight"].abs().max()) > 0 and float(g64["enc_out"].abs().max()) > 0
    # what the trainer's metrics get: the gold targets with EOS, PAD behind, and an arg-max for exactly those positions
    want = [y + [2] + [0] * (4 - len(y)) for y in GOLD]
    assert gold_seq.cpu().tolist() == want and tuple(hyp_seq.shape) == (3, 5)
    assert all(hyp_seq[b, len(y) + 1:].eq(0).all() for b, y in enumerate(GOLD))
    # the loss is the definition's, from the kernel's own statistics
    risk, sums = stats["risk"].double().cpu(), stats["sums"].double().cpu()
    ntok = sum(len(y) + 1 for y in GOLD)
    assert stats["errors"] == [[0, 1, 2], [2, 3], [1, 2, 1]]
    want_loss = m * float(risk.sum()) / 3 + (1 - m) * ((1 - w) * (-float(sums[1]) / ntok) + w * float(stats["ctc"]))
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    assert abs(stats["expected_base"] - (1.0 + 2.5 + 4.0 / 3) / 3) <= 1e-12 and abs(stats["top_error"] - 1.0) <= 1e-12


def test_the_search_supplies_distinct_hypotheses_and_a_finite_loss(cli):
    model = _model(cli, "fp32").train()
    src, lengths, tgt, tl = _batch()
    loss, _, _, stats = model.mwer_step(src, lengths, tgt, tl, 0.5, 0.3, nbest=3)
    assert math.isfinite(float(loss.detach())) and len(stats["hyps"]) == 3
    for hs, es in zip(stats["hyps"], stats["errors"]):
        assert 1 <= len(hs) <= 3 and len(set(map(tuple, hs))) == len(hs) and len(es) == len(hs)
        assert all(0 not in y and 1 not in y and 2 not in y for y in hs)                       # CTC labels: no blank, SOS or EOS
    loss.backward()
    model.decoder.RESCORE_LOGIT_BYTES = 64
    try:
        with pytest.raises(ValueError, match="RESCORE_LOGIT_BYTES"):
            model.mwer_step(src, lengths, tgt, tl, 0.5, 0.3, nbest=3)
    finally:
        del model.decoder.RESCORE_LOGIT_BYTES


def test_a_small_gradient_step_lowers_the_risk_on_the_same_hypotheses(cli):
    """fp32, dropout 0, m = 1 (L is the mean risk alone, so the step is along the risk's own gradient), fixed hypotheses whose errors
    differ (0, 1, 2 / 2, 3 / 1, 2, 1).  First on the CPU restatement: the coefficients are not zero and a step against them lowers the
    restated risk.  Then the model: p -= eta * grad with eta sized for a predicted first-order decrease of 1e-3, and the risk
    recomputed in float64 from score_hypotheses' scores is lower than before."""
    model = _model(cli, "fp32").train()
    src, lengths, tgt, tl = _batch()
    errors = [[0, 1, 2], [2, 3], [1, 2, 1]]

    def risk64():
        was = model.training
        model.eval()
        scores = model.decoder.score_hypotheses(_enc(model, src, lengths), HYPS)
        model.train(was)
        flat, err, off = [], [], [0]
        for ss, es in zip(scores, errors):
            flat += [0.0] + ss
            err += [0.0] + [float(e) for e in es]
            off.append(len(flat))
        return R.mwer(np.asarray(flat), np.asarray(err), off, 1.0 / 3, 0.0), flat, err, off

    before, flat, err, off = risk64()
    coef = before["coef"]
    assert float(coef.abs().max()) > 1e-3
    stepped = R.mwer(np.asarray(flat) - 0.1 * coef.numpy(), np.asarray(err), off, 1.0 / 3, 0.0)
    assert float(stepped["loss"]) < float(before["loss"])                                        # the CPU restatement first
    for p in model.parameters():
        p.grad = None
    loss, _, _, stats = model.mwer_step(src, lengths, tgt, tl, 1.0, 0.3, nbest=3, hyps=HYPS)
    assert abs(float(loss.detach()) - float(before["loss"])) <= 1e-4 * max(1.0, abs(float(before["loss"])))
    loss.backward()
    torch.cuda.synchronize()
    sq = sum(float(p.grad.double().pow(2).sum()) for p in model.parameters() if p.grad is not None)
    assert sq > 0
    eta = 1e-3 / sq
    with torch.no_grad():
        for p in model.parameters():
            if p.grad is not None:
                p.add_(p.grad, alpha=-eta)
    after = risk64()[0]
    print("mean risk %.6f -> %.6f (eta %.3e, |g|^2 %.3e)" % (float(before["loss"]), float(after["loss"]), eta, sq))
    assert float(after["loss"]) < float(before["loss"])


def _corpus(tmp_path):
    rng = np.random.RandomState(0)
    lines = []
    for i, text in enumerate(["ab a", "ba b", "b ab"]):
        wav = tmp_path / ("u%d.wav" % i)
        with wave.open(str(wav), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((rng.randn(8000 + 800 * i) * 2000).astype("<i2").tobytes())
        txt = tmp_path / ("u%d.txt" % i)
        txt.write_text(text + "\n")
        lines.append("%s,%s" % (wav, txt))
    man = tmp_path / "train.csv"
    man.write_text("\n".join(lines))
    lab = tmp_path / "labels.json"
    lab.write_text(json.dumps([" ", "a", "b"]))
    return str(man), str(lab)


def test_train_py_with_mwer_weight_continues_from_a_joint_checkpoint(cli, tmp_path, monkeypatch, caplog):
    """train.py --ctc-weight 0.3 for one epoch writes the checkpoint; train.py --mwer-weight 0.5 --ctc-weight 0.3 --continue-from it
    runs two more epochs on the three-utterance manifest (bf16, --mwer-unit word) through Transformer.mwer_step with finite losses."""
    import logging
    import train as train_mod
    from models.asr.transformer import Transformer
    caplog.set_level(logging.INFO)
    man, lab = _corpus(tmp_path)
    monkeypatch.chdir(tmp_path)
    base = ["--train-manifest-list", man, "--valid-manifest-list", man, "--labels-path", lab, "--cuda", "--batch-size", "3",
            "--num-workers", "0", "--save-every", "1", "--save-folder", str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2",
            "--dim-model", "32", "--dim-key", "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12",
            "--src-max-len", "64", "--label-smoothing", "0.1", "--dropout", "0.1", "--k-lr", "20", "--warmup", "5", "--ctc-weight", "0.3"]
    cli(base + ["--epochs", "1", "--name", "joint"])
    train_mod.main()
    path = str(tmp_path / "save" / "joint" / "best_model.th")
    calls = []
    step = Transformer.mwer_step

    def spy(self, *a, **k):
        out = step(self, *a, **k)
        calls.append((float(out[0].detach()), k.get("nbest"), k.get("unit"), [len(hs) for hs in out[3]["hyps"]]))
        return out
    monkeypatch.setattr(Transformer, "mwer_step", spy)
    cli(base + ["--epochs", "3", "--name", "mwer", "--continue-from", path, "--mwer-weight", "0.5", "--mwer-nbest", "3", "--mwer-unit", "word"])
    train_mod.main()
    assert len(calls) == 2 and all(math.isfinite(c[0]) and c[1] == 3 and c[2] == "word" and all(1 <= n <= 3 for n in c[3]) for c in calls), calls
    state = torch.load(str(tmp_path / "save" / "mwer" / "epoch_3.th"), map_location="cpu", weights_only=False)
    assert np.isfinite(state["metrics"]["train_loss"]) and np.isfinite(state["metrics"]["valid_loss"])
    assert state["optimizer_params"]["_step"] == 3 and state["args"].mwer_weight == 0.5
    log = caplog.text
    assert "mean expected error" in log and "top hypothesis" in log and "does not apply to the MWER step's gold term" in log


def test_with_the_flag_off_the_step_is_the_parents(cli, golden_dir, monkeypatch):
    """--mwer-weight 0 (the default): ops.mwer_loss and ops.seq_logprob_bwd patched to raise are never reached, and the trainer's step on
    vgg_tiny reproduces the golden loss of tests/test_gpu_model.py within that file's fp32 tolerance."""
    from asr_hip import ops
    from test_gpu_model import build
    from trainer.asr.trainer import Trainer
    from utils import constant

    def never(*a, **k):
        raise AssertionError("an MWER kernel was launched with --mwer-weight 0")
    monkeypatch.setattr(ops, "mwer_loss", never)
    monkeypatch.setattr(ops, "seq_logprob_bwd", never)
    old_args, old_explicit = constant.args, constant.explicit
    try:
        z, args, model, opt = build(golden_dir, "vgg_tiny", "fp32")
        assert args.mwer_weight == 0.0 and args.graph_buckets == 0
        tgt = torch.from_numpy(z["tgt"])
        data = (torch.from_numpy(z["src"]), tgt, torch.ones(tgt.shape[0]), torch.from_numpy(z["src_len"]),
                torch.tensor([int((row != 0).sum()) for row in tgt], dtype=torch.int32))
        r = Trainer()._run_batch(model, data, float(z["smoothing"]), "ce", model.id2label, opt)
        r = r.result() if hasattr(r, "result") else r
        assert abs(r[0] - float(z["loss"])) < 2e-5, (r[0], float(z["loss"]))
    finally:
        constant.set_args(old_args)
        constant.explicit = old_explicit
