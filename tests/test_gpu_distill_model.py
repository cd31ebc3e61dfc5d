"""Knowledge distillation at the model, trainer and train.py levels, on the tiny configuration of
tests/test_gpu_mwer_model.py: D 32, 2 + 2 layers, V 11, 3 utterances of 48 frames (12 encoder frames), fp32 and bf16.

Gradients: the same step with F_.DistillFn swapped for plain torch log_softmax arithmetic on the model's own logits
(distill_reference.loss_of), in float64 (the reference) and in fp32 (torch's own fp32); per tensor |g - g64| <= 4 max(max |g32 - g64|,
one fp32 rounding of the largest entry), the bound of the MWER step's test.  In bf16 both sides round dlogits to bf16 once, which the
fp32-against-float64 term measures on this very input."""
import json
import math
import wave

import numpy as np
import pytest
import torch

import distill_reference as D
import mwer_reference as R

pytestmark = pytest.mark.gpu

CHARS = "abcdefg "                       # + PAD, SOS, EOS: V = 11
TINY = ("--num-layers 2 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 16 "
        "--src-max-len 64 --dropout 0 --ctc-weight 0.3 --cuda").split()
GOLD = [[3, 4, 5], [8, 9, 3, 4], [4, 10]]
SMOOTHING = 0.1


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


def _model(cli, precision, seed=0, extra=()):
    from utils import constant
    from utils.functions import init_transformer_model
    torch.manual_seed(seed)
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(CHARS)
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(TINY + ["--precision", precision] + list(extra)), l2i, {i: c for c, i in l2i.items()}).cuda()


def _teacher(cli, precision, seed=1):
    return _model(cli, precision, seed).eval().requires_grad_(False)


def _batch():
    g = torch.Generator().manual_seed(3)
    src = torch.randn(3, 1, 161, 48, generator=g)              # 48 input frames: 12 encoder frames
    tgt = torch.zeros(3, 4, dtype=torch.int64)
    for b, y in enumerate(GOLD):
        tgt[b, :len(y)] = torch.tensor(y)
    return src.cuda(), torch.tensor([48, 40, 32]), tgt.cuda(), torch.tensor([len(y) for y in GOLD], dtype=torch.int32)


def _grads(model, teacher, a, w, c, tau=2.0, swap=None, monkeypatch=None):
    """One distill_step + backward -> (loss, stats, {name: gradient})."""
    from asr_hip import functions as F_
    src, lengths, tgt, tl = _batch()
    for p in model.parameters():
        p.grad = None
    if swap is not None:
        class Plain:
            @staticmethod
            def apply(s, t, gold, smoothing, pad_id, tau_, ce_scale, kd_scale, with_ce):
                loss, sums, am = D.loss_of(s.to(swap), t.to(swap), gold, smoothing, pad_id, tau_, ce_scale, kd_scale, with_ce)
                return loss.float(), sums, am
        monkeypatch.setattr(F_, "DistillFn", Plain)
    try:
        loss, gold, hyp_seq, stats = model.distill_step(src, lengths, tgt, tl, teacher, a, tau, SMOOTHING, ctc_weight=w, distill_ctc_weight=c)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        if swap is not None:
            monkeypatch.undo()
    out = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return float(loss.detach()), {k: float(v) for k, v in stats.items()}, out, gold, hyp_seq


def _compare(model, teacher, a, w, c, monkeypatch, what):
    loss, stats, g, gold, hyp_seq = _grads(model, teacher, a, w, c)
    loss64, _, g64, _, _ = _grads(model, teacher, a, w, c, swap=torch.float64, monkeypatch=monkeypatch)
    loss32, _, g32, _, _ = _grads(model, teacher, a, w, c, swap=torch.float32, monkeypatch=monkeypatch)
    assert math.isfinite(loss) and abs(loss - loss64) <= 4 * max(abs(loss32 - loss64), R.EPS32 * abs(loss64)), (loss, loss64, loss32)
    assert set(g) == set(g64) == set(g32) and "decoder.output_linear.weight" in g and "conv.0.weight" in g
    assert ("ctc_linear.weight" in g) == (w > 0)
    worst = ("", 0.0)
    for k in sorted(g):
        assert bool(torch.isfinite(g[k]).all()), k
        x = R.excess(g[k], g64[k], R.bound32(g64[k], g32[k]))
        worst = max(worst, (k, x), key=lambda t: t[1])
        assert x <= 1.0, (what, k, x, float(g64[k].abs().max()))
    print("%s: worst gradient error / bound %.3f (%s); loss %.6f (float64 arithmetic %.6f) %s" % (what, worst[1], worst[0], loss, loss64, stats))
    assert float(g64["decoder.output_linear.weight"].abs().max()) > 0
    # the loss is the definition's, from the step's own statistics
    l_att = (1 - a) * stats["ce"] + a * stats["kd"]
    want = l_att if w == 0 else (1 - w) * l_att + w * ((1 - c) * stats["ctc"] + c * stats["kdf"])
    assert abs(loss - want) <= 1e-5 * abs(want), (loss, want)
    assert stats["kd"] > 0 and (stats["kdf"] > 0) == (c > 0) and (stats["ctc"] > 0) == (w > 0)
    assert tuple(gold.shape) == tuple(hyp_seq.shape) and gold.shape[0] == 3
    return loss


@pytest.mark.parametrize("a,w,c", [(0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.3, 0.5)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradients_against_plain_torch_arithmetic_on_the_same_logits(cli, monkeypatch, precision, a, w, c):
    teacher = _teacher(cli, precision)
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    model = _model(cli, precision).train()
    _compare(model, teacher, a, w, c, monkeypatch, "%s a %g w %g c %g" % (precision, a, w, c))
    after = teacher.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p.grad is None and not p.requires_grad for p in teacher.parameters()) and not teacher.training


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_low_rank_student_under_a_full_rank_teacher(cli, monkeypatch, precision):
    teacher = _teacher(cli, precision)
    model = _model(cli, precision, extra=["--rank", "4"]).train()
    assert sum(p.numel() for p in model.parameters()) < sum(p.numel() for p in teacher.parameters())
    _compare(model, teacher, 0.5, 0.0, 0.0, monkeypatch, "%s rank 4" % precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_teacher_that_is_the_student_gives_no_kd(cli, precision):
    """A teacher with the weights of a dropout-0 student: |KD| <= 1e-6 (and the loss is the CE term's share alone)."""
    model = _model(cli, precision, seed=0).train()
    teacher = _teacher(cli, precision, seed=0)
    teacher.load_state_dict(model.state_dict())
    src, lengths, tgt, tl = _batch()
    loss, _, _, stats = model.distill_step(src, lengths, tgt, tl, teacher, 0.5, 2.0, SMOOTHING, ctc_weight=0.3, distill_ctc_weight=0.5)
    assert abs(float(stats["kd"])) <= 1e-6 and abs(float(stats["kdf"])) <= 1e-6 and math.isfinite(float(loss.detach()))
    loss.backward()


def _kl64(model, teacher, tau):
    src, lengths, tgt, _ = _batch()
    was = model.training
    model.eval()
    with torch.no_grad():
        s, gold = model(src, lengths, tgt)[:2]
        t = teacher(src, lengths, tgt)[0]
    model.train(was)
    V = s.shape[-1]
    return float(D.distill(s.reshape(-1, V).cpu(), t.reshape(-1, V).cpu(), gold.reshape(-1).cpu(), 0.0, 0, tau, 0.0, 1.0, with_ce=False)["loss"])


def test_a_few_adam_steps_lower_the_kl_to_the_teacher(cli):
    """fp32, a = 1 (the loss is KD alone): four optimiser steps on one batch lower the float64 KL to the teacher on that batch.  The
    optimiser owns the student's parameters and none of the teacher's; the teacher's weights do not move and never get a gradient."""
    from asr_hip import ops
    from utils import constant
    from utils.functions import init_optimizer
    teacher = _teacher(cli, "fp32")
    before_t = {k: v.clone() for k, v in teacher.state_dict().items()}
    model = _model(cli, "fp32", extra=["--k-lr", "1", "--warmup", "4"]).train()
    opt = init_optimizer(constant.args, model, "noam")
    flat = opt.optimizer.flat
    assert flat.total == sum((p.numel() + 63) // 64 * 64 for p in model.parameters())
    assert {id(p) for p in flat.params} == {id(p) for p in model.parameters()} and not any(id(p) in flat.index for p in teacher.parameters())
    src, lengths, tgt, tl = _batch()
    before = _kl64(model, teacher, 2.0)
    for _ in range(4):
        opt.zero_grad()
        loss, _, _, stats = model.distill_step(src, lengths, tgt, tl, teacher, 1.0, 2.0, SMOOTHING)
        ops.backward_from(loss)
        opt.step()
    torch.cuda.synchronize()
    after = _kl64(model, teacher, 2.0)
    print("float64 KD to the teacher: %.6f -> %.6f" % (before, after))
    assert math.isfinite(after) and after < before
    now = teacher.state_dict()
    assert all(torch.equal(now[k], before_t[k]) for k in before_t) and all(p.grad is None for p in teacher.parameters())


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


def test_train_py_distils_a_low_rank_student_from_a_checkpoint(cli, tmp_path, monkeypatch, caplog):
    """train.py for one epoch writes the teacher; train.py --distill-from it --distill-weight 0.5 --distill-temperature 2 --rank 4 runs
    two epochs on the three-utterance manifest through Transformer.distill_step with finite losses; the flags are in the student's
    checkpoint, and load_model of that checkpoint builds no teacher."""
    import logging
    import train as train_mod
    import utils.functions as UF
    from models.asr.transformer import Transformer
    caplog.set_level(logging.INFO)
    man, lab = _corpus(tmp_path)
    monkeypatch.chdir(tmp_path)
    base = ["--train-manifest-list", man, "--valid-manifest-list", man, "--labels-path", lab, "--cuda", "--batch-size", "3",
            "--num-workers", "0", "--save-every", "1", "--save-folder", str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2",
            "--dim-model", "32", "--dim-key", "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12",
            "--src-max-len", "64", "--label-smoothing", "0.1", "--dropout", "0.1", "--k-lr", "20", "--warmup", "5"]
    cli(base + ["--epochs", "1", "--name", "teacher"])
    train_mod.main()
    path = str(tmp_path / "save" / "teacher" / "best_model.th")
    calls = []
    step = Transformer.distill_step

    def spy(self, *a, **k):
        out = step(self, *a, **k)
        calls.append((float(out[0].detach()), a[5], a[6], type(a[4]).__name__, a[4].training, float(out[3]["kd"])))
        return out
    monkeypatch.setattr(Transformer, "distill_step", spy)
    cli(base + ["--epochs", "2", "--name", "student", "--distill-from", path, "--distill-weight", "0.5", "--distill-temperature", "2",
                "--rank", "4"])
    train_mod.main()
    assert len(calls) == 2 and all(math.isfinite(c[0]) and c[1:5] == (0.5, 2.0, "Transformer", False) and math.isfinite(c[5]) for c in calls), calls
    out = str(tmp_path / "save" / "student" / "epoch_2.th")
    state = torch.load(out, map_location="cpu", weights_only=False)
    assert np.isfinite(state["metrics"]["train_loss"]) and np.isfinite(state["metrics"]["valid_loss"])
    assert state["optimizer_params"]["_step"] == 2
    assert (state["args"].distill_from, state["args"].distill_weight, state["args"].distill_temperature, state["args"].rank) == (path, 0.5, 2.0, 4)
    assert set(state) == {"label2id", "id2label", "args", "epoch", "model_state_dict", "optimizer_state_dict", "optimizer_params", "metrics"}
    assert "the distillation step runs as eager launches" in caplog.text

    def never(*a, **k):
        raise AssertionError("load_model built a teacher")
    monkeypatch.setattr(UF, "load_teacher", never)
    model = UF.load_model(out)[0]
    assert type(model).__name__ == "Transformer" and set(model.state_dict()) == set(state["model_state_dict"])


def test_with_the_flags_off_the_step_is_the_parents(cli, golden_dir, monkeypatch):
    """No --distill-* flag (the default): ops.distill_fwd and ops.distill_bwd patched to raise are never reached, and the trainer's step on
    vgg_tiny reproduces the golden loss of tests/test_gpu_model.py within that file's fp32 tolerance."""
    from asr_hip import ops
    from test_gpu_model import build
    from trainer.asr.trainer import Trainer
    from utils import constant

    def never(*a, **k):
        raise AssertionError("a distillation kernel was launched with every --distill flag off")
    monkeypatch.setattr(ops, "distill_fwd", never)
    monkeypatch.setattr(ops, "distill_bwd", never)
    old_args, old_explicit = constant.args, constant.explicit
    try:
        z, args, model, opt = build(golden_dir, "vgg_tiny", "fp32")
        assert args.distill_weight == 0.0 and args.distill_ctc_weight == 0.0 and args.distill_from is None and args.graph_buckets == 0
        tgt = torch.from_numpy(z["tgt"])
        data = (torch.from_numpy(z["src"]), tgt, torch.ones(tgt.shape[0]), torch.from_numpy(z["src_len"]),
                torch.tensor([int((row != 0).sum()) for row in tgt], dtype=torch.int32))
        r = Trainer()._run_batch(model, data, float(z["smoothing"]), "ce", model.id2label, opt)
        r = r.result() if hasattr(r, "result") else r
        assert abs(r[0] - float(z["loss"])) < 2e-5, (r[0], float(z["loss"]))
    finally:
        constant.set_args(old_args)
        constant.explicit = old_explicit
