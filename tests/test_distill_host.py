"""Knowledge distillation from a teacher checkpoint without a GPU: the float64 restatement
tests/distill_reference.py against autograd and against the CE reference, the flags and every refusal of check_distill / load_teacher /
Transformer.distill_step, and the binding of the four new entry points."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distill_reference as D
import rowwise_reference as RW


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("tau", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("M,V", [(1, 3), (7, 11), (9, 257)])
def test_the_kd_term_is_autograd_of_kl_div(M, V, tau):
    """KD = tau^2 / n sum KL(pT || pS) and dKD/ds = tau (pS - pT) / n: the restatement against autograd of F.kl_div on F.log_softmax
    (float64, 1e-12), with dead rows that hold NaN."""
    c = D.case(M, V)
    s, t = c["s"][:, :V].copy(), c["t"][:, :V].copy()
    dead = c["gold"] == D.PAD
    ref = D.distill(np.where(dead[:, None], np.nan, s), np.where(dead[:, None], np.nan, t), c["gold"], 0.0, D.PAD, tau, 0.0, 1.0, with_ce=False)
    kd, grad = D.kd_autograd(s, t, c["gold"], D.PAD, tau)
    assert abs(float(ref["loss"]) - float(kd)) <= 1e-12 * max(1.0, abs(float(kd)))
    assert float((ref["dlogits"] - grad).abs().max()) <= 1e-12
    n = float((~dead).sum())
    pS = torch.softmax(torch.as_tensor(s).double() / tau, 1)
    pT = torch.softmax(torch.as_tensor(t).double() / tau, 1)
    want = tau * (pS - pT) / n * torch.as_tensor(~dead).double()[:, None]
    assert float((grad - want).abs().max()) <= 1e-12
    assert bool((ref["kd"][torch.as_tensor(~dead)] > 0).all()) and bool((ref["kd"][torch.as_tensor(dead)] == 0).all())
    assert bool((ref["row_stats"][torch.as_tensor(dead)] == 0).all()) and float(ref["sums"][0]) == 0.0 and float(ref["sums"][2]) == 0.0


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_the_ce_term_is_the_ce_reference_and_the_terms_add(smoothing):
    """ce_scale = 1, kd_scale = 0: loss, sums[0..2], argmax and gradient are rowwise_reference.ce_reference's; and the combined gradient
    is the weighted sum of the two terms' (float64, 1e-12)."""
    c = D.case(9, 11)
    s, t, gold = c["s"][:, :11], c["t"][:, :11], torch.as_tensor(c["gold"])
    ce = RW.ce_reference(torch.as_tensor(s), gold, smoothing, D.PAD, 1.5)
    only_ce = D.distill(s, t, gold, smoothing, D.PAD, 2.0, 1.0, 0.0, grad_out=1.5)
    assert abs(float(only_ce["loss"]) - float(ce["sums"][0]) / ce["sums"][1]) <= 1e-12
    assert float(only_ce["sums"][1]) == ce["sums"][1] and float(only_ce["sums"][2]) == ce["sums"][2]
    live = only_ce["live"]
    assert torch.equal(only_ce["argmax"][live], ce["argmax"][live]) and float((only_ce["dlogits"] - ce["dlogits"]).abs().max()) <= 1e-12
    only_kd = D.distill(s, t, gold, smoothing, D.PAD, 2.0, 0.0, 1.0, grad_out=1.5)
    both = D.distill(s, t, gold, smoothing, D.PAD, 2.0, 0.3, 0.7, grad_out=1.5)
    assert float((both["dlogits"] - (0.3 * only_ce["dlogits"] + 0.7 * only_kd["dlogits"])).abs().max()) <= 1e-12
    assert abs(float(both["loss"]) - (0.3 * float(only_ce["loss"]) + 0.7 * float(only_kd["loss"]))) <= 1e-12
    same = D.distill(s, s, gold, smoothing, D.PAD, 2.0, 0.3, 0.7)
    assert float(same["kd"].abs().max()) == 0.0 and float(same["sums"][3]) == 0.0


@pytest.mark.parametrize("with_ce", [True, False])
def test_the_differentiable_form_of_the_model_tests_is_the_restatement(with_ce):
    """distill_reference.loss_of (what the model tests swap F_.DistillFn for) against distill(): loss, sums and autograd's gradient
    (float64, 1e-12)."""
    c = D.case(9, 11)
    s = torch.as_tensor(c["s"][:, :11]).double().view(3, 3, 11).clone().requires_grad_()
    t, gold = torch.as_tensor(c["t"][:, :11]).double().view(3, 3, 11), torch.as_tensor(c["gold"]).view(3, 3)
    loss, sums, am = D.loss_of(s, t, gold, 0.1, D.PAD, 2.0, 0.3, 0.7, with_ce)
    (loss * 1.5).backward()
    ref = D.distill(c["s"][:, :11], c["t"][:, :11], c["gold"], 0.1, D.PAD, 2.0, 0.3, 0.7, grad_out=1.5, with_ce=with_ce)
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 and float((sums.double() - ref["sums"]).abs().max()) <= 1e-5
    assert float((s.grad.view(9, 11) - ref["dlogits"]).abs().max()) <= 1e-12 and am.shape == (9,)


# ------------------------------------------------------------------------------------------------ flags and refusals
FLAGS = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 12 "
         "--src-max-len 64").split()
CHARS = ("a", "b", " ")


def _labels(chars=CHARS):
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(chars)
    l2i = {c: i for i, c in enumerate(chars)}
    return l2i, {i: c for c, i in l2i.items()}


def _model(cli, extra=(), chars=CHARS):
    from utils.functions import init_transformer_model
    l2i, i2l = _labels(chars)
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, i2l)


def _checkpoint(cli, tmp_path, extra=(), chars=CHARS, name="teacher.th"):
    """A teacher checkpoint with save_model's keys, written from a tiny CPU-built model."""
    l2i, i2l = _labels(chars)
    model = _model(cli, extra, chars)
    from utils import constant
    path = str(tmp_path / name)
    torch.save({"label2id": l2i, "id2label": i2l, "args": copy.deepcopy(constant.args), "epoch": 1,
                "model_state_dict": {k: v.detach().clone() for k, v in model.state_dict().items()}}, path)
    return path, model


def test_the_flags_parse_and_default_to_off(cli):
    a = cli([])
    assert a.distill_from is None and a.distill_weight == 0.0 and a.distill_ctc_weight == 0.0 and a.distill_temperature == 2.0
    a = cli(["--distill-from", "t.th", "--distill-weight", "0.5", "--distill-ctc-weight", "0.25", "--distill-temperature", "4"])
    assert (a.distill_from, a.distill_weight, a.distill_ctc_weight, a.distill_temperature) == ("t.th", 0.5, 0.25, 4.0)


def test_check_distill_refusals(cli):
    from utils.functions import check_distill
    assert check_distill(cli([])) == (0.0, 0.0)
    assert check_distill(cli(["--distill-temperature", "99"])) == (0.0, 0.0)                   # off: nothing else is looked at
    assert check_distill(cli(["--distill-from", "t.th", "--distill-weight", "0.5"])) == (0.5, 0.0)
    assert check_distill(cli(["--distill-from", "t.th", "--distill-weight", "1", "--distill-ctc-weight", "1", "--ctc-weight", "0.3",
                              "--distill-temperature", "16"])) == (1.0, 1.0)
    on = ["--distill-from", "t.th", "--distill-weight", "0.5"]
    for argv, what in ((["--distill-weight", "1.5", "--distill-from", "t.th"], r"--distill-weight must lie in \[0, 1\]"),
                       (["--distill-weight", "-0.1", "--distill-from", "t.th"], r"--distill-weight must lie in \[0, 1\]"),
                       (["--distill-ctc-weight", "1.5", "--distill-from", "t.th"], r"--distill-ctc-weight must lie in \[0, 1\]"),
                       (["--distill-weight", "0.5"], "need --distill-from PATH"),
                       (["--distill-ctc-weight", "0.5", "--ctc-weight", "0.3"], "need --distill-from PATH"),
                       (["--distill-from", "t.th"], "never used"),
                       (on + ["--distill-temperature", "0.25"], r"\[0\.5, 16\]"),
                       (on + ["--distill-temperature", "17"], r"\[0\.5, 16\]"),
                       (on + ["--parallel"], "--parallel"),
                       (on + ["--loss", "ctc"], "--loss ctc"),
                       (on + ["--mwer-weight", "0.5", "--ctc-weight", "0.3"], "--mwer-weight"),
                       (["--distill-from", "t.th", "--distill-ctc-weight", "0.5"], "needs --ctc-weight > 0")):
        with pytest.raises(ValueError, match=what):
            check_distill(cli(argv))


def test_load_teacher_builds_a_frozen_model_and_leaves_the_process_state(cli, tmp_path):
    """The teacher comes from the checkpoint's own Namespace (here: two layers where the student's command line says one), in eval mode,
    with no parameter that requires grad and the checkpoint's weights; constant.args / constant.explicit are the student's, unchanged."""
    from utils import constant
    from utils.functions import load_teacher
    path, src = _checkpoint(cli, tmp_path, ["--num-layers", "2", "--precision", "bf16"])
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    ckpt["args"].parallel = True                                 # as a data-parallel run would have saved it
    torch.save(ckpt, path)
    l2i, _ = _labels()
    args = cli(FLAGS + ["--distill-from", path, "--distill-weight", "0.5", "--rank", "4", "--precision", "fp32"])
    kept_args, kept_vars, kept_explicit = constant.args, copy.deepcopy(vars(constant.args)), copy.deepcopy(constant.explicit)
    teacher = load_teacher(path, args, l2i)
    assert constant.args is kept_args and vars(constant.args) == kept_vars and constant.explicit == kept_explicit
    assert type(teacher).__name__ == "Transformer" and not teacher.training                   # parallel=False: no wrapper
    from asr_hip import ops
    assert ops.compute_dtype() == torch.float32                                              # the student's --precision, not the file's bf16
    assert len(teacher.encoder.layers) == 2 and not any(p.requires_grad for p in teacher.parameters())
    assert all(p.grad is None for p in teacher.parameters())
    sd = src.state_dict()
    got = teacher.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert torch.load(path, map_location="cpu", weights_only=False)["args"].parallel is True   # the copy was changed, not the file's


def test_load_teacher_refusals(cli, tmp_path):
    from utils.functions import load_teacher
    l2i, _ = _labels()
    path, _ = _checkpoint(cli, tmp_path)
    on = FLAGS + ["--distill-from", path, "--distill-weight", "0.5"]
    with pytest.raises(ValueError, match="no such teacher checkpoint"):
        load_teacher(str(tmp_path / "missing.th"), cli(on), l2i)
    with pytest.raises(ValueError, match=r"teacher's labels \(6\) differ from the student's \(5\)"):
        load_teacher(path, cli(on), _labels(("a", "b"))[0])
    swapped = _labels(("b", "a", " "))[0]
    with pytest.raises(ValueError, match="teacher's labels"):
        load_teacher(path, cli(on), swapped)
    for extra, what in ((["--features", "fbank"], "--features spect, the student runs with --features fbank"),
                        (["--num-mel-bins", "40"], "--num-mel-bins 80, the student runs with --num-mel-bins 40"),
                        (["--mel-fmin", "50"], "--mel-fmin"),
                        (["--sample-rate", "8000"], "--sample-rate 16000, the student runs with --sample-rate 8000"),
                        (["--window-size", "0.025"], "--window-size"),
                        (["--window-stride", "0.02"], "--window-stride"),
                        (["--window", "hann"], "--window hamming, the student runs with --window hann")):
        with pytest.raises(ValueError, match=what):
            load_teacher(path, cli(on + extra), l2i)
    ctc = FLAGS + ["--distill-from", path, "--distill-ctc-weight", "0.5", "--ctc-weight", "0.3"]
    with pytest.raises(ValueError, match="has no encoder CTC head"):
        load_teacher(path, cli(ctc), l2i)
    headed, _ = _checkpoint(cli, tmp_path, ["--ctc-weight", "0.3"], name="headed.th")
    with pytest.raises(ValueError, match="--feat_extractor vgg_cnn, the student emb_cnn"):
        load_teacher(headed, cli(FLAGS + ["--distill-from", headed, "--distill-ctc-weight", "0.5", "--ctc-weight", "0.3", "--feat_extractor",
                                          "emb_cnn"]), l2i)
    assert hasattr(load_teacher(headed, cli(FLAGS + ["--distill-from", headed, "--distill-ctc-weight", "0.5", "--ctc-weight", "0.3"]), l2i),
                   "ctc_linear")


def test_the_model_refuses_before_any_device_work(cli):
    """Transformer.distill_step on host tensors: weights and temperature out of range, the frame-level term without the heads it needs."""
    z, tgt = torch.zeros(1, 1, 161, 8), torch.zeros(1, 2, dtype=torch.int64)
    plain, teacher = _model(cli), _model(cli)
    for kw, what in ((dict(distill_weight=0.0, temperature=2.0), r"in \(0, 1\]"), (dict(distill_weight=1.5, temperature=2.0), r"in \(0, 1\]"),
                     (dict(distill_weight=0.5, temperature=0.25), r"\[0\.5, 16\]"), (dict(distill_weight=0.5, temperature=32.0), r"\[0\.5, 16\]"),
                     (dict(distill_weight=0.5, temperature=2.0, distill_ctc_weight=0.5), "needs --ctc-weight > 0"),
                     (dict(distill_weight=0.5, temperature=2.0, distill_ctc_weight=0.5, ctc_weight=0.3), "student with an encoder CTC head")):
        with pytest.raises(ValueError, match=what):
            plain.distill_step(z, [8], tgt, [2], teacher, smoothing=0.1, **kw)
    head = _model(cli, ["--ctc-weight", "0.3"])
    with pytest.raises(ValueError, match="teacher has no encoder CTC head"):
        head.distill_step(z, [8], tgt, [2], teacher, 0.5, 2.0, 0.1, ctc_weight=0.3, distill_ctc_weight=0.5)
    other = _model(cli, ["--ctc-weight", "0.3", "--feat_extractor", "emb_cnn"])
    with pytest.raises(ValueError, match="different frame counts"):
        head.distill_step(z, [8], tgt, [2], other, 0.5, 2.0, 0.1, ctc_weight=0.3, distill_ctc_weight=0.5)


# ------------------------------------------------------------------------------------------------ the binding
def test_the_entry_points_are_declared_and_bound():
    """The four entry points in include/asr_hip.h with the issue's arguments, ctypes signatures of the same length and kinds in
    asr_hip/lib.py, wrappers in ops.py, DistillFn in functions.py, and the ABI version unchanged (the change is additive)."""
    from asr_hip import functions as F_
    from asr_hip import lib as L
    from asr_hip import ops
    src = open(L.HEADER).read()
    want = {
        "asr_distill_partial_blocks": ["int M"],
        "asr_distill_fwd": ["const float* student", "int64_t ld_s", "const float* teacher", "int64_t ld_t", "const int64_t* gold", "int M",
                            "int V", "float smoothing", "int pad_id", "float temperature", "int with_ce", "float* row_stats",
                            "int64_t* argmax", "float* partials", "asr_stream_t stream"],
        "asr_distill_finish": ["const float* partials", "int nblocks", "const float* den", "float ce_scale", "float kd_scale", "float* sums",
                               "float* loss", "asr_stream_t stream"],
        "asr_distill_bwd": ["const float* student", "int64_t ld_s", "const float* teacher", "int64_t ld_t", "const int64_t* gold",
                            "const float* row_stats", "int M", "int V", "float smoothing", "int pad_id", "float temperature",
                            "float ce_scale", "float kd_scale", "const float* grad_out", "const float* count", "void* dlogits",
                            "int64_t ldd", "int out_dtype", "asr_stream_t stream"],
    }
    for name, params in want.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, src)
        assert m, name + " is not declared"
        assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
        res, args = L._SIGS[name]
        kinds = [ctypes.c_void_p if "*" in p or "asr_stream_t" in p else ctypes.c_int64 if p.startswith("int64_t") else
                 ctypes.c_float if p.startswith("float") else ctypes.c_int for p in params]
        assert res is ctypes.c_int and args == kinds, name
        if os.path.exists(L.LIB_PATH):
            assert hasattr(L.load(), name)
    assert re.search(r"int asr_abi_version\(void\);\s*/\* 4 ", src)
    if os.path.exists(L.LIB_PATH):
        assert L.load().asr_abi_version() == 4
        assert [L.load().asr_distill_partial_blocks(m) for m in (0, 1, 8, 9, 64)] == [0, 1, 1, 2, 8]
    assert callable(ops.distill_fwd) and callable(ops.distill_bwd)
    assert issubclass(F_.DistillFn, torch.autograd.Function)
    csrc = os.path.join(os.path.dirname(os.path.dirname(L.HERE)), "end2end-asr-pytorch_amd", "csrc", "distill.hip")
    text = open(csrc).read()
    assert "atomicAdd" not in text and "getenv" not in text and "asr_tuning" not in text
