"""MWER training over the CTC n-best without a GPU: the float64 restatement tests/mwer_reference.py against
autograd, its invariants and edge rules, the error counts, the flags and refusals, and the binding of the two new entry points."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mwer_reference as R


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


NS = [(2,), (16,), (3, 0, 1, 16), (1, 2, 5), (0,), (4, 4, 4)]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("ns", NS)
def test_analytic_coefficients_are_the_gradient_of_the_loss(ns):
    """coef of the closed form == d L_part / d score by autograd of plain softmax arithmetic (float64, 1e-12), and gradcheck of that
    arithmetic itself."""
    score, err, off = R.loss_case(ns)
    B = len(ns)
    rs, gs = 0.5 / B, 0.35 / 17.0
    ref = R.mwer(score, err, off, rs, gs)
    loss, grad = R.mwer_autograd(score, err, off, rs, gs)
    assert abs(float(loss) - float(ref["loss"])) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((grad - ref["coef"]).abs().max()) <= 1e-12
    s = torch.as_tensor(score).double().requires_grad_()
    assert torch.autograd.gradcheck(lambda x: R.mwer_loss_of(x, err, off, rs, gs), (s,), eps=1e-6, atol=1e-8)


@pytest.mark.parametrize("ns", NS)
def test_hypothesis_coefficients_sum_to_zero_and_the_loss_ignores_a_constant_error(ns):
    """sum_i coef_i = 0 over the hypotheses of every utterance (softmax is shift invariant), the gold coefficient is -gold_scale, prob
    is a distribution, and adding a constant to all e_i changes neither risk nor coefficients beyond float64 rounding."""
    score, err, off = R.loss_case(ns)
    ref = R.mwer(score, err, off, 0.25, 0.01)
    shifted = err.copy()
    for b in range(len(ns)):
        shifted[off[b] + 1:off[b + 1]] += 7.0
    ref7 = R.mwer(score, shifted, off, 0.25, 0.01)
    assert float((ref7["risk"] - ref["risk"]).abs().max()) <= 1e-12 and abs(float(ref7["loss"] - ref["loss"])) <= 1e-12
    assert float((ref7["coef"] - ref["coef"]).abs().max()) <= 1e-12
    for b, n in enumerate(ns):
        g = int(off[b])
        assert float(ref["coef"][g]) == -0.01 and float(ref["prob"][g]) == 0.0
        assert abs(float(ref["coef"][g + 1:g + 1 + n].sum())) <= 1e-14
        if n:
            assert abs(float(ref["prob"][g + 1:g + 1 + n].sum()) - 1.0) <= 1e-12


def test_edge_rules():
    """n_b in {0, 1}: risk 0 and zero hypothesis coefficients; a hypothesis score of -inf: P = 0 and coefficient 0, the others
    renormalise among themselves; every hypothesis at -inf: no risk; a gold score of -inf: the loss is +inf."""
    inf = math.inf
    score = np.array([-3.0, -4.0, -5.0, -2.0, -6.0, -inf, -7.0, -1.0, -inf, -inf], dtype=np.float32)
    err = np.array([0.0, 3.0, 0.0, 0.0, 2.0, 9.0, 4.0, 0.0, 1.0, 2.0], dtype=np.float32)
    off = [0, 2, 3, 7, 10]                       # n = 1, 0, 3 (one -inf), 2 (both -inf)
    ref = R.mwer(score, err, off, 0.5, 0.1)
    assert ref["risk"].tolist()[0] == 0.0 and ref["risk"].tolist()[1] == 0.0 and ref["risk"].tolist()[3] == 0.0
    assert ref["coef"].tolist()[1] == 0.0 and ref["prob"].tolist()[1] == 1.0
    assert ref["prob"].tolist()[5] == 0.0 and ref["coef"].tolist()[5] == 0.0
    two = R.mwer(np.array([-2.0, -6.0, -7.0]), np.array([0.0, 2.0, 4.0]), [0, 3], 0.5, 0.1)
    assert abs(float(ref["prob"][4]) - float(two["prob"][1])) <= 1e-15 and abs(float(ref["coef"][6]) - float(two["coef"][2])) <= 1e-15
    assert abs(float(ref["risk"][2]) - float((two["prob"][1:] * (torch.tensor([2.0, 4.0]).double() - 5.0)).sum())) <= 1e-12   # mean over n_b = 3
    assert ref["prob"].tolist()[8:] == [0.0, 0.0] and ref["coef"].tolist()[8:] == [0.0, 0.0]
    assert math.isfinite(float(ref["loss"]))
    score[0] = -inf
    assert float(R.mwer(score, err, off, 0.5, 0.1)["loss"]) == inf


def test_dlogits_is_the_closed_form():
    """autograd of log_softmax(...).gather summed per segment == c ([v == t] - softmax) row by row (float64, 1e-12); rows of an empty
    coefficient or outside every segment are zero."""
    c = R.bwd_case(7, 9, 5)
    V, off = c["V"], c["seg_off"].tolist()
    got = R.dlogits(c["buf"][:, :V], c["tgt"], off, c["coef"], grad_out=0.5)
    p = torch.softmax(torch.as_tensor(c["buf"][:, :V]).double(), dim=1)
    for m in range(9):
        r = max(i for i in range(5) if off[i] <= m)
        want = 0.5 * float(c["coef"][r]) * (torch.nn.functional.one_hot(torch.tensor(int(c["tgt"][m])), V).double() - p[m])
        assert float((got[m] - want).abs().max()) <= 1e-12
    assert off[2] == off[3]


# ------------------------------------------------------------------------------------------------ error counts
FLAGS = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 12 "
         "--src-max-len 64").split()


def _model(cli, extra=(), chars=("a", "b", " ")):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(chars)
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, {i: c for c, i in l2i.items()})


def test_label_and_word_error_counts_on_a_hand_example(cli):
    """a = 3, b = 4, space = 5.  gold 'ab ba'; 'ab bb' is one label and one word off, 'abba' one label (the space) and two words
    (two words became one: a substitution and a deletion), '' five labels and two words, gold itself 0 / 0; leading, trailing and
    double spaces make no empty words."""
    model = _model(cli, ["--ctc-weight", "0.3"])
    gold = [3, 4, 5, 4, 3]
    hyps = [[[3, 4, 5, 4, 4], [3, 4, 4, 3], [], gold, [5, 3, 4, 5, 5, 4, 3, 5]]]
    assert model.mwer_errors(hyps, [gold], "label") == [[1, 1, 5, 0, 3]]
    assert model.mwer_errors(hyps, [gold], "word") == [[1, 2, 2, 0, 0]]
    assert R.words([5, 3, 4, 5, 5, 4, 3, 5], 5) == [(3, 4), (4, 3)] and R.words([], 5) == []
    assert model.mwer_errors([[], [[3]]], [[3], [4]], "label") == [[], [1]]
    with pytest.raises(ValueError, match="mwer-unit"):
        model.mwer_errors(hyps, [gold], "char")
    with pytest.raises(ValueError, match="space label"):
        _model(cli, ["--ctc-weight", "0.3"], chars=("a", "b")).mwer_errors(hyps, [gold], "word")


# ------------------------------------------------------------------------------------------------ flags and refusals
def test_the_flags_parse_and_default_to_off(cli):
    a = cli([])
    assert a.mwer_weight == 0.0 and a.mwer_nbest == 4 and a.mwer_unit == "label"
    a = cli(["--mwer-weight", "0.5", "--mwer-nbest", "8", "--mwer-unit", "word", "--ctc-weight", "0.3"])
    assert a.mwer_weight == 0.5 and a.mwer_nbest == 8 and a.mwer_unit == "word"
    with pytest.raises(SystemExit):
        cli(["--mwer-unit", "char"])


def test_refusals(cli):
    from utils.functions import check_mwer
    assert check_mwer(cli([])) == 0.0
    assert check_mwer(cli(["--mwer-nbest", "99"])) == 0.0                      # off: nothing else is looked at
    assert check_mwer(cli(["--mwer-weight", "0.5", "--ctc-weight", "0.3"]), {" ": 3}) == 0.5
    assert check_mwer(cli(["--mwer-weight", "1", "--ctc-weight", "0.3", "--mwer-nbest", "16", "--mwer-unit", "word"]), {" ": 3}) == 1.0
    for argv, what in ((["--mwer-weight", "1.5", "--ctc-weight", "0.3"], r"\[0, 1\]"),
                       (["--mwer-weight", "-0.1", "--ctc-weight", "0.3"], r"\[0, 1\]"),
                       (["--mwer-weight", "0.5"], "needs --ctc-weight > 0"),
                       (["--mwer-weight", "0.5", "--ctc-weight", "0.3", "--parallel"], "--parallel"),
                       (["--mwer-weight", "0.5", "--ctc-weight", "0.3", "--loss", "ctc"], "--loss ctc"),
                       (["--mwer-weight", "0.5", "--ctc-weight", "0.3", "--mwer-nbest", "1"], "2..16"),
                       (["--mwer-weight", "0.5", "--ctc-weight", "0.3", "--mwer-nbest", "17"], "2..16")):
        with pytest.raises(ValueError, match=what):
            check_mwer(cli(argv), {" ": 3})
    with pytest.raises(ValueError, match="space label"):
        check_mwer(cli(["--mwer-weight", "0.5", "--ctc-weight", "0.3", "--mwer-unit", "word"]), {"a": 3})


def test_the_model_refuses_before_any_device_work(cli):
    """Transformer.mwer_step on host tensors: no CTC head, a weight or an n-best size out of range, 'word' without a space."""
    z = torch.zeros(1, 1, 161, 8)
    plain = _model(cli)
    with pytest.raises(ValueError, match="encoder CTC head"):
        plain.mwer_step(z, [8], torch.zeros(1, 2, dtype=torch.int64), [2], 0.5, 0.3)
    head = _model(cli, ["--ctc-weight", "0.3"])
    for kw, what in ((dict(mwer_weight=0.0, ctc_weight=0.3), r"\(0, 1\]"), (dict(mwer_weight=0.5, ctc_weight=0.0), "--ctc-weight > 0"),
                     (dict(mwer_weight=0.5, ctc_weight=0.3, nbest=1), r"2\.\.16"), (dict(mwer_weight=0.5, ctc_weight=0.3, nbest=17), r"2\.\.16")):
        with pytest.raises(ValueError, match=what):
            head.mwer_step(z, [8], torch.zeros(1, 2, dtype=torch.int64), [2], **kw)
    with pytest.raises(ValueError, match="space label"):
        _model(cli, ["--ctc-weight", "0.3"], chars=("a", "b")).mwer_step(z, [8], torch.zeros(1, 2, dtype=torch.int64), [2], 0.5, 0.3, unit="word")


# ------------------------------------------------------------------------------------------------ the binding
def test_the_entry_points_are_declared_and_bound():
    """asr_seq_logprob_bwd and asr_mwer_loss in include/asr_hip.h with the issue's arguments, ctypes signatures of the same length and
    kinds in asr_hip/lib.py, wrappers in ops.py, and the ABI version unchanged (the change is additive)."""
    from asr_hip import lib as L
    from asr_hip import functions as F_
    from asr_hip import ops
    src = open(L.HEADER).read()
    want = {
        "asr_seq_logprob_bwd": ["const float* logits", "int64_t ld", "const int64_t* tgt", "const int32_t* seg_off", "const float* coef",
                                "const float* grad_out", "int R", "int M", "int V", "void* dlogits", "int64_t ldd", "int out_dtype",
                                "asr_stream_t stream"],
        "asr_mwer_loss": ["const float* score", "const float* err", "const int32_t* utt_off", "int B", "int R", "float risk_scale",
                          "float gold_scale", "float* prob", "float* coef", "float* risk", "float* sums", "asr_stream_t stream"],
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
    assert callable(ops.seq_logprob_bwd) and callable(ops.mwer_loss) and ops.MWER_NBEST_MAX == 16
    assert issubclass(F_.SeqLogProbFn, torch.autograd.Function) and issubclass(F_.MwerLossFn, torch.autograd.Function)
    csrc = os.path.join(os.path.dirname(os.path.dirname(L.HERE)), "end2end-asr-pytorch_amd", "csrc")
    assert '#include "lse.h"' in open(os.path.join(csrc, "mwer.hip")).read() and '#include "lse.h"' in open(os.path.join(csrc, "seq_logprob.hip")).read()
    assert "struct Lse" not in open(os.path.join(csrc, "mwer.hip")).read() and "struct Lse" not in open(os.path.join(csrc, "seq_logprob.hip")).read()
