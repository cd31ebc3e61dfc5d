"""Attention rescoring without a GPU: the float64 restatement tests/attn_rescore_reference.py against brute force, the packing of
hypotheses, the bound of tests/test_gpu_attn_rescore.py on its own inputs, and the feature's flag, start-up errors and binding."""
import math
import os
import re

import numpy as np
import pytest
import torch

import attn_rescore_reference as R


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("V", [1, 2, 3, 4, 5])
def test_token_logprobs_are_a_distribution_over_the_targets(V):
    """exp(token_logprobs) over all V targets of a row sums to 1 within 1e-12, and each equals the brute-force exp(x_t) / sum exp(x)."""
    g = np.random.default_rng(V)
    logits = g.standard_normal((6, V)) * 4.0
    total = np.zeros(6)
    for t in range(V):
        lp = R.token_logprobs(logits, np.full(6, t)).numpy()
        brute = np.exp(logits[:, t]) / np.exp(logits).sum(axis=1)
        assert np.allclose(np.exp(lp), brute, rtol=1e-12, atol=0)
        total += np.exp(lp)
    assert np.abs(total - 1.0).max() <= 1e-12
    assert torch.all(R.token_logprobs(logits, np.full(6, V)) == -math.inf) and torch.all(R.token_logprobs(logits, np.full(6, -1)) == -math.inf)


def test_sequence_scores_sum_their_rows_and_empty_segments_score_zero():
    g = np.random.default_rng(0)
    logits, tgt = g.standard_normal((7, 5)), g.integers(0, 5, size=7)
    score, tok = R.sequence_scores(logits, tgt, [0, 0, 3, 3, 7, 7])
    assert score.tolist()[0] == 0.0 and score.tolist()[2] == 0.0 and score.tolist()[4] == 0.0
    assert abs(float(score[1]) - float(tok[:3].sum())) == 0.0 and abs(float(score[3]) - float(tok[3:].sum())) == 0.0
    assert R.sequence_scores(np.zeros((0, 4)), np.zeros(0, dtype=np.int64), [0, 0, 0])[0].tolist() == [0.0, 0.0]


def test_pack():
    """The empty hypothesis is [SOS] / [EOS] with length 1; ragged lists keep their order; an utterance without a hypothesis adds nothing."""
    assert R.pack([[[]]]) == ([[R.SOS]], [[R.EOS]], [1])
    ys, targets, lengths = R.pack([[[5, 6, 7], []], [], [[9]]])
    assert ys == [[R.SOS, 5, 6, 7], [R.SOS], [R.SOS, 9]]
    assert targets == [[5, 6, 7, R.EOS], [R.EOS], [9, R.EOS]]
    assert lengths == [4, 1, 2]
    assert R.pack([[], []]) == ([], [], [])


def test_combine_is_the_convex_form():
    assert R.combine(-3.0, -5.0, 0.0) == -3.0 and R.combine(-3.0, -5.0, 1.0) == -5.0
    assert R.combine(-3.0, -5.0, 0.25) == 0.75 * -3.0 + 0.25 * -5.0


def _fp32_restatement(logits, tgt, seg_off):
    """An fp32 implementation that is not torch's: numpy float32, (x_t - max) - log1p(sum of exp(x - max) over every column but the
    arg max), the sum taken column by column in index order (a row whose target holds most of the mass has a log-probability near 0:
    log of a rounded 1 + s would lose it, and the bound's floor is relative to the term); the segment sums are taken in float64 and
    rounded once."""
    x = np.asarray(logits, dtype=np.float32)
    rows = np.arange(x.shape[0])
    am = x.argmax(axis=1)
    m = x[rows, am]
    s = np.zeros(x.shape[0], dtype=np.float32)
    for v in range(x.shape[1]):
        s = np.where(am == v, s, (s + np.exp(x[:, v] - m)).astype(np.float32))
    tok = ((x[rows, tgt] - m) - np.log1p(s)).astype(np.float32)
    score = np.array([np.float32(tok[a:b].astype(np.float64).sum()) for a, b in zip(seg_off[:-1], seg_off[1:])], dtype=np.float32)
    return score, tok


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_the_bound_is_neither_vacuous_nor_broken_by_a_correct_fp32_implementation(name):
    """On the inputs of the GPU cases: torch's fp32 log_softmax + gather + sum lies inside the bound (by construction: four times its own
    error), so does an independent fp32 implementation that sums in another order, and the bound itself stays below 1e-5 of the scale
    max(1, sum |tok_lp|) -- a result off by one part in 10^5 fails it."""
    c = R.cases()[name]
    lg = R.logits_of(c)
    score, tok, score_b, tok_b = R.bounds(lg, c["tgt"], c["seg_off"])
    s32, t32 = R.torch32(lg, c["tgt"], c["seg_off"])
    assert torch.all((s32 - score).abs() <= score_b) and torch.all((t32 - tok).abs() <= tok_b)
    s_np, t_np = _fp32_restatement(lg, c["tgt"], c["seg_off"].tolist())
    err_s, err_t = (torch.from_numpy(s_np).double() - score).abs(), (torch.from_numpy(t_np).double() - tok).abs()
    print("%s: numpy fp32 worst score error %.3e of bound %.3e, token error / bound %.3f"
          % (name, float(err_s.max()), float(score_b.max()), float((err_t / tok_b.clamp_min(1e-300)).max())))
    if c["V"] > 1:
        assert torch.all(err_s <= score_b) and torch.all(err_t <= tok_b)
    else:                       # V = 1: every term is exactly 0, and so is the bound
        assert float(score_b.max()) == 0.0 and float(tok_b.max()) == 0.0 and float(err_s.max()) == 0.0
    off = c["seg_off"].tolist()
    for r in range(len(off) - 1):
        assert float(score_b[r]) <= 1e-5 * max(1.0, float(tok[off[r]:off[r + 1]].abs().sum()))
    assert torch.all(tok_b <= 1e-5 * tok.abs().clamp_min(1.0))


# ------------------------------------------------------------------------------------------------ the feature (fails without it)
FLAGS = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 12 "
         "--src-max-len 64").split()


def _model(cli, extra=()):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, "a", "b", " "]
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, {i: c for c, i in l2i.items()})


def test_the_flag_parses_and_defaults_to_off(cli):
    assert cli([]).attention_rescoring_weight == 0.0
    assert cli(["--ctc-beam-search", "--attention-rescoring-weight", "0.4"]).attention_rescoring_weight == 0.4


def test_start_up_errors(cli):
    """test.py refuses the weight without --ctc-beam-search and outside [0, 1]; Transformer.evaluate and ctc_beam_search refuse the same
    before any device work (host tensors, no GPU needed to get the error)."""
    import test as test_mod
    head = _model(cli, ["--ctc-weight", "0.3"])
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--attention-rescoring-weight", "0.4"]), head)
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--attention-rescoring-weight", "1"]), head)
    with pytest.raises(ValueError, match="--ctc-beam-search"):
        test_mod.check_ctc_decoding(cli(["--attention-rescoring-weight", "0.4"]), head)
    with pytest.raises(ValueError, match="--ctc-beam-search"):
        test_mod.check_ctc_decoding(cli(["--beam-search", "--attention-rescoring-weight", "0.4"]), head)
    for bad in ("1.5", "-0.1"):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--attention-rescoring-weight", bad]), head)
    x = torch.zeros(1, 1, 161, 8)
    tgt = torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="--ctc-beam-search"):
        head.evaluate(x, [8], tgt, attention_rescoring_weight=0.3)
    with pytest.raises(ValueError, match="--ctc-beam-search"):
        head.evaluate(x, [8], tgt, beam_search=True, beam_width=2, attention_rescoring_weight=0.3)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        head.evaluate(x, [8], tgt, ctc_beam=True, beam_width=4, attention_rescoring_weight=1.5)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        head.ctc_beam_search(torch.zeros(1, 2, 32), [2], 4, rescoring_weight=1.5)
    with pytest.raises(ValueError, match="one list of hypotheses per utterance"):
        head.decoder.score_hypotheses(torch.zeros(2, 3, 32), [[[3]]])
    with pytest.raises(ValueError, match="11"):                   # --tgt-max-len 12 positions: SOS and 11 labels
        head.decoder.score_hypotheses(torch.zeros(1, 3, 32), [[[3] * 12]])


def test_the_entry_point_is_declared_and_bound():
    """asr_seq_logprob in include/asr_hip.h with the issue's argument list, a ctypes signature of the same length and kinds in
    asr_hip/lib.py, the ABI version unchanged, and the comment cites what it replaces."""
    import ctypes
    from asr_hip import lib as L
    src = open(L.HEADER).read()
    m = re.search(r"int asr_seq_logprob\(([^;]*)\);", src)
    assert m, "asr_seq_logprob is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const float* logits", "int64_t ld", "const int64_t* tgt", "const int32_t* seg_off", "int R", "int M", "int V",
                      "float* tok_lp", "float* score", "asr_stream_t stream"]
    res, args = L._SIGS["asr_seq_logprob"]
    kinds = [ctypes.c_void_p if "*" in p or "asr_stream_t" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_int for p in params]
    assert res is ctypes.c_int and args == kinds
    before = src[:m.start()]
    comment = before[before.rindex("/*"):]
    assert "log_softmax" in comment and "gather" in comment and "masked sum" in comment
    assert re.search(r"int asr_abi_version\(void\);\s*/\* 4 ", src)
    if os.path.exists(L.LIB_PATH):
        assert L.load().asr_abi_version() == 4 and hasattr(L.load(), "asr_seq_logprob")
