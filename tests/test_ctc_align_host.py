"""CTC forced alignment, host side: the NumPy restatement tests/ctc_align_reference.py against enumeration of all
alignments, its tie rule, torch's ctc_loss as an upper bound, the infeasible cases, and the two precisions of the restatement against each
other on the GPU test's own inputs; then encoder_frame_span, word grouping, the JSON writer and test.py's start-up error."""
import itertools
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_align_reference as R


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


# ------------------------------------------------------------------------------------------------ the restatement
def _path_score(lg, path, target, blank=0):
    return float(sum(np.float64(lg[t, blank if s % 2 == 0 else target[s >> 1]]) for t, s in enumerate(path)))


def test_reference_against_enumeration_of_all_alignments():
    """T <= 6, V = 4, L <= 3, every target over the labels {1, 2, 3} (repeats included): the best raw score over all V ** T frame
    sequences that collapse to the target equals the float64 reference's raw score to 1e-12, the reference's path attains it and
    collapses to the target; where no sequence collapses to it the reference says infeasible."""
    rng = np.random.default_rng(0)
    n = 0
    for T in range(1, 7):
        lg = rng.standard_normal((T, 4)) * 2.0
        lse = float(R.lse_rows(lg).sum())
        for L in range(0, 4):
            for target in itertools.product((1, 2, 3), repeat=L):
                best, arg = R.enumerate_best(lg, target, T)
                r = R.align_one(lg, target, T, dtype=np.float64)
                if arg is None:
                    assert r["path"] is None and r["score"] == -np.inf, (T, target)
                    continue
                assert abs(best - (r["score"] + lse)) <= 1e-12, (T, target, best, r["score"] + lse)
                assert abs(_path_score(lg, r["path"], target) - best) <= 1e-12 and R.collapse(r["path"], target) == list(target)
                assert abs(sum(r["lab_score"]) + sum(lg[t, 0] - R.lse_rows(lg[t]) for t, s in enumerate(r["path"]) if s % 2 == 0)
                           - r["score"]) <= 1e-9
                n += 1
    assert n > 150


def test_tie_rule_on_integer_lattices():
    """All-zero logits: every alignment ties.  Stay wins over advance and the last state wins the final tie, so the path reaches the final
    blank as early as the lattice allows and stays there; then advance against skip, tied and strictly greater."""
    lg = np.zeros((6, 4), dtype=np.float32)
    for dt in (np.float32, np.float64):
        r = R.align_one(lg, [1, 2], 6, dtype=dt)
        assert r["path"] == [1, 3, 4, 4, 4, 4] and r["start"] == [0, 1] and r["end"] == [1, 2], r
        assert R.align_one(lg, [1, 1], 6, dtype=dt)["path"] == [1, 2, 3, 4, 4, 4]      # equal neighbours: no skip, the blank between them
        assert R.align_one(lg, [], 3, dtype=dt)["path"] == [0, 0, 0]
    # the final tie: S_b - 1 unless S_b - 2 is STRICTLY greater
    lg = np.zeros((2, 4), dtype=np.float32)
    assert R.align_one(lg, [1], 2)["path"] == [1, 2]
    lg[1, 1] = 1.0
    assert R.align_one(lg, [1], 2)["path"] == [1, 1]
    # into state 3 at the last frame: staying is worse (-5), advancing from the blank and skipping from label 1 tie at 0 -> advance
    lg = np.zeros((3, 4), dtype=np.float32)
    lg[1, 2], lg[2, 2] = -5.0, 3.0
    assert R.align_one(lg, [1, 2], 3)["path"] == [1, 2, 3]
    lg[1, 1] = 1.0                                                                     # the skip strictly greater -> skip
    assert R.align_one(lg, [1, 2], 3)["path"] == [1, 1, 3]
    lg = np.zeros((2, 4), dtype=np.float32)
    assert R.align_one(lg, [1, 2], 2)["path"] == [1, 3]                                # the only alignment: a skip


def test_score_is_bounded_by_the_sum_over_alignments():
    """The best path is one of the alignments torch's ctc_loss sums over: score <= -F.ctc_loss(sum) in float64, and a peaky posterior
    makes the two meet."""
    rng = np.random.default_rng(1)
    T, V = 40, 9
    for peak in (0.0, 30.0):
        lg = rng.standard_normal((T, V)) * 2.0
        target = [3, 3, 5, 4, 8, 8, 6]
        if peak:
            frames = [0, 3, 0, 3, 5, 4, 8, 0, 8, 6] + [0] * (T - 10)
            for t, c in enumerate(frames):
                lg[t, c] += peak
        lp = F.log_softmax(torch.from_numpy(lg), dim=1)
        nll = F.ctc_loss(lp.unsqueeze(1), torch.tensor([target]), torch.tensor([T]), torch.tensor([len(target)]), reduction="sum").item()
        r = R.align_one(lg, target, T, dtype=np.float64)
        assert r["score"] <= -nll + 1e-9, (r["score"], -nll)
        if peak:
            assert abs(r["score"] + nll) <= 1e-6 and R.collapse(r["path"], target) == target
            assert [lp_t for lp_t in r["start"]] == [1, 3, 4, 5, 6, 8, 9]


def test_infeasible_targets():
    lg = np.random.default_rng(2).standard_normal((3, 5, 6))
    tg = np.array([[3, 3, 9], [3, 4, 5], [3, 0, 9]])
    out = R.align(lg, tg, [2, 2, 5], [2, 3, 2])                 # "3 3" in two frames; L > T_b; a blank inside the target
    assert np.isneginf(out["score"]).all() and (out["path"] == -1).all() and (out["start"] == -1).all() and (out["end"] == -1).all()
    assert (out["lab_score"] == 0).all()
    ok = R.align(lg, tg, [3, 3, 5], [2, 3, 1])                  # one more frame each, and the target cut before the blank
    assert np.isfinite(ok["score"]).all() and ok["path"][0, :3].tolist() == [1, 2, 3] and ok["path"][1, :3].tolist() == [1, 3, 5]
    assert R.align(lg[:1], np.array([[6]]), [5], [1])["score"][0] == -np.inf          # id = V
    assert R.align(lg[:1], np.array([[3]]), [0], [1])["score"][0] == -np.inf and R.align(lg[:1], np.array([[3]]), [0], [0])["score"][0] == 0.0


def test_both_precisions_agree_on_the_gpu_cases():
    """The GPU test takes path / start / end from the float32 restatement and the scores from the float64 one; that is one yardstick only
    if both walk the same path on those inputs.  They do, and the float32 raw score stays within 3e-7 relative of float64 up to T 625,
    which leaves the 2e-5 bound of the GPU test about 70x room; the rounding of T sequential adds grows with T, and the one longer case
    (T 1100, there for the workspace arm) is held to 1e-6, 20x room."""
    for name, c in R.cases().items():
        a32 = R.align(dtype=np.float32, **c)
        a64 = R.align(dtype=np.float64, **c)
        for k in ("path", "start", "end"):
            assert np.array_equal(a32[k], a64[k]), (name, k)
        fin = np.isfinite(a64["score"])
        assert np.array_equal(fin, np.isfinite(a32["score"])), name
        err = np.abs(a32["score"][fin] - a64["score"][fin]) / np.maximum(1.0, np.abs(a64["score"][fin]))
        print("%s: float32 recursion within %.2e of float64" % (name, err.max() if err.size else 0.0))
        T = c["logits"].shape[1]
        assert (err <= (3e-7 if T <= 625 else 1e-6)).all(), (name, err)
        for b in range(len(fin)):
            Lb, Tb = c["target_lengths"][b], c["input_lengths"][b]
            if fin[b]:
                assert R.collapse(a32["path"][b, :Tb].tolist(), c["targets"][b]) == [int(x) for x in c["targets"][b, :Lb]]
            assert (a32["path"][b, Tb:] == -1).all() and (a32["start"][b, Lb:] == -1).all() and T >= Tb
    e = R.align(**R.cases()["edges"])
    assert np.isfinite(e["score"]).tolist() == [True, True, False, False, False, False, False, True] and e["score"][1] == 0.0


# ------------------------------------------------------------------------------------------------ frames to seconds
@pytest.mark.parametrize("feat", ["vgg_cnn", "emb_cnn", "none"])
def test_encoder_frame_span_tiles_the_input(feat):
    """The spans of the frames_after_cnn(n) encoder frames of an n-frame input follow one another without gap or overlap, are as wide as
    the front end's stride, and after the clamp to n lie inside [0, n); vgg_cnn leaves at most the 3 frames its pools drop, emb_cnn
    starts at its first cell's centre."""
    from models.asr.transformer import encoder_frame_span, frames_after_cnn
    stride = {"vgg_cnn": 4, "emb_cnn": 2, "none": 1}[feat]
    first = {"vgg_cnn": 0, "emb_cnn": 4, "none": 0}[feat]
    for n in range(24, 60):
        m = frames_after_cnn(n, feat)
        spans = [encoder_frame_span(j, feat) for j in range(m)]
        assert m >= 1 and spans[0][0] == first
        assert all(b - a == stride for a, b in spans) and all(spans[j][1] == spans[j + 1][0] for j in range(m - 1))
        assert all(0 <= a < n and min(b, n) > a for a, b in spans)
        assert n - spans[-1][1] < {"vgg_cnn": 4, "emb_cnn": 7, "none": 1}[feat]
        if feat == "emb_cnn":                        # the centre cell of the receptive field [2j - 10, 2j + 20]
            assert all(a == (2 * j - 10 + 2 * j + 20) // 2 - 1 for j, (a, b) in enumerate(spans))


# ------------------------------------------------------------------------------------------------ words and the writer
def _timed(text, logp=-0.5):
    return [{"id": 3 + i, "label": ch, "start": 0.04 * i, "end": 0.04 * i + 0.04 * (1 + i % 2), "logp": logp * (1 + i % 2), "frames": 1 + i % 2}
            for i, ch in enumerate(text)]


def test_word_grouping_mixed_english_chinese():
    from utils.align import group_words
    labs = _timed("hi 你好ok  a")
    words = group_words(labs)
    assert [w["word"] for w in words] == ["hi", "你", "好", "ok", "a"]
    assert words[0]["start"] == labs[0]["start"] and words[0]["end"] == labs[1]["end"]
    assert words[3]["start"] == labs[5]["start"] and words[3]["end"] == labs[6]["end"]
    assert all(abs(w["logp"] + 0.5) <= 1e-12 for w in words)                   # every frame of every label carries -0.5
    labs[0]["logp"], labs[0]["frames"] = -3.0, 1
    assert abs(group_words(labs)[0]["logp"] - (-3.0 - 1.0) / 3) <= 1e-12        # "h" one frame at -3, "i" two frames at -0.5 each
    assert group_words([]) == [] and group_words(_timed("  ")) == []


def test_records_and_writer(tmp_path):
    from utils.align import AlignmentWriter, utterance_record
    ali = {"score": -7.5, "frames": 5, "path": [0, 1, 1, 2, 3],
           "labels": [{"id": 4, "label": "a", "start_frame": 1, "end_frame": 3, "logp": -1.0},
                      {"id": 5, "label": "b", "start_frame": 4, "end_frame": 5, "logp": -0.25}]}
    rec = utterance_record(7, "ab", ali, "vgg_cnn", 0.01, 19)
    assert rec["utt"] == 7 and rec["text"] == "ab" and rec["score"] == -7.5 and abs(rec["score_per_frame"] + 1.5) <= 1e-12
    assert [(l["label"], l["id"]) for l in rec["labels"]] == [("a", 4), ("b", 5)] and "frames" not in rec["labels"][0]
    assert abs(rec["labels"][0]["start"] - 0.04) <= 1e-12 and abs(rec["labels"][0]["end"] - 0.12) <= 1e-12
    assert abs(rec["labels"][1]["start"] - 0.16) <= 1e-12 and abs(rec["labels"][1]["end"] - 0.19) <= 1e-12      # clamped to 19 input frames
    assert len(rec["words"]) == 1 and rec["words"][0]["word"] == "ab" and abs(rec["words"][0]["logp"] + 1.25 / 3) <= 1e-12
    assert rec["words"][0]["start"] == rec["labels"][0]["start"] and rec["words"][0]["end"] == rec["labels"][1]["end"]
    emb = utterance_record(0, "ab", ali, "emb_cnn", 0.01, 100)
    assert abs(emb["labels"][0]["start"] - 0.06) <= 1e-12 and abs(emb["labels"][0]["end"] - 0.10) <= 1e-12
    bad = utterance_record(8, "zz", {"score": -math.inf, "frames": 5, "path": [], "labels": []}, "vgg_cnn", 0.01, 19)
    assert bad == {"utt": 8, "text": "zz", "score": None, "score_per_frame": None, "labels": [], "words": []}
    path = tmp_path / "ali.jsonl"
    with AlignmentWriter(str(path)) as w:
        w.write(rec)
        w.write(bad)
        w.write(utterance_record(9, "你", {"score": -1.0, "frames": 1, "path": [1], "labels": [
            {"id": 6, "label": "你", "start_frame": 0, "end_frame": 1, "logp": -1.0}]}, "none", 0.01, 1))
        assert w.count == 3
    lines = path.read_text(encoding="utf-8").splitlines()
    assert len(lines) == 3 and json.loads(lines[0]) == rec and json.loads(lines[1])["score"] is None
    assert "你" in lines[2] and json.loads(lines[2])["words"][0]["word"] == "你"


def test_hypothesis_labels_strip_sos_eos_and_trailing_pad():
    from models.asr.transformer import hypothesis_labels
    assert hypothesis_labels([1, 5, 6, 6, 2]) == [5, 6, 6] and hypothesis_labels([5, 0, 0]) == [5] and hypothesis_labels([1, 2]) == []
    assert hypothesis_labels([1, 5, 0, 6, 2]) == [5, 0, 6]                      # a blank inside stays: the aligner reports it infeasible


# ------------------------------------------------------------------------------------------------ the command line
FLAGS = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 12 "
         "--src-max-len 64").split()


def _model(cli, extra=()):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, "a", "b", " "]
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, {i: c for c, i in l2i.items()})


def test_align_out_flags_and_start_up_error(cli, tmp_path):
    import test as test_mod
    a = cli([])
    assert a.align_out is None and a.align_source == "gold"
    a = cli(["--align-out", "x.jsonl", "--align-source", "hyp"])
    assert a.align_out == "x.jsonl" and a.align_source == "hyp"
    with pytest.raises(SystemExit):
        cli(["--align-source", "attention"])
    plain, head = _model(cli), _model(cli, ["--ctc-weight", "0.3"])
    with pytest.raises(ValueError, match="CTC head"):
        test_mod.check_ctc_decoding(cli(["--align-out", str(tmp_path / "a.jsonl")]), plain)
    test_mod.check_ctc_decoding(cli(["--align-out", str(tmp_path / "a.jsonl")]), head)
    test_mod.check_ctc_decoding(cli([]), plain)
    # the model's own entry points refuse the same before any device work
    x = torch.zeros(1, 1, 161, 8)
    with pytest.raises(ValueError, match="CTC head"):
        plain.evaluate(x, [8], torch.zeros(1, 2, dtype=torch.int64), align_source="gold", target_lengths=[2])
    with pytest.raises(ValueError, match="CTC head"):
        plain.ctc_align(torch.zeros(1, 2, 32), [2], [[3]])
    with pytest.raises(ValueError, match="align_source"):
        head.evaluate(x, [8], torch.zeros(1, 2, dtype=torch.int64), align_source="attention")
    with pytest.raises(ValueError, match="target_lengths"):
        head.evaluate(x, [8], torch.zeros(1, 2, dtype=torch.int64), align_source="gold")
    assert not (tmp_path / "a.jsonl").exists()
