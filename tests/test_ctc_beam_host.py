"""CTC prefix beam search, host side: the NumPy restatement tests/ctc_beam_reference.py against enumeration of all
alignments and torch's ctc_loss (unpruned beam), its merge and tie rules, T_b = 0, the doubled label, and the conditions under which
tests/test_gpu_ctc_beam.py may hold the kernel to it (asserted here, so that the GPU test cannot hide a failure behind them); then the
command line's flag and start-up errors."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_beam_reference as R


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


# ------------------------------------------------------------------------------------------------ the restatement
def test_unpruned_beam_equals_enumeration_and_ctc_loss():
    """T <= 5, V <= 4, C = V and W larger than the number of label sequences: nothing is pruned, so the search returns EVERY sequence that
    has an alignment, each with the log of the summed probability of all its alignments -- by brute force over the V ** T alignments to
    1e-10, and equal to -F.ctc_loss(reduction='sum') in float64 to 1e-9."""
    rng = np.random.default_rng(0)
    n = 0
    for T, V in ((1, 2), (2, 3), (3, 3), (4, 4), (5, 4), (5, 3)):
        lg = rng.standard_normal((T, V)) * 2.0
        truth = R.enumerate_all(lg, T)
        r = R.search_one(lg, T, W=4096, C=V, nbest=4096)
        assert sorted(map(tuple, r["seqs"])) == sorted(truth) and r["prune_margin"] > 0
        assert r["scores"] == sorted(r["scores"], reverse=True)
        lp = torch.from_numpy(lg).log_softmax(-1).unsqueeze(1)
        for g, s in zip(r["seqs"], r["scores"]):
            assert abs(s - truth[tuple(g)]) <= 1e-10, (T, V, g, s, truth[tuple(g)])
            if g:
                nll = F.ctc_loss(lp, torch.tensor([g]), torch.tensor([T]), torch.tensor([len(g)]), blank=0, reduction="sum")
                assert abs(s + float(nll)) <= 1e-9, (T, V, g)
            n += 1
        assert abs(np.logaddexp.reduce(r["scores"])) <= 1e-10                    # the sequences partition the alignments
    assert n > 150


def test_merge_rule_adds_both_routes():
    """"a" and "ab" are in the list and "b" is a candidate: "ab" is reached by repeating its b and by extending "a" with b.  Both routes
    land in the stay slot of "ab" (probabilities add), no second "ab" appears, and "a" extended by ITS last label starts from p_b only."""
    a, b = 1, 2
    lp = np.log(np.array([0.5, 0.2, 0.3]))
    state = [((a,), math.log(0.3), math.log(0.1)), ((a, b), math.log(0.05), math.log(0.02))]
    new, slots = R.step(state, lp, [b, a], W=8, C=2)
    got = {g: (pb, pnb) for g, pb, pnb in new}
    assert [g for g, _, _ in new].count((a, b)) == 1 and len(new) == len(got) == 5
    assert abs(math.exp(got[(a, b)][1]) - (0.02 * 0.3 + (0.3 + 0.1) * 0.3)) <= 1e-15          # repeat + extension of "a"
    assert abs(math.exp(got[(a, b)][0]) - (0.05 + 0.02) * 0.5) <= 1e-15
    assert abs(math.exp(got[(a,)][1]) - 0.1 * 0.2) <= 1e-15 and abs(math.exp(got[(a,)][0]) - 0.4 * 0.5) <= 1e-15
    assert got[(a, a)][0] == -np.inf and abs(math.exp(got[(a, a)][1]) - 0.3 * 0.2) <= 1e-15      # through the blank only
    assert abs(math.exp(got[(a, b, a)][1]) - 0.07 * 0.2) <= 1e-15 and abs(math.exp(got[(a, b, b)][1]) - 0.05 * 0.3) <= 1e-15
    # the operand order of the merged log-add is (repeat term, extension term)
    assert got[(a, b)][1] == R.lae2(math.log(0.02) + lp[b], R.lae2(math.log(0.3), math.log(0.1)) + lp[b])
    # the dead extension slot W + 0 * C + 0 is not among the finite slots
    assert sorted(s[0] for s in slots) == [0, 1, 8 + 1, 8 + 2, 8 + 2 + 1]
    # a pruned prefix is gone: without "ab" in the list the extension starts from the extension term alone
    new, _ = R.step(state[:1], lp, [b, a], W=8, C=2)
    got = {g: (pb, pnb) for g, pb, pnb in new}
    assert got[(a, b)][0] == -np.inf and abs(math.exp(got[(a, b)][1]) - 0.4 * 0.3) <= 1e-15


def test_tie_rules_of_candidates_and_prune():
    """All-zero logits tie everything: the candidates are the lowest indices, and the slots keep their index order -- the stay slot, then
    the extensions by candidate position."""
    lg = np.zeros((2, 4), dtype=np.float32)
    assert R.candidates(lg[0], 4) == [1, 2, 3] and R.candidates(lg[0], 2) == [1] and R.candidates(np.array([0., 1, 1, 0]), 2) == [1, 2]
    for dt in (np.float32, np.float64):
        assert R.search_one(lg, 1, W=2, C=4, nbest=2, dtype=dt)["seqs"] == [[], [1]]
        assert R.search_one(lg, 1, W=3, C=4, nbest=3, dtype=dt)["seqs"] == [[], [1], [2]]
        r = R.search_one(lg, 1, W=2, C=4, nbest=2, dtype=dt)
        assert r["prune_margin"] == 0.0 and r["top_margin"] == 0.0
    # the slot index decides among equals, whatever the order of the list: "2" before "1" in the list keeps its extensions first
    lp = np.log(np.full(3, 1 / 3))
    state = [((2,), math.log(0.25), -np.inf), ((1,), math.log(0.25), -np.inf)]
    _, slots = R.step(state, lp, [1, 2], W=4, C=2)
    assert [s[0] for s in slots] == [0, 1, 4, 5, 6, 7] and [s[1] for s in slots[2:]] == [(2, 1), (2, 2), (1, 1), (1, 2)]


def test_no_frames_returns_the_empty_prefix():
    lg = np.full((3, 4), np.nan, dtype=np.float32)
    r = R.search_one(lg, 0, W=4, C=4, nbest=4)
    assert r["seqs"] == [[]] and r["scores"] == [0.0] and r["prune_margin"] == r["top_margin"] == r["lineage_margin"] == np.inf
    out = R.search(lg[None], [0], 4, 4, 4)
    assert out["lengths"].tolist() == [[0, -1, -1, -1]] and out["scores"][0, 0] == 0.0 and np.all(out["scores"][0, 1:] == -np.inf)
    assert np.array_equal(R.search(lg[None], [-3], 4, 4, 4)["lengths"], out["lengths"])          # clamped


def test_doubled_label_needs_its_blank():
    lg = np.full((3, 4), -4.0, dtype=np.float32)
    lg[0, 2] = lg[1, 0] = lg[2, 2] = 4.0
    assert R.search_one(lg, 3, W=4, C=4)["seqs"] == [[2, 2]]
    lg[1, 0], lg[1, 2] = -4.0, 4.0
    assert R.search_one(lg, 3, W=4, C=4)["seqs"] == [[2]]
    assert R.search_one(lg, 3, W=1, C=1)["seqs"] == [[2]]


def test_pruned_parent_created_again_merges_into_its_child():
    """"1" is pruned while "1 1" / "1 2 1" stay in the list, and is created again later: its extension is merged into the old child
    because the restatement knows prefixes by their labels.  A search that knew them by their place of creation would return [1,2,1] twice
    (-3.216, -3.784) on the first input and [2,1,1] -2.2406 as the best of the second."""
    a = R.search_one(np.array(R.RELINK_A), 5, W=4, C=3, nbest=4)
    assert a["seqs"] == [[1, 1], [1], [1, 2, 1], [1, 1, 2]] and a["relinked"] >= 1
    assert np.allclose(a["scores"], [-0.818, -1.045, -2.767, -4.622], atol=1e-3)
    b = R.search_one(np.array(R.RELINK_B), 6, W=3, C=3, nbest=3)
    assert b["seqs"][0] == [2, 1, 2, 1] and abs(b["scores"][0] + 2.1125) <= 1e-4 and b["relinked"] >= 1
    for r in (a, b):
        assert min(r["prune_margin"], r["lineage_margin"], r["top_margin"]) >= R.DELTA
        assert len(set(map(tuple, r["seqs"]))) == len(r["seqs"])
    # unpruned, the same sequences have at least these scores, and every sequence is an enumerated one
    truth = R.enumerate_all(np.array(R.RELINK_A), 5)
    assert all(s <= truth[tuple(g)] + 1e-12 for g, s in zip(a["seqs"], a["scores"]))


@pytest.mark.parametrize("V", [3, 4, 5, 6])
def test_conditions_of_the_sweep(V):
    """The GPU sweep's batches: at least 400 of the 500 drawn utterances pass the margin filter, every batch holds utterances that merge
    into the child of a re-created parent, no n-best holds a sequence twice, and the float32 restatement returns the same sequences."""
    hits = 0
    for W in (3, 4, 5):
        lg, tb, r = R.sweep(V, W)
        n = int((r["relinked"] > 0).sum())
        print("V %d W %d: %d utterances kept, %d with a re-created parent" % (V, W, len(tb), n))
        assert len(tb) >= 400 and n >= 1
        hits += n
        r32 = R.search(lg, tb, W, V, W, dtype=np.float32)
        assert np.array_equal(r32["ids"], r["ids"]) and np.array_equal(r32["lengths"], r["lengths"])
        for b in range(len(tb)):
            rows = [tuple(r["ids"][b, k, :r["lengths"][b, k]]) for k in range(W) if r["lengths"][b, k] >= 0]
            assert len(set(rows)) == len(rows)
    assert hits >= 8


# ------------------------------------------------------------------------------------------------ the conditions of the GPU cases
def test_shapes_of_the_gpu_cases():
    shapes = {k: c["logits"].shape + (c["W"], c["C"], c["nbest"]) for k, c in R.cases_cached().items()}
    assert shapes == {"exhaustive": (2, 3, 3, 16, 3, 16), "small_w3": (6, 12, 6, 3, 3, 3), "small_w4": (6, 24, 12, 4, 4, 4),
                      "mid": (8, 75, 40, 8, 8, 8), "widest_slot_set": (4, 75, 4364, 16, 16, 16), "long": (2, 400, 40, 8, 16, 8)}
    for name in ("small_w3", "small_w4"):
        assert {0, 1} <= set(R.cases_cached()[name]["lengths"])
    assert R.DELTA == 2 * 2e-5


@pytest.mark.parametrize("name", ["exhaustive", "small_w3", "small_w4", "mid", "widest_slot_set", "long"])
def test_conditions_of_the_gpu_cases(name):
    """delta = 4e-5, twice the GPU test's score tolerance.  Small cases: every utterance's prune_margin >= delta (so the whole n-best is
    compared); every case: lineage_margin and top_margin >= delta for every utterance (so the best hypothesis is decided); larger cases: at
    most one utterance in four below delta; and the float32 restatement returns the float64 one's sequences, scores within 2e-6."""
    c = R.cases_cached()[name]
    r64, r32 = R.expected(name), R.expected(name, "float32")
    B = len(c["lengths"])
    print(name, "prune", r64["prune_margin"], "lineage", r64["lineage_margin"], "top", r64["top_margin"])
    assert np.all(r64["lineage_margin"] >= R.DELTA) and np.all(r64["top_margin"] >= R.DELTA)
    if c["small"]:
        assert np.all(r64["prune_margin"] >= R.DELTA)
    else:
        assert int((r64["prune_margin"] < R.DELTA).sum()) * 4 <= B
    assert np.array_equal(r64["ids"], r32["ids"]) and np.array_equal(r64["lengths"], r32["lengths"])
    fin = np.isfinite(r64["scores"])
    assert np.array_equal(fin, np.isfinite(r32["scores"]))
    rel = np.abs(r64["scores"][fin] - r32["scores"][fin]) / np.maximum(1.0, np.abs(r64["scores"][fin]))
    print(name, "float32 against float64: worst relative score difference %.2e" % rel.max())
    assert rel.max() <= 2e-6
    if name == "exhaustive":                              # nothing is pruned: the scores are exact CTC likelihoods
        for b in range(B):
            truth = R.enumerate_all(c["logits"][b].astype(np.float64), 3)
            assert int((r64["lengths"][b] >= 0).sum()) == len(truth) <= 15
            for n in range(len(truth)):
                g = tuple(r64["ids"][b, n, :r64["lengths"][b, n]].tolist())
                assert abs(r64["scores"][b, n] - truth[g]) <= 1e-10


def test_planted_inputs_hold_a_doubled_label():
    """Every full-length utterance of the planted cases decodes to a sequence whose second label repeats its first."""
    for name in ("small_w4", "mid", "widest_slot_set", "long"):
        c, r = R.cases_cached()[name], R.expected(name)
        T = c["logits"].shape[1]
        full = [b for b, n in enumerate(c["lengths"]) if n == T]
        assert full and all(r["lengths"][b, 0] >= 2 and r["ids"][b, 0, 0] == r["ids"][b, 0, 1] for b in full), name


# ------------------------------------------------------------------------------------------------ the command line
FLAGS = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 12 "
         "--src-max-len 64").split()


def _model(cli, extra=()):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, "a", "b", " "]
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(FLAGS + list(extra)), l2i, {i: c for c, i in l2i.items()})


def test_ctc_beam_search_flag_and_start_up_errors(cli):
    import test as test_mod
    assert cli([]).ctc_beam_search is False
    assert cli(["--ctc-beam-search", "--beam-width", "8"]).ctc_beam_search is True
    plain, head = _model(cli), _model(cli, ["--ctc-weight", "0.3"])
    with pytest.raises(ValueError, match="CTC head"):
        test_mod.check_ctc_decoding(cli(["--ctc-beam-search"]), plain)
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search"]), head)
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--beam-width", "16", "--ctc-candidates", "16", "--lm-rescoring"]), head)
    for extra in (["--beam-search"], ["--ctc-greedy"], ["--ctc-decode-weight", "0.3"], ["--beam-search", "--ctc-decode-weight", "0.3"]):
        with pytest.raises(ValueError, match="--ctc-beam-search"):
            test_mod.check_ctc_decoding(cli(["--ctc-beam-search"] + extra), head)
    for width in ("0", "17", "-1"):
        with pytest.raises(ValueError, match=r"1\.\.16"):
            test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--beam-width", width]), head)
    with pytest.raises(ValueError, match=r"0\.\.16"):
        test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--ctc-candidates", "17"]), head)
    test_mod.check_ctc_decoding(cli(["--beam-search", "--beam-width", "20"]), head)          # the limit is the CTC search's alone
    # the model's own entry points refuse the same before any device work
    x = torch.zeros(1, 1, 161, 8)
    tgt = torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="CTC head"):
        plain.evaluate(x, [8], tgt, ctc_beam=True, beam_width=4)
    with pytest.raises(ValueError, match="CTC head"):
        plain.ctc_beam_search(torch.zeros(1, 2, 32), [2], 4)
    for kw in (dict(beam_search=True), dict(ctc_greedy=True), dict(beam_search=True, ctc_weight=0.3)):
        with pytest.raises(ValueError, match="CTC head alone"):
            head.evaluate(x, [8], tgt, ctc_beam=True, beam_width=4, **kw)
    with pytest.raises(ValueError, match="lm_rescoring"):
        head.evaluate(x, [8], tgt, ctc_beam=True, beam_width=4, lm_rescoring=True)
    for width in (0, 17):
        with pytest.raises(ValueError, match=r"1\.\.16"):
            head.ctc_beam_search(torch.zeros(1, 2, 32), [2], width)
