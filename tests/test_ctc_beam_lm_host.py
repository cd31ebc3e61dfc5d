"""The fused arm of the CTC prefix beam search, host side: the float64 restatement tests/ctc_beam_lm_reference.py
against the plain restatement (LM switched off), against brute force over all alignments (nothing pruned), and the conditions under
which tests/test_gpu_ctc_beam_lm.py may hold the kernel to it, asserted here so that the GPU test cannot hide a failure behind them."""
import numpy as np
import pytest

import ctc_beam_lm_reference as M
import ctc_beam_reference as R


@pytest.mark.parametrize("name", ["small_w3", "small_w4"])
@pytest.mark.parametrize("eos", [M.EOS, -1])
def test_switched_off_it_is_the_plain_search(name, eos):
    """alpha = beta = 0: the fused key is the CTC score itself and the end term weighs nothing, so the restatement returns exactly what
    ctc_beam_reference.search returns; lm still reports the LM's sum."""
    c = R.cases_cached()[name]
    lm = M.synthetic_lm(c["logits"].shape[2])
    got = M.search(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], lm, 0.0, 0.0, M.BOS, eos)
    ref = R.expected(name)
    for k in ("ids", "lengths", "scores"):
        assert np.array_equal(got[k], ref[k]), (name, k)
    assert np.all(got["fused"][got["lengths"] >= 0] == 0.0)
    for b in range(len(c["lengths"])):
        for n in range(c["nbest"]):
            if got["lengths"][b, n] >= 0:
                g = got["ids"][b, n, :got["lengths"][b, n]].tolist()
                assert abs(got["lm"][b, n] - lm.score(g, M.BOS, eos)) <= 1e-5 * max(1.0, abs(got["lm"][b, n]))


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_unpruned_keys_equal_brute_force(order):
    """The "exhaustive" case (T 3, V 3, W 16: nothing is pruned): every hypothesis' final key is the log of the summed probability of all
    its alignments (enumerate_all) + alpha * NgramLM.score + beta * len -- a route that shares no code with the search --, every sequence
    with an alignment is returned, and the order is by that key."""
    c = R.cases_cached()["exhaustive"]
    lm = M.synthetic_lm(3, order)
    for eos in (M.EOS, -1):
        r = M.search(c["logits"], c["lengths"], 16, 3, 16, lm, M.ALPHA, M.BETA, M.BOS, eos)
        for b in range(2):
            truth = R.enumerate_all(c["logits"][b].astype(np.float64), 3)
            n = int((r["lengths"][b] >= 0).sum())
            assert n == len(truth)
            want = {g: p + M.ALPHA * lm.score(g, M.BOS, eos) + M.BETA * len(g) for g, p in truth.items()}
            for k in range(n):
                g = tuple(r["ids"][b, k, :r["lengths"][b, k]].tolist())
                assert abs(r["keys"][b, k] - want[g]) <= 1e-6 * max(1.0, abs(want[g])), (b, g)
                assert abs(r["scores"][b, k] - truth[g]) <= 1e-10
                assert abs(r["fused"][b, k] - (want[g] - truth[g])) <= 1e-6
            assert np.all(np.diff(r["keys"][b, :n]) <= 0)
            assert [tuple(r["ids"][b, k, :r["lengths"][b, k]]) for k in range(n)] == sorted(want, key=lambda g: -want[g])


def test_the_lm_changes_which_prefixes_survive():
    """With the LM on, the small cases' n-best differ from the plain search's somewhere (else the GPU tests would test nothing new), and a
    one-frame example: two labels with near-equal posteriors, the LM's favourite wins."""
    changed = 0
    for name in ("small_w3", "small_w4", "mid"):
        changed += int(not np.array_equal(M.expected(name)["ids"], R.expected(name)["ids"]))
    assert changed >= 1
    lg, lm = M.lm_decides_case()
    plain = R.search(lg, [lg.shape[1]], 4, 3, 4)
    fused = M.search(lg, [lg.shape[1]], 4, 3, 4, lm, M.ALPHA, 0.0, M.BOS, M.EOS)
    assert plain["ids"][0, 0, :plain["lengths"][0, 0]].tolist() == [1] and fused["ids"][0, 0, :fused["lengths"][0, 0]].tolist() == [2]
    for r in (plain, fused):
        assert min(r["prune_margin"][0], r["lineage_margin"][0], r["top_margin"][0]) >= R.DELTA
    lg = M.beta_decides_case()
    lm = M.synthetic_lm(3)
    plain = M.search(lg, [2], 4, 3, 4, lm, 0.0, 0.0, M.BOS, -1)
    bonus = M.search(lg, [2], 4, 3, 4, lm, 0.0, 2.0, M.BOS, -1)
    assert plain["lengths"][0, 0] == 0 and bonus["lengths"][0, 0] == 1 and bonus["ids"][0, 0, 0] == 1
    assert min(bonus["prune_margin"][0], bonus["lineage_margin"][0], bonus["top_margin"][0]) >= R.DELTA


@pytest.mark.parametrize("V", [3, 5])
@pytest.mark.parametrize("W", [3, 5])
def test_conditions_of_the_sweep(V, W):
    """Of the 200 drawn utterances per (V, W) at least 180 pass the margin filter under the trigram LM, alpha 0.5, beta 0.3; no n-best
    holds a sequence twice; the final keys do not increase."""
    lg, tb, r = M.sweep(V, W)
    print("V %d W %d: %d of %d utterances kept" % (V, W, len(tb), M.SWEEP_DRAWS))
    assert M.SWEEP_DRAWS == 200 and (M.ALPHA, M.BETA) == (0.5, 0.3) and M.synthetic_lm(V).order == 3
    assert len(tb) >= 180
    for b in range(len(tb)):
        rows = [tuple(r["ids"][b, k, :r["lengths"][b, k]]) for k in range(W) if r["lengths"][b, k] >= 0]
        assert len(set(rows)) == len(rows)
        assert np.all(np.diff(r["keys"][b, :len(rows)]) <= 0)


@pytest.mark.parametrize("name,order,eos", [("small_w3", 3, M.EOS), ("small_w4", 3, M.EOS), ("small_w3", 3, -1), ("small_w4", 1, M.EOS),
                                            ("small_w4", 2, M.EOS), ("small_w4", 4, M.EOS), ("mid", 3, M.EOS),
                                            ("widest_slot_set", 3, M.EOS)])
def test_conditions_of_the_gpu_cases(name, order, eos):
    """Every case the GPU test runs: lineage_margin and top_margin at least delta for every utterance (the best hypothesis is decided),
    the small cases' prune_margin too (the whole n-best is compared).  The larger cases' prune margins are printed: a fused key is some
    ten times a CTC score (alpha times the LM's sum over 20 labels), so a relative gap of delta is ten times as wide in absolute terms and
    the 8 or 16 entries of their lists rarely all keep it over 75 frames; there the best hypothesis is what is compared."""
    r = M.expected(name, order, eos)
    print(name, order, eos, "prune", r["prune_margin"], "lineage", r["lineage_margin"], "top", r["top_margin"])
    assert np.all(r["lineage_margin"] >= R.DELTA) and np.all(r["top_margin"] >= R.DELTA)
    if R.cases_cached()[name]["small"]:
        assert np.all(r["prune_margin"] >= R.DELTA)


def test_conditions_of_the_relink_inputs():
    for lg, W in ((R.RELINK_A, 4), (R.RELINK_B, 3)):
        x = np.array([lg], dtype=np.float32)
        r = M.search(x, [len(lg)], W, 3, W, M.synthetic_lm(3), M.ALPHA, M.BETA, M.BOS, M.EOS)
        assert min(r["prune_margin"][0], r["lineage_margin"][0], r["top_margin"][0]) >= R.DELTA
