"""Phrase biasing of the CTC prefix beam search, host side: utils/context.py against a brute-force evaluation of
its definition, its compressed table against its own goto function, the file and the refusals, the ABI and the flags; then the float64
restatement tests/ctc_beam_ctx_reference.py against the restatements it extends (gamma = 0) and the conditions under which
tests/test_gpu_ctc_beam_ctx.py may hold the kernel to it, asserted here so that the GPU test cannot hide a failure behind them."""
import ctypes
import re

import numpy as np
import pytest

import ctc_beam_ctx_reference as X
import ctc_beam_lm_reference as M
import ctc_beam_reference as R
from utils.context import ContextGraph, pack
from utils.ngram import hash_slot


# ------------------------------------------------------------------------------------------------ the automaton
def _brute(phrases, y):
    """(state as a label tuple, credit, hold of the state) of y straight from the definition: string comparisons and scans."""
    phrases = {tuple(p) for p in phrases}
    P = {p[:n] for p in phrases for n in range(len(p) + 1)} | {()}

    def state(z):
        return next(z[i:] for i in range(len(z) + 1) if z[i:] in P)

    def T(u):
        return max([n for n in range(1, len(u) + 1) if u[:n] in phrases], default=0)
    y = tuple(y)
    credit = 0
    for i in range(1, len(y) + 1):
        s = state(y[:i])
        if s in phrases:
            credit += len(s) - T(s[:-1])
    s = state(y)
    return s, credit + len(s) - T(s), len(s) - T(s)


def _random_graph(rng, V):
    phrases = [rng.integers(1, V, size=int(rng.integers(1, 5))).tolist() for _ in range(int(rng.integers(1, 7)))]
    return phrases, ContextGraph.from_phrases(phrases, V, reserved=(0,))


def _labels_of(graph, s):
    out = []
    while s:
        out.append(next(c for c, v in graph.child[graph.parent[s]].items() if v == s))
        s = graph.parent[s]
    return tuple(reversed(out))


@pytest.mark.parametrize("V", [4, 12])
def test_walk_equals_the_definition_by_brute_force(V):
    """1200 random sequences per V (2400 in all) over 120 random phrase lists: state, credit and earned of ContextGraph.walk are what
    the definition gives by string comparison and scanning; a step's delta is the difference of two credits."""
    rng = np.random.default_rng(70 + V)
    for _ in range(120):
        phrases, graph = _random_graph(rng, V)
        for _ in range(10):
            y = rng.integers(1, V, size=int(rng.integers(0, 11))).tolist()
            s, credit = graph.walk(y)
            want_state, want, want_hold = _brute(phrases, y)
            assert _labels_of(graph, s) == want_state and credit == want, (phrases, y)
            assert int(graph.hold[s]) == want_hold and graph.earned(y) == want - want_hold
            if y:
                s0, c0 = graph.walk(y[:-1])
                assert graph.step(s0, y[-1]) == (s, credit - c0)


def _graph(*phrases):
    return ContextGraph.from_phrases([list(p) for p in phrases], 8, reserved=(0,))


def test_hand_cases():
    a, b, c, d, x = 1, 2, 3, 4, 5
    g = _graph((a, b), (a, b, c))                                  # a phrase that continues another
    assert [g.walk(y)[1] for y in ([a], [a, b], [a, b, c], [a, b, x], [a, b, c, x])] == [1, 2, 3, 2, 3]
    assert g.earned([a, b, c]) == 3 and g.earned([a]) == 0 and g.earned([a, b, x]) == 2    # a completed phrase keeps its labels
    g = _graph((a, b), (b, c))                                     # overlapping phrases are each credited
    assert g.walk([a, b, c])[1] == 4 and g.earned([a, b, c]) == 4
    g = _graph((a, b, c, d), (b, c, x))                            # the match moves over to the other phrase, which completes
    assert [g.walk(y)[1] for y in ([a], [a, b], [a, b, c], [a, b, c, x])] == [1, 2, 3, 3]
    assert g.earned([a, b, c]) == 0 and g.earned([a, b, c, x]) == 3
    g = _graph((a, b, c, d), (b, c))                               # a phrase strictly inside another's partial match is not credited
    assert g.walk([a, b, c])[1] == 3 and g.earned([a, b, c]) == 0 and g.walk([a, b, c, x]) == (0, 0)
    assert g.earned([b, c]) == 2 and g.earned([a, b, c, d]) == 4
    g = _graph((a,))                                               # a single label
    assert [g.earned(y) for y in ([a], [a, a], [x, a], [x], [])] == [1, 2, 1, 0, 0]
    g = _graph((a, b, c))                                          # a broken match nets 0
    assert [g.walk(y)[1] for y in ([a], [a, b], [a, b, x])] == [1, 2, 0] and g.step(g.walk([a, b])[0], x) == (0, -2)
    assert _graph((a, b), (a, b), (a, b)).phrases == [(a, b)]      # duplicates merge


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("V", [4, 12])
def test_compressed_table_equals_the_goto_function(V):
    """Of 60 random graphs per V: the device's lookup rule on the host equals step() for EVERY (state, label), labels outside the table's
    range and states outside the graph included; every stored key is found within max_probe; the capacity is a power of two; only the
    transitions the rule needs are stored."""
    rng = np.random.default_rng(80 + V)
    for _ in range(60):
        phrases, graph = _random_graph(rng, V)
        table = graph.hash_table()
        keys, vals, max_probe = table
        cap = len(keys)
        assert cap >= 16 and cap & (cap - 1) == 0 and max_probe >= 1 and keys.dtype == np.uint64 and vals.dtype == np.int32
        stored, svals = graph.transitions()
        assert np.count_nonzero(keys) == len(stored) <= cap // 2 and len(set(stored.tolist())) == len(stored)
        for k, v in zip(stored.tolist(), svals.tolist()):
            slot = graph.find(table, k)
            home = int(hash_slot(np.array([k], dtype=np.uint64), cap)[0])
            assert slot >= 0 and ((slot - home) & (cap - 1)) < max_probe and vals[slot].tolist() == v
        for s in range(graph.states):
            for c in range(V):
                nxt, delta = graph.step(s, c)
                assert graph.table_step(table, s, c) == (nxt, delta), (phrases, s, c)
                explicit = pack(s, c) in set(stored.tolist())
                assert explicit == (nxt != 0 if s == 0 else nxt != 0 and nxt != graph.goto(0, c)), (phrases, s, c)
            for c in (-1, 65535, 1 << 20):
                assert graph.table_step(table, s, c) == (0, -int(graph.hold[s]))
        assert graph.table_step(table, graph.states, 1) == graph.step(0, 1) and graph.table_step(table, -1, 1) == graph.step(0, 1)
        y = rng.integers(1, V, size=30).tolist()
        assert graph.walk(y, lambda s, c: graph.table_step(table, s, c)) == graph.walk(y)


def test_a_large_list_builds_a_table_near_the_size_of_its_trie():
    """1000 phrases of 2 to 6 labels over 4364 labels (the measured shape): the builder proves its table without visiting every (state,
    label) pair, and the table holds fewer than two transitions per state."""
    rng = np.random.default_rng(3)
    graph = ContextGraph.from_phrases([rng.integers(3, 4364, size=int(rng.integers(2, 7))).tolist() for _ in range(1000)], 4364)
    keys, _, max_probe = graph.hash_table()
    assert graph.states > 3000 and np.count_nonzero(keys) < 2 * graph.states and max_probe <= 16
    assert graph.hash_table() is graph.hash_table()


# ------------------------------------------------------------------------------------------------ the file and the refusals
def test_file_and_refusals(tmp_path):
    label2id = {ch: i for i, ch in enumerate(["_", "<", ">"] + list("abc d"))}
    id2label = {i: ch for ch, i in label2id.items()}
    path = tmp_path / "phrases.txt"
    path.write_text("# names\nab c\n\n  \nDad\nab c\n", encoding="utf8")
    g = ContextGraph.from_file(str(path), label2id)
    ids = [[label2id[ch] for ch in "ab c"], [label2id[ch] for ch in "dad"]]
    assert g.phrases == sorted(tuple(p) for p in ids) and g.V == 8
    assert g.earned(ids[0]) == 4 and g.earned(ids[1] + ids[0]) == 7
    g.check_labels(id2label)
    g.check_labels([id2label[i] for i in range(8)])
    for other in ([id2label[i] for i in range(7)], [id2label[i] for i in range(7)] + ["x"]):
        with pytest.raises(ValueError, match="another label file"):
            g.check_labels(other)
    plain = ContextGraph.from_phrases(ids, 8)                       # no labels on record: the size alone is checked
    plain.check_labels([id2label[i] for i in range(7)] + ["x"])
    with pytest.raises(ValueError, match="another label file"):
        plain.check_labels(list("abc"))
    path.write_text("ab\n\nabz\n", encoding="utf8")
    with pytest.raises(ValueError, match=r"line 3.*'z'"):
        ContextGraph.from_file(str(path), label2id)
    path.write_text("# nothing\n\n", encoding="utf8")
    with pytest.raises(ValueError, match="no phrase"):
        ContextGraph.from_file(str(path), label2id)
    path.write_text("a<b\n", encoding="utf8")                       # SOS's character is a label, but no phrase may hold it
    with pytest.raises(ValueError, match="SOS"):
        ContextGraph.from_file(str(path), label2id)
    with pytest.raises(ValueError, match="empty"):
        ContextGraph.from_phrases([], 8)
    with pytest.raises(ValueError, match="at least one label"):
        ContextGraph.from_phrases([[3], []], 8)
    for bad in (0, 1, 2):
        with pytest.raises(ValueError, match="blank / PAD, SOS or EOS"):
            ContextGraph.from_phrases([[3, bad, 4]], 8)
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="outside"):
            ContextGraph.from_phrases([[3, bad]], 8)
    with pytest.raises(ValueError, match="65535"):
        ContextGraph.from_phrases([[3]], 65536)
    ContextGraph.from_phrases([[65534]], 65535)                     # the largest label that fits


# ------------------------------------------------------------------------------------------------ the ABI and the flags
def test_header_and_signatures_of_the_new_entry_points():
    """asr_ctx_step and asr_ctc_beam_search_ctx in include/asr_hip.h with the issue's argument lists, ctypes signatures of the same length
    and kinds; the new entry opens with the plain search's arguments and goes on with the LM entry's; the ABI version stays 4."""
    from asr_hip import lib as L
    src = open(L.HEADER).read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "asr_stream_t": ctypes.c_void_p}

    def names(entry):
        m = re.search(r"int %s\(([^;]*)\);" % entry, src)
        assert m, entry
        return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    for name, count in (("asr_ctx_step", 12), ("asr_ctc_beam_search_ctx", 34)):
        args = names(name)
        res, sig = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(sig) == count
        for a, s in zip(args, sig):
            assert s is (ctypes.c_void_p if "*" in a else kinds[a.split()[0]]), (name, a)
    assert [a.split()[-1].lstrip("*") for a in names("asr_ctx_step")] == [
        "keys", "vals", "capacity", "max_probe", "hold", "states", "state", "sym", "n", "next", "delta", "stream"]
    ctx, fused = names("asr_ctc_beam_search_ctx"), names("asr_ctc_beam_search_lm")
    last = [a.split()[-1].lstrip("*") for a in ctx]
    assert last[:15] == [a.split()[-1].lstrip("*") for a in fused[:15]]
    assert last[15:] == ["ng_keys", "ng_vals", "ng_capacity", "ng_max_probe", "ng_order", "bos", "eos", "alpha", "beta", "lm", "cx_keys",
                         "cx_vals", "cx_capacity", "cx_max_probe", "cx_hold", "cx_states", "gamma", "credit", "stream"]
    assert re.search(r"int asr_abi_version\(void\);\s*/\* 4 ", src)


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def test_flags_and_start_up_errors(cli):
    import test as test_mod
    import test_ctc_beam_host as H
    import torch
    a = cli([])
    assert a.context_path is None and a.context_score == 3.0
    a = cli(["--ctc-beam-search", "--context-path", "p.txt", "--context-score", "1.5"])
    assert (a.context_path, a.context_score) == ("p.txt", 1.5)
    head = H._model(cli, ["--ctc-weight", "0.3"])
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--context-path", "p.txt"]), head)
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--context-path", "p.txt", "--ngram-path", "x.pt", "--attention-rescoring-weight",
                                     "0.3", "--lm-rescoring"]), head)
    for extra in ([], ["--beam-search"], ["--ctc-greedy"]):
        with pytest.raises(ValueError, match="--context-path needs --ctc-beam-search"):
            test_mod.check_ctc_decoding(cli(["--context-path", "p.txt"] + extra), head)
    V = len(head.id2label)
    graph = ContextGraph.from_phrases([[3, 4]], V)
    with pytest.raises(ValueError, match="--context-path needs --ctc-beam-search"):
        head.evaluate(torch.zeros(1, 1, 161, 8), [8], torch.zeros(1, 2, dtype=torch.int64), context=graph)
    with pytest.raises(ValueError, match="another label file"):
        head.ctc_beam_search(torch.zeros(1, 2, 32), [2], 4, context=ContextGraph.from_phrases([[3, 4]], V + 1))


# ------------------------------------------------------------------------------------------------ the restatement and its conditions
@pytest.mark.parametrize("name", ["small_w3", "small_w4", "mid"])
def test_with_gamma_zero_the_restatement_is_the_one_it_extends(name):
    """gamma = 0: with an LM every output of ctc_beam_lm_reference.search's cached case, keys included, bit for bit; without one and with
    beta = 0 ctc_beam_reference.search's.  credit still reports what every hypothesis earned."""
    c = R.cases_cached()[name]
    graph = X.case_graph(name)
    lm = M.synthetic_lm(c["logits"].shape[2])
    got = X.search(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], graph, 0.0, lm, M.ALPHA, M.BETA, M.BOS, M.EOS)
    ref = M.expected(name)
    for k in ("ids", "lengths", "scores", "lm", "keys", "prune_margin", "lineage_margin", "top_margin"):
        assert np.array_equal(got[k], ref[k]), (name, k)
    plain = X.search(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], graph, 0.0)
    ref = R.expected(name)
    for k in ("ids", "lengths", "scores"):
        assert np.array_equal(plain[k], ref[k]), (name, k)
    for r in (got, plain):
        for b in range(len(c["lengths"])):
            for n in range(c["nbest"]):
                want = graph.earned(r["ids"][b, n, :r["lengths"][b, n]].tolist()) if r["lengths"][b, n] >= 0 else -1
                assert r["credit"][b, n] == want
    assert np.all(plain["lm"][plain["lengths"] >= 0] == 0.0) and np.all(np.isneginf(plain["lm"][plain["lengths"] < 0]))


def test_unpruned_keys_equal_brute_force():
    """The "exhaustive" case (T 3, V 3, W 16: nothing is pruned): every hypothesis' final key is the log of the summed probability of all
    its alignments + alpha * NgramLM.score + beta * len + gamma * earned, by a route that shares no code with the search."""
    c = R.cases_cached()["exhaustive"]
    graph = X.graph_of([[1, 2], [2], [2, 2, 1]], 3)
    for lm, alpha, eos in ((None, 0.0, -1), (M.synthetic_lm(3), M.ALPHA, M.EOS)):
        r = X.search(c["logits"], c["lengths"], 16, 3, 16, graph, X.GAMMA, lm, alpha, M.BETA, M.BOS, eos)
        for b in range(2):
            truth = R.enumerate_all(c["logits"][b].astype(np.float64), 3)
            n = int((r["lengths"][b] >= 0).sum())
            assert n == len(truth)
            want = {g: p + (alpha * lm.score(g, M.BOS, eos) if lm else 0.0) + M.BETA * len(g) + X.GAMMA * graph.earned(g)
                    for g, p in truth.items()}
            for k in range(n):
                g = tuple(r["ids"][b, k, :r["lengths"][b, k]].tolist())
                assert abs(r["keys"][b, k] - want[g]) <= 1e-6 * max(1.0, abs(want[g])), (b, g)
                assert r["credit"][b, k] == graph.earned(g) and abs(r["scores"][b, k] - truth[g]) <= 1e-10
            assert [tuple(r["ids"][b, k, :r["lengths"][b, k]]) for k in range(n)] == sorted(want, key=lambda g: -want[g])


@pytest.mark.parametrize("name,order", [("small_w3", 0), ("small_w3", 3), ("small_w4", 0), ("small_w4", 3), ("small_w4", 1),
                                        ("small_w4", 4), ("mid", 0), ("mid", 3), ("widest_slot_set", 0), ("widest_slot_set", 3)])
def test_conditions_of_the_gpu_cases(name, order):
    """Every case the GPU test runs, phrases only (order 0) and with an LM: lineage_margin and top_margin at least delta for every
    utterance, the small cases' prune_margin too (their whole n-best is compared); the list has something to say (some hypothesis
    earned a label).  Somewhere the phrases change the n-best, else the GPU tests would test nothing new."""
    r = X.expected(name, order)
    print(name, order, "prune", r["prune_margin"], "lineage", r["lineage_margin"], "top", r["top_margin"])
    assert np.all(r["lineage_margin"] >= R.DELTA) and np.all(r["top_margin"] >= R.DELTA)
    if R.cases_cached()[name]["small"]:
        assert np.all(r["prune_margin"] >= R.DELTA)
    assert r["credit"].max() >= 2
    if name != "small_w3":
        assert not np.array_equal(r["ids"], (M.expected(name, order) if order else R.expected(name))["ids"])


@pytest.mark.parametrize("V", [3, 5])
@pytest.mark.parametrize("W", [3, 5])
@pytest.mark.parametrize("order", [0, 3])
def test_conditions_of_the_sweep(V, W, order):
    """Of the 200 drawn utterances per (V, W) at least 180 pass the margin filter, phrases only and under the trigram; every group has 2
    to 4 phrases of 1 to 3 labels; no n-best holds a sequence twice; the final keys do not increase."""
    groups = X.sweep(V, W, order)
    kept = sum(len(tb) for _, _, tb, _ in groups)
    print("V %d W %d order %d: %d of %d utterances kept" % (V, W, order, kept, X.SWEEP_DRAWS))
    assert X.SWEEP_DRAWS == 200 and X.GAMMA == 1.5 and kept >= 180
    for graph, lg, tb, r in groups:
        assert 1 <= len(graph.phrases) <= 4 and all(1 <= len(p) <= 3 for p in graph.phrases) and min(tb) >= 4 and max(tb) <= 13
        for b in range(len(tb)):
            rows = [tuple(r["ids"][b, k, :r["lengths"][b, k]]) for k in range(W) if r["lengths"][b, k] >= 0]
            assert len(set(rows)) == len(rows) and np.all(np.diff(r["keys"][b, :len(rows)]) <= 0)


def test_conditions_of_the_relink_inputs():
    """Under each phrase list a prefix that was pruned comes back while it stands mid-phrase (hold > 0), and all margins hold."""
    for case in X.RELINK:
        _, r, graph, _, recreated = X.relink_search(case)
        assert min(r["prune_margin"][0], r["lineage_margin"][0], r["top_margin"][0]) >= R.DELTA
        assert any(graph.hold[graph.walk(g)[0]] > 0 for g in recreated), (case, recreated)


def _best(r):
    return r["ids"][0, 0, :r["lengths"][0, 0]].tolist()


def test_conditions_of_the_hand_made_inputs():
    """The phrase decides; the unfinished phrase earns nothing (and would have won with what it held); the phrase survives only through the
    bonus.  In each the best hypothesis is decided by at least delta."""
    lg = X.phrase_decides_case()
    assert np.allclose(lg[0, :, 1] - lg[0, :, 2], 0.1)
    plain = R.search(lg, [3], 4, 3, 4)
    biased = X.search(lg, [3], 4, 3, 4, X.graph_of([[2]], 4), 3.0)
    assert _best(plain) == [1] and _best(biased) == [2] and biased["credit"][0, 0] == 1
    for r in (plain, biased):
        assert min(r["lineage_margin"][0], r["top_margin"][0]) >= R.DELTA
    # unfinished: ranked with the held labels the best would be a prefix that stands mid-phrase; the final order takes them back
    lg, phrases = X.unfinished_case()
    graph = X.graph_of(phrases, 5)
    r = X.search(lg, [4], 4, 4, 4, graph, 3.0)
    assert min(r["prune_margin"][0], r["lineage_margin"][0], r["top_margin"][0]) >= R.DELTA
    rows = [r["ids"][0, k, :r["lengths"][0, k]].tolist() for k in range(4)]
    held = [r["scores"][0, k] + 3.0 * graph.walk(g)[1] for k, g in enumerate(rows)]
    k = int(np.argmax(held))
    assert k != 0 and graph.hold[graph.walk(rows[k])[0]] == 2 and r["credit"][0, k] == 0 and rows[k] == [1, 2]
    assert all(r["credit"][0, n] == graph.earned(rows[n]) for n in range(4))
    # deep pruning
    lg, phrases, W = X.deep_pruning_case()
    lp = lg[0, 1] - R.lse_rows(lg[0, 1])
    assert sorted(range(6), key=lambda v: -lp[v]).index(3) >= W                     # label 3 is outside the top W of its frame
    plain = R.search(lg, [6], W, 5, W)
    biased = X.search(lg, [6], W, 5, W, X.graph_of(phrases, 6), 4.0)
    assert all(3 not in plain["ids"][0, k, :plain["lengths"][0, k]] for k in range(W))      # no rescoring of these finds it
    assert _best(biased) == [3, 4] and biased["credit"][0, 0] == 2
    assert min(biased["prune_margin"][0], biased["lineage_margin"][0], biased["top_margin"][0]) >= R.DELTA
