"""asr_ctc_beam_search_ctx, the phrase arms of the CTC prefix beam search (csrc/ctc_beam.hip), against the float64 restatement
tests/ctc_beam_ctx_reference.py (pinned by tests/test_context_host.py, which also asserts the conditions the cases below rely on), then
the model and test.py levels on the tiny model of tests/test_gpu_joint_ctc.py.

The rule of tests/test_gpu_ctc_beam_lm.py: scores (the CTC log-probability) and alpha * lm + beta * len + gamma * credit within 2e-5 *
max(1, |ref|) of the restatement, -inf patterns identical, no NaN; sequences, lengths and credit torch.equal for the whole n-best of
every utterance whose prune_margin (on the fused key) is at least delta = 4e-5, elsewhere for the best hypothesis, whose lineage_margin
and top_margin are asserted to be at least delta; no sequence appears twice; every credit is ContextGraph.earned of its sequence."""
import copy
import math
import types

import numpy as np
import pytest
import torch

import ctc_beam_ctx_reference as X
import ctc_beam_lm_reference as M
import ctc_beam_reference as R

pytestmark = pytest.mark.gpu

TOL = 2e-5


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _run(logits, lengths, W, C, nbest, graph=None, gamma=X.GAMMA, lm=None, alpha=M.ALPHA, beta=M.BETA, eos=None, ld_pad=0):
    """ops.ctc_beam_search on the device; eos None: the tests' end term with an LM, none without."""
    from asr_hip import ops
    dev = torch.device("cuda")
    lg = torch.from_numpy(np.asarray(logits))
    if ld_pad:                                       # a row stride above V: the logits as a view of a wider buffer that holds 50.0
        wide = torch.full(lg.shape[:2] + (lg.shape[2] + ld_pad,), 50.0)
        wide[..., :lg.shape[2]] = lg
        g = wide.to(dev)[..., :lg.shape[2]]
    else:
        g = lg.to(dev)
    tb = torch.tensor(lengths, dtype=torch.int32, device=dev)
    kw = {}
    if lm is not None:
        kw.update(ngram=lm, alpha=alpha, bos=M.BOS, eos=M.EOS if eos is None else eos)
    if lm is not None or graph is not None:
        kw.update(beta=beta)
    if graph is not None:
        kw.update(context=graph, gamma=gamma)
    out = ops.ctc_beam_search(g, tb, W, C, nbest, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _compare(got, ref, graph, alpha, beta, gamma, what):
    """The comparison rules of the module docstring; -> the worst relative error of the two compared quantities."""
    ids, lens, cr = got["ids"], got["lengths"], got["credit"]
    sc, lm = got["scores"].double().numpy(), got["lm"].double().numpy()
    assert ids.dtype == lens.dtype == cr.dtype == torch.int32 and got["scores"].dtype == got["lm"].dtype == torch.float32
    assert tuple(ids.shape) == ref["ids"].shape and tuple(lens.shape) == ref["lengths"].shape == tuple(got["lm"].shape) == tuple(cr.shape)
    assert not np.isnan(sc).any() and not np.isnan(lm).any(), what
    whole = ref["prune_margin"] >= R.DELTA
    assert np.all(ref["lineage_margin"] >= R.DELTA) and np.all(ref["top_margin"] >= R.DELTA), what
    worst = 0.0
    for b in range(ids.shape[0]):
        none = lens[b].numpy() < 0
        assert np.array_equal(np.isneginf(sc[b]), none) and np.array_equal(np.isneginf(lm[b]), none), (what, b)
        assert np.array_equal(cr[b].numpy() == -1, none) and int(cr[b].min()) >= -1, (what, b)
        assert np.isfinite(sc[b][~none]).all() and np.isfinite(lm[b][~none]).all() and int(lens[b].max()) <= ids.shape[2], (what, b)
        found = [tuple(ids[b, k, :lens[b, k]].tolist()) for k in range(ids.shape[1]) if lens[b, k] >= 0]
        assert len(set(found)) == len(found), (what, b, "a sequence appears twice", found)
        assert [int(cr[b, k]) for k in range(len(found))] == [graph.earned(g) for g in found], (what, b)      # (found ones come first)
        n = ids.shape[1] if whole[b] else 1
        assert torch.equal(lens[b, :n], torch.from_numpy(ref["lengths"][b, :n])), (what, b, lens[b].tolist(), ref["lengths"][b].tolist())
        assert torch.equal(ids[b, :n], torch.from_numpy(ref["ids"][b, :n])), (what, b)
        assert torch.equal(cr[b, :n], torch.from_numpy(ref["credit"][b, :n])), (what, b)
        fin = ref["lengths"][b, :n] >= 0
        fused = alpha * lm[b, :n][fin] + beta * lens[b, :n].double().numpy()[fin] + gamma * cr[b, :n].double().numpy()[fin]
        for g, r in ((sc[b, :n][fin], ref["scores"][b, :n][fin]), (fused, ref["fused"][b, :n][fin])):
            err = np.abs(g - r) / np.maximum(1.0, np.abs(r))
            worst = max(worst, float(err.max()) if err.size else 0.0)
    print("%s: worst relative error %.3e; whole n-best compared for %d of %d utterances" % (what, worst, int(whole.sum()), len(whole)))
    assert worst <= TOL, (what, worst)
    return worst


def _case(name, order=0, **kw):
    """A cached case under its phrase list; order 0: phrases only, else with synthetic_lm(V, order) and the end term."""
    c = R.cases_cached()[name]
    graph = X.case_graph(name)
    lm = M.synthetic_lm(c["logits"].shape[2], order) if order else None
    got = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], graph, X.GAMMA, lm, **kw)
    _compare(got, X.expected(name, order), graph, M.ALPHA if order else 0.0, M.BETA, X.GAMMA, "%s order %d" % (name, order))
    return c, graph, lm, got


# ------------------------------------------------------------------------------------------------ off means off
@pytest.mark.parametrize("name", ["small_w3", "small_w4", "mid", "widest_slot_set"])
def test_gamma_zero_returns_the_bits_of_the_entries_without_phrases(name):
    """gamma = 0 with an LM: ids, lengths, scores and lm torch.equal to asr_ctc_beam_search_lm's; without an LM and with beta = 0: ids,
    lengths and scores torch.equal to asr_ctc_beam_search's, lm 0 (-inf where there is no hypothesis).  In both, credit is
    ContextGraph.earned of every returned sequence."""
    c = R.cases_cached()[name]
    graph = X.case_graph(name)
    lm = M.synthetic_lm(c["logits"].shape[2])
    a = (c["logits"], c["lengths"], c["W"], c["C"], c["nbest"])
    for ref, got, keys in ((_run(*a, lm=lm), _run(*a, graph, 0.0, lm), ("ids", "lengths", "scores", "lm")),
                           (_run(*a), _run(*a, graph, 0.0, beta=0.0), ("ids", "lengths", "scores"))):
        assert "credit" not in ref
        for k in keys:
            assert torch.equal(got[k], ref[k]), (name, k)
        for b in range(got["ids"].shape[0]):
            for n in range(c["nbest"]):
                want = graph.earned(got["ids"][b, n, :got["lengths"][b, n]].tolist()) if got["lengths"][b, n] >= 0 else -1
                assert int(got["credit"][b, n]) == want, (name, b, n)
    found = got["lengths"] >= 0
    assert torch.all(got["lm"][found] == 0.0) and torch.all(got["lm"][~found] == -math.inf)
    assert int(got["credit"].max()) >= 2                                  # (the list has something to say about these hypotheses)


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("order", [0, 3])
@pytest.mark.parametrize("name", ["small_w3", "small_w4"])
def test_small_ragged_batches(name, order):
    """B 6 with T_b = 0 and T_b = 1 among the lengths, the whole n-best of every utterance compared.  T_b = 0: the empty sequence alone,
    score 0, credit 0."""
    c, graph, lm, got = _case(name, order)
    assert np.all(X.expected(name, order)["prune_margin"] >= R.DELTA)
    b0 = c["lengths"].index(0)
    assert got["lengths"][b0].tolist() == [0] + [-1] * (c["nbest"] - 1) and float(got["scores"][b0, 0]) == 0.0
    assert got["credit"][b0].tolist() == [0] + [-1] * (c["nbest"] - 1) and torch.all(got["ids"][b0] == 0)
    assert float(got["lm"][b0, 0]) == (float(lm.logp((M.BOS,), M.EOS)) if order else 0.0)


@pytest.mark.parametrize("order", [1, 4])
def test_other_orders(order):
    _case("small_w4", order)


@pytest.mark.parametrize("order", [0, 3])
def test_mid_sized_case(order):
    _case("mid", order)


@pytest.mark.parametrize("order", [0, 3])
def test_widest_slot_set(order):
    """B 4, T 75, V 4364, W = C = 16: all 272 slots on the 320-thread launch."""
    _case("widest_slot_set", order)


def test_pruned_parent_created_again_gets_the_same_state_and_credit():
    """The two inputs on which a prefix is pruned and created again while its child stays in the list, under phrase lists that leave the
    re-created prefix mid-phrase (asserted on the host): state and credit depend on the labels alone, so the merge by label sequence
    still holds, no sequence appears twice and every credit is what its labels earn."""
    for case in X.RELINK:
        lg, W, phrases, gamma, order = case
        x, ref, graph, lm, _ = X.relink_search(case)
        assert ref["prune_margin"][0] >= R.DELTA
        _compare(_run(x, [len(lg)], W, 3, W, graph, gamma, lm), ref, graph, M.ALPHA if order else 0.0, M.BETA, gamma,
                 "re-created parent, W %d order %d" % (W, order))


@pytest.mark.parametrize("order", [0, 3])
@pytest.mark.parametrize("V", [3, 5])
def test_sweep_of_small_random_utterances(V, order):
    """At least 180 of 200 random-logit utterances per (V, W), T_b 4..13, C = V, W 3 and 5, in four groups under their own 2 to 4 random
    phrases of 1 to 3 labels, gamma 1.5, beta 0.3, phrases only and with the trigram: the whole n-best against the restatement."""
    for W in (3, 5):
        groups = X.sweep(V, W, order)
        assert sum(len(tb) for _, _, tb, _ in groups) >= 180
        lm = M.synthetic_lm(V, order) if order else None
        for i, (graph, lg, tb, ref) in enumerate(groups):
            _compare(_run(lg, tb, W, V, W, graph, X.GAMMA, lm), ref, graph, M.ALPHA if order else 0.0, M.BETA, X.GAMMA,
                     "sweep V %d W %d order %d group %d (%d utterances)" % (V, W, order, i, len(tb)))


def _best(r):
    return r["ids"][0, 0, :r["lengths"][0, 0]].tolist()


def test_the_phrase_decides_between_two_near_equal_labels():
    """Label 1 leads label 2 by 0.1 for three frames: the plain best is [1], with the phrase [2] and gamma 3 it is [2], and both equal
    their restatements."""
    lg = X.phrase_decides_case()
    plain = _run(lg, [3], 4, 3, 4)
    ref_plain = R.search(lg, [3], 4, 3, 4)
    assert torch.equal(plain["ids"][:, :1], torch.from_numpy(ref_plain["ids"][:, :1])) and _best(plain) == [1]
    graph = X.graph_of([[2]], 4)
    biased = _run(lg, [3], 4, 3, 4, graph, 3.0, beta=0.0)
    _compare(biased, X.search(lg, [3], 4, 3, 4, graph, 3.0), graph, 0.0, 0.0, 3.0, "the phrase decides")
    assert _best(biased) == [2] and int(biased["credit"][0, 0]) == 1


def test_the_unfinished_phrase_earns_nothing():
    """[1, 2] stands two labels into the phrase [1, 2, 3] when the utterance ends: ranked with what it holds it would be the best (asserted
    on the host); the final order takes the held labels back, equals the restatement's, and credit excludes them."""
    lg, phrases = X.unfinished_case()
    graph = X.graph_of(phrases, 5)
    got = _run(lg, [4], 4, 4, 4, graph, 3.0, beta=0.0)
    ref = X.search(lg, [4], 4, 4, 4, graph, 3.0)
    assert ref["prune_margin"][0] >= R.DELTA
    _compare(got, ref, graph, 0.0, 0.0, 3.0, "unfinished phrase")
    rows = [got["ids"][0, k, :got["lengths"][0, k]].tolist() for k in range(4)]
    k = rows.index([1, 2])
    assert k > 0 and int(got["credit"][0, k]) == 0 and graph.walk([1, 2])[1] == 2


def test_a_phrase_survives_only_through_the_bonus():
    """W 2: the phrase's first label ranks fourth in its frame by the CTC score alone (asserted on the host), so the plain search prunes
    it there and no rescoring of its 2-best brings it back; with the bonus in the pruning the best hypothesis is the phrase."""
    lg, phrases, W = X.deep_pruning_case()
    plain = _run(lg, [6], W, 5, W)
    assert all(3 not in plain["ids"][0, k, :plain["lengths"][0, k]].tolist() for k in range(W))
    graph = X.graph_of(phrases, 6)
    got = _run(lg, [6], W, 5, W, graph, 4.0, beta=0.0)
    _compare(got, X.search(lg, [6], W, 5, W, graph, 4.0), graph, 0.0, 0.0, 4.0, "deep pruning")
    assert _best(got) == [3, 4] and int(got["credit"][0, 0]) == 2


@pytest.mark.parametrize("name,order", [("small_w4", 0), ("mid", 3)])
def test_padded_frames_row_stride_and_two_calls_give_the_same_bits(name, order):
    """Frames >= T_b filled with NaN, the logits as a view of a wider buffer (row stride V + 5) that holds 50.0 beside them, and a second
    call: the first call's result, bit for bit, credit included."""
    c, graph, lm, first = _case(name, order)
    lg = c["logits"].copy()
    for b, n in enumerate(c["lengths"]):
        lg[b, n:] = np.nan
    a = (c["lengths"], c["W"], c["C"], c["nbest"], graph, X.GAMMA, lm)
    for got in (_run(lg, *a), _run(c["logits"], *a, ld_pad=5), _run(lg, *a, ld_pad=3), _run(c["logits"], *a)):
        for k in ("ids", "lengths", "scores", "lm", "credit"):
            assert torch.equal(got[k], first[k]), (name, k)


def test_refusals():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    graph = X.graph_of([[3, 4], [4, 5, 6]], 12)
    lm = M.synthetic_lm(12)
    one = torch.tensor([4], dtype=torch.int32, device=dev)
    lg = torch.zeros(1, 4, 12, device=dev)

    def fake(V, **over):                       # the real table under another V / capacity / probe length / state count
        t = dict(graph.device_table(dev), **over)
        return types.SimpleNamespace(V=V, device_table=lambda d: t)
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_beam_search(torch.zeros(1, 4, 65536, device=dev), one, 4, 4, 1, context=fake(65536), gamma=1.0)      # V above 65535
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_beam_search(lg, one, 4, 4, 5, context=graph, gamma=1.0)                                              # nbest > W
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_beam_search(lg, one, 17, 4, 1, context=graph, gamma=1.0)
    cap = graph.device_table(dev)["capacity"]
    for over in (dict(capacity=cap - 1), dict(capacity=0), dict(max_probe=0), dict(states=0), dict(keys=None), dict(vals=None),
                 dict(hold=None)):
        with pytest.raises(L.AsrHipError):
            ops.ctc_beam_search(lg, one, 4, 4, 1, context=fake(12, **over), gamma=1.0)
    for kw in (dict(bos=12), dict(eos=12), dict(eos=-2), dict(bos=-1)):          # with an LM its marks are checked as in the LM arm
        with pytest.raises(L.AsrHipError):
            ops.ctc_beam_search(lg, one, 4, 4, 1, context=graph, gamma=1.0, ngram=lm, **kw)
    with pytest.raises(ValueError, match="labels"):
        ops.ctc_beam_search(lg[:, :, :8], one, 4, 4, 1, context=graph, gamma=1.0)                                    # a list over other labels
    with pytest.raises(ValueError, match="labels"):
        ops.ctc_beam_search(lg, one, 4, 4, 1, context=graph, gamma=1.0, ngram=M.synthetic_lm(5))
    out = ops.ctc_beam_search(lg, one, 16, 0, 16, context=graph, gamma=1.0, ngram=lm, alpha=0.5, beta=0.1)
    assert tuple(out["credit"].shape) == (1, 16) and out["credit"].dtype == torch.int32 and tuple(out["lm"].shape) == (1, 16)


# ------------------------------------------------------------------------------------------------ model and test.py level
def _model_graph(model):
    """Phrases over the tiny model's labels 3..11, its own labels on record."""
    from utils.context import ContextGraph
    rng = np.random.default_rng(17)
    phrases = [rng.integers(3, 12, size=int(rng.integers(1, 4))).tolist() for _ in range(12)]
    return ContextGraph.from_phrases(phrases, 12, labels=[model.id2label[i] for i in range(12)])


def test_model_level_scores_follow_the_formulas(cli, monkeypatch):
    """Transformer.ctc_beam_search(context=...) on the tiny model, B 3, W 4, C 8, with and without an n-gram LM: every hypothesis it ranks
    has context_credit = ContextGraph.earned of its labels (an int), ctc_score, ngram_score (0 without an LM) and score = ctc_score +
    ngram_weight * ngram_score + length_bonus * len + context_score * context_credit; with rescoring_weight l also att_score and
    (1 - l) * ctc_score + l * att_score + the same three terms.  context=None makes only the two old launches; the table goes to the
    device once."""
    import test_gpu_ctc_beam as G
    import test_gpu_ctc_beam_lm as GL
    from asr_hip import lib as L
    model, J = G._head_model(cli)
    _, _, _, enc, logits, frames = G._encoded(model, J)
    graph, lm = _model_graph(model), GL._model_lm(model)
    W, C, a, beta, gamma, lam = 4, 8, 0.5, 0.3, 2.0, 0.4
    seen = GL._recorded(monkeypatch)
    for ngram in (None, lm):
        kw = dict(nbest=W, candidates=C, c_weight=0, ngram=ngram, ngram_weight=a, length_bonus=beta, context=graph, context_score=gamma)
        del seen[:]
        strs, ids = model.ctc_beam_search(enc, frames, W, return_ids=True, **kw)
        model.ctc_beam_search(enc, frames, W, rescoring_weight=lam, **kw)
        assert len(seen) == 2 and len(strs) == len(ids) == 3
        credited = 0
        for b in range(3):
            assert strs[b] == ["".join(model.id2label[x] for x in row) for row in ids[b]]
            for h in seen[0][b]:
                assert type(h["context_credit"]) is int and h["context_credit"] == graph.earned(h["yseq"])
                credited += h["context_credit"]
                if ngram is None:
                    assert h["ngram_score"] == 0.0
                assert h["score"] == h["ctc_score"] + a * h["ngram_score"] + beta * len(h["yseq"]) + gamma * h["context_credit"]
            assert [h["yseq"] for h in seen[1][b]] == [h["yseq"] for h in seen[0][b]]
            for h, h0 in zip(seen[1][b], seen[0][b]):
                assert h["ctc_score"] == h0["ctc_score"] and h["ngram_score"] == h0["ngram_score"] and math.isfinite(h["att_score"])
                assert h["context_credit"] == h0["context_credit"]
                want = ((1 - lam) * h["ctc_score"] + lam * h["att_score"] + a * h["ngram_score"] + beta * len(h["yseq"])
                        + gamma * h["context_credit"])
                assert abs(h["score"] - want) <= 1e-9 * max(1.0, abs(want))
        assert credited > 0
    # the kernel's hypotheses are the restatement's on the model's own logits, where the margins decide them
    from utils import constant
    ref = X.search(logits, frames, W, C, W, graph, gamma, lm, a, beta, constant.SOS_TOKEN, constant.EOS_TOKEN)
    for b in range(3):
        if min(ref["lineage_margin"][b], ref["top_margin"][b]) >= R.DELTA:
            assert seen[0][b][0]["yseq"] == ref["ids"][b, 0, :ref["lengths"][b, 0]].tolist()
            assert seen[0][b][0]["context_credit"] == ref["credit"][b, 0]
    # None: the two old paths, through the two old entries
    calls, orig = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *x: (calls.append(name), orig(name, *x))[1])
    model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, context=None, context_score=5.0)
    model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, ngram=lm, ngram_weight=a, context=None, context_score=5.0)
    assert "asr_ctc_beam_search" in calls and "asr_ctc_beam_search_lm" in calls and "asr_ctc_beam_search_ctx" not in calls
    assert "context_credit" not in seen[-1][0][0]
    model.ctc_beam_search(enc, frames, W, context=graph, context_score=gamma)
    assert "asr_ctc_beam_search_ctx" in calls
    assert len(graph._tables) == 1                                              # the table went to the device once


def test_evaluate_and_test_py_route_the_context(cli, tmp_path):
    """evaluate(ctc_beam=True, context=...) returns the best of ctc_beam_search with the same arguments; test.py's evaluate() hands
    --context-score on with the list read from --context-path's file, beside the n-gram's arguments; --context-path alone is refused."""
    import test as test_mod
    import test_gpu_ctc_beam as G
    import test_gpu_ctc_beam_lm as GL
    import test_gpu_joint_ctc as J
    from utils.context import ContextGraph
    model, _ = G._head_model(cli)
    src, lengths, tgt, enc, _, frames = G._encoded(model, J)
    graph, lm = _model_graph(model), GL._model_lm(model)
    best = model.ctc_beam_search(enc, frames, 4, nbest=1, c_weight=0.1, context=graph, context_score=2.0)
    hyps = model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, beam_nbest=3, c_weight=0.1, context=graph, context_score=2.0)[1]
    assert hyps == [rows[0] for rows in best]
    with pytest.raises(ValueError, match="--context-path needs --ctc-beam-search"):
        model.evaluate(src, lengths, tgt, context=graph)
    path = tmp_path / "phrases.txt"
    path.write_text("# two phrases\n%s\n\n%s\n" % ("".join(model.id2label[i] for i in (4, 5, 6)), model.id2label[9]), encoding="utf8")
    label2id = {model.id2label[i]: i for i in range(12)}
    flags = J.TINY + ["--precision", "fp32", "--ctc-weight", "0.3", "--beam-width", "4", "--beam-nbest", "2", "--context-path", str(path),
                      "--context-score", "2.5"]
    with pytest.raises(ValueError, match="--context-path needs --ctc-beam-search"):
        test_mod.check_ctc_decoding(cli(flags), model)
    args = cli(flags + ["--ctc-beam-search"])
    test_mod.check_ctc_decoding(args, model)
    loaded = ContextGraph.from_file(args.context_path, label2id)
    assert loaded.phrases == [(4, 5, 6), (9,)]
    loaded.check_labels(model.id2label)
    seen, orig = [], model.ctc_beam_search

    def recording(*a, **k):
        seen.append(k)
        return orig(*a, **k)
    model.ctc_beam_search = recording
    try:
        cer, wer = test_mod.evaluate(model, G._loader(), context=loaded)
        test_mod.evaluate(model, G._loader(), ngram=lm, context=loaded)
        test_mod.evaluate(model, G._loader())
    finally:
        del model.ctc_beam_search
    assert np.isfinite(cer) and np.isfinite(wer) and len(seen) == 3
    assert seen[0]["context"] is loaded and seen[0]["context_score"] == 2.5 and seen[0].get("ngram") is None
    assert seen[1]["context"] is loaded and seen[1]["ngram"] is lm and seen[1]["context_score"] == 2.5
    assert seen[2].get("context") is None and seen[2].get("ngram") is None
