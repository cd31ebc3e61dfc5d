"""asr_ctc_beam_search_lm, the fused arm of the CTC prefix beam search (csrc/ctc_beam.hip), against the float64 restatement
tests/ctc_beam_lm_reference.py (pinned by tests/test_ctc_beam_lm_host.py, which also asserts the conditions the cases below rely on),
then the model and test.py levels on the tiny model of tests/test_gpu_joint_ctc.py.

The rule of tests/test_gpu_ctc_beam.py: scores (the CTC log-probability) and alpha * lm + beta * len within 2e-5 * max(1, |ref|) of the
restatement, -inf patterns identical, no NaN; sequences and lengths torch.equal for the whole n-best of every utterance whose
prune_margin (on the fused key) is at least delta = 4e-5, elsewhere for the best hypothesis, whose lineage_margin and top_margin are
asserted to be at least delta; no sequence appears twice."""
import copy
import math
import types

import numpy as np
import pytest
import torch

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


def _run(logits, lengths, W, C, nbest, lm=None, alpha=M.ALPHA, beta=M.BETA, eos=M.EOS, ld_pad=0, bos=M.BOS):
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
    if lm is None:
        out = ops.ctc_beam_search(g, tb, W, C, nbest)
    else:
        out = ops.ctc_beam_search(g, tb, W, C, nbest, ngram=lm, alpha=alpha, beta=beta, bos=bos, eos=eos)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _compare(got, ref, alpha, beta, what):
    """The comparison rules of the module docstring; -> the worst relative error of the two compared quantities."""
    ids, lens, sc, lm = got["ids"], got["lengths"], got["scores"].double().numpy(), got["lm"].double().numpy()
    assert ids.dtype == torch.int32 and lens.dtype == torch.int32 and got["scores"].dtype == got["lm"].dtype == torch.float32
    assert tuple(ids.shape) == ref["ids"].shape and tuple(lens.shape) == ref["lengths"].shape == tuple(got["lm"].shape), what
    assert not np.isnan(sc).any() and not np.isnan(lm).any(), what
    whole = ref["prune_margin"] >= R.DELTA
    assert np.all(ref["lineage_margin"] >= R.DELTA) and np.all(ref["top_margin"] >= R.DELTA), what
    worst = 0.0
    for b in range(ids.shape[0]):
        none = lens[b].numpy() < 0
        assert np.array_equal(np.isneginf(sc[b]), none) and np.array_equal(np.isneginf(lm[b]), none), (what, b)
        assert np.isfinite(sc[b][~none]).all() and np.isfinite(lm[b][~none]).all() and int(lens[b].max()) <= ids.shape[2], (what, b)
        found = [tuple(ids[b, k, :lens[b, k]].tolist()) for k in range(ids.shape[1]) if lens[b, k] >= 0]
        assert len(set(found)) == len(found), (what, b, "a sequence appears twice", found)
        n = ids.shape[1] if whole[b] else 1
        assert torch.equal(lens[b, :n], torch.from_numpy(ref["lengths"][b, :n])), (what, b, lens[b].tolist(), ref["lengths"][b].tolist())
        assert torch.equal(ids[b, :n], torch.from_numpy(ref["ids"][b, :n])), (what, b)
        fin = ref["lengths"][b, :n] >= 0
        fused = alpha * lm[b, :n][fin] + beta * lens[b, :n].double().numpy()[fin]
        for g, r in ((sc[b, :n][fin], ref["scores"][b, :n][fin]), (fused, ref["fused"][b, :n][fin])):
            err = np.abs(g - r) / np.maximum(1.0, np.abs(r))
            worst = max(worst, float(err.max()) if err.size else 0.0)
    print("%s: worst relative error %.3e; whole n-best compared for %d of %d utterances" % (what, worst, int(whole.sum()), len(whole)))
    assert worst <= TOL, (what, worst)
    return worst


def _case(name, order=3, eos=M.EOS, **kw):
    c = R.cases_cached()[name]
    lm = M.synthetic_lm(c["logits"].shape[2], order)
    got = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], lm, eos=eos, **kw)
    _compare(got, M.expected(name, order, eos), M.ALPHA, M.BETA, "%s order %d eos %d" % (name, order, eos))
    return c, lm, got


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", ["small_w3", "small_w4", "mid"])
def test_switched_off_it_returns_the_plain_search_bit_for_bit(name):
    """alpha = beta = 0: ids, lengths and scores are torch.equal to asr_ctc_beam_search's, with and without the end term; lm still holds
    the LM's log-probability of every hypothesis (NgramLM.score of its labels)."""
    c = R.cases_cached()[name]
    lm = M.synthetic_lm(c["logits"].shape[2])
    plain = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"])
    assert "lm" not in plain
    for eos in (M.EOS, -1):
        got = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], lm, 0.0, 0.0, eos)
        for k in ("ids", "lengths", "scores"):
            assert torch.equal(got[k], plain[k]), (name, eos, k)
        for b in range(got["ids"].shape[0]):
            for n in range(c["nbest"]):
                if got["lengths"][b, n] < 0:
                    assert got["lm"][b, n] == -math.inf
                else:
                    want = lm.score(got["ids"][b, n, :got["lengths"][b, n]].tolist(), M.BOS, eos)
                    assert abs(float(got["lm"][b, n]) - want) <= TOL * max(1.0, abs(want)), (name, eos, b, n)


@pytest.mark.parametrize("name,eos", [("small_w3", M.EOS), ("small_w4", M.EOS), ("small_w3", -1)])
def test_small_ragged_batches(name, eos):
    """B 6 with T_b = 0 and T_b = 1 among the lengths, the whole n-best of every utterance compared.  T_b = 0: the empty sequence alone,
    score 0, lm = q([bos], eos) (0 without an end term)."""
    c, lm, got = _case(name, eos=eos)
    assert np.all(M.expected(name, 3, eos)["prune_margin"] >= R.DELTA)
    b0 = c["lengths"].index(0)
    assert got["lengths"][b0].tolist() == [0] + [-1] * (c["nbest"] - 1) and float(got["scores"][b0, 0]) == 0.0
    assert float(got["lm"][b0, 0]) == (float(lm.logp((M.BOS,), eos)) if eos >= 0 else 0.0) and torch.all(got["ids"][b0] == 0)


@pytest.mark.parametrize("order", [1, 2, 4])
def test_other_orders(order):
    _case("small_w4", order)


def test_mid_sized_case():
    _case("mid")


def test_widest_slot_set():
    """B 4, T 75, V 4364, W = C = 16: all 272 slots on the 320-thread launch, a trigram table over the benchmark vocabulary."""
    _case("widest_slot_set")


def test_pruned_parent_created_again_gets_the_same_lm_state():
    """The two inputs on which a prefix is pruned and created again while its child stays in the list: lm, len and the context depend on
    the labels alone, so the merge by label sequence still holds and no sequence appears twice."""
    lm = M.synthetic_lm(3)
    for lg, W in ((R.RELINK_A, 4), (R.RELINK_B, 3)):
        x = np.array([lg], dtype=np.float32)
        ref = M.search(x, [len(lg)], W, 3, W, lm, M.ALPHA, M.BETA, M.BOS, M.EOS)
        assert ref["prune_margin"][0] >= R.DELTA
        _compare(_run(x, [len(lg)], W, 3, W, lm), ref, M.ALPHA, M.BETA, "re-created parent, W %d" % W)


@pytest.mark.parametrize("V", [3, 5])
def test_sweep_of_small_random_utterances(V):
    """At least 180 of 200 random-logit utterances per (V, W), T_b 4..13, C = V, W 3 and 5, trigram LM, alpha 0.5, beta 0.3: the whole
    n-best against the restatement."""
    for W in (3, 5):
        lg, tb, ref = M.sweep(V, W)
        assert len(tb) >= 180
        _compare(_run(lg, tb, W, V, W, M.synthetic_lm(V)), ref, M.ALPHA, M.BETA, "sweep V %d W %d (%d utterances)" % (V, W, len(tb)))


def test_the_lm_decides_between_two_near_equal_labels():
    """Label 1 leads label 2 by 0.1 in the logits, the LM has seen 2 open ten times as many sentences: the plain best is [1], the fused
    best [2], and both equal their restatements."""
    lg, lm = M.lm_decides_case()
    plain = _run(lg, [3], 4, 3, 4)
    ref_plain = R.search(lg, [3], 4, 3, 4)
    assert torch.equal(plain["ids"], torch.from_numpy(ref_plain["ids"])) and plain["ids"][0, 0, :plain["lengths"][0, 0]].tolist() == [1]
    fused = _run(lg, [3], 4, 3, 4, lm, M.ALPHA, 0.0)
    _compare(fused, M.search(lg, [3], 4, 3, 4, lm, M.ALPHA, 0.0, M.BOS, M.EOS), M.ALPHA, 0.0, "the LM decides")
    assert fused["ids"][0, 0, :fused["lengths"][0, 0]].tolist() == [2]


def test_the_length_bonus_turns_an_empty_best_into_a_label():
    lg, lm = M.beta_decides_case(), M.synthetic_lm(3)
    for beta, want in ((0.0, []), (2.0, [1])):
        got = _run(lg, [2], 4, 3, 4, lm, 0.0, beta, -1)
        _compare(got, M.search(lg, [2], 4, 3, 4, lm, 0.0, beta, M.BOS, -1), 0.0, beta, "length bonus %g" % beta)
        assert got["ids"][0, 0, :got["lengths"][0, 0]].tolist() == want


@pytest.mark.parametrize("name", ["small_w4", "mid"])
def test_padded_frames_row_stride_and_two_calls_give_the_same_bits(name):
    """Frames >= T_b filled with NaN, the logits as a view of a wider buffer (row stride V + 5) that holds 50.0 beside them, and a second
    call: the first call's result, bit for bit."""
    c, lm, first = _case(name)
    lg = c["logits"].copy()
    for b, n in enumerate(c["lengths"]):
        lg[b, n:] = np.nan
    a = (c["lengths"], c["W"], c["C"], c["nbest"], lm)
    for got in (_run(lg, *a), _run(c["logits"], *a, ld_pad=5), _run(lg, *a, ld_pad=3), _run(c["logits"], *a)):
        for k in ("ids", "lengths", "scores", "lm"):
            assert torch.equal(got[k], first[k]), (name, k)


def test_refusals():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    lm = M.synthetic_lm(12)
    one = torch.tensor([4], dtype=torch.int32, device=dev)
    lg = torch.zeros(1, 4, 12, device=dev)

    def fake(V, **over):                       # the real table under another V / order / capacity
        t = dict(lm.device_table(dev), **over)
        return types.SimpleNamespace(V=V, device_table=lambda d: t)
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_beam_search(torch.zeros(1, 4, 65536, device=dev), one, 4, 4, 1, ngram=fake(65536))       # V above 65535
    ops.ctc_beam_search(torch.zeros(1, 4, 65536, device=dev), one, 4, 4, 1)                                # (the plain arm takes it)
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_beam_search(lg, one, 4, 4, 5, ngram=lm)                                                    # nbest > W
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_beam_search(lg, one, 17, 4, 1, ngram=lm)
    for over in (dict(order=5), dict(order=0), dict(capacity=lm.device_table(dev)["capacity"] - 1), dict(max_probe=0)):
        with pytest.raises(L.AsrHipError):
            ops.ctc_beam_search(lg, one, 4, 4, 1, ngram=fake(12, **over))
    for kw in (dict(bos=12), dict(eos=12), dict(eos=-2), dict(bos=-1)):
        with pytest.raises(L.AsrHipError):
            ops.ctc_beam_search(lg, one, 4, 4, 1, ngram=lm, **kw)
    with pytest.raises(ValueError, match="labels"):
        ops.ctc_beam_search(lg[:, :, :8], one, 4, 4, 1, ngram=lm)                                          # an LM over other labels
    out = ops.ctc_beam_search(lg, one, 16, 0, 16, ngram=lm, alpha=0.5, beta=0.1)
    assert tuple(out["lm"].shape) == (1, 16) and tuple(out["ids"].shape) == (1, 16, 4)


# ------------------------------------------------------------------------------------------------ model and test.py level
def _model_lm(model, order=3):
    """A Witten-Bell LM over the tiny model's 12 labels (corpus over the ids 3..11, SOS / EOS as the sentence marks)."""
    from utils import constant
    from utils.ngram import NgramLM
    corpus = [[x + 2 for x in s] for s in M.synthetic_corpus(10, 21, 200)]
    return NgramLM.estimate(corpus, 12, order, constant.SOS_TOKEN, constant.EOS_TOKEN, labels=[model.id2label[i] for i in range(12)])


def _recorded(monkeypatch):
    """Records the hypotheses Transformer.ctc_beam_search hands to rank_ended (copies: the ranking may add to them)."""
    from asr_hip import search
    seen, orig = [], search.rank_ended

    def recording(ended, *a, **k):
        seen.append(copy.deepcopy(ended))
        return orig(ended, *a, **k)
    monkeypatch.setattr(search, "rank_ended", recording)
    return seen


def test_model_level_search_equals_the_reference_and_scores_follow_the_formulas(cli, monkeypatch):
    """Transformer.ctc_beam_search(ngram=...) on the tiny model, B 3, W 4, C 8: the hypotheses it ranks are the restatement's on the
    model's own ctc_logits (bos = SOS, eos = EOS) under the margin rule, each with ctc_score, ngram_score and score = ctc_score +
    ngram_weight * ngram_score + length_bonus * len; with rescoring_weight l also att_score and (1 - l) * ctc_score + l * att_score + the
    same two terms; ngram=None returns what it returned before, by the plain entry."""
    import test_gpu_ctc_beam as G
    from utils import constant
    model, J = G._head_model(cli)
    _, _, _, enc, logits, frames = G._encoded(model, J)
    lm = _model_lm(model)
    W, C, a, beta, lam = 4, 8, 0.5, 0.3, 0.4
    ref = M.search(logits, frames, W, C, W, lm, a, beta, constant.SOS_TOKEN, constant.EOS_TOKEN)
    print("margins: prune %s lineage %s top %s" % (ref["prune_margin"], ref["lineage_margin"], ref["top_margin"]))
    seen = _recorded(monkeypatch)
    strs, ids = model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, c_weight=0, return_ids=True, ngram=lm, ngram_weight=a,
                                      length_bonus=beta)
    model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, c_weight=0, ngram=lm, ngram_weight=a, length_bonus=beta,
                          rescoring_weight=lam)
    assert len(seen) == 2 and len(strs) == len(ids) == 3
    for b in range(3):
        assert ref["lineage_margin"][b] >= R.DELTA and ref["top_margin"][b] >= R.DELTA
        n = int((ref["lengths"][b] >= 0).sum()) if ref["prune_margin"][b] >= R.DELTA else 1
        want = [ref["ids"][b, k, :ref["lengths"][b, k]].tolist() for k in range(n)]
        assert [h["yseq"] for h in seen[0][b]][:n] == want and ids[b][0] == want[0], (b, ids[b], want)
        assert strs[b] == ["".join(model.id2label[x] for x in row) for row in ids[b]]
        for k, h in enumerate(seen[0][b]):
            assert h["score"] == h["ctc_score"] + a * h["ngram_score"] + beta * len(h["yseq"])
            assert abs(h["ngram_score"] - lm.score(h["yseq"], constant.SOS_TOKEN, constant.EOS_TOKEN)) <= TOL * max(1.0, abs(h["ngram_score"]))
            if k < n:
                assert abs(h["ctc_score"] - ref["scores"][b, k]) <= TOL * max(1.0, abs(ref["scores"][b, k]))
        assert [h["yseq"] for h in seen[1][b]] == [h["yseq"] for h in seen[0][b]]
        for h, h0 in zip(seen[1][b], seen[0][b]):
            assert h["ctc_score"] == h0["ctc_score"] and h["ngram_score"] == h0["ngram_score"] and math.isfinite(h["att_score"])
            want_score = (1 - lam) * h["ctc_score"] + lam * h["att_score"] + a * h["ngram_score"] + beta * len(h["yseq"])
            assert abs(h["score"] - want_score) <= 1e-9 * max(1.0, abs(want_score))
    # None: the plain search, through the plain entry
    from asr_hip import lib as L
    calls, orig = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *x: (calls.append(name), orig(name, *x))[1])
    plain = model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, c_weight=0.1, return_ids=True)
    assert model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, c_weight=0.1, return_ids=True, ngram=None, ngram_weight=0.7,
                                 length_bonus=1.0) == plain
    assert "asr_ctc_beam_search" in calls and "asr_ctc_beam_search_lm" not in calls and "ctc_score" not in seen[-1][0][0]
    model.ctc_beam_search(enc, frames, W, ngram=lm, ngram_weight=a)
    assert "asr_ctc_beam_search_lm" in calls
    assert len(lm._tables) == 1                                                 # the table went to the device once


def test_evaluate_and_test_py_route_the_ngram(cli, tmp_path, monkeypatch):
    """evaluate(ctc_beam=True, ngram=...) returns the best of ctc_beam_search with the same three arguments; test.py's evaluate() hands
    --ngram-weight and --ngram-length-bonus on with the LM loaded from --ngram-path's file; --ngram-path alone is refused."""
    import test as test_mod
    import test_gpu_ctc_beam as G
    import test_gpu_joint_ctc as J
    from utils.ngram import NgramLM
    model, _ = G._head_model(cli)
    src, lengths, tgt, enc, _, frames = G._encoded(model, J)
    lm = _model_lm(model)
    best = model.ctc_beam_search(enc, frames, 4, nbest=1, c_weight=0.1, ngram=lm, ngram_weight=0.6, length_bonus=0.2)
    hyps = model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, beam_nbest=3, c_weight=0.1, ngram=lm, ngram_weight=0.6,
                          length_bonus=0.2)[1]
    assert hyps == [rows[0] for rows in best]
    with pytest.raises(ValueError, match="--ngram-path needs --ctc-beam-search"):
        model.evaluate(src, lengths, tgt, ngram=lm)
    path = str(tmp_path / "ngram.pt")
    lm.save(path)
    flags = J.TINY + ["--precision", "fp32", "--ctc-weight", "0.3", "--beam-width", "4", "--beam-nbest", "2", "--ngram-path", path,
                      "--ngram-weight", "0.6", "--ngram-length-bonus", "0.2"]
    with pytest.raises(ValueError, match="--ngram-path needs --ctc-beam-search"):
        test_mod.check_ctc_decoding(cli(flags), model)
    args = cli(flags + ["--ctc-beam-search"])
    test_mod.check_ctc_decoding(args, model)
    loaded = NgramLM.load(args.ngram_path, model.id2label)
    seen, orig = [], model.ctc_beam_search

    def recording(*a, **k):
        seen.append(k)
        return orig(*a, **k)
    model.ctc_beam_search = recording
    try:
        cer, wer = test_mod.evaluate(model, G._loader(), ngram=loaded)
        test_mod.evaluate(model, G._loader())
    finally:
        del model.ctc_beam_search
    assert np.isfinite(cer) and np.isfinite(wer) and len(seen) == 2
    assert seen[0]["ngram"] is loaded and seen[0]["ngram_weight"] == 0.6 and seen[0]["length_bonus"] == 0.2
    assert seen[1]["ngram"] is None
