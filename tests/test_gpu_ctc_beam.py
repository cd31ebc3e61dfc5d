"""asr_ctc_beam_search (csrc/ctc_beam.hip) against the float64 restatement tests/ctc_beam_reference.py (pinned by
tests/test_ctc_beam_host.py, which also asserts the conditions the cases below rely on), then the model and test.py levels on the tiny
model of tests/test_gpu_joint_ctc.py.

Scores: within 2e-5 * max(1, |ref|), -inf patterns identical, no NaN -- the project's bound for its CTC kernels (tests/test_gpu_ctc_prefix.py,
tests/test_gpu_ctc_align.py).  Sequences and lengths: torch.equal -- the whole n-best of every utterance whose prune_margin is at least
delta = 4e-5 (a gap below two score errors cannot be decided: there a rounding error may legitimately change which prefixes the beam
holds), the best hypothesis of EVERY utterance (its lineage_margin and top_margin are at least delta on every case)."""
import json
import math
import os

import numpy as np
import pytest
import torch

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


def _run(logits, lengths, W, C, nbest, ld_pad=0, blank=0):
    from asr_hip import ops
    dev = torch.device("cuda")
    lg = torch.from_numpy(np.asarray(logits))
    if ld_pad:                                       # a row stride above V: the logits as a view of a wider buffer that holds 50.0
        wide = torch.full(lg.shape[:2] + (lg.shape[2] + ld_pad,), 50.0)
        wide[..., :lg.shape[2]] = lg
        g = wide.to(dev)[..., :lg.shape[2]]
    else:
        g = lg.to(dev)
    out = ops.ctc_beam_search(g, torch.tensor(lengths, dtype=torch.int32, device=dev), W, C, nbest, blank)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _compare(got, ref, what):
    """The comparison rules of the module docstring; -> the worst relative score error."""
    ids, lens, sc = got["ids"], got["lengths"], got["scores"].double().numpy()
    assert ids.dtype == torch.int32 and lens.dtype == torch.int32 and got["scores"].dtype == torch.float32
    assert tuple(ids.shape) == ref["ids"].shape and tuple(lens.shape) == ref["lengths"].shape, what
    assert not np.isnan(sc).any(), what
    whole = ref["prune_margin"] >= R.DELTA
    assert np.all(ref["lineage_margin"] >= R.DELTA) and np.all(ref["top_margin"] >= R.DELTA), what
    worst = 0.0
    for b in range(ids.shape[0]):
        # every row of every utterance: -inf exactly where there is no hypothesis, a length within the frames, scores non-increasing
        assert np.array_equal(np.isneginf(sc[b]), lens[b].numpy() < 0) and np.isfinite(sc[b][lens[b].numpy() >= 0]).all(), (what, b)
        assert int(lens[b].max()) <= ids.shape[2] and np.all(sc[b][:-1] >= sc[b][1:]), (what, b, sc[b].tolist())
        found = [tuple(ids[b, k, :lens[b, k]].tolist()) for k in range(ids.shape[1]) if lens[b, k] >= 0]
        assert len(set(found)) == len(found), (what, b, "a sequence appears twice", found)
        n = ids.shape[1] if whole[b] else 1
        assert torch.equal(lens[b, :n], torch.from_numpy(ref["lengths"][b, :n])), (what, b, lens[b].tolist(), ref["lengths"][b].tolist())
        assert torch.equal(ids[b, :n], torch.from_numpy(ref["ids"][b, :n])), (what, b)
        r, g = ref["scores"][b, :n], sc[b, :n]
        assert np.array_equal(np.isneginf(g), np.isneginf(r)) and np.array_equal(np.isneginf(g), ref["lengths"][b, :n] < 0), (what, b)
        fin = ~np.isneginf(r)
        assert np.isfinite(g[fin]).all(), (what, b)
        err = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        worst = max(worst, float(err.max()) if err.size else 0.0)
    print("%s: worst relative score error %.3e; whole n-best compared for %d of %d utterances" % (what, worst, int(whole.sum()), len(whole)))
    assert worst <= TOL, (what, worst)
    return worst


def _check(name, **kw):
    c = R.cases_cached()[name]
    got = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], **kw)
    _compare(got, R.expected(name), name)
    return c, got


# ------------------------------------------------------------------------------------------------ the kernel
def test_exhaustive_beam_returns_exact_ctc_likelihoods():
    """B 2, T 3, V 3, W 16, C 3: at most 15 sequences have an alignment, nothing is pruned, and every score is the log of the summed
    probability of all alignments of its sequence (brute force over the 27 alignments); entries beyond them are -1 / -inf."""
    c, got = _check("exhaustive")
    for b in range(2):
        truth = R.enumerate_all(c["logits"][b].astype(np.float64), 3)
        n = len(truth)
        assert got["lengths"][b, :n].min() >= 0 and torch.all(got["lengths"][b, n:] == -1) and torch.all(got["scores"][b, n:] == -math.inf)
        for k in range(n):
            g = tuple(got["ids"][b, k, :got["lengths"][b, k]].tolist())
            assert abs(float(got["scores"][b, k]) - truth[g]) <= TOL * max(1.0, abs(truth[g])), (b, g)


@pytest.mark.parametrize("name", ["small_w3", "small_w4"])
def test_small_ragged_batches(name):
    """B 6 with T_b = 0 (the empty prefix, score 0) and T_b = 1 among the lengths; the whole n-best of every utterance is compared."""
    c, got = _check(name)
    assert np.all(R.expected(name)["prune_margin"] >= R.DELTA)
    b0 = c["lengths"].index(0)
    assert got["lengths"][b0].tolist() == [0] + [-1] * (c["nbest"] - 1) and float(got["scores"][b0, 0]) == 0.0
    assert torch.all(got["ids"][b0] == 0)


@pytest.mark.parametrize("name", ["small_w3", "small_w4"])
def test_padded_frames_are_never_read_and_row_stride(name):
    """Frames >= T_b filled with NaN, and the logits as a view of a wider buffer (row stride V + 5) that holds 50.0 beside them: the
    result is the plain run's, bit for bit."""
    c, plain = _check(name)
    lg = c["logits"].copy()
    for b, n in enumerate(c["lengths"]):
        lg[b, n:] = np.nan
    for got in (_run(lg, c["lengths"], c["W"], c["C"], c["nbest"]), _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], ld_pad=5),
                _run(lg, c["lengths"], c["W"], c["C"], c["nbest"], ld_pad=3)):
        for k in ("ids", "lengths", "scores"):
            assert torch.equal(got[k], plain[k]), (name, k)


def test_width_one_and_one_candidate_and_nbest_below_width():
    """W = 1 and C = 1 (a beam of one prefix, one label tried per frame) on the small case against the restatement with those limits;
    nbest < W returns the first rows of the full n-best."""
    c = R.cases_cached()["small_w4"]
    for W, C in ((1, 1), (1, 4), (4, 1)):
        ref = R.search(c["logits"], c["lengths"], W, C, W)
        _compare(_run(c["logits"], c["lengths"], W, C, W), ref, "small_w4 W %d C %d" % (W, C))
    full = _run(c["logits"], c["lengths"], 4, 4, 4)
    for nbest in (1, 2):
        part = _run(c["logits"], c["lengths"], 4, 4, nbest)
        assert tuple(part["ids"].shape) == (6, nbest, 24)
        for k in ("ids", "lengths", "scores"):
            assert torch.equal(part[k], full[k][:, :nbest]), (nbest, k)


def test_mid_sized_case():
    _check("mid")


def test_widest_slot_set():
    """B 4, T 75, V 4364, W 16, C 16: all 272 slots, one thread each on the 320-thread launch, at the benchmark vocabulary."""
    _check("widest_slot_set")


def test_long_sequence():
    """B 2, T 400 (ragged), W 8, C 16: 25 staged chunks, a trie of 3201 nodes per utterance, sequences of about 100 labels."""
    c, got = _check("long")
    assert int(got["lengths"][:, 0].min()) >= 60


def test_another_blank_and_determinism():
    """blank = 2 instead of 0 (the restatement with the same blank), and two calls on one input return identical outputs."""
    c = R.cases_cached()["mid"]
    ref = R.search(c["logits"], c["lengths"], 4, 8, 4, blank=2)
    _compare(_run(c["logits"], c["lengths"], 4, 8, 4, blank=2), ref, "mid, blank 2")
    for name in ("mid", "widest_slot_set"):
        c = R.cases_cached()[name]
        a = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"])
        b = _run(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"])
        for k in ("ids", "lengths", "scores"):
            assert torch.equal(a[k], b[k]), (name, k)


def test_pruned_parent_created_again_still_merges_into_its_child():
    """Two inputs on which a prefix is pruned and re-created while its child stays in the list: the new parent's extension must be merged
    into the old child (prefixes are identified by their labels, not by where they were created), else the sequence appears twice in the
    n-best and loses the probability mass of that route."""
    for lg, W, want in ((R.RELINK_A, 4, [[1, 1], [1], [1, 2, 1], [1, 1, 2]]), (R.RELINK_B, 3, [[2, 1, 2, 1], [2, 1, 1], [2, 1, 2]])):
        x = np.array([lg], dtype=np.float32)
        ref = R.search(x, [len(lg)], W, 3, W)
        assert ref["relinked"][0] > 0 and ref["prune_margin"][0] >= R.DELTA
        got = _run(x, [len(lg)], W, 3, W)
        _compare(got, ref, "re-created parent, W %d" % W)
        assert [got["ids"][0, k, :got["lengths"][0, k]].tolist() for k in range(len(want))] == want


@pytest.mark.parametrize("V", [3, 4, 5, 6])
def test_sweep_of_small_random_utterances(V):
    """About 500 random-logit utterances per (V, W), T_b 4..13, C = V, W 3, 4, 5, those whose three margins are at least delta: the whole
    n-best against the restatement.  Random logits prune and re-create prefixes constantly; tests/test_ctc_beam_host.py counts the
    utterances of every batch that merge into a child of a re-created parent."""
    worst = 0.0
    for W in (3, 4, 5):
        lg, tb, ref = R.sweep(V, W)
        assert len(tb) >= 400 and int((ref["relinked"] > 0).sum()) >= 1
        worst = max(worst, _compare(_run(lg, tb, W, V, W), ref, "sweep V %d W %d (%d utterances, %d with a re-created parent)"
                                    % (V, W, len(tb), int((ref["relinked"] > 0).sum()))))
    print("sweep V %d: worst relative score error %.3e" % (V, worst))


def test_tie_rules_on_equal_logits():
    """All logits equal, one frame: every slot ties exactly.  The candidates are the lowest indices (the top-k's tie order) and the slots
    keep their index order (the rank count's tie rule): the empty prefix, then the labels in candidate order."""
    for V, W, C in ((4, 2, 4), (4, 3, 4), (4, 3, 2), (20, 16, 16), (20, 5, 0)):
        lg = np.zeros((2, 3, V), dtype=np.float32)
        lg[1] = 1.5
        got = _run(lg, [1, 1], W, C, W)
        ref = R.search(lg, [1, 1], W, C, W)
        assert np.all(ref["top_margin"] == 0.0)
        n_c = (C if C else min(V, 16)) - 1                       # the blank is index 0, first among equals: always among the top C
        want = [[]] + [[c] for c in range(1, n_c + 1)]
        for b in range(2):
            rows = [got["ids"][b, k, :got["lengths"][b, k]].tolist() for k in range(W) if got["lengths"][b, k] >= 0]
            assert rows == want[:W], (V, W, C, rows)
        assert torch.equal(got["ids"], torch.from_numpy(ref["ids"])) and torch.equal(got["lengths"], torch.from_numpy(ref["lengths"]))
        fin = ref["lengths"] >= 0
        assert np.allclose(got["scores"].numpy()[fin], -math.log(V), rtol=0, atol=TOL * math.log(V))
        assert torch.all(got["scores"][torch.from_numpy(~fin)] == -math.inf)


def test_refusals():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    lg = torch.zeros(1, 4, 20, device=dev)
    one = torch.tensor([4], dtype=torch.int32, device=dev)
    for W, C, nbest in ((17, 4, 1), (4, 17, 1), (4, 4, 5)):
        with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
            ops.ctc_beam_search(lg, one, W, C, nbest)
    with pytest.raises(L.AsrHipError):
        ops.ctc_beam_search(lg, one, 4, 4, 1, blank=20)
    with pytest.raises(L.AsrHipError):
        ops.ctc_beam_search(lg[:, :, :3], one, 4, 4, 1)                   # C above V
    with pytest.raises(L.AsrHipError):
        ops.ctc_beam_search(lg.cpu(), one.cpu(), 4, 4, 1)                 # host tensors
    with pytest.raises(AssertionError):
        ops.ctc_beam_search(lg.bfloat16(), one, 4, 4, 1)
    out = ops.ctc_beam_search(lg, one, 16, 0, 16)                          # candidates = 0: min(V, 16)
    assert tuple(out["ids"].shape) == (1, 16, 4)
    assert L.load().asr_ctc_beam_workspace(0, 4, 4, 4) == 0 and L.load().asr_ctc_beam_workspace(1, 4, 2, 3) == 4 + 12 + 24 + 2 * 9


# ------------------------------------------------------------------------------------------------ model and test.py level
def _head_model(cli, gain=4.0):
    """The tiny fp32 model of tests/test_gpu_joint_ctc.py with a CTC head; the head's weights times `gain`, so that a randomly initialised
    head has the peaked posteriors of a trained one (near-uniform posteriors fill a beam with ties no float32 search can be held to)."""
    import test_gpu_joint_ctc as J
    model = J._model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).eval()
    with torch.no_grad():
        model.ctc_linear.weight.mul_(gain)
    return model, J


def _encoded(model, J):
    src, lengths, tgt, _ = J._batch()
    with torch.no_grad():
        enc, _ = model.encoder(model._features(src), lengths)
        logits = model.ctc_logits(enc).cpu().numpy()
    frames = model.ctc_frame_lengths(lengths, enc.shape[1])
    assert frames == [40, 30, 22]
    return src, lengths, tgt, enc, logits, frames


def test_model_level_search_equals_the_reference_on_its_own_logits(cli):
    """Transformer.ctc_beam_search on the tiny model, B 3, W 4, C 8: the kernel's hypotheses (read before the ranking, c_weight 0 keeps
    their order) equal the restatement run on the model's own ctc_logits under the margin rule; W = 1, C = 1 likewise; the strings are
    the ids' labels; a model without the head raises."""
    model, J = _head_model(cli)
    _, _, _, enc, logits, frames = _encoded(model, J)
    for W, C in ((4, 8), (1, 1)):
        ref = R.search(logits, frames, W, C, W)
        print("W %d C %d margins: prune %s lineage %s top %s" % (W, C, ref["prune_margin"], ref["lineage_margin"], ref["top_margin"]))
        strs, ids = model.ctc_beam_search(enc, frames, W, nbest=W, candidates=C, c_weight=0, return_ids=True)
        assert len(strs) == len(ids) == 3
        for b in range(3):
            n = int((ref["lengths"][b] >= 0).sum()) if ref["prune_margin"][b] >= R.DELTA else 1
            want = [ref["ids"][b, k, :ref["lengths"][b, k]].tolist() for k in range(n)]
            assert ids[b][:n] == want, (W, C, b, ids[b], want)
            assert ref["lineage_margin"][b] >= R.DELTA and ref["top_margin"][b] >= R.DELTA
            assert strs[b] == ["".join(model.id2label[x] for x in row) for row in ids[b]]
            assert all(0 not in row for row in ids[b])                       # CTC labels as they stand: never the blank
        assert [s[0] for s in model.ctc_beam_search(enc, frames, W, candidates=C, c_weight=0)] == [s[0] for s in strs]
    plain = J._model(cli, ["--precision", "fp32"]).eval()
    with pytest.raises(ValueError, match="CTC head"):
        plain.ctc_beam_search(enc, frames, 4)


def test_evaluate_routes_to_the_ctc_beam_search(cli):
    """evaluate(ctc_beam=True) returns one string per utterance: the best of ctc_beam_search; align_source='hyp' aligns those ids unchanged
    (feasible by construction: the path collapses back to them)."""
    import ctc_align_reference as A
    model, J = _head_model(cli)
    src, lengths, tgt, enc, _, frames = _encoded(model, J)
    best, best_ids = model.ctc_beam_search(enc, frames, 4, nbest=1, c_weight=0.1, return_ids=True)
    _, hyps, gold, ali = model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, beam_nbest=3, c_weight=0.1, align_source="hyp")
    assert len(hyps) == len(gold) == 3 and all(isinstance(h, str) for h in hyps) and hyps == [rows[0] for rows in best]
    for b in range(3):
        want = best_ids[b][0]
        assert [x["id"] for x in ali[b]["labels"]] == want
        if want:
            assert math.isfinite(ali[b]["score"]) and A.collapse(ali[b]["path"], want) == want
    assert model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, c_weight=0.1)[1] == hyps
    with pytest.raises(ValueError, match="CTC head alone"):
        model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, ctc_greedy=True)


def test_lm_rescoring_orders_the_nbest_by_the_rank_ended_formula(cli, golden_dir):
    """With the fixture LM the n-best order equals a host re-ranking of the kernel's hypotheses by
    score + lm_weight * (lm - 2 * oov) + sqrt(words) * c_weight (Decoder._rank_ended), stable among equals."""
    from asr_hip import ops
    from utils.lstm_utils import LM, calculate_lm_scores
    model, J = _head_model(cli)
    _, _, _, enc, _, frames = _encoded(model, J)
    lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
    W, lm_weight, c_weight = 6, 0.3, 0.2
    with torch.no_grad():
        raw = ops.ctc_beam_search(model.ctc_logits(enc), torch.tensor(frames, dtype=torch.int32, device="cuda"), W, 0, W)
    strs, ids = model.ctc_beam_search(enc, frames, W, nbest=W, lm=lm, lm_weight=lm_weight, c_weight=c_weight, return_ids=True)
    plain = model.ctc_beam_search(enc, frames, W, nbest=W, c_weight=c_weight, return_ids=True)[1]
    changed = 0
    for b in range(3):
        hyps = [(raw["ids"][b, n, :raw["lengths"][b, n]].tolist(), float(raw["scores"][b, n])) for n in range(W) if raw["lengths"][b, n] >= 0]
        triples = calculate_lm_scores([g for g, _ in hyps], lm, model.id2label)
        final = [s + lm_weight * (lm_score - 2 * oov) + math.sqrt(words) * c_weight for (_, s), (lm_score, words, oov) in zip(hyps, triples)]
        order = sorted(range(len(hyps)), key=lambda i: -final[i])
        assert ids[b] == [hyps[i][0] for i in order], (b, ids[b], final)
        assert sorted(map(tuple, ids[b])) == sorted(map(tuple, plain[b]))
        changed += ids[b] != plain[b]
    print("utterances whose n-best order the LM changed: %d of 3" % changed)


def _loader():
    """Two utterances as the collate function delivers them: (inputs, targets, percentages, input sizes, target sizes)."""
    g = torch.Generator().manual_seed(3)
    src = torch.randn(2, 1, 161, 120, generator=g)
    src[1, :, :, 90:] = 0
    tgt = torch.tensor([[3, 4, 11, 5, 5, 6], [7, 11, 8, 0, 0, 0]])
    return [(src, tgt, torch.tensor([1.0, 0.75]), torch.tensor([120, 90], dtype=torch.int32), torch.tensor([6, 3], dtype=torch.int32))]


def test_test_py_decodes_with_ctc_beam_search(cli, tmp_path):
    """test.py's evaluate() with --ctc-beam-search on a two-utterance loader, with --align-out and --align-source hyp: it runs, one
    parseable line per utterance whose labels are the hypothesis' ids; a checkpoint without the head and the excluded flag combinations
    give the ValueError."""
    import test as test_mod
    import test_gpu_joint_ctc as J
    from utils import constant
    model, _ = _head_model(cli)
    out = tmp_path / "hyp.jsonl"
    flags = J.TINY + ["--precision", "fp32", "--ctc-weight", "0.3", "--ctc-beam-search", "--beam-width", "4", "--beam-nbest", "2"]
    args = cli(flags + ["--align-out", str(out), "--align-source", "hyp"])
    test_mod.check_ctc_decoding(args, model)
    seen = []
    orig = model.ctc_beam_search

    def recording(*a, **k):
        res = orig(*a, **k)
        seen.append(res)
        return res
    model.ctc_beam_search = recording
    try:
        cer, wer = test_mod.evaluate(model, _loader())
    finally:
        del model.ctc_beam_search
    assert np.isfinite(cer) and np.isfinite(wer) and len(seen) == 1
    strs, ids = seen[0]
    recs = [json.loads(l) for l in out.read_text(encoding="utf-8").splitlines()]
    assert len(recs) == 2
    for b, r in enumerate(recs):
        text = strs[b][0]
        for ch in (constant.EOS_CHAR, constant.SOS_CHAR, constant.PAD_CHAR):
            text = text.replace(ch, "")
        assert [l["id"] for l in r["labels"]] == ids[b][0] and r["text"] == text
        assert (r["score"] is not None and math.isfinite(r["score"])) or not ids[b][0]
    plain = J._model(cli, ["--precision", "fp32"]).eval()
    with pytest.raises(ValueError, match="CTC head"):
        test_mod.check_ctc_decoding(cli(flags), plain)
    for extra in (["--beam-search"], ["--ctc-greedy"], ["--ctc-decode-weight", "0.5"]):
        with pytest.raises(ValueError, match="--ctc-beam-search"):
            test_mod.check_ctc_decoding(cli(flags + extra), model)
    with pytest.raises(ValueError, match=r"1\.\.16"):
        test_mod.check_ctc_decoding(cli(flags + ["--beam-width", "17"]), model)
