"""Transformer.transducer_beam_search(ngram=..., context=...), evaluate(transducer_ngram=..., transducer_context=...) and test.py
--transducer-beam-search --transducer-ngram-path --transducer-context-path on the tiny model of
tests/test_gpu_rnnt_model.py: D 32, V 11, a handful of encoder frames.  The kernel's fused arms are pinned by
tests/test_gpu_rnnt_beam_fused.py; here the model hands them the right tensors and tables, forms every hypothesis' score by the formula
and ranks through asr_hip.search.rank_ended -- and with the tables off makes the launches and returns the bits it did before."""
import copy

import numpy as np
import pytest
import torch

import ctc_beam_lm_reference as M
from test_gpu_mwer_model import CHARS, GOLD, _batch, _corpus, cli, process_wide_random_state_is_left_as_found  # noqa: F401  (fixtures)
from test_gpu_rnnt_beam_model import _head_tensors
from test_gpu_rnnt_model import HEAD, _model

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _tables(model):
    """A Witten-Bell trigram over the tiny model's 11 labels (corpus over the ids 3..10, SOS / EOS as the sentence marks) and a phrase
    list in them."""
    from utils import constant
    from utils.context import ContextGraph
    from utils.ngram import NgramLM
    labels = [model.id2label[i] for i in range(11)]
    corpus = [[x + 2 for x in s] for s in M.synthetic_corpus(9, 21, 200)]
    lm = NgramLM.estimate(corpus, 11, 3, constant.SOS_TOKEN, constant.EOS_TOKEN, labels=labels)
    return lm, ContextGraph.from_phrases([[3, 4], [5], [4, 4, 6]], 11, labels)


def _sharp_model(cli, precision="fp32"):
    model = _model(cli, HEAD + ["--precision", precision], seed=1).eval()
    with torch.no_grad():
        model.rnnt_out.weight.mul_(8.0)          # a fresh head's rows are nearly uniform
    return model


def _calls(monkeypatch):
    from asr_hip import lib as L
    calls, orig = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *x: (calls.append(name), orig(name, *x))[1])
    return calls


def test_both_tables_against_the_formula_through_rank_ended(cli, monkeypatch):
    """W 6, K 0, S 2 with the trigram and the phrase list: the hypotheses handed to rank_ended are the kernel's (ops.rnnt_beam_search
    with bos = SOS, eos = EOS), each with rnnt_score, ngram_score, context_credit and score = rnnt_score + a * ngram_score + b * len + g *
    context_credit; the n-best is rank_ended's of exactly those, computed here in Python.  ngram_score is NgramLM.score with the EOS
    term, context_credit ContextGraph.earned.  One rnnt_enc GEMM, ONE search launch."""
    from asr_hip import ops, search
    from utils import constant
    model = _sharp_model(cli)
    lm, graph = _tables(model)
    enc = torch.randn(3, 6, 32, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = [6, 4, 0]
    W, a, b, g = 6, 0.5, 0.3, 1.5
    Pg = _head_tensors(model, enc)
    raw = ops.rnnt_beam_search(Pg["e"], Pg["tables"], Pg["w_out"], Pg["b_out"], torch.tensor(lengths, dtype=torch.int32, device="cuda"), W,
                               0, 2, W, ngram=lm, alpha=a, beta=b, bos=constant.SOS_TOKEN, eos=constant.EOS_TOKEN, context=graph, gamma=g)
    raw = {k: v.cpu() for k, v in raw.items()}
    assert sorted(raw) == ["credit", "ids", "lengths", "lm", "scores"]

    def ended():
        out = []
        for bi in range(3):
            hs = []
            for n in range(W):
                if raw["lengths"][bi, n] < 0:
                    continue
                y = raw["ids"][bi, n, :raw["lengths"][bi, n]].tolist()
                s, q, c = float(raw["scores"][bi, n]), float(raw["lm"][bi, n]), int(raw["credit"][bi, n])
                hs.append({'yseq': y, 'rnnt_score': s, 'ngram_score': q, 'context_credit': c, 'score': s + a * q + b * len(y) + g * c})
            out.append(hs)
        return out
    seen, orig = [], search.rank_ended

    def recording(e, *x, **k):
        seen.append(copy.deepcopy(e))
        return orig(e, *x, **k)
    monkeypatch.setattr(search, "rank_ended", recording)
    calls = _calls(monkeypatch)
    strs, ids = model.transducer_beam_search(enc, lengths, W, nbest=3, max_symbols=2, c_weight=0.2, return_ids=True, ngram=lm,
                                             ngram_weight=a, length_bonus=b, context=graph, context_score=g)
    assert [c for c in calls if c.startswith("asr_rnnt_beam")] == ["asr_rnnt_beam_search_ctx"]
    monkeypatch.setattr(search, "rank_ended", orig)
    assert len(seen) == 1 and seen[0] == ended()
    want = [[h['yseq'] for h in hs] for hs in orig(ended(), 3, 0.2, model.id2label, None, 0.1)]
    assert ids == want and strs == [["".join(model.id2label[x] for x in row) for row in rows] for rows in ids]
    assert seen[0][2] == [{'yseq': [], 'rnnt_score': 0.0, 'ngram_score': float(lm.logp((constant.SOS_TOKEN,), constant.EOS_TOKEN)),
                           'context_credit': 0, 'score': a * float(lm.logp((constant.SOS_TOKEN,), constant.EOS_TOKEN))}]
    n_credit = 0
    for hs in seen[0]:
        for h in hs:
            q = lm.score(h['yseq'], constant.SOS_TOKEN, constant.EOS_TOKEN)
            assert abs(h['ngram_score'] - q) <= TOL * max(1.0, abs(q)) and h['context_credit'] == graph.earned(h['yseq'])
            n_credit += h['context_credit'] > 0
    print("hypotheses with earned credit: %d" % n_credit)
    # the LM alone and the phrases alone take their own entries and carry their own fields
    for kw, entry, fields in ((dict(ngram=lm, ngram_weight=a, length_bonus=b), "asr_rnnt_beam_search_lm", {'ngram_score'}),
                              (dict(context=graph, context_score=g), "asr_rnnt_beam_search_ctx", {'ngram_score', 'context_credit'})):
        calls.clear()
        seen.clear()
        monkeypatch.setattr(search, "rank_ended", recording)
        model.transducer_beam_search(enc, lengths, W, nbest=3, max_symbols=2, **kw)
        monkeypatch.setattr(search, "rank_ended", orig)
        assert [c for c in calls if c.startswith("asr_rnnt_beam")] == [entry]
        assert all(set(h) == {'yseq', 'score', 'rnnt_score'} | fields for hs in seen[0] for h in hs)
        if 'ngram' not in kw:
            assert all(h['ngram_score'] == 0.0 and h['score'] == h['rnnt_score'] + g * h['context_credit'] for hs in seen[0] for h in hs)
    assert len(lm._tables) == 1 and len(graph._tables) == 1                     # each table went to the device once


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_with_the_tables_off_the_launches_and_the_bits_are_the_plain_search(cli, monkeypatch, precision):
    from asr_hip import ops
    model = _sharp_model(cli, precision)
    enc = torch.randn(3, 6, 32, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = [6, 4, 0]
    Pg = _head_tensors(model, enc)
    fl = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    calls = _calls(monkeypatch)
    plain = model.transducer_beam_search(enc, lengths, 4, nbest=4, candidates=3, max_symbols=2, c_weight=0.1, return_ids=True)
    first = list(calls)
    calls.clear()
    off = model.transducer_beam_search(enc, lengths, 4, nbest=4, candidates=3, max_symbols=2, c_weight=0.1, return_ids=True, ngram=None,
                                       ngram_weight=0.7, length_bonus=1.0, context=None, context_score=2.0)
    assert off == plain and calls == first and [c for c in calls if c.startswith("asr_rnnt_beam")] == ["asr_rnnt_beam_search"]
    # and with both tables at weight zero the kernel's three outputs are the plain entry's bits
    lm, graph = _tables(model)
    a = (Pg["e"], Pg["tables"], Pg["w_out"], Pg["b_out"], fl, 4, 3, 2, 4)
    raw, zero = ops.rnnt_beam_search(*a), ops.rnnt_beam_search(*a, ngram=lm, context=graph)
    assert sorted(raw) == ["ids", "lengths", "scores"] and all(torch.equal(raw[k], zero[k]) for k in raw)


def _loader():
    """Two utterances as the collate function delivers them: (inputs, targets, percentages, input sizes, target sizes)."""
    g = torch.Generator().manual_seed(3)
    src = torch.randn(2, 1, 161, 48, generator=g)
    src[1, :, :, 40:] = 0
    tgt = torch.tensor([[3, 4, 10, 5], [7, 10, 8, 0]])
    return [(src, tgt, torch.tensor([1.0, 0.8]), torch.tensor([48, 40], dtype=torch.int32), torch.tensor([4, 3], dtype=torch.int32))]


def test_evaluate_and_test_py_route_both_tables(cli, tmp_path):
    """evaluate(transducer_beam=True, transducer_ngram=..., transducer_context=...) returns the best of transducer_beam_search with the
    same five arguments; test.py's checks pass with --transducer-beam-search and its evaluate() hands the weights of the command line on
    with the LM loaded from --transducer-ngram-path's file and the list read from --transducer-context-path's; without the mode both
    paths are refused before any launch."""
    import test as test_mod
    from utils.context import ContextGraph
    from utils.ngram import NgramLM
    model = _sharp_model(cli)
    lm, graph = _tables(model)
    src, lengths, tgt, _ = _batch()
    with torch.no_grad():
        enc = model.encoder(model._features(src), lengths)[0]
        frames = model.ctc_frame_lengths(lengths, enc.shape[1])
        best = model.transducer_beam_search(enc, frames, 4, nbest=1, max_symbols=2, c_weight=0.1, ngram=lm, ngram_weight=0.6,
                                            length_bonus=0.2, context=graph, context_score=2.0)
        hyps = model.evaluate(src, lengths, tgt, transducer_beam=True, beam_width=4, beam_nbest=3, c_weight=0.1, transducer_max_symbols=2,
                              transducer_ngram=lm, transducer_ngram_weight=0.6, transducer_length_bonus=0.2, transducer_context=graph,
                              transducer_context_score=2.0)[1]
    assert hyps == [rows[0] for rows in best]
    with pytest.raises(ValueError, match="--transducer-ngram-path needs --transducer-beam-search"):
        model.evaluate(src, lengths, tgt, transducer_ngram=lm)
    with pytest.raises(ValueError, match="--transducer-context-path needs --transducer-beam-search"):
        model.evaluate(src, lengths, tgt, transducer_greedy=True, transducer_context=graph)
    ngram_path, context_path = str(tmp_path / "ngram.pt"), str(tmp_path / "phrases.txt")
    lm.save(ngram_path)
    with open(context_path, "w", encoding="utf8") as f:
        f.write("# names\nab\nc\n\nbbd\n")
    from test_gpu_mwer_model import TINY
    flags = TINY + HEAD + ["--precision", "fp32", "--beam-width", "4", "--beam-nbest", "2", "--transducer-max-symbols", "2",
                           "--transducer-ngram-path", ngram_path, "--transducer-ngram-weight", "0.6", "--transducer-ngram-length-bonus", "0.2",
                           "--transducer-context-path", context_path, "--transducer-context-score", "2.0"]
    with pytest.raises(ValueError, match="--transducer-ngram-path needs --transducer-beam-search"):
        test_mod.check_transducer_decoding(cli(flags), model)
    with pytest.raises(ValueError, match="needs --transducer-beam-search"):
        test_mod.check_transducer_decoding(cli(flags + ["--transducer-greedy"]), model)
    args = cli(flags + ["--transducer-beam-search"])
    test_mod.check_transducer_decoding(args, model)
    test_mod.check_ctc_decoding(args, model)
    label2id = {c: i for i, c in model.id2label.items()}
    loaded = NgramLM.load(args.transducer_ngram_path, model.id2label)
    listed = ContextGraph.from_file(args.transducer_context_path, label2id)
    assert listed.earned([3, 4]) == 2 and listed.earned([4, 4, 6]) == 3 and listed.earned([5]) == 1          # "ab", "bbd", "c"
    seen, orig = [], model.transducer_beam_search

    def recording(*a, **k):
        seen.append(k)
        return orig(*a, **k)
    model.transducer_beam_search = recording
    try:
        cer, wer = test_mod.evaluate(model, _loader(), transducer_ngram=loaded, transducer_context=listed)
        test_mod.evaluate(model, _loader())
    finally:
        del model.transducer_beam_search
    assert np.isfinite(cer) and np.isfinite(wer) and len(seen) == 2
    assert seen[0]["ngram"] is loaded and seen[0]["ngram_weight"] == 0.6 and seen[0]["length_bonus"] == 0.2
    assert seen[0]["context"] is listed and seen[0]["context_score"] == 2.0 and seen[0]["max_symbols"] == 2
    assert seen[1]["ngram"] is None and seen[1]["context"] is None
