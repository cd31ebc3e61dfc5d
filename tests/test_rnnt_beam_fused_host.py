"""The float64 restatement of the fused arms of the transducer beam search (tests/rnnt_beam_fused_reference.py) pinned on the CPU --
against the plain restatement with the weights at zero, against NgramLM and ContextGraph.walk on every result, against the training
lattice where the beam holds every sequence, on hand-built inputs for the tie orders, the end term, T_b = 0 and an unfinished phrase --
and the host side of --transducer-ngram-path / --transducer-context-path: flag defaults and every new refusal, before any launch."""
import math

import numpy as np
import pytest
import torch

import rnnt_beam_fused_reference as F
import rnnt_beam_reference as R
import rnnt_reference as RL


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _rows(T, V, C, seed, J=8):
    P = R.random_case(1, T, J, V, C, seed)
    return R.table_row(P["e"][0], P["tables"], P["w_out"], P["b_out"])


def _plain(h):
    return [(y, float(s)) for y, s in h]


@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("C", [1, 2])
def test_weights_zero_is_the_plain_restatement(order, C):
    """alpha = beta = gamma = 0 with both tables present: sequences, scores, the last frame's D and the pruning margins are the plain
    restatement's; lm and credit are still reported."""
    V = 7
    row = _rows(4, V, C, 3 + C)
    lm, graph = F.synthetic_lm(V, order), F.random_graph(V, 1)
    for Tb in (4, 1, 0):
        a = R.search(row, Tb, V, W=4, K=3, S=2, nbest=4, C=C)
        b = F.search(row, Tb, V, W=4, K=3, S=2, nbest=4, C=C, lm=lm, graph=graph)
        assert [(y, float(s)) for y, s, _, _ in b["hyps"]] == _plain(a["hyps"]) and _plain(b["last_d"]) == _plain(a["last_d"])
        assert b["margins"] == a["margins"] and b["pruned"] == a["pruned"] and b["maxabs"] == a["maxabs"]
        assert any(h[2] != 0.0 for h in b["hyps"])


@pytest.mark.parametrize("order,eos", [(1, 0), (2, 0), (4, 0), (3, -1)])
def test_lm_len_and_credit_of_every_result_are_the_host_structures_values(order, eos):
    V = 9
    row = _rows(5, V, 2, 11)
    lm, graph = F.synthetic_lm(V, order), F.random_graph(V, 2)
    res = F.search(row, 5, V, W=6, K=4, S=2, nbest=6, lm=lm, alpha=F.ALPHA, beta=F.BETA, eos=eos, graph=graph, gamma=F.GAMMA)
    assert len(res["hyps"]) == 6 and res["pruned"]
    for (y, s, lmv, cr), key in zip(res["hyps"], res["keys"]):
        want = lm.score(list(y), F.BOS, eos)                  # NgramLM: float32 queries summed in float64
        assert abs(lmv - want) <= 1e-5 * max(1.0, abs(want)), (y, lmv, want)
        state, credit = graph.walk(y)
        assert cr == credit - int(graph.hold[state]) == graph.earned(y)
        assert abs(key - (float(s) + F.ALPHA * lmv + F.BETA * len(y) + F.GAMMA * cr)) <= 1e-9
    assert res["keys"] == sorted(res["keys"], reverse=True)
    if eos < 0:
        assert all(abs(h[2] - lm.score(list(h[0]), F.BOS, None)) <= 1e-5 * max(1.0, abs(h[2])) for h in res["hyps"])


def test_the_fused_key_changes_what_survives():
    V = 9
    row = _rows(5, V, 2, 11)
    a = R.search(row, 5, V, W=3, K=4, S=2, nbest=3)
    b = F.search(row, 5, V, W=3, K=4, S=2, nbest=3, lm=F.synthetic_lm(V, 3), alpha=2.0, beta=1.0, graph=F.random_graph(V, 2), gamma=3.0)
    assert [y for y, _ in a["hyps"]] != [h[0] for h in b["hyps"]]


def test_where_the_beam_holds_every_sequence_the_score_is_still_the_training_likelihood():
    """V 3, T 2, S 1: 7 sequences of at most 2 labels; W 16 holds them all, whatever the bonus, and each acoustic score is -nll of the
    training lattice (len(y) <= S) or the enumerated sum over its alignments."""
    row = _rows(2, 3, 2, 21)
    lm, graph = F.synthetic_lm(3, 2), F.graph_of([[2, 1], [1]], 3)
    res = F.search(row, 2, 3, W=16, K=2, S=1, nbest=16, lm=lm, alpha=1.5, beta=0.7, graph=graph, gamma=2.0)
    truth = R.enumerate_scores(row, 2, 3, 1, 2)
    assert not res["pruned"] and len(res["hyps"]) == len(truth) == 7
    for y, s, _, _ in res["hyps"]:
        assert abs(float(s) - truth[y]) <= 1e-12 * max(1.0, abs(truth[y]))
        if len(y) <= 1:
            lg = torch.from_numpy(R.training_logits(row, y, 2, 3, 2))[None]
            nll = float(RL.loss_and_grad(lg, torch.tensor([list(y) + [0]]), [2], [len(y)])["nll"][0])
            assert abs(float(s) + nll) <= 1e-12 * max(1.0, abs(nll)), (y, float(s), -nll)
    plain = R.search(row, 2, 3, W=16, K=2, S=1, nbest=16)
    assert [h[0] for h in res["hyps"]] != [y for y, _ in plain["hyps"]]          # the order is the fused key's, the scores are not


def test_tie_orders_at_the_frame_end_and_in_the_final_order():
    """Uniform rows, a uniform unigram LM and no phrase that any sequence meets: every key of a length is a tie.  Candidates: the parent's
    place, then the label id; D: first insertion; the final order: the place in A.  beta > 0 then puts longer sequences first, and ties
    within a length keep those orders."""
    from utils.ngram import NgramLM
    row = lambda t, ctx: np.zeros(3)      # noqa: E731
    lm = NgramLM.estimate([[1], [2]], 3, 1, F.BOS, F.EOS)
    assert lm.logp((0,), 1) == lm.logp((0,), 2)
    res = F.search(row, 1, 3, W=3, K=2, S=2, nbest=3, C=1, lm=lm, alpha=0.0, beta=0.0)
    assert [y for y, _ in res["last_d"]] == [(), (1,), (2,), (1, 1), (1, 2), (2, 1)]
    assert [h[0] for h in res["hyps"]] == [(), (1,), (2,)] and res["margins"]["cand"] == 0.0 and res["margins"]["order"] == 0.0
    res = F.search(row, 1, 3, W=3, K=2, S=2, nbest=3, C=1, lm=lm, alpha=0.0, beta=5.0)
    assert [y for y, _ in res["last_d"]] == [(1, 1), (1, 2), (2, 1), (1,), (2,), ()]
    assert [h[0] for h in res["hyps"]] == [(1, 1), (1, 2), (2, 1)] and res["margins"]["beam"] > 0 and res["margins"]["order"] == 0.0
    # the final key alone: [1] holds the phrase [1, 2] unfinished and leads A; at the end it earns nothing and ties with [2]: place first
    graph = F.graph_of([[1, 2]], 3)
    res = F.search(row, 1, 3, W=2, K=2, S=1, nbest=2, C=1, graph=graph, gamma=1.0, beta=3.0)
    assert [y for y, _ in res["last_d"]] == [(1,), (2,), ()] and [h[0] for h in res["hyps"]] == [(1,), (2,)]
    assert res["margins"]["order"] == 0.0 and [h[3] for h in res["hyps"]] == [0, 0]


def test_no_end_term_for_eos_minus_one():
    V = 6
    row = _rows(3, V, 1, 5)
    lm = F.synthetic_lm(V, 3)
    a = F.search(row, 3, V, W=4, K=3, S=1, nbest=4, C=1, lm=lm, alpha=1.0, eos=-1)
    b = F.search(row, 3, V, W=4, K=3, S=1, nbest=4, C=1, lm=lm, alpha=1.0, eos=F.EOS)
    assert {h[0] for h in a["hyps"]} == {h[0] for h in b["hyps"]}                # the end term enters the final order only
    lm_a, lm_b = {h[0]: h[2] for h in a["hyps"]}, {h[0]: h[2] for h in b["hyps"]}
    for y in lm_a:
        assert abs(lm_a[y] - lm.score(list(y), F.BOS, None)) <= 1e-5 * max(1.0, abs(lm_a[y]))
        assert abs((lm_b[y] - lm_a[y]) - float(lm.logp((F.BOS,) + y, F.EOS))) <= 1e-5


def test_no_frames():
    row = _rows(2, 5, 2, 1)
    lm, graph = F.synthetic_lm(5, 3), F.random_graph(5, 3)
    for eos, want in ((F.EOS, float(lm.logp((F.BOS,), F.EOS))), (-1, 0.0)):
        res = F.search(row, 0, 5, W=4, K=2, S=2, nbest=4, lm=lm, alpha=0.5, beta=0.3, eos=eos, graph=graph, gamma=2.0)
        assert len(res["hyps"]) == 1 and res["last_d"] == [] and F.min_margin(res) == math.inf
        y, s, lmv, cr = res["hyps"][0]
        assert y == () and float(s) == 0.0 and abs(lmv - want) <= 1e-6 and cr == 0
    ids, lens, sc, lmv, credit = F.as_arrays([res], 4, 4)
    assert lens[0].tolist() == [0, -1, -1, -1] and np.all(lmv[0, 1:] == 0.0) and np.all(credit[0] == 0) and np.all(np.isneginf(sc[0, 1:]))


def test_an_unfinished_phrase_earns_nothing():
    """The head spells 2 then 3; the phrase [2, 3, 4] is two labels in when the utterance ends.  While the beam is pruned [2, 3] carries a
    credit of 2; the result reports 0 for it and orders it by that."""
    P = R.cut_case(2)
    P["b_out"] = np.array([0.0, -3.0, 3.0, 2.5, -3.0], dtype=np.float32)
    P["tables"], P["w_out"] = [np.zeros((5, 8), dtype=np.float32)], np.zeros((5, 8), dtype=np.float32)
    row = R.table_row(P["e"][0], P["tables"], P["w_out"], P["b_out"])
    graph = F.graph_of([[2, 3, 4], [3]], 5)
    assert graph.walk([2, 3])[1] == 2 and graph.earned([2, 3]) == 0 and graph.earned([3]) == 1
    res = F.search(row, 2, 5, W=8, K=3, S=1, nbest=8, C=1, graph=graph, gamma=3.0)
    got = {h[0]: h[3] for h in res["hyps"]}
    assert got[(2, 3)] == 0 and got[(3,)] == 1 and got[(2,)] == 0
    for (y, s, _, cr), key in zip(res["hyps"], res["keys"]):
        assert abs(key - (float(s) + 3.0 * cr)) <= 1e-12


def test_the_survival_input():
    """[3] is in no plain n-best and in both fused arms': it survives only through the bonus in the pruning."""
    P = F.survival_case()
    row = R.table_row(P["e"][0], P["tables"], P["w_out"], P["b_out"])
    plain = R.search(row, 2, 5, W=2, K=3, S=1, nbest=2, C=1)
    assert [y for y, _ in plain["hyps"]] == [(2,), (4,)] and R.min_margin(plain) >= 0.1
    ctx = F.search(row, 2, 5, W=2, K=3, S=1, nbest=2, C=1, graph=F.graph_of([[3]], 5), gamma=3.0)
    lm = F.search(row, 2, 5, W=2, K=3, S=1, nbest=2, C=1, lm=F.survival_lm(), alpha=2.0)
    assert ctx["hyps"][0][0] == (3,) and lm["hyps"][0][0] == (3,) and F.min_margin(ctx) >= 0.1 and F.min_margin(lm) >= 0.1


# ------------------------------------------------------------------------------------------------ the command line
TINY = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 16 "
        "--src-max-len 64 --dropout 0").split()


def _model(cli, extra=()):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list("ab ")
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(TINY + list(extra)), l2i, {i: c for c, i in l2i.items()})


def test_flag_defaults():
    from utils import constant
    a = constant.parse([])
    assert a.transducer_ngram_path is None and a.transducer_context_path is None
    assert a.transducer_ngram_weight == 0.3 and a.transducer_ngram_length_bonus == 0.0 and a.transducer_context_score == 3.0
    a = constant.parse(["--transducer-beam-search", "--transducer-ngram-path", "n", "--transducer-ngram-weight", "0.7",
                        "--transducer-ngram-length-bonus", "0.2", "--transducer-context-path", "c", "--transducer-context-score", "1.5"])
    assert (a.transducer_ngram_path, a.transducer_ngram_weight, a.transducer_ngram_length_bonus) == ("n", 0.7, 0.2)
    assert (a.transducer_context_path, a.transducer_context_score) == ("c", 1.5) and a.ngram_path is None and a.context_path is None


def test_every_new_refusal_comes_before_any_launch(cli):
    import test as test_mod
    from utils.context import ContextGraph
    from utils.ngram import NgramLM
    head = _model(cli, ["--transducer-weight", "0.3", "--ctc-weight", "0.3", "--transducer-dim-joint", "16"])
    for flag, msg in ((["--transducer-ngram-path", "x"], "--transducer-ngram-path needs --transducer-beam-search"),
                      (["--transducer-context-path", "x"], "--transducer-context-path needs --transducer-beam-search")):
        for mode in ([], ["--transducer-greedy"], ["--ctc-beam-search"], ["--beam-search"]):
            with pytest.raises(ValueError, match=msg):
                test_mod.check_transducer_decoding(cli(flag + mode), head)
        test_mod.check_transducer_decoding(cli(flag + ["--transducer-beam-search"]), head)
    # the CTC search's flags keep their meaning beside the transducer search
    with pytest.raises(ValueError, match="cannot be combined with --ngram-path"):
        test_mod.check_transducer_decoding(cli(["--transducer-beam-search", "--transducer-ngram-path", "x", "--ngram-path", "y"]), head)
    V = len(head.id2label)
    labels = [head.id2label[i] for i in range(V)]
    lm = NgramLM.estimate([[3, 4], [4, 5]], V, 2, 1, 2, labels=labels)
    graph = ContextGraph.from_phrases([[3, 4]], V, labels)
    x, y = torch.zeros(1, 1, 161, 8), torch.zeros(1, 2, dtype=torch.int64)
    for kw in (dict(transducer_ngram=lm), dict(transducer_context=graph)):
        for mode in ({}, dict(transducer_greedy=True), dict(ctc_beam=True, beam_width=4), dict(beam_search=True, beam_width=4)):
            with pytest.raises(ValueError, match="needs --transducer-beam-search"):
                head.evaluate(x, [8], y, **kw, **mode)
    other = NgramLM.estimate([[3, 4]], V + 1, 2, 1, 2)
    with pytest.raises(ValueError, match="another label file"):
        head.evaluate(x, [8], y, transducer_beam=True, beam_width=4, transducer_ngram=other)
    with pytest.raises(ValueError, match="another label file"):
        head.evaluate(x, [8], y, transducer_beam=True, beam_width=4, transducer_context=ContextGraph.from_phrases([[3]], V + 1))
    enc = torch.zeros(1, 2, 32)
    with pytest.raises(ValueError, match="another label file"):
        head.transducer_beam_search(enc, [2], 4, ngram=other)
    with pytest.raises(ValueError, match="another label file"):
        head.transducer_beam_search(enc, [2], 4, context=ContextGraph.from_phrases([[3]], V + 1))


def test_evaluate_hands_the_tables_and_weights_on(cli, monkeypatch):
    """test.evaluate's fusion arguments: the transducer flags' values under the transducer_* keywords, nothing without a table."""
    import test as test_mod
    seen = {}

    class Model:
        def eval(self):
            pass

        def evaluate(self, *a, **kw):
            seen.update(kw)
            return None, [], []
    args = cli(["--transducer-beam-search", "--transducer-ngram-weight", "0.7", "--transducer-ngram-length-bonus", "0.2",
                "--transducer-context-score", "1.5"])
    args.cuda = False
    monkeypatch.setattr(test_mod.constant, "USE_CUDA", False, raising=False)
    batch = [(torch.zeros(1, 1, 161, 8), torch.zeros(1, 2, dtype=torch.int64), None, [8], [2])]
    test_mod.evaluate(Model(), batch, transducer_ngram="N", transducer_context="C")
    assert seen["transducer_ngram"] == "N" and seen["transducer_ngram_weight"] == 0.7 and seen["transducer_length_bonus"] == 0.2
    assert seen["transducer_context"] == "C" and seen["transducer_context_score"] == 1.5 and seen["transducer_beam"] is True
    assert "ngram" not in seen and "context" not in seen
    seen.clear()
    test_mod.evaluate(Model(), batch)
    assert not any(k.startswith("transducer_ngram") or k.startswith("transducer_context") or k == "transducer_length_bonus" for k in seen)


def test_the_binding_declares_the_new_entries():
    from asr_hip import lib as L
    assert {"asr_rnnt_beam_search_lm", "asr_rnnt_beam_search_ctx"} <= set(L.header_symbols()) & set(L._SIGS)
    assert len(L._SIGS["asr_rnnt_beam_search_lm"][1]) == 22 + 11 and len(L._SIGS["asr_rnnt_beam_search_ctx"][1]) == 22 + 19
    assert L._SIGS["asr_rnnt_beam_search_lm"][1][:22] == L._SIGS["asr_rnnt_beam_search"][1][:22]


def test_the_op_refuses_tables_over_other_labels_before_the_library_is_touched():
    from asr_hip import ops
    e, tab, w, b = torch.zeros(2, 3, 8), torch.zeros(5, 8), torch.zeros(5, 8), torch.zeros(5)
    n = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="n-gram LM has 6 labels, the head 5"):
        ops.rnnt_beam_search(e, [tab], w, b, n, 4, ngram=F.synthetic_lm(6, 2))
    with pytest.raises(ValueError, match="phrase list has 6 labels, the head 5"):
        ops.rnnt_beam_search(e, [tab], w, b, n, 4, context=F.graph_of([[2]], 6))
