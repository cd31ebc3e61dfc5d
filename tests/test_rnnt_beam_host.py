"""The float64 restatement of the transducer beam search (tests/rnnt_beam_reference.py) pinned on the CPU -- against brute force over
every alignment, against the training lattice of tests/rnnt_reference.py, on hand-built inputs -- and the host side of
--transducer-beam-search: argument parsing and every refusal of test.check_transducer_decoding, before any launch."""
import math

import numpy as np
import pytest
import torch

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


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_an_unpruned_search_sums_every_alignment(T, S, C):
    """V 3, W large enough that nothing is pruned: the score of EVERY sequence is the log of the enumerated sum over its alignments with
    at most S labels per frame, and for S >= len(y) it is -nll of the training lattice."""
    row = _rows(T, 3, C, 10 * T + S)
    res = R.search(row, T, 3, W=1000, K=2, S=S, nbest=1000, C=C)
    truth = R.enumerate_scores(row, T, 3, S, C)
    assert not res["pruned"] and len(res["hyps"]) == len(truth) == sum(2 ** n for n in range(T * S + 1))
    for y, s in res["hyps"]:
        assert abs(float(s) - truth[y]) <= 1e-12 * max(1.0, abs(truth[y])), (y, float(s), truth[y])
        if len(y) <= S:
            lg = torch.from_numpy(R.training_logits(row, y, T, 3, C))[None]
            nll = float(RL.loss_and_grad(lg, torch.tensor([list(y) + [0]]), [T], [len(y)])["nll"][0])
            assert abs(float(s) + nll) <= 1e-12 * max(1.0, abs(nll)), (y, float(s), -nll)
    assert [s for _, s in res["hyps"]] == sorted((s for _, s in res["hyps"]), reverse=True)


def test_the_fp32_run_of_the_same_search_stays_within_fp32_of_it():
    row = _rows(3, 5, 2, 3)
    a = R.search(row, 3, 5, W=4, K=3, S=2, nbest=4)
    b = R.search(row, 3, 5, W=4, K=3, S=2, nbest=4, dtype=np.float32)
    assert [y for y, _ in a["hyps"]] == [y for y, _ in b["hyps"]] and all(s.dtype == np.float32 for _, s in b["hyps"])
    assert max(abs(float(s) - float(t)) for (_, s), (_, t) in zip(a["hyps"], b["hyps"])) <= 64 * R.EPS32 * a["maxabs"]


def test_the_winner_wins_only_through_the_merge():
    P = R.merge_case()
    row = R.table_row(P["e"][0], P["tables"], P["w_out"], P["b_out"])
    res = R.search(row, 2, 4, W=4, K=3, S=1, nbest=4, C=1)
    (y0, s0), (y1, s1) = res["hyps"][:2]
    assert y0 == (2,) and y1 == (3,)
    lp = lambda t, y: R.log_softmax(np.asarray(row(t, R.context(y, 1)), dtype=np.float64))     # noqa: E731
    label_first = lp(0, ())[2] + lp(0, (2,))[0] + lp(1, (2,))[0]
    blank_first = lp(0, ())[0] + lp(1, ())[2] + lp(1, (2,))[0]
    assert label_first < float(s1) and blank_first < float(s1) < float(s0)
    assert abs(float(s0) - np.logaddexp(label_first, blank_first)) <= 1e-12
    assert R.min_margin(res) >= 0.1


def test_max_symbols_cuts_a_head_that_never_offers_the_blank():
    P = R.cut_case(2)
    row = R.table_row(P["e"][0], P["tables"], P["w_out"], P["b_out"])
    for S in (1, 2, 4):
        res = R.search(row, 2, 3, W=16, K=1, S=S, nbest=16, C=1)
        assert sorted(len(y) for y, _ in res["hyps"]) == list(range(2 * S + 1)) and all(set(y) <= {2} for y, _ in res["hyps"])
        truth = R.enumerate_scores(row, 2, 3, S, 1)
        assert all(abs(float(s) - truth[y]) <= 1e-12 for y, s in res["hyps"])


def test_tie_order():
    """Uniform rows: every decision is a tie.  Candidates: the parent's place in C_s first, then the label id; D: first insertion; the
    K best labels of a row: the lowest ids."""
    row = lambda t, ctx: np.zeros(3)      # noqa: E731
    res = R.search(row, 1, 3, W=3, K=2, S=2, nbest=3, C=1)
    assert [y for y, _ in res["last_d"]] == [(), (1,), (2,), (1, 1), (1, 2), (2, 1)]
    assert [y for y, _ in res["hyps"]] == [(), (1,), (2,)] and res["margins"]["cand"] == 0.0 and res["pruned"]
    row4 = lambda t, ctx: np.zeros(4)     # noqa: E731
    res = R.search(row4, 1, 4, W=2, K=1, S=1, nbest=2, C=2)
    assert [y for y, _ in res["hyps"]] == [(), (1,)] and res["margins"]["topk"] == 0.0
    res = R.search(row4, 1, 4, W=2, K=3, S=1, nbest=2, C=2)
    assert [y for y, _ in res["last_d"]] == [(), (1,), (2,)]


def test_no_frames_and_fewer_hypotheses_than_nbest():
    row = _rows(2, 3, 2, 1)
    empty = R.search(row, 0, 3, W=4, K=2, S=2, nbest=4)
    assert empty["hyps"] == [((), 0.0)] and empty["last_d"] == [] and R.min_margin(empty) == math.inf
    few = R.search(row, 1, 3, W=16, K=2, S=1, nbest=16)
    assert sorted(y for y, _ in few["hyps"]) == [(), (1,), (2,)]
    ids, lens, sc = R.as_arrays([empty, few], 16, 2)
    assert lens[0].tolist() == [0] + [-1] * 15 and sc[0, 0] == 0.0 and np.all(np.isneginf(sc[0, 1:])) and np.all(ids[0] == 0)
    assert sorted(lens[1].tolist()) == [-1] * 13 + [0, 1, 1] and np.all(np.isneginf(sc[1, 3:])) and np.all(np.isfinite(sc[1, :3]))


def test_context_is_the_last_labels_first_with_sos_in_front():
    assert R.context((), 2) == (1, 1) and R.context((5,), 2) == (5, 1) and R.context((5, 6, 7), 2) == (7, 6) and R.context((5, 6), 1) == (6,)


# ------------------------------------------------------------------------------------------------ the command line
TINY = ("--num-layers 1 --num-heads 2 --dim-model 32 --dim-key 16 --dim-value 16 --dim-inner 64 --dim-emb 32 --tgt-max-len 16 "
        "--src-max-len 64 --dropout 0").split()


def _model(cli, extra=()):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list("ab ")
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(TINY + list(extra)), l2i, {i: c for c, i in l2i.items()})


def test_arguments():
    from utils import constant
    a = constant.parse([])
    assert a.transducer_beam_search is False and a.transducer_candidates == 0
    a = constant.parse(["--transducer-beam-search", "--transducer-candidates", "4", "--beam-width", "8", "--transducer-max-symbols", "3"])
    assert a.transducer_beam_search is True and a.transducer_candidates == 4 and a.beam_width == 8 and a.transducer_max_symbols == 3


def test_decoding_refusals_and_the_arguments_evaluate_gets(cli):
    import test as test_mod
    plain = _model(cli)
    head = _model(cli, ["--transducer-weight", "0.3", "--ctc-weight", "0.3", "--transducer-dim-joint", "16"])
    flag = ["--transducer-beam-search"]
    with pytest.raises(ValueError, match="--transducer-beam-search needs a model with a transducer head"):
        test_mod.check_transducer_decoding(cli(flag), plain)
    for other in (["--transducer-greedy"], ["--beam-search"], ["--ctc-greedy"], ["--ctc-beam-search"],
                  ["--beam-search", "--ctc-decode-weight", "0.3"], ["--ctc-beam-search", "--attention-rescoring-weight", "0.5"],
                  ["--ngram-path", "x"], ["--context-path", "x"], ["--align-out", "x"]):
        with pytest.raises(ValueError, match="--transducer-beam-search decodes from the transducer head alone: it cannot be combined with "
                           + other[0]):
            test_mod.check_transducer_decoding(cli(flag + other), head)
    for w in ("0", "17"):
        with pytest.raises(ValueError, match="1..16"):
            test_mod.check_transducer_decoding(cli(flag + ["--beam-width", w]), head)
    with pytest.raises(ValueError, match="--transducer-candidates"):
        test_mod.check_transducer_decoding(cli(flag + ["--transducer-candidates", "17"]), head)
    with pytest.raises(ValueError, match="at least 1"):
        test_mod.check_transducer_decoding(cli(flag + ["--transducer-max-symbols", "0"]), head)
    with pytest.raises(ValueError, match="1024"):
        test_mod.check_transducer_decoding(cli(flag + ["--beam-width", "16", "--transducer-max-symbols", "64"]), head)
    test_mod.check_transducer_decoding(cli(flag + ["--beam-width", "16", "--transducer-candidates", "16", "--lm-rescoring"]), head)
    test_mod.check_transducer_decoding(cli(["--beam-width", "40", "--beam-search"]), plain)      # without the flag nothing is checked
    assert test_mod.transducer_decoding(cli([])) == {}
    assert test_mod.transducer_decoding(cli(["--transducer-greedy"])) == dict(transducer_greedy=True, transducer_max_symbols=5)
    assert test_mod.transducer_decoding(cli(flag + ["--transducer-candidates", "4", "--transducer-max-symbols", "3"])) == dict(
        transducer_beam=True, transducer_max_symbols=3, transducer_candidates=4)
    # the model's own entry points refuse the same misuse before any device work
    x, y = torch.zeros(1, 1, 161, 8), torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="transducer head"):
        plain.evaluate(x, [8], y, transducer_beam=True, beam_width=4)
    for other in (dict(transducer_greedy=True), dict(beam_search=True), dict(ctc_greedy=True), dict(ctc_beam=True),
                  dict(align_source="gold")):
        with pytest.raises(ValueError, match="--transducer-beam-search decodes from the transducer head alone"):
            head.evaluate(x, [8], y, transducer_beam=True, beam_width=4, **other)
    with pytest.raises(ValueError, match="1..16"):
        head.evaluate(x, [8], y, transducer_beam=True, beam_width=17)
    with pytest.raises(ValueError, match="at least 1"):
        head.evaluate(x, [8], y, transducer_beam=True, beam_width=4, transducer_max_symbols=0)
    with pytest.raises(ValueError, match="needs lm"):
        head.evaluate(x, [8], y, transducer_beam=True, beam_width=4, lm_rescoring=True)
    enc = torch.zeros(1, 2, 32)
    with pytest.raises(ValueError, match="transducer head"):
        plain.transducer_beam_search(enc, [2], 4)
    for kw, msg in ((dict(beam_width=0), "1..16"), (dict(beam_width=17), "1..16"), (dict(beam_width=4, nbest=0), "nbest"),
                    (dict(beam_width=4, max_symbols=0), "at least 1"), (dict(beam_width=4, candidates=17), "0..16")):
        with pytest.raises(ValueError, match=msg):
            head.transducer_beam_search(enc, [2], **kw)


def test_the_binding_declares_the_new_entries():
    from asr_hip import lib as L
    assert {"asr_rnnt_beam_workspace", "asr_rnnt_beam_search"} <= set(L.header_symbols()) & set(L._SIGS)
    assert len(L._SIGS["asr_rnnt_beam_search"][1]) == 23 and len(L._SIGS["asr_rnnt_beam_workspace"][1]) == 6


def test_the_op_refuses_mismatched_tensors_with_a_value_error():
    """Every argument check of ops.rnnt_beam_search is a ValueError raised before the library is touched (host tensors suffice)."""
    from asr_hip import ops
    e, tab, w, b = torch.zeros(2, 3, 8), torch.zeros(5, 8), torch.zeros(5, 8), torch.zeros(5)
    n = torch.zeros(2, dtype=torch.int32)
    for kw, msg in ((dict(tables=[]), "one or two"), (dict(tables=[tab.bfloat16()]), r"tables\[0\]"), (dict(w_out=torch.zeros(5, 16)), "w_out"),
                    (dict(e=e.double(), tables=[tab.double()], w_out=w.double()), "e must be"), (dict(b_out=b.bfloat16()), "b_out"),
                    (dict(b_out=torch.zeros(4)), "b_out"), (dict(lengths=n.long()), "lengths"), (dict(lengths=n[:1]), "lengths")):
        args = dict(dict(e=e, tables=[tab], w_out=w, b_out=b, lengths=n), **kw)
        with pytest.raises(ValueError, match=msg):
            ops.rnnt_beam_search(args["e"], args["tables"], args["w_out"], args["b_out"], args["lengths"], 4)
