"""Attention rescoring of the CTC prefix beam search's n-best: asr_seq_logprob (csrc/seq_logprob.hip) against
the float64 restatement tests/attn_rescore_reference.py, Decoder.score_hypotheses pinned to the executed reference's own logits
(tests/golden/dec_d128.npz), and the model, ranking and test.py levels on the tiny model of tests/test_gpu_joint_ctc.py.

Kernel bound (tests/attn_rescore_reference.py `bounds`; tests/test_attn_rescore_host.py shows it is neither vacuous nor broken by a
correct fp32 implementation): per segment |got - ref64| <= 4 * max(|torch32 - ref64|, eps32 * sum |tok_lp|), per row the same with the
row's own term; -inf exactly where the reference is -inf; no NaN.
Model bound: a score of n + 1 terms within (n + 1) * 2 * 2e-4 * max |logit| -- the per-logit fp32 bound
tests/test_gpu_decode.py::test_d128_fp32_reproduces_the_reference_logits_and_strings holds, doubled for the two terms of a
log-probability (the target's logit and the log-sum-exp); bf16: 3e-2 in place of 2e-4, that file's bf16 logit bound."""
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_rescore_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


# ------------------------------------------------------------------------------------------------ the kernel
def _run(buf, V, tgt, seg_off):
    """The logits as the first V columns of `buf` on the device (a view: row stride buf.shape[1]) -> (score, tok) on the host."""
    from asr_hip import ops
    dev = torch.device("cuda")
    wide = torch.as_tensor(np.asarray(buf)).to(dev)
    out = ops.seq_logprob(wide[:, :V], torch.as_tensor(np.asarray(tgt)).to(dev), torch.as_tensor(np.asarray(seg_off, dtype=np.int32)).to(dev))
    torch.cuda.synchronize()
    assert out["tok"].dtype == out["score"].dtype == torch.float32
    assert tuple(out["tok"].shape) == (len(tgt),) and tuple(out["score"].shape) == (len(seg_off) - 1,)
    return out["score"].cpu(), out["tok"].cpu()


def _run_case(name):
    c = R.cases()[name]
    return c, _run(c["buf"], c["V"], c["tgt"], c["seg_off"])


def _within(got, ref, bound, what):
    """-inf exactly where the reference is, no NaN, |got - ref| <= bound elsewhere; -> the worst error / bound."""
    g = got.double()
    assert not torch.isnan(g).any(), what
    inf = torch.isneginf(ref)
    assert torch.equal(torch.isneginf(g), inf) and torch.isfinite(g[~inf]).all(), what
    err = (g - ref)[~inf].abs()
    over = err > bound[~inf]
    ratio = float((err / bound[~inf].clamp_min(1e-300)).max()) if err.numel() and float(err.max()) > 0 else 0.0
    assert not over.any(), (what, "worst error %.3e, %.2f of its bound" % (float(err.max()), ratio))
    return ratio


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_kernel_against_the_float64_restatement(name):
    c, (score, tok) = _run_case(name)
    ref_s, ref_t, bound_s, bound_t = R.bounds(R.logits_of(c), c["tgt"], c["seg_off"])
    rt = _within(tok, ref_t, bound_t, name + " tok_lp")
    rs = _within(score, ref_s, bound_s, name + " score")
    print("%s: worst error / bound: tok_lp %.3f, score %.3f (largest score bound %.3e)" % (name, rt, rs, float(bound_s.max())))
    if c["V"] == 1:
        assert torch.equal(tok, torch.zeros_like(tok)) and torch.equal(score, torch.zeros_like(score))
    off = c["seg_off"].tolist()
    for r in range(len(off) - 1):
        if off[r] == off[r + 1]:
            assert float(score[r]) == 0.0 and not math.copysign(1.0, float(score[r])) < 0, (name, r)


def test_no_rows_and_no_segments():
    """M = 0: every segment is empty and scores 0 (nothing is launched); R = 0 returns empty outputs."""
    score, tok = _run(np.zeros((0, 40), dtype=np.float32), 40, np.zeros(0, dtype=np.int64), [0, 0, 0, 0])
    assert torch.equal(score, torch.zeros(3)) and tok.numel() == 0
    score, tok = _run(np.zeros((0, 40), dtype=np.float32), 40, np.zeros(0, dtype=np.int64), [0])
    assert score.numel() == 0 and tok.numel() == 0


@pytest.mark.parametrize("V,ld", [(40, 40), (4364, 4416), (4365, 4365)])
def test_all_the_mass_on_the_target_scores_exactly_zero(V, ld):
    """A row of zeros with 200 at the target: exp(-200) is 0 in fp32, so tok_lp == 0.0 and score == 0.0 exactly."""
    M = 11
    g = np.random.default_rng(V)
    tgt = g.integers(0, V, size=M)
    tgt[0], tgt[1] = 0, V - 1
    buf = np.zeros((M, ld), dtype=np.float32)
    buf[np.arange(M), tgt] = 200.0
    score, tok = _run(buf, V, tgt, [0, 3, 11])
    assert torch.equal(tok, torch.zeros(M)) and torch.equal(score, torch.zeros(2))


def test_minus_infinity_and_targets_outside_the_vocabulary():
    """A target logit of -inf, a target of V and a target of -1: that row and its segment are -inf (never NaN, nothing read outside
    the row), every other row and segment keeps the plain run's bits.  Other -inf logits in a row are ordinary zeros of the sum."""
    c, (score0, tok0) = _run_case("v257")
    V, off = c["V"], c["seg_off"].tolist()                       # segments [0, 5) and [5, 17)
    buf, tgt = c["buf"].copy(), c["tgt"].copy()
    buf[2, tgt[2]] = -np.inf
    score, tok = _run(buf, V, tgt, off)
    assert float(tok[2]) == -math.inf and float(score[0]) == -math.inf
    keep = torch.arange(len(tgt)) != 2
    assert torch.equal(tok[keep], tok0[keep]) and torch.equal(score[1:], score0[1:])
    for bad in (V, -1, 2 ** 40):
        tgt = c["tgt"].copy()
        tgt[7] = bad
        score, tok = _run(c["buf"], V, tgt, off)
        keep = torch.arange(len(tgt)) != 7
        assert float(tok[7]) == -math.inf and float(score[1]) == -math.inf
        assert torch.equal(tok[keep], tok0[keep]) and torch.equal(score[:1], score0[:1])
    buf = c["buf"].copy()
    buf[3, :200] = -np.inf                                      # whole 16-byte groups and whole lanes of -inf; the target stays finite
    tgt = c["tgt"].copy()
    tgt[3] = 230
    ref_s, ref_t, bound_s, bound_t = R.bounds(buf[:, :V], tgt, off)
    score, tok = _run(buf, V, tgt, off)
    _within(tok, ref_t, bound_t, "-inf columns, tok_lp")
    _within(score, ref_s, bound_s, "-inf columns, score")


@pytest.mark.parametrize("name", ["v50_wide", "v4364", "v4365"])
def test_padding_and_unowned_rows_are_never_read(name):
    """NaN in the columns >= V of the buffer and in rows no segment owns (seg_off[0] = 2): bit for bit the plain run."""
    c = R.cases()[name]
    off = c["seg_off"].copy()
    off[0] = 2
    off = np.maximum(off, 2)
    plain_s, plain_t = _run(c["buf"], c["V"], c["tgt"], off)
    buf = c["buf"].copy()
    buf[:, c["V"]:] = np.nan
    buf[:2] = np.nan
    score, tok = _run(buf, c["V"], c["tgt"], off)
    assert torch.equal(score, plain_s) and torch.equal(tok[2:], plain_t[2:])
    assert torch.isfinite(score).all()


@pytest.mark.parametrize("name", ["v257", "v4364", "one_segment_300"])
def test_two_calls_give_the_same_bits(name):
    _, (s0, t0) = _run_case(name)
    _, (s1, t1) = _run_case(name)
    assert torch.equal(s0, s1) and torch.equal(t0, t1)


@pytest.mark.parametrize("name", ["v257", "v4365", "empty_segments"])
def test_permuting_the_segments_permutes_the_scores_bit_for_bit(name):
    """(v257: row stride 257, so a row's base alignment -- and with it the load arm -- changes with its position.)"""
    c, (score0, tok0) = _run_case(name)
    off = c["seg_off"].tolist()
    R_ = len(off) - 1
    perm = np.arange(R_)[::-1].copy()
    assert R_ > 1
    rows = np.concatenate([np.arange(off[r], off[r + 1]) for r in perm]).astype(np.int64)
    new_off = np.concatenate([[0], np.cumsum([off[r + 1] - off[r] for r in perm])])
    score, tok = _run(c["buf"][rows], c["V"], c["tgt"][rows], new_off)
    assert torch.equal(score, score0[torch.from_numpy(perm)]) and torch.equal(tok, tok0[torch.from_numpy(rows)])


@pytest.mark.parametrize("V", [261, 4365])
def test_the_scalar_arm_and_the_vector_arm_give_the_same_bits(V):
    """ld = V odd: three rows of four start off a 16-byte boundary and take the one-by-one loads; the same rows copied into a buffer
    whose rows are 16-byte aligned take the 16-byte loads.  Same tok_lp, bit for bit (and both within the bound)."""
    M = 13
    g = np.random.default_rng(V)
    x = (g.standard_normal((M, V)) * 3.0).astype(np.float32)
    tgt = g.integers(0, V, size=M)
    off = [0, 6, 13]
    s_sc, t_sc = _run(x, V, tgt, off)
    wide = np.full((M, (V + 7) // 4 * 4), np.nan, dtype=np.float32)
    wide[:, :V] = x
    s_ve, t_ve = _run(wide, V, tgt, off)
    assert torch.equal(t_sc, t_ve) and torch.equal(s_sc, s_ve)
    ref_s, ref_t, bound_s, bound_t = R.bounds(x, tgt, off)
    _within(t_sc, ref_t, bound_t, "arms, tok_lp")
    _within(s_sc, ref_s, bound_s, "arms, score")


def test_refusals():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    lg, tgt = torch.zeros(4, 8, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    tok, score = torch.empty(4, device=dev), torch.empty(1, device=dev)
    for ld, V in ((7, 8), (8, 0), (8, -1)):                       # ld < V; V = 0
        with pytest.raises(L.AsrHipError, match="invalid"):
            L.call("asr_seq_logprob", L.ptr(lg), ld, L.ptr(tgt), L.ptr(off), 1, 4, V, L.ptr(tok), L.ptr(score), L.stream())
    with pytest.raises(L.AsrHipError):
        L.call("asr_seq_logprob", L.ptr(lg), 8, L.ptr(tgt), L.ptr(off), -1, 4, 8, L.ptr(tok), L.ptr(score), L.stream())
    with pytest.raises(L.AsrHipError):
        ops.seq_logprob(lg.cpu(), tgt.cpu(), off.cpu())               # host tensors
    with pytest.raises(AssertionError):
        ops.seq_logprob(lg.bfloat16(), tgt, off)
    with pytest.raises(AssertionError):
        ops.seq_logprob(lg, tgt.int(), off)


# ------------------------------------------------------------------------------------------------ pinned to the executed reference
def _reference_case(golden_dir, precision, name="dec_d128"):
    """(the loader of tests/test_gpu_decode.py)"""
    from utils import constant
    from utils.functions import init_transformer_model
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    chars = constant.PAD_CHAR + constant.SOS_CHAR + constant.EOS_CHAR + "_'abcdefghijklmnopqrstuvwxyz "
    l2i = {c: i for i, c in enumerate(chars)}
    i2l = {i: c for c, i in l2i.items()}
    args = constant.parse(str(z["flags"]).split() + ["--precision", precision, "--cuda"])
    model = init_transformer_model(args, l2i, i2l)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}, strict=True)
    return z, model.cuda().eval()


def _check_scores(got, got_tok, ref, ref_tok, lens, per_logit, what):
    """got / ref: nested scores; lens: labels per hypothesis; the model bound of the module docstring.  -> worst error / bound."""
    worst = 0.0
    for b, (gs, rs) in enumerate(zip(got, ref)):
        assert len(gs) == len(rs), (what, b)
        for k, (g_, r_) in enumerate(zip(gs, rs)):
            n = lens[b][k]
            assert math.isfinite(g_), (what, b, k)
            worst = max(worst, abs(g_ - r_) / ((n + 1) * per_logit))
            if got_tok is not None:
                assert len(got_tok[b][k]) == n + 1 == len(ref_tok[b][k]), (what, b, k)
                worst = max(worst, max(abs(x - y) for x, y in zip(got_tok[b][k], ref_tok[b][k])) / per_logit)
    print("%s: worst error %.3f of the bound (%.3e per logit term)" % (what, worst, per_logit))
    assert worst <= 1.0, (what, worst)
    return worst


def test_score_hypotheses_reproduces_the_reference_on_its_own_greedy_logits(golden_dir, cli):
    """tests/golden/dec_d128.npz: the reference's greedy ids and the logits of all 300 greedy positions.  Prefixes of the ids of lengths
    0, 1, 7 and 40 of each of the 4 utterances as hypotheses: score_hypotheses equals the float64 sequence_scores of the reference's
    logits at positions 0 .. n, targets the next id and EOS last, within (n + 1) * 2 * 2e-4 * max |logit|."""
    from utils import constant
    z, model = _reference_case(golden_dir, "fp32")
    with torch.no_grad():
        enc, _ = model.encoder(model._features(torch.from_numpy(z["src"]).cuda()), torch.from_numpy(z["src_len"]))
    ids, ref_logits = z["greedy_ids"].astype(np.int64), z["greedy_logits"].astype(np.float64)
    lengths = (0, 1, 7, 40)
    hyps = [[ids[b, :n].tolist() for n in lengths] for b in range(4)]
    got, got_tok = model.decoder.score_hypotheses(enc, hyps, return_tokens=True)
    ref, ref_tok = [], []
    for b in range(4):
        ref.append([])
        ref_tok.append([])
        for n in lengths:
            s, t = R.sequence_scores(ref_logits[b, :n + 1], ids[b, :n].tolist() + [constant.EOS_TOKEN], [0, n + 1])
            ref[b].append(float(s[0]))
            ref_tok[b].append(t.tolist())
    per_logit = 2 * 2e-4 * float(np.abs(ref_logits).max())
    _check_scores(got, got_tok, ref, ref_tok, [list(lengths)] * 4, per_logit, "dec_d128 fp32 against the reference's logits")
    assert model.decoder.score_hypotheses(enc, hyps) == got          # without the token terms: the same floats


# ------------------------------------------------------------------------------------------------ model level
def _head_model(cli, extra=(), precision="fp32", gain=4.0):
    """The tiny model of tests/test_gpu_joint_ctc.py with a CTC head, built as tests/test_gpu_ctc_beam.py::_head_model does (head gain 4);
    --tgt-max-len 64: a CTC hypothesis may have as many labels as the utterance has frames (40), and each needs a decoder position."""
    import test_gpu_joint_ctc as J
    model = J._model(cli, ["--precision", precision, "--ctc-weight", "0.3", "--tgt-max-len", "64"] + list(extra)).eval()
    with torch.no_grad():
        model.ctc_linear.weight.mul_(gain)
    return model, J


def _encoded(model, J):
    src, lengths, tgt, _ = J._batch()
    with torch.no_grad():
        enc, _ = model.encoder(model._features(src), lengths)
    frames = model.ctc_frame_lengths(lengths, enc.shape[1])
    assert frames == [40, 30, 22]
    return src, lengths, tgt, enc, frames


def _nbest(model, enc, frames, W):
    """The kernel's hypotheses per utterance, best first: (label ids, CTC score)."""
    from asr_hip import ops
    with torch.no_grad():
        raw = ops.ctc_beam_search(model.ctc_logits(enc), torch.tensor(frames, dtype=torch.int32, device="cuda"), W, 0, W)
    return [[(raw["ids"][b, n, :raw["lengths"][b, n]].tolist(), float(raw["scores"][b, n])) for n in range(W) if raw["lengths"][b, n] >= 0]
            for b in range(len(frames))]


def _by_step_logits(dec, enc, hyps):
    """The plain way: _step_logits on the repeat_interleave'd encoder output, one padded row per hypothesis, and the float64 restatement
    on its logits.  -> (scores, token terms, max |logit|), nested like hyps."""
    from utils import constant
    ys, targets, lengths = R.pack(hyps)
    owner = [b for b, hs in enumerate(hyps) for _ in hs]
    L = max(lengths)
    pad = torch.tensor([y + [constant.PAD_TOKEN] * (L - len(y)) for y in ys], dtype=torch.int64, device=enc.device)
    with torch.no_grad():
        logits = dec._step_logits(pad, enc[torch.tensor(owner, device=enc.device)]).float().cpu().double()
    scores, toks, at = [], [], 0
    for hs in hyps:
        scores.append([])
        toks.append([])
        for _ in hs:
            s, t = R.sequence_scores(logits[at, :lengths[at]], targets[at], [0, lengths[at]])
            scores[-1].append(float(s[0]))
            toks[-1].append(t.tolist())
            at += 1
    return scores, toks, float(logits.abs().max())


def _lens(hyps):
    return [[len(y) for y in hs] for hs in hyps]


@pytest.mark.parametrize("W", [4, 1])
def test_folded_cross_attention_and_row_gather_change_nothing(cli, W):
    """score_hypotheses on the W hypotheses of ctc_beam_search against _step_logits on the repeat_interleave'd encoder output plus the
    float64 restatement: the (B, W L, D) view for cross-attention and the gather of the scored rows are a re-arrangement only."""
    model, J = _head_model(cli)
    _, _, _, enc, frames = _encoded(model, J)
    hyps = [[y for y, _ in hs] for hs in _nbest(model, enc, frames, W)]
    assert all(len(hs) == W for hs in hyps)
    _compare_with_step_logits(model, enc, hyps, W, "W %d" % W)


def test_folded_cross_attention_on_long_ragged_hypotheses(cli):
    """The tiny model's CTC hypotheses are a few labels long; the same comparison on planted label sequences of 0, 1, 9, 23 and 40
    labels per utterance (W 5: more positions than one attention tile, every utterance ragged, the longest in another slot each)."""
    model, J = _head_model(cli)
    _, _, _, enc, frames = _encoded(model, J)
    g = torch.Generator().manual_seed(17)
    lengths = [0, 1, 9, 23, 40]
    hyps = [[torch.randint(3, 12, (lengths[(k + b) % 5],), generator=g).tolist() for k in range(5)] for b in range(3)]
    _compare_with_step_logits(model, enc, hyps, 5, "planted lengths")


def _compare_with_step_logits(model, enc, hyps, W, what):
    owner = torch.tensor([b for b, hs in enumerate(hyps) for _ in hs], device=enc.device)
    assert torch.equal(enc[owner], enc.repeat_interleave(W, dim=0))          # what _by_step_logits feeds _step_logits
    ref, ref_tok, top = _by_step_logits(model.decoder, enc, hyps)
    got, got_tok = model.decoder.score_hypotheses(enc, hyps, return_tokens=True)
    _check_scores(got, got_tok, ref, ref_tok, _lens(hyps), 2 * 2e-4 * top, what + " against _step_logits on the repeated encoder output")


def test_scores_agree_with_the_kv_cached_step_path(cli):
    """The same tokens through DecoderKVCache.step, one position per call, log-softmax terms summed on the host: the two hypotheses of
    ctc_beam_search per utterance (a few labels each on this model) and a planted one of 25 labels."""
    from asr_hip.decode import DecoderKVCache
    from utils import constant
    model, J = _head_model(cli)
    _, _, _, enc, frames = _encoded(model, J)
    g = torch.Generator().manual_seed(23)
    hyps = [[y for y, _ in hs] + [torch.randint(3, 12, (25,), generator=g).tolist()] for hs in _nbest(model, enc, frames, 2)]
    ys, targets, lengths = R.pack(hyps)
    owner = [b for b, hs in enumerate(hyps) for _ in hs]
    L = max(lengths)
    pad = torch.tensor([y + [constant.PAD_TOKEN] * (L - len(y)) for y in ys], dtype=torch.int64, device="cuda")
    cache = DecoderKVCache(model.decoder, enc[torch.tensor(owner, device="cuda")], max_len=L)
    with torch.no_grad():
        logits = torch.stack([cache.step(pad[:, t].contiguous()).float().clone() for t in range(L)], dim=1).cpu().double()
    ref, ref_tok, at = [], [], 0
    for hs in hyps:
        ref.append([])
        ref_tok.append([])
        for _ in hs:
            s, t = R.sequence_scores(logits[at, :lengths[at]], targets[at], [0, lengths[at]])
            ref[-1].append(float(s[0]))
            ref_tok[-1].append(t.tolist())
            at += 1
    got, got_tok = model.decoder.score_hypotheses(enc, hyps, return_tokens=True)
    _check_scores(got, got_tok, ref, ref_tok, _lens(hyps), 2 * 2e-4 * float(logits.abs().max()), "against DecoderKVCache.step")


def test_nesting_chunking_and_a_hypothesis_alone(cli, monkeypatch):
    """An utterance with no hypothesis and one with only the empty hypothesis come back in the right nesting; a hypothesis scored alone
    and inside the batch agrees within the bound; with the cap on a pass's logits lowered so that every utterance is a chunk of its own
    the scores are those of one pass (within the bound: the shapes of the launches differ); a hypothesis longer than the positional
    encoding raises a ValueError that names the limit."""
    from models.asr.transformer import Decoder
    model, J = _head_model(cli)
    dec = model.decoder
    _, _, _, enc, frames = _encoded(model, J)
    found = [[y for y, _ in hs] for hs in _nbest(model, enc, frames, 4)]
    hyps = [found[0], [], [[]]]
    got, got_tok = dec.score_hypotheses(enc, hyps, return_tokens=True)
    assert [len(g) for g in got] == [4, 0, 1] and got_tok[1] == [] and len(got_tok[2][0]) == 1
    ref, ref_tok, top = _by_step_logits(dec, enc, hyps)
    per_logit = 2 * 2e-4 * top
    _check_scores(got, got_tok, ref, ref_tok, _lens(hyps), per_logit, "ragged nesting")
    assert dec.score_hypotheses(enc, [[], [], []]) == [[], [], []]
    alone = dec.score_hypotheses(enc[:1], [[found[0][2]]])
    _check_scores(alone, None, [[got[0][2]]], None, [[len(found[0][2])]], per_logit, "alone against inside the batch")
    whole = dec.score_hypotheses(enc, found)
    passes = []
    orig = Decoder._score_chunk

    def counting(self, enc_c, hyps_c, return_tokens):
        passes.append(len(hyps_c))
        return orig(self, enc_c, hyps_c, return_tokens)
    monkeypatch.setattr(Decoder, "_score_chunk", counting)
    assert dec.score_hypotheses(enc, found) == whole and passes == [3]
    del passes[:]
    rows = [sum(len(y) + 1 for y in hs) for hs in found]
    monkeypatch.setattr(Decoder, "RESCORE_LOGIT_BYTES", 4 * dec.num_trg_vocab * max(rows))      # no two utterances fit together
    chunked = dec.score_hypotheses(enc, found)
    assert passes == [1, 1, 1]
    _check_scores(chunked, None, whole, None, _lens(found), per_logit, "three chunks against one pass")
    del passes[:]
    monkeypatch.setattr(Decoder, "RESCORE_LOGIT_BYTES", 1)                                      # below one utterance: it still runs alone
    assert dec.score_hypotheses(enc, found) == chunked and passes == [1, 1, 1]
    limit = dec.positional_encoding.pe.shape[1] - 1
    assert limit == 63
    with pytest.raises(ValueError, match="63"):
        dec.score_hypotheses(enc, [[[3] * 64], [], []])
    assert len(dec.score_hypotheses(enc[:1], [[[3] * 63]])[0]) == 1


def _words(model, ids):
    from utils import constant
    s = "".join(model.id2label[t] for t in ids)
    for ch in (constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR):
        s = s.replace(ch, "")
    return len(s.replace("  ", " ").split())


@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_ranking_is_the_weighted_sum_then_rank_ended(cli, golden_dir, lam):
    """ctc_score from ops.ctc_beam_search, att_score from score_hypotheses (recorded from the call itself, so both sides hold the same
    device numbers), (1 - lambda) ctc + lambda att + sqrt(words) c_weight in Python, a stable sort: ctc_beam_search(rescoring_weight =
    lambda, nbest = W) returns exactly that order; with the fixture LM, the _rank_ended formula on the combined score."""
    from utils.lstm_utils import LM, calculate_lm_scores
    model, J = _head_model(cli)
    _, _, _, enc, frames = _encoded(model, J)
    W, c_weight, lm_weight = 6, 0.2, 0.3
    nbest = _nbest(model, enc, frames, W)
    seen = []
    orig = model.decoder.score_hypotheses

    def recording(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]
    model.decoder.score_hypotheses = recording
    try:
        strs, ids = model.ctc_beam_search(enc, frames, W, nbest=W, c_weight=c_weight, return_ids=True, rescoring_weight=lam)
        lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
        _, ids_lm = model.ctc_beam_search(enc, frames, W, nbest=W, c_weight=c_weight, lm=lm, lm_weight=lm_weight, return_ids=True,
                                          rescoring_weight=lam)
    finally:
        del model.decoder.score_hypotheses
    assert len(seen) == 2 and [len(a) for a in seen[0]] == [len(hs) for hs in nbest]      # ALL W survivors were rescored, in one call
    plain = model.ctc_beam_search(enc, frames, W, nbest=W, c_weight=c_weight, return_ids=True)[1]
    changed = 0
    for b, hs in enumerate(nbest):
        for att, want_ids, with_lm in ((seen[0][b], ids[b], False), (seen[1][b], ids_lm[b], True)):
            score = [R.combine(ctc, a, lam) for (_, ctc), a in zip(hs, att)]
            if with_lm:
                triples = calculate_lm_scores([y for y, _ in hs], lm, model.id2label)
                final = [s + lm_weight * (lm_score - 2 * oov) + math.sqrt(words) * c_weight for s, (lm_score, words, oov) in zip(score, triples)]
            else:
                final = [s + math.sqrt(_words(model, y)) * c_weight for s, (y, _) in zip(score, hs)]
            order = sorted(range(len(hs)), key=lambda i: -final[i])
            assert want_ids == [hs[i][0] for i in order], (b, with_lm, want_ids, final)
        assert strs[b] == ["".join(model.id2label[x] for x in row) for row in ids[b]]
        assert sorted(map(tuple, ids[b])) == sorted(map(tuple, plain[b]))
        changed += ids[b][0] != plain[b][0]
    print("lambda %.1f: utterances whose best hypothesis the decoder changed: %d of %d" % (lam, changed, len(nbest)))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        model.ctc_beam_search(enc, frames, W, rescoring_weight=1.2)


def test_weight_zero_makes_no_decoder_launch(cli, monkeypatch):
    """rescoring_weight = 0 (and the default): _step_logits and score_hypotheses are never called and the result is the plain search's."""
    from models.asr.transformer import Decoder
    model, J = _head_model(cli)
    src, lengths, tgt, enc, frames = _encoded(model, J)
    plain = model.ctc_beam_search(enc, frames, 4, nbest=4, c_weight=0.1, return_ids=True)
    plain_eval = model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, beam_nbest=2, c_weight=0.1)[1]

    def refuse(*a, **k):
        raise AssertionError("a decoder pass with rescoring off")
    monkeypatch.setattr(Decoder, "_step_logits", refuse)
    monkeypatch.setattr(Decoder, "score_hypotheses", refuse)
    assert model.ctc_beam_search(enc, frames, 4, nbest=4, c_weight=0.1, return_ids=True, rescoring_weight=0.0) == plain
    assert model.ctc_beam_search(enc, frames, 4, nbest=4, c_weight=0.1, return_ids=True) == plain
    assert model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, beam_nbest=2, c_weight=0.1, attention_rescoring_weight=0.0)[1] == plain_eval
    with pytest.raises(AssertionError, match="rescoring off"):
        model.ctc_beam_search(enc, frames, 4, rescoring_weight=0.5)


def test_bf16_scores_follow_the_fp32_model(cli):
    """The same weights in bf16: scores within (n + 1) * 2 * 3e-2 * max |logit| of the fp32 model's on the same hypotheses."""
    model, J = _head_model(cli)
    _, _, _, enc, frames = _encoded(model, J)
    hyps = [[y for y, _ in hs] for hs in _nbest(model, enc, frames, 4)]
    ref, ref_tok, top = _by_step_logits(model.decoder, enc, hyps)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    enc32 = enc.float().clone()
    model16, _ = _head_model(cli, precision="bf16", gain=1.0)
    model16.load_state_dict(state)
    got, got_tok = model16.decoder.score_hypotheses(enc32, hyps, return_tokens=True)
    _check_scores(got, got_tok, ref, ref_tok, _lens(hyps), 2 * 3e-2 * top, "bf16 against the fp32 model")


def test_low_rank_model_scores_and_matches_its_own_step_logits(cli):
    """--rank: no stacked K | V projection and no KV-cache kernels; the per-layer projection runs on the B utterances."""
    model, J = _head_model(cli, extra=["--rank", "8"])
    _, _, _, enc, frames = _encoded(model, J)
    assert not model.decoder._kv_cache_supported()
    hyps = [[y for y, _ in hs] for hs in _nbest(model, enc, frames, 3)]
    ref, ref_tok, top = _by_step_logits(model.decoder, enc, hyps)
    got, got_tok = model.decoder.score_hypotheses(enc, hyps, return_tokens=True)
    _check_scores(got, got_tok, ref, ref_tok, _lens(hyps), 2 * 2e-4 * top, "--rank 8 against its own _step_logits")


def test_evaluate_with_attention_rescoring(cli):
    """evaluate(ctc_beam=True, attention_rescoring_weight=0.3, align_source='hyp'): the best rescored hypothesis per utterance, aligned."""
    model, J = _head_model(cli)
    src, lengths, tgt, enc, frames = _encoded(model, J)
    best, best_ids = model.ctc_beam_search(enc, frames, 4, nbest=1, c_weight=0.1, return_ids=True, rescoring_weight=0.3)
    _, hyps, gold, ali = model.evaluate(src, lengths, tgt, ctc_beam=True, beam_width=4, beam_nbest=3, c_weight=0.1,
                                        attention_rescoring_weight=0.3, align_source="hyp")
    assert len(hyps) == len(gold) == 3 and hyps == [rows[0] for rows in best]
    for b in range(3):
        assert [x["id"] for x in ali[b]["labels"]] == best_ids[b][0]
    with pytest.raises(ValueError, match="--ctc-beam-search"):
        model.evaluate(src, lengths, tgt, attention_rescoring_weight=0.3)


def _loader():
    """Two utterances as the collate function delivers them: (inputs, targets, percentages, input sizes, target sizes)."""
    g = torch.Generator().manual_seed(3)
    src = torch.randn(2, 1, 161, 120, generator=g)
    src[1, :, :, 90:] = 0
    tgt = torch.tensor([[3, 4, 11, 5, 5, 6], [7, 11, 8, 0, 0, 0]])
    return [(src, tgt, torch.tensor([1.0, 0.75]), torch.tensor([120, 90], dtype=torch.int32), torch.tensor([6, 3], dtype=torch.int32))]


def test_test_py_decodes_with_attention_rescoring(cli, tmp_path):
    """test.py's evaluate() with --ctc-beam-search --attention-rescoring-weight 0.3 --align-out on a two-utterance loader: the weight
    reaches ctc_beam_search, and there is one parseable line per utterance whose labels are the best hypothesis' ids."""
    import test as test_mod
    import test_gpu_joint_ctc as J
    model, _ = _head_model(cli)
    out = tmp_path / "hyp.jsonl"
    flags = J.TINY + ["--precision", "fp32", "--ctc-weight", "0.3", "--tgt-max-len", "64", "--ctc-beam-search", "--beam-width", "4",
                      "--beam-nbest", "2", "--attention-rescoring-weight", "0.3"]
    args = cli(flags + ["--align-out", str(out), "--align-source", "hyp"])
    test_mod.check_ctc_decoding(args, model)
    seen = []
    orig = model.ctc_beam_search

    def recording(*a, **k):
        seen.append((k.get("rescoring_weight"), orig(*a, **k)))
        return seen[-1][1]
    model.ctc_beam_search = recording
    try:
        cer, wer = test_mod.evaluate(model, _loader())
    finally:
        del model.ctc_beam_search
    assert np.isfinite(cer) and np.isfinite(wer) and len(seen) == 1 and seen[0][0] == 0.3
    strs, ids = seen[0][1]
    recs = [json.loads(l) for l in out.read_text(encoding="utf-8").splitlines()]
    assert len(recs) == 2
    for b, r in enumerate(recs):
        assert [l["id"] for l in r["labels"]] == ids[b][0]
