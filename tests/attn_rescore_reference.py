"""The yardstick of attention rescoring, in float64 with torch / numpy only: per-token and per-sequence
log-probabilities of a batch of logits rows (what csrc/seq_logprob.hip computes), the teacher-forced packing of hypotheses and the
convex combination of the two scores; and the inputs of the kernel cases, shared by tests/test_attn_rescore_host.py (which shows the
bound on them is neither vacuous nor broken by a correct fp32 implementation) and tests/test_gpu_attn_rescore.py."""
import functools
import math

import numpy as np
import torch

PAD, SOS, EOS = 0, 1, 2
EPS32 = float(np.finfo(np.float32).eps)


def token_logprobs(logits, tgt):
    """logits (M, V) -> float64 (M,): log_softmax(logits)[m, tgt[m]]; -inf for a target outside [0, V)."""
    lg = torch.as_tensor(np.asarray(logits)).double()
    t = torch.as_tensor(np.asarray(tgt)).long()
    M, V = lg.shape
    out = torch.full((M,), -math.inf, dtype=torch.float64)
    ok = (t >= 0) & (t < V)
    if M and bool(ok.any()):
        lp = torch.log_softmax(lg, dim=1)
        out[ok] = lp[ok].gather(1, t[ok].unsqueeze(1)).squeeze(1)
    return out


def sequence_scores(logits, tgt, seg_off):
    """-> (float64 (R,) sums of token_logprobs over rows seg_off[r] .. seg_off[r+1]-1 (an empty segment 0), the token terms)."""
    tok = token_logprobs(logits, tgt)
    off = [int(x) for x in seg_off]
    score = torch.zeros(len(off) - 1, dtype=torch.float64)
    for r in range(len(off) - 1):
        if off[r + 1] > off[r]:
            score[r] = tok[off[r]:off[r + 1]].sum()
    return score, tok


def pack(hyps):
    """hyps: one list per utterance of label-id lists -> (ys, targets, lengths), one entry per hypothesis in order: decoder input
    [SOS] + y, targets y + [EOS], n + 1 rows.  The empty hypothesis: [SOS] / [EOS], length 1; an utterance without one adds nothing."""
    ys, targets, lengths = [], [], []
    for hs in hyps:
        for y in hs:
            y = [int(t) for t in y]
            ys.append([SOS] + y)
            targets.append(y + [EOS])
            lengths.append(len(y) + 1)
    return ys, targets, lengths


def combine(ctc, att, lam):
    """(1 - lam) * ctc + lam * att, in Python floats: the expression Transformer.ctc_beam_search evaluates."""
    return (1.0 - lam) * ctc + lam * att


# ------------------------------------------------------------------------------------------------ torch's own fp32, and the bound
def torch32(logits, tgt, seg_off):
    """torch's fp32 CPU log_softmax + gather + sum on the same input -> (score, tok) as float64 tensors (out-of-range targets: -inf)."""
    lg = torch.as_tensor(np.asarray(logits)).float()
    t = torch.as_tensor(np.asarray(tgt)).long()
    M, V = lg.shape
    tok = torch.full((M,), -math.inf, dtype=torch.float32)
    ok = (t >= 0) & (t < V)
    if M and bool(ok.any()):
        tok[ok] = torch.log_softmax(lg, dim=1)[ok].gather(1, t[ok].unsqueeze(1)).squeeze(1)
    off = [int(x) for x in seg_off]
    score = torch.zeros(len(off) - 1, dtype=torch.float32)
    for r in range(len(off) - 1):
        if off[r + 1] > off[r]:
            score[r] = tok[off[r]:off[r + 1]].sum()
    return score.double(), tok.double()


def bounds(logits, tgt, seg_off):
    """-> (ref score, ref tok, score bound, tok bound): |got - ref64| <= 4 * max(|torch32 - ref64|, eps32 * sum |tok_lp|) per segment
    -- four times torch's own fp32 error, with a floor of one rounding per addition -- and the same per row.  Entries whose reference
    is -inf have bound 0: they must be -inf exactly."""
    score, tok = sequence_scores(logits, tgt, seg_off)
    s32, t32 = torch32(logits, tgt, seg_off)
    fin_t, fin_s = torch.isfinite(tok), torch.isfinite(score)
    tok_b = torch.zeros_like(tok)
    tok_b[fin_t] = 4.0 * torch.maximum((t32 - tok)[fin_t].abs(), EPS32 * tok[fin_t].abs())
    off = [int(x) for x in seg_off]
    mass = torch.tensor([float(tok[off[r]:off[r + 1]].abs().sum()) if fin_s[r] else 0.0 for r in range(len(off) - 1)], dtype=torch.float64)
    score_b = torch.zeros_like(score)
    score_b[fin_s] = 4.0 * torch.maximum((s32 - score)[fin_s].abs(), EPS32 * mass[fin_s])
    return score, tok, score_b, tok_b


# ------------------------------------------------------------------------------------------------ the kernel cases
def _case(V, ld, seg_off, seed, scale=3.0, kind="normal"):
    """A buffer (M, ld) fp32 whose first V columns are logits (the others hold 50.0), targets and offsets."""
    g = np.random.default_rng(seed)
    M = int(seg_off[-1])
    buf = np.full((M, ld), 50.0, dtype=np.float32)
    if kind == "normal":
        buf[:, :V] = (g.standard_normal((M, V)) * scale).astype(np.float32)
        tgt = g.integers(0, V, size=M)
    else:                        # planted: +-80 with the row maximum in the LAST column (the online pass rescales to the very end)
        x = g.uniform(-80.0, 79.0, size=(M, V)).astype(np.float32)
        x[:, V - 1] = 80.0
        buf[:, :V] = x
        tgt = np.full(M, V - 1) if kind == "target_is_max" else x.argmin(axis=1)
    return dict(buf=buf, V=V, tgt=tgt.astype(np.int64), seg_off=np.asarray(seg_off, dtype=np.int32))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(buf (M, ld) fp32, V, tgt (M,) int64, seg_off (R+1,) int32).  The smallest shapes at which each branch of the kernel
    can go wrong: V = 1; ld = V = 3 (rows at 12-byte steps: the scalar arm on three rows of four); V 40 and 50 below one wave's 256
    columns of 16-byte loads; V 257 (one 16-byte round and a one-column tail); V 4364 / 4365 in the 4416-wide buffer of the benchmark
    vocabulary (17 rounds, without and with a tail); one segment of 300 rows; empty segments first, in the middle and last; more rows
    than one workgroup's 8 everywhere but v1."""
    return {
        "v1": _case(1, 1, [0, 2, 5], 1),
        "v3_ld3": _case(3, 3, [0, 4, 9, 13], 2),
        "v40": _case(40, 40, [0, 7, 8, 20], 3),
        "v50_wide": _case(50, 56, [0, 11, 19], 4),
        "v257": _case(257, 257, [0, 5, 17], 5),
        "v4364": _case(4364, 4416, [0, 9, 10, 24], 6),
        "v4365": _case(4365, 4416, [0, 9, 10, 24], 7),
        "one_segment_300": _case(40, 40, [0, 300], 8),
        "empty_segments": _case(40, 40, [0, 0, 5, 5, 5, 12, 12], 9),
        "max_last_target_max_257": _case(257, 260, [0, 6, 13], 10, kind="target_is_max"),
        "max_last_target_min_257": _case(257, 260, [0, 6, 13], 11, kind="target_is_min"),
        "max_last_target_max_4364": _case(4364, 4416, [0, 4, 9], 12, kind="target_is_max"),
        "max_last_target_min_4364": _case(4364, 4416, [0, 4, 9], 13, kind="target_is_min"),
    }


def logits_of(c):
    return c["buf"][:, :c["V"]]
