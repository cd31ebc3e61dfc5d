"""The yardstick of MWER training over the CTC n-best, in float64 with torch only: the ONE definition the
kernels of csrc/mwer.hip, the host side and the documents share.

Per utterance b: gold g_b and n_b <= N distinct hypotheses with scores s_i = log p(y_i, EOS | x) and raw Levenshtein counts e_i.
    P_i     = softmax_i(s_i) over the n_b hypotheses (gold is not in the list); a score of -inf has P = 0
    risk_b  = sum_i P_i (e_i - mean_j e_j);     d risk_b / d s_i = P_i (e_i - sum_j P_j e_j);     n_b <= 1: risk 0, coefficients 0
    L_part  = m (1/B) sum_b risk_b + (1 - m)(1 - w) NLL,     NLL = - sum_b s_gold_b / sum_b (len(g_b) + 1)
    coef    = risk_scale * d risk / d s on hypotheses, -gold_scale on gold (risk_scale = m / B, gold_scale = (1 - m)(1 - w) / Ntok)
    dlogits[m, v] = c ([v == tgt[m]] - softmax(logits[m])[v]) for a row of a segment with coefficient c: autograd of
                    log_softmax(logits).gather(tgt) summed per segment (seq_scores).
Segments are laid out as asr_mwer_loss takes them: utt_off (B + 1), the FIRST segment of an utterance is its gold.

Bound of the GPU tests (the project's rule for row-wise kernels, tests/rowwise_reference.py): per tensor, |got - ref64| <= 4 x the largest
error of torch's own fp32 evaluation of the same formulas on the same input against float64, with a floor of one fp32 rounding of the
tensor's largest entry; a bf16 output adds one bf16 rounding elementwise (2**-8 |ref|)."""
import functools
import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
BF16_REL = 2.0 ** -8
B32_FACTOR = 4.0


# ------------------------------------------------------------------------------------------------ the loss
def mwer(score, err, utt_off, risk_scale, gold_scale, dtype=torch.float64):
    """-> dict(prob (R,), coef (R,), risk (B,), sums (2,), loss) in `dtype`, by the closed forms above, one utterance after the other."""
    s = torch.as_tensor(score).to(dtype)
    e = torch.as_tensor(err).to(dtype)
    off = [int(x) for x in utt_off]
    R, B = s.numel(), len(off) - 1
    prob, coef, risk = torch.zeros(R, dtype=dtype), torch.zeros(R, dtype=dtype), torch.zeros(B, dtype=dtype)
    gold_sum = torch.zeros((), dtype=dtype)
    for b in range(B):
        g, end = off[b], off[b + 1]
        if g >= end:
            continue
        coef[g] = -gold_scale
        gold_sum = gold_sum + s[g]
        h = slice(g + 1, end)
        n = end - g - 1
        sh, eh = s[h], e[h]
        if n == 0 or not bool(torch.isfinite(sh).any()):
            continue
        p = torch.softmax(sh, dim=0)
        prob[h] = p
        if n == 1:
            continue
        risk[b] = (p * (eh - eh.mean())).sum()
        coef[h] = risk_scale * p * (eh - (p * eh).sum())
    sums = torch.stack([risk.sum(), gold_sum])
    loss = risk_scale * sums[0] - (gold_scale * sums[1] if gold_scale != 0.0 else 0.0)
    return dict(prob=prob, coef=coef, risk=risk, sums=sums, loss=loss)


def mwer_autograd(score, err, utt_off, risk_scale, gold_scale, dtype=torch.float64):
    """The same loss as a differentiable function of the scores, with nothing but softmax arithmetic -> (loss, d loss / d score)."""
    s = torch.as_tensor(score).to(dtype).clone().requires_grad_()
    loss = mwer_loss_of(s, err, utt_off, risk_scale, gold_scale)
    loss.backward()
    return loss.detach(), s.grad.detach()


def mwer_loss_of(s, err, utt_off, risk_scale, gold_scale):
    """L_part of differentiable scores `s` (any float dtype, any device): plain torch softmax arithmetic."""
    e = torch.as_tensor(err).to(dtype=s.dtype, device=s.device)
    off = [int(x) for x in utt_off]
    loss = s.new_zeros(())
    for b in range(len(off) - 1):
        g, end = off[b], off[b + 1]
        if g >= end:
            continue
        loss = loss - gold_scale * s[g]
        if end - g - 1 >= 2:
            keep = torch.isfinite(s[g + 1:end].detach())
            sh, eh = s[g + 1:end], e[g + 1:end]
            if bool(keep.any()):
                p = torch.softmax(sh[keep], dim=0)
                loss = loss + risk_scale * (p * (eh[keep] - eh.mean())).sum()
    return loss


def total_loss(part, ctc, m, w):
    """L = L_part + (1 - m) w CTC."""
    return part + (1.0 - m) * w * ctc


# ------------------------------------------------------------------------------------------------ the row kernel
def seq_scores(logits, tgt, seg_off):
    """Differentiable segment scores: log_softmax(logits).gather(tgt) summed over the rows of each segment; rows whose target lies
    outside [0, V) contribute nothing here (the forward kernel scores them -inf, the backward gives them no gradient)."""
    M, V = logits.shape
    t = torch.as_tensor(tgt).long().to(logits.device)
    ok = (t >= 0) & (t < V)
    lp = torch.log_softmax(logits, dim=1).gather(1, t.clamp(0, V - 1).unsqueeze(1)).squeeze(1)
    lp = torch.where(ok, lp, torch.zeros_like(lp))
    off = [int(x) for x in seg_off]
    return torch.stack([lp[off[r]:off[r + 1]].sum() for r in range(len(off) - 1)]) if len(off) > 1 else lp.new_zeros((0,))


def dlogits(logits, tgt, seg_off, coef, grad_out=None, dtype=torch.float64):
    """(M, V) in `dtype`: autograd of grad_out * sum_r coef[r] * score[r] with respect to the logits."""
    lg = torch.as_tensor(np.asarray(logits)).to(dtype).clone().requires_grad_()
    c = torch.as_tensor(np.asarray(coef)).to(dtype)
    if lg.shape[0] == 0 or c.numel() == 0:
        return torch.zeros(lg.shape, dtype=dtype)
    go = 1.0 if grad_out is None else float(grad_out)
    (torch.as_tensor(go, dtype=dtype) * (c * seq_scores(lg, tgt, seg_off)).sum()).backward()
    return lg.grad.detach()


def bound32(ref, got32):
    """The per-tensor fp32 part of the bound: 4 x max(largest |torch fp32 - float64|, one rounding of the largest entry)."""
    ref = ref.double()
    if ref.numel() == 0:
        return 0.0
    fin = torch.isfinite(ref)
    err = float((got32.double() - ref)[fin].abs().max()) if bool(fin.any()) else 0.0
    top = float(ref[fin].abs().max()) if bool(fin.any()) else 0.0
    return B32_FACTOR * max(err, EPS32 * top)


def excess(got, ref, b32, bf16_stored=False):
    """max over elements of |got - ref| / bound (> 1: outside); a non-finite got where the reference is finite counts +inf; a bound of 0
    demands equality."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    bound = torch.full_like(ref, float(b32)) + (BF16_REL * ref.abs() if bf16_stored else 0.0)
    diff = (got - ref).abs()
    r = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, math.inf)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ the kernel cases
@functools.lru_cache(maxsize=None)
def bwd_case(V, M, R, seed=0):
    """logits (M, ld) fp32 whose first V columns count (the others hold 50.0), targets, R segments with an empty one (R = 5: the third;
    R = 1: a single segment), coefficients of both signs.  ld = V for V = 3 (rows at 12-byte steps: misaligned bases), V rounded up to 4
    plus 4 otherwise (a view of a wider buffer)."""
    g = np.random.default_rng(1000 * V + 10 * M + R + seed)
    ld = V if V in (1, 3) else (V + 3) // 4 * 4 + 4
    buf = np.full((M, ld), 50.0, dtype=np.float32)
    buf[:, :V] = (g.standard_normal((M, V)) * 3.0).astype(np.float32)
    tgt = g.integers(0, V, size=M).astype(np.int64)
    if R == 1:
        off = [0, M]
    else:
        assert R == 5
        c = sorted(int(x) for x in g.integers(0, M + 1, size=3))
        off = [0, c[0], c[1], c[1], c[2], M]                       # segment 2 is empty
    coef = (g.standard_normal(R) * 0.7).astype(np.float32)
    return dict(buf=buf, V=V, ld=ld, tgt=tgt, seg_off=np.asarray(off, dtype=np.int32), coef=coef)


def loss_case(ns, seed=0):
    """Utterances with ns[b] hypotheses each: scores around -20 a few nats apart, integer errors 0..9, gold scores around -15."""
    g = np.random.default_rng(77 + seed + sum((i + 1) * n for i, n in enumerate(ns)))
    score, err, off = [], [], [0]
    for n in ns:
        score += [float(-15.0 + g.standard_normal())] + [float(x) for x in (-20.0 + 3.0 * g.standard_normal(n))]
        err += [0.0] + [float(x) for x in g.integers(0, 10, size=n)]
        off.append(off[-1] + 1 + n)
    return np.asarray(score, dtype=np.float32), np.asarray(err, dtype=np.float32), np.asarray(off, dtype=np.int32)


def words(ids, space):
    """The runs of ids between the space label's id, as tuples (--mwer-unit word)."""
    out, cur = [], []
    for t in ids:
        if t == space:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(t)
    return out + ([tuple(cur)] if cur else [])
