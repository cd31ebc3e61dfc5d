"""The yardstick of knowledge distillation from a teacher's logits, in float64 with torch only: the ONE definition
csrc/distill.hip, the model step and the documents share.

Row m is LIVE iff gold[m] != pad_id; n = the number of live rows.  With temperature tau, pS = softmax(s / tau), pT = softmax(t / tau):
    kd_m      = tau^2 sum_v pT_v (log pT_v - log pS_v)                                         (Hinton et al. 2015: tau^2 KL(pT || pS))
    ce_m      = the label-smoothed row loss of tests/rowwise_reference.py (ce_reference: smoothing mass eps / V on every class)
    sums      = [sum ce_m, n, #(argmax == gold), sum kd_m] over live rows
    loss      = (ce_scale sums[0] + kd_scale sums[3]) / n
    dlogits   = (grad_out / n) [ce_scale (softmax(s)_v sum_q - q_v) + kd_scale tau (pS_v - pT_v)] on live rows, 0 on dead ones
    row_stats = [lse(s), lse(s / tau), lse(t / tau), kd_m], zeros on dead rows.
Dead rows' logits never enter: they are replaced by zeros before any arithmetic, so a NaN there is harmless here too.

Bound of the GPU tests (the project's rule for row-wise kernels, tests/rowwise_reference.py): per tensor, |got - ref64| <= 4 x the largest
error of torch's own fp32 evaluation of the same formulas on the same input against float64, with a floor of one fp32 rounding of the
tensor's largest entry; a bf16 output adds one bf16 rounding elementwise (2**-8 |ref|).  The fp32 evaluation of the gradient is taken both
from exp(log_softmax) and from exp(z - lse) with the fp32 evaluation's own lse stored in fp32 -- the backward kernel's interface, as for
asr_ce_bwd (rowwise_reference.ce_case_reference).  A sum of row values (sums[0], sums[3], and the loss made of them) takes as the fp32
evaluation's error the larger of the sum's own and the sum of its rows' absolute errors, as ce_case_reference takes the CE loss sum's."""
import functools

import numpy as np
import torch

import rowwise_reference as RW
from mwer_reference import EPS32, bound32, excess  # noqa: F401  (the rule's two helpers, shared with the MWER tests)

PAD = 0
F64, F32 = torch.float64, torch.float32


def distill(student, teacher, gold, smoothing, pad_id, tau, ce_scale, kd_scale, grad_out=1.0, with_ce=True, dt=F64, stored_lse=False):
    """-> dict(row_stats (M,4), kd (M,), ce (M,), argmax, sums (4,), loss, dlogits (M,V), live) in `dt`.  with_ce=False: the CE
    statistics are 0 and gold only marks the live rows.  stored_lse: the gradient's probabilities as exp(z - lse) with lse rounded to
    fp32 first (what a backward that reads the forward's fp32 row statistics computes)."""
    s, t = torch.as_tensor(student).to(dt), torch.as_tensor(teacher).to(dt)
    gold = torch.as_tensor(gold).long()
    M, V = s.shape
    live = gold != pad_id
    s = torch.where(live[:, None], s, torch.zeros_like(s))
    t = torch.where(live[:, None], t, torch.zeros_like(t))
    n = float(live.sum())
    zs, zt = s / tau, t / tau
    lse_s, lse_zs, lse_zt = torch.logsumexp(s, 1), torch.logsumexp(zs, 1), torch.logsumexp(zt, 1)
    lps, lpt = torch.log_softmax(zs, 1), torch.log_softmax(zt, 1)
    kd = (tau * tau) * (torch.exp(lpt) * (lpt - lps)).sum(1) * live.to(dt)
    if stored_lse:
        pS = torch.exp(zs - lse_zs.float().to(dt)[:, None])
        pT = torch.exp(zt - lse_zt.float().to(dt)[:, None])
    else:
        pS, pT = torch.exp(lps), torch.exp(lpt)
    dl = (grad_out / n) * kd_scale * tau * (pS - pT) * live.to(dt)[:, None]
    ce = torch.zeros(M, dtype=dt)
    am = torch.zeros(M, dtype=torch.int64)
    correct = 0.0
    if with_ce:
        g = torch.where(live, gold, torch.full_like(gold, pad_id))
        r = RW.ce_reference(s, g, smoothing, pad_id, grad_out, dt=dt, lse_in=lse_s.float() if stored_lse else None)
        ce, correct = r["loss_rows"], r["sums"][2]
        am = torch.where(live, r["argmax"], torch.zeros_like(r["argmax"]))
        dl = dl + ce_scale * r["dlogits"]
    else:
        ce_scale = 0.0
    sums = torch.stack([ce.sum(), torch.tensor(n, dtype=dt), torch.tensor(float(correct), dtype=dt), kd.sum()])
    loss = (ce_scale * sums[0] + kd_scale * sums[3]) / n
    z = torch.zeros(M, dtype=dt)
    stats = torch.stack([torch.where(live, lse_s, z) if with_ce else z, torch.where(live, lse_zs, z), torch.where(live, lse_zt, z), kd], 1)
    return dict(row_stats=stats, kd=kd, ce=ce, argmax=am, sums=sums, loss=loss, dlogits=dl, live=live)


def loss_of(s, t, gold, smoothing, pad_id, tau, ce_scale, kd_scale, with_ce=True):
    """The same loss as a differentiable function of the student logits `s` (any shape (..., V), any float dtype, any device), with nothing
    but log_softmax arithmetic -> (loss, sums (4,) detached fp32, argmax (M,)): what F_.DistillFn returns, for the model tests."""
    V = s.shape[-1]
    s2, t2, g = s.reshape(-1, V), t.detach().reshape(-1, V).to(s.dtype), gold.reshape(-1)
    live = g != pad_id
    sl, tl, gl = s2[live], t2[live], g[live]
    n = float(live.sum())
    lps, lpt = torch.log_softmax(sl / tau, 1), torch.log_softmax(tl / tau, 1)
    kd = (tau * tau) * (torch.exp(lpt) * (lpt - lps)).sum()
    ce, correct = s2.new_zeros(()), 0.0
    if with_ce:
        lp = torch.log_softmax(sl, 1)
        lpg = lp.gather(1, gl[:, None])[:, 0]
        ce = -((1.0 - smoothing) * lpg + (smoothing / V) * (lp.sum(1) - lpg)).sum() if smoothing > 0 else -lpg.sum()
        correct = float((sl.detach().argmax(1) == gl).sum())
    else:
        ce_scale = 0.0
    loss = (ce_scale * ce + kd_scale * kd) / n
    sums = torch.stack([ce.detach().float(), ce.new_tensor(n).float(), ce.new_tensor(correct).float(), kd.detach().float()])
    return loss, sums, s2.detach().argmax(1)


def kd_autograd(student, teacher, gold, pad_id, tau):
    """(KD, d KD / d student) in float64 by autograd of F.kl_div on F.log_softmax: KD = tau^2 / n * sum over live rows of KL(pT || pS)."""
    import torch.nn.functional as F
    s = torch.as_tensor(student).double().clone().requires_grad_()
    t = torch.as_tensor(teacher).double()
    live = torch.as_tensor(gold).long() != pad_id
    kl = F.kl_div(F.log_softmax(s[live] / tau, 1), F.softmax(t[live] / tau, 1), reduction="sum")
    kd = tau * tau * kl / float(live.sum())
    kd.backward()
    return kd.detach(), s.grad.detach()


def bounds(student, teacher, gold, smoothing, pad_id, tau, ce_scale, kd_scale, grad_out, with_ce, ref):
    """{tensor: b32} of a case: bound32 of torch's fp32 evaluation against `ref` (the float64 evaluation), the gradient both ways."""
    e = distill(student, teacher, gold, smoothing, pad_id, tau, ce_scale, kd_scale, grad_out, with_ce, dt=F32)
    e2 = distill(student, teacher, gold, smoothing, pad_id, tau, ce_scale, kd_scale, grad_out, with_ce, dt=F32, stored_lse=True)
    b = {k: bound32(ref[k], e[k]) for k in ("kd", "dlogits")}
    b["loss"] = bound32(ref["loss"].reshape(1), e["loss"].reshape(1))
    b["sums"] = [bound32(ref["sums"][i:i + 1], e["sums"][i:i + 1]) for i in range(4)]          # each sum is its own quantity
    # a sum of row values: the fp32 evaluation's error is taken as the larger of the sum's own and the sum of its rows' absolute errors,
    # as rowwise_reference.ce_case_reference takes the CE loss sum's (a handful of row errors that happen to cancel in torch's order
    # of summation say nothing about another order); the loss is the weighted mean of the two sums
    rows = {0: float((e["ce"].double() - ref["ce"]).abs().sum()), 3: float((e["kd"].double() - ref["kd"]).abs().sum())}
    for i, r in rows.items():
        b["sums"][i] = max(b["sums"][i], 4.0 * r)
    n = float(ref["sums"][1])
    b["loss"] = max(b["loss"], 4.0 * ((ce_scale if with_ce else 0.0) * rows[0] + kd_scale * rows[3]) / n)
    b["dlogits"] = max(b["dlogits"], bound32(ref["dlogits"], e2["dlogits"]))
    return b


# ------------------------------------------------------------------------------------------------ the kernel cases
@functools.lru_cache(maxsize=None)
def case(M, V, seed=0):
    """student / teacher (M, ld) fp32 whose first V columns count (the others hold 50.0), gold with dead rows (every third row from row
    1; M = 1: the row is live).  ld = V rounded up to 4 plus 4: 16-byte-aligned row bases, a view of a wider buffer.  The teacher is
    the student plus noise of the student's own scale: the KL is neither tiny nor huge."""
    g = np.random.default_rng(100000 * seed + 1000 * V + M)
    ld = (V + 3) // 4 * 4 + 4
    sb = np.full((M, ld), 50.0, dtype=np.float32)
    tb = np.full((M, ld), 50.0, dtype=np.float32)
    sb[:, :V] = (g.standard_normal((M, V)) * 3.0).astype(np.float32)
    tb[:, :V] = (sb[:, :V] + g.standard_normal((M, V)) * 2.0).astype(np.float32)
    gold = g.integers(1, max(2, V), size=M).astype(np.int64)
    gold[1::3] = PAD
    if M > 2:
        gold[2] = int(np.argmax(sb[2, :V])) or 1          # a correct row (unless its arg-max is the PAD column)
    return dict(s=sb, t=tb, gold=gold, V=V, ld=ld, M=M)
