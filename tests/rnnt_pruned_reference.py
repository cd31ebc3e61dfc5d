"""Float64 restatement of pruned transducer training (csrc/rnnt_pruned.hip) in plain torch on the CPU: the simple
joiner's loss and gradient, the band rule, the banded loss and gradient, the banded joint and its two reductions.  Every function takes
a dtype so the SAME formula can be run in fp32 (the tolerance rule of tests/rnnt_reference.py: bound32, excess).

Notation (tests/rnnt_reference.py): blank = 0 = PAD, utterance b has T_b frames and labels y_1 .. y_{U_b}, U1 = Umax + 1.
  simple:  N(t,u) = (ma[t] + ml[u]) + log(max(dot(t,u), FLT_MIN)),  dot = sum_v exp(am - ma) exp(lm - ml),  ma / ml the row maxima
           blank(t,u) = (am[t,0] + lm[u,0]) - N,  label(t,u) = (am[t,y_{u+1}] + lm[u,y_{u+1}]) - N,  then the lattice of rnnt_reference
           G = (gb + gl) / max(dot, FLT_MIN);  d nll / d am[t,v] = Ea[t,v] sum_u G(t,u) El[u,v] - [v = 0] sum_u gb - sum_{u: y_{u+1} = v} gl
  band:    W = min(S, U1); U_b + 1 <= W: s = 0.  Else fin = U_b + 1 - W, raw(t) = the lowest a in 0..fin maximising sum_{u=a}^{a+W-1}
           occ(t,u) (a direct float64 sum in ascending u from +0.0); s(0) = 0, s(t) = min(max(raw(t), s(t-1)), s(t-1) + W - 1);
           s(T_b-1) = fin; for t = T_b-2 .. 0: s(t) = max(s(t), s(t+1) - (W-1)).  Frames t >= T_b: 0.
  pruned:  logits (B,T,W,V), row (b,t,w) = lattice cell (t, s(t) + w); blank = label = -inf for every node outside the band."""
import itertools
import math

import numpy as np
import torch

import rnnt_reference as R
from rnnt_reference import BLANK, NEG, bound32, excess  # noqa: F401

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def _clamp(v, lo, hi):
    return max(lo, min(hi, int(v)))


# ------------------------------------------------------------------------------------------------ the simple loss
def simple_loss_and_grad(am, lm, targets, frames, lengths, V=None, blank=BLANK, dtype=torch.float64, grad_out=1.0):
    """am (B,T,>=V), lm (B,U1,>=V) (only live rows and the first V columns are read) -> dict(nll (B,), loss, gb / gl / dot (B,T,U1), dam
    (B,T,V), dlm (B,U1,V) = grad_out * d loss / d am, d lm), all in `dtype`."""
    B, T = am.shape[:2]
    U1 = lm.shape[1]
    V = am.shape[2] if V is None else V
    nll = torch.zeros(B, dtype=dtype)
    gb_all, gl_all, dot_all = (torch.zeros((B, T, U1), dtype=dtype) for _ in range(3))
    dam, dlm = torch.zeros((B, T, V), dtype=dtype), torch.zeros((B, U1, V), dtype=dtype)
    for b in range(B):
        Tb, Ub = _clamp(frames[b], 0, T), _clamp(lengths[b], 0, U1 - 1)
        y = [int(v) for v in targets[b][:Ub]]
        if not R.valid(y, Tb, V, blank):
            nll[b] = math.inf
            continue
        a = torch.as_tensor(am[b, :Tb, :V]).to(dtype)
        l = torch.as_tensor(lm[b, :Ub + 1, :V]).to(dtype)
        ma, ml = a.max(1).values, l.max(1).values
        Ea, El = torch.exp(a - ma[:, None]), torch.exp(l - ml[:, None])
        dot = Ea @ El.t()
        n = (ma[:, None] + ml[None, :]) + torch.log(dot.clamp_min(FLT_MIN))
        lpb = (a[:, None, blank] + l[None, :, blank]) - n
        yi = torch.tensor(y, dtype=torch.int64)
        lpl = (a[:, yi] + l[torch.arange(Ub), yi][None, :]) - n[:, :Ub] if Ub else n.new_zeros((Tb, 0))
        alpha, beta, logz = R.lattice(lpb, lpl)
        nll[b] = -logz
        dot_all[b, :Tb, :Ub + 1] = dot
        if not math.isfinite(float(logz)):
            continue
        bnext = torch.full((Tb, Ub + 1), NEG, dtype=dtype)
        bnext[:Tb - 1] = beta[1:]
        bnext[Tb - 1, Ub] = 0.0
        gb = torch.exp(alpha + lpb + bnext - logz)
        gl = torch.zeros((Tb, Ub + 1), dtype=dtype)
        if Ub:
            gl[:, :Ub] = torch.exp(alpha[:, :Ub] + lpl + beta[:, 1:] - logz)
        gb_all[b, :Tb, :Ub + 1], gl_all[b, :Tb, :Ub + 1] = gb, gl
        G = (gb + gl) / dot.clamp_min(FLT_MIN)
        c = torch.tensor(grad_out, dtype=dtype) / torch.tensor(float(B * max(Ub, 1)), dtype=dtype)
        da = c * (Ea * (G @ El).clamp_max(FLT_MAX))           # the kernel's guard past the stated limit (0 * inf)
        dl = c * (El * (G.t() @ Ea).clamp_max(FLT_MAX))
        da[:, blank] -= c * gb.sum(1)
        dl[:, blank] -= c * gb.sum(0)
        for u in range(Ub):                                  # one owner, u order: labels may repeat
            da[:, y[u]] -= c * gl[:, u]
            dl[u, y[u]] -= c * gl[:, u].sum()
        dam[b, :Tb], dlm[b, :Ub + 1] = da, dl
    den = torch.tensor([float(max(1, _clamp(n_, 0, U1 - 1))) for n_ in lengths], dtype=dtype)
    return dict(nll=nll, loss=(nll / den).sum() / B, gb=gb_all, gl=gl_all, dot=dot_all, dam=dam, dlm=dlm)


def materialised(am, lm):
    """The joint logits the simple joiner stands for: am[:,:,None] + lm[:,None] (B,T,U1,V)."""
    return am[:, :, None, :] + lm[:, None, :, :]


# ------------------------------------------------------------------------------------------------ the band
def prune_ranges(occ, frames, lengths, S):
    """occ (B,T,U1) node occupancies (any dtype; each is widened to float64 and the window sums are direct float64 sums) -> s_begin (B,T)
    int32."""
    B, T, U1 = occ.shape
    W = min(int(S), U1)
    o = occ.double().tolist()
    s_all = torch.zeros((B, T), dtype=torch.int32)
    for b in range(B):
        Tb, Ub = _clamp(frames[b], 0, T), _clamp(lengths[b], 0, U1 - 1)
        fin = Ub + 1 - W
        if fin <= 0 or Tb == 0:
            continue
        s = []
        for t in range(Tb):
            best, top = 0, -1.0
            for a in range(fin + 1):
                tot = 0.0
                for u in range(a, a + W):
                    tot += o[b][t][u]
                if tot > top:
                    best, top = a, tot
            s.append(best)
        s[0] = 0
        for t in range(1, Tb):
            s[t] = min(max(s[t], s[t - 1]), s[t - 1] + W - 1)
        s[Tb - 1] = fin
        for t in range(Tb - 2, -1, -1):
            s[t] = max(s[t], s[t + 1] - (W - 1))
        s_all[b, :Tb] = torch.tensor(s, dtype=torch.int32)
    return s_all


def band_properties(s, Tb, Ub, W):
    """s(0) = 0, s(T_b-1) = fin and 0 <= s(t+1) - s(t) <= W - 1 (for an utterance with U_b + 1 > W)."""
    s = [int(v) for v in s[:Tb]]
    return s[0] == 0 and s[-1] == Ub + 1 - W and all(0 <= s[i + 1] - s[i] <= W - 1 for i in range(Tb - 1))


def feasible(Tb, Ub, W):
    return Ub + 1 <= W or (Tb - 1) * (W - 1) >= Ub + 1 - W


# ------------------------------------------------------------------------------------------------ the banded loss
def pruned_loss_and_grad(logits, targets, frames, lengths, s_begin, Umax, V=None, blank=BLANK, dtype=torch.float64, grad_out=1.0):
    """logits (B,T,W,>=V) whose row (b,t,w) is cell (t, s_begin[b,t] + w) -> dict(nll (B,), loss, dlogits (B,T,W,V)) in `dtype`."""
    B, T, W = logits.shape[:3]
    V = logits.shape[3] if V is None else V
    U1 = Umax + 1
    nll = torch.zeros(B, dtype=dtype)
    dl = torch.zeros((B, T, W, V), dtype=dtype)
    for b in range(B):
        Tb, Ub = _clamp(frames[b], 0, T), _clamp(lengths[b], 0, Umax)
        y = [int(v) for v in targets[b][:Ub]]
        if not R.valid(y, Tb, V, blank):
            nll[b] = math.inf
            continue
        s = [_clamp(s_begin[b, t], 0, U1 - W) for t in range(Tb)]
        lpb = torch.full((Tb, Ub + 1), NEG, dtype=dtype)
        lpl = torch.full((Tb, Ub), NEG, dtype=dtype)
        lps = {}
        for t in range(Tb):
            for w in range(W):
                u = s[t] + w
                if u > Ub:
                    continue
                lp = torch.log_softmax(torch.as_tensor(logits[b, t, w, :V]).to(dtype), -1)
                lps[(t, w)] = lp
                lpb[t, u] = lp[blank]
                if u < Ub:
                    lpl[t, u] = lp[y[u]]
        alpha, beta, logz = R.lattice(lpb, lpl)
        nll[b] = -logz
        if not math.isfinite(float(logz)):
            continue
        c = torch.tensor(grad_out, dtype=dtype) / torch.tensor(float(B * max(Ub, 1)), dtype=dtype)
        for (t, w), lp in lps.items():
            u = s[t] + w
            bnext = beta[t + 1, u] if t + 1 < Tb else (lp.new_zeros(()) if u == Ub else lp.new_full((), NEG))
            gb = torch.exp(alpha[t, u] + lpb[t, u] + bnext - logz)
            gl = torch.exp(alpha[t, u] + lpl[t, u] + beta[t, u + 1] - logz) if u < Ub else lp.new_zeros(())
            g = (gb + gl) * torch.exp(lp)
            g[blank] -= gb
            if u < Ub:
                g[y[u]] -= gl
            dl[b, t, w] = c * g
    den = torch.tensor([float(max(1, _clamp(n_, 0, Umax))) for n_ in lengths], dtype=dtype)
    return dict(nll=nll, loss=(nll / den).sum() / B, dlogits=dl)


def gather_band(full, s_begin, W):
    """The band rows of full logits (B,T,U1,...) -> (B,T,W,...)."""
    B, T, U1 = full.shape[:3]
    out = full.new_zeros((B, T, W) + tuple(full.shape[3:]))
    for b in range(B):
        for t in range(T):
            a = _clamp(s_begin[b, t], 0, U1 - W)
            out[b, t] = full[b, t, a:a + W]
    return out


def nll_band_brute_force(x, y, s, W, blank=BLANK):
    """-log of the sum over every alignment of ONE utterance (x (T,U+1,V) full logits) that visits only nodes inside the band
    s(t) <= u < s(t) + W; +inf when there is none."""
    T, U1, _ = x.shape
    U = U1 - 1
    lp = torch.log_softmax(x.double(), -1)
    inside = lambda t, u: s[t] <= u < s[t] + W  # noqa: E731
    total = []
    for labels_at in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        acc, ok = 0.0, inside(0, 0)
        for i in range(T - 1 + U):
            if not ok:
                break
            if i in labels_at:
                acc += float(lp[t, u, y[u]])
                u += 1
            else:
                acc += float(lp[t, u, blank])
                t += 1
            ok = inside(t, u)
        if ok:
            total.append(acc + float(lp[T - 1, U, blank]))
    if not total:
        return math.inf
    m = max(total)
    return -(m + math.log(sum(math.exp(v - m) for v in total)))


def nll_autograd_band(xb, y, s, Ub, blank=BLANK):
    """-log Z of ONE utterance from its band logits xb (T_b,W,V) (requires_grad) through a cell-by-cell torch.logaddexp lattice under
    autograd: the band rows scattered into (T_b,U_b+1) log-probabilities, -1e30 standing for -inf outside the band."""
    Tb, W, V = xb.shape
    rows = {}
    for t in range(Tb):
        for w in range(W):
            if int(s[t]) + w <= Ub:
                rows[(t, int(s[t]) + w)] = torch.log_softmax(xb[t, w], -1)
    out = xb.new_full((), -1e30)
    alpha = [[None] * (Ub + 1) for _ in range(Tb)]

    def lp(t, u, v):
        return rows[(t, u)][v] if (t, u) in rows else out
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                alpha[t][u] = xb.new_zeros(())
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1][u] + lp(t - 1, u, blank))
            if u > 0:
                terms.append(alpha[t][u - 1] + lp(t, u - 1, y[u - 1]))
            alpha[t][u] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return -(alpha[Tb - 1][Ub] + lp(Tb - 1, Ub, blank))


# ------------------------------------------------------------------------------------------------ the banded joint
def joint_pruned(e, p, s_begin, W, dtype=torch.float64):
    return torch.tanh(e.to(dtype)[:, :, None, :] + gather_band(p.to(dtype)[:, None].expand(-1, e.shape[1], -1, -1), s_begin, W))


def joint_pruned_bwd(dz, z, s_begin, U1, dtype=torch.float64):
    """de (B,T,J) = sum_w, dp (B,U1,J) = the sum over the frames whose window holds u (ascending t), of dz (1 - z^2)."""
    B, T, W, J = z.shape
    g = dz.to(dtype) * (1.0 - z.to(dtype) * z.to(dtype))
    de = g[:, :, 0].clone()
    for w in range(1, W):
        de = de + g[:, :, w]
    dp = torch.zeros((B, U1, J), dtype=dtype)
    for b in range(B):
        for t in range(T):
            a = _clamp(s_begin[b, t], 0, U1 - W)
            dp[b, a:a + W] += g[b, t]
    return de, dp


# ------------------------------------------------------------------------------------------------ the kernel cases
def simple_case(V, seed=0, ld=None, B=3, T=7, Umax=5, frames=(7, 1, 3), lengths=(5, 0, 2), scale=2.0, labels=None):
    """am (B,T,ld), lm (B,Umax+1,ld) fp32 whose first V columns count, NaN in the pad columns and in every dead row; targets (B,Umax)."""
    g = torch.Generator().manual_seed(7000 * V + seed)
    ld = V if ld is None else ld
    am = torch.full((B, T, ld), math.nan)
    lm = torch.full((B, Umax + 1, ld), math.nan)
    tg = torch.zeros((B, max(Umax, 1)), dtype=torch.int64)
    for b in range(B):
        am[b, :frames[b], :V] = torch.randn((frames[b], V), generator=g) * scale
        lm[b, :lengths[b] + 1, :V] = torch.randn((lengths[b] + 1, V), generator=g) * scale
        if lengths[b]:
            tg[b, :lengths[b]] = torch.randint(1, V, (lengths[b],), generator=g)
    if labels is not None:
        for b, row in labels.items():
            tg[b, :len(row)] = torch.tensor(row)
    return dict(am=am, lm=lm, targets=tg, frames=torch.tensor(frames, dtype=torch.int32), lengths=torch.tensor(lengths, dtype=torch.int32),
                V=V, ld=ld)
