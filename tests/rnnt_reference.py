"""Float64 restatement of the transducer head (csrc/rnnt.hip) in plain torch on the CPU: the lattice, the loss, its
gradient with respect to the logits by the closed formula, the joint and its two reductions, and the time-synchronous greedy search with
the margin of every decision.  Every function takes a dtype so the SAME formula can be run in fp32: the tolerance of the GPU tests is
four times the error of that fp32 run against the float64 one (tests/mwer_reference.py: bound32, excess).

Definitions (blank = 0 = PAD; utterance b has T_b live frames and U_b labels y_1 .. y_U):
    alpha(t,u) = logaddexp(alpha(t-1,u) + blank(t-1,u), alpha(t,u-1) + label(t,u-1)),   alpha(0,0) = 0
    beta(t,u)  = logaddexp(beta(t+1,u) + blank(t,u), beta(t,u+1) + label(t,u)),   beta(T_b,U_b) = 0, every other beta(T_b,u) = -inf
    nll_b = -(alpha(T_b-1,U_b) + blank(T_b-1,U_b)),   loss = mean_b nll_b / max(U_b, 1)
Edge rules: U_b = 0 is legal; T_b = 0 or a label that is the blank or outside [0,V): nll_b = +inf and zero gradient rows; cells with
t >= T_b or u > U_b are dead (never read, zero gradient)."""
import itertools
import math

import torch

from mwer_reference import BF16_REL, EPS32, bound32, excess  # noqa: F401  (re-exported: the tolerance rule of tests/test_gpu_mwer.py)

BLANK, SOS = 0, 1
NEG = -math.inf


def valid(y, Tb, V, blank=BLANK):
    return Tb > 0 and all(0 <= int(v) < V and int(v) != blank for v in y)


def lattice(lpb, lpl):
    """lpb (T,U+1) blank log-probabilities, lpl (T,U) label log-probabilities (label(t,u) = log p(y_{u+1} | t,u)) -> (alpha, beta, logZ),
    walked by anti-diagonals like the kernel (the cells of a diagonal are independent)."""
    T, U1 = lpb.shape
    U = U1 - 1
    dt = lpb.dtype
    alpha = torch.full((T, U1), NEG, dtype=dt)
    beta = torch.full((T, U1), NEG, dtype=dt)
    alpha[0, 0] = 0.0
    for d in range(1, T + U):
        u = torch.arange(max(0, d - (T - 1)), min(d, U) + 1)
        t = d - u
        a0 = torch.full((u.numel(),), NEG, dtype=dt)
        a1 = torch.full((u.numel(),), NEG, dtype=dt)
        m0 = t > 0
        a0[m0] = alpha[t[m0] - 1, u[m0]] + lpb[t[m0] - 1, u[m0]]
        m1 = u > 0
        a1[m1] = alpha[t[m1], u[m1] - 1] + lpl[t[m1], u[m1] - 1]
        alpha[t, u] = torch.logaddexp(a0, a1)
    beta[T - 1, U] = lpb[T - 1, U]
    for d in range(T + U - 2, -1, -1):
        u = torch.arange(max(0, d - (T - 1)), min(d, U) + 1)
        t = d - u
        b0 = torch.full((u.numel(),), NEG, dtype=dt)
        b1 = torch.full((u.numel(),), NEG, dtype=dt)
        m0 = t + 1 < T
        b0[m0] = beta[t[m0] + 1, u[m0]] + lpb[t[m0], u[m0]]
        m1 = u < U
        b1[m1] = beta[t[m1], u[m1] + 1] + lpl[t[m1], u[m1]]
        beta[t, u] = torch.logaddexp(b0, b1)
    return alpha, beta, alpha[T - 1, U] + lpb[T - 1, U]


def loss_and_grad(logits, targets, frames, lengths, V=None, blank=BLANK, dtype=torch.float64, grad_out=1.0):
    """logits (B,T,U1,>=V) (only the live cells and the first V columns are read), targets (B,>=Umax) ids, frames / lengths per utterance
    -> dict(nll (B,), loss, dlogits (B,T,U1,V) = grad_out * d loss / d logits, alpha / beta / logz per utterance), all in `dtype`."""
    B, T, U1 = logits.shape[:3]
    V = logits.shape[3] if V is None else V
    nll = torch.zeros(B, dtype=dtype)
    dl = torch.zeros((B, T, U1, V), dtype=dtype)
    lat = []
    for b in range(B):
        Tb, Ub = max(0, min(T, int(frames[b]))), max(0, min(U1 - 1, int(lengths[b])))
        y = [int(v) for v in targets[b][:Ub]]
        if not valid(y, Tb, V, blank):
            nll[b] = math.inf
            lat.append(None)
            continue
        x = torch.as_tensor(logits[b, :Tb, :Ub + 1, :V]).to(dtype)
        lp = torch.log_softmax(x, -1)
        lpb = lp[..., blank]
        yi = torch.tensor(y, dtype=torch.int64)
        lpl = lp[:, :Ub, :].gather(2, yi.view(1, Ub, 1).expand(Tb, Ub, 1))[..., 0] if Ub else lp.new_zeros((Tb, 0))
        alpha, beta, logz = lattice(lpb, lpl)
        nll[b] = -logz
        lat.append((alpha, beta, logz))
        if not math.isfinite(float(logz)):
            continue
        bnext = torch.full((Tb, Ub + 1), NEG, dtype=dtype)
        bnext[:Tb - 1] = beta[1:]
        bnext[Tb - 1, Ub] = 0.0
        gb = torch.exp(alpha + lpb + bnext - logz)
        gl = torch.zeros((Tb, Ub + 1), dtype=dtype)
        if Ub:
            gl[:, :Ub] = torch.exp(alpha[:, :Ub] + lpl + beta[:, 1:] - logz)
        g = (gb + gl)[..., None] * torch.exp(lp)
        g[..., blank] -= gb
        if Ub:
            g[:, :Ub, :].scatter_add_(2, yi.view(1, Ub, 1).expand(Tb, Ub, 1), -gl[:, :Ub, None])
        c = torch.tensor(grad_out, dtype=dtype) / torch.tensor(float(B * max(Ub, 1)), dtype=dtype)
        dl[b, :Tb, :Ub + 1] = c * g
    den = torch.tensor([float(max(1, max(0, min(U1 - 1, int(n))))) for n in lengths], dtype=dtype)
    return dict(nll=nll, loss=(nll / den).sum() / B, dlogits=dl, lattice=lat)


def nll_autograd(x, y, blank=BLANK):
    """-log Z of ONE utterance from logits x (T,U+1,V) (requires_grad) through a cell-by-cell torch.logaddexp lattice: what autograd
    differentiates in tests/test_rnnt_host.py."""
    T, U1, _ = x.shape
    lp = torch.log_softmax(x, -1)
    alpha = [[None] * U1 for _ in range(T)]
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                alpha[t][u] = lp.new_zeros(())
                continue
            terms = []
            if t > 0:
                terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(alpha[t][u - 1] + lp[t, u - 1, y[u - 1]])
            alpha[t][u] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    return -(alpha[T - 1][U1 - 1] + lp[T - 1, U1 - 1, blank])


def nll_brute_force(x, y, blank=BLANK):
    """-log of the sum over EVERY alignment, enumerated: the T - 1 frame advances and the U labels in any order, then the last blank."""
    T, U1, _ = x.shape
    U = U1 - 1
    lp = torch.log_softmax(x.double(), -1)
    total = []
    for labels_at in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        s = 0.0
        for i in range(T - 1 + U):
            if i in labels_at:
                s += float(lp[t, u, y[u]])
                u += 1
            else:
                s += float(lp[t, u, blank])
                t += 1
        total.append(s + float(lp[T - 1, U, blank]))
    m = max(total)
    return -(m + math.log(sum(math.exp(v - m) for v in total)))


# ------------------------------------------------------------------------------------------------ the joint
def joint(e, p, dtype=torch.float64):
    return torch.tanh(e.to(dtype)[:, :, None, :] + p.to(dtype)[:, None, :, :])


def joint_bwd(dz, z, dtype=torch.float64):
    g = dz.to(dtype) * (1.0 - z.to(dtype) * z.to(dtype))
    return g.sum(2), g.sum(1)


# ------------------------------------------------------------------------------------------------ greedy search
def greedy(e, tables, w_out, b_out, lengths, max_symbols, blank=BLANK, sos=SOS):
    """Time-synchronous greedy search in float64: e (B,T,J) the encoder side of the joint, tables C predictor tables (V,J) (tables[k]:
    the label k places back), w_out (V,J), b_out (V) -> (ids per utterance, decisions per utterance = [(frame, arg-max, margin to the
    runner-up)] in the order they were taken).  At frame t: emit the arg-max while it is not blank, at most max_symbols times."""
    e = e.double()
    tables = [t.double() for t in tables]
    w_out, b_out = w_out.double(), b_out.double()
    ids, decisions = [], []
    for b in range(e.shape[0]):
        hist, out, dec = [sos] * len(tables), [], []
        for t in range(max(0, min(e.shape[1], int(lengths[b])))):
            for _ in range(max_symbols):
                z = torch.tanh(e[b, t] + sum(tab[h] for tab, h in zip(tables, hist)))
                logit = w_out @ z + b_out
                top = torch.topk(logit, 2)
                k = int(top.indices[0])
                dec.append((t, k, float(top.values[0] - top.values[1])))
                if k == blank:
                    break
                out.append(k)
                hist = [k] + hist[:-1]
        ids.append(out)
        decisions.append(dec)
    return ids, decisions


def decided_prefix(ids, decisions, margin, blank=BLANK):
    """The labels of `ids` emitted before the first decision whose margin is below `margin` (everything when none is)."""
    n = 0
    for _, k, m in decisions:
        if m < margin:
            return ids[:n], False
        n += k != blank
    return ids, True


# ------------------------------------------------------------------------------------------------ the kernel cases
SHAPE = dict(B=3, T=7, Umax=5, frames=[7, 1, 3], lengths=[5, 0, 2])


def case(V, seed=0, ld=None, B=3, T=7, Umax=5, frames=(7, 1, 3), lengths=(5, 0, 2), scale=2.0):
    """Logits (B,T,Umax+1,ld) fp32 whose first V columns count, NaN in the pad columns and in every dead row; targets (B,Umax) with PAD
    behind the labels."""
    g = torch.Generator().manual_seed(1000 * V + seed)
    ld = V if ld is None else ld
    x = torch.full((B, T, Umax + 1, ld), math.nan)
    tg = torch.zeros((B, max(Umax, 1)), dtype=torch.int64)
    for b in range(B):
        x[b, :frames[b], :lengths[b] + 1, :V] = torch.randn((frames[b], lengths[b] + 1, V), generator=g) * scale
        if lengths[b]:
            tg[b, :lengths[b]] = torch.randint(1, V, (lengths[b],), generator=g)
    return dict(logits=x, targets=tg, frames=torch.tensor(frames, dtype=torch.int32), lengths=torch.tensor(lengths, dtype=torch.int32),
                V=V, ld=ld)
