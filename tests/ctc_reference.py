"""Float64 restatement of the CTC loss kernels (csrc/ctc.hip: asr_ctc_fwd / asr_ctc_bwd) in plain numpy, written from the formulas in that
file's header comment, plus an integer known answer that shares neither a logarithm nor a recursion with them, plus the named cases of
tests/test_gpu_ctc_arms.py (the CPU checks of tests/test_ctc_reference_host.py run on the same tensors).

    lp_t(v)    = logits[b,t,v] - logsumexp_v logits[b,t,:]
    alpha_t(s) = lp_t(l'_s) + logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) if l'_s != blank and l'_s != l'_{s-2}])
    beta_t(s)  = lp_t(l'_s) + logsumexp(beta_{t+1}(s), beta_{t+1}(s+1), [beta_{t+1}(s+2) if l'_s != blank and l'_s != l'_{s+2}])
    nll_b      = -logsumexp(alpha_{T_b-1}(S_b-1), alpha_{T_b-1}(S_b-2)),  l' = blank-interleaved target, S_b = 2 L_b + 1
    loss       = mean_b(nll_b / max(L_b, 1))
    d nll_b / d logits[b,t,v] = softmax_t(v) - sum_{s: l'_s = v} exp(alpha_t(s) + beta_t(s) - lp_t(v) + nll_b)     (t < T_b, else 0)

Conventions (include/asr_hip.h): T_b = clamp(in_len, 0, T), L_b = clamp(tg_len, 0, Lmax) everywhere; T_b = 0 gives nll 0 for L_b = 0, else
+inf; a label among the L_b used ones outside [0, V) gives +inf; an infinite utterance has NaN rows for t < T_b and zero rows after; exp(-inf)
= 0 and a state whose lp is -inf contributes nothing (torch returns all-NaN gradients for -inf logits and cannot be the truth there)."""
import itertools
import math

import numpy as np

NEG = -np.inf

# deliberate defects of the restatement (tests/test_ctc_reference_host.py shows that the bound of the GPU tests catches each one)
DEFECTS = ("skip_equal", "skip_blank", "no_start1", "no_final2", "unclamped_len", "mean_sum", "pad_softmax", "no_B")


def _lae(*terms):
    """log(sum exp(terms)) elementwise, -inf safe: all -inf gives -inf, never NaN."""
    m = terms[0]
    for x in terms[1:]:
        m = np.maximum(m, x)
    dead = np.isneginf(m)
    ms = np.where(dead, 0, m).astype(m.dtype)
    acc = np.exp(terms[0] - ms)
    for x in terms[1:]:
        acc = acc + np.exp(x - ms)
    with np.errstate(divide="ignore"):
        out = ms + np.log(acc)
    return np.where(dead, NEG, out).astype(m.dtype)


def _shift(row, k, reverse):
    """row[s-k] (or row[s+k] if reverse), -inf where that state does not exist."""
    out = np.full_like(row, NEG)
    if k < row.shape[0]:
        if reverse:
            out[:-k] = row[k:]
        else:
            out[k:] = row[:-k]
    return out


def ctc_reference(logits, targets, in_len, tg_len, blank, grad_out=1.0, dtype=np.float64, defect=None):
    """logits (B,T,V), targets (B,Lmax) ids, lengths (B) -> (loss, nll (B,), dlogits (B,T,V) = grad_out * d loss / d logits), every
    intermediate in `dtype`.  `defect`: one of DEFECTS, for the planted-defect checks."""
    assert defect is None or defect in DEFECTS
    logits = np.asarray(logits)
    targets = np.asarray(targets)
    B, T, V = logits.shape
    Lmax = targets.shape[1]
    dt = np.dtype(dtype).type
    nll = np.zeros(B, dtype=dtype)
    dl = np.zeros((B, T, V), dtype=dtype)
    Ls = []
    for b in range(B):
        Ls.append(max(0, min(Lmax, int(tg_len[b]))))
    denom_all = dt(max(1, sum(Ls)))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            Tb, Lb = max(0, min(T, int(in_len[b]))), Ls[b]
            y = [int(v) for v in targets[b, :Lb]]
            if any(v < 0 or v >= V for v in y):
                nll[b] = np.inf
                dl[b, :Tb] = np.nan
                continue
            if Tb == 0:
                nll[b] = 0.0 if Lb == 0 else np.inf
                continue
            x = logits[b, :Tb].astype(dtype)
            m = x.max(axis=1, keepdims=True)
            lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=dtype))
            lp = x - lse
            S = 2 * Lb + 1
            ext = np.full(S, blank, dtype=np.int64)
            ext[1::2] = y
            s_idx = np.arange(S)
            notblank = ext != blank
            skip_f = (s_idx >= 2) & notblank & (ext != np.roll(ext, 2))
            skip_b = (s_idx + 2 < S) & notblank & (ext != np.roll(ext, -2))
            if defect == "skip_equal":
                skip_f, skip_b = (s_idx >= 2) & notblank, (s_idx + 2 < S) & notblank
            if defect == "skip_blank":
                skip_f = (s_idx >= 2) & (~notblank | (ext != np.roll(ext, 2)))
                skip_b = (s_idx + 2 < S) & (~notblank | (ext != np.roll(ext, -2)))
            lpe = lp[:, ext]                                           # (Tb, S)
            alpha = np.full((Tb, S), NEG, dtype=dtype)
            beta = np.full((Tb, S), NEG, dtype=dtype)
            alpha[0, 0] = lpe[0, 0]
            if S > 1 and defect != "no_start1":
                alpha[0, 1] = lpe[0, 1]
            beta[Tb - 1, S - 1] = lpe[Tb - 1, S - 1]
            if S > 1:
                beta[Tb - 1, S - 2] = lpe[Tb - 1, S - 2]
            for t in range(1, Tb):
                p = alpha[t - 1]
                alpha[t] = _lae(p, _shift(p, 1, False), np.where(skip_f, _shift(p, 2, False), NEG).astype(dtype)) + lpe[t]
            for t in range(Tb - 2, -1, -1):
                p = beta[t + 1]
                beta[t] = _lae(p, _shift(p, 1, True), np.where(skip_b, _shift(p, 2, True), NEG).astype(dtype)) + lpe[t]
            last = alpha[Tb - 1]
            tail = last[S - 2:S - 1] if (S > 1 and defect != "no_final2") else np.full(1, NEG, dtype=dtype)
            nb = -_lae(last[S - 1:S], tail)[0]
            nll[b] = nb
            if not nb < np.inf:
                dl[b, :Tb] = np.nan
                continue
            e = alpha + beta - lpe + nb
            occ = np.where(np.isneginf(alpha) | np.isneginf(beta), 0, np.exp(e)).astype(dtype)       # a dead state contributes nothing
            acc = np.zeros((Tb, V), dtype=dtype)
            for v in np.unique(ext):
                acc[:, v] = occ[:, ext == v].sum(axis=1, dtype=dtype)
            scale = dt(grad_out) / (dt(max(Lb, 1)) * dt(B))
            if defect == "no_B":
                scale = dt(grad_out) / dt(max(Lb, 1))
            if defect == "mean_sum":
                scale = dt(grad_out) / denom_all
            dl[b, :Tb] = (np.exp(lp) - acc) * scale
            if defect == "pad_softmax" and Tb < T:
                xp = logits[b, Tb:].astype(dtype)
                xp = xp - xp.max(axis=1, keepdims=True)
                ep = np.exp(xp)
                dl[b, Tb:] = ep / ep.sum(axis=1, keepdims=True, dtype=dtype) * scale
        lens = np.array([max(1, int(tg_len[b])) if defect == "unclamped_len" else max(1, Ls[b]) for b in range(B)]).astype(dtype)
        if defect == "mean_sum":
            loss = nll.sum(dtype=dtype) / denom_all
        else:
            loss = (nll / lens).sum(dtype=dtype) / dt(B)
    return dt(loss), nll, dl


def collapse(path, blank):
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return tuple(out)


def ctc_count_reference(T, V, target, blank):
    """The integer known answer for ALL-ZERO logits (every frame labelling has probability V^-T): enumerate the V^T labellings, collapse
    each (merge repeats, drop blanks), count the N that give `target` and occ[t, v], how many of those emit v at frame t.
    -> (N, occ, nll = T log V - log N, dnll/dlogits[t, v] = 1/V - occ[t, v] / N)."""
    target = tuple(int(v) for v in target)
    N, occ = 0, np.zeros((T, V), dtype=np.int64)
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) == target:
            N += 1
            for t, v in enumerate(path):
                occ[t, v] += 1
    nll = T * math.log(V) - math.log(N)
    return N, occ, nll, 1.0 / V - occ.astype(np.float64) / N


# ------------------------------------------------------------------------------------------------ the bound of tests/test_gpu_ctc.py
def loss_ok(got, ref):
    """|got - ref| <= 2e-5 max(1, |ref|); two +inf agree."""
    if math.isinf(ref):
        return math.isinf(got) and (got > 0) == (ref > 0)
    return abs(got - ref) <= 2e-5 * max(1.0, abs(ref))


def grad_bound(ref64, err32):
    fin = ref64[np.isfinite(ref64)]
    return max(2e-6 + 2e-5 * (float(np.abs(fin).max()) if fin.size else 0.0), 4.0 * err32)


def grad_err(got, ref64):
    """Largest |got - ref| over the finite entries of ref; inf if the NaN patterns differ."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64)
    if got.shape != ref64.shape or not np.array_equal(np.isnan(got), np.isnan(ref64)):
        return math.inf
    fin = ~np.isnan(ref64)
    return float(np.abs(got[fin] - ref64[fin]).max()) if fin.any() else 0.0


# ------------------------------------------------------------------------------------------------ the cases
def make_case(B, T, V, Lmax, in_len, tg_len, seed, blank=0, repeat=False, scale=2.0, alphabet=None):
    """Random logits x `scale` (fp32), random labels other than the blank (from `alphabet` symbols if given); "repeat": every second label
    repeats its neighbour ("aabbcc")."""
    g = np.random.default_rng(seed)
    logits = (g.standard_normal((B, T, V)) * scale).astype(np.float32)
    ids = np.array([v for v in range(V if alphabet is None else alphabet + 1) if v != blank], dtype=np.int64)
    tgt = ids[g.integers(0, max(1, ids.size), (B, Lmax))] if ids.size else np.zeros((B, Lmax), dtype=np.int64)
    if repeat:
        n = tgt[:, 1::2].shape[1]
        tgt[:, 1::2] = tgt[:, 0::2][:, :n]
    return dict(logits=logits, targets=np.ascontiguousarray(tgt), in_len=np.asarray(in_len, dtype=np.int32),
                tg_len=np.asarray(tg_len, dtype=np.int32), blank=blank)


COUNTED = {"counted_11": (1, 1), "counted_212": (2, 1, 2), "counted_empty": ()}          # T 6, V 3, blank 0: 35, 84, 1 paths
COUNTED_PATHS = {"counted_11": 35, "counted_212": 84, "counted_empty": 1}


def _counted(target, blank=0):
    tgt = np.zeros((1, 3), dtype=np.int64)
    tgt[0, :len(target)] = target
    return dict(logits=np.zeros((1, 6, 3), dtype=np.float32), targets=tgt, in_len=np.array([6], dtype=np.int32),
                tg_len=np.array([len(target)], dtype=np.int32), blank=blank)


def _batch_mean():
    g = np.random.default_rng(101)
    return make_case(70, 5, 6, 2, g.integers(3, 6, 70), g.integers(0, 2, 70), seed=11)


def _tiny_mixed():
    c = make_case(4, 4, 5, 2, [0, 0, 4, 1], [0, 2, 0, 1], seed=17)
    return c


def _neg_inf(reach):
    """blank-in-the-middle shapes; column 7 is in no target (labels are drawn from 0..6 without the blank 5) and is -inf in every frame.
    reach: utterance 0's second label becomes 7, which no frame can emit."""
    c = make_case(3, 14, 9, 4, [14, 9, 6], [4, 2, 1], seed=12, blank=5, repeat=True, alphabet=6)
    assert not (c["targets"] == 7).any()
    c["logits"][:, :, 7] = NEG
    if reach:
        c["targets"][0, 1] = 7
    return c


def _lengths_outside(which):
    c = make_case(3, 14, 9, 4, [14, 9, 6], [4, 2, 1], seed=12, blank=5, repeat=True)
    if which == "over":
        c["in_len"] = np.array([14 + 5, 9, 6], dtype=np.int32)
        c["tg_len"] = np.array([4 + 3, 2, 1], dtype=np.int32)
    else:
        c["in_len"] = np.array([14, -2, 6], dtype=np.int32)
        c["tg_len"] = np.array([4, -3, -1], dtype=np.int32)
    return c


CASES = {
    "batch_mean": _batch_mean,
    "blank_middle": lambda: make_case(3, 14, 9, 4, [14, 9, 6], [4, 2, 1], seed=12, blank=5, repeat=True),
    "blank_last": lambda: make_case(2, 12, 7, 3, [12, 8], [3, 3], seed=13, blank=6),
    "tiny_one_frame": lambda: make_case(3, 1, 6, 1, [1, 1, 1], [1, 0, 1], seed=14),
    "tiny_blank_only": lambda: make_case(2, 5, 1, 1, [5, 3], [0, 0], seed=15),
    "tiny_mixed": _tiny_mixed,
    "states_over_threads": lambda: make_case(2, 300, 8, 145, [300, 295], [145, 130], seed=18),
    "lattice_grant_full": lambda: make_case(1, 2600, 8, 2100, [2600], [2100], seed=19),
    "lattice_grant_padding": lambda: make_case(2, 40, 8, 2100, [40, 31], [12, 5], seed=20, repeat=True),
    "grad_grant_13000": lambda: make_case(2, 6, 13000, 2, [6, 4], [2, 1], seed=21),
    "grad_grant_16384": lambda: make_case(1, 3, 16384, 1, [3], [1], seed=22),
    "peaked": lambda: make_case(3, 40, 33, 10, [40, 33, 17], [10, 7, 2], seed=23, repeat=True, scale=60.0),
    "neg_inf_column": lambda: _neg_inf(False),
    "neg_inf_reach": lambda: _neg_inf(True),
    "lengths_over": lambda: _lengths_outside("over"),
    "lengths_negative": lambda: _lengths_outside("negative"),
    "counted_11": lambda: _counted((1, 1)),
    "counted_212": lambda: _counted((2, 1, 2)),
    "counted_empty": lambda: _counted(()),
}

# the cases torch's F.ctc_loss defines: lengths inside [1, T] and [0, Lmax], no -inf logits
TORCH_DEFINED = ("batch_mean", "blank_middle", "blank_last", "tiny_one_frame", "tiny_blank_only", "states_over_threads",
                 "lattice_grant_full", "lattice_grant_padding", "grad_grant_13000", "grad_grant_16384", "peaked", "counted_11",
                 "counted_212", "counted_empty")

_cache = {}


def case(name):
    """The tensors of a named case, built once (never modified by a test: copy before changing)."""
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]

