"""Host restatement of CTC forced alignment (csrc/ctc_align.hip) in NumPy, pinned by tests/test_ctc_align_host.py.

align(..., dtype=np.float32) is the kernel's recursion literally -- raw logits, compare first and then ONE add in `dtype`, a predecessor
replaces the best only if strictly greater in the order stay, advance, skip, the last state wins the final tie -- so its path / start / end
are what the kernel must produce bit for bit.  align(..., dtype=np.float64) is the yardstick for score and lab_score.  The log-sum-exp
is float64 in both: it enters the two scores only, never the path.

cases() are the inputs of tests/test_gpu_ctc_align.py, kept here so that the host suite can hold the two precisions against each other
on exactly those inputs."""
import itertools

import numpy as np

NEG = -np.inf


def lse_rows(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1)
    return m + np.log(np.exp(x - m[..., None]).sum(axis=-1))


def align_one(lg, target, Tb, blank=0, dtype=np.float32):
    """lg (T,V) array (frames >= Tb are never touched), target: label ids -> dict(path [Tb] or None, start, end, lab_score [L], score).
    Infeasible (no path, or a label that is blank / outside [0,V)): path None, start = end = -1, lab_score 0, score -inf."""
    V = lg.shape[1]
    L = len(target)
    bad = {"path": None, "start": [-1] * L, "end": [-1] * L, "lab_score": [0.0] * L, "score": NEG}
    if any(int(c) == blank or int(c) < 0 or int(c) >= V for c in target):
        return bad
    if Tb == 0:
        return {"path": [], "start": [], "end": [], "lab_score": [], "score": 0.0} if L == 0 else bad
    S = 2 * L + 1
    lab = np.full(S, blank, dtype=np.int64)
    lab[1::2] = np.asarray(target, dtype=np.int64)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (lab[2:] != blank) & (lab[2:] != lab[:-2])
    x = np.asarray(lg[:Tb], dtype=dtype)[:, lab]                  # (Tb, S) emissions in the recursion's precision
    prev = np.full(S, NEG, dtype=dtype)
    prev[:2] = x[0, :2]
    bp = np.zeros((Tb, S), dtype=np.int8)
    for t in range(1, Tb):
        best = prev.copy()
        a1 = np.concatenate([[NEG], prev[:-1]]).astype(dtype)
        m = a1 > best
        best[m] = a1[m]
        bp[t][m] = 1
        a2 = np.concatenate([[NEG, NEG], prev[:-2]]).astype(dtype)[:S]
        m = skip & (a2 > best)
        best[m] = a2[m]
        bp[t][m] = 2
        prev = (best + x[t]).astype(dtype)                        # one add, rounded to `dtype`
    s = S - 1
    if S >= 2 and prev[S - 2] > prev[S - 1]:
        s = S - 2
    raw = float(prev[s])
    if raw == NEG:
        return bad
    path = [0] * Tb
    for t in range(Tb - 1, -1, -1):
        path[t] = s
        s -= int(bp[t][s])
    lse = lse_rows(lg[:Tb])
    start, end, lab_score = [-1] * L, [-1] * L, [0.0] * L
    for t, st in enumerate(path):
        if st & 1:
            l = st >> 1
            if start[l] < 0:
                start[l] = t
            end[l] = t + 1
            lab_score[l] += float(np.asarray(lg[t, lab[st]], dtype=np.float64)) - float(lse[t])
    return {"path": path, "start": start, "end": end, "lab_score": lab_score, "score": raw - float(lse.sum())}


def align(logits, targets, input_lengths, target_lengths, blank=0, dtype=np.float32):
    """The batch, in the kernel's output layout: path (B,T) int32 (-1 padded), start / end (B,Lmax) int32, lab_score (B,Lmax) and score
    (B) float64.  Lengths are clamped to [0,T] and [0,Lmax] as the kernel clamps them."""
    logits = np.asarray(logits)
    targets = np.asarray(targets)
    B, T, _ = logits.shape
    Lmax = targets.shape[1]
    out = {"path": np.full((B, T), -1, dtype=np.int32), "start": np.full((B, Lmax), -1, dtype=np.int32),
           "end": np.full((B, Lmax), -1, dtype=np.int32), "lab_score": np.zeros((B, Lmax)), "score": np.full(B, NEG)}
    for b in range(B):
        Tb = max(0, min(T, int(input_lengths[b])))
        Lb = max(0, min(Lmax, int(target_lengths[b])))
        r = align_one(logits[b], [int(c) for c in targets[b, :Lb]], Tb, blank, dtype)
        out["score"][b] = r["score"]
        if r["path"] is None:
            continue
        out["path"][b, :Tb] = r["path"]
        out["start"][b, :Lb], out["end"][b, :Lb], out["lab_score"][b, :Lb] = r["start"], r["end"], r["lab_score"]
    return out


def collapse(states, target):
    """The label sequence a lattice path spells: its odd states, repeats of one state merged."""
    out, prev = [], None
    for s in states:
        if s != prev and s & 1:
            out.append(int(target[s >> 1]))
        prev = s
    return out


def enumerate_best(lg, target, Tb, blank=0):
    """The maximum over ALL frame-wise label sequences of length Tb that collapse to `target` of the summed raw logits, by brute force
    (V ** Tb sequences), and one sequence that attains it; (-inf, None) when there is none."""
    V = lg.shape[1]
    best, arg = NEG, None
    for seq in itertools.product(range(V), repeat=Tb):
        out, prev = [], None
        for c in seq:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        if out != list(target):
            continue
        sc = float(sum(np.float64(lg[t, c]) for t, c in enumerate(seq)))
        if sc > best:
            best, arg = sc, seq
    return best, arg


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
def _logits(B, T, V, seed):
    return (np.random.default_rng(seed).standard_normal((B, T, V)) * 2.0).astype(np.float32)


def _repeated(rng, L, V):
    """L labels in [3, V), every second one a repeat of the one before it."""
    seq = rng.integers(3, V, size=L)
    seq[1::2] = seq[0::2][:len(seq[1::2])]
    return seq


def cases():
    """name -> dict(logits (B,T,V) float32, targets (B,Lmax) int64, input_lengths, target_lengths).  Frames >= T_b hold NaN and targets >=
    L_b hold V + 5 where the case says so: neither may be read."""
    out = {}
    B, T, V = 3, 12, 7
    tb, tl = [12, 5, 1], [4, 2, 1]
    tg = np.full((B, 4), V + 5, dtype=np.int64)
    tg[0, :4], tg[1, :2], tg[2, :1] = [3, 3, 5, 4], [6, 3], [4]                  # row 0 starts with a repeated pair
    for name, lg in (("small", _logits(B, T, V, 21)),
                     ("small_integer", np.random.default_rng(22).integers(-3, 4, size=(B, T, V)).astype(np.float32))):
        lg = lg.copy()
        for b in range(B):
            lg[b, tb[b]:] = np.nan
        out[name] = dict(logits=lg, targets=tg.copy(), input_lengths=tb, target_lengths=tl)
    rng = np.random.default_rng(23)
    out["two_states_per_thread"] = dict(logits=_logits(1, 300, 32, 24), targets=_repeated(rng, 140, 32)[None], input_lengths=[300],
                                        target_lengths=[140])
    lg = _logits(2, 100, 4364, 25)
    lg[1, 73:] = np.nan
    tg = rng.integers(3, 4364, size=(2, 30))
    out["benchmark_vocabulary"] = dict(logits=lg, targets=tg, input_lengths=[100, 73], target_lengths=[30, 22])
    out["largest_project_shape"] = dict(logits=_logits(1, 625, 64, 26), targets=_repeated(rng, 300, 64)[None], input_lengths=[625],
                                        target_lengths=[300])
    # past the LDS of a CU whatever the packing: 69 chunks of 601 back-pointer words are 166 KB, so the workspace arm runs
    lg = _logits(2, 1100, 8, 27)
    lg[1, 900:] = np.nan
    tg = np.stack([_repeated(rng, 300, 8), _repeated(rng, 300, 8)])
    out["back_pointers_in_the_workspace"] = dict(logits=lg, targets=tg, input_lengths=[1100, 900], target_lengths=[300, 260])
    # edge batch: rows 0, 1, 7 are feasible; 2..6 are not and must leave their neighbours alone
    V = 6
    lg = _logits(8, 6, V, 28)
    tb = [6, 0, 0, 2, 2, 5, 5, 4]
    tl = [0, 0, 1, 2, 3, 2, 2, 2]
    tg = np.array([[V + 5] * 3, [V + 5] * 3, [3, V + 5, V + 5], [3, 3, V + 5], [3, 4, 5], [3, 0, V + 5], [3, V, V + 5], [4, 5, V + 5]],
                  dtype=np.int64)
    for b in range(8):
        lg[b, tb[b]:] = np.nan
    out["edges"] = dict(logits=lg, targets=tg, input_lengths=tb, target_lengths=tl)
    return out
