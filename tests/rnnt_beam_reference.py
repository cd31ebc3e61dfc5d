"""Float64 restatement of the transducer beam search (csrc/rnnt_beam.hip) in NumPy on the CPU.

Blank = 0 = PAD.  A hypothesis is a label sequence y with score = the log-probability summed over all alignments found for it so far;
its context is its last C labels, SOS where it has fewer (ctx[0] = the last label).  logp(t, h) = log_softmax(row(t, ctx(h))): the
callback `row` returns a logits row, so the search does not care who made the logits.  Parameters W (beam), K (label candidates per
row, 0: min(V - 1, 16)), S (max_symbols >= 1).  Per utterance:

    A = {(empty, 0)}; for each frame t < T_b:
        C_0 = A, D = {}; for s = 0 .. S:
            blank step   every h of C_s: (h.y, h.score + logp(t,h)[blank]) joins D; a sequence D already holds is merged by logaddexp
            label step   (s < S) candidates (h.y + k, h.score + logp(t,h)[k]) for the K largest non-blank entries k of each row (greater
                         logit first, lower label first among equals); C_{s+1} = the W best: score descending, then the parent's place
                         in C_s, then the label id, both ascending.  Nothing merges here
        A = the W best of D: score descending, then order of first insertion
    result: the nbest <= W best of A, best first; T_b = 0: the empty sequence with score 0; missing entries: length -1, score -inf

Every function takes a dtype, so the SAME search can be run in fp32: the tolerance of the GPU tests is four times the error of that
fp32 run against the float64 one, with a floor of one fp32 rounding of the largest magnitude that entered a sum.

search() also reports the smallest margin of every kind of decision it took:
    topk    the K-th against the (K+1)-th non-blank logit of a row
    cand    the W-th against the (W+1)-th candidate of a label step
    beam    the W-th against the (W+1)-th entry of D at the end of a frame
    order   neighbours among the returned nbest (and the last of them against the next entry of A): what fixes the ORDER of the result
A case whose margins are all well above the score error has ONE right answer; the GPU tests assert that before they compare."""
import itertools
import math

import numpy as np

BLANK, SOS = 0, 1
EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 1e-3                                  # what the GPU tests require of every margin


def log_softmax(x):
    m = x.max()
    return (x - m) - np.log(np.exp(x - m).sum(dtype=x.dtype))


def context(y, C, sos=SOS):
    """The last C labels of y, the last one first, SOS where y has fewer."""
    return tuple(([sos] * C + [int(v) for v in y])[::-1][:C])


def search(row, Tb, V, W, K=0, S=5, nbest=1, C=2, blank=BLANK, sos=SOS, dtype=np.float64):
    """-> dict(hyps [(y tuple, score)] best first (at most nbest), last_d [(y, score)] = the last frame's D in rank order (empty for
    Tb = 0), margins {topk, cand, beam, order}, pruned (bool: some candidate or D entry was dropped), maxabs (the largest magnitude
    that entered a sum))."""
    K = int(K) if K else min(V - 1, 16)
    assert 1 <= K < V and W >= 1 and S >= 1 and 1 <= nbest <= W
    A = [((), dtype(0.0))]
    margins = dict(topk=math.inf, cand=math.inf, beam=math.inf, order=math.inf)
    pruned, maxabs, last_d = False, 0.0, []
    for t in range(max(0, int(Tb))):
        Cs, D = A, {}
        for s in range(S + 1):
            rows = []
            for y, sc in Cs:
                x = np.asarray(row(t, context(y, C, sos)), dtype=dtype)
                assert x.shape == (V,)
                lp = log_softmax(x)
                rows.append((x, lp))
                v = dtype(sc + lp[blank])
                maxabs = max(maxabs, abs(float(sc)), abs(float(lp[blank])))
                D[y] = dtype(np.logaddexp(D[y], v)) if y in D else v
            if s == S:
                break
            cands = []
            for r, ((y, sc), (x, lp)) in enumerate(zip(Cs, rows)):
                labels = sorted((k for k in range(V) if k != blank), key=lambda k: (-x[k], k))
                if len(labels) > K:
                    margins["topk"] = min(margins["topk"], float(x[labels[K - 1]] - x[labels[K]]))
                for k in labels[:K]:
                    cands.append((dtype(sc + lp[k]), r, k, y + (k,)))
                    maxabs = max(maxabs, abs(float(lp[k])))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            if len(cands) > W:
                pruned = True
                margins["cand"] = min(margins["cand"], float(cands[W - 1][0] - cands[W][0]))
            Cs = [(c[3], c[0]) for c in cands[:W]]
        items = list(D.items())
        order = sorted(range(len(items)), key=lambda i: (-items[i][1], i))
        if len(order) > W:
            pruned = True
            margins["beam"] = min(margins["beam"], float(items[order[W - 1]][1] - items[order[W]][1]))
        last_d = [items[i] for i in order]
        A = last_d[:W]
    hyps = A[:nbest]
    for i in range(min(len(A) - 1, len(hyps))):
        margins["order"] = min(margins["order"], float(A[i][1] - A[i + 1][1]))
    return dict(hyps=[(tuple(y), sc) for y, sc in hyps], last_d=last_d, margins=margins, pruned=pruned, maxabs=maxabs)


def min_margin(res):
    return min(res["margins"].values())


def as_arrays(results, nbest, L, blank=BLANK):
    """The kernel's output form of a list of search() results: ids (B,nbest,L) int32 with blank behind the length, lengths (B,nbest)
    int32 (-1: no such hypothesis), scores (B,nbest) float64 (-inf: none)."""
    B = len(results)
    ids = np.full((B, nbest, L), blank, dtype=np.int32)
    lens = np.full((B, nbest), -1, dtype=np.int32)
    sc = np.full((B, nbest), -math.inf, dtype=np.float64)
    for b, res in enumerate(results):
        for n, (y, s) in enumerate(res["hyps"]):
            ids[b, n, :len(y)] = y
            lens[b, n] = len(y)
            sc[b, n] = float(s)
    return ids, lens, sc


# ------------------------------------------------------------------------------------------------ callbacks
def table_row(e, tables, w_out, b_out, dtype=np.float64):
    """row(t, ctx) of ONE utterance from the head's parameters in `dtype`: e (T,J), tables C arrays (V,J) (tables[k]: the label k places
    back), w_out (V,J), b_out (V): w_out tanh(e[t] + sum_k tables[k][ctx[k]]) + b_out."""
    e = np.asarray(e, dtype=dtype)
    tables = [np.asarray(t, dtype=dtype) for t in tables]
    w_out, b_out = np.asarray(w_out, dtype=dtype), np.asarray(b_out, dtype=dtype)

    def row(t, ctx):
        p = tables[0][ctx[0]]
        for tab, c in zip(tables[1:], ctx[1:]):
            p = p + tab[c]
        return w_out @ np.tanh(e[t] + p) + b_out
    return row


def lookup_row(logits):
    """row(t, ctx) from a dict {(t, ctx): logits row} (the GPU tests fill it with the project's own joint and projection)."""
    return lambda t, ctx: logits[(t, tuple(ctx))]


# ------------------------------------------------------------------------------------------------ brute force
def enumerate_scores(row, Tb, V, S, C=2, blank=BLANK, sos=SOS, max_len=None):
    """{y: log of the summed probability of every alignment of y over Tb frames with at most S labels per frame}, float64, by
    enumeration: frame t emits n_t <= S labels and then the blank."""
    labels = [k for k in range(V) if k != blank]
    cache = {}

    def lp(t, y):
        key = (t, context(y, C, sos))
        if key not in cache:
            cache[key] = log_softmax(np.asarray(row(t, key[1]), dtype=np.float64))
        return cache[key]
    total = {}
    for counts in itertools.product(range(S + 1), repeat=Tb):
        U = sum(counts)
        if max_len is not None and U > max_len:
            continue
        for y in itertools.product(labels, repeat=U):
            s, u = 0.0, 0
            for t, n in enumerate(counts):
                for _ in range(n):
                    s += float(lp(t, y[:u])[y[u]])
                    u += 1
                s += float(lp(t, y[:u])[blank])
            total.setdefault(y, []).append(s)
    out = {}
    for y, terms in total.items():
        m = max(terms)
        out[y] = m + math.log(sum(math.exp(v - m) for v in terms))
    return out


def training_logits(row, y, Tb, V, C=2, sos=SOS):
    """(Tb, len(y) + 1, V) float64: the logits the training lattice of y reads, cell (t,u) = row(t, ctx(y[:u]))."""
    return np.stack([np.stack([np.asarray(row(t, context(y[:u], C, sos)), dtype=np.float64) for u in range(len(y) + 1)])
                     for t in range(Tb)])


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
def exact_case(B, T, J, V, C, seed):
    """Parameters on which every arm computes the SAME logits bit for bit: e and table entries in {-20, 0, 20}, so tanh saturates to
    exactly -1, 0 or 1 in fp32 and in bf16; w_out small integers and halves (beyond the first 8 columns only a few are non-zero, so the
    logits stay small); b_out distinct multiples of 1/512, which separate the logits of labels whose weights agree.
    -> dict of float32 arrays e (B,T,J), tables [C x (V,J)], w_out (V,J), b_out (V)."""
    g = np.random.default_rng(seed)
    e = g.choice(np.array([-20.0, 0.0, 20.0], dtype=np.float32), size=(B, T, J))
    tables = [g.choice(np.array([-20.0, 0.0, 20.0], dtype=np.float32), size=(V, J), p=[0.2, 0.6, 0.2]) for _ in range(C)]
    w_out = (g.integers(-4, 5, size=(V, J)) / 2.0).astype(np.float32)
    w_out[:, 8:] *= (g.random((V, max(J - 8, 0))) < 8.0 / max(J, 8))
    b_out = g.permutation(V).astype(np.float32) / 512.0 - 4.0
    return dict(e=e, tables=tables, w_out=w_out, b_out=b_out)


def random_case(B, T, J, V, C, seed, scale=1.0):
    """Gaussian parameters, float32: e (B,T,J), tables, w_out (scaled by scale / sqrt(J)), b_out."""
    g = np.random.default_rng(seed)
    e = g.standard_normal((B, T, J)).astype(np.float32)
    tables = [g.standard_normal((V, J)).astype(np.float32) for _ in range(C)]
    w_out = (g.standard_normal((V, J)) * (3.0 * scale / math.sqrt(J))).astype(np.float32)
    b_out = g.standard_normal(V).astype(np.float32)
    return dict(e=e, tables=tables, w_out=w_out, b_out=b_out)


def merge_case():
    """Hand-set parameters (B 1, T 2, J 8, V 4, C 1) whose winner wins only through the merge.  Joint dimension 0 carries the frame (+1,
    -1), dimension 1 whether the context is still SOS (+1) or a label (-1), both saturated by the tanh; the probabilities are
        frame 0 from ():   blank 0.2985, label 2 0.2985, label 3 0.403     (logits 0, -20, 0, 0.3)
        frame 1 from ():   blank 0.5, label 2 0.5                          (logits 0, -20, 0, -9.7)
        after a label:     blank ~1                                        (logits 0, -20, -10, <= -9.7)
    (2) is reached as label-then-blank (0.2985) and as blank-then-label (0.149): each is below (3)'s 0.403, together they are 0.448."""
    e = np.zeros((1, 2, 8), dtype=np.float32)
    e[0, 0, 0], e[0, 1, 0] = 20.0, -20.0
    tab = np.zeros((4, 8), dtype=np.float32)
    tab[:, 1] = -20.0
    tab[SOS, 1] = 20.0
    w_out = np.zeros((4, 8), dtype=np.float32)
    w_out[2, 1] = 5.0
    w_out[3, 0], w_out[3, 1] = 5.0, 5.0
    b_out = np.array([0.0, -20.0, -5.0, -9.7], dtype=np.float32)
    return dict(e=e, tables=[tab], w_out=w_out, b_out=b_out)


def cut_case(T=2):
    """Hand-set parameters (B 1, J 8, V 3, C 1) of a head that always prefers label 2 (logits 0, -3, 3 whatever the frame and the
    context): only max_symbols ends a frame, and the longest sequence the search can return has T S labels."""
    return dict(e=np.zeros((1, T, 8), dtype=np.float32), tables=[np.zeros((3, 8), dtype=np.float32)],
                w_out=np.zeros((3, 8), dtype=np.float32), b_out=np.array([0.0, -3.0, 3.0], dtype=np.float32))
