"""Float64 restatement of the fused arms of the transducer beam search (asr_rnnt_beam_search_lm / _ctx, csrc/rnnt_beam.hip; DESIGN.md
section 7) in NumPy on the CPU, pinned by tests/test_rnnt_beam_fused_host.py.  It extends tests/rnnt_beam_reference.py, whose definition
holds for everything not said here.  q(h, c) is the query of utils/ngram.py with the table's float32 values widened and added in float64
(ctc_beam_lm_reference.q64); state, credit and hold are those of utils.context.ContextGraph.

    state        every entry of C_s, D and A also carries lm = the sum of q over its labels, len, the n-gram context (the last order - 1
                 symbols of [bos] + y), cst = state(y) and cnt = credit(y): functions of the label sequence alone, looked up by y here
    key          f(h) = score(h) + bonus(h), bonus = (alpha lm + beta len) + gamma cnt; gamma cnt is the float32 product the kernel forms,
                 the other terms are float64; without an LM lm = 0 and len still counts
    label step   the K candidates of a row stay the K best non-blank entries by logit; C_{s+1} = the W best by f descending, then the
                 parent's place, then the label id
    blank step   as in the plain search: a sequence D already holds merges its score by logaddexp; its state is equal by construction
    frame end    A = the W best of D by f descending, then the order of first insertion
    result       the entries of A ordered by score + bonus(lm + q(ctx, eos), len, cnt - hold(cst)) (no end term for eos = -1), the place
                 in A first among equals; per hypothesis: y, score (the acoustic log-probability), lm with the end term, credit = earned.
                 T_b = 0: the empty sequence, score 0, lm = q([bos], eos), credit 0

With alpha = beta = gamma = 0 every key is the score and the result is rnnt_beam_reference.search's.  margins: topk as there; cand, beam
and order are taken on f / on the final key (order: neighbours among the returned nbest and the last of them against the next entry
of the final order)."""
import math

import numpy as np

import ctc_beam_ctx_reference as X
import ctc_beam_lm_reference as M
import rnnt_beam_reference as R

MARGIN = R.MARGIN
BOS = EOS = 0              # the kernel tests' sentence marks: the blank's id, which no hypothesis holds
ALPHA, BETA, GAMMA = 0.5, 0.3, 1.5


class State:
    """lm, len, state and credit of a label sequence, by the recursions of the definition, memoised."""

    def __init__(self, lm=None, bos=BOS, eos=EOS, graph=None):
        self.lm, self.bos, self.eos, self.graph = lm, bos, eos, graph
        self.score = M._Scorer(lm, bos) if lm is not None else None
        self.credit = X._Credit(graph) if graph is not None else None

    def lm_of(self, y):
        return self.score(tuple(y)) if self.score is not None else 0.0

    def end_of(self, y):
        return self.score.end(tuple(y), self.eos) if self.score is not None else 0.0

    def cnt_of(self, y):
        return self.credit(tuple(y))[1] if self.credit is not None else 0

    def earned_of(self, y):
        return self.credit.earned(tuple(y)) if self.credit is not None else 0


def bonus(alpha, beta, gamma, lm, n, cnt):
    return (alpha * lm + beta * n) + X.bonus32(gamma, cnt)


def search(row, Tb, V, W, K=0, S=5, nbest=1, C=2, blank=R.BLANK, sos=R.SOS, dtype=np.float64, lm=None, alpha=0.0, beta=0.0, bos=BOS,
           eos=EOS, graph=None, gamma=0.0):
    """-> dict(hyps [(y tuple, score, lm with the end term, earned credit)] best first (at most nbest), keys (their final keys), last_d
    [(y, score)] = the last frame's D in rank order, margins {topk, cand, beam, order}, pruned, maxabs) -- rnnt_beam_reference.search's
    form with the two fused values behind every hypothesis."""
    K = int(K) if K else min(V - 1, 16)
    assert 1 <= K < V and W >= 1 and S >= 1 and 1 <= nbest <= W
    st = State(lm, bos, eos, graph)

    def f(y, sc):
        return float(sc) + bonus(alpha, beta, gamma, st.lm_of(y), len(y), st.cnt_of(y))

    A = [((), dtype(0.0))]
    margins = dict(topk=math.inf, cand=math.inf, beam=math.inf, order=math.inf)
    pruned, maxabs, last_d = False, 0.0, []
    for t in range(max(0, int(Tb))):
        Cs, D = A, {}
        for s in range(S + 1):
            rows = []
            for y, sc in Cs:
                x = np.asarray(row(t, R.context(y, C, sos)), dtype=dtype)
                assert x.shape == (V,)
                lp = R.log_softmax(x)
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
                    v = dtype(sc + lp[k])
                    cands.append((f(y + (k,), v), r, k, y + (k,), v))
                    maxabs = max(maxabs, abs(float(lp[k])))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            if len(cands) > W:
                pruned = True
                margins["cand"] = min(margins["cand"], float(cands[W - 1][0] - cands[W][0]))
            Cs = [(c[3], c[4]) for c in cands[:W]]
        items = list(D.items())
        keys = [f(y, sc) for y, sc in items]
        order = sorted(range(len(items)), key=lambda i: (-keys[i], i))
        if len(order) > W:
            pruned = True
            margins["beam"] = min(margins["beam"], float(keys[order[W - 1]] - keys[order[W]]))
        last_d = [items[i] for i in order]
        A = last_d[:W]
    fin = []
    for i, (y, sc) in enumerate(A):
        lmv, cr = st.lm_of(y) + st.end_of(y), st.earned_of(y)
        fin.append((float(sc) + bonus(alpha, beta, gamma, lmv, len(y), cr), i, tuple(y), sc, lmv, cr))
    fin.sort(key=lambda e: (-e[0], e[1]))
    for i in range(min(len(fin) - 1, nbest)):
        margins["order"] = min(margins["order"], float(fin[i][0] - fin[i + 1][0]))
    return dict(hyps=[(e[2], e[3], e[4], e[5]) for e in fin[:nbest]], keys=[e[0] for e in fin[:nbest]], last_d=last_d, margins=margins,
                pruned=pruned, maxabs=maxabs)


def min_margin(res):
    return min(res["margins"].values())


def as_arrays(results, nbest, L, blank=R.BLANK):
    """The kernel's output form: rnnt_beam_reference.as_arrays' three and lm (B,nbest) float64, credit (B,nbest) int32, both 0 where there
    is no hypothesis."""
    ids, lens, sc = R.as_arrays([dict(hyps=[(h[0], h[1]) for h in res["hyps"]]) for res in results], nbest, L, blank)
    lm = np.zeros((len(results), nbest), dtype=np.float64)
    credit = np.zeros((len(results), nbest), dtype=np.int32)
    for b, res in enumerate(results):
        for n, h in enumerate(res["hyps"]):
            lm[b, n], credit[b, n] = h[2], h[3]
    return ids, lens, sc, lm, credit


# ------------------------------------------------------------------------------------------------ the tests' tables and inputs
def synthetic_lm(V, order):
    """ctc_beam_lm_reference's Witten-Bell LM over the ids 1..V-1 with bos = eos = 0 (a unigram for every label)."""
    return M.synthetic_lm(V, order)


def graph_of(phrases, V):
    return X.graph_of(phrases, V)


def random_graph(V, seed, n=6):
    """n random phrases of one to three labels over 2..V-1, some with a shared first label (failure links and broken-off matches)."""
    g = np.random.default_rng(seed)
    phrases = [g.integers(2, V, size=int(g.integers(1, 4))).tolist() for _ in range(n)]
    phrases += [[p[0]] + p for p in phrases[:2]]
    return graph_of(phrases, V)


def survival_case():
    """Hand-set parameters (B 1, T 2, J 8, V 5, C 1), to be searched with W 2, K 3, S 1.  Joint dimension 0 carries the frame (+1, -1),
    dimension 1 whether the context is still SOS (+1) or a label (-1), both saturated by the tanh (rnnt_beam_reference.merge_case):
        frame 0 from ():   logits blank -1, label 2 2.0, label 4 1.5, label 3 1.0: the plain beam of two keeps [2] and [4] and drops
                           [3] for good
        frame 1 from ():   the blank far ahead (6), the labels near -2
        after a label:     the blank ten higher than from (): blank ~1, nothing is appended
    The plain 2-best is [2], [4].  With the phrase [3] (gamma 3), or with an LM that has seen 3 open nearly every sentence (alpha 2), the
    candidate [3] passes both WHILE the candidates are pruned: it is in the fused arms' n-best, and no rescoring of the plain search's
    n-best could have found it."""
    e = np.zeros((1, 2, 8), dtype=np.float32)
    e[0, 0, 0], e[0, 1, 0] = 20.0, -20.0
    tab = np.zeros((5, 8), dtype=np.float32)
    tab[:, 1] = -20.0
    tab[R.SOS, 1] = 20.0
    f0 = np.array([-1.0, -20.0, 2.0, 1.0, 1.5])
    f1 = np.array([6.0, -20.0, -2.0, -2.25, -2.5])
    w_out = np.zeros((5, 8), dtype=np.float32)
    w_out[:, 0] = (f0 - f1) / 2.0                  # logit from () = w[:, 0] * (+1 | -1) + (f0 + f1) / 2
    w_out[0, 1] = -5.0
    b_out = ((f0 + f1) / 2.0).astype(np.float32)
    b_out[0] += 5.0                                # the blank: unchanged from (), + 10 after a label
    return dict(e=e, tables=[tab], w_out=w_out, b_out=b_out)


def survival_lm():
    from utils.ngram import NgramLM
    return NgramLM.estimate([[3]] * 40 + [[2]] + [[4, 3]] * 2, 5, 2, BOS, EOS)
