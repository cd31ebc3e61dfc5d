"""Host restatement of the phrase arms of the CTC prefix beam search (asr_ctc_beam_search_ctx, csrc/ctc_beam.hip) in
float64, pinned by tests/test_context_host.py.  It extends tests/ctc_beam_lm_reference.py (and through it tests/ctc_beam_reference.py),
whose definitions hold for everything not said here.  The phrase automaton is utils.context.ContextGraph: state and credit of a prefix
are functions of its labels alone and are looked up by the prefix here.

  state    every list entry also carries cst = state(prefix) and cnt = credit(prefix); before frame 0: eps and 0
  prune    slots ranked by f = tot + ((alpha lm + beta len) + gamma cnt); without an LM lm is 0 and len still counts; gamma cnt is the
           float32 product the kernel forms (gamma times an integer: the kernel, the host and this file get the same bits), the other
           terms and the sums are float64 as in the LM arm's restatement; greater first, lower slot index first among equals; live iff tot
           is finite
  result   the W entries ordered by the same key with earned = cnt - hold(cst) in place of cnt, + alpha q(ctx, eos) with an LM and an
           end term; the list position first among equals.  The first nbest: scores = tot, lm = the lm sum with the end term (0 without an
           LM), credit = earned

The three margins are those of ctc_beam_lm_reference, taken on this key; search_one also returns `recreated`, the prefixes that entered
the list again after they had been pruned.  `fused` = alpha lm + beta len + gamma earned of every
hypothesis, `keys` its final key."""
import functools

import numpy as np

import ctc_beam_lm_reference as M
import ctc_beam_reference as R
from ctc_beam_reference import DELTA, _gap, candidates, lae2, lse_rows

NEG = -np.inf
GAMMA = 1.5
RESERVED = (0,)        # the kernel tests' blank, bos and eos: id 0, which no phrase may hold


def bonus32(gamma, n):
    return float(np.float32(gamma) * np.float32(n))


class _Credit:
    """(state, credit) of a prefix by the recursion of the definition, memoised."""

    def __init__(self, graph):
        self.graph, self.memo = graph, {(): (0, 0)}

    def __call__(self, g):
        v = self.memo.get(g)
        if v is None:
            s, n = self(g[:-1])
            t, d = self.graph.step(s, g[-1])
            v = self.memo[g] = (t, n + d)
        return v

    def earned(self, g):
        s, n = self(g)
        return n - int(self.graph.hold[s])


def search_one(lg, Tb, W, C, nbest, graph, gamma, lm=None, alpha=0.0, beta=0.0, bos=0, eos=-1, blank=0):
    """-> dict(seqs, scores (tot), lm, credit (earned), fused, keys of up to nbest hypotheses, best first; prune_margin, lineage_margin,
    top_margin)."""
    score = M._Scorer(lm, bos) if lm is not None else None
    credit = _Credit(graph)

    def lm_of(g):
        return score(g) if score is not None else 0.0

    def end_of(g):
        return score.end(g, eos) if score is not None else 0.0

    def key(g, tot):
        return float(tot) + ((alpha * lm_of(g) + beta * len(g)) + bonus32(gamma, credit(g)[1]))

    state = [((), np.float64(0.0), np.float64(NEG))]
    hist, dropped, prune = [[]], [], np.inf
    ever, recreated = {()}, []                         # every prefix that has been in the list; those that came back after a pruning
    if Tb > 0:
        x = np.asarray(lg[:Tb])
        lse = lse_rows(x)
        for t in range(Tb):
            lp = x[t].astype(np.float64) - lse[t]
            old = {g for g, _, _ in state}
            state, slots = M.step(state, lp, candidates(x[t], C, blank), W, C, key, blank)
            recreated += [g for g, _, _ in state if g not in old and g in ever]
            ever.update(g for g, _, _ in state)
            hist = [hist[s[5]] + [s[6]] for s in slots[:W]]
            if len(slots) > W:
                dropped.append(slots[W][6])
                prune = min(prune, _gap(slots[W - 1][6], slots[W][6]))
            else:
                dropped.append(NEG)
    final = []
    for i, (g, pb, pnb) in enumerate(state):
        tot = float(lae2(pb, pnb))
        k = tot + ((alpha * lm_of(g) + beta * len(g)) + bonus32(gamma, credit.earned(g)))
        final.append((k + alpha * end_of(g), i, g, tot, lm_of(g) + end_of(g), credit.earned(g)))
    final.sort(key=lambda e: (-e[0], e[1]))
    for a, b in zip(final, final[1:]):
        prune = min(prune, _gap(a[0], b[0]))
    lineage = min([_gap(a, d) for a, d in zip(hist[final[0][1]], dropped) if d > NEG], default=np.inf)
    top = _gap(final[0][0], final[1][0]) if len(final) > 1 else np.inf
    final = final[:nbest]
    return dict(seqs=[list(e[2]) for e in final], scores=[e[3] for e in final], lm=[e[4] for e in final], credit=[e[5] for e in final],
                fused=[alpha * e[4] + beta * len(e[2]) + gamma * e[5] for e in final], keys=[e[0] for e in final], prune_margin=prune,
                lineage_margin=lineage, top_margin=top, recreated=recreated)


def search(logits, lengths, W, C, nbest, graph, gamma, lm=None, alpha=0.0, beta=0.0, bos=0, eos=-1, blank=0):
    """The batch in the kernel's output layout (ctc_beam_lm_reference.search) plus credit (B,nbest) int32, -1 where there is no
    hypothesis.  C = 0: min(V, 16)."""
    logits = np.asarray(logits)
    B, T, V = logits.shape
    C = C if C else min(V, 16)
    out = dict(ids=np.full((B, nbest, T), blank, dtype=np.int32), lengths=np.full((B, nbest), -1, dtype=np.int32),
               credit=np.full((B, nbest), -1, dtype=np.int32), prune_margin=np.zeros(B), lineage_margin=np.zeros(B), top_margin=np.zeros(B))
    for k in ("scores", "lm", "fused", "keys"):
        out[k] = np.full((B, nbest), NEG)
    for b in range(B):
        r = search_one(logits[b], max(0, min(T, int(lengths[b]))), W, C, nbest, graph, gamma, lm, alpha, beta, bos, eos, blank)
        for n, g in enumerate(r["seqs"]):
            out["ids"][b, n, :len(g)] = g
            out["lengths"][b, n] = len(g)
            for k in ("scores", "lm", "fused", "keys", "credit"):
                out[k][b, n] = r[k][n]
        for k in ("prune_margin", "lineage_margin", "top_margin"):
            out[k][b] = r[k]
    return out


# ------------------------------------------------------------------------------------------------ the tests' phrase lists and inputs
def graph_of(phrases, V):
    from utils.context import ContextGraph
    return ContextGraph.from_phrases(phrases, V, reserved=RESERVED)


@functools.lru_cache(maxsize=None)
def case_graph(name, seed=5):
    """A phrase list for ctc_beam_reference.cases()[name]: pieces of one to three labels cut from the plain search's second- and
    third-best hypotheses (so that the bonus moves hypotheses past each other), each piece also with its first label doubled in front
    (a shared suffix: failure links are taken) and with a random label behind it (a shared prefix that breaks off), and four random ones."""
    c, ref = R.cases_cached()[name], R.expected(name)
    V = c["logits"].shape[2]
    rng = np.random.default_rng(seed)
    phrases = []
    for b in range(ref["ids"].shape[0]):
        for n in (1, 2):
            if n < ref["ids"].shape[1] and ref["lengths"][b, n] > 0:
                hyp = ref["ids"][b, n, :ref["lengths"][b, n]].tolist()
                i = int(rng.integers(0, len(hyp)))
                piece = hyp[i:i + int(rng.integers(1, 4))]
                phrases += [piece, [piece[0]] + piece, piece + [int(rng.integers(1, V))]]
    phrases += [rng.integers(1, V, size=int(rng.integers(1, 4))).tolist() for _ in range(4)]
    return graph_of(phrases, V)


@functools.lru_cache(maxsize=None)
def expected(name, order=0, gamma=GAMMA, beta=M.BETA):
    """search() on ctc_beam_reference.cases()[name] with case_graph(name); order 0: phrases only, else with synthetic_lm(V, order),
    alpha M.ALPHA and the end term.  Once per process."""
    c = R.cases_cached()[name]
    lm = M.synthetic_lm(c["logits"].shape[2], order) if order else None
    return search(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], case_graph(name), gamma, lm, M.ALPHA if order else 0.0, beta,
                  M.BOS, M.EOS if order else -1)


SWEEP_DRAWS, SWEEP_GROUPS = 200, 4


@functools.lru_cache(maxsize=None)
def sweep(V, W, order=0):
    """ctc_beam_reference.sweep's generator with SWEEP_DRAWS draws per (V, W) in SWEEP_GROUPS groups, each group under its own list of two
    to four random phrases of one to three labels, gamma 1.5, beta 0.3 (order 3: also the trigram synthetic_lm(V), alpha 0.5), kept where
    all three margins are at least DELTA.  -> [(graph, logits, lengths, the search of the kept utterances with nbest = W)], drawn."""
    rng = np.random.default_rng(3000 + 100 * order + 10 * V + W)
    lg = (rng.standard_normal((SWEEP_DRAWS, 13, V)) * 2.0).astype(np.float32)
    tb = rng.integers(4, 14, size=SWEEP_DRAWS)
    lm = M.synthetic_lm(V, order) if order else None
    out, n = [], SWEEP_DRAWS // SWEEP_GROUPS
    for g in range(SWEEP_GROUPS):
        phrases = [rng.integers(1, V, size=int(rng.integers(1, 4))).tolist() for _ in range(int(rng.integers(2, 5)))]
        graph = graph_of(phrases, V)
        sl = slice(g * n, (g + 1) * n)
        r = search(lg[sl], tb[sl], W, V, W, graph, GAMMA, lm, M.ALPHA if order else 0.0, M.BETA, M.BOS, M.EOS if order else -1)
        keep = (r["prune_margin"] >= DELTA) & (r["lineage_margin"] >= DELTA) & (r["top_margin"] >= DELTA)
        out.append((graph, lg[sl][keep], tb[sl][keep].tolist(), {k: v[keep] for k, v in r.items()}))
    return out


def phrase_decides_case():
    """logits (1,3,4): label 1 leads label 2 by 0.1 in each of three frames; the blank is the likeliest symbol of the outer two (so that
    one label is likelier than two, and 2 x 2 costs more than the second phrase pays) and unlikely in the middle one; the frames differ,
    so that no two sequences tie.  Without a list the best is [1]; with the phrase [2] and gamma 3 it is [2]."""
    lg = np.full((1, 3, 4), -3.0, dtype=np.float32)
    for t, (a, b) in enumerate(zip((2.0, 1.7, 2.3), (4.0, -0.5, 4.3))):
        lg[0, t, 1], lg[0, t, 2], lg[0, t, 0] = a, a - 0.1, b
    return lg


# The re-link inputs of ctc_beam_reference with a phrase list under which a prefix that is pruned and created again stands mid-phrase
# (hold > 0) when it comes back: (logits, W, phrases, gamma, LM order or 0).  RELINK_A re-creates such a prefix only under the trigram.
RELINK = ((R.RELINK_A, 4, [[2, 1, 2, 2]], 0.3, 3), (R.RELINK_B, 3, [[2, 1, 2, 2]], 0.3, 0), (R.RELINK_B, 3, [[2, 1, 2, 2]], 0.3, 3))


def relink_search(case):
    """-> (x (1,T,3), the search of a RELINK entry with nbest = W, its graph, its LM or None, the re-created prefixes)."""
    lg, W, phrases, gamma, order = case
    x = np.array([lg], dtype=np.float32)
    graph, lm = graph_of(phrases, 3), M.synthetic_lm(3, order) if order else None
    args = (graph, gamma, lm, M.ALPHA if order else 0.0, M.BETA, M.BOS, M.EOS if order else -1)
    return x, search(x, [len(lg)], W, 3, W, *args), graph, lm, search_one(x[0], len(lg), W, 3, W, *args)["recreated"]


def unfinished_case():
    """-> (logits (1,4,5), phrases): frames spell 1 then 2; the phrase [1, 2, 3] is two labels in when the utterance ends, [2] is whole.
    With gamma 3 the prefix [1, 2] holds 2 unearned labels while the beam is pruned (key + 6) and none at the end, where [1, 2]'s rivals
    that end in a finished [2] keep theirs: the final order is not the order of the last frame's keys."""
    lg = np.full((1, 4, 5), -2.0, dtype=np.float32)
    lg[0, 0, 1], lg[0, 1, 0], lg[0, 2, 2], lg[0, 3, 0] = 3.0, 2.0, 2.5, 2.0
    lg[0, 0, 4], lg[0, 2, 4] = 2.2, 1.0
    return lg, [[1, 2, 3], [4, 2]]


def deep_pruning_case():
    """-> (logits (1,6,6), phrases, W = 2): at frame 1 label 3 ranks fourth by its CTC score alone, far outside a beam of 2; the phrase
    [3, 4] with gamma 4 keeps the prefix [3] in, and the frames that follow spell 4 clearly, so the best hypothesis is [3, 4].  Rescoring
    the plain search's 2-best cannot find it: [3] is pruned at frame 1."""
    lg = np.full((1, 6, 6), -4.0, dtype=np.float32)
    lg[0, 0, 0] = 3.0
    lg[0, 1, 1], lg[0, 1, 2], lg[0, 1, 0], lg[0, 1, 3] = 3.0, 2.4, 2.0, 1.2
    lg[0, 2, 0] = 3.0
    lg[0, 3, 4], lg[0, 4, 4] = 4.0, 3.5
    lg[0, 5, 0] = 3.0
    lg += (np.random.default_rng(9).standard_normal(lg.shape) * 0.05).astype(np.float32)
    return lg, [[3, 4]], 2
