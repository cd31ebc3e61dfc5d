"""Host restatement of the fused arm of the CTC prefix beam search (asr_ctc_beam_search_lm, csrc/ctc_beam.hip) in
float64, pinned by tests/test_ctc_beam_lm_host.py.  It extends tests/ctc_beam_reference.py, whose definition holds for everything not
said here.  q(h, c) is the query of utils/ngram.py with the table's float32 values widened and added in float64.

  state    every list entry also carries lm = the sum of q over its labels, len, and ctx = the last N-1 symbols of [bos] + prefix (all
           three functions of the label sequence: they are looked up by the prefix here); before frame 0: lm 0, len 0, ctx [bos]
  prune    slots ranked by f = tot + (alpha lm + beta len), tot = lae2(p_b', p_nb'); greater first, lower slot index first among equals;
           live iff tot is finite
  result   the W entries ordered by f + alpha q(ctx, eos) (f alone for eos -1), the list position first among equals; the first nbest:
           scores = tot, lm = the lm sum with the end term

The three margins are taken on the fused key: prune_margin over the frames (last kept against first dropped slot) and between ALL
neighbours of the final order; lineage_margin of the FINALLY best hypothesis' ancestors against the first dropped slot; top_margin first
against second of the final order.  `fused` = alpha lm + beta len of every hypothesis, `keys` its final key."""
import functools

import numpy as np

from ctc_beam_reference import DELTA, _gap, candidates, lae2, lse_rows

NEG = -np.inf


def q64(lm, ctx, c):
    """utils.ngram.NgramLM.logp with float64 adds of the widened float32 values; ctx: symbols, oldest first."""
    key = lm.context(ctx)
    m = 0
    while m < lm.order - 1 and (key >> (16 * m)) & 0xffff:
        m += 1
    acc = 0.0
    for m in range(m, 0, -1):
        h = key & ((1 << (16 * m)) - 1)
        e = lm._map.get((h << 16) | (c + 1))
        if e is not None:
            return acc + float(e[0])
        e = lm._map.get(h)
        if e is not None:
            acc += float(e[1])
    return acc + float(lm._map[c + 1][0])


class _Scorer:
    """lm(prefix) by the recursion of the definition, memoised: the same value however a prefix was reached."""

    def __init__(self, lm, bos):
        self.lm, self.bos, self.memo = lm, bos, {(): 0.0}

    def __call__(self, g):
        v = self.memo.get(g)
        if v is None:
            v = self.memo[g] = self(g[:-1]) + q64(self.lm, (self.bos,) + g[:-1], g[-1])
        return v

    def end(self, g, eos):
        return q64(self.lm, (self.bos,) + g, eos) if eos >= 0 else 0.0


def step(state, lp, cands, W, C, key, blank=0):
    """ctc_beam_reference.step with the slots ranked by key(prefix, tot).  -> (new state, slots): slots = [(slot index, prefix, p_b',
    p_nb', tot, origin, f)] of all live slots in rank order."""
    index = {g: i for i, (g, _, _) in enumerate(state)}
    merged, ext, slots = {}, [], []
    for j, (h, pb, pnb) in enumerate(state):
        tot = lae2(pb, pnb)
        for k, c in enumerate(cands):
            term = np.float64((pb if h and h[-1] == c else tot) + lp[c])
            i = index.get(h + (c,))
            if i is not None:
                merged[i] = term
            else:
                ext.append((W + j * C + k, h + (c,), np.float64(NEG), term, term, j))
    for i, (g, pb, pnb) in enumerate(state):
        npb = np.float64(lae2(pb, pnb) + lp[blank])
        npnb = np.float64(pnb + lp[g[-1]]) if g else np.float64(NEG)
        if i in merged:
            npnb = lae2(npnb, merged[i])
        slots.append((i, g, npb, npnb, lae2(npb, npnb), i))
    slots = [s + (key(s[1], s[4]),) for s in slots + ext if s[4] > NEG]
    slots.sort(key=lambda s: (-s[6], s[0]))
    return [(s[1], s[2], s[3]) for s in slots[:W]], slots


def search_one(lg, Tb, W, C, nbest, lm, alpha, beta, bos, eos, blank=0):
    """-> dict(seqs, scores (tot), lm, fused, keys of up to nbest hypotheses, best first; prune_margin, lineage_margin, top_margin)."""
    score = _Scorer(lm, bos)

    def key(g, tot):
        return float(tot) + (alpha * score(g) + beta * len(g))

    state = [((), np.float64(0.0), np.float64(NEG))]
    hist, dropped, prune = [[]], [], np.inf
    if Tb > 0:
        x = np.asarray(lg[:Tb])
        lse = lse_rows(x)
        for t in range(Tb):
            lp = x[t].astype(np.float64) - lse[t]
            state, slots = step(state, lp, candidates(x[t], C, blank), W, C, key, blank)
            hist = [hist[s[5]] + [s[6]] for s in slots[:W]]
            if len(slots) > W:
                dropped.append(slots[W][6])
                prune = min(prune, _gap(slots[W - 1][6], slots[W][6]))
            else:
                dropped.append(NEG)
    final = []
    for i, (g, pb, pnb) in enumerate(state):
        tot = float(lae2(pb, pnb))
        final.append((key(g, tot) + alpha * score.end(g, eos), i, g, tot, score(g) + score.end(g, eos)))
    final.sort(key=lambda e: (-e[0], e[1]))
    for a, b in zip(final, final[1:]):
        prune = min(prune, _gap(a[0], b[0]))
    lineage = min([_gap(a, d) for a, d in zip(hist[final[0][1]], dropped) if d > NEG], default=np.inf)
    top = _gap(final[0][0], final[1][0]) if len(final) > 1 else np.inf
    final = final[:nbest]
    return dict(seqs=[list(e[2]) for e in final], scores=[e[3] for e in final], lm=[e[4] for e in final],
                fused=[alpha * e[4] + beta * len(e[2]) for e in final], keys=[e[0] for e in final], prune_margin=prune,
                lineage_margin=lineage, top_margin=top)


def search(logits, lengths, W, C, nbest, lm, alpha, beta, bos, eos, blank=0):
    """The batch in the kernel's output layout (ctc_beam_reference.search) plus lm, fused, keys (B,nbest) float64, -inf where there is no
    hypothesis.  C = 0: min(V, 16)."""
    logits = np.asarray(logits)
    B, T, V = logits.shape
    C = C if C else min(V, 16)
    out = dict(ids=np.full((B, nbest, T), blank, dtype=np.int32), lengths=np.full((B, nbest), -1, dtype=np.int32),
               prune_margin=np.zeros(B), lineage_margin=np.zeros(B), top_margin=np.zeros(B))
    for k in ("scores", "lm", "fused", "keys"):
        out[k] = np.full((B, nbest), NEG)
    for b in range(B):
        r = search_one(logits[b], max(0, min(T, int(lengths[b]))), W, C, nbest, lm, alpha, beta, bos, eos, blank)
        for n, g in enumerate(r["seqs"]):
            out["ids"][b, n, :len(g)] = g
            out["lengths"][b, n] = len(g)
            for k in ("scores", "lm", "fused", "keys"):
                out[k][b, n] = r[k][n]
        for k in ("prune_margin", "lineage_margin", "top_margin"):
            out[k][b] = r[k]
    return out


# ------------------------------------------------------------------------------------------------ the tests' LMs and inputs
BOS = EOS = 0          # the kernel tests' sentence marks: the blank's id, which no prefix holds
ALPHA, BETA = 0.5, 0.3
SWEEP_DRAWS = 200


def synthetic_corpus(V, seed, sentences=300, max_len=8):
    """Random sentences over the ids 1..V-1 from a seeded first-order chain with skewed rows: an LM with something to say."""
    rng = np.random.default_rng(seed)
    rows = rng.dirichlet(np.full(V - 1, 0.5), size=V)
    out = []
    for _ in range(sentences):
        prev, s = 0, []
        for _ in range(int(rng.integers(1, max_len + 1))):
            prev = 1 + int(rng.choice(V - 1, p=rows[prev]))
            s.append(prev)
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_lm(V, order=3, seed=7, sentences=300):
    """The Witten-Bell LM of synthetic_corpus with bos = eos = 0, once per process (treat it as read-only)."""
    from utils.ngram import NgramLM
    return NgramLM.estimate(synthetic_corpus(V, seed + 100 * V, sentences), V, order, BOS, EOS)


def lm_decides_case():
    """-> (logits (1,3,4), an LM): label 1 leads label 2 by 0.1 in the one frame that holds a label, and the bigram LM has seen 2 open
    twenty sentences and 1 two: the plain search's best is [1], the fused one's (alpha 0.5) [2]."""
    from utils.ngram import NgramLM
    lg = np.full((1, 3, 4), -3.0, dtype=np.float32)
    lg[0, 0, 1], lg[0, 0, 2] = 2.0, 1.9
    lg[0, 1:, 0] = 4.0
    return lg, NgramLM.estimate([[2]] * 20 + [[1]] * 2 + [[3, 2]] * 3, 4, 2, BOS, EOS)


def beta_decides_case():
    """logits (1,2,3) whose blank holds about 0.8 of every frame: the empty sequence (0.67) beats [1] (0.25) until a bonus of 2 per label
    (the frames differ, so that no two sequences tie)."""
    return np.array([[[2.0, 0.0, -1.0], [2.0, 0.3, -1.2]]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def expected(name, order=3, eos=EOS, alpha=ALPHA, beta=BETA):
    """search() on ctc_beam_reference.cases()[name] with synthetic_lm(V, order), once per process."""
    import ctc_beam_reference as R
    c = R.cases_cached()[name]
    lm = synthetic_lm(c["logits"].shape[2], order)
    return search(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], lm, alpha, beta, BOS, eos)


@functools.lru_cache(maxsize=None)
def sweep(V, W):
    """ctc_beam_reference.sweep's generator with SWEEP_DRAWS draws per (V, W) under the trigram synthetic_lm(V), alpha 0.5, beta 0.3, kept
    where all three margins are at least DELTA.  -> (logits, lengths, the search of the kept utterances with nbest = W, drawn)."""
    rng = np.random.default_rng(2000 + 10 * V + W)
    lg = (rng.standard_normal((SWEEP_DRAWS, 13, V)) * 2.0).astype(np.float32)
    tb = rng.integers(4, 14, size=SWEEP_DRAWS)
    r = search(lg, tb, W, V, W, synthetic_lm(V), ALPHA, BETA, BOS, EOS)
    keep = (r["prune_margin"] >= DELTA) & (r["lineage_margin"] >= DELTA) & (r["top_margin"] >= DELTA)
    return lg[keep], tb[keep].tolist(), {k: v[keep] for k, v in r.items()}
