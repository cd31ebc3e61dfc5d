"""Host restatement of CTC prefix beam search (csrc/ctc_beam.hip) in NumPy, pinned by tests/test_ctc_beam_host.py.

The definition, literally (per utterance, over its T_b true frames; blank = PAD; lp(t, v) = logits[t, v] - lse[t], one subtraction in
`dtype`; every log-add is the -inf safe lae2):
  candidates of frame t   the C labels with the largest raw logit, lowest index first among equals; the blank dropped, order kept
  state                   an ordered list of at most W prefixes with p_b, p_nb; before frame 0 [() : p_b = 0, p_nb = -inf]
  step t                  stay slot i:            p_b' = tot + lp(t, blank), p_nb' = p_nb + lp(t, last) (-inf for the empty prefix)
                          extension slot W + j C + k (j-th prefix h, k-th candidate c):
                                                  p_b' = -inf, p_nb' = (p_b(h) if c == last(h) else tot(h)) + lp(t, c)
  merge                   h.c already list[i]: p_nb'(i) = lae2(repeat term, extension term), the extension slot is dead
  prune                   rank by lae2(p_b', p_nb'), greater first, lower slot index first among equals; the best W finite slots, in order
  result                  the first nbest prefixes after frame T_b - 1 with score = lae2(p_b, p_nb)
search(..., dtype=np.float64) is the yardstick of tests/test_gpu_ctc_beam.py; dtype=np.float32 is the kernel's arithmetic (up to the
device's expf / logf), held against it on the host.  W is not limited here (the kernel's limit is 16): the unpruned checks need it large.

Besides the n-best every utterance gets three margins, each a score gap divided by max(1, |the greater score|):
  prune_margin    the smallest gap, over the frames, between the last kept and the first dropped finite slot, and between neighbours of
                  the final n-best: below it, a rounding error may change WHICH prefixes are in the list or their order
  lineage_margin  the smallest gap, over the frames, between the best final hypothesis' ancestor in the list and the first dropped slot
  top_margin      first against second final hypothesis
and `relinked`, the number of merges into a prefix whose parent was pruned and re-created in between (the parent then is a new entry of the
list, the child an old one: only a search that identifies prefixes by their labels still joins them).
(inf where there is nothing to compare with).  cases() are the GPU test's inputs, generated from seeds."""
import functools

import numpy as np

NEG = -np.inf


def lse_rows(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1)
    return m + np.log(np.exp(x - m[..., None]).sum(axis=-1))


def lae2(a, b, dtype=np.float64):
    """log(exp(a) + exp(b)) in `dtype`, -inf safe; the operand order is kept (m + log(exp(a - m) + exp(b - m)))."""
    a, b = dtype(a), dtype(b)
    m = a if a >= b else b
    if m == NEG:
        return dtype(NEG)
    return dtype(m + np.log(dtype(np.exp(dtype(a - m)) + np.exp(dtype(b - m)))))


def candidates(row, C, blank=0):
    """The C largest raw logits of a frame, lowest index first among equals, without the blank."""
    order = np.argsort(-np.asarray(row), kind="stable")[:C]
    return [int(c) for c in order if int(c) != blank]


def step(state, lp, cands, W, C, blank=0, dtype=np.float64):
    """One frame.  state: list of (prefix tuple, p_b, p_nb); lp: the frame's log-probabilities (V) in `dtype`; cands: its candidates.
    -> (new state, slots): slots = [(slot index, prefix, p_b', p_nb', score, origin)] of ALL finite slots in rank order, origin = the
    index in `state` the slot descends from; new state = the first W of them."""
    index = {g: i for i, (g, _, _) in enumerate(state)}
    slots = []
    merged = {}                                        # stay slot i -> the extension term it receives
    ext = []
    for j, (h, pb, pnb) in enumerate(state):
        tot = lae2(pb, pnb, dtype)
        for k, c in enumerate(cands):
            term = dtype((pb if h and h[-1] == c else tot) + lp[c])
            i = index.get(h + (c,))
            if i is not None:
                merged[i] = term                       # (a prefix has one parent: at most one term per stay slot)
            else:
                ext.append((W + j * C + k, h + (c,), dtype(NEG), term, term, j))
    for i, (g, pb, pnb) in enumerate(state):
        npb = dtype(lae2(pb, pnb, dtype) + lp[blank])
        npnb = dtype(pnb + lp[g[-1]]) if g else dtype(NEG)
        if i in merged:
            npnb = lae2(npnb, merged[i], dtype)
        slots.append((i, g, npb, npnb, lae2(npb, npnb, dtype), i))
    slots = [s for s in slots + ext if s[4] > NEG]
    slots.sort(key=lambda s: (-s[4], s[0]))
    return [(s[1], s[2], s[3]) for s in slots[:W]], slots


def _gap(hi, lo):
    return float((float(hi) - float(lo)) / max(1.0, abs(float(hi))))


def search_one(lg, Tb, W, C, nbest=1, blank=0, dtype=np.float64):
    """lg (T,V) (frames >= Tb are never touched) -> dict(seqs: up to nbest label lists, best first; scores; prune_margin, lineage_margin,
    top_margin)."""
    state = [((), dtype(0.0), dtype(NEG))]
    hist = [[]]                                        # per list entry: the score of its ancestor in the list after every frame
    dropped = []                                       # per frame: the score of the first dropped finite slot (-inf: none)
    prune = np.inf
    born = {(): -1}                                    # prefix in the list -> the frame that created this incarnation of it
    parent_born = {}                                   # prefix in the list -> `born` of its parent when it was created
    relinked = 0
    if Tb > 0:
        x = np.asarray(lg[:Tb])
        lse = lse_rows(x).astype(dtype)
        for t in range(Tb):
            lp = (x[t].astype(dtype) - lse[t]).astype(dtype)
            cands = candidates(x[t], C, blank)
            # merges into a prefix whose parent was pruned and re-created since: a search that knows prefixes by the place they were
            # created at, not by their labels, misses exactly these
            relinked += sum(1 for h, _, _ in state for c in cands if h + (c,) in born and parent_born[h + (c,)] != born[h])
            old = {g for g, _, _ in state}
            state, slots = step(state, lp, cands, W, C, blank, dtype)
            for g, _, _ in state:
                if g not in old:
                    born[g], parent_born[g] = t, born[g[:-1]]
            born = {g: born[g] for g, _, _ in state}
            parent_born = {g: parent_born[g] for g, _, _ in state if g}
            hist = [hist[s[5]] + [float(s[4])] for s in slots[:W]]
            if len(slots) > W:
                dropped.append(float(slots[W][4]))
                prune = min(prune, _gap(slots[W - 1][4], slots[W][4]))
            else:
                dropped.append(NEG)
    final = [(list(g), float(lae2(pb, pnb, dtype))) for g, pb, pnb in state[:nbest]]
    for (_, a), (_, b) in zip(final, final[1:]):
        prune = min(prune, _gap(a, b))
    lineage = min([_gap(a, d) for a, d in zip(hist[0], dropped) if d > NEG], default=np.inf)
    top = _gap(final[0][1], final[1][1]) if len(final) > 1 else np.inf
    return dict(seqs=[g for g, _ in final], scores=[s for _, s in final], prune_margin=prune, lineage_margin=lineage, top_margin=top,
                relinked=relinked)


def search(logits, lengths, W, C=0, nbest=1, blank=0, dtype=np.float64):
    """The batch in the kernel's output layout: ids (B,nbest,T) int32 (blank behind the length), lengths (B,nbest) int32 (-1: no such
    hypothesis), scores (B,nbest) float64 (-inf there), and the three margins (B).  Lengths are clamped to [0,T]; C = 0: min(V, 16)."""
    logits = np.asarray(logits)
    B, T, V = logits.shape
    C = C if C else min(V, 16)
    out = dict(ids=np.full((B, nbest, T), blank, dtype=np.int32), lengths=np.full((B, nbest), -1, dtype=np.int32),
               scores=np.full((B, nbest), NEG), prune_margin=np.zeros(B), lineage_margin=np.zeros(B), top_margin=np.zeros(B),
               relinked=np.zeros(B, dtype=np.int64))
    for b in range(B):
        r = search_one(logits[b], max(0, min(T, int(lengths[b]))), W, C, nbest, blank, dtype)
        for n, (g, s) in enumerate(zip(r["seqs"], r["scores"])):
            out["ids"][b, n, :len(g)] = g
            out["lengths"][b, n] = len(g)
            out["scores"][b, n] = s
        for k in ("prune_margin", "lineage_margin", "top_margin", "relinked"):
            out[k][b] = r[k]
    return out


# ------------------------------------------------------------------------------------------------ enumeration (tiny shapes only)
def collapse(frames, blank=0):
    out, prev = [], None
    for c in frames:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return tuple(out)


def enumerate_all(lg, Tb, blank=0):
    """{label sequence: log of the summed probability of ALL its alignments over Tb frames} by brute force (V ** Tb alignments)."""
    import itertools
    V = lg.shape[1]
    lp = np.asarray(lg[:Tb], dtype=np.float64) - lse_rows(lg[:Tb])[:, None] if Tb else None
    acc = {}
    for seq in itertools.product(range(V), repeat=Tb):
        acc.setdefault(collapse(seq, blank), []).append(sum(lp[t, c] for t, c in enumerate(seq)))
    return {g: float(np.logaddexp.reduce(v)) for g, v in acc.items()}


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
DELTA = 4e-5          # twice the score tolerance of the GPU test: a gap smaller than two score errors cannot be decided


def planted(B, T, V, s, seed, lengths=None, blank=0):
    """Standard-normal logits plus s on one planted winner per frame: a label on the label-start frames (3 to 5 frames apart, so that a
    blank fits between any two), held for a second frame at every other start, the blank everywhere else; the second label of every
    utterance repeats the first (a doubled label, found only through the blank between its occurrences).  Purely random logits fill the
    beam with near-tied junk, and near-ties are what a float32 search cannot be held to."""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B, T, V)).astype(np.float32)
    lengths = [T] * B if lengths is None else lengths
    for b in range(B):
        win = np.full(T, blank, dtype=np.int64)
        t, n, first = int(rng.integers(0, 3)), 0, None
        while t < lengths[b]:
            c = int(rng.integers(1, V))
            if n == 0:
                first = c
            elif n == 1:
                c = first
            win[t] = c
            if n % 2 == 1 and t + 1 < T:
                win[t + 1] = c
            n += 1
            t += int(rng.integers(3, 6))
        lg[b, np.arange(T), win] += np.float32(s)
    return lg


def cases():
    """name -> dict(logits (B,T,V) float32, lengths, W, C, nbest, small: every utterance must have prune_margin >= DELTA)."""
    out = {}
    out["exhaustive"] = dict(logits=np.random.default_rng(41).standard_normal((2, 3, 3)).astype(np.float32), lengths=[3, 3], W=16, C=3,
                             nbest=16, small=False)
    tb = [12, 9, 1, 0, 12, 7]
    out["small_w3"] = dict(logits=planted(6, 12, 6, 5.0, 42, tb), lengths=tb, W=3, C=3, nbest=3, small=True)
    tb = [24, 17, 1, 0, 24, 11]
    out["small_w4"] = dict(logits=planted(6, 24, 12, 5.0, 43, tb), lengths=tb, W=4, C=4, nbest=4, small=True)
    tb = [75, 75, 60, 75, 41, 75, 75, 75]
    out["mid"] = dict(logits=planted(8, 75, 40, 6.0, 44, tb), lengths=tb, W=8, C=8, nbest=8, small=False)
    tb = [75, 75, 58, 75]
    out["widest_slot_set"] = dict(logits=planted(4, 75, 4364, 10.0, 45, tb), lengths=tb, W=16, C=16, nbest=16, small=False)
    tb = [400, 333]
    out["long"] = dict(logits=planted(2, 400, 40, 6.0, 46, tb), lengths=tb, W=8, C=16, nbest=8, small=False)
    return out


# Two inputs on which a pruned parent is re-created while its child is still in the list (T 5, V 3, W 4, C 3 and T 6, V 3, W 3, C 3):
# the extension of the new parent must be merged into the old child, else the sequence appears twice and loses probability mass.
RELINK_A = [[-0.6, -0.3, -6.4], [-0.2, -3.1, -2.4], [-0.7, 1.0, -2.0], [-2.6, 1.4, -1.4], [-3.4, 2.3, -1.5]]
RELINK_B = [[2.2, -2.5, 2.6], [-1.0, -0.6, -0.7], [0.7, -0.2, 2.5], [-2.3, 2.3, 0.1], [0.4, -4.5, 0.4], [-0.2, 1.2, -0.3]]
SWEEP_T, SWEEP_DRAWS = 13, 500


@functools.lru_cache(maxsize=None)
def sweep(V, W):
    """Small random-logit utterances (standard normal times 2, T_b 4..13, C = V), SWEEP_DRAWS drawn per (V, W), kept where all three
    margins of the float64 restatement are at least DELTA: random logits prune and re-create prefixes all the time, which the planted
    cases never do.  -> (logits (B,13,V) float32, lengths, the float64 search of the kept utterances with nbest = W)."""
    rng = np.random.default_rng(1000 + 10 * V + W)
    lg = (rng.standard_normal((SWEEP_DRAWS, SWEEP_T, V)) * 2.0).astype(np.float32)
    tb = rng.integers(4, SWEEP_T + 1, size=SWEEP_DRAWS)
    r = search(lg, tb, W, V, W)
    keep = (r["prune_margin"] >= DELTA) & (r["lineage_margin"] >= DELTA) & (r["top_margin"] >= DELTA)
    return lg[keep], tb[keep].tolist(), {k: v[keep] for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def expected(name, dtype="float64"):
    """search() on cases()[name], computed once per process and shared by the tests (treat it as read-only)."""
    c = cases_cached()[name]
    return search(c["logits"], c["lengths"], c["W"], c["C"], c["nbest"], dtype=getattr(np, dtype))


@functools.lru_cache(maxsize=None)
def cases_cached():
    return cases()
