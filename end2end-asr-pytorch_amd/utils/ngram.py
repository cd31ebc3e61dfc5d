"""Label n-gram language model for first-pass fusion in the CTC prefix beam search (csrc/ngram.h, csrc/ctc_beam.hip; DESIGN.md
section 7).  Host only, NumPy: estimation, the query, the file and the device lookup table.

Symbols are label ids 0..V-1, the order N is 1..4.  Counted are the n-grams of [bos] + ids + [eos] that END at a predicted position
(an id or the eos, never the bos), cut at the sentence start: the bos has no unigram count, (bos, x) is a bigram.

Interpolated Witten-Bell, in float64:   n(h) = sum_c n(hc), T(h) = the number of distinct successors of h, h' = h without its first symbol
    P(c | h) = (n(hc) + T(h) P(c | h')) / (n(h) + T(h))          P(c) = (n(c) + T0 / V) / (n + T0) over ALL V ids
so every id has a finite unigram.  Stored per SEEN n-gram g (and per id as a unigram), as float32 natural logs: logp[g] = log P(last of g
| the rest) and bo[g] = log(T(g) / (n(g) + T(g))), 0 at the highest order and for a g nothing follows.  The query is the one
definition of the LM the kernel and the tests use (float32 adds in this order; csrc/ngram.h is the same on the device):
    q(h, c):  acc = 0.f
              for m = len(h) .. 1:  g = last m of h, then c
                                    if g stored: return acc + logp[g]
                                    if (last m of h) stored: acc += bo[last m of h]
              return acc + logp[(c)]                      (-inf for a c that is no id of the table)
An n-gram's key is 64 bits: its ids + 1 in 16-bit fields, the last symbol lowest (ids below 65535); the order is the highest non-zero
field, 0 is "no n-gram".  A context is the key of the last N-1 symbols.  hash_slot() is the hash stated in include/asr_hip.h."""
import numpy as np

MAX_ORDER = 4
MAX_ID = 65534                                   # id + 1 fits 16 bits
HASH_MUL = np.uint64(0x9E3779B97F4A7C15)
NEG = np.float32(-np.inf)


def pack(ids):
    """Key of an n-gram / context, oldest symbol first; symbols before the last -1 (no symbol, or an id that fits no field) do not
    count."""
    k = 0
    for s in ids:
        k = 0 if s < 0 or s > MAX_ID else (k << 16) | (int(s) + 1)
    return k


def hash_slot(keys, capacity):
    """Home slot of 64-bit keys in a table of `capacity` (a power of two <= 2^31) slots: ((k ^ (k >> 31)) * 0x9E3779B97F4A7C15 mod 2^64)
    >> 32, masked."""
    k = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (k ^ (k >> np.uint64(31))) * HASH_MUL
    return ((h >> np.uint64(32)) & np.uint64(capacity - 1)).astype(np.int64)


def place_keys(keys):
    """Places distinct non-zero keys, ascending, in an open-addressing table with linear probing: -> (slot of every key, capacity,
    max_probe).  The capacity is a power of two >= 16 and twice the entries; max_probe = the most slots a stored key's search reads.
    Entries are placed in rounds: of the pending keys that meet at a free slot the smallest takes it, the others move one slot on."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    cap = 16
    while cap < 2 * n:
        cap *= 2
    taken = np.zeros(cap, dtype=bool)
    home = hash_slot(keys, cap)
    pos, pending = home.copy(), np.arange(n)
    while pending.size:
        p = pos[pending]
        free = ~taken[p]
        slots, first = np.unique(p[free], return_index=True)           # pending is ascending in key order: the first is the smallest
        won = pending[free][first]
        taken[slots] = True
        placed = np.zeros(n, dtype=bool)
        placed[won] = True
        pending = pending[~placed[pending]]
        pos[pending] = (pos[pending] + 1) & (cap - 1)
    max_probe = int((((pos - home) & (cap - 1)) + 1).max()) if n else 1
    return pos, cap, max_probe


class NgramLM:
    def __init__(self, order, V, labels, keys, logp, bo):
        self.order, self.V, self.labels = int(order), int(V), list(labels)
        self.keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.lp = np.ascontiguousarray(logp, dtype=np.float32)
        self.bo = np.ascontiguousarray(bo, dtype=np.float32)
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError("n-gram order must lie in 1..%d, got %d" % (MAX_ORDER, self.order))
        if not 1 <= self.V <= MAX_ID + 1:
            raise ValueError("label ids must be below 65535 (16-bit key fields), got V = %d" % self.V)
        if len(self.labels) != self.V or not (len(self.keys) == len(self.lp) == len(self.bo)):
            raise ValueError("inconsistent n-gram arrays")
        self._map = {int(k): (l, b) for k, l, b in zip(self.keys.tolist(), self.lp, self.bo)}
        self._tables = {}

    # ------------------------------------------------------------------------------------------------ estimation
    @classmethod
    def estimate(cls, sentences, V, order, bos, eos, labels=None):
        """sentences: id lists (no bos / eos).  Deterministic: the arrays are sorted by key."""
        V, order = int(V), int(order)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError("n-gram order must lie in 1..%d, got %d" % (MAX_ORDER, order))
        if V > MAX_ID + 1:
            raise ValueError("label ids must be below 65535 (16-bit key fields), got V = %d" % V)
        count = [dict() for _ in range(order + 1)]           # count[k][key of a k-gram]
        for ids in sentences:
            w = [int(bos)] + [int(x) for x in ids] + [int(eos)]
            if min(w) < 0 or max(w) >= V:
                raise ValueError("a symbol outside 0..%d" % (V - 1))
            for i in range(1, len(w)):
                for k in range(1, min(order, i + 1) + 1):
                    g = pack(w[i - k + 1:i + 1])
                    count[k][g] = count[k].get(g, 0) + 1
        # n(h) and T(h) of every context h (a k-gram, k < order; the bos alone is one, though it is no counted unigram)
        n_ctx, t_ctx = {}, {}
        for k in range(2, order + 1):
            for g, n in count[k].items():
                h = g >> 16
                n_ctx[h] = n_ctx.get(h, 0) + n
                t_ctx[h] = t_ctx.get(h, 0) + 1
        n1, t0 = sum(count[1].values()), len(count[1])
        prob = {}                                            # key -> P(last | rest), float64
        for c in range(V):
            prob[c + 1] = (count[1].get(c + 1, 0) + t0 / V) / (n1 + t0) if n1 + t0 else 1.0 / V
        for k in range(2, order + 1):
            for g, n in count[k].items():
                h = g >> 16
                lower = g & ((1 << (16 * (k - 1))) - 1)      # h' then c: seen whenever g is
                prob[g] = (n + t_ctx[h] * prob[lower]) / (n_ctx[h] + t_ctx[h])
        keys = sorted(prob)
        top = 1 << (16 * (order - 1))
        bo = [np.log(t_ctx[g] / (n_ctx[g] + t_ctx[g])) if g < top and g in t_ctx else 0.0 for g in keys]
        return cls(order, V, labels if labels is not None else [str(i) for i in range(V)], np.array(keys, dtype=np.uint64),
                   np.log(np.array([prob[g] for g in keys], dtype=np.float64)).astype(np.float32), np.array(bo, dtype=np.float32))

    # ------------------------------------------------------------------------------------------------ the query
    def context(self, ids):
        """Key of the last order-1 symbols of `ids`."""
        n = self.order - 1
        return pack(list(ids)[-n:]) if n else 0

    def logp_key(self, ctx, c):
        """q(context key, c) in float32."""
        c = int(c)
        if not 0 <= c <= MAX_ID:
            return NEG
        acc = np.float32(0.0)
        m = 0
        while m < self.order - 1 and (ctx >> (16 * m)) & 0xffff:
            m += 1
        for m in range(m, 0, -1):
            h = ctx & ((1 << (16 * m)) - 1)
            e = self._map.get((h << 16) | (c + 1))
            if e is not None:
                return np.float32(acc + e[0])
            e = self._map.get(h)
            if e is not None:
                acc = np.float32(acc + e[1])
        e = self._map.get(c + 1)
        return np.float32(acc + e[0]) if e is not None else NEG

    def logp(self, ctx, c):
        """q(h, c): ctx = the symbols before c, oldest first (-1: no symbol; only the last order-1 count)."""
        return self.logp_key(self.context(ctx), c)

    def score(self, ids, bos, eos=None):
        """Sum of q over `ids` after [bos], and over the eos (None or -1: no end term), in float64."""
        seq = [int(bos)] + [int(x) for x in ids]
        tot = 0.0
        for i in range(1, len(seq)):
            tot += float(self.logp(seq[:i], seq[i]))
        if eos is not None and eos >= 0:
            tot += float(self.logp(seq, eos))
        return tot

    # ------------------------------------------------------------------------------------------------ the file
    def save(self, path):
        import torch
        torch.save({"order": self.order, "V": self.V, "labels": list(self.labels), "keys": torch.from_numpy(self.keys.view(np.int64).copy()),
                    "logp": torch.from_numpy(self.lp.copy()), "bo": torch.from_numpy(self.bo.copy())}, path)

    @classmethod
    def load(cls, path, id2label=None):
        """id2label (a list, or a dict id -> label): the model's labels; a file made for other labels is refused."""
        import torch
        ck = torch.load(path, map_location="cpu", weights_only=True)
        lm = cls(ck["order"], ck["V"], ck["labels"], ck["keys"].numpy().view(np.uint64), ck["logp"].numpy(), ck["bo"].numpy())
        if id2label is not None:
            lm.check_labels(id2label)
        return lm

    def check_labels(self, id2label):
        want = [id2label[i] for i in range(len(id2label))]
        if want != self.labels:
            raise ValueError("the n-gram LM was estimated for another label file (%d labels, the model has %d%s)" % (
                len(self.labels), len(want), "" if len(want) != len(self.labels) else "; they differ"))

    # ------------------------------------------------------------------------------------------------ the device table
    def hash_table(self):
        """-> (keys (capacity) uint64, vals (capacity, 2) float32 = (logp, bo), max_probe): open addressing, linear probing, capacity a
        power of two >= twice the entries, key 0 = empty; max_probe = the most slots a stored key's search reads.  Entries are placed in
        rounds: of the pending keys that meet at a free slot the smallest takes it, the others move one slot on.  Same arrays, same bytes."""
        slots, cap, max_probe = place_keys(self.keys)
        keys, vals = np.zeros(cap, dtype=np.uint64), np.zeros((cap, 2), dtype=np.float32)
        keys[slots] = self.keys
        vals[slots, 0], vals[slots, 1] = self.lp, self.bo
        return keys, vals, max_probe

    def find(self, table, key):
        """Slot of `key` in a hash_table() result, or -1: the search the device runs (at most max_probe slots, an empty slot ends it)."""
        keys, _, max_probe = table
        cap = len(keys)
        s = int(hash_slot(np.array([key], dtype=np.uint64), cap)[0])
        for _ in range(max_probe):
            if int(keys[s]) == key:
                return s
            if int(keys[s]) == 0:
                return -1
            s = (s + 1) & (cap - 1)
        return -1

    def device_table(self, device):
        """dict(keys int64 (capacity) [the uint64 bits], vals float32 (capacity, 2), capacity, max_probe, order) on `device`, built once
        per device and cached."""
        import torch
        dev = torch.device(device)
        t = self._tables.get(dev)
        if t is None:
            keys, vals, max_probe = self.hash_table()
            t = self._tables[dev] = dict(keys=torch.from_numpy(keys.view(np.int64)).to(dev), vals=torch.from_numpy(vals).to(dev),
                                         capacity=len(keys), max_probe=max_probe, order=self.order)
        return t


def encode_transcript(text, label2id):
    """Label ids of a transcript as utils/data_loader.py maps it: characters outside the label file and id 0 are dropped (SOS / EOS
    characters in the text likewise: the LM adds its own)."""
    from utils import constant
    ids = [label2id.get(c) for c in text]
    return [i for i in ids if i and i not in (constant.SOS_TOKEN, constant.EOS_TOKEN)]
