"""Phrase (hotword) biasing for the CTC prefix beam search (csrc/context.h, csrc/ctc_beam.hip).  Host only, NumPy:
the phrase automaton, its credit, the file and the device lookup table.

A phrase list is a set of label-id sequences over the model's labels, each with at least one label and none with blank / PAD, SOS or
EOS; duplicates merge.  P = all prefixes of all phrases, the empty prefix eps included; u in P is WHOLE if u is itself a phrase.
    state(y)   the longest suffix of the label sequence y that lies in P (the Aho-Corasick state); state(()) = eps
    T(u)       the length of the longest whole prefix of u, u included; 0 if there is none
    hold(u)    |u| - T(u): the labels of a partial match that are not yet earned; 0 for a whole u
    credit(y)  an INTEGER: with s_i = state(y[:i]),  sum over the i with s_i whole of (|s_i| - T(s_i without its last label)) + hold(s_n).
               Per step  delta = e(s') + hold(s') - hold(s),  e(s') = hold(parent(s')) + 1 if s' is whole, else 0
    earned(y)  credit(y) - hold(state(y)): what stays when the utterance ends there
Every label that advances a match earns 1 at once, a match that breaks gives back what it held, a completed phrase keeps its labels for
good.  Overlapping phrases are each credited: with `ab` and `bc`, `abc` earns 4.  A phrase that occurs only strictly inside another's
partial match is not credited, because only the state itself is looked at: with `abcd` and `bc`, `abc...` credits no `bc`.

States are numbered in breadth-first order of the trie of P, eps = 0.  step() is the full goto function (failure links by the usual
breadth-first pass).  The device table (include/asr_hip.h states it) is an open-addressing table of the n-gram table's form that holds
a transition (s, c) only if s = eps or goto(s, c) is neither eps nor goto(eps, c), so it stays near the size of the trie:
    key (s + 1) << 16 | (c + 1), value (next, delta);   lookup: (s, c) stored: its value;  else (eps, c) stored: (next, delta_eps - hold[s]);
    else (eps, -hold[s])
table_step() is that rule on the host; the builder proves it against step() for every stored state before it hands a table out."""
import numpy as np

from utils.ngram import MAX_ID, hash_slot, place_keys


def pack(s, c):
    """Key of the transition (state s, label c)."""
    return (int(s) + 1) << 16 | (int(c) + 1)


class ContextGraph:
    def __init__(self, phrases, V, labels=None):
        """phrases: validated, distinct tuples of ids (from_phrases / from_file make them)."""
        self.V, self.labels = int(V), None if labels is None else list(labels)
        self.phrases = sorted(set(tuple(int(x) for x in p) for p in phrases))
        # the trie of P in breadth-first order
        child, parent, depth, whole = [{}], [0], [0], [False]
        level = [((), 0)]
        by_len = {}
        for p in self.phrases:
            for n in range(1, len(p) + 1):
                by_len.setdefault(n, set()).add(p[:n])
        for n in sorted(by_len):
            index = dict(level)
            level = []
            for u in sorted(by_len[n]):
                s = len(child)
                child[index[u[:-1]]][u[-1]] = s
                child.append({})
                parent.append(index[u[:-1]])
                depth.append(n)
                whole.append(False)
                level.append((u, s))
        for p in self.phrases:
            s = 0
            for c in p:
                s = child[s][c]
            whole[s] = True
        self.child, self.parent, self.depth, self.whole = child, parent, depth, whole
        self.states = len(child)
        # failure links (parents come first in this numbering), T and hold
        fail, tlen = [0] * self.states, [0] * self.states
        for s in range(1, self.states):
            tlen[s] = depth[s] if whole[s] else tlen[parent[s]]
            if parent[s]:
                c = next(k for k, v in child[parent[s]].items() if v == s)
                f = fail[parent[s]]
                while f and c not in child[f]:
                    f = fail[f]
                fail[s] = child[f].get(c, 0)
        self.fail = fail
        self.hold = np.array([d - t for d, t in zip(depth, tlen)], dtype=np.int32)
        self._tables = {}
        self._table = None

    # ------------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_phrases(cls, phrases, V, labels=None, reserved=None):
        """phrases: lists of label ids in 0..V-1.  reserved: ids no phrase may hold (default: PAD / blank, SOS, EOS of utils.constant)."""
        V = int(V)
        if not 1 <= V <= MAX_ID + 1:
            raise ValueError("label ids must be below 65535 (16-bit key fields), got V = %d" % V)
        if reserved is None:
            from utils import constant
            reserved = (constant.PAD_TOKEN, constant.SOS_TOKEN, constant.EOS_TOKEN)
        out = []
        for n, p in enumerate(phrases):
            p = tuple(int(x) for x in p)
            if not p:
                raise ValueError("phrase %d is empty: a phrase has at least one label" % n)
            if min(p) < 0 or max(p) >= V:
                raise ValueError("phrase %d holds a label outside 0..%d" % (n, V - 1))
            if any(x in reserved for x in p):
                raise ValueError("phrase %d holds blank / PAD, SOS or EOS (ids %s): the search never emits them" % (n, sorted(reserved)))
            out.append(p)
        if not out:
            raise ValueError("the phrase list is empty")
        return cls(out, V, labels)

    @classmethod
    def from_file(cls, path, label2id):
        """UTF-8, one phrase per line, lower-cased as the loader lower-cases transcripts; blank lines and lines that start with # are
        skipped.  A character that is no label is refused with its line number."""
        phrases = []
        with open(path, encoding="utf8") as f:
            for n, line in enumerate(f, 1):
                text = line.rstrip("\r\n")
                if not text.strip() or text.lstrip().startswith("#"):
                    continue
                text = text.strip().lower()
                for ch in text:
                    if ch not in label2id:
                        raise ValueError("%s, line %d: %r is not a label of this model" % (path, n, ch))
                phrases.append([label2id[ch] for ch in text])
        if not phrases:
            raise ValueError("%s holds no phrase" % path)
        labels = [None] * len(label2id)
        for ch, i in label2id.items():
            labels[i] = ch
        try:
            return cls.from_phrases(phrases, len(label2id), labels)
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e))

    def check_labels(self, id2label):
        want = [id2label[i] for i in range(len(id2label))]
        if len(want) != self.V or (self.labels is not None and want != self.labels):
            raise ValueError("the phrase list was read for another label file (%d labels, the model has %d%s)" % (
                self.V, len(want), "" if len(want) != self.V else "; they differ"))

    # ------------------------------------------------------------------------------------------------ the automaton
    def goto(self, s, c):
        """The state after label c in state s."""
        while s and c not in self.child[s]:
            s = self.fail[s]
        return self.child[s].get(c, 0)

    def step(self, s, c):
        """-> (next state, delta of the credit)."""
        s, c = int(s), int(c)
        n = self.goto(s, c)
        e = int(self.hold[self.parent[n]]) + 1 if self.whole[n] else 0
        return n, e + int(self.hold[n]) - int(self.hold[s])

    def walk(self, ids, step=None):
        """-> (state(ids), credit(ids)); step: another transition function of step()'s form."""
        step = step or self.step
        s, credit = 0, 0
        for c in ids:
            s, d = step(s, c)
            credit += d
        return s, credit

    def earned(self, ids):
        s, credit = self.walk(ids)
        return credit - int(self.hold[s])

    # ------------------------------------------------------------------------------------------------ the device table
    def transitions(self):
        """The stored transitions, sorted by key: -> (keys uint64, vals (n, 2) int32 = (next, delta))."""
        rows = {}
        for c in self.child[0]:
            rows[pack(0, c)] = self.step(0, c)
        for s in range(1, self.states):
            seen, f = set(), s
            while f:                                   # the labels with a goto other than that of eps: children along the failure chain
                seen.update(self.child[f])
                f = self.fail[f]
            for c in seen:
                n, d = self.step(s, c)
                if n != 0 and n != self.goto(0, c):
                    rows[pack(s, c)] = (n, d)
        keys = sorted(rows)
        return np.array(keys, dtype=np.uint64), np.array([rows[k] for k in keys], dtype=np.int32).reshape(-1, 2)

    def hash_table(self):
        """-> (keys (capacity) uint64, vals (capacity, 2) int32, max_probe): the placement of utils.ngram.place_keys.  Proven before it
        is returned: walk() through table_step() equals walk() through step() on every phrase followed by the next one (every stored
        transition and every kind of fall-through is on those walks), and from every state every label that any state knows, and one
        that none does, steps as step() does -- all of them for a small graph, those along the state's failure chain for a large one."""
        if self._table is None:
            k, v = self.transitions()
            slots, cap, max_probe = place_keys(k)
            keys, vals = np.zeros(cap, dtype=np.uint64), np.zeros((cap, 2), dtype=np.int32)
            keys[slots], vals[slots] = k, v
            table = (keys, vals, max_probe)

            def by_table(s, c):
                return self.table_step(table, s, c)
            for p, q in zip(self.phrases, self.phrases[1:] + self.phrases[:1]):
                for ids in (p + q, p[:-1] + q, p + p):
                    if self.walk(ids, by_table) != self.walk(ids):
                        raise AssertionError("the compressed table walks %s differently from the goto function" % (ids,))
            known = sorted({c for ch in self.child for c in ch})
            small = self.states * len(known) <= 1 << 16
            for s in range(self.states):
                labels, f = set(), s
                while f and not small:
                    labels.update(self.child[f])
                    f = self.fail[f]
                for c in (known if small else sorted(labels)) + [-1]:
                    if by_table(s, c) != self.step(s, c):
                        raise AssertionError("the compressed table disagrees with the goto function at state %d, label %d" % (s, c))
            self._table = table
        return self._table

    def find(self, table, key):
        """Slot of `key` in a hash_table() result, or -1: at most max_probe slots, an empty slot ends the search."""
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

    def table_step(self, table, s, c):
        """step() by the device's rule on a hash_table() result; a label outside 0..65534 or a state outside the table: as from / to eps."""
        s, c = int(s), int(c)
        h = int(self.hold[s]) if 0 <= s < self.states else 0
        if not 0 <= c <= MAX_ID:
            return 0, -h
        if not 0 <= s < self.states:
            s = 0
        i = self.find(table, pack(s, c))
        if i >= 0:
            return int(table[1][i, 0]), int(table[1][i, 1])
        i = self.find(table, pack(0, c))
        if i >= 0:
            return int(table[1][i, 0]), int(table[1][i, 1]) - h
        return 0, -h

    def device_table(self, device):
        """dict(keys int64 (capacity) [the uint64 bits], vals int32 (capacity, 2), hold int32 (states), capacity, max_probe, states) on
        `device`, built once per device and cached."""
        import torch
        dev = torch.device(device)
        t = self._tables.get(dev)
        if t is None:
            keys, vals, max_probe = self.hash_table()
            t = self._tables[dev] = dict(keys=torch.from_numpy(keys.view(np.int64)).to(dev), vals=torch.from_numpy(vals).to(dev),
                                         hold=torch.from_numpy(self.hold).to(dev), capacity=len(keys), max_probe=max_probe,
                                         states=self.states)
        return t
