"""Float64 host restatement of the CTC prefix scorer (csrc/ctc_prefix.hip; Watanabe et al. 2017, algorithm 2): init, step, select.
The yardstick of tests/test_gpu_ctc_prefix.py and tests/test_gpu_joint_ctc.py; pinned itself by tests/test_ctc_prefix_host.py against
brute-force enumeration and F.ctc_loss.  numpy only.

  lp (B,T,V) log-probabilities, blank = 0, frames[b] = T_b.  A row's state (T,2) holds (r_n[t], r_b[t]): the log-probability of all
  alignments of its prefix over frames 0..t that end in a non-blank / in a blank.  Frames >= T_b are -inf and never read.
"""
import numpy as np

NEG = -np.inf
BLANK, SOS, EOS = 0, 1, 2


def log_softmax(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def init_state(lp, frames, row_utt, blank=BLANK):
    """-> state (R,T,2) of the empty prefix: r_n = -inf, r_b[t] = sum_{tau <= t} lp[tau, blank]."""
    B, T, V = lp.shape
    st = np.full((len(row_utt), T, 2), NEG)
    for r, u in enumerate(row_utt):
        Tb = int(min(max(int(frames[u]), 0), T))
        st[r, :Tb, 1] = np.cumsum(lp[u, :Tb, blank])
    return st


def _row_step(lp_u, Tb, st, last, first, cands, blank, sos, eos):
    T, V = lp_u.shape
    K = len(cands)
    psi = np.full(K, NEG)
    new = np.full((K, T, 2), NEG)
    if Tb == 0:
        if first:
            psi[cands == eos] = 0.0
        return psi, new
    psi[cands == eos] = np.logaddexp(st[Tb - 1, 0], st[Tb - 1, 1])
    ok = (cands >= 0) & (cands < V) & (cands != blank) & (cands != sos) & (cands != eos)
    c = cands[ok]
    if c.size == 0:
        return psi, new
    same = c == last
    rn = lp_u[0, c].copy() if first else np.full(c.size, NEG)
    rb = np.full(c.size, NEG)
    ps = rn.copy()
    out = np.full((c.size, T, 2), NEG)
    out[:, 0, 0] = rn
    for t in range(1, Tb):
        phi = np.where(same, st[t - 1, 1], np.logaddexp(st[t - 1, 0], st[t - 1, 1]))
        nrn = np.logaddexp(rn, phi) + lp_u[t, c]
        nrb = np.logaddexp(rn, rb) + lp_u[t, blank]
        ps = np.logaddexp(ps, phi + lp_u[t, c])
        rn, rb = nrn, nrb
        out[:, t, 0], out[:, t, 1] = rn, rb
    psi[ok] = ps
    new[ok] = out
    return psi, new


def step(lp, frames, state, row_utt, last, first, cand, blank=BLANK, sos=SOS, eos=EOS):
    """state (R,T,2), last (R), first (R) bool, cand (R,K) -> (psi (R,K), new_state (R,K,T,2))."""
    B, T, V = lp.shape
    cand = np.asarray(cand, dtype=np.int64)
    R, K = cand.shape
    psi = np.full((R, K), NEG)
    new = np.full((R, K, T, 2), NEG)
    with np.errstate(invalid="ignore"):          # logaddexp(-inf, -inf) is -inf; numpy only warns about the inf - inf inside
        for r in range(R):
            u = int(row_utt[r])
            Tb = int(min(max(int(frames[u]), 0), T))
            psi[r], new[r] = _row_step(lp[u], Tb, state[r], int(last[r]), bool(first[r]), cand[r], blank, sos, eos)
    return psi, new


def select(new_state, flat):
    """Survivors: row i of the result continues (row, candidate) pair flat[i] = row * K + k of new_state (R,K,T,2)."""
    R, K, T, _ = new_state.shape
    return new_state.reshape(R * K, T, 2)[np.asarray(flat, dtype=np.int64)].copy()


def score_sequence(lp_u, Tb, seq, eos=EOS):
    """One utterance, one label sequence scored label by label through init, step and select ->
    ([psi of every prefix], psi of the whole sequence = seq . EOS)."""
    lp = lp_u[None]
    frames, row_utt = [Tb], [0]
    st = init_state(lp, frames, row_utt)
    last, out = SOS, []
    for i, c in enumerate(seq):
        psi, new = step(lp, frames, st, row_utt, [last], [i == 0], [[int(c)]])
        out.append(psi[0, 0])
        st = select(new, [0])
        last = int(c)
    fin, _ = step(lp, frames, st, row_utt, [last], [len(seq) == 0], [[eos]])
    return out, fin[0, 0]


class HostPrefixScorer:
    """The scorer object of the beam search (asr_hip.decode.CTCPrefixScorer's interface) on the float64 host recursion."""

    def __init__(self, ctc_logits, frames, row_utt):
        import torch
        self._torch = torch
        self.lp = log_softmax(ctc_logits.detach().double().cpu().numpy())
        self.frames = [int(x) for x in frames]
        self.row_utt = [int(x) for x in row_utt]
        self.state = init_state(self.lp, self.frames, self.row_utt)
        self.new = None

    def step(self, last, cand):
        last = last.cpu().numpy()
        psi, self.new = step(self.lp, self.frames, self.state, self.row_utt, last, last == SOS, cand.cpu().numpy())
        return self._torch.from_numpy(psi)

    def select(self, flat):
        self.state = select(self.new, flat)
