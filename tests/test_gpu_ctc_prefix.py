"""asr_ctc_prefix_init / asr_ctc_prefix_step (csrc/ctc_prefix.hip) against the float64 host scorer of tests/ctc_prefix_reference.py
(pinned by tests/test_ctc_prefix_host.py).  GPU and reference run in lockstep through init, step and select; between steps the frames
>= T_b of the GPU state are overwritten with NaN, so a kernel that read them would show it in the next step's scores.

Bound: -inf patterns identical; finite psi and both state arrays within 2e-5 * max(1, |ref|), the project's bound for the CTC lattice
(tests/test_gpu_ctc.py); an fp32 run of the same sequential recursion stays within 4e-7 * |ref| of float64 on these shapes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_prefix_reference as R

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _close(got, ref, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), what
    inf_g, inf_r = np.isneginf(got), np.isneginf(ref)
    assert np.array_equal(inf_g, inf_r), (what, int(inf_g.sum()), int(inf_r.sum()))
    assert np.isfinite(got[~inf_r]).all(), what
    err = np.abs(got[~inf_r] - ref[~inf_r]) / np.maximum(1.0, np.abs(ref[~inf_r]))
    worst = float(err.max()) if err.size else 0.0
    print("%s: worst relative error %.3e over %d finite values, %d -inf" % (what, worst, err.size, int(inf_r.sum())))
    assert worst <= TOL, (what, worst)


class Lockstep:
    """The GPU scorer (ops level) and the reference on the same logits, rows and candidates."""

    def __init__(self, logits, frames, row_utt, ld_pad=0):
        from asr_hip import ops
        self.ops = ops
        B, T, V = logits.shape
        self.frames, self.row_utt = list(frames), list(row_utt)
        self.lp64 = R.log_softmax(logits.double().numpy())
        self.st64 = R.init_state(self.lp64, self.frames, self.row_utt)
        dev = torch.device("cuda")
        if ld_pad:                                   # a row stride above V: the logits as a view of a wider buffer
            wide = torch.full((B, T, V + ld_pad), 50.0)
            wide[..., :V] = logits
            g = wide.to(dev)[..., :V]
        else:
            g = logits.to(dev)
        self.frames_d = torch.tensor(self.frames, dtype=torch.int32, device=dev)
        self.utt_d = torch.tensor(self.row_utt, dtype=torch.int32, device=dev)
        self.lp, self.st = ops.ctc_prefix_init(g, self.frames_d, self.utt_d)
        _close(self.lp.cpu().numpy(), self.lp64, "lp")
        self._check_state(self.st.cpu().numpy()[:, None], self.st64[:, None], "initial state")
        self._poison()

    def _tb(self, r):
        return self.frames[self.row_utt[r]]

    def _check_state(self, got, ref, what):
        # frames >= T_b are not part of the contract (never written, never read): compare frames < T_b of every row
        for r in range(ref.shape[0]):
            Tb = self._tb(r)
            _close(got[r, :, :Tb], ref[r, :, :Tb], "%s row %d" % (what, r))

    def _poison(self):
        for r in range(len(self.row_utt)):
            self.st[r, self._tb(r):] = float("nan")

    def step(self, last, first, cand, what):
        dev = self.st.device
        psi, new = self.ops.ctc_prefix_step(self.lp, self.frames_d, self.st, self.utt_d,
                                            torch.tensor(last, dtype=torch.int64, device=dev),
                                            torch.tensor([int(f) for f in first], dtype=torch.int32, device=dev),
                                            torch.tensor(cand, dtype=torch.int64, device=dev))
        psi64, new64 = R.step(self.lp64, self.frames, self.st64, self.row_utt, last, first, cand)
        _close(psi.cpu().numpy(), psi64, what + " psi")
        self._check_state(new.cpu().numpy(), new64, what + " state")
        self.new, self.new64 = new, new64
        return psi64

    def select(self, flat):
        Rr, K, T, _ = self.new.shape
        self.st = self.new.view(Rr * K, T, 2).index_select(0, torch.tensor(flat, dtype=torch.int64, device=self.new.device))
        self.st64 = R.select(self.new64, flat)
        self._poison()


def _logits(B, T, V, seed):
    return torch.randn(B, T, V, generator=torch.Generator().manual_seed(seed)) * 2.0


def test_every_candidate_kind_over_three_extensions():
    """B 3, T' 12, V 7, K = V (blank, SOS and EOS are among the candidates), T_b = [12, 5, 1]: the first step (empty prefix), a step with
    c == last for one candidate of every row, and a third extension of states that came out of the kernel and through the select.  The
    one-frame utterance cannot hold a second label: -inf from the second step on."""
    B, T, V = 3, 12, 7
    row_utt = [0, 0, 1, 1, 2, 2]
    ls = Lockstep(_logits(B, T, V, 11), [12, 5, 1], row_utt, ld_pad=3)
    rng = np.random.default_rng(0)
    cand = [list(rng.permutation(V)) for _ in row_utt]
    psi = ls.step([R.SOS] * 6, [True] * 6, cand, "step 1")
    assert all(np.isneginf(psi[r, cand[r].index(x)]) for r in range(6) for x in (R.BLANK, R.SOS))
    assert all(psi[r, cand[r].index(R.EOS)] > -np.inf for r in range(6))       # p(empty sequence) = all blanks
    picks = [3, 4, 5, 3, 6, 4]                                                # the label every row continues with
    ls.select([r * V + cand[r].index(picks[r]) for r in range(6)])
    cand = [list(rng.permutation(V)) for _ in row_utt]
    psi = ls.step(picks, [False] * 6, cand, "step 2")
    assert np.isneginf(psi[4:]).sum() >= 2 * (V - 1)                           # T_b = 1: only EOS is left
    picks2 = [3, 5, 5, 3, 3, 4]                                               # rows 0 and 3 repeat their label (c == last)
    ls.select([r * V + cand[r].index(picks2[r]) for r in range(6)])
    cand = [list(rng.permutation(V)) for _ in row_utt]
    psi = ls.step(picks2, [False] * 6, cand, "step 3")
    assert np.isfinite(psi[0]).sum() >= 4 and np.isneginf(psi[4:]).all()       # T_b = 1 holds one label: "3 3" / "4 4" is impossible


def test_wave_straddles_rows_and_utterances():
    """R = 7 rows of K = 10 candidates: 70 lanes, the first wave ends inside row 6 and spans all three utterances."""
    B, T, V, K = 3, 12, 11, 10
    row_utt = [0, 0, 0, 1, 1, 2, 2]
    ls = Lockstep(_logits(B, T, V, 12), [12, 5, 7], row_utt)
    rng = np.random.default_rng(1)
    cand = [list(rng.permutation(V)[:K]) for _ in row_utt]
    ls.step([R.SOS] * 7, [True] * 7, cand, "step 1")
    picks = []
    for c in cand:
        picks.append(next(x for x in c if x > R.EOS))
    ls.select([r * K + cand[r].index(picks[r]) for r in range(7)])
    cand = [[picks[r]] + [x for x in rng.permutation(V) if x != picks[r]][:K - 1] for r in range(7)]      # c == last in slot 0
    ls.step(picks, [False] * 7, cand, "step 2")


def test_benchmark_vocabulary():
    """V 4364, T' 100, K 16 (the widest candidate list the library takes), ragged frames."""
    B, T, V, K = 2, 100, 4364, 16
    row_utt = [0, 0, 1, 1]
    ls = Lockstep(_logits(B, T, V, 13), [100, 73], row_utt)
    rng = np.random.default_rng(2)
    cand = [[int(x) for x in rng.choice(np.arange(3, V), size=K, replace=False)] for _ in row_utt]
    cand[0][5], cand[3][0] = R.EOS, R.BLANK
    ls.step([R.SOS] * 4, [True] * 4, cand, "step 1")
    picks = [cand[r][1] for r in range(4)]
    ls.select([r * K + 1 for r in range(4)])
    cand = [[int(x) for x in rng.choice(np.arange(3, V), size=K, replace=False)] for _ in row_utt]
    for r in range(4):
        cand[r][7] = picks[r]
    cand[2][0] = R.EOS
    ls.step(picks, [False] * 4, cand, "step 2")


def test_long_sequence_label_by_label_equals_ctc_loss():
    """T' 300, V 32: one 140-label sequence with repeats, scored label by label through init, step and select; the final EOS score is
    -F.ctc_loss(sum) in float64."""
    T, V, L, K = 300, 32, 140, 2
    logits = _logits(1, T, V, 14)
    rng = np.random.default_rng(3)
    seq = rng.integers(3, V, size=L)
    seq[1::2] = seq[0::2][:len(seq[1::2])]
    ls = Lockstep(logits, [T], [0])
    last = R.SOS
    for i, c in enumerate(seq):
        other = int(3 + (c - 3 + 1 + i % (V - 4)) % (V - 3))
        ls.step([last], [i == 0], [[int(c), other]], "label %d" % i)
        ls.select([0])
        last = int(c)
    fin = ls.step([last], [False], [[R.EOS, int(seq[0])]], "eos")[0, 0]
    lp = F.log_softmax(logits[0].double(), dim=1)
    nll = F.ctc_loss(lp.unsqueeze(1), torch.tensor(seq).unsqueeze(0), torch.tensor([T]), torch.tensor([L]), reduction="sum").item()
    assert abs(fin + nll) <= 1e-9                       # the yardstick itself
    from asr_hip import ops                             # and the kernel's last score against torch directly
    got, _ = ops.ctc_prefix_step(ls.lp, ls.frames_d, ls.st, ls.utt_d, torch.tensor([last], device="cuda"),
                                 torch.zeros(1, dtype=torch.int32, device="cuda"), torch.tensor([[R.EOS]], device="cuda"))
    assert abs(got.item() + nll) <= TOL * max(1.0, abs(nll)), (got.item(), -nll)


def test_prefix_that_cannot_fit_is_minus_inf_never_nan():
    """T_b = 3 of 8 frames: "3 3" needs three frames (a blank between the equal labels), a third label has no frame left."""
    ls = Lockstep(_logits(1, 8, 7, 15), [3], [0])
    p1 = ls.step([R.SOS], [True], [[3, 4]], "label 1")
    ls.select([0])
    p2 = ls.step([3], [False], [[3, 4]], "label 2")
    ls.select([0])
    p3 = ls.step([3], [False], [[4, 3, R.EOS]], "label 3")
    assert np.isfinite(p1).all() and np.isfinite(p2).all() and np.isneginf(p3[0, :2]).all() and np.isfinite(p3[0, 2])
    ls.select([0])
    p4 = ls.step([4], [False], [[5, R.EOS]], "label 4")      # every state entry is -inf by now
    assert np.isneginf(p4).all()


def test_more_than_sixteen_candidates_are_refused():
    from asr_hip import lib as L, ops
    dev = torch.device("cuda")
    frames = torch.tensor([4], dtype=torch.int32, device=dev)
    utt = torch.zeros(1, dtype=torch.int32, device=dev)
    lp, st = ops.ctc_prefix_init(_logits(1, 4, 20, 16).to(dev), frames, utt)
    with pytest.raises(L.AsrHipError, match="unsupported|not supported"):
        ops.ctc_prefix_step(lp, frames, st, utt, torch.ones(1, dtype=torch.int64, device=dev), torch.ones(1, dtype=torch.int32, device=dev),
                            torch.arange(3, 20, device=dev).view(1, 17))
