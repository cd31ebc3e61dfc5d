"""Pins the float64 CTC prefix reference (tests/ctc_prefix_reference.py) before the GPU tests use it as their yardstick: against
brute-force enumeration of every alignment, and against F.ctc_loss for whole sequences (psi(y . EOS) = -nll)."""
import itertools
from collections import defaultdict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_prefix_reference as R


def _lp(T, V, seed):
    rng = np.random.default_rng(seed)
    return R.log_softmax(rng.normal(size=(T, V)) * 2.0), rng


def test_reference_equals_enumeration_of_all_alignments():
    T, V = 5, 4
    lp, _ = _lp(T, V, 0)
    tot = defaultdict(float)                      # collapsed label sequence -> probability, over all 4^5 alignments
    for path in itertools.product(range(V), repeat=T):
        p = float(np.exp(sum(lp[t, path[t]] for t in range(T))))
        col = tuple(k for k, _ in itertools.groupby(path) if k != 0)
        tot[col] += p
    # labels 1..3 of this toy vocabulary are ordinary labels: move SOS / EOS out of the way
    for seq in [(1,), (1, 1), (2, 1, 2), (3, 3), (1, 2, 3)]:
        st = R.init_state(lp[None], [T], [0])
        last = -1
        for i, c in enumerate(seq):
            psi, new = R.step(lp[None], [T], st, [0], [last], [i == 0], [[c]], sos=98, eos=99)
            st, last = R.select(new, [0]), c
            pre = seq[:i + 1]
            brute = sum(p for s, p in tot.items() if s[:i + 1] == pre)
            assert abs(np.exp(psi[0, 0]) - brute) <= 1e-12, (seq, i)
        fin, _ = R.step(lp[None], [T], st, [0], [last], [False], [[99]], sos=98, eos=99)
        assert abs(np.exp(fin[0, 0]) - tot.get(seq, 0.0)) <= 1e-12, seq


@pytest.mark.parametrize("T,V,L", [(40, 7, 12), (300, 32, 140)])
def test_whole_sequence_score_is_minus_ctc_loss(T, V, L):
    lp, rng = _lp(T, V, 1)
    seq = rng.integers(3, V, size=L)
    seq[1::2] = seq[0::2][:len(seq[1::2])]        # every second label repeats its neighbour
    _, fin = R.score_sequence(lp, T, list(seq))
    nll = F.ctc_loss(torch.tensor(lp).unsqueeze(1), torch.tensor(seq).unsqueeze(0), torch.tensor([T]), torch.tensor([L]),
                     reduction="sum").item()
    assert np.isfinite(fin) and abs(fin + nll) <= 1e-9, (fin, -nll)


def test_prefix_longer_than_the_frames_is_minus_inf_not_nan():
    lp, _ = _lp(6, 7, 2)
    pre, fin = R.score_sequence(lp, 3, [3, 3, 4, 5])      # "3 3" alone needs 3 frames; T_b = 3 of the 6
    assert np.isfinite(pre[0]) and np.isfinite(pre[1]) and pre[2] == -np.inf and pre[3] == -np.inf and fin == -np.inf
    assert not np.isnan(np.array(pre + [fin])).any()
    # frames >= T_b of a state are -inf and a NaN there changes nothing: they are never read
    st = R.init_state(lp[None], [3], [0])
    psi, new = R.step(lp[None], [3], st, [0], [R.SOS], [True], [[3, 4]])
    st2 = st.copy()
    st2[:, 3:] = np.nan
    psi2, _ = R.step(lp[None], [3], st2, [0], [R.SOS], [True], [[3, 4]])
    assert np.array_equal(psi, psi2) and np.isinf(new[:, :, 3:]).all()
