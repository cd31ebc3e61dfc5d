"""CPU checks of tests/ctc_reference.py, the float64 restatement that tests/test_gpu_ctc_arms.py holds csrc/ctc.hip against:
it equals torch's F.log_softmax + F.ctc_loss in float64 wherever torch defines the case, it equals the integer path count on all-zero
logits, its conventions beyond torch (clamped lengths, T_b = 0, -inf logits, labels outside [0, V)) are asserted on three-frame examples
worked by hand, and the bound of the GPU tests catches each of eight planted defects on a named case of that suite."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_reference as R


def torch_truth(c, dtype):
    """F.log_softmax + F.ctc_loss on the CPU in `dtype` -> (loss, nll (B,), dlogits of the mean loss), numpy float64."""
    x = torch.from_numpy(c["logits"]).to(dtype).requires_grad_()
    lp = F.log_softmax(x.transpose(0, 1), dim=2)
    args = (torch.from_numpy(c["targets"]), torch.from_numpy(c["in_len"]).long(), torch.from_numpy(c["tg_len"]).long())
    loss = F.ctc_loss(lp, *args, blank=c["blank"], reduction="mean")
    nll = F.ctc_loss(lp, *args, blank=c["blank"], reduction="none")
    assert torch.isfinite(loss)
    loss.backward()
    return float(loss.detach()), nll.detach().double().numpy(), x.grad.double().numpy()


def _ref(c, **kw):
    return R.ctc_reference(c["logits"], c["targets"], c["in_len"], c["tg_len"], c["blank"], **kw)


@pytest.mark.parametrize("name", R.TORCH_DEFINED)
def test_restatement_equals_torch_float64(name):
    c = R.case(name)
    loss, nll, dl = _ref(c)
    t_loss, t_nll, t_dl = torch_truth(c, torch.float64)
    e_loss, e_nll, e_dl = abs(float(loss) - t_loss), float(np.abs(nll - t_nll).max()), float(np.abs(dl - t_dl).max())
    print("%s: loss %.12g |d loss| %.2e  max |d nll| / max(1, |nll|) %.2e  max |d gradient| %.2e" % (
        name, t_loss, e_loss, float((np.abs(nll - t_nll) / np.maximum(1.0, np.abs(t_nll))).max()), e_dl))
    assert dl.dtype == np.float64 and dl.shape == c["logits"].shape
    assert e_loss <= 1e-12 and e_dl <= 1e-12
    assert np.all(np.abs(nll - t_nll) <= 1e-12 * np.maximum(1.0, np.abs(t_nll)))
    for b, Tb in enumerate(c["in_len"]):
        assert not dl[b, Tb:].any()


def test_grad_out_scales_the_gradient_only():
    c = R.case("blank_middle")
    loss, nll, dl = _ref(c)
    loss2, nll2, dl2 = _ref(c, grad_out=-2.0)
    assert loss2 == loss and np.array_equal(nll, nll2) and np.array_equal(dl2, -2.0 * dl)


@pytest.mark.parametrize("name,blank", [("counted_11", 0), ("counted_212", 0), ("counted_empty", 0), ("counted_212", 2)])
def test_restatement_equals_the_path_count(name, blank):
    """All-zero logits, T 6, V 3: nll = 6 log 3 - log N and d nll / d logit[t, v] = 1/3 - occ[t, v] / N from the enumeration of the 729
    labellings.  With blank = 2 the target (2, 1, 2) becomes (0, 1, 0): the same count by symmetry (0 <-> 2)."""
    target = R.COUNTED[name]
    if blank == 2:
        target = tuple(2 - v for v in target)
    c = dict(R.case(name))
    c["blank"] = blank
    c["targets"] = np.zeros((1, 3), dtype=np.int64)
    c["targets"][0, :len(target)] = target
    N, occ, nll_n, g = R.ctc_count_reference(6, 3, target, blank)
    assert N == R.COUNTED_PATHS[name]
    assert occ.sum() == 6 * N and (occ.sum(axis=1) == N).all()
    loss, nll, dl = _ref(c)
    L = max(1, len(target))
    print("%s blank %d: N %d  nll %.15g  |d nll| %.2e  max |d gradient| %.2e" % (name, blank, N, nll_n, abs(nll[0] - nll_n),
                                                                              float(np.abs(dl[0] * L - g).max())))
    assert abs(nll[0] - nll_n) <= 1e-14 and abs(float(loss) - nll_n / L) <= 1e-14
    assert np.abs(dl[0] * L - g).max() <= 1e-14


def _three(logits, target, in_len, tg_len, blank=0, Lmax=None):
    Lmax = Lmax or max(1, len(target))
    tg = np.zeros((1, Lmax), dtype=np.int64)
    tg[0, :len(target)] = target
    return dict(logits=np.asarray(logits, dtype=np.float32)[None], targets=tg, in_len=np.array([in_len], dtype=np.int32),
                tg_len=np.array([tg_len], dtype=np.int32), blank=blank)


def test_convention_clamped_lengths():
    """Three frames over {blank, a}, all-zero logits, target (a): the labellings that collapse to (a) are a--, -a-, --a, aa-, -aa, aaa (a-a
    gives (a, a)): 6 of 8, nll = log(8 / 6).  in_len = 8 is 3 and tg_len = 4 is Lmax = 1: the same bits; in_len = -1 and tg_len = -5 are 0."""
    z = np.zeros((3, 2))
    want = _ref(_three(z, (1,), 3, 1))
    assert abs(want[1][0] - math.log(8 / 6)) <= 1e-15 and abs(float(want[0]) - math.log(8 / 6)) <= 1e-15
    got = _ref(_three(z, (1,), 8, 4))
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    empty = _ref(_three(z, (1,), 3, 0))                         # ---: 1 of 8
    assert abs(empty[1][0] - math.log(8)) <= 1e-15
    neg = _ref(_three(z, (1,), 3, -5))
    assert neg[0] == empty[0] and np.array_equal(neg[2], empty[2])
    none = _ref(_three(z, (1,), -1, 0))
    assert none[0] == 0 and none[1][0] == 0 and not none[2].any()


def test_convention_no_frames():
    """T_b = 0: the empty labelling collapses to the empty target and to nothing else.  nll = 0 (L_b = 0) or +inf; no row has a gradient."""
    z = np.zeros((3, 2))
    loss, nll, dl = _ref(_three(z, (), 0, 0))
    assert loss == 0 and nll[0] == 0 and not dl.any()
    loss, nll, dl = _ref(_three(z, (1,), 0, 1))
    assert loss == np.inf and nll[0] == np.inf and not dl.any() and not np.isnan(dl).any()


def test_convention_minus_infinity_logits():
    """Three frames over {blank, a, c}, zero logits but c = -inf in every frame: the softmax is 1/2, 1/2, 0.  Target (a): 6 labellings of
    probability 1/8 each (as above), nll = log(8 / 6); a is emitted at frame 0 by a--, aa-, aaa (3), at frame 1 by -a-, aa-, -aa, aaa (4), at
    frame 2 by 3: d nll / d logit[t, a] = 1/2 - (3, 4, 3) / 6, the blank column the opposite, column c exactly 0.  Target (c): no labelling
    with a non-zero probability, +inf.  torch gives NaN gradients for the first and cannot be asked."""
    x = np.zeros((3, 3))
    x[:, 2] = -np.inf
    loss, nll, dl = _ref(_three(x, (1,), 3, 1))
    assert abs(nll[0] - math.log(8 / 6)) <= 1e-15
    want = np.array([[-(0.5 - 3 / 6), 0.5 - 3 / 6, 0], [-(0.5 - 4 / 6), 0.5 - 4 / 6, 0], [-(0.5 - 3 / 6), 0.5 - 3 / 6, 0]])
    assert np.abs(dl[0] - want).max() <= 1e-15 and not dl[0, :, 2].any() and not np.isnan(dl).any()
    loss, nll, dl = _ref(_three(x, (2,), 3, 1))
    assert loss == np.inf and nll[0] == np.inf and np.isnan(dl).all()
    l32, n32, d32 = _ref(_three(x, (1,), 3, 1), dtype=np.float32)
    assert d32.dtype == np.float32 and n32.dtype == np.float32 and abs(float(n32[0]) - math.log(8 / 6)) <= 1e-6


def test_convention_labels_outside_the_vocabulary():
    """V = 2: the labels 2, -1 and 2^40 exist in no frame.  In a used slot: +inf, NaN rows for t < T_b = 2, a zero row after.  In a slot
    l >= L_b: nothing changes."""
    z = np.zeros((3, 2))
    for bad in (2, -1, 2 ** 40):
        loss, nll, dl = _ref(_three(z, (bad,), 2, 1))
        assert loss == np.inf and nll[0] == np.inf and np.isnan(dl[0, :2]).all() and not dl[0, 2].any()
        c = _three(z, (1, bad), 3, 1, Lmax=2)
        want = _ref(_three(z, (1, 1), 3, 1, Lmax=2))
        got = _ref(c)
        assert got[0] == want[0] and np.array_equal(got[2], want[2]) and abs(got[1][0] - math.log(8 / 6)) <= 1e-15


# each planted defect, the named case of tests/test_gpu_ctc_arms.py whose bound it breaks, and through which figure
PLANTED = [
    ("skip_equal", "blank_middle", "loss"),          # "aabb": a path may jump from a to a without the blank between them
    ("skip_blank", "blank_last", "loss"),            # a blank may be entered from the blank two states back, skipping a label
    ("no_start1", "tiny_one_frame", "loss"),         # one frame, one label: the only path starts in s = 1 -> +inf
    ("no_final2", "tiny_one_frame", "loss"),         # ... and ends in s = S - 2 -> +inf
    ("unclamped_len", "lengths_over", "loss"),       # tg_len = Lmax + 3: the loss divides by 7, the lattice has 4 labels
    ("mean_sum", "blank_middle", "loss"),            # L = (4, 2, 1): sum nll / 7 is not mean(nll / L)
    ("pad_softmax", "blank_middle", "gradient"),     # in_len = (14, 9, 6): frames 9..13 of utterance 1 must stay 0
    ("no_B", "blank_last", "gradient"),              # B = 2: every row doubled
]


def _yardstick32(name, c, r64):
    """err32 of the GPU tests: torch in float32 where torch defines the case, else the restatement in float32."""
    if name in R.TORCH_DEFINED:
        g32 = torch_truth(c, torch.float32)[2]
    else:
        g32 = _ref(c, dtype=np.float32)[2]
    return R.grad_err(g32, r64[2])


@pytest.mark.parametrize("defect,name,figure", PLANTED, ids=["%s-on-%s" % p[:2] for p in PLANTED])
def test_planted_defect_breaks_the_bound(defect, name, figure):
    c = R.case(name)
    r64 = _ref(c)
    err32 = _yardstick32(name, c, r64)
    bound = R.grad_bound(r64[2], err32)
    clean = _ref(c, dtype=np.float32)
    assert R.loss_ok(float(clean[0]), float(r64[0])) and R.grad_err(clean[2], r64[2]) <= bound, "the clean float32 evaluation must pass"
    bad = _ref(c, dtype=np.float32, defect=defect)
    loss_broken = not R.loss_ok(float(bad[0]), float(r64[0]))
    grad_broken = not R.grad_err(bad[2], r64[2]) <= bound
    print("%s on %s: loss %.6g (truth %.6g), gradient error %.3e, bound %.3e (err32 %.3e)" % (
        defect, name, float(bad[0]), float(r64[0]), R.grad_err(bad[2], r64[2]), bound, err32))
    assert {"loss": loss_broken, "gradient": grad_broken}[figure], (defect, name)


def test_every_defect_is_planted():
    assert sorted(p[0] for p in PLANTED) == sorted(R.DEFECTS)
    assert all(p[1] in R.CASES for p in PLANTED)
