"""Every arm of the CTC loss kernels (csrc/ctc.hip: asr_ctc_fwd / asr_ctc_bwd) against the float64 restatement of tests/ctc_reference.py,
through the C ABI so that row strides, the blank and every buffer are the test's (tests/test_ctc_reference_host.py shows on the CPU that the
restatement is torch's float64 ctc_loss where torch defines the case, and that the bound below catches eight planted defects).

Bound, the one of tests/test_gpu_ctc.py: loss within 2e-5 max(1, |ref|); gradient error <= max(2e-6 + 2e-5 max|ref|, 4 err32), err32 = the
error of the float32 CPU evaluation against float64 on the same tensors (torch's F.ctc_loss where torch defines the case, else the
restatement in float32).  Bit for bit (uint32 views): pad columns and padded frames zero, strided against contiguous rows, padding filled
with NaN / out-of-range ids against clean padding, lengths outside their range against the clamped ones, the neighbours of an utterance
without an alignment, forward twice.  Every call runs between 64-float guards around the workspace, the loss and dlogits, and dlogits is
NaN before the call.  Every figure is printed before it is asserted (`-s`)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_reference as R

pytestmark = pytest.mark.gpu

G, FILL = 64, -7.0
EINVAL = -1


class card:
    """A launch or runtime error of the card ends the session: nothing more runs on a card that has just faulted.  A refused argument
    or any other Python error fails the one test."""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        return self

    def __exit__(self, et, e, tb):
        if et is None:
            try:
                torch.cuda.synchronize()
            except RuntimeError as err:
                pytest.exit("%s: %r" % (self.what, err), returncode=3)
            return False
        if isinstance(e, RuntimeError):
            from asr_hip import lib as L
            s = str(e)
            if (isinstance(e, L.AsrHipError) and (s.endswith("(-2)") or s.endswith("(-4)"))) or "HIP error" in s or "CUDA error" in s:
                pytest.exit("%s: %r" % (self.what, e), returncode=3)
        return False


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Buffers:
    """The device side of one case: logits with row stride ld (pad columns NaN), and the three outputs between guards."""

    def __init__(self, c, ld=None, ldo=None, grad_out=1.0):
        from asr_hip import lib as L
        self.c = c
        x = c["logits"]
        self.B, self.T, self.V = x.shape
        self.Lmax = c["targets"].shape[1]
        self.ld, self.ldo = ld or self.V, ldo or self.V
        dev = torch.device("cuda:0")
        host = torch.full((self.B, self.T, self.ld), float("nan"))
        host[..., :self.V] = torch.from_numpy(x)
        self.x = host.to(dev)
        self.tg = torch.from_numpy(c["targets"]).to(dev)
        self.il = torch.from_numpy(c["in_len"]).to(dev)
        self.tl = torch.from_numpy(c["tg_len"]).to(dev)
        self.n = int(L.load().asr_ctc_workspace(self.B, self.T, self.Lmax))
        assert self.n == self.B * self.T + 2 * self.B * self.T * (2 * self.Lmax + 1) + self.B
        self.ws = torch.full((self.n + 2 * G,), FILL, device=dev)
        self.loss = torch.full((1 + 2 * G,), FILL, device=dev)
        self.dl = torch.full((self.B * self.T * self.ldo + 2 * G,), float("nan"), device=dev)
        self.dl[:G] = FILL
        self.dl[-G:] = FILL
        self.go = torch.tensor([grad_out], dtype=torch.float32, device=dev)

    def fwd_args(self):
        from asr_hip import lib as L
        return [L.ptr(self.x), self.ld, L.ptr(self.tg), L.ptr(self.il), L.ptr(self.tl), self.B, self.T, self.V, self.Lmax, self.c["blank"],
                self.ws[G:].data_ptr(), self.n, self.loss[G:].data_ptr(), L.stream()]

    def bwd_args(self):
        from asr_hip import lib as L
        return [L.ptr(self.x), self.ld, L.ptr(self.tg), L.ptr(self.il), L.ptr(self.tl), self.B, self.T, self.V, self.Lmax, self.c["blank"],
                self.ws[G:].data_ptr(), L.ptr(self.go), self.dl[G:].data_ptr(), self.ldo, L.stream()]

    def guards_intact(self):
        for name, buf in (("workspace", self.ws), ("loss", self.loss), ("dlogits", self.dl)):
            guard = torch.full((G,), FILL)
            assert torch.equal(buf[:G].cpu(), guard) and torch.equal(buf[-G:].cpu(), guard), "guard of the %s overwritten" % name

    def results(self):
        loss = self.loss[G:G + 1].cpu().numpy()[0]
        nll = self.ws[G + self.n - self.B:G + self.n].cpu().numpy()
        dl = self.dl[G:-G].view(self.B, self.T, self.ldo).cpu().numpy()
        return loss, nll, dl


def run(c, what, ld=None, ldo=None, grad_out=1.0, keep=False):
    """asr_ctc_fwd + asr_ctc_bwd on case c -> (loss fp32, nll (B,), dlogits (B,T,ldo)) [and the Buffers]; guards checked."""
    from asr_hip import lib as L
    d = Buffers(c, ld, ldo, grad_out)
    with card(what):
        L.call("asr_ctc_fwd", *d.fwd_args())
        L.call("asr_ctc_bwd", *d.bwd_args())
    d.guards_intact()
    out = d.results()
    return out + (d,) if keep else out


def torch32(c):
    """Gradient of torch's float32 F.log_softmax + F.ctc_loss on the CPU (finite cases torch defines)."""
    x = torch.from_numpy(c["logits"]).clone().requires_grad_()
    lp = F.log_softmax(x.transpose(0, 1), dim=2)
    loss = F.ctc_loss(lp, torch.from_numpy(c["targets"]), torch.from_numpy(c["in_len"]).long(), torch.from_numpy(c["tg_len"]).long(),
                      blank=c["blank"], reduction="mean")
    assert torch.isfinite(loss)
    loss.backward()
    return x.grad.numpy()


_TRUTH = {}          # name -> (restatement in float64, err32), computed once and shared (never modified)


def truth(name):
    if name not in _TRUTH:
        c = R.case(name)
        r64 = R.ctc_reference(c["logits"], c["targets"], c["in_len"], c["tg_len"], c["blank"])
        if name in R.TORCH_DEFINED:
            g32 = torch32(c)
        else:
            g32 = R.ctc_reference(c["logits"], c["targets"], c["in_len"], c["tg_len"], c["blank"], dtype=np.float32)[2]
        _TRUTH[name] = (r64, R.grad_err(g32, r64[2]))
    return _TRUTH[name]


def check(what, got, r64, err32, V):
    """The bound of the module docstring on (loss, nll, dlogits[..., :V]); pad columns exactly +0."""
    loss, nll, dl = got
    ref_loss, ref_nll, ref_dl = r64
    e_loss = abs(float(loss) - float(ref_loss)) if math.isfinite(ref_loss) else 0.0
    err, bound = R.grad_err(dl[..., :V], ref_dl), R.grad_bound(ref_dl, err32)
    print("%s: loss %.7g (float64 %.7g, error %.2e, allowed %.2e)  gradient error %.3e  err32 %.3e  bound %.3e" % (
        what, float(loss), float(ref_loss), e_loss, 2e-5 * max(1.0, abs(float(ref_loss))) if math.isfinite(ref_loss) else 0.0, err, err32, bound))
    assert R.loss_ok(float(loss), float(ref_loss)), (what, float(loss), float(ref_loss))
    for b in range(len(ref_nll)):
        assert R.loss_ok(float(nll[b]), float(ref_nll[b])), (what, b, float(nll[b]), float(ref_nll[b]))
    assert err <= bound, (what, err, err32, bound)
    assert not bits(dl[..., V:]).any(), "pad columns"


# ------------------------------------------------------------------------------------------------ the named cases
NAMED = ["batch_mean", "blank_middle", "blank_last", "tiny_one_frame", "tiny_blank_only", "tiny_mixed", "states_over_threads",
         "lattice_grant_full", "lattice_grant_padding", "grad_grant_13000", "grad_grant_16384", "peaked", "neg_inf_column", "neg_inf_reach"]


@pytest.mark.parametrize("name", NAMED)
def test_case_against_the_restatement(name):
    c = R.case(name)
    r64, err32 = truth(name)
    B, T, V = c["logits"].shape
    loss, nll, dl, d = run(c, name, keep=True)
    check(name, (loss, nll, dl), r64, err32, V)
    for b in range(B):
        Tb = max(0, min(T, int(c["in_len"][b])))
        assert not bits(dl[b, Tb:]).any(), "padded frames of utterance %d" % b
    S = 2 * d.Lmax + 1
    if name == "batch_mean":
        assert B > 64 and len(set(c["tg_len"].tolist())) == 2
    if name == "tiny_blank_only":
        assert float(loss) == 0.0 and not nll.any() and not dl.any()
    if name == "tiny_mixed":
        assert nll[0] == 0.0 and nll[1] == np.inf and math.isfinite(nll[2]) and math.isfinite(nll[3]) and loss == np.inf
        assert not bits(dl[:2]).any()
    if name in ("lattice_grant_full", "lattice_grant_padding"):
        assert 3 * S * 4 > 48 * 1024
    if name == "lattice_grant_full":
        assert math.isfinite(float(r64[0])) and S == 4201
    if name in ("grad_grant_13000", "grad_grant_16384"):
        assert V * 4 > 48 * 1024
    if name == "peaked":                                       # the lattice legitimately holds -inf inside the live region
        alpha = d.ws[G + B * T:G + B * T + B * T * S].view(B, T, S)[2, :17, :5].cpu().numpy()
        assert np.isneginf(alpha).any() and np.isfinite(alpha).any() and np.isfinite(dl).all()
    if name == "neg_inf_column":
        assert math.isfinite(float(loss)) and not dl[..., 7].any() and np.isfinite(dl).all()
    if name == "neg_inf_reach":
        assert nll[0] == np.inf and loss == np.inf and np.isnan(dl[0]).all() and np.isfinite(dl[1:]).all() and not dl[1:, :, 7].any()


@pytest.mark.parametrize("name", sorted(R.COUNTED))
def test_uniform_logits_against_the_path_count(name):
    """All-zero logits, T 6, V 3: loss and gradient from the enumeration of the 729 labellings (no logarithm or recursion shared)."""
    c = R.case(name)
    target = R.COUNTED[name]
    N, occ, nll_n, g = R.ctc_count_reference(6, 3, target, 0)
    assert N == R.COUNTED_PATHS[name]
    L = max(1, len(target))
    counted = (np.float64(nll_n / L), np.array([nll_n]), (g / L)[None])
    check(name + " (N = %d)" % N, run(c, name), counted, truth(name)[1], 3)


def test_blank_last_through_ctcfn():
    """CTCFn.apply with blank = V - 1: the same kernels behind the Python entry point, upstream gradient 1."""
    from asr_hip.functions import CTCFn
    c = R.case("blank_last")
    r64, err32 = truth("blank_last")
    x = torch.from_numpy(c["logits"]).cuda().requires_grad_()
    with card("CTCFn"):
        loss = CTCFn.apply(x, torch.from_numpy(c["targets"]).cuda(), torch.from_numpy(c["in_len"]), torch.from_numpy(c["tg_len"]), c["blank"])
        loss.backward()
    got = (loss.detach().cpu().numpy(), r64[1], x.grad.cpu().numpy())
    check("blank_last through CTCFn", got, r64, err32, 7)
    assert same_bits(got[0], run(c, "blank_last")[0])


# ------------------------------------------------------------------------------------------------ strides and padding
def test_strided_rows_give_the_bits_of_contiguous_rows():
    """ld = V + 3 with NaN in the pad columns, ldo = V + 5 into a NaN-filled buffer: pad columns exactly 0, the rest the bits of ld = ldo = V."""
    c = R.case("blank_middle")
    r64, err32 = truth("blank_middle")
    V = 9
    plain = run(c, "contiguous")
    wide = run(c, "strided", ld=V + 3, ldo=V + 5)
    check("strided ld %d ldo %d" % (V + 3, V + 5), wide, r64, err32, V)
    assert wide[2].shape[2] == V + 5 and not bits(wide[2][..., V:]).any()
    assert same_bits(plain[0], wide[0]) and same_bits(plain[1], wide[1]) and same_bits(plain[2], wide[2][..., :V])


def test_padding_is_never_read():
    """NaN in the logits of frames t >= T_b; -1, 2^40 and V in target slots l >= L_b: every bit of the clean (strided) run."""
    c = R.case("blank_middle")
    V, T = 9, 14
    clean = run(c, "clean", ld=V + 3, ldo=V + 5)
    dirty = dict(c, logits=c["logits"].copy(), targets=c["targets"].copy())
    fill = [-1, 2 ** 40, V]
    k = 0
    for b, (Tb, Lb) in enumerate(zip(c["in_len"], c["tg_len"])):
        dirty["logits"][b, Tb:] = np.nan
        for l in range(Lb, 4):
            dirty["targets"][b, l] = fill[k % 3]
            k += 1
    assert k >= 3 and np.isnan(dirty["logits"]).any()
    got = run(dirty, "dirty padding", ld=V + 3, ldo=V + 5)
    assert same_bits(clean[0], got[0]) and same_bits(clean[1], got[1]) and same_bits(clean[2], got[2])
    assert math.isfinite(float(got[0]))
    for b, Tb in enumerate(c["in_len"]):
        assert not bits(got[2][b, Tb:]).any() and np.isfinite(got[2][b, :Tb]).all()


# ------------------------------------------------------------------------------------------------ upstream gradient
def test_upstream_gradient_scales_every_row():
    """grad_out in {1, 0.3, -2, 0}.  A row is fl(x s) with the scale s = fl(grad_out / (L_b B)), which the grad_out = 1 run rounded as
    s_1 = fl(1 / (L_b B)): the result is the grad_out = 1 result times s / s_1 (both quotients are IEEE, formed here in float32 too)
    within the one rounding each of the two products carries, 2 x 2^-24 relative.  s / s_1 is grad_out within the roundings of the two
    quotients, so against the plain product with grad_out the same holds with 4 x 2^-24; on the CPU that plain figure reaches
    1.17 x 2^-23 for 0.3 / 12, which is why the first form is the one held to one rounding step.  -2 is exact, 0 gives exact zeros.
    neg_inf_reach adds an infinite utterance: its rows stay NaN whatever grad_out is."""
    for name in ("blank_middle", "neg_inf_reach"):
        c = R.case(name)
        B = c["logits"].shape[0]
        one = run(c, name + " grad_out 1")
        fin = np.isfinite(one[2])
        LB = np.float32(B) * np.maximum(np.clip(c["tg_len"], 0, 4), 1).astype(np.float32)
        for go in (0.3, -2.0, 0.0):
            got = run(c, "%s grad_out %g" % (name, go), grad_out=go)
            assert same_bits(got[0], one[0]) and same_bits(got[1], one[1])
            assert np.array_equal(np.isnan(got[2]), ~fin)
            ratio = ((np.float32(go) / LB).astype(np.float64) / (np.float32(1) / LB).astype(np.float64))[:, None, None]
            assert np.all(np.abs(ratio - float(np.float32(go))) <= 2.0 ** -23 * abs(go))
            want = (one[2].astype(np.float64) * ratio)[fin]
            plain = one[2][fin].astype(np.float64) * float(np.float32(go))
            d, dp = np.abs(got[2][fin].astype(np.float64) - want), np.abs(got[2][fin].astype(np.float64) - plain)
            rel = float((d / np.maximum(np.abs(want), 1e-30)).max()) if go else 0.0
            relp = float((dp / np.maximum(np.abs(plain), 1e-30)).max()) if go else 0.0
            print("%s grad_out %g: largest relative deviation from (grad_out = 1 result) x s / s_1 %.3f x 2^-23, from (grad_out = 1 result) x "
                  "grad_out %.3f x 2^-23" % (name, go, rel / 2.0 ** -23, relp / 2.0 ** -23))
            assert np.all(d <= 2.0 ** -23 * np.abs(want)) and np.all(dp <= 2.0 ** -22 * np.abs(plain))
            if go == 0.0:
                assert not got[2][fin].any()
            if go == -2.0:
                assert np.array_equal(got[2][fin], -2.0 * one[2][fin])


# ------------------------------------------------------------------------------------------------ lengths outside their range
def test_lengths_outside_the_range_are_clamped():
    """in_len = T + 5 and tg_len = Lmax + 3 give the bits of T and Lmax, negative lengths those of 0: loss (which divided by the unclamped
    target length before the fix), nll and gradient."""
    base = R.case("blank_middle")
    over = run(R.case("lengths_over"), "lengths over")
    want = run(base, "lengths at the limit")
    print("over: loss %.7g, clamped %.7g" % (float(over[0]), float(want[0])))
    assert same_bits(over[0], want[0]) and same_bits(over[1], want[1]) and same_bits(over[2], want[2])
    check("lengths over", over, *truth("lengths_over"), 9)
    neg = R.case("lengths_negative")
    zero = dict(neg, in_len=np.maximum(neg["in_len"], 0), tg_len=np.maximum(neg["tg_len"], 0))
    got, want = run(neg, "lengths negative"), run(zero, "lengths zero")
    print("negative: loss %.7g nll %s, zero: %.7g %s" % (float(got[0]), got[1], float(want[0]), want[1]))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    check("lengths negative", got, *truth("lengths_negative"), 9)
    assert got[1][1] == 0.0 and not bits(got[2][1]).any() and math.isfinite(float(got[0]))        # utterance 1: no frames, no labels


# ------------------------------------------------------------------------------------------------ utterances without an alignment
@pytest.mark.parametrize("how", ["too_few_frames", "no_frames", "label_V", "label_minus_1"])
def test_an_utterance_without_alignment_keeps_to_itself(how):
    """Utterance 1 of 3 ("aa": three frames at least) made infinite: nll_1 and the loss +inf, its rows NaN for t < T_1 and 0 after, and
    utterances 0 and 2 keep every bit of nll and gradient of the well-formed run."""
    c = R.case("blank_middle")
    V = 9
    assert c["targets"][1, 0] == c["targets"][1, 1] and c["tg_len"][1] == 2
    want = run(c, "well formed")
    bad = dict(c, in_len=c["in_len"].copy(), targets=c["targets"].copy())
    if how == "too_few_frames":
        bad["in_len"][1] = 2
    elif how == "no_frames":
        bad["in_len"][1] = 0
    elif how == "label_V":
        bad["targets"][1, 1] = V
    else:
        bad["targets"][1, 0] = -1
    T1 = int(bad["in_len"][1])
    loss, nll, dl = run(bad, how)
    print("%s: loss %s nll %s" % (how, loss, nll))
    assert nll[1] == np.inf and loss == np.inf
    assert np.isnan(dl[1, :T1]).all() and not bits(dl[1, T1:]).any()
    for b in (0, 2):
        assert same_bits(nll[b:b + 1], want[1][b:b + 1]) and same_bits(dl[b], want[2][b]), (how, b)
    r = R.ctc_reference(bad["logits"], bad["targets"], bad["in_len"], bad["tg_len"], bad["blank"])
    assert r[0] == np.inf and np.array_equal(np.isnan(r[2]), np.isnan(dl))


# ------------------------------------------------------------------------------------------------ buffers
def test_sentinels_and_a_short_workspace():
    """64 guard floats either side of the workspace, the loss and dlogits survive forward and backward (run() asserts it in every test;
    here on the strided case, with the interior shown to be written); a workspace one float short is refused before any launch."""
    from asr_hip import lib as L
    c = R.case("blank_middle")
    loss, nll, dl, d = run(c, "sentinels", ld=12, ldo=14, keep=True)
    assert not np.isnan(dl).any()                                              # every float of dlogits between the guards was written
    inside = d.ws[G:G + d.n].cpu().numpy()
    B, T, S = 3, 14, 9
    assert not (inside[:B * T] == FILL).any() and not (inside[-B:] == FILL).any()      # row lse and nll written
    lat = inside[B * T:B * T + B * T * S].reshape(B, T, S)
    assert not (lat[0] == FILL).any() and (lat[2, 6:] == FILL).all()                    # frames >= T_b of the lattice are not touched
    short = Buffers(c)
    args = short.fwd_args()
    args[11] = short.n - 1
    with card("short workspace"):
        assert L.load().asr_ctc_fwd(*args) == EINVAL
    assert torch.equal(short.ws.cpu(), torch.full((short.n + 2 * G,), FILL)) and torch.equal(short.loss.cpu(), torch.full((1 + 2 * G,), FILL))


def test_two_calls():
    """Forward twice: the same bits everywhere (no atomics).  Backward twice: columns shared by several lattice states (the blank always)
    are summed with LDS atomics, S = 291 states over five waves here; whether the bits were equal is printed, the difference is held to
    the bound."""
    from asr_hip import lib as L
    name = "states_over_threads"
    c = R.case(name)
    r64, err32 = truth(name)
    a = run(c, "first", keep=True)
    b = run(c, "second", keep=True)
    assert torch.equal(a[3].ws.view(torch.int32), b[3].ws.view(torch.int32)) and same_bits(a[0], b[0])
    first = a[2].copy()
    with card("backward again"):
        L.call("asr_ctc_bwd", *a[3].bwd_args())
    again = a[3].results()[2]
    a[3].guards_intact()
    diff = float(np.abs(first.astype(np.float64) - again).max())
    print("two backward calls on one workspace: bits equal %s, across two workspaces: %s, largest difference %.3e (bound %.3e)" % (
        same_bits(first, again), same_bits(first, b[2]), diff, R.grad_bound(r64[2], err32)))
    assert diff <= R.grad_bound(r64[2], err32) and float(np.abs(first.astype(np.float64) - b[2]).max()) <= R.grad_bound(r64[2], err32)


# ------------------------------------------------------------------------------------------------ refusals
def _untouched(d):
    d.guards_intact()
    assert (d.ws == FILL).all().item() and (d.loss == FILL).all().item() and torch.isnan(d.dl[G:-G]).all().item()


def test_argument_errors():
    """ASR_EINVAL before any launch: a null pointer in each position, B = 0, T = 0, Lmax = 0, ld < V, ldo < V, blank = V, blank = -1."""
    from asr_hip import lib as L
    lib = L.load()
    d = Buffers(R.case("blank_middle"))
    V = 9
    with card("argument errors"):
        for i in (0, 2, 3, 4, 10, 12):                                          # logits, targets, input_lengths, target_lengths, workspace, loss
            args = d.fwd_args()
            args[i] = None
            assert lib.asr_ctc_fwd(*args) == EINVAL, ("fwd null", i)
        for i in (0, 2, 3, 4, 10, 11, 12):                                      # ..., workspace, grad_out, dlogits
            args = d.bwd_args()
            args[i] = None
            assert lib.asr_ctc_bwd(*args) == EINVAL, ("bwd null", i)
        for i, v in ((5, 0), (6, 0), (8, 0), (1, V - 1), (9, V), (9, -1)):       # B, T, Lmax, ld, blank
            f, b = d.fwd_args(), d.bwd_args()
            f[i] = b[i] = v
            assert lib.asr_ctc_fwd(*f) == EINVAL and lib.asr_ctc_bwd(*b) == EINVAL, (i, v)
        b = d.bwd_args()
        b[13] = V - 1                                                          # ldo
        assert lib.asr_ctc_bwd(*b) == EINVAL
        assert lib.asr_ctc_workspace(0, 14, 4) == 0 and lib.asr_ctc_workspace(3, 0, 4) == 0
    _untouched(d)


def test_unsupported_sizes_are_refused():
    """V = 16385: one row of V floats exceeds 64 KB of LDS, asr_ctc_bwd returns ASR_EUNSUPPORTED (the forward has no such limit and runs);
    Lmax = 2731: three rows of 2 Lmax + 1 words do, asr_ctc_fwd returns it.  Nothing is written; through CTCFn both raise AsrHipError."""
    from asr_hip import lib as L
    from asr_hip.functions import CTCFn
    lib = L.load()
    big_v = R.make_case(1, 3, 16385, 1, [3], [1], seed=31)
    d = Buffers(big_v)
    with card("V 16385"):
        assert lib.asr_ctc_fwd(*d.fwd_args()) == 0
        assert lib.asr_ctc_bwd(*d.bwd_args()) == L.EUNSUPPORTED
    d.guards_intact()
    assert torch.isnan(d.dl[G:-G]).all().item() and math.isfinite(float(d.results()[0]))
    long_l = R.make_case(1, 2, 4, 2731, [2], [1], seed=32)
    d = Buffers(long_l)
    with card("Lmax 2731"):
        assert lib.asr_ctc_fwd(*d.fwd_args()) == L.EUNSUPPORTED
    _untouched(d)
    ok = R.make_case(1, 2, 4, 2730, [2], [1], seed=32)                           # the largest supported Lmax: 3 (2 Lmax + 1) words = 65532 bytes
    r = R.ctc_reference(ok["logits"], ok["targets"], ok["in_len"], ok["tg_len"], 0)
    check("Lmax 2730", run(ok, "Lmax 2730"), r, 0.0, 4)
    for c in (big_v, long_l):
        x = torch.from_numpy(c["logits"]).cuda().requires_grad_()
        with pytest.raises(L.AsrHipError):
            with card("CTCFn refusal"):
                loss = CTCFn.apply(x, torch.from_numpy(c["targets"]).cuda(), torch.from_numpy(c["in_len"]), torch.from_numpy(c["tg_len"]), 0)
                loss.backward()
        assert x.grad is None
