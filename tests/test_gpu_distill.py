"""csrc/distill.hip on the GPU: asr_distill_fwd / _finish / _bwd against the float64 restatement
tests/distill_reference.py under the project's rule for row-wise kernels (4 x torch's own fp32 error on the same input, floored at one
fp32 rounding of the tensor's largest entry, + one bf16 rounding for bf16 outputs), and the exact properties: sentinels, dead rows, pad
columns, NaN where nothing may be read, aligned against misaligned row bases, teacher == student, two identical calls, the refusals.

Shapes: V in {3, 11, 257, 4364} (below one 16-byte chunk per lane, a tail behind whole chunks, more than one 256-column sweep with a tail,
the benchmark's vocabulary); M in {1, 7, 9, 64} (a partial block of 8 rows, two blocks, eight blocks); tau in {1, 2, 4}; smoothing in {0, 0.1}."""
import numpy as np
import pytest
import torch

import distill_reference as D

pytestmark = pytest.mark.gpu

SHAPES = [(M, V) for V in (3, 11, 257, 4364) for M in (1, 7, 9, 64)]
TAUS = (1.0, 2.0, 4.0)
GRAD_OUT = 1.75
S_F, S_I = -768.0, -7            # sentinels around every output


def _run(s_view, t_view, gold, V, smoothing, tau, ce_scale, kd_scale, with_ce=True, out_dtype=torch.float32, ldd=None, argmax_null=False):
    """One forward + finish + backward through the C ABI, every output inside a buffer of sentinels -> dict of the outputs' views and the
    whole buffers.  s_view / t_view: (M, >= V) device views with unit column stride."""
    from asr_hip import lib as L
    dev = s_view.device
    M = s_view.shape[0]
    ldd = ldd or (V + 7) // 8 * 8 + 8
    nb = int(L.load().asr_distill_partial_blocks(M))
    full = dict(stats=torch.full((M + 2, 4), S_F, device=dev), am=torch.full((M + 2,), S_I, device=dev, dtype=torch.int64),
                part=torch.full((nb + 2, 4), S_F, device=dev), sums=torch.full((3, 4), S_F, device=dev), loss=torch.full((3,), S_F, device=dev),
                dl=torch.full((M + 2, ldd), S_F, device=dev).to(out_dtype))
    go = torch.tensor([GRAD_OUT], device=dev)
    g = gold.to(dev)
    L.call("asr_distill_fwd", L.ptr(s_view), s_view.stride(0), L.ptr(t_view), t_view.stride(0), L.ptr(g), M, V, float(smoothing), D.PAD,
           float(tau), 1 if with_ce else 0, L.ptr(full["stats"][1:]), None if argmax_null else L.ptr(full["am"][1:]), L.ptr(full["part"][1:]),
           L.stream())
    L.call("asr_distill_finish", L.ptr(full["part"][1:]), nb, None, float(ce_scale), float(kd_scale), L.ptr(full["sums"][1:]),
           L.ptr(full["loss"][1:]), L.stream())
    L.call("asr_distill_bwd", L.ptr(s_view), s_view.stride(0), L.ptr(t_view), t_view.stride(0), L.ptr(g), L.ptr(full["stats"][1:]), M, V,
           float(smoothing), D.PAD, float(tau), float(ce_scale), float(kd_scale), L.ptr(go), L.ptr(full["sums"][1, 1:2]), L.ptr(full["dl"][1:]),
           ldd, L.dt(full["dl"]), L.stream())
    torch.cuda.synchronize()
    out = dict(stats=full["stats"][1:M + 1], am=full["am"][1:M + 1], part=full["part"][1:nb + 1], sums=full["sums"][1], loss=full["loss"][1],
               dl=full["dl"][1:M + 1])
    out["full"] = full
    return out


def _sentinels_untouched(o):
    f = o["full"]
    return all(bool((f[k][0].float() == s).all()) and bool((f[k][-1].float() == s).all())
               for k, s in (("stats", S_F), ("am", S_I), ("part", S_F), ("sums", S_F), ("loss", S_F), ("dl", S_F)))


def _same(a, b, keys=("stats", "am", "part", "sums", "loss", "dl")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _dev(c):
    return torch.from_numpy(c["s"]).cuda(), torch.from_numpy(c["t"]).cuda(), torch.from_numpy(c["gold"])


_refs = {}


def _reference(M, V, tau, smoothing, ce_scale, kd_scale, with_ce=True):
    """(float64 reference, bounds) of a case, computed once per process and shared (callers leave it unchanged)."""
    key = (M, V, tau, smoothing, ce_scale, kd_scale, with_ce)
    if key not in _refs:
        c = D.case(M, V)
        a = (c["s"][:, :V], c["t"][:, :V], c["gold"], smoothing, D.PAD, tau, ce_scale, kd_scale, GRAD_OUT, with_ce)
        ref = D.distill(*a)
        _refs[key] = (ref, D.bounds(*a, ref))
    return _refs[key]


def _check(o, ref, b, V, bf16=False, what=""):
    live = ref["live"]
    x = dict(kd=D.excess(o["stats"][:, 3], ref["kd"], b["kd"]), loss=D.excess(o["loss"].reshape(1), ref["loss"].reshape(1), b["loss"]),
             dlogits=D.excess(o["dl"][:, :V].float(), ref["dlogits"], b["dlogits"], bf16_stored=bf16))
    for i in (0, 3):
        x["sums%d" % i] = D.excess(o["sums"][i:i + 1], ref["sums"][i:i + 1], b["sums"][i])
    print("%s error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(x.items()))))
    assert all(v <= 1.0 for v in x.values()), (what, x, b)
    assert o["sums"][1].item() == float(ref["sums"][1]) and o["sums"][2].item() == float(ref["sums"][2])
    dl = o["dl"].float().cpu()
    assert bool((dl[~live] == 0).all()) and bool((dl[:, V:] == 0).all())                     # dead rows and pad columns: exactly 0
    assert bool((o["stats"].cpu()[~live] == 0).all())
    assert _sentinels_untouched(o), what


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("M,V", SHAPES)
def test_against_the_float64_restatement(M, V, tau):
    from asr_hip import ops
    c = D.case(M, V)
    s, t, gold = _dev(c)
    live = gold != D.PAD
    for smoothing in (0.0, 0.1):
        ref, b = _reference(M, V, tau, smoothing, 0.6, 0.4)
        for dtype in (torch.float32, torch.bfloat16):
            o = _run(s[:, :V], t[:, :V], gold, V, smoothing, tau, 0.6, 0.4, out_dtype=dtype)
            _check(o, ref, b, V, bf16=dtype == torch.bfloat16, what="M%d V%d tau%g eps%g %s" % (M, V, tau, smoothing, dtype))
        am = o["am"].cpu()
        assert torch.equal(am[live], ops.argmax_rows(s[:, :V]).cpu()[live]) and torch.equal(am[live], ref["argmax"][live])
        assert bool((am[~live] == 0).all())
        # the lse columns feed the backward: against float64 within 4 fp32 roundings of their own size
        st = o["stats"].double().cpu()
        assert float((st[:, :3] - ref["row_stats"][:, :3]).abs().max()) <= 4 * D.EPS32 * max(1.0, float(ref["row_stats"][:, :3].abs().max()))


@pytest.mark.parametrize("M,V", [(9, 3), (7, 11), (9, 257), (9, 4364)])
def test_nothing_is_read_in_dead_rows_or_behind_column_V(M, V):
    """NaN in the dead rows of both logit tensors and in the columns >= V of every row changes no output bit."""
    c = D.case(M, V)
    s, t, gold = _dev(c)
    want = _run(s[:, :V], t[:, :V], gold, V, 0.1, 2.0, 0.6, 0.4)
    s2, t2 = s.clone(), t.clone()
    dead = (gold == D.PAD).cuda()
    assert bool(dead.any()) and c["ld"] > V
    for x in (s2, t2):
        x[dead] = float("nan")
        x[:, V:] = float("nan")
    got = _run(s2[:, :V], t2[:, :V], gold, V, 0.1, 2.0, 0.6, 0.4)
    assert _same(got, want) and not torch.isnan(got["dl"]).any()


@pytest.mark.parametrize("M,V", [(9, 3), (7, 11), (64, 257), (9, 4364)])
def test_misaligned_row_bases_give_the_bits_of_aligned_ones(M, V):
    """ld = V (odd V: rows at 12-, 44-, 1028-byte steps) and a base one float behind a 16-byte boundary, for either tensor, against the
    padded 16-byte-aligned copy: torch.equal for every output, fp32 and bf16 gradients."""
    c = D.case(M, V)
    s, t, gold = _dev(c)
    assert s.data_ptr() % 16 == 0 and (c["ld"] * 4) % 16 == 0
    for dtype in (torch.float32, torch.bfloat16):
        want = _run(s[:, :V], t[:, :V], gold, V, 0.1, 2.0, 0.6, 0.4, out_dtype=dtype)
        tight_s, tight_t = s[:, :V].contiguous(), t[:, :V].contiguous()
        views = [(tight_s, tight_t), (tight_s, t[:, :V]), (s[:, :V], tight_t)] if V % 4 else []
        for x in (s, t):
            buf = torch.zeros(x.numel() + 1, device="cuda")
            buf[1:] = x.reshape(-1)
            off = buf[1:].view(M, c["ld"])[:, :V]
            assert off.data_ptr() % 16 == 4
            views.append((off, t[:, :V]) if x is s else (s[:, :V], off))
        for sv, tv in views:
            assert _same(_run(sv, tv, gold, V, 0.1, 2.0, 0.6, 0.4, out_dtype=dtype), want)
        # and the gradient buffer on a stride that leaves its rows off the vector-store alignment
        odd = _run(s[:, :V], t[:, :V], gold, V, 0.1, 2.0, 0.6, 0.4, out_dtype=dtype, ldd=V + 1 + (V % 2))
        assert torch.equal(odd["dl"][:, :V], want["dl"][:, :V]) and bool((odd["dl"][:, V:].float() == 0).all()) and _sentinels_untouched(odd)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("M,V", [(7, 3), (9, 11), (9, 257), (64, 4364)])
def test_a_teacher_with_the_students_bits_gives_no_kd_at_all(M, V, tau):
    """Teacher bits == student bits: every kd_m and sums[3] are exactly 0 and the gradient is torch.equal to the same call with
    kd_scale = 0 (pS and pT come from one instruction sequence)."""
    c = D.case(M, V)
    s, _, gold = _dev(c)
    twin = s.clone()
    for dtype in (torch.float32, torch.bfloat16):
        o = _run(s[:, :V], twin[:, :V], gold, V, 0.1, tau, 0.6, 0.4, out_dtype=dtype)
        assert bool((o["stats"][:, 3] == 0).all()) and o["sums"][3].item() == 0.0
        assert torch.equal(o["stats"][:, 1], o["stats"][:, 2])
        z = _run(s[:, :V], twin[:, :V], gold, V, 0.1, tau, 0.6, 0.0, out_dtype=dtype)
        assert torch.equal(o["dl"], z["dl"]) and float(z["dl"].float().abs().max()) > 0


def test_two_identical_calls_give_identical_bits():
    c = D.case(64, 4364)
    s, t, gold = _dev(c)
    a = _run(s[:, :4364], t[:, :4364], gold, 4364, 0.1, 2.0, 0.6, 0.4, out_dtype=torch.bfloat16)
    b = _run(s[:, :4364], t[:, :4364], gold, 4364, 0.1, 2.0, 0.6, 0.4, out_dtype=torch.bfloat16)
    assert _same(a, b)


@pytest.mark.parametrize("M,V", [(7, 11), (9, 257)])
def test_without_the_ce_term_gold_only_marks_the_live_rows(M, V):
    """with_ce = 0: slots 0 and 2 of every partial and of sums are 0, argmax may be NULL (its buffer keeps its sentinels), and live
    rows whose gold lies far outside [0, V) are harmless; the KD statistics and gradient are the restatement's."""
    c = D.case(M, V)
    s, t, gold = _dev(c)
    wild = gold.clone()
    wild[gold != D.PAD] = torch.tensor([10 ** 12, -5, V, 2 ** 31 + 3])[torch.arange(int((gold != D.PAD).sum())) % 4]
    ref, b = _reference(M, V, 2.0, 0.0, 0.0, 1.0, with_ce=False)
    o = _run(s[:, :V], t[:, :V], wild, V, 0.0, 2.0, 0.0, 1.0, with_ce=False, argmax_null=True)
    _check(o, ref, b, V, what="M%d V%d with_ce=0" % (M, V))
    assert bool((o["part"][:, 0] == 0).all()) and bool((o["part"][:, 2] == 0).all()) and o["sums"][0].item() == 0 and o["sums"][2].item() == 0
    assert bool((o["full"]["am"] == S_I).all())
    plain = _run(s[:, :V], t[:, :V], gold, V, 0.0, 2.0, 0.0, 1.0, with_ce=False)
    assert _same(plain, o, keys=("stats", "part", "sums", "loss", "dl"))


@pytest.mark.parametrize("tau", [1.0, 2.0])
def test_a_confident_student_on_a_label_the_teacher_doubts(tau):
    """A student row 60 logits ahead on one label that the teacher gives little mass: log pS of the other labels is about -60 / tau,
    nothing under- or overflows, and loss, kd and gradient stay within the rule."""
    M, V = 7, 257
    c = D.case(M, V)
    sb, tb = c["s"].copy(), c["t"].copy()
    sb[0, :V] = 0.0
    sb[0, 5] = 60.0
    tb[0, 5] = -8.0
    gold = torch.from_numpy(c["gold"]).clone()
    gold[0] = 5
    a = (sb[:, :V], tb[:, :V], gold, 0.1, D.PAD, tau, 0.6, 0.4, GRAD_OUT, True)
    ref = D.distill(*a)
    b = D.bounds(*a, ref)
    assert float(ref["kd"][0]) > 20.0
    o = _run(torch.from_numpy(sb).cuda()[:, :V], torch.from_numpy(tb).cuda()[:, :V], gold, V, 0.1, tau, 0.6, 0.4)
    assert bool(torch.isfinite(o["stats"]).all()) and bool(torch.isfinite(o["dl"]).all()) and bool(torch.isfinite(o["loss"]))
    _check(o, ref, b, V, what="confident row, tau %g" % tau)


def test_refusals():
    """ASR_EINVAL for M < 1, V < 1, a leading dimension below V, a temperature outside [0.5, 16], a smoothing outside [0, 1), another
    out_dtype and a NULL required pointer; nothing is launched."""
    from asr_hip import lib as L
    M, V = 7, 11
    c = D.case(M, V)
    s, t, gold = _dev(c)
    g = gold.cuda()
    stats = torch.zeros(M, 4, device="cuda")
    am = torch.zeros(M, dtype=torch.int64, device="cuda")
    part = torch.zeros(4, device="cuda")
    one = torch.ones(1, device="cuda")
    dl = torch.zeros(M, 16, device="cuda")
    h = L.load()
    ld = c["ld"]

    def fwd(**k):
        a = dict(s=L.ptr(s), ld_s=ld, t=L.ptr(t), ld_t=ld, g=L.ptr(g), M=M, V=V, eps=0.1, tau=2.0, ce=1, st=L.ptr(stats), am=L.ptr(am),
                 part=L.ptr(part))
        a.update(k)
        return h.asr_distill_fwd(a["s"], a["ld_s"], a["t"], a["ld_t"], a["g"], a["M"], a["V"], a["eps"], D.PAD, a["tau"], a["ce"], a["st"], a["am"],
                                 a["part"], L.stream())

    def bwd(**k):
        a = dict(s=L.ptr(s), ld_s=ld, t=L.ptr(t), ld_t=ld, g=L.ptr(g), st=L.ptr(stats), M=M, V=V, eps=0.1, tau=2.0, go=L.ptr(one), n=L.ptr(one),
                 dl=L.ptr(dl), ldd=16, dt=L.F32)
        a.update(k)
        return h.asr_distill_bwd(a["s"], a["ld_s"], a["t"], a["ld_t"], a["g"], a["st"], a["M"], a["V"], a["eps"], D.PAD, a["tau"], 0.6, 0.4, a["go"],
                                 a["n"], a["dl"], a["ldd"], a["dt"], L.stream())
    assert fwd() == 0 and bwd() == 0 and fwd(ce=0, am=None) == 0
    EINVAL = -1
    for k in (dict(M=0), dict(V=0), dict(ld_s=V - 1), dict(ld_t=V - 1), dict(tau=0.49), dict(tau=16.5), dict(eps=-0.1), dict(eps=1.0),
              dict(s=None), dict(t=None), dict(g=None), dict(st=None)):
        assert fwd(**k) == EINVAL, k
        assert bwd(**k) == EINVAL, k
    for k in (dict(am=None), dict(part=None)):
        assert fwd(**k) == EINVAL, k
    for k in (dict(ldd=V - 1), dict(dt=2), dict(dt=-1), dict(go=None), dict(n=None), dict(dl=None)):
        assert bwd(**k) == EINVAL, k
    assert h.asr_distill_finish(None, 1, None, 1.0, 1.0, L.ptr(one), L.ptr(one), L.stream()) == EINVAL
    assert h.asr_distill_finish(L.ptr(part), 1, None, 1.0, 1.0, None, L.ptr(one), L.stream()) == EINVAL
    torch.cuda.synchronize()


def test_the_autograd_function_hands_back_the_kernel_gradient():
    """F_.DistillFn on plain (not handed-over) logits: loss, sums and the fp32 gradient of ops.distill_fwd / distill_bwd, no gradient for
    the teacher, and a second backward-free call with with_ce=False returns an empty argmax."""
    from asr_hip import functions as F_
    M, V = 9, 11
    c = D.case(M, V)
    s, t, gold = _dev(c)
    x = s[:, :V].contiguous().view(3, 3, V).requires_grad_()
    y = t[:, :V].contiguous().view(3, 3, V).requires_grad_()
    loss, sums, am = F_.DistillFn.apply(x, y, gold.cuda().view(3, 3), 0.1, D.PAD, 2.0, 0.6, 0.4, True)
    (loss * GRAD_OUT).backward()
    ref, b = _reference(M, V, 2.0, 0.1, 0.6, 0.4)
    assert y.grad is None and not sums.requires_grad and am.shape == (M,)
    assert D.excess(x.grad.reshape(M, V), ref["dlogits"], b["dlogits"]) <= 1.0
    assert D.excess(loss.detach().reshape(1), ref["loss"].reshape(1), b["loss"]) <= 1.0
    _, _, none = F_.DistillFn.apply(x.detach(), y.detach(), gold.cuda().view(3, 3), 0.0, D.PAD, 2.0, 0.0, 1.0, False)
    assert none.numel() == 0
