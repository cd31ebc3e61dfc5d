"""The pruned-transducer kernels (csrc/rnnt_pruned.hip) against the float64 restatement (tests/rnnt_pruned_reference.py).

Shapes: the house case B 3, T 7, Umax 5 with (T_b, U_b) = (7,5), (1,0), (3,2); V in {2, 63, 64, 65, 257} and one case at 4364; row strides
ld = V and ld > V with NaN in the pad columns; NaN in every dead row; T 70, U 66, V 257 crosses the 64-wide contraction tiles in all three
K's; T 300, U 299, V 3 for diagonals longer than the workgroup.  Tolerance, the rule of tests/test_gpu_rnnt.py: per tensor 4 x max(largest
|torch fp32 on the CPU - float64| of the same formula, one fp32 rounding of the largest entry), plus one bf16 rounding elementwise where
stored in bf16.  The band is NEVER compared with a band from float64 occupancies (the best and the second-best window routinely tie to
1e-10 and below): asr_rnnt_prune_ranges must equal the restatement run on hand-set dyadic occupancies and on the GPU's OWN gb / gl copied
to the host (the same fp64 additions in the same order), and the banded loss is always checked with the GPU's own s_begin handed to the
restatement.  Bit for bit (torch.equal): sentinels around every output, dead rows and pad columns zero, aligned against misaligned
bases, two identical calls, an utterance's outputs unchanged by its batch neighbours, W = U + 1 against ops.rnnt_fwd / ops.rnnt_bwd."""
import math

import pytest
import torch

import rnnt_pruned_reference as P
import rnnt_reference as R

pytestmark = pytest.mark.gpu

LAYOUTS = [(2, 2), (2, 8), (63, 63), (63, 68), (64, 64), (65, 65), (65, 72), (257, 257), (257, 264)]
HOUSE = dict(B=3, T=7, Umax=5, frames=(7, 1, 3), lengths=(5, 0, 2))
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ the simple loss
def _sdev(c):
    V = c["V"]
    return c["am"].to(DEV)[..., :V], c["lm"].to(DEV)[..., :V], c["targets"].to(DEV), c["frames"].to(DEV), c["lengths"].to(DEV)


def _srun(c, grad_out=None):
    from asr_hip import ops
    am, lm, tg, fr, tl = _sdev(c)
    B = am.shape[0]
    loss, ws, gb, gl = ops.rnnt_simple_fwd(am, lm, tg, fr, tl)
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=DEV)
    dam, dlm = ops.rnnt_simple_bwd(am.shape, lm.shape, tg, fr, tl, ws, go)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), nll=ws[-B:].cpu(), gb=gb.cpu(), gl=gl.cpu(), dam=dam.cpu(), dlm=dlm.cpu(), dev=(gb, gl, fr, tl))


_SREF = {}         # the restatement of a case, computed once and shared by the tests that need it (never modified)


def _sref(V, ld, grad_out=1.0, **kw):
    key = (V, ld, grad_out, repr(sorted(kw.items())))
    if key not in _SREF:
        c = P.simple_case(V, ld=ld, **kw)
        args = (c["am"], c["lm"], c["targets"], c["frames"], c["lengths"])
        _SREF[key] = (c, P.simple_loss_and_grad(*args, V=V, grad_out=grad_out),
                      P.simple_loss_and_grad(*args, V=V, grad_out=grad_out, dtype=torch.float32))
    return _SREF[key]


def _scheck(c, r64, r32, got, what):
    x = {}
    for k in ("nll", "loss", "gb", "gl", "dam", "dlm"):
        ref, r = r64[k].reshape(-1), r32[k].reshape(-1)
        x[k] = P.excess(got[k].reshape(-1), ref, P.bound32(ref, r))
    print("%s: error / bound %s" % (what, "  ".join("%s %.3f" % kv for kv in x.items())))
    assert all(v <= 1.0 for v in x.values()), (what, x)
    for b, (Tb, Ub) in enumerate(zip(c["frames"].tolist(), c["lengths"].tolist())):
        for k in ("gb", "gl"):
            assert not got[k][b, Tb:].any() and not got[k][b, :, Ub + 1:].any(), "dead cells of %s, utterance %d" % (k, b)
        assert not got["dam"][b, Tb:].any() and not got["dlm"][b, Ub + 1:].any(), "dead rows of utterance %d" % b
    assert float(got["dam"].abs().max()) > 0 and float(got["dlm"].abs().max()) > 0


@pytest.mark.parametrize("V,ld", LAYOUTS, ids=["V%d-ld%d" % p for p in LAYOUTS])
def test_simple_loss_and_gradient_against_the_restatement(V, ld):
    go = 0.7 if V == 65 else None
    c, r64, r32 = _sref(V, ld, grad_out=1.0 if go is None else go)
    _scheck(c, r64, r32, _srun(c, go), "simple V %d ld %d" % (V, ld))


def test_simple_loss_at_the_vocabulary_of_the_workload():
    c, r64, r32 = _sref(4364, 4364)
    _scheck(c, r64, r32, _srun(c), "simple V 4364")


def test_simple_loss_across_the_contraction_tiles_in_all_three_k():
    """T 70 and U + 1 = 67 cross the 64-row tiles (and are the K of the two gradient contractions), V 257 crosses the 64-column tiles and
    is K = 16 x 16 + 1 of the first."""
    kw = dict(B=2, T=70, Umax=66, frames=(70, 20), lengths=(66, 12), scale=1.0)
    c, r64, r32 = _sref(257, 257, **kw)
    _scheck(c, r64, r32, _srun(c), "simple T 70 U 66 V 257")


def test_simple_loss_with_a_repeated_label():
    kw = dict(HOUSE, labels={0: [3, 3, 3, 7, 3]})
    c, r64, r32 = _sref(65, 72, **kw)
    assert c["targets"][0].tolist() == [3, 3, 3, 7, 3]
    _scheck(c, r64, r32, _srun(c), "simple y = 3,3,3,7,3")


def test_simple_loss_past_the_stated_limit_stays_finite():
    """Spreads of 100 + 100 > 87: every product of the contraction underflows, the floor FLT_MIN takes over and nothing is inf or NaN."""
    c = P.simple_case(5, **HOUSE)
    for b, (Tb, Ub) in enumerate(zip(HOUSE["frames"], HOUSE["lengths"])):
        c["am"][b, :Tb, :5] = torch.tensor([0.0, 100.0, 0.0, 0.0, 0.0])
        c["lm"][b, :Ub + 1, :5] = torch.tensor([0.0, 0.0, 100.0, 0.0, 0.0])
    got = _srun(c)
    for k in ("loss", "nll", "gb", "gl", "dam", "dlm"):
        assert torch.isfinite(got[k]).all(), k


@pytest.mark.parametrize("what", ["frames", "blank", "low", "high"])
def test_simple_loss_without_alignment_is_infinite_and_the_neighbours_keep_their_bits(what):
    V = 65
    c, _, _ = _sref(V, 72)
    plain = _srun(c)
    bad = dict(c)
    bad["frames"], bad["targets"] = c["frames"].clone(), c["targets"].clone()
    b = 0
    if what == "frames":
        bad["frames"][b] = 0
    else:
        bad["targets"][b, 1] = {"blank": 0, "low": -3, "high": V}[what]
    got = _srun(bad)
    assert math.isinf(float(got["nll"][b])) and float(got["nll"][b]) > 0 and math.isinf(float(got["loss"]))
    for k in ("gb", "gl", "dam", "dlm"):
        assert not got[k][b].any(), k
        for i in (1, 2):
            assert torch.equal(got[k][i], plain[k][i]), (k, i)
    assert torch.equal(got["nll"][1:], plain["nll"][1:])


# ------------------------------------------------------------------------------------------------ the band
def _occ_host(gb, gl):
    return gb.cpu() + gl.cpu()                           # the kernel's fp32 addition


def test_prune_ranges_on_hand_set_dyadic_occupancies_ties_included():
    from asr_hip import ops
    g = torch.Generator().manual_seed(5)
    B, T, U1 = 6, 9, 8
    gb = torch.randint(0, 5, (B, T, U1), generator=g).float() / 8.0           # many equal window sums
    gl = torch.randint(0, 3, (B, T, U1), generator=g).float() / 4.0
    gb[0] = 0.25                                                              # every window ties: the lowest start, then the scans
    gl[0] = 0.0
    frames = torch.tensor([9, 9, 1, 0, 4, 9], dtype=torch.int32)
    lengths = torch.tensor([7, 3, 7, 7, 7, 0], dtype=torch.int32)
    for S in (2, 3, 5, 8, 64):
        s = ops.rnnt_prune_ranges(gb.to(DEV), gl.to(DEV), frames.to(DEV), lengths.to(DEV), S).cpu()
        want = P.prune_ranges(gb + gl, frames, lengths, S)
        assert s.dtype == torch.int32 and torch.equal(s, want), (S, s, want)
        W = min(S, U1)
        for b in range(B):
            Tb, Ub = int(frames[b]), int(lengths[b])
            if Ub + 1 > W and Tb > 0 and P.feasible(Tb, Ub, W):
                assert P.band_properties(s[b], Tb, Ub, W), (S, b, s[b])
            assert not s[b, Tb:].any()
    s = ops.rnnt_prune_ranges(gb.to(DEV), gl.to(DEV), frames.to(DEV), lengths.to(DEV), 3).cpu()
    assert s[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 3, 5]                       # ties pick 0; the end and the backward scan pull it up
    assert s[2].tolist() == [5, 0, 0, 0, 0, 0, 0, 0, 0]                       # T_b = 1: s(0) = fin, no band exists


@pytest.mark.parametrize("S", [2, 3, 5])
def test_prune_ranges_on_the_gpu_s_own_occupancies(S):
    from asr_hip import ops
    for V, kw in ((65, HOUSE), (257, dict(B=2, T=70, Umax=66, frames=(70, 20), lengths=(66, 12), scale=1.0))):
        c = P.simple_case(V, **kw)
        got = _srun(c)
        gb, gl, fr, tl = got["dev"]
        s = ops.rnnt_prune_ranges(gb, gl, fr, tl, S).cpu()
        assert torch.equal(s, P.prune_ranges(_occ_host(gb, gl), c["frames"], c["lengths"], S))
        W = min(S, kw["Umax"] + 1)
        for b, (Tb, Ub) in enumerate(zip(kw["frames"], kw["lengths"])):
            if Ub + 1 > W and P.feasible(Tb, Ub, W):
                assert P.band_properties(s[b], Tb, Ub, W), (S, b, s[b])
        assert torch.equal(s, ops.rnnt_prune_ranges(gb, gl, fr, tl, S).cpu())


# ------------------------------------------------------------------------------------------------ the banded loss
def _band(V, S, seed=0, ld=None, scale=2.0, B=3, T=7, Umax=5, frames=(7, 1, 3), lengths=(5, 0, 2)):
    """A banded case: the GPU's own band (simple loss on random am / lm, then asr_rnnt_prune_ranges) and random band logits (B,T,W,ld) with
    NaN in the pad columns and in every dead row (t >= T_b or s(t) + w > U_b)."""
    from asr_hip import ops
    kw = dict(B=B, T=T, Umax=Umax, frames=frames, lengths=lengths)
    sc = P.simple_case(V, seed=seed, scale=1.0, **kw)
    am, lm, tg, fr, tl = _sdev(sc)
    _, _, gb, gl = ops.rnnt_simple_fwd(am, lm, tg, fr, tl)
    s_dev = ops.rnnt_prune_ranges(gb, gl, fr, tl, S)
    s = s_dev.cpu()
    W = min(S, Umax + 1)
    ld = V if ld is None else ld
    g = torch.Generator().manual_seed(31 * V + S + seed)
    x = torch.full((B, T, W, ld), math.nan)
    for b in range(B):
        for t in range(frames[b]):
            for w in range(W):
                if int(s[b, t]) + w <= lengths[b]:
                    x[b, t, w, :V] = torch.randn(V, generator=g) * scale
    return dict(logits=x, targets=sc["targets"], frames=sc["frames"], lengths=sc["lengths"], s=s, V=V, ld=ld, W=W, Umax=Umax)


def _prun(c, out_dtype=torch.float32, grad_out=None, pad=8):
    from asr_hip import ops
    logits = c["logits"].to(DEV)[..., :c["V"]]
    tg, fr, tl, s = c["targets"].to(DEV), c["frames"].to(DEV), c["lengths"].to(DEV), c["s"].to(DEV)
    B = logits.shape[0]
    loss, ws = ops.rnnt_pruned_fwd(logits, tg, fr, tl, s, c["Umax"])
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=DEV)
    dl = ops.rnnt_pruned_bwd(logits, tg, fr, tl, s, c["Umax"], ws, go, out_dtype=out_dtype, pad=pad)
    torch.cuda.synchronize()
    return loss.cpu(), ws[-B:].cpu(), dl.cpu()


def _pref(c, grad_out=1.0):
    args = (c["logits"], c["targets"], c["frames"], c["lengths"], c["s"], c["Umax"])
    return (P.pruned_loss_and_grad(*args, V=c["V"], grad_out=grad_out),
            P.pruned_loss_and_grad(*args, V=c["V"], grad_out=grad_out, dtype=torch.float32))


def _pcheck(c, r64, r32, got, out_dtype, what, finite=True):
    loss, nll, dl = got
    B, T, W = c["logits"].shape[:3]
    V = c["V"]
    fin = torch.isfinite(r64["nll"])
    assert torch.equal(torch.isinf(nll), ~fin) and bool((nll[~fin] > 0).all())
    x_nll = P.excess(nll[fin], r64["nll"][fin], P.bound32(r64["nll"], r32["nll"]))
    x_loss = P.excess(loss, r64["loss"].reshape(1), P.bound32(r64["loss"].reshape(1), r32["loss"].reshape(1))) if finite else 0.0
    full = dl.float().view(B, T, W, -1)
    x_dl = P.excess(full[..., :V], r64["dlogits"], P.bound32(r64["dlogits"], r32["dlogits"]), bf16_stored=out_dtype == torch.bfloat16)
    print("%s: nll error / bound %.3f, loss %.3f, gradient %.3f" % (what, x_nll, x_loss, x_dl))
    assert x_nll <= 1.0 and x_loss <= 1.0 and x_dl <= 1.0, (what, x_nll, x_loss, x_dl)
    assert dl.dtype == out_dtype and not full[..., V:].any(), "pad columns"
    for b, (Tb, Ub) in enumerate(zip(c["frames"].tolist(), c["lengths"].tolist())):
        assert not full[b, Tb:].any(), "dead frames of utterance %d" % b
        for t in range(Tb):
            first_dead = max(0, min(W, Ub + 1 - int(c["s"][b, t])))
            assert not full[b, t, first_dead:].any(), "dead band cells of utterance %d" % b
    assert float(full.abs().max()) > 0


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("V,ld", [(2, 8), (63, 63), (64, 64), (65, 72), (257, 257)])
def test_banded_loss_and_gradient_against_the_restatement(V, ld, S, out_dtype):
    c = _band(V, S, ld=ld)
    go = 0.7 if V == 65 else None
    r64, r32 = _pref(c, 1.0 if go is None else go)
    assert torch.isfinite(r64["nll"]).all() and float(r64["nll"][0]) > 0
    pad = 64 if out_dtype == torch.bfloat16 else 8
    got = _prun(c, out_dtype, go, pad)
    assert got[2].shape == (3 * 7 * S, (V + 63) // 64 * 64 if pad == 64 else V)
    _pcheck(c, r64, r32, got, out_dtype, "band V %d ld %d S %d %s" % (V, ld, S, out_dtype))


def test_banded_loss_at_the_vocabulary_of_the_workload():
    c = _band(4364, 3)
    r64, r32 = _pref(c)
    _pcheck(c, r64, r32, _prun(c, torch.bfloat16, None, 64), torch.bfloat16, "band V 4364 S 3")


def test_banded_loss_is_never_below_the_full_loss_on_the_same_logits():
    from asr_hip import ops
    full = R.case(65, ld=72)
    c = _band(65, 3, ld=72)
    x = torch.nan_to_num(full["logits"], nan=0.0)
    c = dict(c, logits=P.gather_band(x, c["s"], 3), targets=full["targets"])
    _, nll_p, _ = _prun(c)
    _, ws = ops.rnnt_fwd(x.to(DEV)[..., :65], full["targets"].to(DEV), full["frames"].to(DEV), full["lengths"].to(DEV))
    nll_f = ws[-3:].cpu()
    assert bool((nll_p >= nll_f).all()) and float(nll_p[0]) > float(nll_f[0]), (nll_p, nll_f)
    assert torch.equal(nll_p[1:], nll_f[1:])               # U_b + 1 <= W: the band is the whole lattice


def test_banded_diagonals_longer_than_the_workgroup():
    kw = dict(B=2, T=300, Umax=299, frames=(300, 150), lengths=(299, 100))
    c = _band(3, 4, scale=1.0, **kw)
    for b in range(2):
        assert P.band_properties(c["s"][b], kw["frames"][b], kw["lengths"][b], 4)
    r64, r32 = _pref(c)
    assert torch.isfinite(r64["nll"]).all()
    _pcheck(c, r64, r32, _prun(c), torch.float32, "band T 300 U 299 V 3 S 4")


@pytest.mark.parametrize("out_dtype,pad", [(torch.float32, 8), (torch.bfloat16, 64)], ids=["f32", "bf16"])
def test_an_utterance_without_a_band_is_infinite_and_its_neighbours_keep_their_bits(out_dtype, pad):
    """(T_b, U_b) = (1, 4) with S = 2: (T_b - 1)(W - 1) < fin, no path stays inside any band."""
    ok = _band(65, 2, ld=72)
    bad = _band(65, 2, ld=72, lengths=(5, 4, 2))
    assert int(bad["s"][1, 0]) == 3                         # s(0) = fin: node (0,0) is outside its own band
    for k in (0, 2):                                        # the neighbours: the band, the logits and the labels of the feasible batch
        bad["logits"][k], bad["s"][k], bad["targets"][k] = ok["logits"][k], ok["s"][k], ok["targets"][k]
    r64, r32 = _pref(bad)
    assert math.isinf(float(r64["nll"][1])) and not r64["dlogits"][1].any()
    want, got = _prun(ok, out_dtype, None, pad), _prun(bad, out_dtype, None, pad)
    _pcheck(bad, r64, r32, got, out_dtype, "no band %s" % out_dtype, finite=False)
    assert math.isinf(float(got[0])) and float(got[0]) > 0
    dl, ref = got[2].view(3, 7, 2, -1), want[2].view(3, 7, 2, -1)
    assert not dl[1].any()
    for i in (0, 2):
        assert torch.equal(got[1][i], want[1][i]) and torch.equal(dl[i], ref[i]), i


@pytest.mark.parametrize("V,ld", [(63, 63), (65, 72), (257, 264)])
def test_the_whole_lattice_as_a_band_is_the_full_loss_bit_for_bit(V, ld):
    from asr_hip import ops
    c = R.case(V, ld=ld)
    logits, tg, fr, tl = c["logits"].to(DEV)[..., :V], c["targets"].to(DEV), c["frames"].to(DEV), c["lengths"].to(DEV)
    s = torch.zeros((3, 7), dtype=torch.int32, device=DEV)
    go = torch.tensor([0.3], device=DEV)
    loss_f, ws_f = ops.rnnt_fwd(logits, tg, fr, tl)
    loss_p, ws_p = ops.rnnt_pruned_fwd(logits, tg, fr, tl, s, 5)
    assert ws_f.numel() == ws_p.numel()
    assert torch.equal(loss_f, loss_p) and torch.equal(ws_f[-3:], ws_p[-3:]) and math.isfinite(float(loss_f))
    for out_dtype, pad in ((torch.float32, 8), (torch.bfloat16, 64)):
        d_f = ops.rnnt_bwd(logits, tg, fr, tl, ws_f, go, out_dtype=out_dtype, pad=pad)
        d_p = ops.rnnt_pruned_bwd(logits, tg, fr, tl, s, 5, ws_p, go, out_dtype=out_dtype, pad=pad)
        assert torch.equal(d_f, d_p) and float(d_f.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the banded joint
def _monotone_s(B, T, U1, W, g):
    s = torch.zeros((B, T), dtype=torch.int32)
    for b in range(B):
        for t in range(1, T):
            s[b, t] = min(U1 - W, int(s[b, t - 1]) + int(torch.randint(0, W, (1,), generator=g)))
    return s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [8, 72, 256])
def test_banded_joint_against_the_restatement(J, dtype):
    from asr_hip import ops
    bf = dtype == torch.bfloat16
    g = torch.Generator().manual_seed(J)
    B, T, U1, W = 2, 9, 11, 3
    s = _monotone_s(B, T, U1, W, g)
    e = (torch.randn((B, T, J), generator=g) * 1.5).to(dtype)
    p = (torch.randn((B, U1, J), generator=g) * 1.5).to(dtype)
    dz = torch.randn((B, T, W, J), generator=g).to(dtype)
    z = ops.rnnt_joint_pruned(e.to(DEV), p.to(DEV), s.to(DEV), W)
    z64, z32 = P.joint_pruned(e, p, s, W), P.joint_pruned(e, p, s, W, torch.float32)
    assert z.dtype == dtype and tuple(z.shape) == (B, T, W, J)
    x = P.excess(z.float(), z64, P.bound32(z64, z32), bf16_stored=bf)
    de, dp = ops.rnnt_joint_pruned_bwd(dz.to(DEV), z, s.to(DEV), U1)
    zc = z.cpu()
    (de64, dp64), (de32, dp32) = P.joint_pruned_bwd(dz, zc, s, U1), P.joint_pruned_bwd(dz, zc, s, U1, torch.float32)
    xe = P.excess(de.float(), de64, P.bound32(de64, de32), bf16_stored=bf)
    xp = P.excess(dp.float(), dp64, P.bound32(dp64, dp32), bf16_stored=bf)
    print("J %d %s: z error / bound %.3f, de %.3f, dp %.3f" % (J, dtype, x, xe, xp))
    assert x <= 1.0 and xe <= 1.0 and xp <= 1.0
    again = ops.rnnt_joint_pruned_bwd(dz.to(DEV), z, s.to(DEV), U1)
    assert torch.equal(again[0], de) and torch.equal(again[1], dp) and torch.equal(ops.rnnt_joint_pruned(e.to(DEV), p.to(DEV), s.to(DEV), W), z)
    # the whole lattice as a band is the full joint
    zero = torch.zeros((B, T), dtype=torch.int32, device=DEV)
    assert torch.equal(ops.rnnt_joint_pruned(e.to(DEV), p.to(DEV), zero, U1), ops.rnnt_joint(e.to(DEV), p.to(DEV)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,U1,W,J", [(6, 5, 2, 8), (6, 9, 3, 72), (70, 40, 5, 72), (6, 4, 4, 256)])
def test_banded_joint_reductions_are_exact_on_small_integers(T, U1, W, J, dtype):
    """z handed in from {0, 1}, dz from {-1, 0, 1}: every partial sum (at most 70 terms) is an integer that fp32 and bf16 hold exactly."""
    from asr_hip import ops
    g = torch.Generator().manual_seed(T * 1000 + J)
    B = 2
    s = _monotone_s(B, T, U1, W, g)
    z = torch.randint(0, 2, (B, T, W, J), generator=g).to(dtype)
    dz = torch.randint(-1, 2, (B, T, W, J), generator=g).to(dtype)
    de, dp = ops.rnnt_joint_pruned_bwd(dz.to(DEV), z.to(DEV), s.to(DEV), U1)
    de64, dp64 = P.joint_pruned_bwd(dz, z, s, U1)
    assert torch.equal(de.cpu().double(), de64) and torch.equal(dp.cpu().double(), dp64) and float(dp64.abs().max()) > 1


# ------------------------------------------------------------------------------------------------ bit for bit
def test_sentinels_around_every_output():
    from asr_hip import lib as L
    lib = L.load()
    V, ld, G = 65, 72, 64
    B, T, U, S = 3, 7, 5, 3
    U1 = U + 1
    sc, r64, r32 = _sref(V, ld)
    am, lm, tg, fr, tl = _sdev(sc)
    n = int(lib.asr_rnnt_simple_workspace(B, T, U, V))
    assert n == 10 * B * T * U1 + 3 * B + B * (T + U1) * (1 + V)

    def guarded(numel, dtype=torch.float32):
        return torch.full((numel + 2 * G,), -7, device=DEV, dtype=dtype)

    ws, loss, dam, dlm, s = guarded(n), guarded(1), guarded(B * T * V), guarded(B * U1 * V), guarded(B * T, torch.int32)
    L.call("asr_rnnt_simple_fwd", L.ptr(am), ld, L.ptr(lm), ld, L.ptr(tg), L.ptr(fr), L.ptr(tl), B, T, U, V, 0, L.ptr(ws[G:]), n, L.ptr(loss[G:]),
           L.stream())
    L.call("asr_rnnt_simple_bwd", L.ptr(tg), L.ptr(fr), L.ptr(tl), B, T, U, V, 0, L.ptr(ws[G:]), None, L.ptr(dam[G:]), L.ptr(dlm[G:]), L.stream())
    cells = B * T * U1
    gb = ws[G + 6 * cells + 2 * B:G + 7 * cells + 2 * B]
    gl = ws[G + 7 * cells + 2 * B:G + 8 * cells + 2 * B]
    L.call("asr_rnnt_prune_ranges", L.ptr(gb), L.ptr(gl), L.ptr(fr), L.ptr(tl), B, T, U, S, L.ptr(s[G:]), L.stream())
    plain = _srun(sc)
    assert torch.equal(loss[G:-G].cpu(), plain["loss"]) and torch.equal(dam[G:-G].cpu().view(B, T, V), plain["dam"])
    assert torch.equal(dlm[G:-G].cpu().view(B, U1, V), plain["dlm"]) and torch.equal(gb.cpu().view(B, T, U1), plain["gb"])
    # the band, its joint and its loss
    c = _band(V, S, ld=ld)
    logits, sb = c["logits"].to(DEV)[..., :V], c["s"].to(DEV)
    J = 72
    e, p = torch.randn((B, T, J), device=DEV), torch.randn((B, U1, J), device=DEV)
    z, de, dp = guarded(B * T * S * J), guarded(B * T * J), guarded(B * U1 * J)
    L.call("asr_rnnt_joint_pruned_fwd", L.ptr(e), L.ptr(p), L.ptr(sb), L.ptr(z[G:]), B, T, U1, S, J, L.F32, L.stream())
    dz = torch.randn((B, T, S, J), device=DEV)
    L.call("asr_rnnt_joint_pruned_bwd", L.ptr(dz), L.ptr(z[G:]), L.ptr(sb), L.ptr(de[G:]), L.ptr(dp[G:]), B, T, U1, S, J, L.F32, L.stream())
    m = int(lib.asr_rnnt_pruned_workspace(B, T, U, S))
    assert m == 6 * cells + B * T * S + 3 * B
    outs = [("simple workspace", ws), ("loss", loss), ("dam", dam), ("dlm", dlm), ("s_begin", s), ("z", z), ("de", de), ("dp", dp)]
    for out_dtype, ldd in ((torch.float32, 72), (torch.bfloat16, 128)):
        pws, ploss, dl = guarded(m), guarded(1), guarded(B * T * S * ldd, out_dtype)
        L.call("asr_rnnt_pruned_fwd", L.ptr(logits), ld, L.ptr(tg), L.ptr(fr), L.ptr(tl), L.ptr(sb), B, T, U, S, V, 0, L.ptr(pws[G:]), m,
               L.ptr(ploss[G:]), L.stream())
        L.call("asr_rnnt_pruned_bwd", L.ptr(logits), ld, L.ptr(tg), L.ptr(fr), L.ptr(tl), L.ptr(sb), B, T, U, S, V, 0, L.ptr(pws[G:]), None,
               L.ptr(dl[G:]), ldd, L.dt(dl), L.stream())
        outs += [("pruned workspace", pws), ("pruned loss", ploss), ("dlogits %s" % out_dtype, dl)]
        want = _prun(c, out_dtype, None, 64 if out_dtype == torch.bfloat16 else 8)
        assert torch.equal(ploss[G:-G].cpu(), want[0]) and torch.equal(dl[G:-G].cpu().view(-1, ldd)[:, :want[2].shape[1]], want[2])
    torch.cuda.synchronize()
    for name, buf in outs:
        guard = torch.full((G,), -7, dtype=buf.dtype)
        assert torch.equal(buf[:G].cpu(), guard) and torch.equal(buf[-G:].cpu(), guard), name


@pytest.mark.parametrize("V", [63, 64, 257])
def test_aligned_and_misaligned_bases_give_the_same_bits(V):
    """am, lm and the band logits at a 16-byte aligned base and one float behind it, the gradient at an aligned and a misaligned base."""
    from asr_hip import ops
    sc, _, _ = _sref(V, V)
    c = _band(V, 3)
    out = []
    for off in (0, 1):
        def shifted(x):
            buf = torch.zeros(x.numel() + 4, device=DEV)
            buf[off:off + x.numel()].copy_(x.reshape(-1))
            v = buf[off:off + x.numel()].view(x.shape)
            assert (v.data_ptr() % 16 == 0) == (off == 0)
            return v
        tg, fr, tl = sc["targets"].to(DEV), sc["frames"].to(DEV), sc["lengths"].to(DEV)
        am, lm = shifted(sc["am"]), shifted(sc["lm"])
        loss, ws, gb, gl = ops.rnnt_simple_fwd(am, lm, tg, fr, tl)
        dam, dlm = ops.rnnt_simple_bwd(am.shape, lm.shape, tg, fr, tl, ws)
        logits, s = shifted(c["logits"]), c["s"].to(DEV)
        ploss, pws = ops.rnnt_pruned_fwd(logits, c["targets"].to(DEV), fr, tl, s, 5)
        dl = torch.zeros(3 * 7 * 3 * V + 4, device=DEV)
        from asr_hip import lib as L
        L.call("asr_rnnt_pruned_bwd", L.ptr(logits), V, L.ptr(c["targets"].to(DEV)), L.ptr(fr), L.ptr(tl), L.ptr(s), 3, 7, 5, 3, V, 0, L.ptr(pws), None,
               L.ptr(dl[off:]), V, L.F32, L.stream())
        torch.cuda.synchronize()
        out.append([t.cpu() for t in (loss, gb, gl, dam, dlm, ploss, pws[-3:], dl[off:off + 3 * 7 * 3 * V])])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_two_identical_calls_give_the_same_bits():
    sc, _, _ = _sref(257, 264)
    a, b = _srun(sc, 0.3), _srun(sc, 0.3)
    for k in ("loss", "nll", "gb", "gl", "dam", "dlm"):
        assert torch.equal(a[k], b[k]), k
    c = _band(257, 3, ld=264)
    for out_dtype, pad in ((torch.float32, 8), (torch.bfloat16, 64)):
        a, b = _prun(c, out_dtype, 0.3, pad), _prun(c, out_dtype, 0.3, pad)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_an_utterance_is_unchanged_by_its_batch_neighbours():
    """Utterance 0 alone (B 1, grad_out 1) and in the batch of three (grad_out 3: the same coefficient 1 / U_b): the same bits in every
    output, the band included."""
    from asr_hip import ops
    V = 65
    sc, _, _ = _sref(V, 72)
    alone = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in sc.items()}
    a, b = _srun(alone, 1.0), _srun(sc, 3.0)
    for k in ("nll", "gb", "gl", "dam", "dlm"):
        assert torch.equal(a[k][0], b[k][0]), k
    sa = ops.rnnt_prune_ranges(*a["dev"], 3).cpu()
    sb = ops.rnnt_prune_ranges(*b["dev"], 3).cpu()
    assert torch.equal(sa[0], sb[0])
    c = _band(V, 3, ld=72)
    one = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in c.items()}
    pa, pb = _prun(one, torch.float32, 1.0), _prun(c, torch.float32, 3.0)
    assert torch.equal(pa[1][0], pb[1][0]) and torch.equal(pa[2].view(1, 7, 3, V)[0], pb[2].view(3, 7, 3, V)[0])


def test_argument_errors():
    from asr_hip import lib as L
    lib = L.load()
    sc, _, _ = _sref(65, 72)
    am, lm, tg, fr, tl = _sdev(sc)
    n = int(lib.asr_rnnt_simple_workspace(3, 7, 5, 65))
    ws, loss = torch.empty(n, device=DEV), torch.empty(1, device=DEV)
    args = lambda **k: [L.ptr(am), k.get("ld", 72), L.ptr(lm), 72, L.ptr(tg), L.ptr(fr), L.ptr(tl), 3, k.get("T", 7), 5, k.get("V", 65),  # noqa: E731
                        k.get("blank", 0), L.ptr(ws), k.get("n", n), L.ptr(loss), L.stream()]
    for k in (dict(ld=64), dict(T=0), dict(V=0), dict(blank=65), dict(blank=-1), dict(n=n - 1)):
        assert lib.asr_rnnt_simple_fwd(*args(**k)) == -1, k
    s = torch.zeros((3, 7), dtype=torch.int32, device=DEV)
    assert lib.asr_rnnt_prune_ranges(L.ptr(ws), L.ptr(ws), L.ptr(fr), L.ptr(tl), 3, 7, 5, 0, L.ptr(s), L.stream()) == -1           # S < 1
    e = torch.zeros(3 * 7 * 8 * 12, device=DEV)
    assert lib.asr_rnnt_joint_pruned_fwd(L.ptr(e), L.ptr(e), L.ptr(s), L.ptr(e), 3, 7, 6, 3, 12, L.F32, L.stream()) == L.EUNSUPPORTED   # J % 8
    assert lib.asr_rnnt_joint_pruned_fwd(L.ptr(e), L.ptr(e), L.ptr(s), L.ptr(e), 3, 7, 6, 7, 8, L.F32, L.stream()) == -1           # W > U1
    assert lib.asr_rnnt_pruned_workspace(3, 7, 5, 7) == 0
    m = int(lib.asr_rnnt_pruned_workspace(3, 7, 5, 3))
    pws = torch.empty(m, device=DEV)
    x = torch.zeros(3 * 7 * 3 * 72, device=DEV)
    assert lib.asr_rnnt_pruned_fwd(L.ptr(x), 72, L.ptr(tg), L.ptr(fr), L.ptr(tl), L.ptr(s), 3, 7, 5, 3, 65, 0, L.ptr(pws), m - 1, L.ptr(loss),
                                   L.stream()) == -1
    assert lib.asr_rnnt_pruned_bwd(L.ptr(x), 72, L.ptr(tg), L.ptr(fr), L.ptr(tl), L.ptr(s), 3, 7, 5, 3, 65, 0, L.ptr(pws), None, L.ptr(x), 64, L.F32,
                                   L.stream()) == -1                                                                               # ldd < V
    torch.cuda.synchronize()
