"""The transducer kernels (csrc/rnnt.hip) against the float64 restatement (tests/rnnt_reference.py).

Shapes: B 3, T 7, Umax 5 with (T_b, U_b) = (7,5), (1,0), (3,2); V in {2, 63, 64, 65, 257} and one case at 4364; row strides ld = V
(misaligned row bases at V = 63, 65, 257) and ld > V with NaN in the pad columns; NaN in every dead row; T 300, U 299, V 3 for diagonals
longer than the workgroup.  Tolerance of the loss and the fp32 gradient, the rule of tests/test_gpu_mwer.py: per tensor 4 x max(largest
|torch fp32 on the CPU - float64| of the same formula, one fp32 rounding of the largest entry), plus one bf16 rounding elementwise where
the output is stored in bf16.  Bit for bit (torch.equal): sentinels around every output, dead rows and pad columns zero, the +inf
utterance's rows zero with its neighbours' bits unchanged, an aligned against a misaligned base, two identical calls."""
import math

import pytest
import torch

import rnnt_reference as R

pytestmark = pytest.mark.gpu

LAYOUTS = [(2, 2), (2, 8), (63, 63), (63, 68), (64, 64), (65, 65), (65, 72), (257, 257), (257, 264)]


def _dev(c):
    d = torch.device("cuda")
    return (c["logits"].to(d)[..., :c["V"]], c["targets"].to(d), c["frames"].to(d), c["lengths"].to(d))


def _run(c, out_dtype=torch.float32, grad_out=None, pad=8):
    from asr_hip import ops
    logits, tg, fr, tl = _dev(c)
    B = logits.shape[0]
    loss, ws = ops.rnnt_fwd(logits, tg, fr, tl)
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=logits.device)
    dl = ops.rnnt_bwd(logits, tg, fr, tl, ws, go, out_dtype=out_dtype, pad=pad)
    torch.cuda.synchronize()
    return loss.cpu(), ws[-B:].cpu(), dl.cpu(), ws.cpu()


_REF = {}          # the restatement of a case, computed once and shared by the tests that need it (never modified)


def _ref(V, ld, grad_out=1.0, **kw):
    key = (V, ld, grad_out, tuple(sorted(kw.items())))
    if key not in _REF:
        c = R.case(V, ld=ld, **kw)
        r64 = R.loss_and_grad(c["logits"], c["targets"], c["frames"], c["lengths"], V=V, grad_out=grad_out)
        r32 = R.loss_and_grad(c["logits"], c["targets"], c["frames"], c["lengths"], V=V, grad_out=grad_out, dtype=torch.float32)
        _REF[key] = (c, r64, r32)
    return _REF[key]


def _check(c, r64, r32, got, out_dtype, V, what):
    loss, nll, dl, _ = got
    B, T, U1 = c["logits"].shape[:3]
    b_nll = R.bound32(r64["nll"], r32["nll"])
    x_nll = R.excess(nll, r64["nll"], b_nll)
    b_loss = R.bound32(r64["loss"].reshape(1), r32["loss"].reshape(1))
    x_loss = R.excess(loss, r64["loss"].reshape(1), b_loss)
    b_dl = R.bound32(r64["dlogits"], r32["dlogits"])
    full = dl.float().view(B, T, U1, -1)
    x_dl = R.excess(full[..., :V], r64["dlogits"], b_dl, bf16_stored=out_dtype == torch.bfloat16)
    print("%s: nll error / bound %.3f (bound %.3e), loss %.3f, gradient %.3f (fp32 bound %.3e)" % (what, x_nll, b_nll, x_loss, x_dl, b_dl))
    assert x_nll <= 1.0 and x_loss <= 1.0 and x_dl <= 1.0, (what, x_nll, x_loss, x_dl)
    assert dl.dtype == out_dtype
    assert torch.equal(full[..., V:], torch.zeros_like(full[..., V:])), "pad columns"
    for b, (Tb, Ub) in enumerate(zip(c["frames"].tolist(), c["lengths"].tolist())):
        assert torch.equal(full[b, Tb:], torch.zeros_like(full[b, Tb:])) and torch.equal(full[b, :, Ub + 1:], torch.zeros_like(full[b, :, Ub + 1:])), \
            "dead rows of utterance %d" % b
    assert float(full.abs().max()) > 0


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,ld", LAYOUTS, ids=["V%d-ld%d" % p for p in LAYOUTS])
def test_loss_and_gradient_against_the_restatement(V, ld, out_dtype):
    go = 0.7 if V == 65 else None
    c, r64, r32 = _ref(V, ld, grad_out=1.0 if go is None else go)
    pad = 64 if out_dtype == torch.bfloat16 else 8
    got = _run(c, out_dtype, go, pad)
    assert got[2].shape == (3 * 7 * 6, (V + 63) // 64 * 64 if pad == 64 else V)          # (pad 8: the (M,V) view of the padded buffer)
    _check(c, r64, r32, got, out_dtype, V, "V %d ld %d %s" % (V, ld, out_dtype))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_vocabulary_of_the_workload(out_dtype):
    c, r64, r32 = _ref(4364, 4364)
    _check(c, r64, r32, _run(c, out_dtype, None, 64), out_dtype, 4364, "V 4364 %s" % out_dtype)


def test_diagonals_longer_than_the_workgroup():
    """T 300, U 299, V 3 (rows at 12-byte steps): up to 300 cells on a diagonal, strided over 256 threads; a second, short utterance."""
    kw = dict(B=2, T=300, Umax=299, frames=(300, 4), lengths=(299, 260), scale=1.0)
    c, r64, r32 = _ref(3, 3, **kw)
    assert math.isfinite(float(r64["nll"][0])) and math.isfinite(float(r64["nll"][1]))
    got = _run(c)
    _check(c, r64, r32, got, torch.float32, 3, "T 300 U 299 V 3")
    # the lattice itself, where the restatement has it: alpha and beta of the long utterance
    ws = got[3]
    rows = 2 * 300 * 300
    lat = ws[:4 * rows].view(torch.float64)              # the workspace opens with alpha and beta in fp64
    alpha, beta = lat[:rows].view(2, 300, 300)[0], lat[rows:].view(2, 300, 300)[0]
    a64, b64, _ = r64["lattice"][0]
    a32, b32_, _ = r32["lattice"][0]
    assert R.excess(alpha, a64, R.bound32(a64, a32)) <= 1.0 and R.excess(beta, b64, R.bound32(b64, b32_)) <= 1.0


def test_sentinels_around_every_output():
    from asr_hip import lib as L
    dev = torch.device("cuda")
    V, ld = 65, 72
    c, r64, r32 = _ref(V, ld)
    logits, tg, fr, tl = _dev(c)
    B, T, U = 3, 7, 5
    n = int(L.load().asr_rnnt_workspace(B, T, U))
    assert n == 7 * B * T * (U + 1) + 3 * B
    G = 64
    for out_dtype, ldd in ((torch.float32, 72), (torch.bfloat16, 128)):
        ws = torch.full((n + 2 * G,), -7.0, device=dev)
        loss = torch.full((1 + 2 * G,), -7.0, device=dev)
        dl = torch.full((B * T * (U + 1) * ldd + 2 * G,), -7.0, device=dev, dtype=out_dtype)
        L.call("asr_rnnt_fwd", L.ptr(logits), ld, L.ptr(tg), L.ptr(fr), L.ptr(tl), B, T, U, V, 0, L.ptr(ws[G:]), n, L.ptr(loss[G:]), L.stream())
        L.call("asr_rnnt_bwd", L.ptr(logits), ld, L.ptr(tg), L.ptr(fr), L.ptr(tl), B, T, U, V, 0, L.ptr(ws[G:]), None, L.ptr(dl[G:]), ldd,
               L.dt(dl), L.stream())
        torch.cuda.synchronize()
        for name, buf in (("workspace", ws), ("loss", loss), ("dlogits", dl)):
            guard = torch.full((G,), -7.0, dtype=buf.dtype)
            assert torch.equal(buf[:G].cpu(), guard) and torch.equal(buf[-G:].cpu(), guard), name
        got = (loss[G:G + 1].cpu(), ws[G + n - B:G + n].cpu(), dl[G:-G].view(-1, ldd).cpu(), None)
        _check(c, r64, r32, got, out_dtype, V, "sentinels %s" % out_dtype)
        if out_dtype == torch.float32:
            plain = _run(c)
            assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1]) and torch.equal(plain[2], got[2][:, :V])


@pytest.mark.parametrize("what", ["frames", "blank", "low", "high"])
def test_an_utterance_without_alignment_is_infinite_and_its_neighbours_keep_their_bits(what):
    V = 65
    c, _, _ = _ref(V, 72)
    plain = _run(c)
    bad = dict(c)
    bad["frames"], bad["targets"] = c["frames"].clone(), c["targets"].clone()
    for b in (0, 2):
        if what == "frames":
            bad["frames"][b] = 0
        else:
            bad["targets"][b, 1] = {"blank": 0, "low": -3, "high": V}[what]
        for out_dtype, pad in ((torch.float32, 8), (torch.bfloat16, 64)):
            want = plain if out_dtype == torch.float32 else _run(c, out_dtype, None, pad)
            loss, nll, dl, _ = _run(bad, out_dtype, None, pad)
            assert math.isinf(float(nll[b])) and float(nll[b]) > 0 and math.isinf(float(loss)) and float(loss) > 0
            dl, ref = dl.view(3, 7, 6, -1), want[2].view(3, 7, 6, -1)
            assert torch.equal(dl[b], torch.zeros_like(dl[b]))
            keep = [i for i in range(3) if i != b and not math.isinf(float(nll[i]))]
            assert 1 in keep
            for i in keep:
                assert torch.equal(nll[i], want[1][i]) and torch.equal(dl[i], ref[i]), (what, b, i)


@pytest.mark.parametrize("V", [63, 64, 257])
def test_an_aligned_and_a_misaligned_base_give_the_same_bits(V):
    """The same logits at a 16-byte aligned base and one float behind it (the scalar load arm of the row pass and of the backward), the
    gradient at an aligned and a misaligned base: one set of bits."""
    from asr_hip import lib as L
    dev = torch.device("cuda")
    c, _, _ = _ref(V, V)
    B, T, U = 3, 7, 5
    _, tg, fr, tl = _dev(c)
    flat = c["logits"].reshape(-1)
    n = int(L.load().asr_rnnt_workspace(B, T, U))
    out = []
    for off_in, off_out in ((0, 0), (1, 0), (0, 1), (1, 3)):
        buf = torch.zeros(flat.numel() + 4, device=dev)
        buf[off_in:off_in + flat.numel()].copy_(flat)
        ws = torch.empty(n, device=dev)
        loss = torch.empty(1, device=dev)
        dl = torch.zeros(B * T * (U + 1) * V + 4, device=dev)
        x = buf[off_in:]
        assert (x.data_ptr() % 16 == 0) == (off_in == 0)
        L.call("asr_rnnt_fwd", L.ptr(x), V, L.ptr(tg), L.ptr(fr), L.ptr(tl), B, T, U, V, 0, L.ptr(ws), n, L.ptr(loss), L.stream())
        L.call("asr_rnnt_bwd", L.ptr(x), V, L.ptr(tg), L.ptr(fr), L.ptr(tl), B, T, U, V, 0, L.ptr(ws), None, L.ptr(dl[off_out:]), V, L.F32,
               L.stream())
        torch.cuda.synchronize()
        out.append((loss.cpu(), ws[-B:].cpu(), dl[off_out:off_out + B * T * (U + 1) * V].cpu()))
    for o in out[1:]:
        assert torch.equal(o[0], out[0][0]) and torch.equal(o[1], out[0][1]) and torch.equal(o[2], out[0][2])


def test_two_identical_calls_give_the_same_bits():
    c, _, _ = _ref(257, 264)
    for out_dtype, pad in ((torch.float32, 8), (torch.bfloat16, 64)):
        a, b = _run(c, out_dtype, 0.3, pad), _run(c, out_dtype, 0.3, pad)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_argument_errors():
    from asr_hip import lib as L
    c, _, _ = _ref(65, 72)
    logits, tg, fr, tl = _dev(c)
    n = int(L.load().asr_rnnt_workspace(3, 7, 5))
    ws, loss = torch.empty(n, device="cuda"), torch.empty(1, device="cuda")
    lib = L.load()
    args = lambda **k: [L.ptr(logits), k.get("ld", 72), L.ptr(tg), L.ptr(fr), L.ptr(tl), 3, k.get("T", 7), 5, k.get("V", 65), k.get("blank", 0),  # noqa: E731
                        L.ptr(ws), k.get("n", n), L.ptr(loss), L.stream()]
    for k in (dict(ld=64), dict(T=0), dict(V=0), dict(blank=65), dict(blank=-1), dict(n=n - 1)):
        assert lib.asr_rnnt_fwd(*args(**k)) == -1, k                                   # ASR_EINVAL
    assert lib.asr_rnnt_fwd(L.ptr(logits), 72, L.ptr(tg), L.ptr(fr), L.ptr(tl), 1, 1, 9000, 65, 0, L.ptr(ws), 1 << 40, L.ptr(loss),
                            L.stream()) == L.EUNSUPPORTED                               # two diagonals of 9001 doubles exceed 64 KB of LDS
    dl = torch.empty(3 * 7 * 6 * 72, device="cuda")
    assert lib.asr_rnnt_bwd(L.ptr(logits), 72, L.ptr(tg), L.ptr(fr), L.ptr(tl), 3, 7, 5, 65, 0, L.ptr(ws), None, L.ptr(dl), 64, L.F32,
                            L.stream()) == -1                                          # ldd < V
    assert lib.asr_rnnt_bwd(L.ptr(logits), 72, L.ptr(tg), L.ptr(fr), L.ptr(tl), 3, 7, 5, 65, 0, L.ptr(ws), None, L.ptr(dl), 72, 5,
                            L.stream()) == -1                                          # no such dtype
    e = torch.zeros(2, 3, 12, device="cuda")
    assert lib.asr_rnnt_joint_fwd(L.ptr(e), L.ptr(e), L.ptr(e), 2, 3, 3, 12, L.F32, L.stream()) == L.EUNSUPPORTED      # J % 8
    assert lib.asr_rnnt_joint_fwd(L.ptr(e), L.ptr(e), L.ptr(e), 0, 3, 3, 8, L.F32, L.stream()) == -1
    assert lib.asr_rnnt_joint_bwd(L.ptr(e), L.ptr(e), L.ptr(e), L.ptr(e), None, 0, 1, 1, 40, 8, L.F32, L.stream()) == -1   # U1 > 32 needs the workspace
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the joint
def _joint_inputs(B, T, U1, J, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    e = (torch.randn((B, T, J), generator=g) * 1.5).to(dtype)
    p = (torch.randn((B, U1, J), generator=g) * 1.5).to(dtype)
    dz = torch.randn((B, T, U1, J), generator=g).to(dtype)
    return e, p, dz


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [8, 72, 256])
def test_joint_forward_and_backward_against_the_restatement(J, dtype):
    """Ragged sizes: B 2, T 5, U + 1 = 3, and U + 1 = 37 (more label positions than one LDS piece of the backward holds)."""
    from asr_hip import ops
    bf = dtype == torch.bfloat16
    for U1 in (3, 37):
        e, p, dz = _joint_inputs(2, 5, U1, J, dtype, 7 * J + U1)
        z = ops.rnnt_joint(e.cuda(), p.cuda())
        z64, z32 = R.joint(e, p), R.joint(e, p, torch.float32)
        assert z.dtype == dtype and tuple(z.shape) == (2, 5, U1, J)
        x = R.excess(z.float(), z64, R.bound32(z64, z32), bf16_stored=bf)
        de, dp = ops.rnnt_joint_bwd(dz.cuda(), z)
        torch.cuda.synchronize()
        zc = z.cpu()
        (de64, dp64), (de32, dp32) = R.joint_bwd(dz, zc), R.joint_bwd(dz, zc, torch.float32)
        xe = R.excess(de.float(), de64, R.bound32(de64, de32), bf16_stored=bf)
        xp = R.excess(dp.float(), dp64, R.bound32(dp64, dp32), bf16_stored=bf)
        print("J %d U1 %d %s: z error / bound %.3f, de %.3f, dp %.3f" % (J, U1, dtype, x, xe, xp))
        assert x <= 1.0 and xe <= 1.0 and xp <= 1.0
        again = ops.rnnt_joint_bwd(dz.cuda(), z)
        assert torch.equal(again[0], de) and torch.equal(again[1], dp) and torch.equal(ops.rnnt_joint(e.cuda(), p.cuda()), z)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("U1,J", [(3, 8), (3, 72), (3, 256), (70, 72)])
def test_joint_reductions_are_exact_on_small_integers(U1, J, dtype):
    """z handed in from {0, 1}, dz from {-1, 0, 1}: every product and every partial sum (at most 70 terms) is an integer that fp32 and
    bf16 hold exactly, so the two reductions equal float64 whatever their order.  tanh(0) = 0 exactly: the forward of zeros."""
    from asr_hip import ops
    g = torch.Generator().manual_seed(U1 * 1000 + J)
    B, T = 2, 6
    z = torch.randint(0, 2, (B, T, U1, J), generator=g).to(dtype)
    dz = torch.randint(-1, 2, (B, T, U1, J), generator=g).to(dtype)
    de, dp = ops.rnnt_joint_bwd(dz.cuda(), z.cuda())
    de64, dp64 = R.joint_bwd(dz, z)
    assert torch.equal(de.cpu().double(), de64) and torch.equal(dp.cpu().double(), dp64) and float(de64.abs().max()) > 1
    zero = ops.rnnt_joint(torch.zeros(B, T, J, dtype=dtype, device="cuda"), torch.zeros(B, U1, J, dtype=dtype, device="cuda"))
    assert torch.equal(zero.cpu(), torch.zeros(B, T, U1, J, dtype=dtype))


def test_joint_outputs_between_sentinels():
    from asr_hip import lib as L
    dev = torch.device("cuda")
    B, T, U1, J, G = 2, 5, 37, 72, 64
    e, p, dz = _joint_inputs(B, T, U1, J, torch.bfloat16, 3)
    ed, pd, dzd = e.to(dev), p.to(dev), dz.to(dev)
    z = torch.full((B * T * U1 * J + 2 * G,), -7.0, dtype=torch.bfloat16, device=dev)
    L.call("asr_rnnt_joint_fwd", L.ptr(ed), L.ptr(pd), L.ptr(z[G:]), B, T, U1, J, L.BF16, L.stream())
    n = int(L.load().asr_rnnt_joint_bwd_workspace(B, T, U1, J))
    assert n == B * T * J and L.load().asr_rnnt_joint_bwd_workspace(B, T, 32, J) == 0
    ws = torch.full((n + 2 * G,), -7.0, device=dev)
    de = torch.full((B * T * J + 2 * G,), -7.0, dtype=torch.bfloat16, device=dev)
    dp = torch.full((B * U1 * J + 2 * G,), -7.0, dtype=torch.bfloat16, device=dev)
    L.call("asr_rnnt_joint_bwd", L.ptr(dzd), L.ptr(z[G:]), L.ptr(de[G:]), L.ptr(dp[G:]), L.ptr(ws[G:]), n, B, T, U1, J, L.BF16, L.stream())
    torch.cuda.synchronize()
    for name, buf in (("z", z), ("workspace", ws), ("de", de), ("dp", dp)):
        guard = torch.full((G,), -7.0, dtype=buf.dtype)
        assert torch.equal(buf[:G].cpu(), guard) and torch.equal(buf[-G:].cpu(), guard), name
    from asr_hip import ops
    zz = ops.rnnt_joint(ed, pd)
    want = ops.rnnt_joint_bwd(dzd, zz)
    assert torch.equal(z[G:-G].view(B, T, U1, J), zz) and torch.equal(de[G:-G].view(B, T, J), want[0]) and torch.equal(dp[G:-G].view(B, U1, J), want[1])
