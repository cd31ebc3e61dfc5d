"""Every arm of the row-wise kernels -- csrc/layernorm.hip, the embedding / optimiser / small kernels of csrc/elementwise.hip, csrc/ce.hip --
against the float64 references of tests/rowwise_reference.py, with the dropout mask known on the host (keep_mask restates csrc/common.h).

LayerNorm backward, exact (integer data, torch.equal): the four chunk-count arms NCH = 1 / 2 / 4 / 8 in both types, the second stage with
  1 / 16 / 64 slices (M = 7 / 509 / 4093), the 32-row atomics path (C entry point, null workspace), and the deferred reduction
  (asr_add_ln_bwd_partials + asr_ln_reduce_multi, 26 layers = two launches).  dgamma / dbeta start from non-zero integers.
LayerNorm forward and ragged widths (D no power of two, no whole chunks): z bit for bit, its zero pattern the mask, mean / rstd / out /
  d_res / d_y / dgamma / dbeta within b32 (+ 2**-8 |ref| for bf16 storage), b32 = 4 x the error of the float32 CPU evaluation.
Embedding: backward exact at 2100 positions (every chunk branch of embed_bwd_kernel), forward exact, zero pattern = keep_mask.
Cross entropy: padded leading dimension (ld 37: rows alternate between the 16-byte and the scalar loop), logits x 30, ties, a row of
  -inf, PAD rows; bf16 gradients; pad columns of the 8- and 64-column forms exactly 0 in a NaN-filled buffer.
Optimiser and small kernels: asr_adam_noam_step with shadow and lr_out across the warm-up knee, asr_grad_coef, asr_length_mask,
  asr_cast_flat / asr_widen_flat with guard elements, ops.ratio.
tests/test_rowwise_reference_host.py shows on the CPU that the integer cases are exact in fp32 in any order and that the bounds catch
deliberate defects.  Every figure is printed before it is asserted (`-s`)."""
import ctypes

import numpy as np
import pytest
import torch

import rowwise_reference as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
DT_ID = {F32: "f32", BF16: "bf16"}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    return o


@pytest.fixture
def no_step_state(ops):
    """The dropout seed is the host seed alone unless a test creates the device step state; whatever it creates is gone afterwards."""
    saved = ops._cfg["state"]
    ops._cfg["state"] = None
    yield
    ops._cfg["state"] = saved


class card:
    """A launch or runtime error of the card ends the session: nothing more runs on a card that has just faulted.  A refused argument
    or any other Python error fails the one test."""

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        return self

    def __exit__(self, et, e, tb):
        if et is None:
            torch.cuda.synchronize()
            return False
        if isinstance(e, RuntimeError):
            from asr_hip import lib as L
            s = str(e)
            if (isinstance(e, L.AsrHipError) and (s.endswith("(-2)") or s.endswith("(-4)"))) or "HIP error" in s or "CUDA error" in s:
                pytest.exit("%s: %r" % (self.what, e), returncode=3)
        return False


def eq(name, got, want, fails):
    """torch.equal of a device tensor with a float64 expectation (both finite)."""
    g = got.detach().double().cpu()
    if g.shape != want.shape or not torch.equal(g, want):
        bad = (g != want) if g.shape == want.shape else None
        fails.append("%s: %s" % (name, "shape %s vs %s" % (tuple(g.shape), tuple(want.shape)) if bad is None else
                                 "%d of %d elements differ, first %s, max |diff| %.3e" % (int(bad.sum()), bad.numel(), tuple(int(i) for i in torch.nonzero(bad)[0]),
                                                                                         float((g - want).abs().max()))))


# ------------------------------------------------------------------------------------------------ LayerNorm backward, exact
_ln_dev = {}


def ln_exact_device(M, D, dtype):
    key = (M, D, dtype)
    if key not in _ln_dev:
        x = R.ln_exact_inputs(M, D)
        _ln_dev.clear()                                  # one shape at a time on the card
        _ln_dev[key] = dict(dout=x["dout"].to(dev(), dtype), z=x["z"].to(dev(), dtype), mean=x["mean"].float().to(dev()),
                            rstd=x["rstd"].float().to(dev()), gamma=x["gamma"].float().to(dev()), keep=x["keep"].to(dev()))
    return _ln_dev[key]


_ln_want = {}


def ln_exact_expected(M, D, dtype, p, seed_eff, rows=None):
    """The float64 backward of rows [r0, r1) of the (M, D) pool, rounded once to the storage type: d_res, d_y, dgamma sum, dbeta sum.
    The mask index counts rows from the start of the call."""
    key = (M, D, dtype, p, seed_eff, rows)
    if key not in _ln_want:
        x = R.ln_exact_inputs(M, D)
        r0, r1 = rows or (0, M)
        mask = R.keep_mask(seed_eff, r1 - r0, D, p) if p > 0 else None
        d_res, d_y, dg, db = R.add_ln_bwd_reference(x["dout"][r0:r1], x["z"][r0:r1], x["mean"][r0:r1], x["rstd"][r0:r1], x["gamma"],
                                                    x["keep"][r0:r1], mask, R.drop_threshold(p)[1])
        if len(_ln_want) > 64:
            _ln_want.clear()
        _ln_want[key] = (R.rnd(d_res, dtype), R.rnd(d_y, dtype), dg, db)
    return _ln_want[key]


@pytest.mark.parametrize("c", R.LN_EXACT, ids=[R.ln_id(c) for c in R.LN_EXACT])
def test_layernorm_backward_exact(ops, no_step_state, c):
    """ops.add_ln_bwd: the 8-rows-per-block first stage and ln_partial_reduce_kernel with 1 / 16 / 64 slices."""
    M, D, dtype, p = c["M"], c["D"], c["dtype"], c["p"]
    x, d = R.ln_exact_inputs(M, D), ln_exact_device(M, D, dtype)
    want = ln_exact_expected(M, D, dtype, p, R.effective_seed(R.SEED, ops))
    dg, db = x["dgamma0"].float().to(dev()), x["dbeta0"].float().to(dev())
    with card(R.ln_id(c)):
        d_res, d_y = ops.add_ln_bwd(d["dout"], d["z"], d["mean"], d["rstd"], d["gamma"], d["keep"], dg, db, p=p, seed=R.SEED)
    assert (d_y is d_res) == (p == 0)
    fails = []
    eq("d_res", d_res, want[0], fails)
    eq("d_y", d_y, want[1], fails)
    eq("dgamma", dg, x["dgamma0"] + want[2], fails)
    eq("dbeta", db, x["dbeta0"] + want[3], fails)
    assert not fails, "%s:\n  %s" % (R.ln_id(c), "\n  ".join(fails))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("D", [32, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_layernorm_backward_exact_atomics_path(ops, no_step_state, dtype, D, p):
    """asr_add_ln_bwd with a null workspace: 32 rows per block, fp32 atomics on dgamma / dbeta (integer sums do not depend on order).
    M = 70: two full blocks and a tail of 6 rows."""
    from asr_hip import lib as L
    M = 70
    x, d = R.ln_exact_inputs(M, D), ln_exact_device(M, D, dtype)
    want = ln_exact_expected(M, D, dtype, p, R.effective_seed(R.SEED, ops))
    dg, db = x["dgamma0"].float().to(dev()), x["dbeta0"].float().to(dev())
    d_res = torch.empty_like(d["z"])
    d_y = torch.empty_like(d["z"]) if p > 0 else None
    with card("atomics path D %d" % D):
        L.call("asr_add_ln_bwd", L.ptr(d["dout"]), L.ptr(d["z"]), L.ptr(d["mean"]), L.ptr(d["rstd"]), L.ptr(d["gamma"]), L.ptr(d["keep"]),
               L.ptr(d_res), L.ptr(d_y), L.ptr(dg), L.ptr(db), None, 0, M, D, float(p), R.SEED, None, L.dt(d["z"]), L.stream())
    fails = []
    eq("d_res", d_res, want[0], fails)
    if p > 0:
        eq("d_y", d_y, want[1], fails)
    eq("dgamma", dg, x["dgamma0"] + want[2], fails)
    eq("dbeta", db, x["dbeta0"] + want[3], fails)
    assert not fails, "\n  ".join(fails)


@pytest.mark.parametrize("D", [32, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_layernorm_backward_exact_deferred_reduction(ops, no_step_state, dtype, D):
    """What graph capture runs: asr_add_ln_bwd_partials per layer, then asr_ln_reduce_multi over all of them.  26 layers (more than
    LN_MULTI = 24: two launches) with 8 i + 3 rows each, every layer another window of the 509-row pool and other prior contents of
    dgamma / dbeta; D = 32 leaves most of a 256-column block idle."""
    from asr_hip import lib as L
    h = L.load()
    M, p, n = 509, 0.5, 26
    x, d = R.ln_exact_inputs(M, D), ln_exact_device(M, D, dtype)
    seed_eff = R.effective_seed(R.SEED, ops)
    layers = []
    with card("deferred reduction D %d" % D):
        for i in range(n):
            rows, r0 = 8 * i + 3, 7 * i
            nws = h.asr_add_ln_bwd_workspace(rows, D)
            lay = dict(rows=rows, r0=r0, ws=torch.full((nws,), float("nan"), device=dev()), d_res=torch.empty((rows, D), device=dev(), dtype=dtype),
                       d_y=torch.empty((rows, D), device=dev(), dtype=dtype), dg=(x["dgamma0"] + i).float().to(dev()),
                       db=(x["dbeta0"] - i).float().to(dev()))
            sl = slice(r0, r0 + rows)
            L.call("asr_add_ln_bwd_partials", L.ptr(d["dout"][sl]), L.ptr(d["z"][sl]), L.ptr(d["mean"][sl]), L.ptr(d["rstd"][sl]),
                   L.ptr(d["gamma"]), L.ptr(d["keep"][sl]), L.ptr(lay["d_res"]), L.ptr(lay["d_y"]), L.ptr(lay["ws"]), nws, rows, D, float(p),
                   R.SEED, None, L.dt(d["z"]), L.stream())
            layers.append(lay)
        P_, I_ = ctypes.c_void_p * n, ctypes.c_int * n
        L.call("asr_ln_reduce_multi", P_(*[l["ws"].data_ptr() for l in layers]), I_(*[l["rows"] for l in layers]),
               P_(*[l["dg"].data_ptr() for l in layers]), P_(*[l["db"].data_ptr() for l in layers]), n, D, L.stream())
    fails = []
    for i, l in enumerate(layers):
        want = ln_exact_expected(M, D, dtype, p, seed_eff, rows=(l["r0"], l["r0"] + l["rows"]))
        eq("layer %d d_res" % i, l["d_res"], want[0], fails)
        eq("layer %d d_y" % i, l["d_y"], want[1], fails)
        eq("layer %d dgamma" % i, l["dg"], x["dgamma0"] + i + want[2], fails)
        eq("layer %d dbeta" % i, l["db"], x["dbeta0"] - i + want[3], fails)
    assert not fails, "\n  ".join(fails[:12])


# ------------------------------------------------------------------------------------------------ LayerNorm, ragged widths, tolerance
def run_ln_tol(ops, c, v, tag):
    M, D, dtype, bf = c["M"], c["D"], c["dtype"], c["dtype"] == BF16
    x = R.ln_tol_inputs(c)
    seed_eff = R.effective_seed(R.SEED, ops)
    mask = R.keep_mask(seed_eff, M, D, v["p"]) if v["p"] > 0 else None
    inv_keep = R.drop_threshold(v["p"])[1]
    ref, b32 = R.ln_tol_reference(c, v, x, mask, inv_keep)
    G = dev()
    yz = x["y"].to(G, dtype)
    keep = x["keep"].to(G) if v["keep"] else None
    gamma = x["gamma"].to(G)
    dg, db = torch.zeros(D, device=G), torch.zeros(D, device=G)
    with card(R.ln_tol_id(c, v)):
        out, mean, rstd = ops.add_ln_fwd(yz, x["res"].to(G, dtype) if v["res"] else None, gamma, x["beta"].to(G),
                                         post_add=x["post"].to(G) if v["post"] else None, row_keep=keep, p=v["p"], seed=R.SEED)
        d_res, d_y = ops.add_ln_bwd(x["dout"].to(G, dtype), yz, mean, rstd, gamma, keep, dg, db, p=v["p"], seed=R.SEED)
    fails = []
    zc = yz.cpu()
    if not v["res"] and v["p"] > 0 and not torch.equal(zc != 0, torch.as_tensor(mask)):
        fails.append("z: zero pattern differs from keep_mask at %d elements (effective seed 0x%016x)" % (int(((zc != 0) != torch.as_tensor(mask)).sum()), seed_eff))
    if not torch.equal(zc, ref["z"]):
        fails.append("z: %d of %d elements differ in their bits" % (int((zc != ref["z"]).sum()), zc.numel()))
    got = dict(mean=mean, rstd=rstd, out=out, d_res=d_res, d_y=d_y, dgamma=dg, dbeta=db)
    for t in R.LN_TENSORS:
        ex = R.excess(got[t], ref[t], b32[t], bf and t in R.LN_STORED)
        print("ROWWISE_ARMS %-8s %-36s %-6s error / bound %.3f  (b32 %.2e)" % (tag, R.ln_tol_id(c, v), t, ex, b32[t]))
        if not ex <= 1.0:
            fails.append("%s: error / bound %.3f (b32 %.2e)" % (t, ex, b32[t]))
    if v["keep"]:
        dead = x["keep"] == 0
        if not (out.float().cpu()[dead] == 0).all() or not (d_res.float().cpu()[dead] == 0).all():
            fails.append("a row dropped by row_keep is not exactly zero in out / d_res")
    assert not fails, "%s:\n  %s" % (R.ln_tol_id(c, v), "\n  ".join(fails))


LN_TOL_PARAMS = [(c, v) for c in R.LN_TOL for v in R.LN_TOL_VARIANTS]


@pytest.mark.parametrize("c,v", LN_TOL_PARAMS, ids=[R.ln_tol_id(c, v) for c, v in LN_TOL_PARAMS])
def test_layernorm_ragged_width_against_float64(ops, no_step_state, c, v):
    run_ln_tol(ops, c, v, "arms")


def test_layernorm_step_state_is_mixed_into_the_seed(ops, no_step_state):
    """The device step counter, advanced twice, moves the mask: the restated asr_mix_seed (counter read back) predicts it."""
    ops.step_state(dev())
    ops.step_advance()
    ops.step_advance()
    assert int(ops.step_state()[0].item()) != 0 and R.effective_seed(R.SEED, ops) != R.SEED
    run_ln_tol(ops, R.LN_TOL[4], R.LN_TOL_VARIANTS[2], "step")


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("c", R.EMBED_CASES, ids=[R.embed_id(c) for c in R.EMBED_CASES])
def test_embedding_exact(ops, no_step_state, c):
    """2100 positions: a full `list` (256 hits in one sub-chunk), an owner beyond position 1024, hits in the owner's second and third
    1024-position chunk, a token at the last position only, PAD positions; dtable starts from non-zero integers and its PAD row stays."""
    D, dtype, p = c["D"], c["dtype"], c["p"]
    x = R.embed_inputs(D)
    n = R.EMB_B * R.EMB_T
    seed_eff = R.effective_seed(R.SEED, ops)
    mask = R.keep_mask(seed_eff, n, D, p) if p > 0 else None
    inv_keep = R.drop_threshold(p)[1]
    G = dev()
    tok = x["tok"].to(G)
    dtab = x["dtable0"].float().to(G)
    with card(R.embed_id(c)):
        ops.embed_bwd(tok, x["dout"].to(G, dtype), dtab, R.EMB_SCALE, p, R.SEED, R.EMB_PAD)
        out = ops.embed_fwd(tok, x["table"].float().to(G), x["pe"].float().to(G), R.EMB_SCALE, p, R.SEED, dtype)
        ones = ops.embed_fwd(tok, torch.ones(R.EMB_V, D, device=G), torch.ones(R.EMB_T, D, device=G), R.EMB_SCALE, p, R.SEED, dtype)
    fails = []
    eq("dtable", dtab, R.embed_bwd_reference(x["tok"], x["dout"], x["dtable0"], R.EMB_SCALE, mask, inv_keep, R.EMB_PAD), fails)
    eq("embed_fwd", out, R.embed_reference(x["tok"], x["table"], x["pe"], R.EMB_SCALE, mask, inv_keep), fails)
    kept = torch.ones(n, D, dtype=torch.bool) if mask is None else torch.as_tensor(mask)
    if not torch.equal((ones != 0).cpu().view(n, D), kept):
        fails.append("embed_fwd: zero pattern differs from keep_mask (effective seed 0x%016x)" % seed_eff)
    eq("embed_fwd, table of ones", ones, torch.full((R.EMB_B, R.EMB_T, D), 1.5, dtype=torch.float64) * kept.view(R.EMB_B, R.EMB_T, D) * inv_keep, fails)
    assert not fails, "%s:\n  %s" % (R.embed_id(c), "\n  ".join(fails))


# ------------------------------------------------------------------------------------------------ cross entropy
def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("c", R.CE_CASES, ids=[R.ce_id(c) for c in R.CE_CASES])
def test_cross_entropy_against_float64(ops, c):
    from asr_hip import lib as L
    M, V, ld, eps = c["M"], c["V"], c["ld"], c["smoothing"]
    x, ref, b = R.ce_case_reference(c)
    G = dev()
    buf = torch.full((M, ld), float("nan"), device=G)
    logits = buf[:, :V]
    logits.copy_(x["logits"].to(G))
    gold = x["gold"].to(G)
    gout = torch.tensor([R.CE_GRAD_OUT], device=G)
    rows = ref["finite"]                               # (the all -inf row has no lse; it is a PAD row and nothing reads it)
    full = {}
    with card(R.ce_id(c)):
        lse, am, sums = ops.ce_fwd(logits, gold, eps, R.CE_PAD)
        lse_d, am_d, sums_d, loss_d = ops.ce_fwd_det(logits, gold, eps, R.CE_PAD)
        dl32 = ops.ce_bwd(logits, gold, lse, eps, R.CE_PAD, gout, sums[1:2])
        dl16 = ops.ce_bwd(logits, gold, lse, eps, R.CE_PAD, gout, sums[1:2], out_dtype=BF16)
        for pad in (8, 64):
            for dtype in DTYPES:
                ldd = (V + pad - 1) // pad * pad
                f = torch.full((M, ldd), float("nan"), device=G, dtype=dtype)
                L.call("asr_ce_bwd", L.ptr(logits), logits.stride(0), L.ptr(gold), L.ptr(lse), M, V, float(eps), R.CE_PAD, L.ptr(gout),
                       L.ptr(sums[1:2]), L.ptr(f), ldd, L.dt(f), L.stream())
                full[(pad, dtype)] = f
    fails = []
    s, sd = sums.cpu().double(), sums_d.cpu().double()
    if (float(s[1]), float(s[2])) != (ref["sums"][1], ref["sums"][2]) or (float(sd[1]), float(sd[2])) != (ref["sums"][1], ref["sums"][2]):
        fails.append("counts: %s / %s, reference %s" % (s[1:].tolist(), sd[1:].tolist(), ref["sums"][1:]))
    if not torch.equal(am.cpu(), ref["argmax"]):
        fails.append("argmax differs at rows %s" % torch.nonzero(am.cpu() != ref["argmax"])[:8, 0].tolist())
    if not (torch.equal(_bits(lse_d), _bits(lse)) and torch.equal(am_d, am)):
        fails.append("ce_fwd_det: lse / argmax bits differ from ce_fwd")
    e_lse = float((lse.cpu().double() - ref["lse"])[rows].abs().max())
    sabs = float(ref["loss_rows"].abs().sum())
    e_loss = [abs(float(t[0]) - float(ref["sums"][0])) / sabs for t in (s, sd)]
    e_dl = float((dl32.cpu().double() - ref["dlogits"]).abs().max())
    r16 = float(((dl16.float().cpu().double() - ref["dlogits"]).abs() / (R.BF16_REL * ref["dlogits"].abs() + b["dlogits"])).max())
    print("ROWWISE_ARMS ce %-26s lse %.2e (bound %.2e)  loss rel %.2e / %.2e (bound %.2e)  dlogits %.2e (bound %.2e)  bf16 dlogits error / bound %.3f"
          % (R.ce_id(c), e_lse, b["lse"], e_loss[0], e_loss[1], b["loss_rel"], e_dl, b["dlogits"], r16))
    if not e_lse <= b["lse"]:
        fails.append("lse: %.3e > %.3e" % (e_lse, b["lse"]))
    if not max(e_loss) <= b["loss_rel"]:
        fails.append("loss sum: relative %.3e / %.3e > %.3e" % (e_loss[0], e_loss[1], b["loss_rel"]))
    if not abs(float(loss_d) - float(ref["sums"][0]) / ref["sums"][1]) <= b["loss_rel"] * sabs / ref["sums"][1] + 2.0 ** -23 * abs(float(loss_d)):
        fails.append("ce_fwd_det loss %.8g, reference %.8g" % (float(loss_d), float(ref["sums"][0]) / ref["sums"][1]))
    if not (torch.isfinite(dl32).all() and e_dl <= b["dlogits"]):
        fails.append("dlogits: %.3e > %.3e" % (e_dl, b["dlogits"]))
    if not (torch.isfinite(dl16.float()).all() and r16 <= 1.0):
        fails.append("bf16 dlogits: error / bound %.3f" % r16)
    for (pad, dtype), f in full.items():
        if not R.pad_columns_clean(f, V):
            fails.append("pad %d %s: a NaN survived or a pad column is not 0" % (pad, DT_ID[dtype]))
        if not torch.equal(f[:, :V], dl32 if dtype == F32 else dl16):
            fails.append("pad %d %s: values differ from the 8-column form's" % (pad, DT_ID[dtype]))
        if not (f[(~ref["live"]).to(G)] == 0).all():
            fails.append("pad %d %s: a PAD row is not 0" % (pad, DT_ID[dtype]))
    assert tuple(ops.ce_bwd(logits, gold, lse, eps, R.CE_PAD, gout, sums[1:2], out_dtype=BF16, pad=64).shape) == (M, (V + 63) // 64 * 64)
    assert not fails, "%s:\n  %s" % (R.ce_id(c), "\n  ".join(fails))


# ------------------------------------------------------------------------------------------------ optimiser and small kernels
@pytest.mark.parametrize("scale", [None, 0.37], ids=["noscale", "scale"])
@pytest.mark.parametrize("n", [1001, 4099])
def test_adam_noam_step_against_float64(ops, no_step_state, n, scale):
    """Three steps at t = 1, 4000, 4001 (both sides of the warm-up knee), each compared with one float64 step from the kernel's own
    previous state; the bf16 shadow is the new p rounded, scalar tail included; lr_out is the Noam rate."""
    G = dev()
    x = R.adam_inputs(n)
    p, m, v = (x[k].clone().to(G) for k in ("p", "m", "v"))
    shadow = torch.full((n + 8,), -3.0, device=G, dtype=BF16)
    lr_out = torch.zeros(1, device=G)
    gs = None if scale is None else torch.tensor([scale], device=G)
    st = ops.step_state(G)
    fails = []
    for t, f in zip(R.ADAM_STEPS, x["factors"]):
        g = x["g"] * f
        st[1] = t
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
        with card("adam n %d t %d" % (n, t)):
            ops.adam_noam_step(p, g.to(G), m, v, grad_scale=gs, lr_out=lr_out, shadow=shadow[:n], **R.ADAM)
        assert int(st[1].item()) == t and int(st[2].item()) == 0
        rp, rm, rv, lr, upd = R.adam_noam_reference(p0, g, m0, v0, t, scale, **R.ADAM)
        bd = R.adam_bounds(rp, rm, rv, upd)
        ex = {k: float(((got.cpu().double() - ref).abs() / bd[k]).max()) for k, got, ref in (("p", p, rp), ("m", m, rm), ("v", v, rv))}
        e_lr = abs(float(lr_out) - lr) / lr
        print("ROWWISE_ARMS adam n %d t %d scale %s: error / bound p %.3f m %.3f v %.3f  lr %.6e rel err %.2e (bound %.2e)"
              % (n, t, scale, ex["p"], ex["m"], ex["v"], float(lr_out), e_lr, 2.0 ** -22))
        for k in ("p", "m", "v"):
            if not ex[k] <= 1.0:
                fails.append("t %d %s: error / bound %.3f" % (t, k, ex[k]))
        if not e_lr <= 2.0 ** -22:
            fails.append("t %d lr_out %.8e, reference %.8e" % (t, float(lr_out), lr))
        if not torch.equal(shadow[:n], p.to(BF16)):
            fails.append("t %d shadow differs from p.to(bfloat16) in %d elements (tail equal: %s)" % (
                t, int((shadow[:n] != p.to(BF16)).sum()), bool(shadow[n - 1] == p[n - 1].to(BF16))))
        if not (shadow[n:].float() == -3.0).all():
            fails.append("t %d shadow written behind n" % t)
    # the floor of the rate
    st[1] = 1
    ops.adam_noam_step(p, (x["g"]).to(G), m, v, lr_out=lr_out, **dict(R.ADAM, min_lr=1e-3))
    torch.cuda.synchronize()
    if float(lr_out) != float(np.float32(1e-3)):
        fails.append("min_lr floor: lr_out %.8e" % float(lr_out))
    assert not fails, "\n  ".join(fails)


@pytest.mark.parametrize("sumsq,max_norm,denom", [(1234.5, 0.5, 37.0), (1234.5, 0.5, 0.25), (1e-4, 400.0, 3.0), (9e6, 400.0, 1600.0),
                                                  (None, 400.0, 12.0), (1234.5, 0.5, None)])
def test_grad_coef(ops, sumsq, max_norm, denom):
    """asr_grad_coef = s * min(1, max_norm / (||g|| s + 1e-6)) with s = 1 / max(denom, 1); denom < 1 counts 1; no sumsq: s alone."""
    G = dev()
    ss = None if sumsq is None else torch.tensor([sumsq], device=G)
    dn = None if denom is None else torch.tensor([denom], device=G)
    coef = torch.zeros(1, device=G)
    ops.grad_coef(ss, max_norm, dn, coef)
    torch.cuda.synchronize()
    s = 1.0 / max(float(np.float32(denom)), 1.0) if denom is not None else 1.0
    want = s if sumsq is None else s * min(1.0, float(np.float32(max_norm)) / (np.sqrt(float(np.float32(sumsq))) * s + float(np.float32(1e-6))))
    print("ROWWISE_ARMS grad_coef %s: %.8e, reference %.8e" % ((sumsq, max_norm, denom), float(coef), want))
    assert abs(float(coef) - want) <= 2.0 ** -22 * want


def test_length_mask_and_ratio(ops):
    G = dev()
    B, T = 3, 300
    lengths = torch.tensor([0, 257, 300], dtype=torch.int32)
    got = ops.length_mask(lengths.to(G), T)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu().view(B, T), (torch.arange(T)[None, :] < lengths[:, None]).to(torch.uint8))
    for num, den in ((7.25, 3.0), (1.0, 4364.0), (0.0, 5.0)):
        r = ops.ratio(torch.tensor([num], device=G), torch.tensor([den], device=G))
        want = float(np.float32(num)) / float(np.float32(den))
        assert abs(float(r) - want) <= 2.0 ** -23 * abs(want), (num, den, float(r))


@pytest.mark.parametrize("n", [1, 1023, 4098])
def test_cast_flat_and_widen_flat(ops, n):
    """Bit for bit torch's cast, 16-byte body and scalar tail; the elements behind n keep their sentinel."""
    G = dev()
    g = torch.Generator().manual_seed(n)
    src = (torch.randn(n + 8, generator=g) * 3).to(G)
    for dtype in DTYPES:
        dst = torch.full((n + 8,), -7.0, device=G, dtype=dtype)
        ops.cast_flat(src[:n], dst[:n])
        assert torch.equal(dst[:n], src[:n].to(dtype)) and (dst[n:].float() == -7.0).all(), (n, dtype)
    sb = src.to(BF16)
    wide = torch.full((n + 8,), -7.0, device=G)
    ops.widen_flat(sb[:n], wide[:n])
    assert torch.equal(wide[:n], sb[:n].float()) and (wide[n:] == -7.0).all(), n
