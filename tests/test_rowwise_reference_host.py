"""CPU checks of tests/rowwise_reference.py, the yardstick of tests/test_gpu_rowwise_arms.py (no GPU):
  a. every exact-integer case evaluated in float32 in two summation orders is torch.equal to float64: all intermediates are representable
     in fp32, so any kernel summation order and any FMA contraction give the same bits and torch.equal on the GPU is a fair demand;
  b. every tolerance case's bound rejects each deliberate defect on the case's own data, and admits the honest float32 evaluation;
  c. keep_mask keeps 1 - p of 2**18 indices within 3 sigma;
  d. asr_ln_reduce_multi refuses D % 4 != 0 with the library's argument error (the library loads without a GPU).
`-s` prints the measured bounds and margins recorded in rowwise_reference's docstring."""
import numpy as np
import pytest
import torch

import rowwise_reference as R

F32, F64 = torch.float32, torch.float64


def _mask(M, D, p, **kw):
    return R.keep_mask(R.SEED, M, D, p, **kw) if p > 0 else None


# ------------------------------------------------------------------------------------------------ a. exact cases
LN_SHAPES = sorted({(c["M"], c["D"]) for c in R.LN_EXACT} | {(70, 32), (70, 512)})


@pytest.mark.parametrize("M,D", LN_SHAPES, ids=["M%d-D%d" % s for s in LN_SHAPES])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_layernorm_backward_integer_cases_are_exact_in_fp32(M, D, p):
    x = R.ln_exact_inputs(M, D)
    mask = _mask(M, D, p)
    inv_keep = R.drop_threshold(p)[1]
    assert inv_keep == (2.0 if p else 1.0)
    ref = R.add_ln_bwd_reference(x["dout"], x["z"], x["mean"], x["rstd"], x["gamma"], x["keep"], mask, inv_keep)
    assert float(((x["z"] - x["mean"][:, None]) * x["rstd"][:, None]).abs().max()) <= 4 and float(x["dout"].abs().max()) <= 2
    for t in (x["z"], x["dout"]):
        assert torch.equal(t.to(torch.bfloat16).double(), t)               # the operands are exact in both storage types
    for order in (0, 1):
        got = R.add_ln_bwd_reference(x["dout"], x["z"], x["mean"], x["rstd"], x["gamma"], x["keep"], mask, inv_keep, dt=F32, order=order)
        for name, a, b in zip(("d_res", "d_y", "dgamma", "dbeta"), got, ref):
            assert torch.equal(a.double(), b), (name, order, float((a.double() - b).abs().max()))
    # the accumulated destinations too
    for acc0, s in ((x["dgamma0"], ref[2]), (x["dbeta0"], ref[3])):
        assert torch.equal((acc0.float() + s.float()).double(), acc0 + s)
    assert float(ref[0].abs().max()) > 0 and float(ref[2].abs().max()) > 0


@pytest.mark.parametrize("D", [72, 520])
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_embedding_integer_cases_are_exact_in_fp32(D, p):
    x = R.embed_inputs(D)
    n = R.EMB_B * R.EMB_T
    mask = _mask(n, D, p)
    inv_keep = R.drop_threshold(p)[1]
    ref = R.embed_bwd_reference(x["tok"], x["dout"], x["dtable0"], R.EMB_SCALE, mask, inv_keep, R.EMB_PAD)
    for order in (0, 1):
        got = R.embed_bwd_reference(x["tok"], x["dout"], x["dtable0"], R.EMB_SCALE, mask, inv_keep, R.EMB_PAD, dt=F32, order=order)
        assert torch.equal(got.double(), ref), order
    assert torch.equal(ref[R.EMB_PAD], x["dtable0"][R.EMB_PAD])
    fwd = R.embed_reference(x["tok"], x["table"], x["pe"], R.EMB_SCALE, mask, inv_keep)
    assert torch.equal(R.embed_reference(x["tok"], x["table"], x["pe"], R.EMB_SCALE, mask, inv_keep, dt=F32).double(), fwd)
    assert torch.equal(fwd.to(torch.bfloat16).double(), fwd) and torch.equal(x["dout"].to(torch.bfloat16).double(), x["dout"])
    # the layout reaches every branch of embed_bwd_kernel
    t = x["tok"].reshape(-1)
    assert (t[:256] == 1).all() and int(torch.nonzero(t == 2)[0]) > 1024 and int(torch.nonzero(t == 3)[0]) == n - 1 and n > 2048
    assert (t == R.EMB_PAD).any() and (t[1024:2048] == 1).any() and (t[2048:] == 1).any()


# ------------------------------------------------------------------------------------------------ b. deliberate defects
def _honest(c, e32, name):
    return R.rnd(e32[name], c["dtype"]) if name in R.LN_STORED else e32[name]


@pytest.mark.parametrize("c", R.LN_TOL, ids=[R.ln_tol_id(c) for c in R.LN_TOL])
def test_layernorm_bounds_catch_defects(c):
    v = R.LN_TOL_VARIANTS[0]
    M, D, bf = c["M"], c["D"], c["dtype"] == torch.bfloat16
    x = R.ln_tol_inputs(c)
    mask = _mask(M, D, v["p"])
    inv_keep = R.drop_threshold(v["p"])[1]
    ref, b32 = R.ln_tol_reference(c, v, x, mask, inv_keep)
    print("ROWWISE b32 %-16s %s" % (R.ln_tol_id(c), "  ".join("%s %.1e" % (t, b32[t]) for t in R.LN_TENSORS)))
    assert all(b32[t] > 0 for t in R.LN_TENSORS if not (bf and t == "dbeta"))       # (53 bf16 values add exactly in fp32: bound 0)

    def worst(e, names=R.LN_TENSORS):
        return {t: R.excess(_honest(c, e, t), ref[t], b32[t], bf and t in R.LN_STORED) for t in names}

    for order in (0, 1):
        e = R.ln_tol_eval(c, v, x, mask, inv_keep, dt=F32, order=order)
        assert torch.equal(e["z"], ref["z"])
        w = worst(e)
        assert max(w.values()) <= 1.0, (order, w)
    epc = 8 if bf else 4
    kept_row = int(torch.nonzero(x["keep"])[1])
    defects = {
        "one row left out of dgamma": (dict(drop_row=kept_row), ("dgamma", "dbeta")),
        "mask index built with the wrong D": (dict(mask2=_mask(M, D, v["p"], index_D=D + epc)), ("d_y",)),
        "row_keep ignored": (dict(ignore_row_keep=True), ("out", "d_res")),
        "lanes of the last chunk dropped": (dict(live_cols=torch.arange(D) < D - epc), ("mean", "rstd", "out", "d_res")),
        "post_period off by one": (dict(period=c["period"] - 1), ("out",)),
    }
    for name, (kw, seen_in) in defects.items():
        w = worst(R.ln_tol_eval(c, v, x, mask, inv_keep, **kw), seen_in)
        print("ROWWISE defect %-16s %-36s error / bound: %s" % (R.ln_tol_id(c), name, "  ".join("%s %.1e" % kv for kv in w.items())))
        assert max(w.values()) > 1.0, (name, w)
    # the mask defect on the forward side changes z's zero pattern: the exact comparison of z sees it
    zbad = R.add_ln_z(x["y"], None, _mask(M, D, v["p"], index_D=D + epc), inv_keep, c["dtype"])
    assert not torch.equal(zbad != 0, torch.as_tensor(mask))
    assert torch.equal(R.add_ln_z(x["y"], None, mask, inv_keep, c["dtype"]) != 0, torch.as_tensor(mask))


def test_embedding_comparison_catches_a_skipped_chunk():
    x = R.embed_inputs(72)
    ref = R.embed_bwd_reference(x["tok"], x["dout"], x["dtable0"], R.EMB_SCALE, None, 1.0, R.EMB_PAD)
    bad = R.embed_bwd_reference(x["tok"], x["dout"], x["dtable0"], R.EMB_SCALE, None, 1.0, R.EMB_PAD, skip_second_chunk=True)
    rows = [int(r) for r in torch.nonzero((ref != bad).any(1))[:, 0]]
    print("ROWWISE defect embed_bwd second chunk skipped: table rows that change", rows)
    assert 1 in rows and 4 in rows and R.EMB_PAD not in rows and 3 not in rows


@pytest.mark.parametrize("c", R.CE_CASES, ids=[R.ce_id(c) for c in R.CE_CASES])
def test_cross_entropy_bounds_catch_defects(c):
    x, ref, b = R.ce_case_reference(c)
    sabs = float(ref["loss_rows"].abs().sum())
    print("ROWWISE ce %-28s lse %.1e  loss_rel %.1e  dlogits %.1e" % (R.ce_id(c), b["lse"], b["loss_rel"], b["dlogits"]))
    assert int(ref["argmax"][7]) == 0 and int(ref["argmax"][8]) == 5 and int(ref["argmax"][9]) == 0
    assert min(b.values()) > 0
    # torch's own argmax agrees wherever the maximum is unique
    uniq = (x["logits"] == x["logits"].max(1, keepdim=True).values).sum(1) == 1
    assert torch.equal(ref["argmax"][uniq], x["logits"].argmax(1)[uniq])
    for order in (0, 1):
        e = R.ce_reference(x["logits"], x["gold"], c["smoothing"], R.CE_PAD, R.CE_GRAD_OUT, dt=F32, order=order)
        assert abs(float(e["sums"][0]) - float(ref["sums"][0])) <= b["loss_rel"] * sabs
        assert float((e["dlogits"].double() - ref["dlogits"]).abs().max()) <= b["dlogits"]
        bf = e["dlogits"].to(torch.bfloat16).double()
        assert ((bf - ref["dlogits"]).abs() <= R.BF16_REL * ref["dlogits"].abs() + b["dlogits"]).all()
    if c["smoothing"] > 0:
        bad = R.ce_reference(x["logits"], x["gold"], c["smoothing"], R.CE_PAD, R.CE_GRAD_OUT, classes=c["V"] - 1)
        r_loss = abs(float(bad["sums"][0]) - float(ref["sums"][0])) / (b["loss_rel"] * sabs)
        r_dl = float((bad["dlogits"] - ref["dlogits"]).abs().max()) / b["dlogits"]
        r_bf = float(((bad["dlogits"] - ref["dlogits"]).abs() / (R.BF16_REL * ref["dlogits"].abs() + b["dlogits"])).max())
        print("ROWWISE defect ce %-21s smoothing over V - 1: error / bound  loss %.1e  dlogits %.1e  bf16 dlogits %.1e" % (R.ce_id(c), r_loss, r_dl, r_bf))
        # (the loss sees it in every case; the gradient at V = 35 only: at V = 4364 sum_q moves by eps / V = 2e-5 relative, which is what
        # an lse stored in fp32 costs a row whose |lse| is ~100, and far below a bf16 rounding)
        assert r_loss > 1.0 and (c["V"] > 35 or (r_dl > 1.0 and r_bf > 1.0))
    # one non-zero (or NaN) pad column
    full = torch.zeros(c["M"], (c["V"] + 63) // 64 * 64)
    full[:, :c["V"]] = ref["dlogits"].float()
    assert R.pad_columns_clean(full, c["V"])
    for bad_value in (1e-30, float("nan")):
        f2 = full.clone()
        f2[c["M"] - 1, c["V"]] = bad_value
        assert not R.pad_columns_clean(f2, c["V"])


@pytest.mark.parametrize("n", [1001, 4099])
@pytest.mark.parametrize("scale", [None, 0.37])
def test_adam_bounds_admit_the_honest_fp32_step(n, scale):
    x = R.adam_inputs(n)
    for t, f in zip(R.ADAM_STEPS, x["factors"]):
        g = x["g"] * f
        rp, rm, rv, lr, upd = R.adam_noam_reference(x["p"], g, x["m"], x["v"], t, scale, **R.ADAM)
        hp, hm, hv, hlr = R.adam_noam_f32(x["p"], g, x["m"], x["v"], t, scale, **R.ADAM)
        bd = R.adam_bounds(rp, rm, rv, upd)
        assert ((hp.double() - rp).abs() <= bd["p"]).all() and ((hm.double() - rm).abs() <= bd["m"]).all()
        assert ((hv.double() - rv).abs() <= bd["v"]).all() and abs(hlr - lr) <= 2.0 ** -22 * lr
        # a step count off by one moves the rate outside its bound on both sides of the warm-up knee
        assert abs(R.noam_rate(t + 1.0, *[float(np.float32(R.ADAM[k])) for k in ("factor_ms", "warmup", "min_lr")]) - lr) > 2.0 ** -22 * lr
    assert R.noam_rate(4000.0, 1.0, 4000.0, 0.0) == 4000.0 ** -0.5 and R.noam_rate(1.0, 1.0, 4000.0, 0.0) == 4000.0 ** -1.5


# ------------------------------------------------------------------------------------------------ c. mask statistics
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_mask_keep_rate(p):
    n = 2 ** 18
    for seed in (R.SEED, 1234):
        m = R.keep_mask(seed, 512, 512, p)
        assert abs(float(m.mean()) - (1 - p)) <= 3 * np.sqrt(p * (1 - p) / n), (p, seed, float(m.mean()))
    assert R.keep_mask(R.SEED, 4, 8, 0.0).all()
    assert not np.array_equal(R.keep_mask(1, 64, 64, 0.5), R.keep_mask(2, 64, 64, 0.5))
    assert not np.array_equal(R.keep_mask(1, 64, 64, 0.5), R.keep_mask(1 + (1 << 32), 64, 64, 0.5))        # the high seed word counts
    # the index is row * D + col: a (2, 8) mask is the first 16 entries of the (1, 16) mask
    assert np.array_equal(R.keep_mask(7, 2, 8, 0.5).reshape(-1), R.keep_mask(7, 1, 16, 0.5).reshape(-1))
    assert R.drop_threshold(0.5) == (2 ** 31, 2.0) and R.drop_threshold(0.0) == (0, 1.0)


# ------------------------------------------------------------------------------------------------ d. argument check
def test_ln_reduce_multi_refuses_a_width_that_is_no_multiple_of_four():
    """Four consecutive columns of [dgamma | dbeta] per thread: with D % 4 == 2 the group that straddles column D would write past the end
    of dgamma and never reach dbeta[0 .. 1].  Refused before anything is read or launched (n = 0, null arrays)."""
    from asr_hip import build, lib
    build.build()
    h = lib.load()
    for D in (6, 2, 510, 7):
        rc = h.asr_ln_reduce_multi(None, None, None, None, 0, D, None)
        assert rc == -1 and h.asr_strerror(rc).decode() == "invalid argument", (D, rc)
    with pytest.raises(lib.AsrHipError, match="invalid argument"):
        lib.call("asr_ln_reduce_multi", None, None, None, None, 0, 6, None)
