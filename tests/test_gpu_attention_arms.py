"""Every arm of the attention dispatch (attn_choose_fwd / attn_choose_bwd of csrc/attention.hip over the kernels of attention_generic.hip,
attention_d64_*.hip and attention_pp.hip) against a float64 reference, forward AND backward, under dropout, in the layouts the model uses
(asr_hip/functions.py: column slices of one Q|K|V buffer, of a K|V buffer, of the stacked K|V buffer of the decoder's cross attention),
with the fp32 copy of O, and with a batch entry that has no live key.

The dropout mask is known on the host (tests/attn_reference.py keep_mask restates csrc/attention.h), so the reference drops exactly what the
kernels drop and dQ / dK / dV under dropout are compared with autograd, not with another kernel.  Every case asserts:
  1. the probability dump's zero pattern on live entries is keep_mask (ties the restatement to attn_probs_kernel),
  2. the dump is the reference's dropped probabilities within fp32 round-off,
  3. O, o32, dQ, dK, dV within the slice bound (3 x what bf16 rounding costs an emulated flash kernel on the case's own data, per batch
     entry, head and 64 rows; fp32 cases 2e-5 per slice), and lse within the fp32 tolerance on every row (+inf on both sides for a row
     without a live key),
  4. every output finite where the reference is,
  5. a slice whose reference is zero is exactly zero; gradient columns outside the written slices keep their sentinel.
tests/test_attention_reference_host.py shows on the CPU that this bound catches a lost key, an excluded diagonal, a rotated mask row, a
missing rescale and a swapped (b, h) on the data of every case, and one flipped mask bit where a bit moves the most (at an ordinary row a
single bit stays under the bound in eight cases: flip_seen in attn_reference.CASES).  Measured figures: profiles/attention_arms_error.txt.
"""
import numpy as np
import pytest
import torch

import attn_reference as AR
from test_gpu_ops import tol

pytestmark = pytest.mark.gpu

B, H = AR.B, AR.H
SENTINEL = -768.0            # exact in bf16
TENSORS = ("o", "o32", "dq", "dk", "dv")


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


# ------------------------------------------------------------------------------------------------ layouts
def _sliced(x, width, col0, fill, D, dtype):
    """x (B, T, HD) as columns col0 .. col0 + HD of a fresh (B, T, width) buffer filled with `fill`: (view, buffer)."""
    buf = torch.full((x.shape[0], x.shape[1], width), fill, device=D, dtype=dtype)
    view = buf[:, :, col0:col0 + x.shape[2]]
    view.copy_(x.to(D, dtype))
    return view, buf


def place(case, x, D):
    """(q, k, v) device views in the case's layout, (dq, dk, dv) views of sentinel-filled buffers with the same strides, and the list of
    (name, tensor) gradient columns that no kernel may write.  Input columns outside the slices hold NaN: reading them shows."""
    HD, dtype, lay = H * case["d"], case["dtype"], case["layout"]
    nan = float("nan")
    untouched = []

    def grads_like(buf):
        return torch.full_like(buf, SENTINEL)

    if lay == "qkv":
        assert case["Tq"] == case["Tk"]
        buf = torch.full((B, case["Tq"], 3 * HD), nan, device=D, dtype=dtype)
        g = grads_like(buf)
        ins = [buf[:, :, i * HD:(i + 1) * HD] for i in range(3)]
        for dst, t in zip(ins, ("q", "k", "v")):
            dst.copy_(x[t].to(D, dtype))
        outs = [g[:, :, i * HD:(i + 1) * HD] for i in range(3)]
    elif lay in ("kv", "stack"):
        width, c0 = (2 * HD, 0) if lay == "kv" else (4 * HD, 2 * HD)            # stack: layer 1 of two layers' K | V
        qv = x["q"].to(D, dtype).contiguous()
        buf = torch.full((B, case["Tk"], width), nan, device=D, dtype=dtype)
        buf[:, :, c0:c0 + HD].copy_(x["k"].to(D, dtype))
        buf[:, :, c0 + HD:c0 + 2 * HD].copy_(x["v"].to(D, dtype))
        g = grads_like(buf)
        ins = [qv, buf[:, :, c0:c0 + HD], buf[:, :, c0 + HD:c0 + 2 * HD]]
        outs = [torch.full_like(qv, SENTINEL), g[:, :, c0:c0 + HD], g[:, :, c0 + HD:c0 + 2 * HD]]
        if c0:
            untouched.append(("dK|dV buffer, layer 0", g[:, :, :c0]))
    elif lay == "plain":
        ins = [x[t].to(D, dtype).contiguous() for t in ("q", "k", "v")]
        outs = [torch.full_like(t, SENTINEL) for t in ins]
    elif lay == "padded":
        ins, outs = [], []
        for t in ("q", "k", "v"):
            view, _ = _sliced(x[t], HD + 4, 0, nan, D, dtype)
            gview, gbuf = _sliced(torch.full_like(x[t], SENTINEL), HD + 4, 0, SENTINEL, D, dtype)
            ins.append(view)
            outs.append(gview)
            untouched.append(("d%s row padding" % t, gbuf[:, :, HD:]))
    else:
        raise ValueError(lay)
    return ins, outs, untouched


# ------------------------------------------------------------------------------------------------ running and checking
def masks(case, x, D):
    kl = x["key_len"].to(D) if x["key_len"] is not None else None
    kp = x["key_pad"].to(D) if x["key_pad"] is not None else None
    return kl, kp


def forward(case, ops, x, D, ins):
    kl, kp = masks(case, x, D)
    o32 = torch.full((B, case["Tq"], H * case["d"]), float("nan"), device=D, dtype=torch.float32)
    o, lse, probs = ops.attn_fwd(*ins, H, case["d"], key_len=kl, key_pad=kp, causal=case["causal"], scale=AR.SCALE, p=case["p"], seed=AR.SEED,
                                 want_attn=True, o32=o32)
    return o, lse, probs, o32


def backward(case, ops, x, D, ins, outs, o, lse, o32, delta=None):
    kl, kp = masks(case, x, D)
    do = x["do"].to(D, case["dtype"]).contiguous()
    return ops.attn_bwd(*ins, o, do, lse, H, case["d"], key_len=kl, key_pad=kp, causal=case["causal"], scale=AR.SCALE, p=case["p"],
                        seed=AR.SEED, out=tuple(outs), o32=o32, delta=delta)


def host_side(case, x, seed_eff):
    mask, inv_keep = AR.keep_mask(seed_eff, B, H, case["Tq"], case["Tk"], case["p"]) if case["p"] > 0 else (None, 1.0)
    return mask, inv_keep, AR.cached_reference(case, x, mask, inv_keep)


def check_slices(case, tag, got, ref, bound, names, fails):
    for t in names:
        g = got[t].detach().float().cpu()
        if not torch.isfinite(g).all():
            fails.append("%s %s: non-finite output" % (tag, t))
        e = AR.slice_errors(g, ref["o" if t == "o32" else t], H, case["d"])
        worst = float(e.max())
        print("ATTN_ARMS %-28s %-10s %-4s worst slice %.3e  emulation %.3e  bound %.3e" % (case["name"], tag, t, worst,
                                                                                            bound[t] / AR.BOUND_FACTOR, bound[t]))
        if not worst <= bound[t]:
            b, h, blk = np.unravel_index(int(e.argmax()), e.shape)
            fails.append("%s %s: slice (b %d, h %d, rows %d..) error %.3e > bound %.3e" % (tag, t, b, h, 64 * blk, worst, bound[t]))


def device_fault(e):
    """A RuntimeError that reports the card, not the call: the library's ASR_ELAUNCH (-2) / ASR_ERUNTIME (-4), or torch's HIP error at the
    synchronisation.  A refused argument (ASR_EINVAL, ASR_EUNSUPPORTED) or any other Python error fails the one test."""
    from asr_hip import lib as L
    if isinstance(e, L.AsrHipError):
        return str(e).endswith("(-2)") or str(e).endswith("(-4)")
    return "HIP error" in str(e) or "CUDA error" in str(e)


def run_case(case, ops, tag="arms"):
    D = dev()
    x = AR.make_inputs(case)
    seed_eff = AR.effective_seed(AR.SEED, ops)
    mask, inv_keep, ref = host_side(case, x, seed_eff)
    bound = AR.bounds(case, x, mask, inv_keep)
    try:
        ins, outs, untouched = place(case, x, D)
        o, lse, probs, o32 = forward(case, ops, x, D, ins)
        dq, dk, dv = backward(case, ops, x, D, ins, outs, o, lse, o32)
        torch.cuda.synchronize()
    except RuntimeError as e:     # a launch or runtime error of the card ends the session: nothing more runs on a card that has just faulted
        if not device_fault(e):
            raise
        pytest.exit("%s [%s]: %r" % (case["name"], case["arms"], e), returncode=3)
    fails = []
    Tq, Tk = case["Tq"], case["Tk"]
    # 1. the dump's zero pattern on live entries is keep_mask; outside them it is zero
    dump = probs.view(H, B, Tq, Tk).permute(1, 0, 2, 3).double().cpu()
    live = AR.live_keys(B, Tq, Tk, x["key_len"], x["key_pad"], case["causal"]).expand(B, H, Tq, Tk)
    kept = torch.ones_like(live) if mask is None else torch.from_numpy(mask)
    wrong = ((dump != 0) != kept) & live
    if wrong.any():
        fails.append("dump zero pattern differs from keep_mask at %d of %d live entries (effective seed 0x%016x), first %s"
                     % (int(wrong.sum()), int(live.sum()), seed_eff, tuple(int(i) for i in torch.nonzero(wrong)[0])))
    if (dump[~live] != 0).any():
        fails.append("dump is not zero at %d masked entries" % int((dump[~live] != 0).sum()))
    # 2. the dump is the reference's dropped probabilities within fp32 round-off (tolerances of test_attention_fwd_bwd, fp32)
    perr = float((dump - ref["probs"]).abs().max())
    pbound = 1e-6 + tol(torch.float32, 2) * float(ref["probs"].abs().max())
    print("ATTN_ARMS %-28s %-10s dump max abs err %.3e  bound %.3e" % (case["name"], tag, perr, pbound))
    if not perr <= pbound:
        fails.append("dump: max abs err %.3e > %.3e" % (perr, pbound))
    # 3. / 4. / 5. slices (a zero reference slice must be exactly zero; non-finite values fail), lse on every row
    check_slices(case, tag, dict(o=o, o32=o32, dq=dq, dk=dk, dv=dv), ref, bound, TENSORS, fails)
    lse_c = lse.double().cpu()
    bad = AR.lse_mismatch(lse_c, ref["lse"])
    fin = torch.isfinite(ref["lse"])
    print("ATTN_ARMS %-28s %-10s lse max abs err %.3e  bound %.3e  rows without a live key %d" % (
        case["name"], tag, float((lse_c - ref["lse"])[fin].abs().max()), AR.lse_tolerance(ref["lse"]), int((~fin).sum())))
    if bad.any():
        fails.append("lse differs at %d rows, first %s" % (int(bad.sum()), tuple(int(i) for i in torch.nonzero(bad)[0])))
    for name, t in untouched:
        if not (t.float() == SENTINEL).all():
            fails.append("%s was written" % name)
    assert not fails, "%s [%s]:\n  %s" % (case["name"], case["arms"], "\n  ".join(fails))
    return dict(x=x, ins=ins, o=o, lse=lse, o32=o32, dq=dq, dk=dk, dv=dv, ref=ref, bound=bound, mask=mask, inv_keep=inv_keep)


@pytest.mark.parametrize("case", AR.CASES, ids=[c["name"] for c in AR.CASES])
def test_attention_arm_against_float64(ops, no_step_state, case):
    run_case(case, ops)


# ------------------------------------------------------------------------------------------------ call forms
FORM_CASES = ["fwd1_fused2_256", "fwd1_both_100x257"]          # Tk <= 256: the one-pass backward; Tk > 256: attn_bwd_both


@pytest.mark.parametrize("name", FORM_CASES)
def test_step_state_is_mixed_into_the_seed(ops, no_step_state, name):
    """The device step counter, advanced twice, moves the mask: the restated asr_mix_seed (counter read back) predicts it."""
    ops.step_state(dev())
    ops.step_advance()
    ops.step_advance()
    assert int(ops.step_state()[0].item()) != 0
    assert AR.effective_seed(AR.SEED, ops) != AR.SEED
    run_case(AR.CASE_BY_NAME[name], ops, tag="step")


@pytest.mark.parametrize("name", FORM_CASES)
def test_backward_call_forms(ops, no_step_state, name):
    """delta handed in (float64 rowsum(dO * O) as fp32, the gemm_nn_rowdot form) against delta computed by the kernel; o32 = None against o32
    given (delta from the rounded O: the emulation rounds there too); dQ and dK / dV as two launches (ASR_ATTN_DQ, ASR_ATTN_DKV) against
    the one launch: equal bits where both run the same bodies (Tk = 257), within the bound where the one launch is the one-pass kernel."""
    from asr_hip import lib as L
    case = AR.CASE_BY_NAME[name]
    D, d = dev(), case["d"]
    r = run_case(case, ops, tag="forms")
    x, ins, ref, o, lse, o32 = r["x"], r["ins"], r["ref"], r["o"], r["lse"], r["o32"]
    fails = []

    def fresh():
        return place(case, x, D)[1]

    delta64 = (x["do"].double() * ref["o"]).view(B, case["Tq"], H, d).sum(-1).permute(0, 2, 1)
    delta = delta64.float().contiguous().to(D)
    dq, dk, dv = backward(case, ops, x, D, ins, fresh(), o, lse, o32, delta=delta)
    check_slices(case, "delta=", dict(dq=dq, dk=dk, dv=dv), ref, r["bound"], ("dq", "dk", "dv"), fails)
    dq, dk, dv = backward(case, ops, x, D, ins, fresh(), o, lse, None)
    check_slices(case, "o32=None", dict(dq=dq, dk=dk, dv=dv), ref, AR.bounds(case, x, r["mask"], r["inv_keep"], o32=False), ("dq", "dk", "dv"), fails)

    kl, kp = masks(case, x, D)
    do = x["do"].to(D, case["dtype"]).contiguous()
    q, k, v = ins
    sq, sk, sv = fresh()
    dl = torch.empty((B, H, case["Tq"]), device=D, dtype=torch.float32)
    qs, ks, vs, os_ = (ops._bt_strides(t, H, d) for t in (q, k, v, o))
    for parts in (L.ATTN_DELTA, L.ATTN_DQ, L.ATTN_DKV):
        L.call("asr_attn_bwd", L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(o), L.ptr(o32), L.ptr(do), L.ptr(lse), L.ptr(dl), L.ptr(sq), L.ptr(sk),
               L.ptr(sv), B, H, case["Tq"], case["Tk"], d, qs[0], qs[1], ks[0], ks[1], vs[0], vs[1], os_[0], os_[1], L.ptr(kl), L.ptr(kp),
               0, 0, int(case["causal"]), AR.SCALE, case["p"], AR.SEED, None, parts, L.dt(q), L.stream())
    torch.cuda.synchronize()
    check_slices(case, "two halves", dict(dq=sq, dk=sk, dv=sv), ref, r["bound"], ("dq", "dk", "dv"), fails)
    if case["Tk"] > 256:
        for t, a, b_ in (("dq", sq, r["dq"]), ("dk", sk, r["dk"]), ("dv", sv, r["dv"])):
            if not torch.equal(a, b_):
                fails.append("two launches: %s differs from the one launch in %d elements" % (t, int((a != b_).sum())))
    assert not fails, "%s:\n  %s" % (name, "\n  ".join(fails))
