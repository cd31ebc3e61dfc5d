"""tests/attn_reference.py on the CPU: the NumPy dropout mask against a scalar loop written from csrc/attention.h, the float64 reference
against autograd of attn_ref, and the sensitivity of the slice bound: every deliberate defect of attn_reference.DEFECTS, applied to the
reference on the data of every case of tests/test_gpu_attention_arms.py, must break the bound that the GPU test uses for that case."""
import numpy as np
import pytest
import torch

import attn_reference as AR
from test_gpu_ops import attn_ref

M32 = 0xFFFFFFFF


def scalar_keep(seed, B, Tq, b, h, q, k, thr):
    """drop_row, drop_row_key, drop_pair_mix / drop_pair_bits and drop_keep of csrc/attention.h, one key at a time in Python integers."""
    row = ((h * B + b) * Tq + q) & M32
    row_key = ((seed & M32) + ((seed >> 32) & M32) * 0x85EBCA6B + row * 0x9E3779B1) & M32
    y = ((row_key + (k >> 1)) * 0xC2B2AE35) & M32
    y ^= y >> 15
    y = (y * 0x27D4EB2F) & M32
    y ^= y >> 13
    return ((y >> 16) if (k & 1) else (y & 0xFFFF)) >= thr


MASK_CASES = [(AR.SEED, 2, 3, 161, 401, 0.1), (0xFEDCBA9876543210, 3, 2, 65, 65, 0.25), (7, 1, 4, 300, 383, 0.1), (AR.SEED ^ 0x5555, 2, 3, 5, 3, 0.5)]


@pytest.mark.parametrize("seed,B,H,Tq,Tk,p", MASK_CASES)
def test_keep_mask_is_the_scalar_loop_of_attention_h(seed, B, H, Tq, Tk, p):
    mask, inv_keep = AR.keep_mask(seed, B, H, Tq, Tk, p)
    thr, _ = AR.drop_threshold(p)
    assert mask.shape == (B, H, Tq, Tk) and thr == int(p * 65536 + 0.5)
    assert inv_keep == float(np.float32(1.0) / (np.float32(1.0) - np.float32(thr / 65536.0)))
    rng = np.random.default_rng(Tq * 1000 + Tk)
    for _ in range(200):
        b, h, q, k = (int(rng.integers(n)) for n in (B, H, Tq, Tk))
        assert bool(mask[b, h, q, k]) == scalar_keep(seed, B, Tq, b, h, q, k, thr), (b, h, q, k)
    # both ends of the key axis, odd and even
    for k in {0, 1, Tk - 2, Tk - 1} & set(range(Tk)):
        assert bool(mask[B - 1, H - 1, Tq - 1, k]) == scalar_keep(seed, B, Tq, B - 1, H - 1, Tq - 1, k, thr)


@pytest.mark.parametrize("seed,B,H,Tq,Tk,p", MASK_CASES[:3])
def test_keep_mask_keep_rate(seed, B, H, Tq, Tk, p):
    mask, _ = AR.keep_mask(seed, B, H, Tq, Tk, p)
    keep = 1.0 - AR.drop_threshold(p)[0] / 65536.0
    sigma = np.sqrt(keep * (1.0 - keep) / mask.size)
    assert abs(mask.mean() - keep) <= 4.0 * sigma, (mask.mean(), keep, sigma)


def test_keep_mask_depends_on_the_row_index_and_the_key_only():
    """Row (b, h, q) of a (B, H, Tq) problem is row (h B + b) Tq + q: the same linear index in another factorisation gives the same bits."""
    seed, Tk, p = AR.SEED, 77, 0.1
    a, _ = AR.keep_mask(seed, 2, 3, 40, Tk, p)               # (B, H, Tq) = (2, 3, 40)
    flat, _ = AR.keep_mask(seed, 1, 1, 240, Tk, p)           # rows 0 .. 239
    for b in range(2):
        for h in range(3):
            r0 = (h * 2 + b) * 40
            assert np.array_equal(a[b, h], flat[0, 0, r0:r0 + 40]), (b, h)
    c, _ = AR.keep_mask(seed, 6, 1, 40, Tk, p)               # h = 0: row = b Tq + q
    assert np.array_equal(c[:, 0].reshape(240, Tk), flat[0, 0])
    assert not np.array_equal(a, AR.keep_mask(seed, 2, 3, 40, Tk, p, swap_bh=True)[0])
    assert np.array_equal(AR.keep_mask(seed, 2, 3, 40, Tk + 10, p)[0][..., :Tk], a)         # a key's bit does not depend on Tk
    assert AR.keep_mask(seed, 2, 3, 40, Tk, 0.0)[0].all() and AR.keep_mask(seed, 2, 3, 40, Tk, 0.0)[1] == 1.0


def test_effective_seed_mixes_the_device_counter():
    class Ops:
        _cfg = {"state": None}
    assert AR.effective_seed(AR.SEED, Ops) == AR.SEED
    Ops._cfg["state"] = torch.tensor([2, 5, 0, 0], dtype=torch.int64)
    assert AR.effective_seed(AR.SEED, Ops) == (AR.SEED + 2 * 0xD1B54A32D192ED03) % (1 << 64)
    Ops._cfg["state"] = torch.tensor([-1, 0, 0, 0], dtype=torch.int64)          # the counter is a uint64 on the device
    assert AR.effective_seed(3, Ops) == (3 + 0xFFFFFFFFFFFFFFFF * 0xD1B54A32D192ED03) % (1 << 64)


@pytest.mark.parametrize("name", ["fwd1_causal_65", "fwd1_fused2_100x129", "fwd2_mask3d_257"])
def test_reference_is_float64_autograd_of_attn_ref_without_dropout(name):
    case = AR.CASE_BY_NAME[name]
    x = AR.make_inputs(case)
    d = case["d"]
    ref = AR.reference(x["q"], x["k"], x["v"], x["do"], AR.H, d, x["key_len"], x["key_pad"], case["causal"], AR.SCALE, None, 1.0)
    ones = np.ones((AR.B, AR.H, case["Tq"], case["Tk"]), dtype=bool)
    ref1 = AR.reference(x["q"], x["k"], x["v"], x["do"], AR.H, d, x["key_len"], x["key_pad"], case["causal"], AR.SCALE, ones, 1.0)
    q, k, v = (x[t].double().clone().requires_grad_() for t in ("q", "k", "v"))
    o, a = attn_ref(q, k, v, AR.H, d, x["key_len"], x["key_pad"], case["causal"], AR.SCALE)
    o.backward(x["do"].double())
    for got in (ref, ref1):
        for t, want in (("o", o.detach()), ("probs", a.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
            assert (got[t] - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max())), (name, t)
    s = (AR._heads(x["q"].double(), AR.H, d) @ AR._heads(x["k"].double(), AR.H, d).transpose(-1, -2)) * AR.SCALE
    live = AR.live_keys(AR.B, case["Tq"], case["Tk"], x["key_len"], x["key_pad"], case["causal"])
    lse = torch.logsumexp(s.masked_fill(~live, float("-inf")), -1)
    assert (ref["lse"] - lse).abs().max() <= 1e-12


def test_reference_contract_of_a_row_without_a_live_key():
    case = AR.CASE_BY_NAME["dead_fwd1_100x128"]
    x = AR.make_inputs(case)
    mask, inv_keep = AR.keep_mask(AR.SEED, AR.B, AR.H, case["Tq"], case["Tk"], case["p"])
    ref = AR.reference(x["q"], x["k"], x["v"], x["do"], AR.H, 64, x["key_len"], None, False, AR.SCALE, mask, inv_keep)
    assert all(torch.isfinite(ref[t]).all() for t in ("o", "probs", "dq", "dk", "dv"))
    assert torch.isposinf(ref["lse"][1]).all() and torch.isfinite(ref["lse"][0]).all()
    for t in ("o", "probs", "dq", "dk", "dv"):
        assert (ref[t][1] == 0).all() and (ref[t][0] != 0).any(), t
    emu = AR.emulation(x["q"], x["k"], x["v"], x["do"], AR.H, 64, x["key_len"], None, False, AR.SCALE, mask, inv_keep)
    assert all(torch.isfinite(emu[t]).all() and (emu[t][1] == 0).all() for t in emu)


def test_slice_errors_blocks_and_dead_slices():
    Hh, d = 3, 4
    ref = torch.randn(2, 130, Hh * d, generator=torch.Generator().manual_seed(3)).double()
    ref[1, 64:128] = 0                                           # entry 1, block 1: a dead slice in every head
    got = ref.clone()
    assert AR.slice_errors(got, ref, Hh, d).shape == (2, Hh, 3) and (AR.slice_errors(got, ref, Hh, d) == 0).all()
    got[0, 129, d:2 * d] *= 1.5                                  # entry 0, head 1, last (2-row) block
    e = AR.slice_errors(got, ref, Hh, d)
    want = float((0.5 * ref[0, 129, d:2 * d]).norm() / ref[0, 128:, d:2 * d].norm())
    assert abs(float(e[0, 1, 2]) - want) < 1e-12 and int((e != 0).sum()) == 1
    got[1, 70, 0] = 1e-30                                        # a dead slice must be exactly zero
    e = AR.slice_errors(got, ref, Hh, d)
    assert torch.isposinf(e[1, 0, 1]) and int(torch.isinf(e).sum()) == 1
    got[0, 0, 0] = float("nan")
    assert torch.isposinf(AR.slice_errors(got, ref, Hh, d)[0, 0, 0])


TENSORS = ("o", "dq", "dk", "dv")


@pytest.mark.parametrize("case", AR.CASES, ids=[c["name"] for c in AR.CASES])
def test_every_defect_breaks_the_bound_of_every_case(case):
    """The bound of the GPU test (3 x the emulation's worst slice error; the fp32 tolerance per slice for fp32) on each case's own data,
    against the reference with one defect: a slice of O, dQ, dK or dV must leave the bound.  A defect that cannot act on a case (a mask
    defect without dropout, the diagonal without a causal mask, the key length under a 3-D mask) is not applied there.  The single-bit
    flip is applied where one bit moves the most (attn_reference.defective_reference); the same flip at an ordinary row (query Tq // 2) is
    recorded per case (flip_seen in attn_reference.CASES): it moves a slice by 2e-6 .. 4e-2 and stays under the bound in eight bf16 cases."""
    x = AR.make_inputs(case)
    mask, inv_keep = AR.keep_mask(AR.SEED, AR.B, AR.H, case["Tq"], case["Tk"], case["p"]) if case["p"] > 0 else (None, 1.0)
    ref = AR.cached_reference(case, x, mask, inv_keep)
    bound = AR.bounds(case, x, mask, inv_keep)
    if case["dtype"] == torch.bfloat16:
        # the emulation's worst slice is bf16 rounding: a few 2^-9, whatever the case
        assert all(1e-3 < bound[t] / AR.BOUND_FACTOR < 4e-3 for t in TENSORS), bound
    applied = 0
    for defect in AR.DEFECTS:
        bad = AR.defective_reference(case, x, mask, inv_keep, defect)
        if bad is None:
            continue
        applied += 1
        worst = {t: float(AR.slice_errors(bad[t], ref[t], AR.H, case["d"]).max()) for t in TENSORS}
        lse_rows = int(AR.lse_mismatch(bad["lse"], ref["lse"]).sum())
        print("%-26s %-28s %s  lse rows %d  bound %s" % (case["name"], defect, " ".join("%s %.2e" % kv for kv in worst.items()), lse_rows,
                                                        " ".join("%.2e" % bound[t] for t in TENSORS)))
        assert any(worst[t] > bound[t] for t in TENSORS), (case["name"], defect, worst, bound)
    assert applied >= (1 if case["p"] == 0 else 4), (case["name"], applied)
    for defect in AR.REPORTED_DEFECTS:
        bad = AR.defective_reference(case, x, mask, inv_keep, defect)
        if bad is not None:
            worst = {t: float(AR.slice_errors(bad[t], ref[t], AR.H, case["d"]).max()) for t in TENSORS}
            seen = any(worst[t] > bound[t] for t in TENSORS)
            print("%-26s %-28s %s  %s" % (case["name"], defect, " ".join("%s %.2e" % kv for kv in worst.items()),
                                          "caught" if seen else "under the bound"))
            assert seen == case["flip_seen"], "the record in attn_reference.CASES is out of date"
