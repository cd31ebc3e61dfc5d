"""tests/decode_reference.py on the CPU: the restatement IS the operation (against torch's own linear / layer_norm /
scaled_dot_product_attention / argmax in float64, and asr_hip.ops.frag_pack / frag_unpack, which are pure torch); the exact cases of
tests/test_gpu_decode_arms.py are exact in an fp32 emulation and not degenerate; the kernel's arithmetic restated in float64
(attend_as_computed) sits inside the attention bound; and every deliberate defect of MUTANTS fails the checker the GPU file uses."""
import math

import pytest
import torch

import decode_reference as R

BF, F32, F64 = R.BF, R.F32, R.F64


# ------------------------------------------------------------------------------------------------ the restatement is the operation
def test_rb_rounds_once_to_nearest_even():
    x = torch.tensor([1.0, 1.00390625, 1.005859375, 1.001953125, -3.1415926, 257.0, 258.0, 0.0, 1e-3, math.inf], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.0078125, 1.0, -3.140625, 256.0, 258.0, 0.0, 0.00099945068359375, math.inf], dtype=F64)
    assert torch.equal(R.rb(x), want)
    g = torch.Generator().manual_seed(0)
    y = torch.randn(4096, generator=g)
    assert torch.equal(R.rb(y.double()), y.to(BF).double())                  # fp32 -> bf16 is one rounding in torch too
    # a float64 just above a bf16 tie that fp32 rounds ONTO the tie: two roundings go down to even, one goes up
    z = torch.tensor([1.00390625 + 2.0 ** -30], dtype=F64)
    assert float(z.to(F32).to(BF)) == 1.0 and float(R.rb(z)) == 1.0078125


def test_gemm_add_ln_attend_finish_against_torch():
    g = torch.Generator().manual_seed(1)
    x, W, b = torch.randn(5, 64, generator=g).double(), torch.randn(33, 64, generator=g).double(), torch.randn(33, generator=g).double()
    assert torch.allclose(R.gemm(x, W, b, True), torch.nn.functional.linear(x, W, b).relu(), rtol=0, atol=1e-13)
    assert torch.allclose(R.gemm(x, W), torch.nn.functional.linear(x, W), rtol=0, atol=1e-13)
    Y, Rr = torch.randn(7, 320, generator=g).to(BF), (2 * torch.randn(7, 320, generator=g)).to(BF)
    gamma, beta = torch.randn(320, generator=g).double(), torch.randn(320, generator=g).double()
    z = (Y.float() + Rr.float()).to(BF).double()
    assert torch.allclose(R.add_ln(Y, Rr, gamma, beta, 1e-5), torch.nn.functional.layer_norm(z, (320,), gamma, beta, 1e-5), rtol=0, atol=1e-12)
    B, H, L = 3, 2, 77
    q, K, V = torch.randn(B, H * 64, generator=g).double(), torch.randn(B, L, H * 64, generator=g).double(), torch.randn(B, L, H * 64, generator=g).double()
    out, A, S = R.attend(q, K, V, 0.125)
    sdpa = torch.nn.functional.scaled_dot_product_attention(q.view(B, H, 1, 64), K.view(B, L, H, 64).transpose(1, 2), V.view(B, L, H, 64).transpose(1, 2), scale=0.125)
    assert torch.allclose(out, sdpa.reshape(B, H * 64), rtol=0, atol=1e-13)
    assert bool((out.abs() <= A + 1e-15).all()) and bool((S >= 0).all()) and S.shape == (B, H)
    assert torch.allclose(R.attend_as_computed(q, K, V, 0.125), out, rtol=0, atol=2.0 ** -7 * float(A.max()))
    lg = torch.randn(9, 300, generator=g)
    tok, done, o = R.finish(lg, 300, 2, 1, 4, torch.zeros(9, dtype=torch.bool), torch.zeros(4, 9, dtype=torch.int64))
    assert torch.equal(tok, lg.argmax(1)) and torch.equal(o[1], tok) and int(o.sum()) == int(tok.sum()) and torch.equal(done, tok == 2)
    pe = torch.randn(6, 5, generator=g)
    assert torch.equal(R.prepare(pe, 3, 4)[0], pe[3]) and R.prepare(pe, 3, 4)[1].tolist() == [4] * 4
    assert torch.equal(R.embed(torch.tensor([1, 0]), pe, pe, 0.5, 2), pe.double()[[1, 0]] * 0.5 + pe.double()[2])


@pytest.mark.parametrize("rows,K", [(1, 16), (31, 64), (32, 2048), (33, 64), (100, 128)])
def test_frag_index_is_the_order_of_ops_frag_pack(rows, K):
    from asr_hip import ops
    w = torch.arange(rows * K, dtype=torch.float32).view(rows, K) + 1
    f = R.pack(w)
    assert torch.equal(f, ops.frag_pack(w)) and torch.equal(R.unpack(f, rows, K), w) and torch.equal(ops.frag_unpack(f, rows, K), w)
    idx = R.frag_index(rows, K)
    assert idx.unique().numel() == rows * K and int(idx.max()) < (rows + 31) // 32 * 32 * K
    # the header's sentence, literally: lane 32 h + i of block (r, s) holds [32 r + i][16 s + 8 h .. + 7] at ((r K/16 + s) 64 + lane) 8
    r, s, h, i = (rows - 1) // 32, K // 16 - 1, 1, (rows - 1) % 32
    assert idx[32 * r + i, 16 * s + 8 * h:16 * s + 8 * h + 8].tolist() == [((r * K // 16 + s) * 64 + 32 * h + i) * 8 + e for e in range(8)]
    assert math.isnan(float(R.pack(w, fill=math.nan)[-1])) == (rows % 32 != 0)


# ------------------------------------------------------------------------------------------------ the exact cases are exact in fp32
def _all_gemm_cases():
    return [c for t in R.GEMM_TABLES.values() for c in t] + R.SHIPPED + R.PRO1_EXACT + R.PRO2_EXACT


def test_gemm_tables_cover_every_value_with_every_symbol():
    for (grp, f32), table in R.GEMM_TABLES.items():
        assert {c["K"] for c in table} == set(R.K_GROUPS[grp]), (grp, f32)
        assert {c["B"] for c in table} == set(R.B_ALL) and {c["bias"] for c in table} == {True, False} == {c["relu"] for c in table}
        assert {c["w"] for c in table} == {"row", "frag"} == {c["x"] for c in table}
        assert {c["N"] for c in table if c["o"] == "row"} == set(R.N_ROW)
        if not f32:
            assert {c["N"] for c in table if c["o"] == "frag"} == set(R.N_FRAG)
        for c in table:
            nw = 8 if c["K"] > 512 and c["K"] % 128 == 0 else 4
            ks = c["K"] // nw // 16
            assert ks == R.K_STEPS[c["K"]] and {"w4s8": nw == 4 and ks <= 8, "w4s16": nw == 4 and 8 < ks <= 16, "w8s16": nw == 8 and ks <= 16}[grp]
    assert len({R.gemm_id(c) for c in _all_gemm_cases()}) == len(_all_gemm_cases())
    assert {(c["K"], c["f32"], c["o"], c["w"]) for c in R.PRO1_EXACT} >= {(K, f, o, w) for K in (64, 128, 320, 512) for f, o in ((True, "row"), (False, "frag"), (False, "row"))
                                                                         for w in ("row", "frag")}
    assert {c["x_out"] for c in R.PRO1_EXACT} == {True, False}


def test_gemm_exact_cases_are_exact_in_fp32_in_any_order_and_not_degenerate():
    for c in _all_gemm_cases():
        d = R.gemm_exact_case(c)
        x, W = d["x"], d["W"]
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= 2 and float(W.abs().max()) <= 2, R.gemm_id(c)
        assert float((x.abs() @ W.abs().t()).max()) + 8 < 2 ** 24
        for perm in (torch.arange(c["K"]), torch.arange(c["K"]).flip(0)):
            acc = torch.zeros(c["B"], c["N"], dtype=F32)
            for k0 in range(0, c["K"], 16):                                    # fp32 accumulation in K steps of 16, forwards and backwards
                kk = perm[k0:k0 + 16]
                acc = acc + x[:, kk].float() @ W[:, kk].float().t()
            if d["bias"] is not None:
                acc = acc + d["bias"].float()
            if c["relu"]:
                acc = acc.relu()
            got = acc if c["f32"] else acc.to(BF)
            assert torch.equal(got.double(), d["want"]), R.gemm_id(c)
        assert float(d["want"].abs().max()) > 0 and (c["N"] * c["B"] < 8 or d["want"].unique().numel() > 2), R.gemm_id(c)
        if c["pro"] == 1:                                                      # gamma = 0: x is beta bit for bit for any finite Y, R
            xx = R.add_ln(d["Y"], d["R"], d["gamma"], d["beta"], 1e-5, dtype=F32)
            assert torch.equal(xx.double(), d["x"])
        if c["pro"] == 2:
            xx = d["table"].float()[d["tok"]] * 0.5 + d["pe"].float()[d["t"]]
            assert torch.equal(xx.double(), d["x"]) and torch.equal(xx.to(BF).double(), d["x"])


def _attn_fp32(c, K=None, V=None):
    """Single-pass fp32 emulation: exp in fp32, probabilities rounded to bf16 before P V, one bf16 rounding at the end."""
    K, V = c["K"] if K is None else K, c["V"] if V is None else V
    B, HD = c["q"].shape
    H = HD // 64
    s = torch.einsum("bhd,bhjd->bhj", c["q"].float().view(B, H, 64), K.float().view(B, -1, H, 64).permute(0, 2, 1, 3)) * c["scale"]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = torch.einsum("bhj,bhjd->bhd", p.to(BF).float(), V.float().view(B, -1, H, 64).permute(0, 2, 1, 3)) / p.sum(-1, keepdim=True)
    return o.reshape(B, HD).to(BF)


def test_attention_exact_cases_are_exact_in_fp32_and_not_degenerate():
    assert float(torch.exp(torch.tensor(-128.0, dtype=F32))) == 0.0
    seen = set()
    for launch in range(4):
        c = R.onehot_case(1025, 33, 8, launch)
        seen |= set(c["js"].reshape(-1).tolist())
        if launch == 0:
            assert R.same_bits(_attn_fp32(c), c["want"])
            rows = c["want"].view(33 * 8, 64)
            assert rows.unique(dim=0).shape[0] == 33 * 8 and float(rows.float().abs().min(1).values.max()) > 0      # pairwise distinct, non-zero
            assert torch.equal(R.attend(c["q"], c["K"], c["V"], c["scale"])[0], c["want"].double())
            assert torch.equal(R.attend_as_computed(c["q"], c["K"], c["V"], c["scale"]), c["want"].double())
    assert seen == set(range(1025))
    for rows in (600, 1025):
        c = R.twohot_case(rows, 5, 8)
        assert bool((c["j1"] // 512 != c["j2"] // 512).all())
        assert R.same_bits(_attn_fp32(c), c["want"]) and float(c["want"].float().abs().max()) > 0
        assert torch.equal(R.attend_as_computed(c["q"], c["K"], c["V"], c["scale"]), c["want"].double())
    for L in (1, 2, 32, 512, 1024):
        c = R.uniform_case(L, 3, 2)
        assert R.same_bits(_attn_fp32(c), c["want"]) and float(c["want"].float().abs().max()) > 0
        assert torch.equal(R.attend_as_computed(c["q"], c["K"], c["V"], c["scale"]), c["want"].double())


def test_fused_exact_cases_are_exact_and_the_cross_arm_has_a_unique_maximum():
    for mode, D, rows, t, H, oh in (("ln", 64, 64, 63, 1, 0), ("ln", 320, 65, 64, 2, "t"), ("embed", 128, 64, 0, 8, "t"), ("embed", 512, 512, 511, 2, 1),
                                   ("cross", 192, 511, None, 8, 0), ("ln", 512, 512, 0, 2, None), ("cross", 64, 1, None, 1, None)):
        d = R.fused_exact_case(mode, D, rows, t, 3, H, seed=D // 64, onehot=oh)
        proj = R.gemm(d["x"], d["W"], d["bias"])
        assert bool((proj == proj.round()).all()) and float((d["x"].abs() @ d["W"].abs().t()).max()) < 2 ** 24
        acc = d["x"].float() @ d["W"].float().t() + (0 if d["bias"] is None else d["bias"].float())
        HD = H * 64
        assert torch.equal(acc.to(BF).double()[:, :HD], d["q"])
        if mode != "cross":
            assert torch.equal(acc.to(BF).double()[:, HD:2 * HD], d["k"]) and torch.equal(acc.to(BF).double()[:, 2 * HD:], d["v"])
            assert float(d["v"].abs().max()) > 0
        if oh is not None:
            assert bool((d["q"] == 4).all())
            got = R.attend_as_computed(d["q"], d["keys"], d["values"], d["scale"])
            assert torch.equal(got, d["want"]) and float(d["want"].abs().max()) > 0
    for D in (64, 512):
        d = R.cross_argmax_case(D, 5, 8)
        top = d["q"].view(5, 8, 64).topk(2, -1).values
        assert bool((top[..., 0] - top[..., 1] >= 1).all())
        got = R.attend_as_computed(d["q"], d["kc"].double(), d["vc"].double(), d["scale"])
        assert torch.equal(got, d["want"].double()) and d["js"].unique().numel() > 4


# ------------------------------------------------------------------------------------------------ the bound has room
@pytest.mark.parametrize("L", [33, 513, 1100])
def test_attend_as_computed_sits_inside_the_attention_bound(L):
    c = R.bounded_case(L, 5, 8)
    mx = R.pass_maxima(c)
    assert bool((mx[..., 1:] > mx[..., :-1]).all()), "the running maximum must rise at every pass boundary"
    ref, bound = R.attn_bound(c["q"], c["K"], c["V"], c["scale"])
    r = R.ratio(R.attend_as_computed(c["q"], c["K"], c["V"], c["scale"]), ref, bound)
    print("DECODE_HOST attend_as_computed L=%d error / bound %.3f" % (L, r))
    assert r <= 1.0


def test_integer_sweep_needs_the_worst_case_rounding_term():
    """Two or three probabilities carry the softmax of the integer sweep: the correct algorithm in float64 passes 2^-8 A per rounding
    and exceeds the 2^-9 A per rounding that random operands are held to (bf16's unit roundoff is 2^-8)."""
    d = R.fused_exact_case("cross", 64, 512, None, 2, 8, seed=9)
    got = R.attend_as_computed(d["q"], d["keys"], d["values"], d["scale"])
    ref, bound = R.attn_bound(d["q"], d["keys"], d["values"], d["scale"])
    ref, worst = R.attn_bound(d["q"], d["keys"], d["values"], d["scale"], worst_case=True)
    print("DECODE_HOST integer sweep error / bound %.3f, error / worst-case bound %.3f" % (R.ratio(got, ref, bound), R.ratio(got, ref, worst)))
    assert R.ratio(got, ref, worst) <= 1.0 < R.ratio(got, ref, bound)


# ------------------------------------------------------------------------------------------------ every mutant fails its checker
def _mut_drop_key_onehot():
    c = R.onehot_case(1100, 5, 8, 0)
    b, h = 3, 5
    got = R.to_bf(R.attend(c["q"], c["K"], c["V"], c["scale"], drop=(b, h, int(c["js"][b, h])))[0])
    return R.same_bits(got, c["want"])


def _mut_drop_key_uniform():
    c = R.uniform_case(1024, 3, 2)
    got = R.to_bf(R.attend(c["q"], c["K"], c["V"], c["scale"], drop=(1, 1, 700))[0])
    return R.same_bits(got, c["want"])


def _mut_stale_cache_row():
    """self attention, one-hot on the appended row t: the cache's row t (NaN before the call) is used instead of k_new / v_new"""
    c = R.onehot_case(33, 2, 2, 0)
    t = 32
    js = torch.full((2, 2), t)
    K = torch.zeros_like(c["K"])
    K[:, t] = 4.0                                       # k_new
    want = c["V"][:, t]
    ok = R.same_bits(R.to_bf(R.attend(c["q"], K, c["V"], c["scale"])[0]), want)
    assert ok and bool((js == t).all())
    stale_K, stale_V = K.clone(), c["V"].clone()
    stale_K[:, t], stale_V[:, t] = math.nan, math.nan
    got = R.attend(c["q"], stale_K, stale_V, c["scale"])[0].to(F32).to(BF)
    return R.same_bits(got, want)


def _mut_no_rescale_onehot():
    c = R.onehot_case(1025, 33, 8, 2)                    # launch 2: j* from 528 on, after a pass of score-0 keys
    assert int(c["js"].min()) >= 512
    return R.same_bits(R.attend_as_computed(c["q"], c["K"], c["V"], c["scale"], rescale=False).to(F32).to(BF), c["want"])


def _mut_no_rescale_bounded():
    c = R.bounded_case(1100, 5, 8)
    ref, bound = R.attn_bound(c["q"], c["K"], c["V"], c["scale"])
    return R.ratio(R.attend_as_computed(c["q"], c["K"], c["V"], c["scale"], rescale=False), ref, bound) <= 1.0


def _gemm_case_frag():
    c = next(c for c in R.GEMM_TABLES[("w4s8", False)] if c["w"] == "frag")
    return c, R.gemm_exact_case(c)


def _mut_swapped_k_halves():
    c, d = _gemm_case_frag()
    K = c["K"]
    swap = torch.arange(K).view(K // 16, 2, 8).flip(1).reshape(K)           # lane >> 5 exchanged: the two 8-column halves of every 16
    got = R.gemm(d["x"], d["W"][:, swap], d["bias"], c["relu"])
    return torch.equal(R.rb(got), d["want"])


def _mut_fragment_off_by_one_block():
    c = next(c for c in R.GEMM_TABLES[("w4s8", False)] if c["o"] == "frag" and c["N"] == 48)
    d = R.gemm_exact_case(c)
    full = torch.zeros(32, c["N"], dtype=F64)
    full[:c["B"]] = d["want"]
    f = R.pack(full)
    assert torch.equal(R.unpack(f, 32, c["N"])[:c["B"]], d["want"])
    return torch.equal(R.unpack(torch.roll(f, 512), 32, c["N"])[:c["B"]], d["want"])


def _mut_tail_column_unwritten():
    c = next(c for c in R.GEMM_TABLES[("w4s16", True)] if c["N"] == 35)
    d = R.gemm_exact_case(c)
    got = d["want"].clone()
    got[:, -1] = 7.0                                     # the sentinel the GPU test fills with
    return torch.equal(got, d["want"])


def _mut_bias_after_relu():
    c = next(c for t in R.GEMM_TABLES.values() for c in t if c["bias"] and c["relu"])
    d = R.gemm_exact_case(c)
    got = R.gemm(d["x"], d["W"], None, True) + d["bias"]
    return torch.equal(got if c["f32"] else R.rb(got), d["want"])


def _mut_highest_index_on_ties():
    lg, eos = R.finish_case(4364, 33, 4)
    done, out = torch.zeros(33, dtype=torch.bool), torch.zeros(3, 33, dtype=torch.int64)
    a, b = R.finish(lg, 4364, eos, 1, 3, done, out), R.finish(lg, 4364, eos, 1, 3, done, out, highest=True)
    return torch.equal(a[0], b[0])


def _mut_z_not_rounded():
    g = torch.Generator().manual_seed(5)
    B, K = 32, 512
    Y, Rr = torch.randn(B, K, generator=g).to(BF), (2 * torch.randn(B, K, generator=g)).to(BF)
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    good = R.add_ln(Y, Rr, gamma, beta, 1e-5, dtype=F32).to(BF)
    assert R.ln_ratio(good, Y, Rr, gamma, beta, 1e-5) <= 1.0
    bad = R.add_ln(Y, Rr, gamma, beta, 1e-5, dtype=F32, round_z=False).to(BF)
    return R.ln_ratio(bad, Y, Rr, gamma, beta, 1e-5) <= 1.0


MUTANTS = [_mut_drop_key_onehot, _mut_drop_key_uniform, _mut_stale_cache_row, _mut_no_rescale_onehot, _mut_no_rescale_bounded, _mut_swapped_k_halves,
           _mut_fragment_off_by_one_block, _mut_tail_column_unwritten, _mut_bias_after_relu, _mut_highest_index_on_ties, _mut_z_not_rounded]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__[5:] for m in MUTANTS])
def test_mutant_fails_its_checker(mutant):
    assert mutant() is False


def test_finish_cases_hold_every_edge():
    lg, eos = R.finish_case(4364, 33, 4)
    tok, done, out = R.finish(lg, 4364, eos, 5, 3, torch.zeros(33, dtype=torch.bool), torch.full((3, 33), -1, dtype=torch.int64))
    assert bool((out == -1).all())                       # t >= max_len: out untouched
    assert tok[0] == 4363 and tok[1] == 255 and tok[11] == 256 and tok[2] == 3 and tok[3] == 8 and tok[4] == 69 and tok[5] == 0 and tok[6] == 2182 and tok[7] == 0
    assert tok[8] == eos and bool(done[8]) and bool(torch.isinf(lg[:, 4364:]).all())
    for V in (1, 5, 255, 256, 257):
        lg, eos = R.finish_case(V, 33, 3)
        tok = R.finish(lg, V, eos, 0, 1, torch.zeros(33, dtype=torch.bool), None)[0]
        assert int(tok.max()) < V and int(tok.min()) >= 0
