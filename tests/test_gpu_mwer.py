"""The two kernels of MWER training (csrc/mwer.hip) against the float64 restatement tests/mwer_reference.py.

asr_seq_logprob_bwd: V in {1, 3 with ld = 3 (misaligned rows), 257, 4364} x M in {1, 9, 37} x R in {1, 5 with an empty segment} x fp32 /
bf16 output, ldd = V rounded up to 64, grad_out NULL and given.  asr_mwer_loss: B in {1, 3}, n_b in {0, 1, 2, 16} mixed within a batch.
Bound (the project's rule for row-wise kernels, computed here per tensor from the case's own data): 4 x the largest error of torch's own
fp32 evaluation on the same input against float64, with a floor of one fp32 rounding of the largest entry; plus one bf16 rounding
elementwise for a bf16 output.  Everything the issue calls exact is torch.equal."""
import numpy as np
import pytest
import torch

import mwer_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _bwd(c, out_dtype, grad_out=None, rows=None, pad=64, coef=None):
    """asr_seq_logprob_bwd on a view of the case's wide buffer -> the WHOLE (M, ldd) output on the device."""
    from asr_hip import ops
    dev = torch.device("cuda")
    wide = torch.as_tensor(c["buf"]).to(dev)
    go = None if grad_out is None else torch.tensor([grad_out], dtype=torch.float32, device=dev)
    full = ops.seq_logprob_bwd(wide[:, :c["V"]], torch.as_tensor(c["tgt"]).to(dev), torch.as_tensor(c["seg_off"]).to(dev),
                               torch.as_tensor(c["coef"] if coef is None else coef).to(dev), grad_out=go, out_dtype=out_dtype, pad=pad)
    torch.cuda.synchronize()
    return full


@pytest.mark.parametrize("grad_out", [None, 0.37])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R_", [1, 5])
@pytest.mark.parametrize("M", [1, 9, 37])
@pytest.mark.parametrize("V", [1, 3, 257, 4364])
def test_seq_logprob_bwd_against_the_float64_restatement(V, M, R_, out_dtype, grad_out):
    c = R.bwd_case(V, M, R_)
    logits = c["buf"][:, :V]
    ref = R.dlogits(logits, c["tgt"], c["seg_off"], c["coef"], grad_out)
    t32 = R.dlogits(logits, c["tgt"], c["seg_off"], c["coef"], grad_out, dtype=torch.float32)
    b32 = R.bound32(ref, t32)
    full = _bwd(c, out_dtype, grad_out)
    ldd = (V + 63) // 64 * 64
    assert full.dtype == out_dtype and tuple(full.shape) == (M, ldd)
    assert torch.equal(full[:, V:].float().cpu(), torch.zeros(M, ldd - V)), "pad columns"
    x = R.excess(full[:, :V].float(), ref, b32, bf16_stored=out_dtype == torch.bfloat16)
    print("V %d M %d R %d %s grad_out %s: worst error / bound %.3f (fp32 bound %.3e)" % (V, M, R_, out_dtype, grad_out, x, b32))
    assert x <= 1.0, x
    if V == 1:
        assert torch.equal(full.float().cpu(), torch.zeros(M, ldd))              # softmax of one logit is 1: [v == t] - 1 = 0


def test_rows_without_gradient_are_zero_and_their_logits_are_not_read():
    """A segment with coefficient 0: its rows are all zeros although their logits are NaN (so they were not read); a target outside
    [0, V): zeros; rows behind the last segment: zeros; every other row keeps the plain run's bits."""
    c = dict(R.bwd_case(257, 37, 5))
    off = c["seg_off"].tolist()
    seg = max(range(5), key=lambda r: off[r + 1] - off[r])
    plain = _bwd(c, torch.float32).cpu()
    coef = c["coef"].copy()
    coef[seg] = 0.0
    buf = c["buf"].copy()
    buf[off[seg]:off[seg + 1]] = np.nan
    got = _bwd(dict(c, buf=buf), torch.float32, coef=coef).cpu()
    keep = torch.ones(37, dtype=torch.bool)
    keep[off[seg]:off[seg + 1]] = False
    assert off[seg + 1] > off[seg] and torch.equal(got[~keep], torch.zeros_like(got[~keep])) and torch.equal(got[keep], plain[keep])
    for bad in (257, -1, 2 ** 40):
        tgt = c["tgt"].copy()
        tgt[5] = bad
        got = _bwd(dict(c, tgt=tgt), torch.bfloat16).float().cpu()
        assert torch.equal(got[5], torch.zeros(320)) and float(got[4].abs().max()) > 0
    short = c["seg_off"].copy()
    short[-1] = 30                                # rows 30 .. 36 belong to no segment
    short = np.minimum(short, 30).astype(np.int32)
    got = _bwd(dict(c, seg_off=short), torch.float32).cpu()
    assert torch.equal(got[30:], torch.zeros(7, 320)) and torch.equal(got[:30], plain[:30])


@pytest.mark.parametrize("V,ld", [(40, 40), (4364, 4416), (3, 3)])
def test_all_the_mass_on_the_target_gives_exactly_zero(V, ld):
    """A row whose only finite logit is the target: softmax is exactly the indicator, every element exactly 0 in both output types."""
    M = 11
    g = np.random.default_rng(V)
    tgt = g.integers(0, V, size=M).astype(np.int64)
    buf = np.full((M, ld), -np.inf, dtype=np.float32)
    buf[np.arange(M), tgt] = g.standard_normal(M).astype(np.float32) * 5
    c = dict(buf=buf, V=V, tgt=tgt, seg_off=np.asarray([0, 4, 11], dtype=np.int32), coef=np.asarray([0.8, -1.3], dtype=np.float32))
    for dt in (torch.float32, torch.bfloat16):
        got = _bwd(c, dt).float().cpu()
        assert torch.equal(got, torch.zeros_like(got))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nothing_outside_the_output_is_written(out_dtype):
    """The output inside a buffer of sentinels (a row stride wider than ldd, rows in front and behind): the sentinels stay untouched,
    and the inside equals the plain run."""
    from asr_hip import lib as L
    dev = torch.device("cuda")
    c = R.bwd_case(257, 9, 5)
    V, M, ldd, wide_ld = 257, 9, 320, 384
    plain = _bwd(c, out_dtype)
    box = torch.full((M + 2, wide_ld), SENTINEL, dtype=out_dtype, device=dev)
    logits = torch.as_tensor(c["buf"]).to(dev)
    tgt, off, coef = (torch.as_tensor(c[k]).to(dev) for k in ("tgt", "seg_off", "coef"))
    # (the kernel zero-fills a row up to ldd, so a row stride wider than the written width is one call per row, each into the box's row)
    host_off = c["seg_off"].tolist()
    for m in range(M):
        r = max(i for i in range(5) if host_off[i] <= m)
        one_off = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        L.call("asr_seq_logprob_bwd", L.ptr(logits[m:m + 1]), c["ld"], L.ptr(tgt[m:m + 1]), L.ptr(one_off), L.ptr(coef[r:r + 1]), None,
               1, 1, V, L.ptr(box[m + 1:m + 2]), ldd, L.dt(box), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(box[1:M + 1, :ldd], plain)
    assert bool((box[0] == SENTINEL).all()) and bool((box[M + 1] == SENTINEL).all()) and bool((box[1:M + 1, ldd:] == SENTINEL).all())
    # and a whole (M, ldd) output allocated inside a flat sentinel buffer
    flat = torch.full((64 + M * ldd + 64,), SENTINEL, dtype=out_dtype, device=dev)
    L.call("asr_seq_logprob_bwd", L.ptr(logits), c["ld"], L.ptr(tgt), L.ptr(off), L.ptr(coef), None, 5, M, V, L.ptr(flat[64:]), ldd,
           L.dt(flat), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(flat[64:64 + M * ldd].view(M, ldd), plain)
    assert bool((flat[:64] == SENTINEL).all()) and bool((flat[64 + M * ldd:] == SENTINEL).all())


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [257, 4364])
def test_a_row_gives_the_same_bits_through_an_aligned_and_a_misaligned_base(V, out_dtype):
    """The same logits at a 16-byte aligned base and 4 bytes behind one (the scalar load arm), the same output row at an aligned base
    and one element behind one (the scalar store arm): four runs, one set of bits."""
    from asr_hip import lib as L
    dev = torch.device("cuda")
    c = R.bwd_case(V, 9, 1)
    ldd = (V + 63) // 64 * 64
    row = torch.as_tensor(c["buf"][4, :V].copy()).to(dev)
    tgt = torch.as_tensor(c["tgt"][4:5]).to(dev)
    off = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    coef = torch.tensor([0.61], dtype=torch.float32, device=dev)
    outs = []
    for shift_in in (0, 1):
        src = torch.zeros(V + 8, dtype=torch.float32, device=dev)
        src[shift_in:shift_in + V].copy_(row)
        for shift_out in (0, 1):
            dst = torch.full((ldd + 8,), SENTINEL, dtype=out_dtype, device=dev)
            L.call("asr_seq_logprob_bwd", L.ptr(src[shift_in:]), V, L.ptr(tgt), L.ptr(off), L.ptr(coef), None, 1, 1, V,
                   L.ptr(dst[shift_out:]), ldd, L.dt(dst), L.stream())
            torch.cuda.synchronize()
            assert bool((dst[:shift_out] == SENTINEL).all()) and bool((dst[shift_out + ldd:] == SENTINEL).all())
            outs.append(dst[shift_out:shift_out + ldd].clone())
    assert float(outs[0].float().abs().max()) > 0
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_argument_checks():
    from asr_hip import lib as L
    from asr_hip import ops
    dev = torch.device("cuda")
    lg = torch.zeros(4, 8, device=dev)
    tgt = torch.zeros(4, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    coef = torch.ones(1, device=dev)
    out = torch.zeros(4, 64, device=dev)
    for ld, ldd, R_, M, V in ((4, 64, 1, 4, 8), (8, 4, 1, 4, 8), (8, 64, -1, 4, 8), (8, 64, 1, -1, 8), (8, 64, 1, 4, 0)):
        with pytest.raises(L.AsrHipError):
            L.call("asr_seq_logprob_bwd", L.ptr(lg), ld, L.ptr(tgt), L.ptr(off), L.ptr(coef), None, R_, M, V, L.ptr(out), ldd, L.F32, L.stream())
    with pytest.raises(L.AsrHipError):
        L.call("asr_seq_logprob_bwd", L.ptr(lg), 8, L.ptr(tgt), L.ptr(off), L.ptr(coef), None, 1, 4, 8, L.ptr(out), 64, 7, L.stream())
    with pytest.raises(AssertionError):
        ops.seq_logprob_bwd(lg, tgt.int(), off, coef)
    empty = ops.seq_logprob_bwd(lg[:0], tgt[:0], torch.tensor([0, 0], dtype=torch.int32, device=dev), coef, pad=64)
    assert tuple(empty.shape) == (0, 64)


# ------------------------------------------------------------------------------------------------ asr_mwer_loss
def _loss(score, err, off, rs, gs):
    from asr_hip import ops
    dev = torch.device("cuda")
    out = ops.mwer_loss(torch.as_tensor(score).to(dev), torch.as_tensor(err).to(dev), torch.as_tensor(off).to(dev), rs, gs)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("ns", [(2,), (16,), (0,), (1,), (0, 1, 2), (16, 2, 1), (2, 16, 0)], ids=lambda ns: "n" + "_".join(map(str, ns)))
def test_mwer_loss_against_the_float64_restatement(ns):
    score, err, off = R.loss_case(ns)
    B = len(ns)
    rs, gs = 0.5 / B, 0.35 / 23.0
    ref = R.mwer(score, err, off, rs, gs)
    t32 = R.mwer(score, err, off, rs, gs, dtype=torch.float32)
    got = _loss(score, err, off, rs, gs)
    for k in ("prob", "coef", "risk", "sums"):
        b32 = R.bound32(ref[k], t32[k])
        x = R.excess(got[k], ref[k], b32)
        print("ns %s %s: worst error / bound %.3f (bound %.3e)" % (ns, k, x, b32))
        assert got[k].dtype == torch.float32 and x <= 1.0, (k, x)
    again = _loss(score, err, off, rs, gs)
    for k in got:
        assert torch.equal(got[k], again[k]), k                    # a second run on the same input: the same bits
    for b, n in enumerate(ns):
        g = int(off[b])
        assert float(got["coef"][g]) == float(np.float32(-gs)) and float(got["prob"][g]) == 0.0
        if n <= 1:
            assert torch.equal(got["coef"][g + 1:g + 1 + n], torch.zeros(n)) and float(got["risk"][b]) == 0.0


def test_mwer_loss_minus_infinity_scores():
    """A hypothesis at -inf: P = 0 and coefficient 0 exactly, the others renormalise; all at -inf: risk 0; a gold at -inf: sums[1] -inf."""
    inf = np.inf
    score = np.array([-3.0, -4.0, -5.0, -2.0, -6.0, -inf, -7.0, -1.0, -inf, -inf], dtype=np.float32)
    err = np.array([0.0, 3.0, 0.0, 0.0, 2.0, 9.0, 4.0, 0.0, 1.0, 2.0], dtype=np.float32)
    off = np.array([0, 2, 3, 7, 10], dtype=np.int32)
    ref = R.mwer(score, err, off, 0.125, 0.1)
    got = _loss(score, err, off, 0.125, 0.1)
    for k in ("prob", "coef", "risk", "sums"):
        assert R.excess(got[k], ref[k], R.bound32(ref[k], R.mwer(score, err, off, 0.125, 0.1, dtype=torch.float32)[k])) <= 1.0, k
    assert got["prob"][5] == 0 and got["coef"][5] == 0 and got["prob"][1] == 1 and got["coef"][1] == 0
    assert torch.equal(got["prob"][8:], torch.zeros(2)) and torch.equal(got["coef"][8:], torch.zeros(2)) and got["risk"][3] == 0
    score[3] = -inf
    assert float(_loss(score, err, off, 0.125, 0.1)["sums"][1]) == -inf
