"""Every arm of csrc/embcnn.hip -- asr_im2col, asr_col2im, asr_window_sum, the BatchNorm statistics in their three forms, BatchNorm +
Hardtanh forward, backward reduction and backward -- and EmbCNNFn on top of them, against the float64 references of
tests/embcnn_reference.py.

Exact (torch.equal with float64, one RNE where a kernel stores bf16): im2col in its three type arms on eight geometries, zero rows and
  zero pad columns included, in a NaN-filled buffer with guard rows; col2im in both types where C % 8 == 0, NaN in dcol's pad columns,
  adjointness; window_sum without bias, at ldy == Cout, KW = 1, Cout = 4 and over 106 workgroups; the sums of asr_bn_stats (atomics, twice,
  into non-zero integers) and asr_bn_stats_partial (bitwise repeatable) on integer y and centre at every seam of M for C in
  {1, 2, 8, 32, 64, 256}, compact and on a row grid with 1e30 in the gaps; the mean of asr_bn_batch_stats at a power-of-two M; BatchNorm +
  Hardtanh forward, backward sums and -- where the count is a power of two -- backward on integer data, both types, both activation
  layouts, y and dy on row grids, with and without the length mask, elements exactly on lo and hi present and counted.
Bounded by b32 = 4 x the error of the float32 CPU evaluation on the case's data (+ 2^-8 |ref| for bf16 storage): rstd and the running
  buffers; everything at a ragged M on random data; the backward where the count is no power of two.
EmbCNNFn: B = 2, F = 85 (OH_A = 23, OH_B = 2), T = 24 and the odd T = 25, fp32 and bf16 with both settings of the shift forms, against the
  float64 nn.Sequential under the bounds of tests/test_gpu_baseline_shapes.py, e32 / ebf measured here on the case's data.
tests/test_embcnn_reference_host.py proves the yardstick on the CPU.  Every figure is printed before it is asserted (`-s`)."""
import functools

import pytest
import torch

import embcnn_reference as E
from rowwise_reference import excess

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
DT_ID = {F32: "f32", BF16: "bf16"}
REL_BF16, BF16_FLOOR_FACTOR = 5e-2, 2.0          # tests/test_gpu_baseline_shapes.py (the derivation of the factor is written there)


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from asr_hip import lib
    return lib


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
            from asr_hip import lib as L_
            s = str(e)
            if (isinstance(e, L_.AsrHipError) and (s.endswith("(-2)") or s.endswith("(-4)"))) or "HIP error" in s or "CUDA error" in s:
                pytest.exit("%s: %r" % (self.what, e), returncode=3)
        return False


def eq(name, got, want, fails):
    """torch.equal of a device tensor with a float64 expectation (both finite)."""
    g = got.detach().double().cpu()
    if g.shape != want.shape or not torch.equal(g, want):
        bad = (g != want) if g.shape == want.shape else None
        fails.append("%s: %s" % (name, "shape %s vs %s" % (tuple(g.shape), tuple(want.shape)) if bad is None else
                                 "%d of %d elements differ, first %s, max |diff| %.3e" % (int(bad.sum()), bad.numel(), tuple(int(i) for i in torch.nonzero(bad)[0]),
                                                                                         float((g - want).abs().nan_to_num(float("inf")).max()))))


def within(tag, name, got, ref, b32, bf16_stored, fails):
    ex = excess(got, ref, b32, bf16_stored)
    top = float(torch.as_tensor(b32).max())
    print("EMBCNN_ARMS %-52s %-6s error / bound %.3f  (b32 %.2e)" % (tag, name, ex, top))
    if not ex <= 1.0:
        fails.append("%s: error / bound %.3f (b32 %.2e)" % (name, ex, top))


def refused(L, name, *args):
    with pytest.raises(L.AsrHipError):
        L.call(name, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ im2col
IM2COL_ARMS = [(F32, F32), (F32, BF16), (BF16, BF16)]
GUARD_ROWS = 3


def run_im2col(ops, x, g, ld, rows_alloc, out_dtype):
    buf = torch.full((rows_alloc + GUARD_ROWS, ld), float("nan"), device=dev(), dtype=out_dtype)
    ops.im2col(x, g, buf[:rows_alloc])
    return buf


@pytest.mark.parametrize("arm", IM2COL_ARMS, ids=["%s_to_%s" % (DT_ID[a], DT_ID[b]) for a, b in IM2COL_ARMS])
@pytest.mark.parametrize("c", E.GEOMS, ids=E.ids(E.GEOMS))
def test_im2col_exact(ops, c, arm):
    """Rows < rows_alloc = M + 5 equal the reference, zero rows and zero pad columns included; the guard rows behind stay NaN."""
    k = E.col_case(c.id)
    rows = k["M"] + 5
    with card("im2col " + c.id):
        buf = run_im2col(ops, k["x"].to(dev(), arm[0]), k["geom"], k["ld"], rows, arm[1])
    fails = []
    eq("col", buf[:rows], k["col"], fails)
    if not bool(torch.isnan(buf[rows:].float()).all()):
        fails.append("a guard row behind rows_alloc was written")
    assert not fails, "%s:\n  %s" % (c.id, "\n  ".join(fails))


@pytest.mark.parametrize("cid", ["unit", "c3", "first_conv"])
def test_im2col_rounds_to_nearest_even(ops, cid):
    """fp32 -> bf16 on values bf16 cannot hold, ties included: bit for bit the reference of x.bfloat16()."""
    k = E.col_case(cid)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(k["x"].shape, generator=g) * 3
    x.view(-1)[::7] = (torch.randint(-400, 400, x.view(-1)[::7].shape, generator=g).float() * 2 + 1) * 2.0 ** -8    # odd multiples of 2^-8 around 1 .. 3: ties
    rows = k["M"] + 5
    with card("im2col rne " + cid):
        buf = run_im2col(ops, x.to(dev()), k["geom"], k["ld"], rows, BF16)
    want = E.im2col(x.bfloat16(), k["geom"], k["ld"], rows)
    ties = int((x.bfloat16().float() != x).sum())
    print("EMBCNN_ARMS im2col rne %s: %d of %d inputs are not bf16 numbers" % (cid, ties, x.numel()))
    fails = []
    eq("col", buf[:rows], want, fails)
    assert ties > x.numel() // 2 and not fails, fails


def test_im2col_refusals_leave_the_buffer_alone(ops, L):
    k = E.col_case("unit")
    g, M, K, ld = k["geom"], k["M"], k["K"], k["ld"]
    x32, x16 = k["x"].to(dev()), k["x"].to(dev(), BF16)
    buf32 = torch.full((M + 8, ld + 8), float("nan"), device=dev())
    buf16 = torch.full((M + 8, ld + 8), float("nan"), device=dev(), dtype=BF16)
    bad_oh = g[:10] + (g[10] + 1, g[11])
    with card("im2col refusals"):
        refused(L, "asr_im2col", L.ptr(x16), L.ptr(buf32), *g, ld, M, L.dt(x16), L.dt(buf32), L.stream())          # bf16 -> fp32
        refused(L, "asr_im2col", L.ptr(x32), L.ptr(buf32), *g, ld + 4, M, L.dt(x32), L.dt(buf32), L.stream())      # ld % 8 != 0
        refused(L, "asr_im2col", L.ptr(x32), L.ptr(buf32), *g, K - 8, M, L.dt(x32), L.dt(buf32), L.stream())       # ld < K
        refused(L, "asr_im2col", L.ptr(x32), L.ptr(buf32), *g, ld, M - 1, L.dt(x32), L.dt(buf32), L.stream())      # rows_alloc < M
        refused(L, "asr_im2col", L.ptr(x32), L.ptr(buf32), *bad_oh, ld, M + 8, L.dt(x32), L.dt(buf32), L.stream())  # OH does not match
        refused(L, "asr_im2col", L.ptr(x16), L.ptr(buf16), *bad_oh, ld, M + 8, L.dt(x16), L.dt(buf16), L.stream())
    assert bool(torch.isnan(buf32).all()) and bool(torch.isnan(buf16.float()).all())


# ------------------------------------------------------------------------------------------------ col2im
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", E.GEOMS_C8, ids=E.ids(E.GEOMS_C8))
def test_col2im_exact(ops, c, dtype):
    """dx equals the scatter-add reference; pad columns of dcol hold NaN and must not be read; <im2col(x), d> == <x, col2im(d)> on the
    kernels' own outputs."""
    k = E.col_case(c.id)
    g, M, K, ld = k["geom"], k["M"], k["K"], k["ld"]
    dcol = k["dcol"].clone()
    dcol[:, K:] = float("nan")
    with card("col2im " + c.id):
        dx = ops.col2im(dcol.to(dev(), dtype), g)
        col = run_im2col(ops, k["x"].to(dev(), dtype), g, ld, M, dtype)[:M]
    fails = []
    eq("dx", dx, k["dx"], fails)
    lhs = float((col[:, :K].double() * k["dcol"][:, :K].double().to(dev())).sum())
    rhs = float((k["x"].double().to(dev()) * dx.double()).sum())
    print("EMBCNN_ARMS col2im %-10s %-4s <im2col(x), d> %.1f  <x, col2im(d)> %.1f  uncovered pixels %d" % (
        c.id, DT_ID[dtype], lhs, rhs, int((~E.covered(g)).sum())))
    if lhs != rhs:
        fails.append("adjointness: %.1f vs %.1f" % (lhs, rhs))
    assert not fails, "%s:\n  %s" % (c.id, "\n  ".join(fails))


def test_col2im_refuses_channels_that_are_no_multiple_of_8(ops, L):
    for cid in ("c3", "c12", "first_conv"):
        k = E.col_case(cid)
        g = k["geom"]
        dcol = k["dcol"].to(dev())
        dx = torch.full((g[0], g[1], g[2], g[3] + 8), float("nan"), device=dev())
        with card("col2im refusal"):
            refused(L, "asr_col2im", L.ptr(dcol), L.ptr(dx), *g, k["ld"], L.dt(dcol), L.stream())
        assert bool(torch.isnan(dx).all())


# ------------------------------------------------------------------------------------------------ window sum
@pytest.mark.parametrize("c", E.WSUM, ids=E.ids(E.WSUM))
def test_window_sum_arms(ops, c):
    groups, Wg, OW, KW, Cout, ldz, ldy, has_bias = c.args
    k = E.wsum_case(c.id)
    y = torch.full((groups * OW + 3, ldy), 7.0, device=dev())
    with card("window_sum " + c.id):
        ops.window_sum(k["Z"].to(dev()), y, k["bias"].to(dev()) if has_bias else None, groups, Wg, OW, KW, Cout)
    fails = []
    eq("y", y[:groups * OW], k["y"], fails)
    if not bool((y[groups * OW:] == 7.0).all()):
        fails.append("a row behind groups x OW was written")
    assert not fails, "%s:\n  %s" % (c.id, "\n  ".join(fails))


# ------------------------------------------------------------------------------------------------ statistics
def stats_call(ops, ybuf, M, C, eps, momentum, rm, rv, nb, grid, valid):
    return ops.bn_train_stats(ybuf, M, C, eps, momentum, rm, rv, nb, ygrid=grid, valid=valid)


@pytest.mark.parametrize("layout", ["compact", "grid"])
@pytest.mark.parametrize("C", E.STAT_C)
def test_statistics_at_the_seams(ops, L, C, layout):
    """Per M of stat_rows(C): asr_bn_stats twice into non-zero integers, asr_bn_stats_partial (twice, bitwise equal) -- both equal the
    float64 sums; asr_bn_batch_stats: mean equal at a power-of-two M, else within b32; rstd and the running buffers within b32,
    num_batches 1 and then 2; momentum < 0 leaves the buffers bit-identical; on the grid the _v form with valid = row_w (bitwise the
    unmasked result) and valid = 1."""
    G = dev()
    fails = []
    for M in E.stat_rows(C):
        k = E.stat_case(C, M)
        grid = E.stat_grid(M) if layout == "grid" else (0, 0)
        tag = "stats C %d M %d %s" % (C, M, layout)
        ld = C + (4 if layout == "grid" else 0)
        ybuf = E.on_grid(k["y"], grid, 1e30, ld=ld).float().to(G)
        center = k["center"].float().to(G)
        sums = k["prior"].float().to(G)
        nblk = L.load().asr_bn_stats_blocks(M)
        assert nblk == (M + E.BN_ROWS - 1) // E.BN_ROWS
        parts = [torch.full((nblk, 2 * C), float("nan"), device=G) for _ in range(2)]
        psums = [torch.full((2 * C,), float("nan"), device=G) for _ in range(2)]
        rm, rv = k["rm0"].float().to(G), k["rv0"].float().to(G)
        nb = torch.zeros((), dtype=torch.int64, device=G)
        with card(tag):
            for _ in range(2):
                L.call("asr_bn_stats", L.ptr(ybuf), ybuf.stride(0), M, C, L.ptr(center), L.ptr(sums), grid[0], grid[1], L.stream())
            for p, s in zip(parts, psums):
                L.call("asr_bn_stats_partial", L.ptr(ybuf), ybuf.stride(0), M, C, L.ptr(center), L.ptr(p), L.ptr(s), grid[0], grid[1], L.stream())
            mean, rstd = stats_call(ops, ybuf, M, C, 1e-5, 0.1, rm, rv, nb, grid, None)
            rm1, rv1, nb1 = rm.clone(), rv.clone(), int(nb)
            mean2, rstd2 = stats_call(ops, ybuf, M, C, 1e-5, -1.0, rm, rv, nb, grid, None)
            frozen = torch.equal(rm, rm1) and torch.equal(rv, rv1) and int(nb) == 1
            stats_call(ops, ybuf, M, C, 1e-5, 0.1, rm, rv, nb, grid, None)
        f = []
        eq("asr_bn_stats twice on the prior contents", sums, k["prior"] + 2 * k["sums"], f)
        eq("asr_bn_stats_partial", psums[0], k["sums"], f)
        if not (torch.equal(psums[0].view(torch.int32), psums[1].view(torch.int32)) and torch.equal(parts[0].view(torch.int32), parts[1].view(torch.int32))):
            f.append("asr_bn_stats_partial: two calls differ in their bits")
        ref, b32 = E.stat_bounds(C, None)[M]
        if k["pow2"]:
            eq("mean (power-of-two M)", mean, ref["mean"], f)
        got = dict(mean=mean, rstd=rstd, rm=rm1, rv=rv1)
        for t in E.STAT_TENSORS:
            within(tag, t, got[t], ref[t], b32[t], False, f)
        if not (torch.equal(mean2, mean) and torch.equal(rstd2, rstd) and frozen):
            f.append("momentum < 0: statistics differ or a running buffer moved")
        if nb1 != 1 or int(nb) != 2:
            f.append("num_batches %d then %d" % (nb1, int(nb)))
        if layout == "grid":
            row_w = grid[1]
            for nv in sorted({row_w, 1}):
                valid = (nv, row_w)
                refv, b32v = E.stat_bounds(C, "all" if nv == row_w else "one")[M]
                rmv, rvv = k["rm0"].float().to(G), k["rv0"].float().to(G)
                nbv = torch.zeros((), dtype=torch.int64, device=G)
                with card(tag + " valid %d" % nv):
                    mv, rsv = stats_call(ops, ybuf, M, C, 1e-5, 0.1, rmv, rvv, nbv, grid, (torch.tensor([nv], dtype=torch.int32, device=G), row_w))
                gotv = dict(mean=mv, rstd=rsv, rm=rmv, rv=rvv)
                for t in E.STAT_TENSORS:
                    within(tag + " valid %d of %d" % valid, t, gotv[t], refv[t], b32v[t], False, f)
        fails += ["%s: %s" % (tag, x) for x in f]
    assert not fails, "\n  ".join(fails[:16])


def test_statistics_refusals(ops, L):
    G = dev()
    y = torch.zeros(64, 512, device=G)
    out = torch.full((1024,), float("nan"), device=G)
    part = torch.full((4, 1024), float("nan"), device=G)
    mean, rstd = torch.full((512,), float("nan"), device=G), torch.full((512,), float("nan"), device=G)
    with card("statistics refusals"):
        for C, M, grid in ((3, 64, (0, 0)), (512, 64, (0, 0)), (32, 64, (13, 9))):            # 256 % C, C > 256, M % OW != 0
            refused(L, "asr_bn_stats", L.ptr(y), 512, M, C, None, L.ptr(out), grid[0], grid[1], L.stream())
            refused(L, "asr_bn_stats_partial", L.ptr(y), 512, M, C, None, L.ptr(part), L.ptr(out), grid[0], grid[1], L.stream())
            refused(L, "asr_bn_batch_stats", L.ptr(y), 512, M, C, L.ptr(part), L.ptr(mean), L.ptr(rstd), 1e-5, -1.0, None, None, None,
                    grid[0], grid[1], L.stream())
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(part).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(rstd).all())


# ------------------------------------------------------------------------------------------------ BatchNorm + Hardtanh
def run_bn_act(ops, x, dtype):
    """One case through asr_bn_act_fwd and asr_bn_act_bwd_reduce_v + asr_bn_act_bwd_v -> (out (M, C), sums (2C), dy (M, C), dy's gap rows)."""
    G = dev()
    M, C, tH, tW = x["M"], x["C"], x["tH"], x["tW"]
    ybuf = E.on_grid(x["y"], x["ygrid"], 1e30, ld=C + (8 if x["ygrid"][1] else 0)).float().to(G)
    p = [x[n].float().to(G) for n in ("mean", "rstd", "gamma", "beta")]
    ldo = C + (8 if tH == 0 else 0)
    out = torch.full((M * (C if tH else ldo),), -3.0, device=G, dtype=dtype)
    dout = E.to_act(x["dz"], tH, tW, ldo, fill=float("nan")).to(G, dtype)
    dy_rows = M // x["dygrid"][1] * x["dygrid"][0] if x["dygrid"][1] else M
    dyb = torch.full((dy_rows, C + 8), 7.0, device=G, dtype=dtype)
    valid = (torch.tensor([x["valid"][0]], dtype=torch.int32, device=G), x["valid"][1]) if x["valid"] is not None else None
    ops.bn_act_fwd(ybuf, M, C, *p, E.LO, E.HI, out if tH else out.view(M, ldo), tH=tH, tW=tW, ygrid=x["ygrid"])
    sums = ops.bn_act_bwd(dout if tH else dout.view(M, ldo), ybuf, M, C, *p, E.LO, E.HI, dyb, tH=tH, tW=tW, ygrid=x["ygrid"],
                          dygrid=x["dygrid"], valid=valid)
    torch.cuda.synchronize()
    gap = torch.ones(dyb.shape[0], dtype=torch.bool)
    gap[E.grid_rows(M, x["dygrid"])] = False
    untouched = bool((dyb[gap.to(G)].float() == 7.0).all()) and bool((dyb[:, C:].float() == 7.0).all())
    if tH == 0:
        untouched = untouched and bool((out.view(M, ldo)[:, C:].float() == -3.0).all())
    return E.from_act(out, M, C, tH, tW, ldo), sums, E.off_grid(dyb, M, C, x["dygrid"]), untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cid", E.ids(E.ACT_EXACT))
def test_batchnorm_hardtanh_exact(ops, cid, dtype):
    x = E.act_exact_case(cid)
    ref = x["ref"]
    with card("bn_act exact " + cid):
        out, sums, dy, untouched = run_bn_act(ops, x, dtype)
    C = x["C"]
    fails = []
    eq("out", out, E.stored(ref["out"], dtype), fails)
    eq("sum d", sums[:C], ref["s"], fails)
    eq("sum d x^", sums[C:], ref["q"], fails)
    if x["dy_exact"]:
        eq("dy", dy, E.stored(ref["dy"], dtype), fails)
    else:
        within("bn_act exact " + cid + " " + DT_ID[dtype], "dy", dy, ref["dy"], x["b32_dy"], dtype == BF16, fails)
    z = ref["z"]
    on = (z == E.LO) | (z == E.HI)
    keep = E.keep_rows(x["M"], x["valid"])
    print("EMBCNN_ARMS bn_act exact %-34s %-4s on lo %d, on hi %d, active %.2f, dy %s" % (
        cid, DT_ID[dtype], x["on_lo"], x["on_hi"], x["active"], "exact" if x["dy_exact"] else "within b32"))
    if x["on_lo"] == 0 or x["on_hi"] == 0:
        fails.append("no element exactly on lo / hi")
    o = out.double().cpu()
    if not (bool((o[z == E.LO] == E.LO).all()) and bool((o[z == E.HI] == E.HI).all())):
        fails.append("an element on a boundary does not hold the clamp value")
    # no gradient through a boundary element: dy there is the gradient of d = 0
    if x["dy_exact"]:
        d0 = E.stored((-(ref["s"] + ((x["y"] - x["mean"]) * x["rstd"]) * ref["q"]) / E.count_of(x["M"], x["valid"]) * x["gamma"] * x["rstd"]) * keep[:, None], dtype)
        if not torch.equal(dy.double().cpu()[on], d0[on]):
            fails.append("an element on a boundary received a gradient")
    if not untouched:
        fails.append("a gap row of dy or a pad column was written")
    assert not fails, "%s:\n  %s" % (cid, "\n  ".join(fails))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cid", E.ids(E.ACT_TOL))
def test_batchnorm_hardtanh_ragged_rows_against_float64(ops, cid, dtype):
    x = E.act_tol_case(cid)
    ref, b32 = x["ref"], x["b32"]
    # the gradient arrives in the storage type: the reference gets the same rounded dz
    if dtype == BF16:
        x = dict(x, dz=x["dz"].to(BF16).double())
        ref = E.bn_act_eval(x)
    with card("bn_act ragged " + cid):
        out, sums, dy, untouched = run_bn_act(ops, x, dtype)
    C, bf = x["C"], dtype == BF16
    tag = "bn_act ragged %s %s" % (cid, DT_ID[dtype])
    fails = []
    within(tag, "out", out, ref["out"], b32["out"], bf, fails)
    within(tag, "s", sums[:C], ref["s"], b32["s"], False, fails)
    within(tag, "q", sums[C:], ref["q"], b32["q"], False, fails)
    within(tag, "dy", dy, ref["dy"], b32["dy"], bf, fails)
    if x["valid"] is not None and not bool((dy.float().cpu()[~E.keep_rows(x["M"], x["valid"])] == 0).all()):
        fails.append("a masked row received a gradient")
    if not untouched:
        fails.append("a gap row of dy or a pad column was written")
    assert not fails, "%s:\n  %s" % (cid, "\n  ".join(fails))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_batchnorm_hardtanh_plain_entry_points(ops, L, dtype):
    """asr_bn_act_bwd_reduce / asr_bn_act_bwd (no length mask argument) equal the _v forms with a null mask, bit for bit."""
    G = dev()
    x = E.act_exact_case("flat_grid_M512-C32")
    M, C = x["M"], x["C"]
    ybuf = E.on_grid(x["y"], x["ygrid"], 1e30).float().to(G)
    p = [x[n].float().to(G) for n in ("mean", "rstd", "gamma", "beta")]
    dout = x["dz"].to(G, dtype)
    dyb = torch.full((M // x["dygrid"][1] * x["dygrid"][0], C), 7.0, device=G, dtype=dtype)
    sums = torch.zeros(2 * C, device=G)
    with card("bn_act plain entry points"):
        L.call("asr_bn_act_bwd_reduce", L.ptr(dout), C, L.ptr(ybuf), ybuf.stride(0), M, C, *[L.ptr(t) for t in p], E.LO, E.HI, 0, 0,
               x["ygrid"][0], x["ygrid"][1], L.ptr(sums), L.dt(dout), L.stream())
        L.call("asr_bn_act_bwd", L.ptr(dout), C, L.ptr(ybuf), ybuf.stride(0), L.ptr(dyb), C, M, C, *[L.ptr(t) for t in p], E.LO, E.HI, 0, 0,
               x["ygrid"][0], x["ygrid"][1], x["dygrid"][0], x["dygrid"][1], L.ptr(sums), L.dt(dout), L.stream())
    fails = []
    eq("sums", sums, torch.cat([x["ref"]["s"], x["ref"]["q"]]), fails)
    eq("dy", E.off_grid(dyb, M, C, x["dygrid"]), E.stored(x["ref"]["dy"], dtype), fails)
    assert not fails, fails


def test_batchnorm_hardtanh_refusals(ops, L):
    G = dev()
    y = torch.zeros(64, 512, device=G)
    v = torch.ones(512, device=G)
    out = torch.full((64 * 512,), float("nan"), device=G)
    with card("bn_act refusals"):
        for C, M, tH, tW, grid in ((3, 64, 0, 0, (0, 0)), (512, 64, 0, 0, (0, 0)), (32, 64, 0, 0, (13, 9)), (32, 64, 3, 7, (0, 0))):
            refused(L, "asr_bn_act_fwd", L.ptr(y), 512, L.ptr(out), 512, M, C, L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(v), E.LO, E.HI, tH, tW,
                    grid[0], grid[1], L.dt(out), L.stream())
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ EmbCNNFn against the float64 module
PARAMS = ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias")
BUFFERS = ("1.running_mean", "1.running_var", "4.running_mean", "4.running_var")
NOISE = ("0.bias", "3.bias")        # a convolution bias in front of a training-mode BatchNorm: the exact gradient is zero (big_cases.noise_driven)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def module_run(m, src, dout, autocast=False):
    """Training forward + backward of the torch module -> (out, {parameter / buffer: tensor}, per-channel sum |dL/dy| of both convolutions,
    eval-mode output from the updated running statistics)."""
    m.train()
    m.zero_grad()
    taps = {}

    def tap(i):
        def fwd(mod, inp, res):
            res.register_hook(lambda g: taps.__setitem__(i, g.detach().double().abs().sum((0, 2, 3))))
        return fwd
    hooks = [m[i].register_forward_hook(tap(i)) for i in (0, 3)]
    if autocast:
        with torch.autocast("cpu", dtype=BF16):
            out = E.emb_cnn_apply(m, src)
    else:
        out = E.emb_cnn_apply(m, src)
    out.float().backward(dout.float()) if autocast else out.backward(dout.to(out.dtype))
    for h in hooks:
        h.remove()
    t = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    t.update({k: b.detach().clone() for k, b in m.named_buffers() if k in BUFFERS})
    m.eval()
    with torch.no_grad():
        if autocast:
            with torch.autocast("cpu", dtype=BF16):
                ev = E.emb_cnn_apply(m, src)
        else:
            ev = E.emb_cnn_apply(m, src)
    nbt = (int(m[1].num_batches_tracked), int(m[4].num_batches_tracked))
    return out.detach(), t, taps, ev.detach(), nbt


@functools.lru_cache(maxsize=None)
def emb_truth(cid):
    """float64 truth of a shape and the errors e32 / ebf of the same module in float32 and under autocast(cpu, bfloat16) against it."""
    B, Fq, T, seed = [c for c in E.EMB_SHAPES if c.id == cid][0].args
    src = E.emb_src(B, Fq, T, seed)
    m64 = E.emb_cnn_module(F64, seed)
    o_shape = E.emb_cnn_apply(m64, src).shape
    m64 = E.emb_cnn_module(F64, seed)
    dout = torch.randn(o_shape, generator=torch.Generator().manual_seed(T)).double()
    out, t64, taps, ev, nbt = module_run(m64, src, dout)
    floors = {}
    for name, ac in (("e32", False), ("ebf", True)):
        o, t, tp, e_, _ = module_run(E.emb_cnn_module(F32, seed), src.float(), dout.float(), autocast=ac)
        f = {k: (rel_l2(t[k], t64[k]) if k not in NOISE else float(t[k].double().norm() / taps[int(k[0])].norm())) for k in t64}
        f["out_abs"] = float((o.double() - out).abs().max())
        floors[name] = f
    return dict(src=src, dout=dout, out=out, t=t64, taps=taps, eval=ev, nbt=nbt, floors=floors, seed=seed)


def emb_apply(Fn, m, src, training=True):
    c = m
    return Fn.EmbCNNFn.apply(src, c[0].weight, c[0].bias, c[1].weight, c[1].bias, c[3].weight, c[3].bias, c[4].weight, c[4].bias, c[1], c[4], training)


def emb_check(tag, precision, tr, out, m, out_slice=None):
    """Output, eight gradients and four running buffers of a device module against the truth `tr` under the project's bounds."""
    fails = []
    ref_out = tr["out"]
    o = out.detach().double().cpu()
    if out_slice is not None:
        o = o[:, :out_slice]
    amax = float(ref_out.abs().max())
    perr = float((o - ref_out).abs().max())
    pb = 5e-5 * max(1.0, amax) if precision == "fp32" else 4e-2 * amax
    print("EMBCNN_ARMS %-30s output max error %.3e (bound %.3e, max |out| %.2f; float32 torch module %.2e, autocast %.2e)" % (
        tag, perr, pb, amax, tr["floors"]["e32"]["out_abs"], tr["floors"]["ebf"]["out_abs"]))
    if not (bool(torch.isfinite(o).all()) and perr <= pb):
        fails.append("output: %.3e > %.3e" % (perr, pb))
    got = {k: p.grad for k, p in m.named_parameters()}
    got.update({k: b for k, b in m.named_buffers() if k in BUFFERS})
    floor = tr["floors"]["e32" if precision == "fp32" else "ebf"]
    for k in PARAMS + BUFFERS:
        g = got[k].detach().double().cpu()
        err = rel_l2(g, tr["t"][k]) if k not in NOISE else float(g.norm() / tr["taps"][int(k[0])].norm())
        bound = max(2e-4, 4 * floor[k]) if precision == "fp32" else max(REL_BF16, BF16_FLOOR_FACTOR * floor[k])
        print("EMBCNN_ARMS %-30s %-16s %s %.3e  bound %.3e  (torch %s %.3e)" % (
            tag, k, "|g| / |sum |dy||" if k in NOISE else "relative L2    ", err, bound, "e32" if precision == "fp32" else "ebf", floor[k]))
        if not err <= bound:
            fails.append("%s: %.3e > %.3e" % (k, err, bound))
    return fails


EMB_MODES = [("fp32", None), ("bf16", True), ("bf16", False)]


@pytest.mark.parametrize("mode", EMB_MODES, ids=["fp32", "bf16_shift", "bf16_window"])
@pytest.mark.parametrize("c", E.EMB_SHAPES, ids=E.ids(E.EMB_SHAPES))
def test_emb_cnn_function_against_float64_module(ops, c, mode, monkeypatch):
    from asr_hip import functions as Fn
    precision, shift = mode
    if shift is not None:
        monkeypatch.setattr(Fn, "_emb_shift_fwd", shift)
        monkeypatch.setattr(Fn, "_emb_shift_wgrad", shift)
    B, Fq, T, seed = c.args
    tr = emb_truth(c.id)
    G = dev()
    m = E.emb_cnn_module(F32, seed).to(G)
    src = tr["src"].float().to(G)
    prev = ops.compute_dtype()
    ops.set_compute_dtype(BF16 if precision == "bf16" else F32)
    try:
        gA = ops.conv_geom(B, Fq, T, 1, 41, 11, 2, 2, 0, 10)
        gB = ops.conv_geom(B, gA[10], gA[11], 32, 21, 11, 2, 1, 0, 0)
        assert (gA[10], gB[10]) == (23, 2)
        assert Fn._window_ok(gA) == (precision == "bf16" and T % 2 == 0) and Fn._window_ok(gB) == (precision == "bf16")
        tag = "emb %s %s" % (c.id, "fp32" if shift is None else "bf16 shift %d" % shift)
        with card(tag):
            out = emb_apply(Fn, m, src)
            out.backward(tr["dout"].to(G, out.dtype))
        fails = emb_check(tag, precision, tr, out, m)
        nbt = (int(m[1].num_batches_tracked), int(m[4].num_batches_tracked))
        if nbt != tr["nbt"]:
            fails.append("num_batches_tracked %s, reference %s" % (nbt, tr["nbt"]))
        m.eval()
        with card(tag + " eval"):
            with torch.no_grad():
                ev = emb_apply(Fn, m, src, training=False)
        amax = float(tr["eval"].abs().max())
        eerr = float((ev.double().cpu() - tr["eval"]).abs().max())
        eb = 5e-5 * max(1.0, amax) if precision == "fp32" else 4e-2 * amax
        print("EMBCNN_ARMS %-30s eval-mode output max error %.3e (bound %.3e)" % (tag, eerr, eb))
        if not eerr <= eb:
            fails.append("eval-mode output: %.3e > %.3e" % (eerr, eb))
        assert not fails, "%s:\n  %s" % (tag, "\n  ".join(fails))
    finally:
        ops.set_compute_dtype(prev)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_emb_cnn_function_length_mask_on_a_padded_batch(ops, precision, monkeypatch):
    """functions.emb_valid on the T = 24 batch padded by six zero frames: the valid steps of the output, every gradient and the running
    buffers are those of the module on the unpadded batch."""
    from asr_hip import functions as Fn
    c = E.EMB_SHAPES[0]
    B, Fq, T, seed = c.args
    tr = emb_truth(c.id)
    G = dev()
    t1 = (T + 20 - 11) // 2 + 1
    m = E.emb_cnn_module(F32, seed).to(G)
    src = torch.zeros(B, 1, Fq, T + E.EMB_PAD_FRAMES)
    src[..., :T] = tr["src"].float()
    monkeypatch.setattr(Fn, "emb_valid", torch.tensor([t1, t1 - 10], dtype=torch.int32, device=G))
    prev = ops.compute_dtype()
    ops.set_compute_dtype(BF16 if precision == "bf16" else F32)
    try:
        tag = "emb T24+6 valid %s" % precision
        with card(tag):
            out = emb_apply(Fn, m, src.to(G))
            dout = torch.zeros(out.shape, device=G, dtype=out.dtype)
            dout[:, :t1 - 10] = tr["dout"].to(G, out.dtype)
            out.backward(dout)
        assert out.shape[1] == (T + E.EMB_PAD_FRAMES + 20 - 11) // 2 + 1 - 10 and tr["out"].shape[1] == t1 - 10
        fails = emb_check(tag, precision, tr, out, m, out_slice=t1 - 10)
        assert not fails, "%s:\n  %s" % (tag, "\n  ".join(fails))
    finally:
        ops.set_compute_dtype(prev)


def test_emb_cnn_backward_after_a_later_forward_is_refused(ops):
    from asr_hip import functions as Fn
    c = E.EMB_SHAPES[0]
    B, Fq, T, seed = c.args
    G = dev()
    m = E.emb_cnn_module(F32, seed).to(G)
    src = emb_truth(c.id)["src"].float().to(G)
    with card("emb generation"):
        first = emb_apply(Fn, m, src)
        second = emb_apply(Fn, m, src)
    with pytest.raises(RuntimeError, match="backward after a later emb_cnn forward"):
        first.sum().backward()
    with card("emb generation, latest"):
        second.float().sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
