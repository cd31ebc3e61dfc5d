"""tests/embcnn_reference.py checked on the CPU: the float64 references against torch (F.unfold and its autograd, nn.BatchNorm2d +
F.hardtanh and their autograd), the integer cases exact in float32 in two summation orders, and every assertion of
tests/test_gpu_embcnn_arms.py shown to reject a deliberate defect applied to the reference on the case's own data.

Measured here (float32 CPU evaluation against float64, the worse of two summation orders; b32 is four times that):
  statistics, integer data      mean 0 at a power-of-two count, up to 1.2e-7 else; rstd 4e-9 ... 1.8e-6 relative up to M = 1025, 1.9e-5 at
                                M = 8193 (one element after the other); running mean up to 1.1e-7, running variance up to 2.4e-5 relative
  BatchNorm + Hardtanh, random  b32 of out up to 2.9e-6, of dy up to 6.2e-7, of sum d and sum d x^ up to 1.4e-4; every pre-activation at
                                least 9.8e-4 (Z_MARGIN) off 0 and 20
  emb_cnn module, B 2 F 85      T 24 (seed 0): float32 forward error 5.0e-5, smallest distance of a pre-activation to 0 / 20 7.5e-4;
                                T 25 (seed 2): 5.5e-5 and 6.3e-4; seeds 0 and 1 at T 25 reach only 3.8 x and 3.0 x the error"""
import pytest
import torch
import torch.nn.functional as F

import embcnn_reference as E
from rowwise_reference import excess

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ im2col / col2im
def unfold_columns(x_nhwc, g):
    """F.unfold of the NCHW tensor, its (c, ky, kx) column order permuted to the kernels' (ky, kx, c)."""
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    u = F.unfold(x_nhwc.permute(0, 3, 1, 2), (KH, KW), padding=(PH, PW), stride=(SH, SW))          # (B, C KH KW, OH OW)
    return u.view(B, C, KH, KW, OH * OW).permute(0, 4, 2, 3, 1).reshape(B * OH * OW, KH * KW * C)


@pytest.mark.parametrize("c", E.GEOMS, ids=E.ids(E.GEOMS))
def test_im2col_is_unfold_and_col2im_its_gradient(c):
    k = E.col_case(c.id)
    g, M, K, ld = k["geom"], k["M"], k["K"], k["ld"]
    x = k["x"].double().requires_grad_()
    u = unfold_columns(x, g)
    assert torch.equal(k["col"][:M, :K], u.detach())
    assert not k["col"][M:].any() and not k["col"][:, K:].any() and tuple(k["col"].shape) == (M + 5, ld)
    u.backward(k["dcol"][:, :K].double())
    assert torch.equal(k["dx"], x.grad)
    # adjointness, exact on the integer data
    assert float((k["col"][:M, :K] * k["dcol"][:, :K].double()).sum()) == float((k["x"].double() * k["dx"]).sum())


def test_geometry_table_properties():
    """What the table claims of each geometry, read off the index rule."""
    unc = {c.id: int((~E.covered(c.args)).sum()) for c in E.GEOMS}
    print("EMBCNN_HOST input pixels without a window:", unc)
    assert unc["gaps"] > 0 and unc["stride_pad"] == 0              # (the module docstring: why `gaps` was added)
    k = E.col_case("first_conv")
    assert (k["K"], k["ld"]) == (451, 456)
    k = E.col_case("win_x2")
    assert (k["K"], k["ld"]) == (672, 704)
    for cid, straddle in (("c3", False), ("c12", True)):
        C = E.col_case(cid)["geom"][3]
        assert any((k0 // C) != ((k0 + 7) // C) for k0 in range(0, E.col_case(cid)["K"] - 7, 8)) and (C > 8) == straddle


@pytest.mark.parametrize("c", E.GEOMS, ids=E.ids(E.GEOMS))
def test_im2col_assertion_rejects_defects(c):
    k = E.col_case(c.id)
    g, M, ld = k["geom"], k["M"], k["ld"]
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    defects = ["pad_off", "pad_row"]
    if KH * KW > 1 and (KH > 1 and KW > 1):
        defects.append("tap_transposed")
    if SH != SW:
        defects.append("stride_axis")
    if ld > k["K"]:
        defects.append("pad_col")
    for d in defects:
        assert not torch.equal(E.im2col(k["x"], g, ld, M + 5, defect=d), k["col"]), d


@pytest.mark.parametrize("c", E.GEOMS_C8, ids=E.ids(E.GEOMS_C8))
def test_col2im_assertion_rejects_defects(c):
    k = E.col_case(c.id)
    g = k["geom"]
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    defects = ["pad_off"]
    if KH > 1 and KW > 1:
        defects.append("tap_transposed")
    if SH != SW:
        defects.append("stride_axis")
    if not bool(E.covered(g).all()):
        defects.append("uncovered")
    for d in defects:
        assert not torch.equal(E.col2im(k["dcol"], g, defect=d), k["dx"]), d
    # a pad column of dcol that is read: NaN there would reach dx
    if k["ld"] > k["K"]:
        bad = k["dcol"].clone()
        bad[:, k["K"]:] = float("nan")
        assert torch.equal(E.col2im(bad, g), k["dx"])


def test_every_defect_is_exercised_somewhere():
    """Each index defect applies to at least one geometry of each table (the per-geometry tests skip a defect that cannot show)."""
    for table in (E.GEOMS, E.GEOMS_C8):
        gs = [E.conv_geom(*c.args) for c in table]
        assert any(g[4] > 1 and g[5] > 1 for g in gs) and any(g[6] != g[7] for g in gs)
    assert any(not bool(E.covered(c.args).all()) for c in E.GEOMS_C8)
    assert any(E.geom_ld(c) > E.col_case(c.id)["K"] for c in E.GEOMS_C8)


@pytest.mark.parametrize("c", E.GEOMS_C8, ids=E.ids(E.GEOMS_C8))
def test_col2im_exact_in_float32_in_two_orders(c):
    k = E.col_case(c.id)
    g = k["geom"]
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    d = k["dcol"][:k["M"], :k["K"]].float().reshape(B, OH, OW, KH * KW, C)
    for taps in (list(E._taps(g)), list(E._taps(g))[::-1]):
        dx = torch.zeros(B, H, W, C, dtype=F32)
        for tap, ih, vh, iw, vw in taps:
            if bool(vh.any()) and bool(vw.any()):
                dx[:, ih[vh][:, None], iw[vw][None, :]] += d[:, vh][:, :, vw][:, :, :, tap]
        assert torch.equal(dx.double(), k["dx"])


# ------------------------------------------------------------------------------------------------ window sum
@pytest.mark.parametrize("c", E.WSUM, ids=E.ids(E.WSUM))
def test_window_sum_reference(c):
    groups, Wg, OW, KW, Cout, ldz, ldy, has_bias = c.args
    k = E.wsum_case(c.id)
    want = torch.zeros(groups * OW, ldy, dtype=F64)
    for gi in range(min(groups, 3)):                                  # the definition, written out element by element
        for j in range(OW):
            for co in range(Cout):
                want[gi * OW + j, co] = sum(float(k["Z"][gi * Wg + j + kx, kx * Cout + co]) for kx in range(KW)) + (float(k["bias"][co]) if has_bias else 0.0)
    n = min(groups, 3) * OW
    assert torch.equal(k["y"][:n], want[:n]) and not k["y"][:, Cout:].any()
    # float32, taps added from the far end: exact
    acc = torch.zeros(groups * OW, Cout, dtype=F32)
    rows = (torch.arange(groups)[:, None] * Wg + torch.arange(OW)[None, :]).reshape(-1)
    for kx in range(KW - 1, -1, -1):
        acc = acc + k["Z"][rows + kx, kx * Cout:(kx + 1) * Cout]
    if has_bias:
        acc = acc + k["bias"]
    assert torch.equal(acc.double(), k["y"][:, :Cout])
    if KW > 1 or Wg > OW:
        assert not torch.equal(E.window_sum(torch.cat([k["Z"], k["Z"][:1]]), k["bias"], groups, Wg, OW, KW, Cout, ldy, defect="shift"), k["y"])


# ------------------------------------------------------------------------------------------------ statistics
def torch_bn(y, valid, momentum=0.1, rm0=None, rv0=None, eps=1e-5):
    """float64 nn.BatchNorm2d (training) over the kept rows of compact y -> (module, kept rows with grad, output)."""
    M, C = y.shape
    keep = E.keep_rows(M, valid)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        if rm0 is not None:
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
    yk = y[keep].clone().requires_grad_()
    out = bn(yk.t().reshape(1, C, -1, 1)).reshape(C, -1).t()
    return bn, yk, out, keep


@pytest.mark.parametrize("valid", [None, (6, 9), (1, 9)], ids=["all", "valid6of9", "valid1of9"])
@pytest.mark.parametrize("C", [1, 32])
def test_statistics_equal_torch_batchnorm(C, valid):
    g = torch.Generator().manual_seed(5 + C)
    M = 9 * 41
    y = (torch.randn(M, C, generator=g) * 6 + 5).double()
    rm0, rv0 = torch.randn(C, generator=g).double(), (torch.rand(C, generator=g) + 0.5).double()
    # (the kernels take eps and momentum as fp32 arguments, and so does the reference: torch gets the same two numbers)
    eps32, mom32 = float(torch.tensor(1e-5, dtype=F32)), float(torch.tensor(0.1, dtype=F32))
    bn, yk, _, keep = torch_bn(y, valid, mom32, rm0, rv0, eps32)
    st = E.bn_stats(y, 1e-5, 0.1, rm0, rv0, 0, valid)
    yk = yk.detach()
    assert torch.allclose(st["mean"], yk.mean(0), rtol=1e-13, atol=1e-13)
    assert torch.allclose(st["var"], yk.var(0, unbiased=False), rtol=1e-12, atol=0)
    assert torch.allclose(st["rstd"], torch.rsqrt(yk.var(0, unbiased=False) + eps32), rtol=1e-12, atol=0)
    assert torch.allclose(st["rm"], bn.running_mean, rtol=1e-12, atol=1e-13) and torch.allclose(st["rv"], bn.running_var, rtol=1e-12, atol=0)
    assert st["nb"] == int(bn.num_batches_tracked) == 1
    same = E.bn_stats(y, 1e-5, -1.0, rm0, rv0, 3, valid)
    assert torch.equal(same["rm"], rm0) and torch.equal(same["rv"], rv0) and same["nb"] == 3
    # the defects the GPU bounds must reject: each moves a statistic by more than its b32
    ref, err = E.bn_stats_errors(y, 1e-5, 0.1, rm0, rv0, valid)
    print("EMBCNN_HOST stats C %d valid %s float32 error %s" % (C, valid, {k: "%.2e" % v for k, v in err.items()}))
    defects = ["biased_running"] + (["masked_counted", "count_M"] if valid is not None else [])
    for d in defects:
        bad = E.bn_stats(y, 1e-5, 0.1, rm0, rv0, 0, valid, defect=d)
        worst = max(float(((bad[t] - ref[t]).abs() / (ref[t].abs() if t in E.STAT_RELATIVE else 1.0)).max()) / max(E.B32_FACTOR * err[t], 1e-300)
                    for t in E.STAT_TENSORS)
        assert worst > 1.0, (d, worst)


@pytest.mark.parametrize("C", E.STAT_C)
def test_statistics_integer_cases_exact_in_float32(C):
    for M in E.stat_rows(C):
        k = E.stat_case(C, M)
        for order in (0, 1):
            s, q = E.bn_sums(k["y"], k["center"], dt=F32, order=order)
            assert torch.equal(torch.cat([s, q]).double(), k["sums"]), (C, M, order)
            if k["pow2"]:
                st = E.bn_stats(k["y"], 1e-5, 0.1, k["rm0"], k["rv0"], 0, dt=F32, order=order)
                assert torch.equal(st["mean"].double(), k["y"].mean(0)), (C, M, order)
        if M > E.BN_ROWS:
            s, q = E.bn_sums(k["y"], k["center"], drop_last_block=True)
            assert not torch.equal(torch.cat([s, q]), k["sums"]), (C, M)
        # a gap row read: the 1e30 of the grid reaches the sums
        grid = E.stat_grid(M)
        buf = E.on_grid(k["y"], grid, 1e30)
        assert torch.equal(E.off_grid(buf, M, C, grid), k["y"])
        if M > grid[1]:
            assert not torch.equal(buf[:M, :C], k["y"])
    for mask in (None, "all", "one"):
        bounds = E.stat_bounds(C, mask)
        worst = {t: max(float(torch.as_tensor(b[t]).max()) for _, b in bounds.values()) for t in E.STAT_TENSORS}
        print("EMBCNN_HOST stats C %d mask %s: largest b32 %s" % (C, mask, {t: "%.2e" % v for t, v in worst.items()}))
        # (the mean at a power-of-two count is exact: its bound is 0 and demands equality)
        assert all(float(torch.as_tensor(b[t]).min()) > 0 for _, b in bounds.values() for t in E.STAT_TENSORS if t != "mean"), (C, mask)
        # the defects: a masked row counted, M for the count, the biased variance in the running buffer, the last partial row dropped
        for M, (ref, b) in bounds.items():
            k = E.stat_case(C, M)
            row_w = E.stat_grid(M)[1]
            valid = None if mask is None else (row_w if mask == "all" else 1, row_w)
            defects = ["biased_running"] if E.count_of(M, valid) > 1 else []
            if mask == "one" and row_w > 1:
                defects += ["masked_counted", "count_M"]
            if M > E.BN_ROWS and mask is None:
                defects.append("drop_last_block")
            for d in defects:
                bad = E.bn_stats(k["y"], 1e-5, 0.1, k["rm0"], k["rv0"], 0, valid, defect=d)
                assert max(excess(bad[t], ref[t], b[t], False) for t in E.STAT_TENSORS) > 1.0, (C, M, mask, d)


# ------------------------------------------------------------------------------------------------ BatchNorm + Hardtanh
@pytest.mark.parametrize("valid", [None, (6, 9)], ids=["all", "valid6of9"])
def test_batchnorm_hardtanh_passes_equal_torch_autograd(valid):
    C, M = 32, 9 * 41
    g = torch.Generator().manual_seed(9)
    y = (torch.randn(M, C, generator=g) * 6 + 5).double()
    dz = torch.randn(M, C, generator=g).double()
    bn, yk, out, keep = torch_bn(y, valid, eps=float(torch.tensor(1e-5, dtype=F32)))
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
    o = F.hardtanh(bn(yk.t().reshape(1, C, -1, 1)), E.LO, E.HI).reshape(C, -1).t()
    o.backward(dz[keep])
    st = E.bn_stats(y, bn.eps, -1.0, torch.zeros(C), torch.ones(C), 0, valid)
    x = dict(M=M, C=C, y=y, dz=dz, mean=st["mean"], rstd=st["rstd"], gamma=bn.weight.detach(), beta=bn.bias.detach(), valid=valid)
    r = E.bn_act_eval(x)
    assert torch.allclose(r["out"][keep], o.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["s"], bn.bias.grad, rtol=1e-11, atol=1e-11) and torch.allclose(r["q"], bn.weight.grad, rtol=1e-11, atol=1e-11)
    assert torch.allclose(r["dy"][keep], yk.grad, rtol=1e-10, atol=1e-12)
    assert not r["dy"][~keep].any()


@pytest.mark.parametrize("cid", E.ids(E.ACT_EXACT))
def test_integer_batchnorm_cases_exact_in_float32_and_reject_defects(cid):
    x = E.act_exact_case(cid)
    ref = x["ref"]
    tensors = E.ACT_TENSORS if x["dy_exact"] else ("out", "s", "q")
    for order in (0, 1):
        e = E.bn_act_eval(x, dt=F32, order=order)
        for t in tensors:
            assert torch.equal(e[t].double(), ref[t]), (cid, t, order)
    assert x["on_lo"] > 0 and x["on_hi"] > 0 and 0.25 < x["active"] < 0.65, (x["on_lo"], x["on_hi"], x["active"])
    z = ref["z"]
    assert torch.equal(ref["out"][z == E.LO], torch.full_like(ref["out"][z == E.LO], E.LO))
    assert torch.equal(ref["out"][z == E.HI], torch.full_like(ref["out"][z == E.HI], E.HI))
    # the mask rule: a boundary element let through changes the sums or dy unless its dz is 0 or it is masked out
    keep = E.keep_rows(x["M"], x["valid"])
    for d, edge in (("ge_lo", E.LO), ("le_hi", E.HI)):
        hit = (z == edge) & keep[:, None] & (x["dz"] != 0)
        bad = E.bn_act_eval(x, defect=d)
        if bool(hit.any()):
            assert not torch.equal(bad["dy"], ref["dy"]), (cid, d)
    if x["valid"] is not None:
        for d in ("masked_counted", "count_M"):
            assert not torch.equal(E.bn_act_eval(x, defect=d)["dy"], ref["dy"]), (cid, d)
    # layouts: swapping tH and tW, or ignoring the grid, moves elements
    M, C = x["M"], x["C"]
    if x["tH"] > 0:
        assert not torch.equal(E.to_act(ref["out"], x["tH"], x["tW"]), E.to_act(ref["out"], x["tH"], x["tW"], swapped=True))
        B = M // (x["tH"] * x["tW"])
        want = ref["out"].view(B, x["tH"], x["tW"], C).permute(0, 2, 3, 1).reshape(-1)          # (B, tW, C tH): transformer.py:74-76
        assert torch.equal(E.to_act(ref["out"], x["tH"], x["tW"]), want)
        assert torch.equal(E.from_act(want, M, C, x["tH"], x["tW"]), ref["out"])
    if x["ygrid"][1]:
        buf = E.on_grid(x["y"], x["ygrid"], 1e30, ld=C + 3)
        assert torch.equal(E.off_grid(buf, M, C, x["ygrid"]), x["y"]) and not torch.equal(buf[:M, :C], x["y"])
        dyb = E.on_grid(ref["dy"], x["dygrid"], 7.0)
        gap = torch.ones(dyb.shape[0], dtype=torch.bool)
        gap[E.grid_rows(M, x["dygrid"])] = False
        assert bool((dyb[gap] == 7.0).all()) and int(gap.sum()) == M // x["dygrid"][1] * (x["dygrid"][0] - x["dygrid"][1])


def test_exact_cases_cover_the_boundaries_with_a_gradient():
    """Across the exact cases the `>=` and `<=` defects are both caught (an element on the boundary with dz != 0 on a kept row exists)."""
    caught = {"ge_lo": 0, "le_hi": 0}
    for cid in E.ids(E.ACT_EXACT):
        x = E.act_exact_case(cid)
        for d in caught:
            caught[d] += not torch.equal(E.bn_act_eval(x, defect=d)["dy"], x["ref"]["dy"])
    print("EMBCNN_HOST exact cases that catch >= at lo: %d, <= at hi: %d of %d" % (caught["ge_lo"], caught["le_hi"], len(E.ACT_EXACT)))
    assert caught["ge_lo"] >= len(E.ACT_EXACT) // 2 and caught["le_hi"] >= len(E.ACT_EXACT) // 2


@pytest.mark.parametrize("cid", E.ids(E.ACT_TOL))
def test_random_batchnorm_bounds_reject_defects(cid):
    x = E.act_tol_case(cid)
    ref, b32 = x["ref"], x["b32"]
    print("EMBCNN_HOST %-32s margin %.2e  b32 %s" % (cid, x["margin"], {k: "%.2e" % float(torch.as_tensor(v).max()) for k, v in b32.items()}))
    assert all(float(torch.as_tensor(v).max()) > 0 for v in b32.values()) or x["M"] == 1

    def worst(bad):
        return max(excess(bad[t], ref[t], b32[t], False) for t in E.ACT_TENSORS)
    if x["valid"] is not None:
        for d in ("masked_counted", "count_M"):
            assert worst(E.bn_act_eval(x, defect=d)) > 1.0, (cid, d)
    # one row left out of the sums (what a seam defect does)
    if x["M"] > 1:
        y2 = dict(x, dz=x["dz"].clone())
        y2["dz"][x["M"] - 1] = 0
        bad = E.bn_act_eval(y2)
        if bool(((ref["z"][-1] > E.LO) & (ref["z"][-1] < E.HI)).any()) and (x["valid"] is None or bool(E.keep_rows(x["M"], x["valid"])[-1])):
            assert worst(bad) > 1.0, cid


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("shape", [c.args for c in E.EMB_SHAPES], ids=E.ids(E.EMB_SHAPES))
def test_module_preactivations_stay_off_the_hardtanh_boundaries(shape):
    """The function-level GPU cases compare against the float64 module: an element within the fp32 error of 0 or 20 could sit on the other
    side of the mask in a correct kernel.  Margin >= 8 x the float32 module's forward error (both printed); a seed that fails is replaced
    in EMB_SHAPES."""
    B, Fq, T, seed = shape
    src = E.emb_src(B, Fq, T, seed)
    m64 = E.emb_cnn_module(F64, seed)
    a, b = E.emb_cnn_preacts(m64, src)
    assert tuple(a.shape[2:]) == (23, (T + 20 - 11) // 2 + 1) and b.shape[2] == 2
    m32 = E.emb_cnn_module(F32, seed)
    a32, b32_ = E.emb_cnn_preacts(m32, src.float())
    err = max(float((a32.double() - a).abs().max()), float((b32_.double() - b).abs().max()))
    margin = min(float(torch.minimum((t - E.LO).abs(), (t - E.HI).abs()).min()) for t in (a, b))
    print("EMBCNN_HOST module T %d seed %d: float32 forward error %.2e, smallest distance of a pre-activation to 0 / 20: %.2e" % (T, seed, err, margin))
    assert margin >= 8 * err, (margin, err)
    out = E.emb_cnn_apply(m64, src)
    assert tuple(out.shape) == (B, b.shape[3], 32 * 2)


# ------------------------------------------------------------------------------------------------ the coverage tool
def test_kernel_coverage_embcnn_family_and_group_columns(tmp_path, capsys):
    """tools/kernel_coverage.py --family embcnn (host only): the family is csrc/embcnn.hip, no kernel of it hangs on a tuning hook, and
    `--group NAME=CSV` adds a column of launches per symbol from the trace of a part of the file."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(root, "tools", "kernel_coverage.py"))
    kc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kc)
    assert kc.FAMILIES["embcnn"] == ("embcnn.hip",) and kc.HOOK_ONLY_OF["embcnn"] == ()
    assert os.path.exists(os.path.join(root, "end2end-asr-pytorch_amd", "csrc", "embcnn.hip"))
    a, b = "_ZN12_GLOBAL__N_117window_sum_kernelEPKflPflS1_liiii", "_ZN12_GLOBAL__N_115bn_stats_kernelENS_6BnArgsEPKfPfS3_"
    asm = tmp_path / "asm"
    asm.mkdir()
    (asm / "embcnn.hip.s").write_text("".join("\t.globl\t%s\n%s:\n\ts_endpgm\n.Lfunc_end%d:\n\t.amdhsa_kernel %s\n\t.end_amdhsa_kernel\n" % (s, s, i, s)
                                              for i, s in enumerate((a, b))))
    head = '"Kind","Agent_Id","Kernel_Id","Kernel_Name","Start_Timestamp","End_Timestamp"\n'
    (tmp_path / "all.csv").write_text(head + '"KERNEL_DISPATCH",4,7,"%s.kd",1,2\n"KERNEL_DISPATCH",4,7,"%s.kd",3,4\n' % (a, a))
    (tmp_path / "part.csv").write_text(head + '"KERNEL_DISPATCH",4,7,"%s.kd",1,2\n' % a)
    ks = kc.family_kernels(str(asm), kc.FAMILIES["embcnn"])
    if [s for _, s in ks] != sorted([a, b]):
        pytest.fail("the assembly stand-in is not read as two kernels: %s" % (ks,))
    rc = kc.report(str(asm), str(tmp_path / "all.csv"), None, [], "embcnn", ["window_sum=%s" % (tmp_path / "part.csv")])
    out = capsys.readouterr().out
    assert rc == 1 and "never launched: 1" in out and "NEVER" in out and "window_sum" in out.splitlines()[0]
    row = [ln for ln in out.splitlines() if ln.startswith("embcnn.hip") and "window_sum_kernel" in ln][0].split()
    assert row[1:3] == ["2", "1"]
