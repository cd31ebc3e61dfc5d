"""Every arm of the convolution front end and of the pooling kernels (csrc/conv1.hip, conv1_wgrad_mfma.hip, conv_igemm.hip, conv_c64.hip,
conv_ws.hip, conv_wgrad.hip, conv_wgrad_dma.hip, conv_level0.hip, pool.hip; reference models/asr/transformer.py:42-53, 70-76 and their
autograd) through the C ABI, bit for bit against float64.

The data, the references and the case tables are those of tests/conv_reference.py: small integers, so that every partial sum is an fp32
number in any order and every assertion below is torch.equal -- against the float64 reference and, where a hook selects a kernel the
dispatch would not take, also against the kernel it takes with no hook set.  tests/test_conv_reference_host.py shows on the CPU that
the cases are order-independent and that they see a dropped border row, a transposed tap, a shifted bias and a wrong pooling rule.
Hooks are set with lib.set_tuning and cleared in `finally`; cases that set one carry "hooked" in their ids (`-k "not hooked"` is the
run of the automatic dispatch alone; tools/kernel_coverage.py --family conv turns the two kernel traces into launches per symbol).
"""
import contextlib

import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu
D = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]
dtype_id = lambda d: str(d).replace("torch.", "")
case_id = lambda c: c.id


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    return o


@contextlib.contextmanager
def tuning(switches):
    from asr_hip import lib as L
    try:
        for k, v in switches.items():
            L.set_tuning(k, v)
        yield
    finally:
        for k in switches:
            L.set_tuning(k, None)


def pack(ops, w, dtype):
    """(wk, wd) on the device from the library's own packer."""
    Cout, Cin = w.shape[:2]
    wk = torch.empty(Cout, 9, Cin, device=D, dtype=dtype)
    wd = torch.empty(Cin, 9, Cout, device=D, dtype=dtype)
    ops.conv_pack_weight(w.to(D), wk, wd)
    return wk, wd


def same(got, want, what=""):
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got.float() != want.float()).nonzero()
        raise AssertionError("%s: %d of %d elements differ, first at %s (got %s, want %s)" % (
            what, len(bad), got.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))


# ------------------------------------------------------------------------------------------------ conv.0
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("case", R.CONV1_FWD, ids=case_id)
def test_conv1_fwd(ops, case, dtype):
    src, w, bias = R.conv1_case(*case.args)[:3]
    y = ops.conv1_fwd(src.to(D), w.to(D), bias.to(D), dtype)
    same(y, R.conv1_forward_ref(src, w, bias, dtype), case.pins)


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("case", R.CONV1_WGRAD, ids=case_id)
def test_conv1_wgrad_accumulates_exactly(ops, case, dtype):
    """fp32: conv1_wgrad_kernel<float>; bf16: the MFMA kernel at C0 = 64, conv1_wgrad_kernel<bf16> at C0 = 32.  dw / db hold integers on
    entry; a second call adds exactly the same increment."""
    src, w, bias, dy, dw0, db0, dw, db = R.conv1_case(*case.args)
    sd, dyd = src.to(D), dy.to(D, dtype)
    gw, gb = dw0.to(D), db0.to(D)
    for n in (1, 2):
        ops.conv1_wgrad(sd, dyd, gw, gb)
        same(gw, dw0 + n * dw, "%s: dw after call %d" % (case.pins, n))
        same(gb, db0 + n * db, "%s: db after call %d" % (case.pins, n))


# ------------------------------------------------------------------------------------------------ weight packing
PACK_SHAPES = [(64, 64), (128, 64), (128, 128), (64, 128), (64, 192), (128, 192), (64, 64), (128, 128)]        # (Cout, Cin)


def _masters(n):
    g = torch.Generator().manual_seed(n)
    return [torch.randn(co, ci, 3, 3, generator=g) for co, ci in PACK_SHAPES[:n]]


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_pack_weight_is_the_documented_permutation(ops, dtype):
    """wk (Cout, 9, Cin) with tap = ky * 3 + kx and wd (Cin, 9, Cout) with the taps flipped, one rounding to `dtype`; with only wk or
    only wd the other pointer is null."""
    for w in _masters(6)[1:]:
        Cout, Cin = w.shape[:2]
        wk_ref, wd_ref = (t.to(dtype) for t in R.pack_rule(w))
        wk, wd = pack(ops, w, dtype)
        same(wk, wk_ref, "wk")
        same(wd, wd_ref, "wd")
        wk1 = torch.zeros_like(wk)
        ops.conv_pack_weight(w.to(D), wk1, None)
        same(wk1, wk_ref, "wk alone")
        wd1 = torch.zeros_like(wd)
        ops.conv_pack_weight(w.to(D), None, wd1)
        same(wd1, wd_ref, "wd alone")


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("n", [1, 3, 8])
def test_pack_weight_multi_equals_the_single_packs(ops, n, dtype):
    ws = [w.to(D) for w in _masters(n)]
    items = [(w, torch.zeros(w.shape[0], 9, w.shape[1], device=D, dtype=dtype), torch.zeros(w.shape[1], 9, w.shape[0], device=D, dtype=dtype))
             for w in ws]
    ops.conv_pack_weight_multi(items)
    for w, wk, wd in items:
        wk1, wd1 = pack(ops, w.cpu(), dtype)
        assert torch.equal(wk, wk1) and torch.equal(wd, wd1), tuple(w.shape)
        same(wk, R.pack_rule(w.cpu())[0].to(dtype), "wk")
        same(wd, R.pack_rule(w.cpu())[1].to(dtype), "wd")


# ------------------------------------------------------------------------------------------------ asr_conv3x3_igemm
@pytest.mark.parametrize("case", R.IGEMM, ids=case_id)
def test_conv3x3_igemm_arm(ops, case):
    """Forward with bias + ReLU and / or the data gradient through wd with a mask (conv_reference.IGEMM_ARMS), equal to float64; under a
    hook also equal to what the dispatch launches with no hook set."""
    arm, shape, Cin, Cout, dtype = case.args
    spec = R.IGEMM_ARMS[arm]
    for mode in spec.modes:
        x, w, bias, mask, want = R.igemm_case(mode, *shape, Cin, Cout, dtype)
        wk, wd = pack(ops, w, dtype)
        kw = wk if mode == "fwd" else wd                    # (wd's tap order is pinned here: the reference is autograd)
        assert tuple(kw.shape) == (Cout, 9, Cin)
        xd = x.to(D, dtype)
        bd = bias.to(D) if bias is not None else None
        md = mask.to(D, dtype) if mask is not None else None
        with tuning(spec.tuning):
            y = ops.conv3x3(xd, kw, bd, Cout, relu=mode == "fwd", mask_src=md)
        same(y, want, "%s (%s)" % (case.pins, mode))
        if spec.tuning:
            assert torch.equal(y, ops.conv3x3(xd, kw, bd, Cout, relu=mode == "fwd", mask_src=md)), "hooked kernel vs the automatic one"


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_conv3x3_igemm_refuses_other_channel_counts(dtype):
    from asr_hip import lib as L
    for Cin, Cout in ((64, 32), (96, 64), (96, 128), (128, 192)):
        x = torch.zeros(1, 8, 16, Cin, device=D, dtype=dtype)
        wk = torch.zeros(Cout, 9, Cin, device=D, dtype=dtype)
        y = torch.full((1, 8, 16, Cout), 7.0, device=D, dtype=dtype)
        assert not L.call_or_none("asr_conv3x3_igemm", L.ptr(x), L.ptr(wk), None, None, L.ptr(y), 1, 8, 16, Cin, Cout, 0, L.dt(x), L.stream())
        assert bool((y == 7).all()), "a refused call must not write"


@pytest.mark.parametrize("shape", [R.ODD, R.WHOLE], ids=str)
def test_relu_bit_masks_equal_float64(ops, shape):
    """asr_conv3x3_igemm_bits: the 64 -> 128 forward that also writes its ReLU mask as bits (ws<64, 4, 128, 3>) and the 128 -> 128 data
    gradient that applies them (ws<128, 8, 128, 2>)."""
    x, w5, b5, _, y_want = R.igemm_case("fwd", *shape, 64, 128, BF16)
    got = ops.conv3x3_relu_bits(x.to(D, BF16), pack(ops, w5, BF16)[0], b5.to(D), 128)
    assert got is not None
    y, bits = got
    same(y, y_want, "forward with bits out")
    g, w7, _, _ = R.conv_data(*shape, 128, 128, 77)
    z = ops.conv3x3_masked_by_bits(g.to(D, BF16), pack(ops, w7, BF16)[1], None, 128, bits)
    assert z is not None
    same(z, R.conv_dgrad_ref(g, w7, y_want.float(), BF16), "data gradient masked by bits")


# ------------------------------------------------------------------------------------------------ pooled epilogues
def _pooled_want(B, H, W, Cin, Cout):
    x, w, bias, _, y = R.igemm_case("fwd", B, H, W, Cin, Cout, BF16, True)
    m, code = R.pool_rule(y.float())
    g = torch.Generator().manual_seed(H + W)
    dy = torch.randint(-3, 4, tuple(m.shape), generator=g).float()
    return x, w, bias, y, m, code, dy, R.pool_bwd_rule(code, dy, tuple(y.shape))


@pytest.mark.parametrize("case", R.POOLED_C64, ids=case_id)
def test_c64_pooled_epilogue_on_tied_maxima(ops, case):
    """asr_conv3x3_relu_pool / _pool_code (launch_t<16, 8, false, 3, true>) with and without y: the pool, the selection bytes (first maximum
    in scan order, 0 where the maximum is 0) and the gradient asr_maxpool_bwd_code routes with them, on outputs full of positive ties."""
    B, H, W = case.args
    x, w, bias, y_want, m, code, dy, dx_want = _pooled_want(B, H, W, 64, 64)
    xd, bd = x.to(D, BF16), bias.to(D)
    wk, _ = pack(ops, w, BF16)
    y, pool = ops.conv3x3_relu_pool(xd, wk, bd, 64)
    same(y, y_want, "y")
    same(pool, m.to(BF16), "pool")
    for keep_y in (True, False):
        y2, pool2, cd = ops.conv3x3_relu_pool_code(xd, wk, bd, 64, keep_y=keep_y)
        assert (y2 is None) == (not keep_y)
        if keep_y:
            same(y2, y_want, "y (codes)")
        same(pool2, m.to(BF16), "pool (codes, keep_y=%s)" % keep_y)
        same(cd, code, "selection bytes (keep_y=%s)" % keep_y)
        same(ops.maxpool_bwd_code(cd, dy.to(D, BF16), tuple(y_want.shape)), dx_want.to(BF16), "gradient through the codes")
    same(ops.maxpool_bwd(y, dy.to(D, BF16)), dx_want.to(BF16), "gradient through the activations")


@pytest.mark.parametrize("case", R.POOLED_TCF, ids=case_id)
def test_encoder_layout_pooled_epilogues_on_tied_maxima(ops, case):
    """asr_conv3x3_relu_pool_tcf_code / _codecl: pool (B, W/2, C H/2) and its selection bytes from conv_ws.hip (tile pairs, single tiles) and
    from the generic kernel's pooled epilogue."""
    B, H, W, Cin, switches = case.args
    x, w, bias, y_want, m, code, dy, dx_want = _pooled_want(B, H, W, Cin, 128)
    xd, bd = x.to(D, BF16), bias.to(D)
    wk, _ = pack(ops, w, BF16)
    with tuning(switches):
        got = ops.conv3x3_relu_pool_tcf_code(xd, wk, bd, 128)
        got_cl = ops.conv3x3_relu_pool_tcf_code(xd, wk, bd, 128, code_cl=True)
    assert got is not None
    same(got[0], R.to_tcf(m).to(BF16), case.pins)
    same(got[1], R.to_tcf(code), case.pins)
    assert (got_cl is not None) == (Cin == 128 and "WS128" not in switches)         # channel-last bytes: the weight-stationary kernel only
    if got_cl is not None:
        same(got_cl[0], R.to_tcf(m).to(BF16), "pool (channel-last codes)")
        same(got_cl[1], code.permute(0, 2, 1, 3).contiguous(), "channel-last codes")
    same(ops.maxpool_bwd_code(got[1], R.to_tcf(dy).to(D, BF16), tuple(y_want.shape), tcf=True), dx_want.to(BF16), "gradient through the codes")


# ------------------------------------------------------------------------------------------------ 3x3 weight gradients
WGRAD_KERNELS = ["fp32", "fp32_atomics", "bf16_dma", "bf16_atomics"]


@pytest.mark.parametrize("kernel", WGRAD_KERNELS)
@pytest.mark.parametrize("case", R.WGRAD, ids=case_id)
def test_conv3x3_wgrad_arm(ops, case, kernel):
    """conv3x3_wgrad_nhwc_kernel<float> with its workspace (fixed-order fold) and without (atomics), conv3x3_wgrad_dma_kernel (bf16 with a
    workspace) and conv3x3_wgrad_nhwc_kernel<bf16> (bf16 without: a direct call with a null workspace).  dW and db equal float64 on top
    of integer prior contents, a second call adds the same again, and partials + reduce equal the one call."""
    from asr_hip import lib as L
    B, H, W, Cin, Cout = case.args
    x, dy, dw0, db0, dw, db = R.wgrad_case(*case.args)
    dtype = F32 if kernel.startswith("fp32") else BF16
    xd, dyd = x.to(D, dtype), dy.to(D, dtype)

    def run(gw, gb):
        if kernel.endswith("atomics"):
            L.call("asr_conv3x3_wgrad_nhwc", L.ptr(xd), L.ptr(dyd), L.ptr(gw), L.ptr(gb), None, 0, B, H, W, Cin, Cout, L.dt(xd), L.stream())
        else:
            ops.conv3x3_wgrad_nhwc(xd, dyd, gw, gb)

    gw, gb = dw0.to(D), db0.to(D)
    for n in (1, 2):
        run(gw, gb)
        same(gw, dw0 + n * dw, "%s: dW after call %d" % (case.pins, n))
        same(gb, db0 + n * db, "%s: db after call %d" % (case.pins, n))
    if not kernel.endswith("atomics"):
        n_ws = L.load().asr_conv3x3_wgrad_workspace(B, H, W, Cin, Cout)
        ws = torch.empty(n_ws, device=D, dtype=F32)
        gw2, gb2 = dw0.to(D), db0.to(D)
        L.call("asr_conv3x3_wgrad_partials", L.ptr(xd), L.ptr(dyd), L.ptr(gb2), L.ptr(ws), n_ws, B, H, W, Cin, Cout, L.dt(xd), L.stream())
        same(gb2, db0 + db, "db is complete after the partials")
        same(gw2, dw0, "dW waits for the reduction")
        L.call("asr_conv3x3_wgrad_reduce", L.ptr(ws), L.ptr(gw2), B, H, W, Cin, Cout, L.stream())
        same(gw2, dw0 + dw, "partials + reduce")


# ------------------------------------------------------------------------------------------------ pool.hip
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("case", R.POOL, ids=case_id)
def test_maxpool_on_tied_maxima(ops, case, dtype):
    """asr_maxpool_fwd / _bwd / _fwd_code / _bwd_code in both layouts on integers in {0, 1, 2}: over half of the windows hold their positive
    maximum more than once.  One rule everywhere: the first maximum in scan order, nothing where the maximum is 0."""
    B, H, W, C = case.args
    y, dy, m, code, dx = R.pool_case(*case.args)
    yd, shape = y.to(D, dtype), tuple(y.shape)
    epc = 4 if dtype == F32 else 8
    for tcf in (False, True):
        lay = R.to_tcf if tcf else (lambda t: t)
        tag = "%s, %s" % (case.pins, "encoder layout" if tcf else "NHWC")
        dyd = lay(dy).to(D, dtype)
        same(ops.maxpool_fwd(yd, tcf=tcf), lay(m).to(dtype), tag)
        same(ops.maxpool_bwd(yd, dyd, tcf=tcf), dx.to(dtype), tag + ": backward from the activations")
        got = ops.maxpool_fwd_code(yd, tcf=tcf)
        assert (got is None) == (tcf and (H // 2) % epc != 0), tag                 # the code form in the encoder layout: whole 16-byte chunks
        if got is not None:
            same(got[0], lay(m).to(dtype), tag + ": pool beside the codes")
            same(got[1], lay(code), tag + ": codes")
        # backward from the RULE's codes: in the encoder layout this takes any H/2 (by element where a channel's values are no whole chunks)
        same(ops.maxpool_bwd_code(lay(code).to(D), dyd, shape, tcf=tcf), dx.to(dtype), tag + ": backward from the codes")


# ------------------------------------------------------------------------------------------------ level 0
@pytest.mark.parametrize("case", R.LEVEL0, ids=case_id)
def test_level0_equals_the_float64_chain(ops, case):
    """asr_vgg_level0_fwd / _wgrad / _dgrad against conv.0 -> ReLU -> bf16 -> conv.2 -> ReLU -> bf16 -> pool in float64 and its autograd --
    directly, not through the launch chain (which shares csrc/conv_c64_core.h with these kernels); without a hook the launch chain is held
    against the same numbers.  db2 is exact too on this data, whichever way it is summed; a second call doubles every gradient."""
    B, H, W, wsplit, ties = case.args
    (src, w0, b0, w2, b2, dp), ref = R.level0_case(B, H, W, ties)
    sd, w0d, b0d, b2d, dpd = src.to(D), w0.to(D), b0.to(D), b2.to(D), dp.to(D, BF16)
    wk, wd = pack(ops, w2, BF16)
    with tuning({} if wsplit else {"L0_WSPLIT": 0}):
        out = ops.vgg_level0_fwd(sd, w0d, b0d, wk, b2d)
        assert out is not None
        pool, code = out
        same(pool, ref.pool, "pool")
        same(code, ref.code, "selection bytes")
        dw2, db2 = torch.zeros(64, 64, 3, 3, device=D), torch.zeros(64, device=D)
        dw0, db0 = torch.zeros(64, 1, 3, 3, device=D), torch.zeros(64, device=D)
        for n in (1, 2):
            ops.vgg_level0_wgrad(sd, w0d, b0d, dpd, code, dw2, db2)
            ops.vgg_level0_dgrad(dpd, code, sd, w0d, b0d, wd, dw0, db0)
            for name, got, want in (("dW2", dw2, ref.dw2), ("db2", db2, ref.db2), ("dW0", dw0, ref.dw0), ("db0", db0, ref.db0)):
                same(got, n * want, "%s after call %d" % (name, n))
    if wsplit:          # the launch chain the level replaces, on the same data against the same float64 numbers
        y1 = ops.conv1_fwd(sd, w0d, b0d, BF16)
        same(y1, ref.y1.float().to(BF16), "conv.0")
        _, p2, c2 = ops.conv3x3_relu_pool_code(y1, wk, b2d, 64)
        same(p2, ref.pool, "chain: pool")
        same(c2, ref.code, "chain: selection bytes")
        dy2 = ops.maxpool_bwd_code(c2, dpd, (B, H, W, 64))
        same(dy2, ref.dy2.float().to(BF16), "chain: pooled gradient expanded")
        dy1 = ops.conv3x3(dy2, wd, None, 64, relu=False, mask_src=y1)
        same(dy1, ref.dy1.float().to(BF16), "chain: conv.2's data gradient")
        gw2, gb2 = torch.zeros(64, 64, 3, 3, device=D), torch.zeros(64, device=D)
        ops.conv3x3_wgrad_nhwc(y1, dy2, gw2, gb2)
        same(gw2, ref.dw2, "chain: dW2")
        same(gb2, ref.db2, "chain: db2")
        gw0, gb0 = torch.zeros(64, 1, 3, 3, device=D), torch.zeros(64, device=D)
        ops.conv1_wgrad(sd, dy1, gw0, gb0)
        same(gw0, ref.dw0, "chain: dW0")
        same(gb0, ref.db0, "chain: db0")
