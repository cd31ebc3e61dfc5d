"""tests/conv_reference.py checked on the CPU: the yardstick of tests/test_gpu_conv_arms.py must itself be right, and its data must be
able to see the defects those tests exist for.

  * every case of every table passes the exactness guard (it runs inside the references) and evaluates in fp32, in two different
    summation orders, to exactly the float64 reference -- so torch.equal on the GPU asks for nothing that depends on a kernel's order;
  * the explicit pooling rule (first maximum in scan order, nothing where the maximum is 0) is torch's float64 max_pool2d, forward and
    backward, on data where more than a third of the windows tie, odd heights and widths included;
  * the packed data-gradient weights (wd) used as forward weights give the autograd data gradient;
  * each deliberate defect, applied to the reference on a case's own data, breaks the equality.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_reference as R


def conv_fp32(x, wk, bias, per_tap):
    """fp32 convolution of NHWC x with packed weights wk (Cout, 9, Cin): one F.conv2d, or nine 1x1 convolutions of the shifted input
    accumulated from the last tap to the first with the bias added at the end."""
    x, wk = x.float(), wk.float()
    if not per_tap:
        return R.nhwc(F.conv2d(R.nchw(x), R.unpack_rule(wk), None if bias is None else bias.float(), padding=1))
    B, H, W, _ = x.shape
    xp = F.pad(R.nchw(x), (1, 1, 1, 1))
    acc = torch.zeros(B, wk.shape[0], H, W)
    for tap in reversed(range(9)):
        ky, kx = divmod(tap, 3)
        acc = acc + F.conv2d(xp[:, :, ky:ky + H, kx:kx + W], wk[:, tap, :, None, None].contiguous())
    if bias is not None:
        acc = acc + bias.float().view(1, -1, 1, 1)
    return R.nhwc(acc)


def wgrad_fp32(x, dy, reverse):
    """fp32 weight / bias gradient from NHWC x, dy: one autograd call over the batch, or image by image from the last to the first."""
    xs, ds = R.nchw(x).float(), R.nchw(dy).float()
    if not reverse:
        dw, db = R._weight_grad(xs.double(), ds.double())      # (shapes only)
        w = torch.zeros_like(dw, dtype=torch.float32, requires_grad=True)
        b = torch.zeros_like(db, dtype=torch.float32, requires_grad=True)
        F.conv2d(xs, w, b, padding=1).backward(ds)
        return w.grad, b.grad
    dw = db = None
    for i in reversed(range(xs.shape[0])):
        w = torch.zeros(ds.shape[1], xs.shape[1], 3, 3, requires_grad=True)
        b = torch.zeros(ds.shape[1], requires_grad=True)
        F.conv2d(xs[i:i + 1], w, b, padding=1).backward(ds[i:i + 1])
        dw = w.grad if dw is None else dw + w.grad
        db = b.grad if db is None else db + b.grad
    return dw, db


IGEMM_KEYS = sorted({(mode,) + c.args[1] + c.args[2:5] for c in R.IGEMM for mode in R.IGEMM_ARMS[c.args[0]].modes}, key=str)


@pytest.mark.parametrize("key", IGEMM_KEYS, ids=lambda k: "-".join(str(v).replace("torch.", "") for v in k))
def test_igemm_cases_are_exact_in_any_order(key):
    mode, B, H, W, Cin, Cout, dtype = key
    x, w, bias, mask, want = R.igemm_case(mode, B, H, W, Cin, Cout, dtype)          # (the guard runs in here)
    wk = R.pack_rule(w)[0 if mode == "fwd" else 1]                                 # the kernel's weights: wk forward, wd for the gradient
    assert tuple(wk.shape) == (Cout, 9, Cin) and tuple(want.shape) == (B, H, W, Cout) and want.dtype == dtype
    for per_tap in (False, True):
        y = conv_fp32(x, wk, bias, per_tap)
        y = y.clamp_min(0) if mode == "fwd" else y * (mask > 0)
        assert torch.equal(y.to(dtype), want), (mode, per_tap)


@pytest.mark.parametrize("case", R.POOLED_C64 + R.POOLED_TCF, ids=lambda c: c.id)
def test_pooled_cases_are_exact_and_tie_rich(case):
    B, H, W = case.args[:3]
    Cin, Cout = (64, 64) if len(case.args) == 3 else (case.args[3], 128)
    x, w, bias, _, want = R.igemm_case("fwd", B, H, W, Cin, Cout, R.BF16, True)
    wk = R.pack_rule(w)[0]
    for per_tap in (False, True):
        assert torch.equal(conv_fp32(x, wk, bias, per_tap).clamp_min(0).to(R.BF16), want)
    # the block-constant input repeats the convolution's output inside 3 of 4 windows away from the image border (where the zero padding
    # breaks the repetition along one axis) and about half of the maxima are positive: 3/8 expected inside, less at the 5 x 7 shape
    assert R.tied_fraction(want.float()) >= 0.2, R.tied_fraction(want.float())


@pytest.mark.parametrize("args", sorted({c.args for c in R.WGRAD}), ids=str)
def test_wgrad_cases_are_exact_in_any_order(args):
    x, dy, dw0, db0, dw, db = R.wgrad_case(*args)
    for reverse in (False, True):
        gw, gb = wgrad_fp32(x, dy, reverse)
        assert torch.equal(gw, dw) and torch.equal(gb, db), reverse
    assert torch.equal(dw0, dw0.round()) and torch.equal(db0, db0.round()) and float(dw0.abs().max()) <= 4


@pytest.mark.parametrize("args", sorted({c.args for c in R.CONV1_FWD + R.CONV1_WGRAD}), ids=str)
def test_conv1_cases_are_exact_in_any_order(args):
    B, H, W, C0 = args
    src, w, bias, dy, dw0, db0, dw, db = R.conv1_case(*args)
    for dtype in (R.F32, R.BF16):
        want = R.conv1_forward_ref(src, w, bias, dtype)
        for per_tap in (False, True):
            assert torch.equal(conv_fp32(R.nhwc(src), R.pack_rule(w)[0], bias, per_tap).clamp_min(0).to(dtype), want)
    for reverse in (False, True):
        gw, gb = wgrad_fp32(R.nhwc(src), dy, reverse)
        assert torch.equal(gw, dw) and torch.equal(gb, db), reverse


@pytest.mark.parametrize("shape", sorted({c.args[:3] + c.args[4:] for c in R.LEVEL0}), ids=str)
def test_level0_cases_are_exact_in_fp32(shape):
    (src, w0, b0, w2, b2, dp), ref = R.level0_case(*shape)                           # (the guards run in here)
    if shape[3]:        # src constant on 8 x 8 squares: conv.2's output repeats on their inner 4 x 4 pixels and along their edges
        assert R.tied_fraction(ref.y2.float()) >= 0.2, R.tied_fraction(ref.y2.float())
    assert float(ref.y1.max()) <= 18 and float(ref.dy1.abs().max()) <= 39            # integers: exact in bf16, rounded or not
    assert torch.equal(ref.dy1, ref.dy1.round())
    # the same chain in fp32, per-tap order, under the reference's selections
    y1 = conv_fp32(R.nhwc(src), R.pack_rule(w0)[0], b0, True).clamp_min(0)
    assert torch.equal(y1.double(), ref.y1)
    y2 = conv_fp32(y1, R.pack_rule(w2)[0], b2, True).clamp_min(0).to(R.BF16).float()
    assert torch.equal(y2.double(), ref.y2)
    pool, code = R.pool_rule(y2)
    assert torch.equal(pool.to(R.BF16), ref.pool) and torch.equal(code, ref.code)
    dy2 = R.pool_bwd_rule(code, dp, tuple(y2.shape))
    dy1 = conv_fp32(dy2, R.pack_rule(w2)[1], None, True) * (y1 > 0)
    assert torch.equal(dy1.double(), ref.dy1)
    for reverse in (False, True):
        gw2, gb2 = wgrad_fp32(y1, dy2, reverse)
        gw0, gb0 = wgrad_fp32(R.nhwc(src), dy1, reverse)
        assert torch.equal(gw2, ref.dw2) and torch.equal(gb2, ref.db2) and torch.equal(gw0, ref.dw0) and torch.equal(gb0, ref.db0)


@pytest.mark.parametrize("case", R.POOL, ids=lambda c: c.id)
def test_pool_rule_is_torchs_float64_max_pool(case):
    B, H, W, C = case.args
    y, dy, m, code, dx = R.pool_case(*case.args)
    assert R.tied_fraction(y) >= 1 / 3, R.tied_fraction(y)                           # measured 0.56 with {0, 1, 2}
    t = R.nchw(y).double().requires_grad_()
    p = F.max_pool2d(t, 2, stride=2)
    assert torch.equal(R.nhwc(p.detach()), m.double())
    p.backward(R.nchw(dy).double())
    want = R.nhwc(t.grad) * (y > 0)                                                  # nothing where the maximum is 0 (ReLU')
    assert torch.equal(dx.double(), want)
    assert torch.equal(code == 0, m == 0) and int(code.max()) == 4
    if H % 2:
        assert not dx[:, H - 1].any()
    if W % 2:
        assert not dx[:, :, W - 1].any()
    # the encoder layout is the view / transpose of the NCHW pool (transformer.py:74-76)
    B_, C_, H2, W2 = p.shape
    assert torch.equal(R.to_tcf(m).double(), p.detach().reshape(B_, C_ * H2, W2).transpose(1, 2))


def test_pack_rule_is_what_the_data_gradient_needs():
    """wd used as the forward weights of a convolution of dL/dy is the autograd data gradient: the tap flip and the channel transpose."""
    x, w, _, mask, want = R.igemm_case("dgrad", 2, 9, 17, 64, 128, R.F32)
    wk, wd = R.pack_rule(w)
    assert tuple(wk.shape) == (64, 9, 128) and tuple(wd.shape) == (128, 9, 64)
    assert torch.equal(wk[5, 7], w[5, :, 2, 1]) and torch.equal(wd[:, 8 - 7, 5], w[5, :, 2, 1])
    assert torch.equal(conv_fp32(x, wd, None, False) * (mask > 0), want)


# ------------------------------------------------------------------------------------------------ the data can see the defects
def test_defect_border_row_dropped_from_a_weight_gradient():
    for args in (R.ODD + (64, 64), R.BIG + (64, 64)):
        x, dy, _, _, dw, db = R.wgrad_case(*args)
        cut = dy.clone()
        cut[:, -1] = 0                                                               # the last image row never contributes
        gw, gb = wgrad_fp32(x, cut, False)
        assert not torch.equal(gw, dw) and not torch.equal(gb, db)
        cut = dy.clone()
        cut[-1, 7, 16] = 0                                                           # one pixel at a patch seam
        assert not torch.equal(wgrad_fp32(x, cut, False)[0], dw)


@pytest.mark.parametrize("key", [("fwd",) + R.ODD + (64, 64, R.BF16), ("fwd",) + R.ODD + (64, 128, R.BF16),
                                 ("dgrad",) + R.ODD + (128, 64, R.BF16), ("fwd",) + R.TINY + (64, 64, R.F32)], ids=str)
def test_defect_tap_transposed_or_bias_shifted(key):
    mode, B, H, W, Cin, Cout, dtype = key
    x, w, bias, mask, want = R.igemm_case(*key)
    wk = R.pack_rule(w)[0 if mode == "fwd" else 1]

    def run(wk_, bias_):
        y = conv_fp32(x, wk_, bias_, False)
        return (y.clamp_min(0) if mode == "fwd" else y * (mask > 0)).to(dtype)

    assert torch.equal(run(wk, bias), want)
    bad = wk.clone()
    if Cin == Cout:
        bad[:, 5] = wk[:, 5].t()                                                     # one tap's (Cout, Cin) block transposed
    else:
        bad[:, 1], bad[:, 3] = wk[:, 3], wk[:, 1]                                    # taps (0, 1) and (1, 0): the stencil transposed
    assert not torch.equal(run(bad, bias), want)
    if bias is not None:
        assert not torch.equal(run(wk, bias.roll(1)), want)                          # bias one channel off


@pytest.mark.parametrize("case", R.POOL, ids=lambda c: c.id)
def test_defect_last_maximum_or_all_tied_positions(case):
    y, dy, m, code, dx = R.pool_case(*case.args)
    m_last, code_last = R.pool_rule(y, pick="last")
    assert torch.equal(m_last, m) and not torch.equal(code_last, code)
    assert not torch.equal(R.pool_bwd_rule(code_last, dy, tuple(y.shape)), dx)
    assert not torch.equal(R.pool_bwd_all_ties(y, dy), dx)


def test_defects_show_on_the_pooled_convolution_and_level0_data():
    x, w, bias, _, want = R.igemm_case("fwd", *R.ODD, 64, 64, R.BF16, True)
    y = want.float()
    _, code = R.pool_rule(y)
    assert not torch.equal(R.pool_rule(y, pick="last")[1], code)
    (src, w0, b0, w2, b2, dp), ref = R.level0_case(*R.ODD)
    cut = ref.dy2.clone()
    cut[:, -2] = 0                                                                   # the last pooled image row (row 20 is not pooled)
    assert not torch.equal(wgrad_fp32(ref.y1.float(), cut.float(), False)[0], ref.dw2)
    assert not torch.equal(R.level0_ref(src, w0, b0.roll(1), w2, b2, dp).dw0, ref.dw0)


def test_the_guard_rejects_what_is_not_order_independent():
    x, w, bias, _ = R.conv_data(1, 5, 7, 64, 64, 1)
    with pytest.raises(AssertionError):
        R.conv_forward_ref(x * 4097, w * 65, bias, True, None)                       # sums of |terms| far above 2^24
    with pytest.raises(AssertionError):
        R.conv_forward_ref(x, w + 1.0 / 3, bias, True, None)                         # no power-of-two grid
    with pytest.raises(AssertionError):
        R.conv_wgrad_ref(x * 4097, x * 4097)                                             # odd factors: the grid stays 1
