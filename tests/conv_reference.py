"""The yardstick of tests/test_gpu_conv_arms.py, tests/test_gpu_conv_ws.py and tests/test_conv_reference_host.py: exact-integer data for
the convolution front end (csrc/conv1.hip, conv1_wgrad_mfma.hip, conv_igemm.hip, conv_c64.hip, conv_ws.hip, conv_wgrad.hip,
conv_wgrad_dma.hip, conv_level0.hip, pool.hip; reference models/asr/transformer.py:42-53, 70-76 and their autograd), float64 references
of every operation, the max-pool selection rule written out, and the case tables the GPU tests and the host check both iterate.

Why equality: every operand is a small integer (biases: multiples of 0.5), so every product and every partial sum of an output lies on
one power-of-two grid; as long as the sum of the ABSOLUTE terms of an output stays below 2^24 grid steps, each partial sum is an fp32
number whichever order a kernel adds in, and the stored value is the float64 value (after ONE round-to-nearest-even where the kernel
stores bf16).  `guard` checks exactly that, in float64, inside every reference that feeds a torch.equal -- a case that is not
order-independent fails on the CPU, not on the GPU.  This module needs no GPU (only `packed` touches the device, when called)."""
import collections
import functools

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
LIMIT = float(2 ** 24)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the exactness guard
def grid_of(t):
    """The largest power of two (2^4 .. 2^-10) that every element of t is a multiple of."""
    t = t.double()
    for k in range(4, -11, -1):
        s = t / 2.0 ** k
        if torch.equal(s, s.round()):
            return 2.0 ** k
    raise AssertionError("operand is not on a power-of-two grid of at least 2^-10")


def guard(what, abs_sum, *grids):
    """abs_sum: float64 tensor, per output the sum of the absolute values of its terms; grids: the power-of-two grids its terms lie on
    (a product term: the product of its factors' grids).  Every partial sum, in any order, is then a multiple of the finest grid and
    smaller than 2^24 of its steps: an fp32 number."""
    g = min(grids)
    assert g >= 2.0 ** -20, what
    worst = float(abs_sum.max()) if abs_sum.numel() else 0.0
    assert worst / g < LIMIT, "%s: sum of |terms| %.0f on a grid of %g is not below 2^24 steps" % (what, worst, g)
    return worst


def store(t64, dtype):
    """The float64 value as the kernel stores it: exact in fp32 (guard), then one round-to-nearest-even for bf16."""
    return t64.float().to(dtype)


# ------------------------------------------------------------------------------------------------ weights as the kernels read them
def pack_rule(w):
    """(wk, wd) of asr_conv_pack_weight for a master weight w (Cout, Cin, 3, 3), on the CPU: wk (Cout, 9, Cin) with tap = ky * 3 + kx;
    wd (Cin, 9, Cout) with the taps flipped (8 - tap), the forward weights of the data gradient's convolution."""
    Cout, Cin = w.shape[:2]
    wk = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin).contiguous()
    wd = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9, Cout).contiguous()
    return wk, wd


def unpack_rule(wk):
    """The (Cout, Cin, 3, 3) weight whose forward packing is wk (Cout, 9, Cin)."""
    Cout, _, Cin = wk.shape
    return wk.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()


def packed(w, dtype=BF16):
    """(Cout, 9 taps, Cin) on the device: the layout asr_conv_pack_weight produces (tap = ky * 3 + kx)."""
    return pack_rule(w)[0].cuda().to(dtype)


# ------------------------------------------------------------------------------------------------ 3x3 convolutions
def conv_data(B, H, W, Cin, Cout, seed):
    """x (B, H, W, Cin) in {-3 .. 3}, w (Cout, Cin, 3, 3) in {-2 .. 2}, bias multiples of 0.5 in [-4, 4], mask (B, H, W, Cout) in {-1, 0, 1}."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, H, W, Cin), generator=g).float()
    w = torch.randint(-2, 3, (Cout, Cin, 3, 3), generator=g).float()
    bias = torch.randint(-8, 9, (Cout,), generator=g).float() * 0.5
    mask = torch.randint(-1, 2, (B, H, W, Cout), generator=g).float()
    return x, w, bias, mask


def conv_forward_ref(x, w, bias, relu, mask, dtype=BF16):
    """act(conv3x3_pad1(x; w) + bias) (* (mask > 0)) in float64, stored as `dtype`; x, mask NHWC."""
    xd, wd_ = nchw(x).double(), w.double()
    bd = bias.double() if bias is not None else None
    guard("conv forward", F.conv2d(xd.abs(), wd_.abs(), bd.abs() if bd is not None else None, padding=1),
          grid_of(x) * grid_of(w), grid_of(bias) if bias is not None else 1.0)
    y = F.conv2d(xd, wd_, bd, padding=1).permute(0, 2, 3, 1)
    if relu:
        y = y.clamp_min(0)
    if mask is not None:
        y = y * (mask > 0)
    return store(y, dtype)          # exact fp32 value -> ONE round-to-nearest-even, as the kernels' v_cvt_pk_bf16_f32


def _input_grad(g_nchw, w):
    x = torch.zeros(g_nchw.shape[0], w.shape[1], g_nchw.shape[2], g_nchw.shape[3], dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, padding=1).backward(g_nchw)
    return x.grad


def conv_dgrad_ref(g, w, mask, dtype=BF16):
    """The data gradient of y = conv3x3_pad1(x; w), w (Cout, Cin, 3, 3), for dL/dy = g (B, H, W, Cout), by float64 autograd, times
    (mask > 0) (the ReLU that produced x), stored as `dtype`: what asr_conv3x3_igemm computes from g and the packed wd."""
    gd, wd_ = nchw(g).double(), w.double()
    guard("conv data gradient", _input_grad(gd.abs(), wd_.abs()), grid_of(g) * grid_of(w))
    dx = _input_grad(gd, wd_).permute(0, 2, 3, 1)
    if mask is not None:
        dx = dx * (mask > 0)
    return store(dx, dtype)


def _weight_grad(x_nchw, dy_nchw):
    w = torch.zeros(dy_nchw.shape[1], x_nchw.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(dy_nchw.shape[1], dtype=torch.float64, requires_grad=True)
    F.conv2d(x_nchw, w, b, padding=1).backward(dy_nchw)
    return w.grad, b.grad


def conv_wgrad_ref(x, dy):
    """(dW (Cout, Cin, 3, 3), db (Cout)) fp32 of a 3x3 pad-1 convolution from NHWC x and dy, by float64 autograd."""
    xd, dd = nchw(x).double(), nchw(dy).double()
    aw, ab = _weight_grad(xd.abs(), dd.abs())
    # (the tests call twice on top of prior contents of at most 4: twice the increment must be exact as well)
    guard("conv weight gradient", 2 * aw + 4, grid_of(x) * grid_of(dy))
    guard("conv bias gradient", 2 * ab + 4, grid_of(dy))
    dw, db = _weight_grad(xd, dd)
    return dw.float(), db.float()


def wgrad_data(B, H, W, Cin, Cout, seed):
    """x (B, H, W, Cin) and dy (B, H, W, Cout) in {-3 .. 3}; prior contents dw0 in {-4 .. 4}, db0 in {-4 .. 4}."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, H, W, Cin), generator=g).float()
    dy = torch.randint(-3, 4, (B, H, W, Cout), generator=g).float()
    dw0 = torch.randint(-4, 5, (Cout, Cin, 3, 3), generator=g).float()
    db0 = torch.randint(-4, 5, (Cout,), generator=g).float()
    return x, dy, dw0, db0


def tie_rich_input(B, H, W, C, seed, block=4, lim=3):
    """An NHWC input in {-lim .. lim} that is constant on block x block pixel squares starting at ODD rows and columns.  block = 4: a 3x3
    convolution of it is the same on the inner 2 x 2 pixels of a square -- one whole pooling window -- and pairwise equal along the
    square's edges, so that most 2x2 windows of the convolution's output hold a tied maximum, about half of them positive.  block = 8:
    the same for two 3x3 convolutions in a row (level 0), whose output repeats on the inner 4 x 4 pixels."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-lim, lim + 1, (B, (H + 1) // block + 1, (W + 1) // block + 1, C), generator=g).float()
    hi = (torch.arange(H) + 1) // block
    wi = (torch.arange(W) + 1) // block
    return base[:, hi][:, :, wi].contiguous()


# ------------------------------------------------------------------------------------------------ 2x2/2 max-pool, the rule written out
def pool_windows(y):
    """(B, H/2, W/2, C, 4): the four positions of every 2x2 window of NHWC y in scan order (0,0), (0,1), (1,0), (1,1); floor mode."""
    H2, W2 = y.shape[1] // 2, y.shape[2] // 2
    y = y[:, :2 * H2, :2 * W2]
    return torch.stack([y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]], dim=-1)


def pool_rule(y, pick="first"):
    """(pool, code) (B, H/2, W/2, C) of NHWC y >= 0: the maximum, and 0 where it is 0, else 1 + k for the FIRST maximum at window position
    k in scan order.  pick = "last": the deliberate defect of tests/test_conv_reference_host.py."""
    win = pool_windows(y)
    m = win.max(dim=-1).values
    hit = (win == m.unsqueeze(-1)).to(torch.int64)
    k = hit.argmax(dim=-1) if pick == "first" else 3 - hit.flip(-1).argmax(dim=-1)
    code = torch.where(m > 0, k + 1, torch.zeros_like(k)).to(torch.uint8)
    return m, code


def pool_bwd_rule(code, dy, shape):
    """dx (B, H, W, C): dy routed to the window position its code names, zero elsewhere and in the row / column floor mode drops."""
    B, H, W, C = shape
    H2, W2 = H // 2, W // 2
    dx = torch.zeros(shape, dtype=dy.dtype)
    for k in range(4):
        dx[:, k // 2:2 * H2:2, k % 2:2 * W2:2] = dy * (code == k + 1)
    return dx


def pool_bwd_all_ties(y, dy):
    """The deliberate defect: the gradient goes to EVERY position that holds the (positive) maximum."""
    win = pool_windows(y)
    m = win.max(dim=-1).values
    B, H, W, C = y.shape
    dx = torch.zeros(y.shape, dtype=dy.dtype)
    for k in range(4):
        dx[:, k // 2:2 * (H // 2):2, k % 2:2 * (W // 2):2] = dy * ((win[..., k] == m) & (m > 0))
    return dx


def tied_fraction(y, positive=True):
    """Fraction of 2x2 windows whose maximum (positive ones only by default) is held by more than one position."""
    win = pool_windows(y)
    m = win.max(dim=-1).values
    tied = (win == m.unsqueeze(-1)).sum(dim=-1) > 1
    if positive:
        tied = tied & (m > 0)
    return float(tied.float().mean())


def to_tcf(t):
    """(B, H2, W2, C) -> the encoder layout (B, W2, C * H2) of transformer.py:74-76 (view / transpose of the NCHW pool)."""
    B, H2, W2, C = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, W2, C * H2).contiguous()


def pool_data(B, H, W, C, seed):
    """y (B, H, W, C) in {0, 1, 2} -- over half of the 2x2 windows hold their positive maximum more than once (tied_fraction) -- and a
    pooled gradient dy (B, H/2, W/2, C) in {-3 .. 3}; both exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, 3, (B, H, W, C), generator=g).float()
    dy = torch.randint(-3, 4, (B, H // 2, W // 2, C), generator=g).float()
    return y, dy


# ------------------------------------------------------------------------------------------------ conv.0 (one input channel)
def conv1_data(B, H, W, C0, seed):
    """src (B, 1, H, W) in {-3 .. 3}, w (C0, 1, 3, 3) in {-2 .. 2}, bias multiples of 0.5, dy (B, H, W, C0) in {-3 .. 3}, prior dw / db."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(-3, 4, (B, 1, H, W), generator=g).float()
    w = torch.randint(-2, 3, (C0, 1, 3, 3), generator=g).float()
    bias = torch.randint(-8, 9, (C0,), generator=g).float() * 0.5
    dy = torch.randint(-3, 4, (B, H, W, C0), generator=g).float()
    dw0 = torch.randint(-4, 5, (C0, 1, 3, 3), generator=g).float()
    db0 = torch.randint(-4, 5, (C0,), generator=g).float()
    return src, w, bias, dy, dw0, db0


def conv1_forward_ref(src, w, bias, dtype):
    """ReLU(conv.0(src) + bias), NHWC (asr_conv1_fwd applies the ReLU itself)."""
    return conv_forward_ref(nhwc(src), w, bias, True, None, dtype)


def conv1_wgrad_ref(src, dy):
    return conv_wgrad_ref(nhwc(src), dy)


# ------------------------------------------------------------------------------------------------ level 0: conv.0 -> conv.2 -> pool
def level0_data(B, H, W, seed, ties=False):
    """src {-2 .. 2}, w0 {-1 .. 1}, b0 {-1 .. 1}, w2 {-1 .. 1}, b2 multiples of 0.5 in [-4, 4], pooled gradient {-1, 0, 1}: conv.0's output
    is an integer of at most 18 and conv.2's data gradient an integer of at most 39 -- exact in bf16 whether or not a kernel rounds them.
    ties: src constant on 8 x 8 squares (tie_rich_input), same range -- conv.2's output then repeats inside most pooling windows."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(-2, 3, (B, 1, H, W), generator=g).float()
    if ties:
        src = nchw(tie_rich_input(B, H, W, 1, seed, block=8, lim=2))
    w0 = torch.randint(-1, 2, (64, 1, 3, 3), generator=g).float()
    b0 = torch.randint(-1, 2, (64,), generator=g).float()
    w2 = torch.randint(-1, 2, (64, 64, 3, 3), generator=g).float()
    b2 = torch.randint(-8, 9, (64,), generator=g).float() * 0.5
    dp = torch.randint(-1, 2, (B, H // 2, W // 2, 64), generator=g).float()
    return src, w0, b0, w2, b2, dp


Level0 = collections.namedtuple("Level0", "y1 y2 pool code dy2 dy1 dw2 db2 dw0 db0")


def level0_ref(src, w0, b0, w2, b2, dp):
    """The float64 chain conv.0 -> ReLU -> bf16 -> conv.2 -> ReLU -> bf16 -> pool and its autograd under the explicit selection rule.
    y1, y2, dy2, dy1 (conv.0's masked output gradient) NHWC; pool bf16, code uint8, the four gradients fp32."""
    B, _, H, W = src.shape
    s = src.double()
    w0r, b0r = w0.double().requires_grad_(), b0.double().requires_grad_()
    w2r, b2r = w2.double().requires_grad_(), b2.double().requires_grad_()
    a1 = F.conv2d(s, w0r, b0r, padding=1)
    a1.retain_grad()
    y1 = F.relu(a1)
    assert torch.equal(y1.detach(), y1.detach().float().to(BF16).double()), "conv.0's output must be exact in bf16"
    a2 = F.conv2d(y1, w2r, b2r, padding=1)
    y2 = F.relu(a2)
    y2q = y2 + (y2.detach().float().to(BF16).double() - y2.detach())              # bf16 storage of conv.2's output
    y2n = nhwc(y2q.detach())
    pool, code = pool_rule(y2n)
    dy2 = pool_bwd_rule(code, dp.double(), (B, H, W, 64))
    y2q.backward(nchw(dy2))
    dy1 = a1.grad                                                                 # conv.2's data gradient under conv.0's ReLU mask
    assert torch.equal(dy1, dy1.float().to(BF16).double()), "conv.2's data gradient must be exact in bf16"
    y1d, dy2n = y1.detach(), nchw(dy2)
    guard("level 0 conv.0", F.conv2d(s.abs(), w0.double().abs(), b0.double().abs(), padding=1), grid_of(src) * grid_of(w0), grid_of(b0))
    guard("level 0 conv.2", F.conv2d(y1d, w2.double().abs(), b2.double().abs(), padding=1), grid_of(w2), grid_of(b2))
    guard("level 0 conv.2 data gradient", _input_grad(dy2n.abs(), w2.double().abs()), grid_of(dp) * grid_of(w2))
    aw2, ab2 = _weight_grad(y1d, dy2n.abs())
    guard("level 0 dW2", 2 * aw2 + 4, grid_of(dp))              # (twice: the tests call a second time on top of the first)
    guard("level 0 db2", 2 * ab2 + 4, grid_of(dp))
    aw0, ab0 = _weight_grad(s.abs(), dy1.abs())
    guard("level 0 dW0", 2 * aw0 + 4, grid_of(src))
    guard("level 0 db0", 2 * ab0 + 4, 1.0)
    return Level0(nhwc(y1d), y2n, pool.float().to(BF16), code, dy2, nhwc(dy1), w2r.grad.float(), b2r.grad.float(), w0r.grad.float(),
                  b0r.grad.float())


# ------------------------------------------------------------------------------------------------ cached references (computed once)
@functools.lru_cache(maxsize=None)
def igemm_case(mode, B, H, W, Cin, Cout, dtype, ties=False):
    """Data and reference of one asr_conv3x3_igemm launch in the KERNEL's view (Cin channels in, Cout out):
    mode "fwd":   x, the master weight w (Cout, Cin, 3, 3) -> wk, bias, ReLU, no mask;
    mode "dgrad": the output gradient x (Cin channels) of a Cout -> Cin layer with master weight w (Cin, Cout, 3, 3) -> wd (the
                  kernel's weights), no bias, no ReLU, the mask of the layer's input.
    Returns (x, w, bias or None, mask or None, want), all on the CPU."""
    seed = 1000 * B + 10 * H + W + Cin + 2 * Cout + (5 if mode == "dgrad" else 0)
    if mode == "fwd":
        x, w, bias, _ = conv_data(B, H, W, Cin, Cout, seed)
        if ties:
            x = tie_rich_input(B, H, W, Cin, seed)
        return x, w, bias, None, conv_forward_ref(x, w, bias, True, None, dtype)
    x, wt, _, mask = conv_data(B, H, W, Cin, Cout, seed)
    w = wt.permute(1, 0, 2, 3).contiguous()                  # the layer's master weight: (its Cout = Cin here, its Cin = Cout here)
    return x, w, None, mask, conv_dgrad_ref(x, w, mask, dtype)


@functools.lru_cache(maxsize=None)
def wgrad_case(B, H, W, Cin, Cout):
    x, dy, dw0, db0 = wgrad_data(B, H, W, Cin, Cout, 100 * B + H + W + Cin + 3 * Cout)
    return (x, dy, dw0, db0) + conv_wgrad_ref(x, dy)


@functools.lru_cache(maxsize=None)
def conv1_case(B, H, W, C0):
    src, w, bias, dy, dw0, db0 = conv1_data(B, H, W, C0, 10 * B + H + W + C0)
    return (src, w, bias, dy, dw0, db0) + conv1_wgrad_ref(src, dy)


@functools.lru_cache(maxsize=None)
def pool_case(B, H, W, C):
    """y, dy, and under the explicit rule: pool, code (B, H/2, W/2, C) and dx (B, H, W, C)."""
    y, dy = pool_data(B, H, W, C, 7 * H + W + C)
    m, code = pool_rule(y)
    return y, dy, m, code, pool_bwd_rule(code, dy, tuple(y.shape))


@functools.lru_cache(maxsize=None)
def level0_case(B, H, W, ties=False):
    d = level0_data(B, H, W, 13 * H + W + B, ties)
    return d, level0_ref(*d)


# ------------------------------------------------------------------------------------------------ the case tables
# Shapes (B, H, W): the smallest that still hold each property against the tile geometries 8 x 16 (wgrad, level 0, c64 shape 0),
# 16 x 16 and 8 x 32 (c64 shapes 1 and 2), 16 x 16 / 8 x 16 (generic bf16 / fp32), 4 x 16 (weight-stationary).
TINY = (1, 5, 7)            # smaller than every tile
EDGE = (2, 9, 17)           # one row and one column past a tile edge
ODD = (2, 21, 37)           # odd, several border tiles
WHOLE = (1, 16, 32)         # whole tiles only
BIG = (3, 161, 232)         # more tiles than a persistent launch has workgroups (945 / 495 / 504 c64 tiles against 512 / 256 / 256 slots):
                            # several rounds of the pipelines and the tail; the benchmark's odd 161 rows
SMALL = (TINY, EDGE, ODD, WHOLE)

Case = collections.namedtuple("Case", "id pins args")


def _ids(cases):
    return [c.id for c in cases]


# asr_conv1_fwd: args (B, H, W, C0)
CONV1_FWD = [
    Case("full_w16", "W % 4 == 0: the FULL arm (no column bound checks)", (2, 9, 16, 64)),
    Case("ragged_w37", "W % 4 != 0: the bounded arm, odd rows", (2, 21, 37, 64)),
    Case("tiny_c32", "smaller than a row of threads, C0 = 32", (1, 5, 7, 32)),
    Case("rowloop", "B * H = 8372 > 8192 blocks: the block-stride row loop", (52, 161, 16, 64)),
    Case("rowloop_ragged", "the row loop on the bounded arm", (52, 161, 7, 64)),
]
# asr_conv1_wgrad: args (B, H, W, C0); C0 = 64 in bf16 is the MFMA kernel, anything else conv1_wgrad_kernel<T>
CONV1_WGRAD = [
    Case("tiny", "smaller than a tile", (1, 5, 7, 64)),
    Case("edge", "one row / column past a tile edge", (2, 9, 17, 64)),
    Case("odd", "odd sizes, border tiles", (2, 21, 37, 64)),
    Case("odd_c32", "C0 = 32: conv1_wgrad_kernel<bf16> in bf16", (2, 21, 37, 32)),
    Case("rowloop", "B * H = 1127 > 1024 blocks: the block-stride row loop", (7, 161, 24, 64)),
    Case("rowloop_c32", "the row loop of conv1_wgrad_kernel<bf16>", (7, 161, 24, 32)),
    Case("big", "more tiles than the MFMA kernel's persistent workgroups", BIG + (64,)),
]

# asr_conv3x3_igemm and its relatives: args (arm, shape, Cin, Cout, dtype, tuning), the kernel's view of the channels; every case runs
# the forward form (bias + ReLU) and the data-gradient form (wd, mask) unless the arm has only one.
IgemmArm = collections.namedtuple("IgemmArm", "modes tuning")
# An arm with a hook is also held against the kernel the dispatch takes with no hook set (its cases carry "hooked" in their ids, so that
# `-k "not hooked"` is the run that shows what the automatic dispatch reaches).
IGEMM_ARMS = {
    # bf16 64 -> 64: conv3x3_c64_kernel, unmasked launch_t<.., false, 3> forward and masked launch_t<.., true, ..> data gradient
    "c64_s0": IgemmArm(("fwd", "dgrad"), {}),
    "c64_s1": IgemmArm(("fwd", "dgrad"), {"C64_SHAPE": 1}),       # 16 x 16 tiles, 8 waves
    "c64_s2": IgemmArm(("fwd", "dgrad"), {"C64_SHAPE": 2}),       # 8 x 32 tiles, 8 waves
    # bf16 64 -> 128 without a mask: one pass on conv_ws.hip (default) and the two c64 passes it replaces (WS64 = 0)
    "ws64": IgemmArm(("fwd",), {}),
    "c64_two_pass": IgemmArm(("fwd",), {"WS64": 0}),
    # bf16, 128 input channels: conv_ws.hip (default) and the generic kernel it replaces (WS128 = 0)
    "ws128": IgemmArm(("fwd", "dgrad"), {}),
    "generic_ws128_off": IgemmArm(("fwd", "dgrad"), {"WS128": 0}),
    # the generic kernel with no hook: bf16 64 -> 128 WITH a mask (neither conv_ws.hip nor the two passes take a mask), Cin = 192, fp32
    "generic": IgemmArm(("fwd", "dgrad"), {}),
    "generic_masked_only": IgemmArm(("dgrad",), {}),
}


def _igemm_cases():
    out = []
    for s in (0, 1, 2):
        arm = "c64_s%d" % s
        for shape in SMALL:
            out.append(Case("%s-%dx%dx%d" % ((arm,) + shape), "c64 tile shape %d at %s" % (s, shape), (arm, shape, 64, 64, BF16)))
        out.append(Case("%s-big" % arm, "c64 tile shape %d: more tiles than workgroups, pipeline rounds and the tail" % s,
                        (arm, BIG, 64, 64, BF16)))
    for shape in SMALL:
        out.append(Case("c64_two_pass-%dx%dx%d" % shape, "64 -> 128 as two c64 passes (ypix = 256) against the one-pass form",
                        ("c64_two_pass", shape, 64, 128, BF16)))
    out.append(Case("c64_two_pass-big", "the two passes with more tiles than workgroups", ("c64_two_pass", BIG, 64, 128, BF16)))
    out.append(Case("ws64-odd", "64 -> 128 in one weight-stationary pass (ws<64, 4, 128>)", ("ws64", ODD, 64, 128, BF16)))
    for co in (64, 128):
        out.append(Case("ws128-odd-co%d" % co, "128 -> %d weight-stationary, plain and masked" % co, ("ws128", ODD, 128, co, BF16)))
        out.append(Case("generic_bf16-128to%d" % co, "conv3x3_igemm_kernel<bf16, %d> with 128 input channels under WS128 = 0" % co,
                        ("generic_ws128_off", ODD, 128, co, BF16)))
    out.append(Case("generic_bf16-128to64-tiny", "the same below one 16 x 16 tile", ("generic_ws128_off", TINY, 128, 64, BF16)))
    out.append(Case("generic_bf16-64to128-masked", "bf16 64 -> 128 with a mask: the generic kernel with no hook set",
                    ("generic_masked_only", ODD, 64, 128, BF16)))
    out.append(Case("generic_bf16-64to128-masked-edge", "the same one row / column past a 16 x 16 tile",
                    ("generic_masked_only", (2, 17, 17), 64, 128, BF16)))
    for co in (64, 128):
        out.append(Case("generic_bf16-192to%d" % co, "Cin = 192: three 64-channel slices per tap, no special kernel", ("generic", ODD, 192, co, BF16)))
    for ci in (64, 128):
        for co in (64, 128):
            out.append(Case("generic_fp32-%dto%d" % (ci, co), "fp32: 8 x 16 tiles of the generic kernel", ("generic", ODD, ci, co, F32)))
    out.append(Case("generic_fp32-64to64-tiny", "fp32 below one tile", ("generic", TINY, 64, 64, F32)))
    out.append(Case("generic_fp32-64to128-edge", "fp32 one row / column past a tile", ("generic", EDGE, 64, 128, F32)))
    out.append(Case("generic_fp32-128to64-whole", "fp32 whole tiles only", ("generic", WHOLE, 128, 64, F32)))
    return [c._replace(id=c.id + "-hooked") if IGEMM_ARMS[c.args[0]].tuning else c for c in out]


IGEMM = _igemm_cases()

# the pooled c64 epilogue (asr_conv3x3_relu_pool_code, bf16 64 -> 64) on tie-rich inputs: args (B, H, W)
POOLED_C64 = [Case("%dx%dx%d" % s, "pooled epilogue at %s" % (s,), s) for s in (TINY, EDGE, ODD, WHOLE)] + [
    Case("big", "pooled epilogue, more tiles than workgroups", BIG)]
# the pooled encoder-layout epilogues (asr_conv3x3_relu_pool_tcf_code / _codecl, bf16 -> 128): args (B, H, W, Cin, tuning)
POOLED_TCF = [
    Case("ws_pair", "H % 16 == 0: vertical tile pairs of conv_ws.hip (EP = 2)", (2, 16, 32, 128, {})),
    Case("ws_single", "H % 16 == 8: single tiles (EP = 1)", (2, 24, 16, 128, {})),
    Case("ws_single_hooked", "single tiles at H % 16 == 0 under WS_PAIR = 0", (1, 16, 48, 128, {"WS_PAIR": 0})),
    Case("generic_cin128_hooked", "the generic kernel's pooled epilogue (PT) under WS128 = 0", (2, 16, 32, 128, {"WS128": 0})),
    Case("generic_cin64", "64 -> 128: the generic kernel's pooled epilogue with no hook", (2, 32, 16, 64, {})),
]

# asr_conv3x3_wgrad_nhwc / _partials / _reduce: args (B, H, W, Cin, Cout); each runs as fp32, bf16 with a workspace (LDS-DMA kernel) and
# bf16 without one (conv3x3_wgrad_nhwc_kernel<bf16>, atomics)
WGRAD = [Case("64to64-%dx%dx%d" % s, "one dW block at %s" % (s,), s + (64, 64)) for s in SMALL] + [
    Case("64to128-odd", "two dW blocks along Cout", ODD + (64, 128)),
    Case("128to64-odd", "two dW blocks along Cin", ODD + (128, 64)),
    Case("128to128-odd", "four dW blocks", ODD + (128, 128)),
    Case("192to64-edge", "three dW blocks along Cin", EDGE + (192, 64)),
    Case("64to64-big", "several patches per workgroup on every workgroup, 161 rows: the border row of issue 2", BIG + (64, 64)),
]

# pool.hip: args (B, H, W, C)
POOL = [
    Case("scalar_odd_h", "H/2 = 10: the scalar tcf kernels in both types; odd H: the edges kernel", (2, 21, 38, 64)),
    Case("vec", "H/2 = 8: the vector tcf kernels in both types", (2, 16, 12, 64)),
    Case("odd_both", "odd H and W: last row and column get zero gradient; H/2 = 4: vector in fp32, scalar in bf16", (1, 9, 7, 64)),
    Case("mixed_h20", "H/2 = 20: vector in fp32, scalar in bf16; 128 channels", (2, 40, 16, 128)),
    Case("lds_grant", "H/2 = 96: 49 536 B of LDS (62 208 B with codes), above the 48 KB a kernel has without a grant", (1, 192, 4, 128)),
]

# level 0: args (B, H, W, L0_WSPLIT, tie-rich src)
LEVEL0 = [Case("%dx%dx%d-wsplit%d%s" % (s + (ws, "" if ws else "-hooked")), "level 0 at %s, L0_WSPLIT = %d" % (s, ws), s + (ws, False))
          for s in SMALL for ws in (1, 0)] + [
    Case("big-wsplit1", "level 0 with more tiles than workgroups, odd 161 rows", BIG + (1, False)),
    Case("ties-2x21x37-wsplit1", "positive tied maxima in level 0's pooled epilogue, odd sizes", ODD + (1, True)),
    Case("ties-2x32x48-wsplit1", "positive tied maxima, whole tiles", (2, 32, 48, 1, True)),
    Case("ties-2x21x37-wsplit0-hooked", "positive tied maxima under L0_WSPLIT = 0", ODD + (0, True))]
