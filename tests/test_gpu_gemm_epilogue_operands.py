"""The data-gradient GEMMs (csrc/gemm_big.hip gemm_big_nn_kernel, csrc/gemm_nn.hip gemm_nn_kernel) request the global operands of their
epilogue -- ReLU mask, `+=` base, O / O32 of the row-dot -- all together in front of the store loop (the ring forms: in their last K step;
the single-stage four-wave form: behind the staging of the accumulators), at addresses that are CLAMPED for the pieces past M or N, and
consume registers in the store loop.  What can go wrong is an operand taken from
the wrong piece, a clamped piece that is stored after all, and a ring whose counted waits no longer cover its own stages.  So, in the
manner of tests/test_gpu_gemm_exact.py (exact-integer data, bit equality with the float64 host product over the WHOLE output buffer):

  * the shapes are the smallest with a partial last row tile, a partial last column tile, ldc > N and a single K step (the prologue is the
    whole loop); K = 2048 on four stages walks the eight-wave ring's three-deep prologue;
  * the padding columns of the mask and of the destination (ldc > N) hold NaN: a piece that reads them and is stored, or a `+=` that takes
    its base from them, poisons an element the comparison sees; the destination's padding must come back bit for bit;
  * every case runs as plain, mask, `+=` and mask with `+=` (eight-wave; the four-wave cases are the three forms with an operand).

The four-wave kernel's ring is chosen by `t64 <= NN_RING and K >= 256`: the hook moves the first bound only, so at K = 64 and K = 192 no
hook reaches the ring.  Those two shapes therefore run on the single-stage form (the form the dispatch gives them), and the same (M, N, ldc)
run at K = 256 / 320 on both forms: ring (NN_RING = 1 << 20) and single-stage (NN_RING = 0).

Integer data cannot see WHICH product of the row-dot's fp32 sum is rounded (a choice -ffp-contract made by the shape of the surrounding code
until the kernels wrote it out): test_rowdot_o32_rounding_is_pinned holds delta against a step-by-step emulation on data that rounds."""
import pytest
import torch

from test_gpu_gemm_exact import BF, D, SENTINEL, _ints, _place, _premise, _run_rowdot, _same, _seed

pytestmark = pytest.mark.gpu

FORMS = {"plain": (0, 0), "mask": (1, 0), "acc": (0, 1), "mask-acc": (1, 1)}


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    return o


_products = {}


def _product(M, N, K):
    """operands and their float64 product, computed once per shape and shared by the forms (never modified)"""
    if (M, N, K) not in _products:
        g = torch.Generator().manual_seed(_seed("epilogue-operands %d %d %d" % (M, N, K)))
        dy, w = _ints(g, (M, K)), _ints(g, (K, N))
        mask, old = _ints(g, (M, N), -1, 1), _ints(g, (M, N), -8, 8)
        _products[(M, N, K)] = (dy, w, mask, old, dy @ w, float((dy.abs() @ w.abs()).max()) + 8)
    return _products[(M, N, K)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run(ops, M, N, K, ldc, form, hooks):
    from asr_hip import lib as L
    use_mask, acc = FORMS[form]
    dy, w, mask, old, prod, absprod = _product(M, N, K)
    ref = prod * (mask > 0) if use_mask else prod
    if acc:
        ref = old + ref
    name = "gemm_nn %s ldc=%d %s %s" % ((M, N, K), ldc, form, hooks)
    _premise(name, ref, absprod)
    nan = float("nan")
    pad = nan if ldc > N else SENTINEL
    dyd, wd = dy.to(BF).to(D), w.to(BF).to(D)
    md = _place(mask, ldc, 0, BF, nan)[1] if use_mask else None
    flat, Cd, img = _place(old if acc else torch.full((M, N), SENTINEL, dtype=torch.float64), ldc, 0, BF, pad)
    before = flat.cpu()
    try:
        for k, v in hooks.items():
            L.set_tuning(k, v)
        ops.gemm_nn(dyd, wd, out=Cd, accumulate=bool(acc), relu_mask=md)
        torch.cuda.synchronize()
    finally:
        for k in hooks:
            L.set_tuning(k, None)
    got = flat.cpu().view(M, ldc)
    _same(name, got[:, :N], ref.to(BF))
    if ldc > N:         # NaN padding: compared as bits (a NaN differs from itself)
        assert torch.equal(_bits(got[:, N:]), _bits(before.view(M, ldc)[:, N:])), "%s: the padding columns of C were written" % name


# ---- eight-wave kernel, forced (the shapes are far below the 150 blocks of the automatic rule)
BIG = {"130x136x64": (130, 136, 64, 136, {}), "257x120x192-ldc128": (257, 120, 192, 128, {}),
       "128x128x2048-ns4": (128, 128, 2048, 128, {"GEMM_BIG_NS": 4})}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("case", sorted(BIG))
def test_eight_wave_epilogue_operands(ops, case, form):
    M, N, K, ldc, hooks = BIG[case]
    _run(ops, M, N, K, ldc, form, dict(hooks, GEMM_BIG_NN=2))


@pytest.mark.parametrize("use_o32", [True, False], ids=["o32", "obf16"])
def test_eight_wave_rowdot_operands(ops, use_o32):
    """M = 200: the second row tile is partial, so its clamped pieces read row 199 of O and are neither stored nor summed"""
    from asr_hip import lib as L
    try:
        L.set_tuning("GEMM_BIG_NN", 2)
        _run_rowdot(ops, 200, 100, 128, 64, use_o32=use_o32, seed=_seed("epilogue-operands rowdot"))
    finally:
        L.set_tuning("GEMM_BIG_NN", None)


# ---- four-wave kernel: the two shapes at their own K (single-stage: no hook reaches the ring below K = 256), and at K >= 256 on both forms
FOUR = {"65x72x64-single": (65, 72, 64, 72, {}), "300x136x192-ldc144-single": (300, 136, 192, 144, {}),
        "65x72x256-ring": (65, 72, 256, 72, {"NN_RING": 1 << 20}), "65x72x256-single": (65, 72, 256, 72, {"NN_RING": 0}),
        "300x136x320-ldc144-ring": (300, 136, 320, 144, {"NN_RING": 1 << 20}), "300x136x320-ldc144-single": (300, 136, 320, 144, {"NN_RING": 0})}


@pytest.mark.parametrize("form", ["acc", "mask", "mask-acc"])
@pytest.mark.parametrize("case", sorted(FOUR))
def test_four_wave_epilogue_operands(ops, case, form):
    M, N, K, ldc, hooks = FOUR[case]
    _run(ops, M, N, K, ldc, form, dict(hooks, GEMM_BIG_NN=0))


@pytest.mark.parametrize("form", ["eight-wave", "four-wave-single", "four-wave-ring"])
def test_rowdot_o32_rounding_is_pinned(ops, form):
    """delta = rowsum(dO * O32) per head is sum_e fma(O32[e], dO[e], fl(O32[4 + e] * dO[4 + e])) over a lane's 8 columns (e = 0 .. 3, added in
    that order to 0), then the xor-4 / 2 / 1 tree over the head's 8 lanes.  WHICH of the two products is rounded is invisible to integer
    data, and the compiler chose it by the shape of the code around it until it was written out as an fma: here every step rounds.  dy is
    one-hot, so dO is a row of w; all values lie in [1, 2), where the float64 emulation of each fp32 step below is exact."""
    from asr_hip import lib as L
    M, T, N = 200, 100, 128
    K, hooks = {"eight-wave": (64, {"GEMM_BIG_NN": 2}), "four-wave-single": (64, {"GEMM_BIG_NN": 0}),
                "four-wave-ring": (256, {"GEMM_BIG_NN": 0, "NN_RING": 1 << 20})}[form]
    g = torch.Generator().manual_seed(_seed("epilogue-operands rounding"))
    w = (1 + torch.randint(0, 128, (K, N), generator=g).double() / 128).to(BF)                  # bf16 in [1, 2): 8 significant bits
    idx = torch.randint(0, K, (M,), generator=g)
    dy = torch.zeros(M, K, dtype=BF)
    dy[torch.arange(M), idx] = 1
    o32 = (1 + torch.rand(M, N, generator=g, dtype=torch.float64)).float()                      # fp32 in [1, 2): 24 significant bits
    dx = w[idx]                                                                                 # (M, N) bf16, exact
    x, o = dx.double().view(M, N // 8, 8), o32.double().view(M, N // 8, 8)
    lane = torch.zeros(M, N // 8, dtype=torch.float64)
    for e in range(4):
        t = (o[:, :, 4 + e] * x[:, :, 4 + e]).float().double()                                  # the rounded product
        lane = (lane + (o[:, :, e] * x[:, :, e] + t).float().double()).float().double()          # fma: one rounding; then the fp32 add
    a = lane.view(M, N // 64, 8)
    s4 = [(a[:, :, i] + a[:, :, i + 4]).float().double() for i in range(4)]
    s2 = [(s4[i] + s4[i + 2]).float().double() for i in range(2)]
    want = (s2[0] + s2[1]).float().view(M // T, T, N // 64).permute(0, 2, 1).contiguous()
    try:
        for k, v in hooks.items():
            L.set_tuning(k, v)
        got = ops.gemm_nn_rowdot(dy.to(D), w.to(D), o32.to(BF).to(D), o32.to(D), T)
        assert got is not None
        torch.cuda.synchronize()
    finally:
        for k in hooks:
            L.set_tuning(k, None)
    _same("rowdot rounding %s dx" % form, got[0].cpu(), dx)
    _same("rowdot rounding %s delta" % form, got[1].cpu().view(-1, T), want.view(-1, T))
