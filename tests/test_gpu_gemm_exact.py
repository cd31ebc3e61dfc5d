"""Every GEMM entry (csrc/gemm_nt.hip, gemm_nn.hip, gemm_tn.hip, gemm_big.hip) on data for which the answer has no rounding to hide
behind: BIT equality against a float64 torch-CPU reference, at the shapes that sit on either side of every threshold of the dispatch.

tests/test_gpu_ops.py bounds the largest error by a fraction of max|ref|; a kernel that drops one 16-byte chunk of a long contraction
on one tile edge, reads a bias one column off on a partial tile or adds one split's partial sum twice stays under such a bound.  Here

  * operands are seeded random INTEGERS in [-3, 3] (stored in the kernel's input type: exact in bf16), bias values are multiples of
    1/4, alpha is 1, 1/2 or 1/4, and what an accumulating call finds in its output are integers;
  * so every partial sum is a multiple of 1/16 far below 2^24: fp32 accumulation, MFMA accumulation, split-K atomics and workspace
    folds are exact IN ANY ORDER, the fp32 result is the exact result, and a bf16 result is one round-to-nearest-even of it
    (csrc/common.h f32_to_bf16 is the hardware conversion) -- `ref.to(torch.bfloat16)`; `+=` into bf16 is RNE(old + v), the sum exact;
  * the premise is asserted on the CPU before anything is launched (`_premise`): the float64 reference survives a round trip through
    fp32, and both max|ref| and the largest entry of |A| |B|^T are below 2^24;
  * every comparison is `torch.equal` over the WHOLE output buffer: the padding columns of a strided output and the element in front
    of an offset one hold a sentinel that must survive.  A mismatch reports the number of differing elements and the first (row, col).

Each `*_auto` test runs with no tuning hook set: it pins the kernel the dispatch chooses at that shape (tools/kernel_coverage.py turns a
kernel trace of `-k auto` into the list of kernels launched).  Each `*_hooked` test runs the same data twice, automatic and with a
hook (asr_hip.lib.set_tuning) forcing the other arm, and requires both to equal the reference and each other.

asr_gemm_nt_fp8 is not covered here: whether asr_quant_fp8's row scale is exact on integer rows was not established.
"""
import ctypes
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

D = "cuda:0"
F32, BF = torch.float32, torch.bfloat16
COMBOS = {"f32": (F32, F32), "bf16": (BF, BF), "bf16f32": (BF, F32)}
SENTINEL = -640.0          # exact in bf16; no integer result of these cases comes near it by construction of the comparison (it sits in padding only)
LIMIT = float(2 ** 24)


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    return o


def _ints(g, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _quarters(g, n):
    return torch.randint(-8, 9, (n,), generator=g).double() / 4.0


def _premise(name, ref, absprod):
    """The exactness condition of the module docstring, on the CPU: a case that fails it is a bug in this file."""
    assert ref.dtype == torch.float64
    assert torch.equal(ref.float().double(), ref), "%s: the reference is not an fp32 number" % name
    assert float(ref.abs().max()) < LIMIT and float(absprod) < LIMIT, "%s: a partial sum may leave fp32's exact range" % name
    assert float(ref.abs().max()) > 0, "%s: zero reference, nothing compared" % name


def _same(name, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    g2, w2 = (t.reshape(t.shape[0], -1) if t.dim() >= 2 else t.reshape(1, -1) for t in (got.float(), want.float()))
    bad = g2 != w2                                   # (a NaN differs from everything, itself included)
    r, c = bad.nonzero()[0].tolist()
    raise AssertionError("%s: %d of %d elements differ, first at (row, col) (%d, %d): got %r, want %r" % (
        name, int(bad.sum()), bad.numel(), r, c, g2[r, c].item(), w2[r, c].item()))


def _place(vals, ld, off, dtype, pad):
    """vals (R, C) float64 on the CPU -> (flat device buffer, its (R, C) view with row stride ld starting `off` elements in, the CPU
    image of the buffer in float64).  Everything outside the view's elements holds `pad`."""
    R, C = vals.shape
    img = torch.full((off + R * ld,), float(pad), dtype=torch.float64)
    img[off:].view(R, ld)[:, :C] = vals
    flat = img.to(dtype).to(D)
    return flat, flat[off:].view(R, ld)[:, :C], img


def _auto_and_hooked(run, hooks):
    """run() -> {name: CPU tensor}, already compared with the reference; once with no hook, once with `hooks`: the same bits."""
    from asr_hip import lib as L
    a = run()
    try:
        for k, v in hooks.items():
            L.set_tuning(k, v)
        b = run()
    finally:
        for k in hooks:
            L.set_tuning(k, None)
    for k in a:
        _same("hooked %s vs automatic: %s" % (hooks, k), b[k], a[k])


def _seed(name):
    return zlib.crc32(name.encode())


# ================================================================================================ asr_gemm_nt
def nt(combo, M, N, K, **kw):
    return dict(combo=combo, M=M, N=N, K=K, **kw)


def _run_nt(ops, c, seed):
    """One asr_gemm_nt call of case c (see NT_CASES for the keys) -> {"C": the whole output buffer}, compared with the reference."""
    tin, tout = COMBOS[c["combo"]]
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldb, ldc = c.get("lda", K), c.get("ldb", K), c.get("ldc", N)
    g = torch.Generator().manual_seed(seed)
    A, B = _ints(g, (M, K)), _ints(g, (N, K))
    _, Ad, _ = _place(A, lda, c.get("offA", 0), tin, 3.0)          # padding of an operand: a non-zero the kernel must not contract
    _, Bd, _ = _place(B, ldb, c.get("offB", 0), tin, 3.0)
    alpha = c.get("alpha", 1.0)
    ref = alpha * (A @ B.t())
    bias = None
    if c.get("bias"):
        bias = _quarters(g, N)
        ref = ref + bias
    if c.get("relu"):
        ref = ref.clamp_min(0.0)
    mask = None
    if c.get("mask"):
        mask = _ints(g, (M, N), -1, 1)
        ref = ref * (mask > 0)
        _, mask, _ = _place(mask, ldc, 0, tin, 1.0)
    acc = bool(c.get("acc"))
    old = _ints(g, (M, N), -8, 8) if acc else None
    if acc:
        ref = old + ref
    name = "gemm_nt %s" % c
    _premise(name, ref, (A.abs() @ B.abs().t()).max() + 8)
    offC = c.get("offC", 0)
    flat, Cd, img = _place(old if acc else torch.full((M, N), SENTINEL, dtype=torch.float64), ldc, offC, tout, SENTINEL)
    ops.gemm_nt(Ad, Bd, out=Cd, bias=None if bias is None else bias.float().to(D), relu=bool(c.get("relu")), accumulate=acc, alpha=alpha,
                splits=c.get("splits", 1), relu_mask=mask)
    torch.cuda.synchronize()
    img[offC:].view(M, ldc)[:, :N] = ref
    want = img.to(tout)
    got = flat.cpu()
    rows = (want.numel() - offC) // ldc
    _same(name, got[offC:].view(rows, ldc), want[offC:].view(rows, ldc))
    _same(name + " (in front of C)", got[:offC].view(1, -1), want[:offC].view(1, -1))
    return {"C": got}


NT_CASES = {}


def _nt_add(name, case, hooks=None):
    assert name not in NT_CASES
    NT_CASES[name] = (case, hooks)


for _cb in COMBOS:
    _bf = _cb != "f32"
    # ---- the generic tile kernel (dispatch_tile), reached by K % bk != 0, lda % epc != 0 and an operand one element off alignment
    _nt_add("tile64-kragged-%s" % _cb, nt(_cb, 63, 65, 40, bias=1, relu=1))
    _nt_add("tile128-lda-odd-%s" % _cb, nt(_cb, 65, 65, 72, lda=73, alpha=0.5, acc=1))
    _nt_add("tile128x64-offA-%s" % _cb, nt(_cb, 6141, 512, 64, offA=1, bias=1))
    _nt_add("tile128-many-offB-%s" % _cb, nt(_cb, 6144, 1021, 24, offB=1, mask=1, ldc=1024))
    # ---- four-wave fast path, 64 x 64 blocks: M and N of 1, 63, 64, 65, 128 k + 1, 256 k + 1
    for _m, _n in ((1, 1), (63, 65), (64, 64), (65, 63), (129, 257), (257, 129)):
        _nt_add("fast64-%dx%d-%s" % (_m, _n, _cb), nt(_cb, _m, _n, 128, bias=1), {"GEMM_TILE": 0} if (_m, _n) == (129, 257) else None)
    if _bf:
        _nt_add("fast64-ring-65x63-%s" % _cb, nt(_cb, 65, 63, 256, bias=1, relu=1), {"NT_RING": 0})
        _nt_add("fast64-ring-129x257-%s" % _cb, nt(_cb, 129, 257, 320, alpha=0.25), {"GEMM_TILE": 1})
    # ---- epilogues of the fast path (200 x 136 over K = 192: partial blocks both ways)
    _nt_add("fast64-bias-relu-%s" % _cb, nt(_cb, 200, 136, 192, bias=1, relu=1, alpha=0.5))
    _nt_add("fast64-mask-%s" % _cb, nt(_cb, 200, 136, 192, mask=1, bias=1))
    _nt_add("fast64-acc-%s" % _cb, nt(_cb, 200, 136, 192, acc=1, alpha=0.25, bias=1))
    _nt_add("fast64-ldc-chunks-%s" % _cb, nt(_cb, 200, 136, 192, ldc=144, bias=1))
    _nt_add("fast64-ldc-odd-%s" % _cb, nt(_cb, 200, 136, 192, ldc=137, bias=1, relu=1))
    _nt_add("fast64-n70-%s" % _cb, nt(_cb, 200, 70, 192, bias=1), {"GEMM_TILE": 1})
    _nt_add("fast64-offC-%s" % _cb, nt(_cb, 200, 136, 192, offC=1, ldc=136, bias=1), {"GEMM_TILE": 0})
# ---- the ring cut-off NT_RING (512 blocks, K >= 256).  An eight-wave-eligible bf16 call of >= 512 blocks has t128 >= 128 and never gets
# here: the ring's edge is reached by calls the eight-wave path refuses (N % 4 != 0 with fp32 output; a ReLU mask; += into bf16)
_nt_add("ring-512-k256-bf16f32", nt("bf16f32", 32768, 63, 256, bias=1), {"NT_RING": 0})
_nt_add("ring-513-k256-bf16f32", nt("bf16f32", 32769, 63, 256, bias=1), {"NT_RING": 1 << 20})
_nt_add("ring-512-k192-bf16f32", nt("bf16f32", 32768, 63, 192, bias=1))
_nt_add("ring-512-k256-mask-bf16", nt("bf16", 32768, 64, 256, mask=1), {"NT_RING": 0})
_nt_add("ring-513-k256-mask-bf16", nt("bf16", 32769, 64, 256, mask=1), {"NT_RING": 1 << 20})
_nt_add("ring-512-k192-acc-bf16", nt("bf16", 32768, 64, 192, acc=1))
# ---- fast 128 x 64 from t64 = 2400 on (output as wide as the input); 2399 blocks stay 64 x 64
_nt_add("fast128x64-t2400-f32", nt("f32", 153595, 64, 32, bias=1), {"GEMM_TILE": 2})
_nt_add("fast64-t2399-f32", nt("f32", 153536, 64, 32, bias=1), {"GEMM_TILE": 1})
_nt_add("fast128x64-t2400-mask-bf16", nt("bf16", 153595, 64, 64, mask=1, bias=1), {"GEMM_TILE": 2})
_nt_add("fast64-t2399-mask-bf16", nt("bf16", 153536, 64, 64, mask=1, bias=1), {"GEMM_TILE": 1})
_nt_add("fast128x64-t2400-wide-f32", nt("f32", 6400, 1533, 64, bias=1, relu=1, ldc=1536))
# ---- eight-wave blocks (csrc/gemm_big.hip): kBigMin = 128 blocks of 128 x 128, 150 from K = 2048 on
_nt_add("big128-t127-bf16", nt("bf16", 16256, 128, 64, bias=1, relu=1), {"GEMM_BIG": 128})
_nt_add("big128-ns2-t128-bf16", nt("bf16", 16257, 128, 64, bias=1, relu=1), {"GEMM_BIG": 0})
_nt_add("big128-ns3-t128-bf16f32", nt("bf16f32", 16257, 128, 64, bias=1, alpha=0.5, acc=1), {"GEMM_BIG": 0})
_nt_add("big128-t149-k2048-bf16", nt("bf16", 19072, 128, 2048, bias=1), {"GEMM_BIG": 128})
_nt_add("big128-ns4-t150-k2048-bf16", nt("bf16", 19073, 128, 2048, bias=1), {"GEMM_BIG_NS": 2})
_nt_add("big128-ns4-t150-k2048-relu-bf16", nt("bf16", 19073, 120, 2048, relu=1, alpha=0.25, ldc=128), {"GEMM_BIG_NS": 3})
_nt_add("big128-m129-bf16", nt("bf16", 129, 8192, 64, bias=1), {"GEMM_BIG": 256})
_nt_add("big256-m130-n4364-bf16f32", nt("bf16f32", 130, 4364, 64, bias=1), {"GEMM_BIG": 128})
_nt_add("big256-m513-n2052-bf16f32", nt("bf16f32", 513, 2052, 128, alpha=0.5, acc=1, ldc=2056), {"GEMM_BIG": 0})
_nt_add("big256-relu-n2048-bf16f32", nt("bf16f32", 257, 2048, 192, bias=1, relu=1))
# ---- split K: explicit splits that leave a short last slice or fewer slices than asked; the automatic rule (splits = 0, += into fp32)
_nt_add("split3-k320-bf16f32", nt("bf16f32", 200, 136, 320, splits=3, acc=1, bias=1))
_nt_add("split4-becomes-3-k320-bf16f32", nt("bf16f32", 200, 136, 320, splits=4, acc=1, alpha=0.5))
_nt_add("split3-k160-f32", nt("f32", 200, 136, 160, splits=3, acc=1, bias=1))
_nt_add("split2-tile-k100-f32", nt("f32", 100, 100, 100, splits=2, acc=1, bias=1))
_nt_add("split2-tile-k100-bf16f32", nt("bf16f32", 130, 70, 100, splits=2, acc=1))
_nt_add("autosplit-k832-bf16f32", nt("bf16f32", 640, 640, 832, splits=0, acc=1, bias=1))
_nt_add("autosplit-k416-f32", nt("f32", 640, 630, 416, splits=0, acc=1, alpha=0.5, ldc=632))
_nt_add("autosplit-k1024-4-f32", nt("f32", 300, 320, 1024, splits=0, acc=1))


@pytest.mark.parametrize("name", sorted(NT_CASES))
def test_gemm_nt_auto(ops, name):
    _run_nt(ops, NT_CASES[name][0], seed=_seed(name))


@pytest.mark.parametrize("name", sorted(k for k, v in NT_CASES.items() if v[1]))
def test_gemm_nt_hooked(ops, name):
    case, hooks = NT_CASES[name]
    _auto_and_hooked(lambda: _run_nt(ops, case, seed=_seed(name)), hooks)


# ================================================================================================ asr_gemm_nn
def nn(combo, M, N, K, **kw):
    """out (M, N) (+)= alpha * dy (M, K) @ w (K, N) [ReLU mask]: K is the contracted width (ops.gemm_nn calls it N)."""
    return dict(combo=combo, M=M, N=N, K=K, **kw)


def _run_nn(ops, c, seed):
    tin, tout = COMBOS[c["combo"]]
    M, N, K = c["M"], c["N"], c["K"]
    stage = 32 if tin == F32 else 64
    Kp = (K + stage - 1) // stage * stage                      # zero columns in dy up to the kernel's reduction stage
    ldw, ldc = c.get("ldw", N), c.get("ldc", N)
    g = torch.Generator().manual_seed(seed)
    dy, w = _ints(g, (M, K)), _ints(g, (K, N))
    dyp = torch.zeros(M, Kp, dtype=torch.float64)
    dyp[:, :K] = dy
    dyd = dyp.to(tin).to(D)
    _, wd, _ = _place(w, ldw, 0, tin, 3.0)
    alpha = c.get("alpha", 1.0)
    ref = alpha * (dy @ w)
    mask = None
    if c.get("mask"):
        mask = _ints(g, (M, N), -1, 1)
        ref = ref * (mask > 0)
        _, mask, _ = _place(mask, ldc, 0, tin, 1.0)
    acc = bool(c.get("acc"))
    old = _ints(g, (M, N), -8, 8) if acc else None
    if acc:
        ref = old + ref
    name = "gemm_nn %s" % c
    _premise(name, ref, (dy.abs() @ w.abs()).max() + 8)
    flat, Cd, img = _place(old if acc else torch.full((M, N), SENTINEL, dtype=torch.float64), ldc, 0, tout, SENTINEL)
    ops.gemm_nn(dyd, wd, out=Cd, accumulate=acc, relu_mask=mask, alpha=alpha)
    torch.cuda.synchronize()
    img.view(M, ldc)[:, :N] = ref
    got = flat.cpu()
    _same(name, got.view(M, ldc), img.to(tout).view(M, ldc))
    return {"C": got}


NN_CASES = {}


def _nn_add(name, case, hooks=None):
    assert name not in NN_CASES
    NN_CASES[name] = (case, hooks)


for _cb in COMBOS:
    # ---- the four-wave 64-row kernel: partial blocks, a ragged contraction (zero columns up to the stage), ldb > N, ldc > N
    _nn_add("nn64-200x72-%s" % _cb, nn(_cb, 200, 72, 64))
    _nn_add("nn64-kragged-ldb-%s" % _cb, nn(_cb, 130, 100, 100, ldw=104))
    _nn_add("nn64-ldc-%s" % _cb, nn(_cb, 65, 136, 192, ldc=144, ldw=136))
    _nn_add("nn64-acc-%s" % _cb, nn(_cb, 300, 136, 192, acc=1, alpha=0.5))
    # ---- 128-row tiles from kNnBig = 1700 blocks of 64 x 64 on (N = 60: the eight-wave path refuses the bf16 call, t128 = 850)
    _nn_add("nn128-t1700-%s" % _cb, nn(_cb, 108793, 60, 64, ldw=64, alpha=0.5))
    _nn_add("nn64-t1699-%s" % _cb, nn(_cb, 108736, 60, 64, ldw=64, alpha=0.5))
_nn_add("nn64-mask-bf16", nn("bf16", 300, 136, 192, mask=1))
_nn_add("nn64-mask-f32", nn("f32", 300, 136, 96, mask=1, alpha=0.25))
_nn_add("nn128-t1700-mask-acc-bf16", nn("bf16", 108800, 64, 64, ldc=68, mask=1, acc=1))      # ldc % 8 != 0: refused by the eight-wave path
# ---- the eight-wave NN path from 150 blocks of 128 x 128 on; 4 stages for 150 .. 256 blocks over K >= 2048
_nn_add("nnbig-t149-bf16", nn("bf16", 19072, 128, 64), {"GEMM_BIG_NN": 2})
_nn_add("nnbig-t150-bf16", nn("bf16", 19073, 128, 64), {"GEMM_BIG_NN": 0})
_nn_add("nnbig-t150-mask-acc-bf16", nn("bf16", 19073, 120, 128, ldw=128, ldc=128, mask=1, acc=1, alpha=0.5), {"GEMM_BIG_NN": 0})
_nn_add("nnbig-ns4-k2048-bf16", nn("bf16", 19200, 128, 2048), {"GEMM_BIG_NS": 3})
# ---- the ring cut-off NN_RING (512 blocks, K >= 256); N = 60 keeps the eight-wave path away at 513 blocks
_nn_add("nnring-512-bf16", nn("bf16", 32768, 60, 256, ldw=64), {"NN_RING": 0})
_nn_add("nnring-513-bf16", nn("bf16", 32769, 60, 256, ldw=64), {"NN_RING": 1 << 20})
_nn_add("nnring-512-k192-bf16", nn("bf16", 32768, 60, 192, ldw=64))
_nn_add("nnring-512-t128-bf16", nn("bf16", 16384, 128, 320, mask=1), {"NN_RING": 0})


@pytest.mark.parametrize("name", sorted(NN_CASES))
def test_gemm_nn_auto(ops, name):
    _run_nn(ops, NN_CASES[name][0], seed=_seed(name))


@pytest.mark.parametrize("name", sorted(k for k, v in NN_CASES.items() if v[1]))
def test_gemm_nn_hooked(ops, name):
    case, hooks = NN_CASES[name]
    _auto_and_hooked(lambda: _run_nn(ops, case, seed=_seed(name)), hooks)


# ================================================================================================ asr_gemm_nn_rowdot
def _run_rowdot(ops, M, T, N, K, use_o32, seed):
    """dx (M, N) = dy (M, K) @ w (K, N) and rowdot (M / T, N / 64, T) = the sums of dx * o over each run of 64 columns.  Entries in
    {-1, 0, 1} and K <= 256: |dx| <= 256 is an integer bf16 holds exactly, so the row sums are the same whether the kernel multiplies
    the rounded or the un-rounded dx."""
    assert K <= 256
    g = torch.Generator().manual_seed(seed)
    dy, w = _ints(g, (M, K), -1, 1), _ints(g, (K, N), -1, 1)
    o = _ints(g, (M, N))
    dx = dy @ w
    H, Bn = N // 64, M // T
    rd = (dx * o).view(Bn, T, H, 64).sum(-1).permute(0, 2, 1).contiguous()
    name = "gemm_nn_rowdot %s" % ((M, T, N, K, use_o32),)
    _premise(name, dx, (dy.abs() @ w.abs()).max())
    assert torch.equal(dx.to(BF).double(), dx), "dx must be exact in bf16"
    _premise(name + " rowdot", rd, (dx.abs() * o.abs()).view(Bn, T, H, 64).sum(-1).max())
    got = ops.gemm_nn_rowdot(dy.to(BF).to(D), w.to(BF).to(D), o.to(BF).to(D), o.float().to(D) if use_o32 else None, T)
    assert got is not None, "asr_gemm_nn_rowdot refused %s" % name
    torch.cuda.synchronize()
    _same(name + " dx", got[0].cpu(), dx.to(BF))
    _same(name + " rowdot", got[1].cpu().view(Bn * H, T), rd.float().view(Bn * H, T))
    return {"dx": got[0].cpu(), "rowdot": got[1].cpu().view(Bn * H, T)}


ROWDOT_CASES = {
    "rowdot-eightwave-t150": ((19200, 100, 128, 64), {"GEMM_BIG_NN": 0}),
    "rowdot-ring": ((1600, 100, 128, 256), {"NN_RING": 0}),
    "rowdot-ring-forced-eightwave": ((1500, 100, 192, 256), {"GEMM_BIG_NN": 2}),
    "rowdot-plain-k192": ((1600, 100, 128, 192), None),
}


@pytest.mark.parametrize("use_o32", [True, False], ids=["o32", "obf16"])
@pytest.mark.parametrize("name", sorted(ROWDOT_CASES))
def test_gemm_nn_rowdot_auto(ops, name, use_o32):
    _run_rowdot(ops, *ROWDOT_CASES[name][0], use_o32=use_o32, seed=_seed(name))


@pytest.mark.parametrize("name", sorted(k for k, v in ROWDOT_CASES.items() if v[1]))
def test_gemm_nn_rowdot_hooked(ops, name):
    shape, hooks = ROWDOT_CASES[name]
    _auto_and_hooked(lambda: _run_rowdot(ops, *shape, use_o32=True, seed=_seed(name)), hooks)


# ================================================================================================ asr_gemm_tn
def tn(dtype, M, N, K, **kw):
    """dw (N, K) fp32 += dy (M, N)^T @ x (M, K), db (N) += column sums of dy."""
    return dict(dtype=dtype, M=M, N=N, K=K, **kw)


def _run_tn(ops, c, seed):
    from asr_hip import lib as L
    dtype = F32 if c["dtype"] == "f32" else BF
    M, N, K = c["M"], c["N"], c["K"]
    ldy, ldx, ldw = c.get("ldy", N), c.get("ldx", K), c.get("ldw", K)
    g = torch.Generator().manual_seed(seed)
    dy, x = _ints(g, (M, N)), _ints(g, (M, K))
    dw0, db0 = _ints(g, (N, K), -8, 8), _ints(g, (N,), -8, 8)
    _, dyd, _ = _place(dy, ldy, 0, dtype, 3.0)
    _, xd, _ = _place(x, ldx, 0, dtype, 3.0)
    ref_dw, ref_db = dw0 + dy.t() @ x, db0 + dy.sum(0)
    name = "gemm_tn %s" % c
    _premise(name + " dW", ref_dw, (dy.abs().t() @ x.abs()).max() + 8)
    _premise(name + " db", ref_db, dy.abs().sum(0).max() + 8)
    flat, dwd, img = _place(dw0, ldw, 0, F32, SENTINEL)
    dbd = db0.float().to(D) if c.get("db", 1) else None
    if "ws_tiles" in c:
        # a workspace the caller sized for the 64 x 64 kernel (ws_tiles slices of 64 x 64 tiles): too small for the pipelined 128 x 128
        # kernel's slices, which must then leave the call to the 64 x 64 kernel
        n_ws = c["ws_tiles"] * ((N + 63) // 64) * ((K + 63) // 64) * 4096
        assert n_ws < L.load().asr_gemm_tn_workspace(M, N, K, 0, L.dt(dyd))
        ws = torch.empty(n_ws, device=D, dtype=F32)
        L.call("asr_gemm_tn", L.ptr(dyd), dyd.stride(0), L.ptr(xd), xd.stride(0), L.ptr(dwd), dwd.stride(0), L.ptr(dbd), L.ptr(ws), n_ws, M, N, K,
               0, L.dt(dyd), L.stream())
    else:
        ops.gemm_tn(dyd, xd, dwd, colsum_acc=dbd, N=N, K=K, splits=c.get("splits", 0), use_ws=c.get("use_ws", True))
    torch.cuda.synchronize()
    img.view(N, ldw)[:, :K] = ref_dw
    out = {"dW": flat.cpu()}
    _same(name + " dW", out["dW"].view(N, ldw), img.float().view(N, ldw))
    if dbd is not None:
        out["db"] = dbd.cpu().view(1, N)
        _same(name + " db", out["db"], ref_db.float().view(1, N))
    return out


TN_CASES = {}
# ---- the pipelined 128 x 128 kernel (bf16, >= 64 blocks of dW): 8 slices folded through the workspace; ragged rows; one slice
TN_CASES["tn128-s8"] = tn("bf16", 1024, 1024, 1024)
TN_CASES["tn128-s8-m1001-ragged"] = tn("bf16", 1001, 1000, 1024, ldy=1008, ldx=1032, ldw=1028)
TN_CASES["tn128-m900-6-slices"] = tn("bf16", 900, 1024, 1000, ldx=1000, db=0)
for _m in (1, 31, 32, 33, 200):
    TN_CASES["tn128-s1-m%d" % _m] = tn("bf16", _m, 1024, 1024)
TN_CASES["tn128-s1-many-blocks"] = tn("bf16", 640, 2816, 2048)
# ---- calls the pipelined kernel must hand on to the 64 x 64 kernel: no workspace; a workspace too small for its slices
TN_CASES["tn64-no-ws-where-s128-is-8"] = tn("bf16", 1024, 1024, 1024, use_ws=False)
TN_CASES["tn64-ws-too-small-for-s128"] = tn("bf16", 1024, 1024, 1024, ws_tiles=2)
for _dt in ("f32", "bf16"):
    # ---- the 64 x 64 kernel: slices through a workspace, slices through atomics, explicit slices, N < 128, few blocks, short and ragged M
    TN_CASES["tn64-ws-%s" % _dt] = tn(_dt, 2000, 512, 512)
    TN_CASES["tn64-atomics-%s" % _dt] = tn(_dt, 2000, 512, 512, use_ws=False)
    TN_CASES["tn64-splits3-%s" % _dt] = tn(_dt, 1000, 200, 264, splits=3, ldy=208, ldw=268)
    TN_CASES["tn64-few-blocks-%s" % _dt] = tn(_dt, 500, 256, 256)
    for _m in (1, 31, 32, 33, 200):
        TN_CASES["tn64-n70-m%d-%s" % (_m, _dt)] = tn(_dt, _m, 70, 100, ldy=72, ldx=104, ldw=101)


@pytest.mark.parametrize("name", sorted(TN_CASES))
def test_gemm_tn_auto(ops, name):
    _run_tn(ops, TN_CASES[name], seed=_seed(name))


# ================================================================================================ asr_gemm_nn_tn + flush_tn_reduces
@pytest.mark.parametrize("shape", [(200, 64, 64), (130, 192, 72), (37, 64, 200), (1000, 1536, 512), (6400, 64, 1088)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_gemm_nn_tn_auto(ops, shape):
    """dx (M, K) = dy (M, N) @ w (N, K) and dw (N, K) += dy^T x, db += column sums of dy from ONE launch, two layers pending (the second
    with `+=` and a ReLU mask); the partial tiles folded by the next launch and by flush_tn_reduces().  6400 x 1088: the 128-row form."""
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    ldx = (K + 7) // 8 * 8 + 8
    dy, w, x = _ints(g, (M, N)), _ints(g, (N, K)), _ints(g, (M, K))
    dw0, db0 = _ints(g, (N, K), -8, 8), _ints(g, (N,), -8, 8)
    old, mask = _ints(g, (M, K), -8, 8), _ints(g, (M, K), -1, 1)
    dyd, wd = dy.to(BF).to(D), w.to(BF).to(D)
    _, xd, _ = _place(x, ldx, 0, BF, 3.0)
    ref_dx, ref_dw, ref_db = dy @ w, dw0 + dy.t() @ x, db0 + dy.sum(0)
    ref_dx2 = old + ref_dx * (mask > 0)
    name = "gemm_nn_tn %s" % (shape,)
    _premise(name + " dx", ref_dx, (dy.abs() @ w.abs()).max() + 8)
    _premise(name + " dx +=", ref_dx2, (dy.abs() @ w.abs()).max() + 8)
    _premise(name + " dW", ref_dw, (dy.abs().t() @ x.abs()).max() + 8)
    _premise(name + " db", ref_db, dy.abs().sum(0).max() + 8)
    dw_a, db_a, dw_b = dw0.float().to(D), db0.float().to(D), dw0.float().to(D)
    out_b = old.to(BF).to(D)
    ops.reset_pending()
    try:
        out_a = ops.gemm_nn_tn(dyd, wd, xd, dw_a, db_a)
        ops.gemm_nn_tn(dyd, wd, xd, dw_b, None, out=out_b, accumulate=True, relu_mask=mask.to(BF).to(D))
        ops.flush_tn_reduces()
        torch.cuda.synchronize()
    finally:
        ops.reset_pending()
    _same(name + " dx", out_a.cpu(), ref_dx.to(BF))
    _same(name + " dx += masked", out_b.cpu(), ref_dx2.to(BF))
    _same(name + " dW folded by the next launch", dw_a.cpu(), ref_dw.float())
    _same(name + " dW folded by flush_tn_reduces", dw_b.cpu(), ref_dw.float())
    _same(name + " db", db_a.cpu().view(1, N), ref_db.float().view(1, N))


# ================================================================================================ asr_gemm_tn_grouped
def _headline_layers():
    """(M, N, K) of the 46 linear layers whose weight gradients one grouped launch of the configs[1] step computes (B = 32: 6400 encoder
    rows, 3200 decoder rows) -- the list of tests/test_host.py test_grouped_weight_gradient_plan."""
    enc = lambda M: [(M, 512, 2048), (M, 2048, 512), (M, 512, 512), (M, 1536, 512)]
    dec = lambda Md, Me: [(Md, 512, 2048), (Md, 2048, 512), (Md, 512, 512), (Me, 1024, 512), (Md, 512, 512), (Md, 512, 512), (Md, 1536, 512)]
    layers = [(3200, 4416, 512)] + dec(3200, 6400) * 4 + enc(6400) * 4 + [(6400, 512, 2560)]
    assert len(layers) == 46
    return layers


EDGE_LAYERS = [(1700, 512, 512, 512, 512, True), (933, 1536, 512, 1536, 512, True), (400, 2048, 512, 2048, 512, True),
               (1601, 512, 2048, 512, 2048, True), (640, 300, 512, 320, 512, True), (777, 512, 264, 512, 264, False),
               (0, 64, 64, 64, 64, True), (3300, 256, 256, 256, 256, True), (1, 64, 72, 64, 72, True), (33, 130, 257, 136, 264, True)]


def _run_grouped(ops, layers, seed):
    """layers: (M, N, K, ld_dy, ld_x, has_bias).  Problems of one shape share two operand pairs, each used with both signs of dy: the
    float64 products are computed once per pair, and no two problems of a launch have the same answer."""
    g = torch.Generator().manual_seed(seed)
    pairs, count, probs, want = {}, {}, [], []
    for (M, N, K, ldy, ldx, hb) in layers:
        key = (M, N, K, ldy, ldx)
        i = count.get(key, 0)
        count[key] = i + 1
        R = max(M, 1)
        if (key, (i // 2) % 2) not in pairs:
            dy, x = _ints(g, (R, N)), _ints(g, (R, K))
            name = "gemm_tn_grouped %s" % (key,)
            prod, colsum = dy[:M].t() @ x[:M], dy[:M].sum(0)
            if M > 0:
                _premise(name + " dW", prod, (dy[:M].abs().t() @ x[:M].abs()).max() + 8)
            assert float(dy[:M].abs().sum(0).max() if M else 0) + 8 < LIMIT
            pairs[(key, (i // 2) % 2)] = (dy, x, prod, colsum, {})
        dy, x, prod, colsum, dev = pairs[(key, (i // 2) % 2)]
        sign = -1.0 if i % 2 else 1.0
        if sign not in dev:
            dev[sign] = (_place(sign * dy, ldy, 0, BF, 3.0)[1][:M], _place(x, ldx, 0, BF, 3.0)[1][:M])
        dyd, xd = dev[sign]
        dw0, db0 = _ints(g, (N, K), -8, 8), _ints(g, (N,), -8, 8)
        probs.append((dyd, xd, dw0.float().to(D), db0.float().to(D) if hb else None, N, K))
        want.append(((dw0 + sign * prod).float(), (db0 + sign * colsum).float() if hb else None))
    for at in range(0, len(probs), 48):
        ops.gemm_tn_grouped(probs[at:at + 48])
    torch.cuda.synchronize()
    out = {}
    for n, (pr, (rdw, rdb)) in enumerate(zip(probs, want)):
        tag = "gemm_tn_grouped problem %d %s" % (n, layers[n])
        out["dW%d" % n] = pr[2].cpu()
        _same(tag + " dW", out["dW%d" % n], rdw)
        if rdb is not None:
            out["db%d" % n] = pr[3].cpu().view(1, -1)
            _same(tag + " db", out["db%d" % n], rdb.view(1, -1))
    return out


def test_gemm_tn_grouped_auto_headline_layers(ops):
    _run_grouped(ops, [(M, N, K, N, K, True) for M, N, K in _headline_layers()], seed=46)


def test_gemm_tn_grouped_auto_edge_shapes(ops):
    _run_grouped(ops, EDGE_LAYERS, seed=10)


@pytest.mark.parametrize("M", [9599, 9600])
def test_gemm_tn_grouped_auto_shared_forms(ops, M):
    """Eight equal 512 x 512 layers: a list the whole-block plan declines (32 blocks of 300 stages on 256 CUs), so the dispatch takes a
    shared form by its own condition -- equal pieces on one workgroup per CU below slice_min = 9 600 rows, per-slice blocks that meet in
    fp32 atomics from there on."""
    from asr_hip import lib as L
    layers = [(M, 512, 512)] * 8
    n = len(layers)
    I = ctypes.c_int * n
    sp = I()
    assert L.load().asr_gemm_tn_grouped_plan(n, I(*[l[0] for l in layers]), I(*[l[1] for l in layers]), I(*[l[2] for l in layers]), sp) == 0
    _run_grouped(ops, [(m, N, K, N, K, True) for m, N, K in layers], seed=M)


@pytest.mark.parametrize("tile", [1, 128, 256])
def test_gemm_tn_grouped_hooked(ops, tile):
    _auto_and_hooked(lambda: _run_grouped(ops, EDGE_LAYERS, seed=10), {"TN_GROUP_TILE": tile})
