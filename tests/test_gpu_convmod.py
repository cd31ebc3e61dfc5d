"""The three kernels of the convolution module (csrc/convmod.hip) on the MI355X against the float64 restatement of their definition
(tests/convmod_reference.py, itself held against torch's composition and autograd by tests/test_convmod_host.py).

Shapes: the smallest at which the kernels can go wrong -- one element; T < K (all halo); T no multiple of the 64-frame tile with D no
power of two (a half-filled 128-channel chunk); several tiles and slices at the model's width; and 165 tiles, more than the weight
gradient's 128 row slices, so that a slice sums more than one tile.

Bounds, e(x) = max|x - ref64| / max|ref64| per tensor:
  fp32 arm     s, v, du, dwd, dbd: e <= 4 e_torch32 + 1e-6, e_torch32 = the same torch composition (and its autograd) in fp32 on the CPU
               against the same float64 values: torch's own fp32 error, never the kernel's.
  bf16 arm     s, v, du (stored in bf16): |x - ref| <= 2^-8 |ref| + 1e-5 max|ref| elementwise, ref in float64 on the SAME bf16 inputs
               and, for the backward, on the saved s as given (one bf16 rounding is 2^-9; the bound doubles it);
               dwd, dbd (fp32 accumulation): 4 e_torch32 + 1e-6 as above, e_torch32 on the bf16 inputs.
  exact arm    gate = 40, bd = 96, small integers: v, du, dwd, dbd torch.equal to the float64 restatement rounded to the output's
               dtype (float64 holds sigma(34) = 1 - 1.7e-15, so it is the integers up to 1e-9; float32 NumPy gives them exactly).
Each check prints its figures before it asserts (pytest -s shows them).
"""
import numpy as np
import pytest
import torch

import convmod_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [((1, 1, 8, 3), [1]), ((3, 5, 64, 31), [5, 3, 1]), ((2, 67, 192, 7), [67, 40]), ((4, 300, 512, 15), [300, 299, 150, 17]),
          ((33, 257, 8, 3), [257 - 7 * (i % 30) for i in range(33)])]
IDS = ["%dx%dx%dx%d" % s for s, _ in SHAPES]
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _fwd(u, wd, bd, lens, dtype):
    from asr_hip import ops
    B, T, D2 = u.shape
    D, K = D2 // 2, wd.shape[1]
    ud = _dev(u, dtype).reshape(B * T, D2)
    s, v = ops.convmod_fwd(ud, _dev(wd), _dev(bd), _dev(lens, torch.int32), B, T, D, K)
    return ud, s, v


def _bwd(dv, s, ud, wd, lens, shape, dwd=None, dbd=None):
    from asr_hip import ops
    B, T, D, K = shape
    dvd = _dev(dv, ud.dtype).reshape(B * T, D)
    ld = _dev(lens, torch.int32)
    dwd = torch.zeros(D * K, device="cuda") if dwd is None else dwd
    dbd = torch.zeros(D, device="cuda") if dbd is None else dbd
    ops.convmod_bwd_weight(dvd, s, ud, ld, B, T, D, K, dwd, dbd)
    du = ops.convmod_bwd_data(dvd, s, ud, _dev(wd), ld, B, T, D, K)
    return du, dwd, dbd


def _np64(t, shape):
    return t.detach().double().cpu().numpy().reshape(shape)


def _e(x, ref):
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-300))


_cache = {}


def _random_reference(i, arm):
    """Inputs (rounded to the arm's storage type), the float64 chain on them and torch's own fp32 errors; computed once per case."""
    key = (i, arm)
    if key not in _cache:
        shape, lens = SHAPES[i]
        u, wd, bd, dv, lens = R.random_case(*shape, lens, seed=100 + i)
        if arm == "bf16":
            u, dv = (torch.from_numpy(x).bfloat16().double().numpy() for x in (u, dv))
        wd, bd = wd.astype(np.float32).astype(np.float64), bd.astype(np.float32).astype(np.float64)
        s, v, _ = R.forward(u, wd, bd, lens)
        du, dwd, dbd = R.backward(dv, s, u, wd, lens)
        ut = torch.from_numpy(u).float().requires_grad_(True)
        wt = torch.from_numpy(wd).float().reshape(shape[2], 1, -1).requires_grad_(True)
        bt = torch.from_numpy(bd).float().requires_grad_(True)
        s32, v32 = R.torch_core(ut, wt, bt, torch.from_numpy(lens))
        (v32 * torch.from_numpy(dv).float()).sum().backward()
        e32 = dict(s=_e(s32.detach().double().numpy(), s), v=_e(v32.detach().double().numpy(), v), du=_e(ut.grad.double().numpy(), du),
                   dwd=_e(wt.grad.double().numpy().reshape(dwd.shape), dwd), dbd=_e(bt.grad.double().numpy(), dbd))
        _cache[key] = (u, wd, bd, dv, lens, dict(s=s, v=v, du=du, dwd=dwd, dbd=dbd), e32)
    return _cache[key]


def _check_e(name, x, ref, e32):
    e, bound = _e(x, ref), 4 * e32 + 1e-6
    print("%-4s e %.3e  e_torch32 %.3e  bound %.3e  ratio %.3f" % (name, e, e32, bound, e / bound))
    assert e <= bound, (name, e, bound)


def _check_bf16(name, x, ref):
    slack = 2.0 ** -8 * np.abs(ref) + 1e-5 * np.abs(ref).max()
    ratio = float((np.abs(x - ref) / np.maximum(slack, 1e-300)).max())
    print("%-4s worst |x - ref| / (2^-8 |ref| + 1e-5 max|ref|) = %.3f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_fp32_arm_within_four_times_torchs_own_error(i):
    shape = SHAPES[i][0]
    B, T, D, K = shape
    u, wd, bd, dv, lens, ref, e32 = _random_reference(i, "fp32")
    ud, s, v = _fwd(u, wd, bd, lens, torch.float32)
    du, dwd, dbd = _bwd(dv, s, ud, wd, lens, shape)
    assert s.dtype == v.dtype == du.dtype == torch.float32
    print(shape)
    _check_e("s", _np64(s, (B, T, D)), ref["s"], e32["s"])
    _check_e("v", _np64(v, (B, T, D)), ref["v"], e32["v"])
    _check_e("du", _np64(du, (B, T, 2 * D)), ref["du"], e32["du"])
    _check_e("dwd", _np64(dwd, (D, K)), ref["dwd"], e32["dwd"])
    _check_e("dbd", _np64(dbd, (D,)), ref["dbd"], e32["dbd"])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_bf16_arm_within_two_roundings(i):
    shape = SHAPES[i][0]
    B, T, D, K = shape
    u, wd, bd, dv, lens, ref, e32 = _random_reference(i, "bf16")
    ud, s, v = _fwd(u, wd, bd, lens, torch.bfloat16)
    du, dwd, dbd = _bwd(dv, s, ud, wd, lens, shape)
    assert s.dtype == v.dtype == du.dtype == torch.bfloat16 and dwd.dtype == torch.float32
    print(shape)
    _check_bf16("s", _np64(s, (B, T, D)), ref["s"])
    _check_bf16("v", _np64(v, (B, T, D)), ref["v"])
    # the backward's reference: float64 on the same inputs and on the saved (bf16) s as the kernel reads it
    du_r, dwd_r, dbd_r = R.backward(dv, _np64(s, (B, T, D)), u, wd, lens)
    _check_bf16("du", _np64(du, (B, T, 2 * D)), du_r)
    _check_e("dwd", _np64(dwd, (D, K)), dwd_r, e32["dwd"])
    _check_e("dbd", _np64(dbd, (D,)), dbd_r, e32["dbd"])


def _exact(i, dtype):
    shape, lens = SHAPES[i]
    u, wd, bd, dv, lens = R.exact_case(*shape, lens, seed=40 + i)
    s, v, _ = R.forward(u, wd, bd, lens)
    du, dwd, dbd = R.backward(dv, s, u, wd, lens)
    return shape, u, wd, bd, dv, lens, dict(v=v, du=du, dwd=dwd, dbd=dbd)


@pytest.mark.parametrize("arm", ["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_exact_arm_equals_float64(i, arm):
    dtype = DTYPES[arm]
    shape, u, wd, bd, dv, lens, ref = _exact(i, dtype)
    B, T, D, K = shape
    ud, s, v = _fwd(u, wd, bd, lens, dtype)
    du, dwd, dbd = _bwd(dv, s, ud, wd, lens, shape)
    want = lambda x, dt: torch.from_numpy(x).to(dt)
    assert torch.equal(v.cpu().reshape(B, T, D), want(ref["v"], dtype))
    assert torch.equal(du.cpu().reshape(B, T, 2 * D), want(ref["du"], dtype))
    assert not du.cpu().reshape(B, T, 2 * D)[..., D:].any()                     # sigma(40) (1 - sigma(40)) = 0: the gate half
    assert torch.equal(dwd.cpu().reshape(D, K), want(ref["dwd"], torch.float32))
    assert torch.equal(dbd.cpu(), want(ref["dbd"], torch.float32))
    # the weight gradient ACCUMULATES: a second call doubles it, exactly
    _bwd(dv, s, ud, wd, lens, shape, dwd, dbd)
    assert torch.equal(dwd.cpu().reshape(D, K), 2 * want(ref["dwd"], torch.float32))
    assert torch.equal(dbd.cpu(), 2 * want(ref["dbd"], torch.float32))


@pytest.mark.parametrize("arm", ["fp32", "bf16"])
@pytest.mark.parametrize("i", [2, 3, 4], ids=IDS[2:])
def test_weight_gradient_is_deterministic(i, arm):
    shape = SHAPES[i][0]
    u, wd, bd, dv, lens, _, _ = _random_reference(i, arm)
    ud, s, v = _fwd(u, wd, bd, lens, DTYPES[arm])
    a = _bwd(dv, s, ud, wd, lens, shape)
    b = _bwd(dv, s, ud, wd, lens, shape)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("arm", ["fp32", "bf16"])
@pytest.mark.parametrize("i", [1, 2, 3, 4], ids=IDS[1:])
def test_padding_is_never_read(i, arm):
    """1e30 in u and dv at and behind len_b (and lengths given beyond T or below 0 instead of T and 0): every output bit as before;
    v and du exactly 0 there."""
    shape, _ = SHAPES[i]
    B, T, D, K = shape
    u, wd, bd, dv, lens, _, _ = _random_reference(i, arm)
    ud, s, v = _fwd(u, wd, bd, lens, DTYPES[arm])
    du, dwd, dbd = _bwd(dv, s, ud, wd, lens, shape)
    pad = np.arange(T)[None, :, None] >= lens[:, None, None]
    u2, dv2 = np.where(pad, 1e30, u), np.where(pad, 1e30, dv)
    lens2 = np.where(lens == T, T + 5, lens)
    ud2, s2, v2 = _fwd(u2, wd, bd, lens2, DTYPES[arm])
    du2, dwd2, dbd2 = _bwd(dv2, s2, ud2, wd, lens2, shape)
    for x, y in ((s, s2), (v, v2), (du, du2), (dwd, dwd2), (dbd, dbd2)):
        assert torch.equal(x, y)
    padt = torch.from_numpy(pad).cuda()
    assert not (v2.reshape(B, T, D) * padt).any() and not (du2.reshape(B, T, 2 * D) * padt).any()
    # a negative length is an empty utterance
    lens3 = lens.copy()
    lens3[-1] = 0
    lens4 = lens3.copy()
    lens4[-1] = -2
    a, b = _fwd(u, wd, bd, lens3, DTYPES[arm]), _fwd(u, wd, bd, lens4, DTYPES[arm])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and not a[2].reshape(B, T, D)[-1].any()


@pytest.mark.parametrize("B,T,D,K", [(2, 9, 16, 4), (2, 9, 16, 33), (2, 9, 12, 3), (2, 9, 16, 1)])
def test_unsupported_arguments_are_refused_before_any_launch(B, T, D, K):
    from asr_hip import lib as L
    from asr_hip import ops
    assert L.load().asr_convmod_workspace(B, T, D, K) == 0
    u = torch.randn(B * T, 2 * D, device="cuda")
    wd, bd, lens = torch.randn(D, K, device="cuda"), torch.randn(D, device="cuda"), torch.full((B,), T, device="cuda", dtype=torch.int32)
    s = torch.full((B * T, D), 7.0, device="cuda")
    v, dv, du = s.clone(), s.clone(), torch.full((B * T, 2 * D), 7.0, device="cuda")
    dwd, dbd, ws = torch.full((D * K,), 7.0, device="cuda"), torch.full((D,), 7.0, device="cuda"), torch.full((64,), 7.0, device="cuda")
    calls = [("asr_convmod_fwd", (L.ptr(u), L.ptr(wd), L.ptr(bd), L.ptr(lens), B, T, D, K, L.F32, L.ptr(s), L.ptr(v), L.stream())),
             ("asr_convmod_bwd_data", (L.ptr(dv), L.ptr(s), L.ptr(u), L.ptr(wd), L.ptr(lens), B, T, D, K, L.F32, L.ptr(du), L.stream())),
             ("asr_convmod_bwd_weight", (L.ptr(dv), L.ptr(s), L.ptr(u), L.ptr(lens), B, T, D, K, L.F32, L.ptr(ws), 64, L.ptr(dwd), L.ptr(dbd),
                                         L.stream()))]
    for name, a in calls:
        assert getattr(L.load(), name)(*a) == L.EUNSUPPORTED, name
    with pytest.raises(L.AsrHipError) as e:
        ops.convmod_fwd(u, wd, bd, lens, B, T, D, K)
    assert "(%d)" % L.EUNSUPPORTED in str(e.value)
    torch.cuda.synchronize()
    for t in (s, v, du, dwd, dbd, ws):
        assert (t == 7.0).all()                              # nothing ran
    # a storage type the kernels do not have is refused the same way
    assert D != 16 or L.load().asr_convmod_fwd(L.ptr(u), L.ptr(wd), L.ptr(bd), L.ptr(lens), B, T, 16, 3, 5, L.ptr(s), L.ptr(v), L.stream()) == L.EUNSUPPORTED
