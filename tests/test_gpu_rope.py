"""asr_rope (csrc/rope.hip) on the MI355X against the float64 restatement of tests/rope_reference.py: both arms bit for bit on data whose
every result is exact, real angles within the rounding the kernel is allowed, the refused arguments, and RopeFn's gradient.

Exact arm: data are integers in [-8, 8] and every table entry is one of (1,0), (0,1), (-1,0), (0,-1), (0.5,0.5), (0.5,-0.5), so every
product is a multiple of 0.5 of magnitude <= 8 and every result a multiple of 0.5 of magnitude <= 8: exact in bf16 and fp32, whatever
the order of the roundings.  The operand lies inside a buffer of sentinels and the WHOLE buffer is compared, so the columns beside the
view (V of the fused Q|K|V layout) and the elements in front of and behind it must keep their bits."""
import pytest
import torch

import rope_reference as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
ENTRIES = torch.tensor([[1, 0], [0, 1], [-1, 0], [0, -1], [0.5, 0.5], [0.5, -0.5]], dtype=torch.float32)
EPS32 = 2.0 ** -24
GUARD = 16                 # sentinel elements in front of and behind the operand (16 elements keep a 16-byte alignment in both types)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _exact_table(T, d, seed):
    return ENTRIES[torch.randint(0, len(ENTRIES), (T, d // 2), generator=_gen(seed))].contiguous()


def _operand(data, layout, dtype, front=GUARD):
    """data (B,T,W) on the host -> (flat device buffer, the (B,T,W) view of it the kernel gets): contiguous, or the first W columns of rows of
    W + W/2 (Q|K of a fused Q|K|V buffer); `front` sentinel elements before the view, GUARD behind it."""
    B, T, W = data.shape
    Wb = W if layout == "contiguous" else W + W // 2
    flat = torch.full((front + B * T * Wb + GUARD,), 3.0, dtype=dtype)
    rows = flat[front:front + B * T * Wb].view(B, T, Wb)
    rows[:, :, W:] = 5.0
    rows[:, :, :W] = data.to(dtype)
    flat = flat.cuda()
    return flat, flat[front:front + B * T * Wb].view(B, T, Wb)[:, :, :W]


def _expected(flat_before, view_of, ref):
    """The whole buffer as it must look afterwards: `ref` in the view, every other element as before."""
    want = flat_before.clone()
    view_of(want).copy_(ref.to(want.dtype))
    return want


def _run_exact(B, T, nheads, d, arm, layout, front=GUARD, seed=0):
    from asr_hip import ops
    dtype = DTYPES[arm]
    W = nheads * d
    data = torch.randint(-8, 9, (B, T, W), generator=_gen(seed + 1)).float()
    cs = _exact_table(T, d, seed + 2)
    Wb = W if layout == "contiguous" else W + W // 2
    view_of = lambda f: f[front:front + B * T * Wb].view(B, T, Wb)[:, :, :W]
    for inverse in (False, True):
        flat, x = _operand(data, layout, dtype, front)
        before = flat.clone()
        assert ops.rope_(x, cs.cuda(), nheads, d, inverse=inverse) is x
        torch.cuda.synchronize()
        ref = R.rope64(data, cs, nheads, d, inverse=inverse)
        assert torch.equal(ref, torch.round(ref * 2) / 2) and ref.abs().max().item() <= 8          # the exactness argument above
        assert torch.equal(flat.cpu(), _expected(before.cpu(), view_of, ref)), (inverse, layout)
        assert not torch.equal(flat, before)


@pytest.mark.parametrize("layout", ["contiguous", "qk_of_qkv"])
@pytest.mark.parametrize("B,T,nheads", [(1, 1, 1), (2, 5, 3), (3, 33, 10)])
@pytest.mark.parametrize("d", [16, 32, 64])
@pytest.mark.parametrize("arm", ["fp32", "bf16"])
def test_exact_data_bit_for_bit(arm, d, B, T, nheads, layout):
    _run_exact(B, T, nheads, d, arm, layout)


@pytest.mark.parametrize("layout", ["contiguous", "qk_of_qkv"])
@pytest.mark.parametrize("arm", ["fp32", "bf16"])
def test_view_offset_by_two_elements_takes_the_pair_arm(arm, layout):
    """8 bytes (fp32) or 4 bytes (bf16) past a 16-byte boundary: no 16-byte access is possible, the pair arm serves the call."""
    _run_exact(3, 33, 10, 32, arm, layout, front=2, seed=10)
    _run_exact(2, 5, 3, 16, arm, layout, front=GUARD + 2, seed=11)


@pytest.mark.parametrize("arm", ["fp32", "bf16"])
def test_chunk_count_that_is_no_multiple_of_the_block(arm):
    """nheads d / 8 = 10 chunks a row (20 in fp32), 77 rows: 770 (1540) chunks = 3 (6) whole blocks of 256 and a tail of 2 (4) lanes."""
    _run_exact(1, 77, 5, 16, arm, "contiguous", seed=20)
    _run_exact(1, 77, 5, 16, arm, "qk_of_qkv", seed=21)


@pytest.mark.parametrize("arm,nheads", [("fp32", 16), ("bf16", 32)])
def test_more_chunks_than_the_grid_has_lanes(arm, nheads):
    """B 9, T 257, d 64: 592 128 chunks of 16 bytes (16 heads in fp32, 32 in bf16) against 2048 x 256 = 524 288 lanes, so the grid-stride
    loop runs a second time for some lanes and not for others."""
    assert 9 * 257 * nheads * 64 // (4 if arm == "fp32" else 8) > 2048 * 256
    _run_exact(9, 257, nheads, 64, arm, "contiguous", seed=30)


# ------------------------------------------------------------------------------------------------ real angles
def _pair_sum(x):
    """|x0| + |x1| of each element's pair, in the element's place."""
    a = x.abs().reshape(*x.shape[:-1], -1, 2)
    return a.sum(-1, keepdim=True).expand_as(a).reshape(x.shape)


def _bound(arm, ref, pair_sum):
    """fp32: at most three fp32 roundings per result (two products, one sum), each below 2^-24 (|x0| + |x1|), and the table is shared with
    the reference.  bf16: one round-to-nearest to bf16 on top of that."""
    b = 4 * EPS32 * pair_sum
    return b if arm == "fp32" else b + 2.0 ** -8 * ref.abs()


@pytest.mark.parametrize("B,T,nheads,d", [(2, 75, 10, 64), (1, 7, 2, 16)])
@pytest.mark.parametrize("arm", ["fp32", "bf16"])
def test_real_angles_within_the_roundings_of_the_format(arm, B, T, nheads, d):
    from asr_hip import ops
    dtype = DTYPES[arm]
    cs = ops.rope_table(T, d)
    x = torch.randn(B, T, nheads * d, generator=_gen(40)).to(dtype)
    x64 = x.double()
    for inverse in (False, True):
        got = ops.rope_(x.cuda().clone(), cs.cuda(), nheads, d, inverse=inverse).cpu().double()
        ref = R.rope64(x64, cs, nheads, d, inverse=inverse)
        ratio = ((got - ref).abs() / _bound(arm, ref, _pair_sum(x64))).max().item()
        print("%s %s inverse=%d: worst |got - ref| / bound = %.3f" % (arm, (B, T, nheads, d), inverse, ratio))
        assert ratio <= 1.0
    assert (R.rope64(x64, cs, nheads, d) - x64).abs().max().item() > 0.5 or T == 1          # (real rotations, not the identity)


@pytest.mark.parametrize("B,T,nheads,d", [(2, 75, 10, 64), (1, 7, 2, 16)])
@pytest.mark.parametrize("arm", ["fp32", "bf16"])
def test_inverse_after_forward_returns_the_input(arm, B, T, nheads, d):
    """Within twice the bounds of the test above, the reference being the input itself.  The bf16 bound has an ELEMENTWISE term,
    2^-8 |x|, and the inverse rotation mixes the two bf16 rounding errors of a pair (each up to 2^-8 of its own element) into both
    results: before its own rounding a result is off by up to 2^-8 ||pair||, whatever the size of x itself.  So that term can hold only
    where the members of a pair are of comparable size.  With magnitudes in [1, 2] (one binade, ulp 2^-7) the deviation before the
    last rounding is at most 2^-8 sqrt 8 = 1.42 ulp < 1.5 ulp, so the rounded result is at most ONE ulp = 2^-7 <= 2 * 2^-8 |x| from x:
    that is the data of the elementwise check (a ratio of 1.000 there is one ulp at |x| = 1).  Gaussian data, where one member of a
    pair can be tiny, are held to the same figures with the pair's |x0| + |x1| >= ||pair|| in place of |x|."""
    from asr_hip import ops
    dtype = DTYPES[arm]
    cs = ops.rope_table(T, d).cuda()
    g = _gen(50)
    comparable = ((1 + torch.rand(B, T, nheads * d, generator=g)) * (1 - 2 * torch.randint(0, 2, (B, T, nheads * d), generator=g))).to(dtype)
    gauss = torch.randn(B, T, nheads * d, generator=g).to(dtype)
    for name, x in (("comparable", comparable), ("gaussian", gauss)):
        y = ops.rope_(x.cuda().clone(), cs, nheads, d)
        back = ops.rope_(y, cs, nheads, d, inverse=True).cpu().double()
        x64 = x.double()
        ps = _pair_sum(x64)
        bound = 2 * _bound(arm, x64 if name == "comparable" else ps, ps)
        ratio = ((back - x64).abs() / bound).max().item()
        print("%s %s %s: worst |inverse(forward(x)) - x| / (2 bound) = %.3f" % (arm, (B, T, nheads, d), name, ratio))
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ arguments
def test_unsupported_arguments_are_refused_before_any_launch():
    from asr_hip import lib as L
    from asr_hip import ops
    h = L.load()
    B, T = 2, 6
    x = torch.full((B, T, 264), 7.0, device="cuda")
    cs = torch.full((T, 66, 2), 0.5, device="cuda")
    st = L.stream()
    for d in (0, 2, 8, 24, 48, 128):                                   # a head width the attention kernels do not contract
        assert h.asr_rope(L.ptr(x), T * 264, 264, B, T, 2, d, L.ptr(cs), 0, L.F32, st) == L.EUNSUPPORTED, d
    for sb, s_t in ((T * 264, 263), (T * 264 + 1, 264), (T * 33, 33)):       # odd strides
        assert h.asr_rope(L.ptr(x), sb, s_t, B, T, 2, 16, L.ptr(cs), 0, L.F32, st) == L.EUNSUPPORTED, (sb, s_t)
        assert h.asr_rope(L.ptr(x), sb, s_t, B, T, 2, 16, L.ptr(cs), 1, L.BF16, st) == L.EUNSUPPORTED, (sb, s_t)
    assert h.asr_rope(None, T * 264, 264, B, T, 2, 16, L.ptr(cs), 0, L.F32, st) == -1          # ASR_EINVAL
    assert h.asr_rope(L.ptr(x), T * 264, 264, B, T, 2, 16, None, 0, L.F32, st) == -1
    assert h.asr_rope(L.ptr(x), T * 264, 264, B, T, 2, 16, L.ptr(cs), 0, 5, st) == -1          # no such storage type
    with pytest.raises(L.AsrHipError) as e:
        ops.rope_(x[:, :, :48], cs[:, :12].contiguous(), 2, 24)
    assert "(%d)" % L.EUNSUPPORTED in str(e.value)
    with pytest.raises(AssertionError):
        ops.rope_(x[:, :, :32], cs[:, :8], 2, 16)                       # a table that is not contiguous
    with pytest.raises(AssertionError):
        ops.rope_(x[:, :, :32], cs[:4, :8].contiguous(), 2, 16)         # a table with the wrong number of rows
    torch.cuda.synchronize()
    assert (x == 7.0).all()                                            # nothing ran


def test_zero_sizes_are_ok_and_launch_nothing():
    from asr_hip import lib as L
    from asr_hip import ops
    h = L.load()
    x = torch.full((2, 6, 32), 7.0, device="cuda")
    cs = torch.full((6, 8, 2), 0.5, device="cuda")
    st = L.stream()
    for B, T, nheads in ((0, 6, 2), (2, 0, 2), (2, 6, 0), (0, 0, 0)):
        assert h.asr_rope(L.ptr(x), 6 * 32, 32, B, T, nheads, 16, L.ptr(cs), 0, L.F32, st) == 0
        assert h.asr_rope(None, 6 * 32, 32, B, T, nheads, 16, None, 1, L.BF16, st) == 0
    e = torch.empty((0, 6, 32), device="cuda")
    assert ops.rope_(e, cs, 2, 16) is e
    torch.cuda.synchronize()
    assert (x == 7.0).all()


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("B,T,nheads,d", [(2, 75, 10, 64), (1, 7, 2, 16)])
def test_ropefn_gradient_is_the_restatements(B, T, nheads, d):
    from asr_hip import ops
    from asr_hip.functions import RopeFn
    cs = ops.rope_table(T, d)
    x = torch.randn(B, T, nheads * d, generator=_gen(60))
    g = torch.randn(B, T, nheads * d, generator=_gen(61))
    xd = x.cuda().requires_grad_(True)
    keep = xd.detach().clone()
    y = RopeFn.apply(xd, cs.cuda(), nheads, d)
    (y * g.cuda()).sum().backward()
    assert torch.equal(xd.detach(), keep)                              # out of place
    x64 = x.double().requires_grad_(True)
    y64 = R.rope64(x64, cs, nheads, d)
    (y64 * g.double()).sum().backward()
    assert ((y.detach().cpu().double() - y64.detach()).abs() <= 4 * EPS32 * _pair_sum(x.double())).all()
    ratio = ((xd.grad.cpu().double() - x64.grad).abs() / (4 * EPS32 * _pair_sum(g.double()))).max().item()
    print("worst |grad - grad64| / bound = %.3f" % ratio)
    assert ratio <= 1.0
