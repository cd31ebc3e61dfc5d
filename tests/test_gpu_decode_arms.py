"""Every arm of the decode-step kernels (csrc/decode.hip: asr_dec_gemm, asr_dec_attn, asr_dec_attn_fused, asr_dec_finish;
csrc/elementwise.hip: asr_kv_append, asr_decode_prepare) against the float64 restatement of tests/decode_reference.py.

Exact arms: integer operands (every partial sum below 2^24) must give the float64 result bit for bit, one-hot softmaxes must return
a value row.  Bounded arms: random operands inside the derived bounds of decode_reference (printed as DECODE_ARMS ... error / bound
before they are asserted).  Every output sits in a buffer filled with a sentinel and 64 guard elements either side; operands carry
NaN wherever the kernels must not read (pad columns, rows >= B of a fragment-major x, cache rows past t).  Every pointer, stride and
position handed to a kernel is in bounds by construction; the refusal tests only take paths that return before a launch."""
import math

import pytest
import torch

import decode_reference as R

pytestmark = pytest.mark.gpu
BF, F32, F64 = R.BF, R.F32, R.F64
SENT = 7.0
EINVAL, OK = -1, 0
NAN = math.nan


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from asr_hip import lib
    lib.load()
    return lib


def dev(x, dtype=None):
    return (x if dtype is None else x.to(dtype)).cuda()


class Guarded:
    """n elements filled with a sentinel, 64 guard elements either side.  written(mask): the bits outside `mask` have not changed."""

    def __init__(self, n, dtype, fill=SENT):
        self.buf = torch.full((n + 128,), fill, dtype=dtype, device="cuda")
        self.t = self.buf[64:64 + n]
        self.before = self.buf.clone()
        self.n = n

    def untouched_outside(self, mask=None):
        m = torch.zeros(self.n + 128, dtype=torch.bool)
        if mask is not None:
            m[64:64 + self.n] = mask.reshape(-1)
        a, b = self.buf.cpu(), self.before.cpu()
        return R.same_bits(a[~m], b[~m])


def eq(got, want):
    """bit-for-bit as values: got (device, bf16 / fp32) against float64 `want` (-0 == 0)."""
    return bool(torch.equal(got.detach().to(F64).cpu(), want.to(F64)))


# ================================================================================================ 2.1 asr_dec_gemm
def run_gemm(ops, c, d):
    """Launch one GEMM case in the layouts it names; returns (out (B, N) on the CPU in its dtype, x_out or None).  Asserts the sentinels."""
    K, N, B = c["K"], c["N"], c["B"]
    kw = {}
    if c["w"] == "row":                                   # ldw > K, NaN in the pad columns and in a guard row after the last row
        Wb = torch.full((N + 1, K + 8), NAN, dtype=BF)
        Wb[:N, :K] = d["W"].to(BF)
        W = Wb.cuda()[:N, :K]
    else:
        W = R.pack(d["W"].to(BF)).cuda()
        kw["w_frag"] = (N, K)
    if c["pro"] == 0:
        if c["x"] == "row":
            xb = torch.full((B, K + 8), NAN, dtype=BF)
            xb[:, :K] = d["x"].to(BF)
            kw["x"] = xb.cuda()[:, :K]
        else:
            kw["x"], kw["x_frag"] = R.pack(d["x"].to(BF), fill=NAN).cuda(), True            # rows >= B: NaN
    elif c["pro"] == 1:
        kw["ln"] = (dev(d["Y"]), dev(d["R"]), dev(d["gamma"], F32), dev(d["beta"], F32), d.get("eps", 1e-5))
    else:
        state = torch.tensor([d["t"], 5], dtype=torch.int64, device="cuda")
        kw["embed"] = (dev(d["tok"]), dev(d["table"], F32), dev(d["pe"], F32), d.get("scale", 0.5), state)
    xg = None
    if c.get("x_out"):
        xg = Guarded(32 * K, BF)
        kw["x_out"] = xg.t.view(32, K)[:B]
    odt = F32 if c["f32"] else BF
    if c["o"] == "row":
        ldo = (N + 3) // 4 * 4 + 4
        og = Guarded(32 * ldo, odt)
        out = og.t.view(32, ldo)[:B, :N]
        mask = torch.zeros(32, ldo, dtype=torch.bool)
        mask[:B, :N] = True
    else:
        og = Guarded(32 * N, odt)
        out = og.t
        kw.update(out_frag=True, B=B)
        mask = torch.zeros(32 * N, dtype=torch.bool)
        mask[R.frag_index(32, N)[:B].reshape(-1)] = True
    ops.dec_gemm(W, None if d["bias"] is None else dev(d["bias"], F32), out, relu=c["relu"], **kw)
    torch.cuda.synchronize()
    assert og.untouched_outside(mask), "%s: out written outside its B x N elements" % R.gemm_id(c)
    got = out.cpu() if c["o"] == "row" else R.unpack(og.t.cpu(), 32, N)[:B]
    x_out = None
    if xg is not None:
        xm = torch.zeros(32, K, dtype=torch.bool)
        xm[:B] = True
        assert xg.untouched_outside(xm), "%s: x_out written outside its B rows" % R.gemm_id(c)
        x_out = xg.t.view(32, K)[:B].cpu()
    if c["pro"] == 2:
        assert kw["embed"][4].tolist() == [d["t"], 5]
    return got, x_out


def check_exact(ops, c):
    d = R.gemm_exact_case(c)
    got, x_out = run_gemm(ops, c, d)
    assert eq(got, d["want"]), "%s: %d of %d elements differ from float64" % (R.gemm_id(c), int((got.double() != d["want"]).sum()), got.numel())
    if x_out is not None:
        assert eq(x_out, d["x"]), "%s: x_out" % R.gemm_id(c)


@pytest.mark.parametrize("group,f32", R.GEMM_SYMBOLS, ids=["%s-%s" % (g, "f32" if f else "bf16") for g, f in R.GEMM_SYMBOLS])
def test_dec_gemm_exact_every_value_with_every_kernel(ops, group, f32):
    for c in R.GEMM_TABLES[(group, f32)]:
        check_exact(ops, c)


@pytest.mark.parametrize("c", R.SHIPPED, ids=[R.gemm_id(c) for c in R.SHIPPED])
def test_dec_gemm_exact_shipped_combinations(ops, c):
    check_exact(ops, c)


def test_dec_gemm_exact_layernorm_prologue(ops):
    for c in R.PRO1_EXACT:
        check_exact(ops, c)


def test_dec_gemm_exact_embedding_prologue(ops):
    for c in R.PRO2_EXACT:
        check_exact(ops, c)


RANDOM_GEMM = [dict(pro=0, K=K, N=N, B=B, f32=f32, bias=True, relu=relu, w=w, x=x, o="row", seed=50 + i)
               for i, (K, N, B, f32, relu, w, x) in enumerate(((512, 100, 32, True, False, "frag", "row"), (448, 33, 5, False, True, "row", "row"),
                                                              (960, 96, 31, True, True, "row", "frag"), (704, 35, 32, False, False, "frag", "frag"),
                                                              (2048, 100, 32, False, True, "frag", "frag"), (640, 33, 7, True, False, "row", "row")))]


def _random_gemm_operands(c):
    g = torch.Generator().manual_seed(1000 + c["seed"])
    K, N, B = c["K"], c["N"], c["B"]
    return dict(x=torch.randn(B, K, generator=g).to(BF).double(), W=(torch.randn(N, K, generator=g) * K ** -0.5).to(BF).double(),
                bias=torch.randn(N, generator=g).double() if c["bias"] else None)


@pytest.mark.parametrize("c", RANDOM_GEMM, ids=[R.gemm_id(c) for c in RANDOM_GEMM])
def test_dec_gemm_random_operands_inside_the_fp32_bound(ops, c):
    d = _random_gemm_operands(c)
    got, _ = run_gemm(ops, c, d)
    r = R.gemm_ratio(got, d["x"], d["W"], None if d["bias"] is None else d["bias"].float(), c["relu"])
    print("DECODE_ARMS gemm %-44s error / bound %.3f" % (R.gemm_id(c), r))
    assert r <= 1.0


@pytest.mark.parametrize("B,K,form", [(32, 512, "vocab"), (7, 320, "w1"), (1, 64, "row"), (31, 128, "row")])
def test_dec_gemm_layernorm_prologue_real_gamma_beta(ops, B, K, form):
    """x_out is asr_add_ln_fwd's output bit for bit and inside that kernel's float64 bound; the GEMM is bounded ON the stored x_out."""
    g = torch.Generator().manual_seed(B * 7 + K)
    N, f32, bias, relu, o = {"vocab": (100, True, False, False, "row"), "w1": (48, False, True, True, "frag"), "row": (35, False, True, False, "row")}[form]
    c = dict(pro=1, K=K, N=N, B=B, f32=f32, bias=bias, relu=relu, w="frag", x="row", o=o, x_out=True, seed=0)
    d = dict(Y=torch.randn(B, K, generator=g).to(BF), R=(2 * torch.randn(B, K, generator=g)).to(BF), gamma=1 + 0.2 * torch.randn(K, generator=g),
             beta=0.3 * torch.randn(K, generator=g), W=(torch.randn(N, K, generator=g) * K ** -0.5).to(BF).double(),
             bias=torch.randn(N, generator=g).double() if bias else None, eps=1e-5)
    got, x_out = run_gemm(ops, c, d)
    x_k, _, _ = ops.add_ln_fwd(d["Y"].cuda().clone(), d["R"].cuda(), d["gamma"].cuda(), d["beta"].cuda())
    assert torch.equal(x_out, x_k.cpu())
    rl = R.ln_ratio(x_out, d["Y"], d["R"], d["gamma"], d["beta"], 1e-5)
    rg = R.gemm_ratio(got, x_out.double(), d["W"], None if d["bias"] is None else d["bias"].float(), relu)
    print("DECODE_ARMS ln-prologue B%d K%d %-5s x_out error / bound %.3f, gemm error / bound %.3f" % (B, K, form, rl, rg))
    assert rl <= 1.0 and rg <= 1.0


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384, 448, 512])
def test_layernorm_prologues_are_add_ln_fwd_bit_for_bit(ops, K):
    """include/asr_hip.h promises that the LayerNorm prologue of asr_dec_gemm and of asr_dec_attn_fused gives asr_add_ln_fwd's bits.
    A summation order or a contracted multiply-add that differs moves 1 element in 100 000 by a bf16 ulp (measured on the kernels
    before they were matched: 15 of 1.6 M), so this compares 20 seeds x 32 rows at every width: 1.6 M elements per prologue over the
    eight widths -- about 16 expected differences for such a defect, none allowed.  Zero weights: only x_out is looked at."""
    B = 32
    W = torch.zeros(64, K, dtype=BF, device="cuda")
    out = torch.zeros(B, 64, dtype=BF, device="cuda")
    kc = torch.zeros(B, 1, 64, dtype=BF, device="cuda")
    W3, ks, vs = torch.zeros(192, K, dtype=BF, device="cuda"), kc.clone(), kc.clone()      # the self-attention instantiation, t = 0
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    differ_gemm = differ_fused = differ_self = 0
    for seed in range(20):
        g = torch.Generator().manual_seed(seed * 100 + K)
        Y, Rr = torch.randn(B, K, generator=g).to(BF).cuda(), (2 * torch.randn(B, K, generator=g)).to(BF).cuda()
        gamma, beta = (1 + 0.2 * torch.randn(K, generator=g)).cuda(), (0.3 * torch.randn(K, generator=g)).cuda()
        xg, xf, xs = (torch.zeros(B, K, dtype=BF, device="cuda") for _ in range(3))
        ops.dec_gemm(W, None, out, ln=(Y, Rr, gamma, beta, 1e-5), x_out=xg)
        ops.dec_attn_fused(W, None, kc, kc, out, 1, 64, 0.125, ln=(Y, Rr, gamma, beta, 1e-5), x_out=xf, self_attention=False)
        ops.dec_attn_fused(W3, None, ks, vs, out, 1, 64, 0.125, ln=(Y, Rr, gamma, beta, 1e-5), x_out=xs, state=state, self_attention=True)
        x_k, _, _ = ops.add_ln_fwd(Y.clone(), Rr, gamma, beta)
        differ_gemm += int((xg != x_k).sum())
        differ_fused += int((xf != x_k).sum())
        differ_self += int((xs != x_k).sum())
    print("DECODE_ARMS K=%d x_out elements that differ from asr_add_ln_fwd, of %d: asr_dec_gemm %d, asr_dec_attn_fused cross %d, self %d" %
          (K, 20 * B * K, differ_gemm, differ_fused, differ_self))
    assert differ_gemm == 0 and differ_fused == 0 and differ_self == 0


def test_dec_gemm_embedding_prologue_real_table(ops):
    """fp32 table / pe whose products and sums are exact in fp32 (multiples of 2^-6 below 8, scale 0.5): x_out is the float64 value rounded once."""
    g = torch.Generator().manual_seed(3)
    B, K, N = 9, 512, 96
    c = dict(pro=2, K=K, N=N, B=B, f32=False, bias=True, relu=False, w="frag", x="row", o="row", x_out=True, seed=0)
    table = torch.randint(-512, 513, (R.EMB_V, K), generator=g).double() / 64
    pe = torch.randint(-512, 513, (R.PE_ROWS, K), generator=g).double() / 64
    d = dict(tok=torch.randint(0, R.EMB_V, (B,), generator=g), table=table, pe=pe, t=3, scale=0.5, W=(torch.randn(N, K, generator=g) * K ** -0.5).to(BF).double(),
             bias=torch.randn(N, generator=g).double())
    got, x_out = run_gemm(ops, c, d)
    x64 = R.embed(d["tok"], table, pe, 0.5, 3)
    assert torch.equal(x64.float().double(), x64) and eq(x_out, R.rb(x64))
    r = R.gemm_ratio(got, x_out.double(), d["W"], d["bias"].float(), False)
    print("DECODE_ARMS embed-prologue gemm error / bound %.3f" % r)
    assert r <= 1.0


# ================================================================================================ 2.2 asr_dec_attn
def run_attn(ops, q, K, V, scale, H, state=None, k_new=None, v_new=None, frag=False, pads=False, shared=False, qkv_slice=False):
    """q (B, HD), K / V (B | 1, rows, HD) bf16 on the CPU.  pads: ldq / ld_new / cache row stride / ldo wider than H 64 with NaN in the pad
    columns (sentinel for out).  Returns (out (B, HD) on the CPU, the two device caches as given to the kernel)."""
    B, HD = q.shape
    rows = K.shape[1]
    pad = 8 if pads else 0

    def wide(x):                                          # (..., HD) -> a view of a buffer with `pad` NaN columns per row
        if not pad:
            return x.cuda().contiguous()
        b = torch.full(x.shape[:-1] + (HD + pad,), NAN, dtype=BF)
        b[..., :HD] = x
        return b.cuda()[..., :HD]
    if qkv_slice:                                         # q | k_new | v_new as slices of one (B, 3 HD + pad) buffer, like the model's qkv
        b = torch.full((B, 3 * HD + pad), NAN, dtype=BF)
        b[:, :HD] = q
        if k_new is not None:
            b[:, HD:2 * HD], b[:, 2 * HD:3 * HD] = k_new, v_new
        b = b.cuda()
        qd = b[:, :HD]
        knd, vnd = (b[:, HD:2 * HD], b[:, 2 * HD:3 * HD]) if k_new is not None else (None, None)
    else:
        qd = wide(q)
        knd, vnd = (wide(k_new), wide(v_new)) if k_new is not None else (None, None)
    Kd, Vd = wide(K), wide(V)
    if shared:
        assert K.shape[0] == 1
        Kd, Vd = Kd.expand(B, rows, HD), Vd.expand(B, rows, HD)
    K0, V0 = Kd.clone(), Vd.clone()
    if frag:
        og = Guarded(32 * HD, BF)
        out = og.t
        mask = torch.zeros(32 * HD, dtype=torch.bool)
        mask[R.frag_index(32, HD)[:B].reshape(-1)] = True
    else:
        ldo = HD + pad
        og = Guarded(B * ldo, BF)
        out = og.t.view(B, ldo)[:, :HD]
        mask = torch.zeros(B, ldo, dtype=torch.bool)
        mask[:, :HD] = True
    ops.dec_attn(qd, Kd, Vd, out, H, 64, scale, k_new=knd, v_new=vnd, state=state, out_frag=frag)
    torch.cuda.synchronize()
    assert og.untouched_outside(mask), "attention output written outside its rows"
    got = R.unpack(og.t.cpu(), 32, HD)[:B] if frag else out.cpu()
    return got, (Kd, Vd, K0, V0)


def caches_unchanged(c4, except_row=None):
    Kd, Vd, K0, V0 = [x.cpu() for x in c4]
    if except_row is not None:
        keep = torch.ones(Kd.shape[1], dtype=torch.bool)
        keep[except_row] = False
        Kd, Vd, K0, V0 = Kd[:, keep], Vd[:, keep], K0[:, keep], V0[:, keep]
    return R.same_bits(Kd, K0) and R.same_bits(Vd, V0)


@pytest.mark.parametrize("launch", [0, 1, 2, 3])
def test_dec_attn_one_hot_on_every_key_position_of_three_passes(ops, launch):
    """B 33 x H 8 workgroups, rows 1025: four launches put the one-hot on every key position 0..1024.  out EQUALS V[j*]: j* in a later
    pass than keys of score 0 pins the rescale (corr = exp(-128) = 0), j* in pass 0 pins that the later passes add nothing."""
    c = R.onehot_case(1025, 33, 8, launch)
    got, c4 = run_attn(ops, c["q"], c["K"], c["V"], c["scale"], 8)
    bad = (R.bits(got) != R.bits(c["want"])).view(33, 8, 64).any(-1)
    assert not bad.any(), "wrong rows at (sequence, head, j*): %s" % [(int(b), int(h), int(c["js"][b, h])) for b, h in bad.nonzero()[:8]]
    assert caches_unchanged(c4)


@pytest.mark.parametrize("rows", [600, 1025])
def test_dec_attn_two_hot_across_passes_and_key_groups(ops, rows):
    c = R.twohot_case(rows, 5, 8)
    got, _ = run_attn(ops, c["q"], c["K"], c["V"], c["scale"], 8)
    assert R.same_bits(got, c["want"])


@pytest.mark.parametrize("Lk", [1, 2, 32, 512, 1024])
def test_dec_attn_uniform_every_key_counts_once(ops, Lk):
    c = R.uniform_case(Lk, 3, 2)
    got, _ = run_attn(ops, c["q"], c["K"], c["V"], c["scale"], 2)
    assert R.same_bits(got, c["want"])


@pytest.mark.parametrize("t", [0, 31, 32, 511, 512, 1024])
def test_dec_attn_self_one_hot_on_the_appended_row(ops, t):
    """Cache rows >= t hold NaN before the call; afterwards row t of both caches is k_new / v_new bit for bit, every other row keeps its
    bits (NaN rows included), and out = v_new."""
    g = torch.Generator().manual_seed(t)
    B, H, rows = 2, 8, t + 3
    HD = H * 64
    K = torch.zeros(B, rows, HD)
    V = torch.randn(B, rows, HD, generator=g)
    K[:, t:], V[:, t:] = NAN, NAN
    q, k_new = torch.full((B, HD), 4.0).to(BF), torch.full((B, HD), 4.0).to(BF)
    v_new = torch.randn(B, HD, generator=g).to(BF)
    state = torch.tensor([t, 9], dtype=torch.int64, device="cuda")
    got, c4 = run_attn(ops, q, K.to(BF), V.to(BF), 0.125, H, state=state, k_new=k_new, v_new=v_new, qkv_slice=True, pads=t % 2 == 1)
    assert R.same_bits(got, v_new)
    assert R.same_bits(c4[0][:, t].cpu(), k_new) and R.same_bits(c4[1][:, t].cpu(), v_new)
    assert caches_unchanged(c4, except_row=t) and state.tolist() == [t, 9]


def test_dec_attn_state_without_new_rows_and_state_beyond_the_cache(ops):
    """state with k_new == NULL: rows 0..t are attended (rows past t hold NaN), nothing is written.  state[0] >= rows: every row is
    attended and the caches stay untouched even when k_new / v_new are given."""
    rows, t, B, H = 40, 36, 5, 2
    c = R.onehot_case(t + 1, B, H, 0)
    K = torch.full((B, rows, H * 64), NAN, dtype=BF)
    V = K.clone()
    K[:, :t + 1], V[:, :t + 1] = c["K"], c["V"]
    state = torch.tensor([t, 0], dtype=torch.int64, device="cuda")
    got, c4 = run_attn(ops, c["q"], K, V, c["scale"], H, state=state)
    assert R.same_bits(got, c["want"]) and caches_unchanged(c4)
    for ts in (rows, rows + 5):
        c = R.onehot_case(rows, B, H, 1)
        state = torch.tensor([ts, 0], dtype=torch.int64, device="cuda")
        poison = torch.full((B, H * 64), NAN, dtype=BF)
        got, c4 = run_attn(ops, c["q"], c["K"], c["V"], c["scale"], H, state=state, k_new=poison, v_new=poison)
        assert R.same_bits(got, c["want"]) and caches_unchanged(c4)


@pytest.mark.parametrize("H,B,frag,shared", [(1, 1, True, False), (1, 33, False, True), (2, 5, True, True), (2, 33, False, False), (8, 1, False, True),
                                             (8, 5, True, False), (8, 32, True, False)])
def test_dec_attn_layouts(ops, H, B, frag, shared):
    """q as a slice of a wider qkv buffer; ldq, cache row stride and ldo wider than H 64 with NaN / sentinel pads; batch stride 0 (the
    encoder keys shared by every sequence); fragment-major output whose slots of rows >= B keep their bits."""
    rows = 70
    c = R.onehot_case(rows, B, H, 0, seed=H)
    K, V, want = c["K"], c["V"], c["want"]
    if shared:                                            # one key / value set: the j* of sequence b must come from q, so q is one-hot too
        K = torch.zeros(1, rows, H, 64)
        for j in range(rows):
            K[0, j, :, j % 64] = 1024.0 if j < 64 else 0.0
        V = c["V"][:1]
        g = torch.Generator().manual_seed(B)
        js = torch.randint(0, 64, (B, H), generator=g)
        q = torch.zeros(B, H, 64)
        q[torch.arange(B).view(B, 1), torch.arange(H).view(1, H), js] = 1.0          # score(j*) = 1024 / 8 = 128, the others 0
        c = dict(q=q.view(B, H * 64).to(BF), scale=0.125)
        K = K.view(1, rows, H * 64).to(BF)
        want = V.view(1, rows, H, 64)[0][js, torch.arange(H).view(1, H)].reshape(B, H * 64)
    got, _ = run_attn(ops, c["q"], K, V, c["scale"], H, frag=frag, pads=True, shared=shared, qkv_slice=not shared)
    assert R.same_bits(got, want)


@pytest.mark.parametrize("Lk", [33, 513, 1100])
def test_dec_attn_random_operands_inside_the_attention_bound(ops, Lk):
    c = R.bounded_case(Lk, 5, 8)
    ref, bound = R.attn_bound(c["q"], c["K"], c["V"], c["scale"])
    got, _ = run_attn(ops, c["q"], c["K"], c["V"], c["scale"], 8)
    r = R.ratio(got, ref, bound)
    print("DECODE_ARMS attn L=%d error / bound %.3f" % (Lk, r))
    assert r <= 1.0
    # the same keys as a self-attention at t = L - 1 (last row appended by the launch)
    state = torch.tensor([Lk - 1, 0], dtype=torch.int64, device="cuda")
    K, V = c["K"].clone(), c["V"].clone()
    K[:, Lk - 1], V[:, Lk - 1] = NAN, NAN
    got, c4 = run_attn(ops, c["q"], K, V, c["scale"], 8, state=state, k_new=c["K"][:, Lk - 1], v_new=c["V"][:, Lk - 1])
    r = R.ratio(got, ref, bound)
    print("DECODE_ARMS attn self t=%d error / bound %.3f" % (Lk - 1, r))
    assert r <= 1.0 and R.same_bits(c4[0].cpu(), c["K"]) and R.same_bits(c4[1].cpu(), c["V"])


# ================================================================================================ 2.3 asr_dec_attn_fused
def run_fused(ops, d, frag=False, pad=False, shared=False, x_out=True):
    """One asr_dec_attn_fused launch of a case of decode_reference; returns (out (B, HD), x_out or None, k cache, v cache, before, before)."""
    B, H, D, rows = d["B"], d["H"], d["D"], d["rows"]
    HD = H * 64
    self_attn = d["mode"] != "cross"
    kc, vc = d["kc"], d["vc"]
    if shared:
        kc, vc = kc[:1].cuda().expand(B, rows, HD), vc[:1].cuda().expand(B, rows, HD)
    else:
        kc, vc = kc.cuda(), vc.cuda()
    k0, v0 = kc.clone(), vc.clone()
    kw = {}
    state = None
    if d["mode"] == "embed":
        kw["embed"] = (dev(d["tok"]), dev(d["table"], F32), dev(d["pe"], F32), d["emb_scale"])
    else:
        kw["ln"] = (dev(d["Y"]), dev(d["R"]), dev(d["gamma"], F32), dev(d["beta"], F32), d.get("eps", 1e-5))
    if self_attn:
        state = torch.tensor([d["t"], 3], dtype=torch.int64, device="cuda")
    xg = None
    if x_out:
        xg = Guarded(B * D, BF)
        kw["x_out"] = xg.t.view(B, D)
    if frag:
        og = Guarded(32 * HD, BF)
        out = og.t
        mask = torch.zeros(32 * HD, dtype=torch.bool)
        mask[R.frag_index(32, HD)[:B].reshape(-1)] = True
    else:
        ldo = HD + (8 if pad else 0)
        og = Guarded(B * ldo, BF)
        out = og.t.view(B, ldo)[:, :HD]
        mask = torch.zeros(B, ldo, dtype=torch.bool)
        mask[:, :HD] = True
    ops.dec_attn_fused(dev(d["W"], BF), None if d["bias"] is None else dev(d["bias"], F32), kc, vc, out, H, 64, d["scale"], state=state,
                       self_attention=self_attn, out_frag=frag, **kw)
    torch.cuda.synchronize()
    assert og.untouched_outside(mask), "fused attention output written outside its rows"
    if xg is not None:
        assert xg.untouched_outside(torch.ones(B * D, dtype=torch.bool))
    if state is not None:
        assert state.tolist() == [d["t"], 3]
    got = R.unpack(og.t.cpu(), 32, HD)[:B] if frag else out.cpu()
    return got, (xg.t.view(B, D).cpu() if xg is not None else None), kc.cpu(), vc.cpu(), k0.cpu(), v0.cpu()


def check_fused_caches(d, kc, vc, k0, v0):
    """self: row t of both caches is the float64 projection rounded ONCE, every other row keeps its bits; cross: nothing is written."""
    if d["mode"] == "cross":
        assert R.same_bits(kc, k0) and R.same_bits(vc, v0)
        return
    t = d["t"]
    assert eq(kc[:, t], d["k"]) and eq(vc[:, t], d["v"]), "appended row differs from float64 rounded once"
    keep = torch.ones(d["rows"], dtype=torch.bool)
    keep[t] = False
    assert R.same_bits(kc[:, keep], k0[:, keep]) and R.same_bits(vc[:, keep], v0[:, keep])


# (mode, D, rows, t, H, B, fragment-major out, ldo > H 64, x_out): every D, rows, t in {0, 63, 64, rows - 1} and H of the issue's sweep
FUSED_SWEEP = [("ln", 64, 1, 0, 1, 5, False, True, True), ("ln", 128, 63, 62, 2, 3, True, False, False), ("ln", 192, 64, 63, 8, 2, False, False, True),
               ("ln", 320, 65, 64, 2, 32, True, False, True), ("ln", 512, 511, 510, 1, 5, False, True, True), ("ln", 512, 512, 511, 8, 2, True, False, True),
               ("embed", 64, 512, 64, 2, 3, False, True, True), ("embed", 128, 65, 63, 8, 2, True, False, True), ("embed", 192, 511, 0, 1, 5, False, False, False),
               ("embed", 320, 64, 0, 2, 3, False, False, True), ("embed", 512, 512, 511, 8, 2, False, True, True), ("embed", 512, 63, 62, 1, 32, True, False, True),
               ("cross", 64, 512, None, 8, 2, True, False, True), ("cross", 128, 1, None, 1, 5, False, True, True), ("cross", 192, 63, None, 2, 3, False, False, False),
               ("cross", 320, 511, None, 2, 3, True, False, True), ("cross", 512, 65, None, 8, 2, False, True, True), ("cross", 512, 64, None, 1, 32, True, False, True)]


@pytest.mark.parametrize("mode,D,rows,t,H,B,frag,pad,xo", FUSED_SWEEP, ids=["%s-D%d-rows%d-t%s-H%d-B%d%s%s" % (s[0], s[1], s[2], s[3], s[4], s[5], "-frag" if s[6] else "", "-pad" if s[7] else "")
                                                                             for s in FUSED_SWEEP])
def test_dec_attn_fused_exact_projections(ops, mode, D, rows, t, H, B, frag, pad, xo):
    """Integer x and W: the appended key / value rows and x_out are exact; the attention output is inside the worst-case form of the
    attention bound on the reference's (here: the exact) q / k / v.  Cross arms run on caches shared by every sequence (batch stride 0)."""
    d = R.fused_exact_case(mode, D, rows, t, B, H, seed=D // 64 + H)
    shared = mode == "cross"
    if shared:
        d["keys"], d["values"] = d["keys"][:1].expand(B, -1, -1), d["values"][:1].expand(B, -1, -1)
    got, x_out, kc, vc, k0, v0 = run_fused(ops, d, frag=frag, pad=pad, shared=shared, x_out=xo)
    if xo:
        assert eq(x_out, d["x"])
    check_fused_caches(d, kc, vc, k0, v0)
    ref, bound = R.attn_bound(d["q"], d["keys"], d["values"], d["scale"], worst_case=True)      # two or three keys carry the softmax: see attn_bound
    r = R.ratio(got, ref, bound)
    print("DECODE_ARMS fused exact-projection %-6s D%d rows%d error / worst-case bound %.3f" % (mode, D, rows, r))
    assert r <= 1.0


@pytest.mark.parametrize("mode,launch", [("cross", 0), ("cross", 1), ("cross", 2), ("cross", 3), ("ln", 0), ("ln", 1), ("ln", 2), ("ln", 3), ("ln", "t"), ("embed", 0), ("embed", "t")])
def test_dec_attn_fused_one_hot_through_the_projection(ops, mode, launch):
    """W_q is a single 1 in column 0 and x[0] = 4: q = 4 in every channel, out = V[j*].  B 16 x H 8 workgroups, four launches sweep j*
    over every position of the 512 rows (self attention: of the 511 cached rows at t = 511; `t`: j* = t with W_k = W_q, and then
    out = bf16(W_v x + b_v))."""
    t = None if mode == "cross" else 511
    d = R.fused_exact_case(mode, 128, 512, t, 16, 8, seed=2 if launch in (1, "t") else 1, onehot=launch)
    got, x_out, kc, vc, k0, v0 = run_fused(ops, d, frag=launch == 2)
    bad = (got.double() != d["want"]).view(16, 8, 64).any(-1)
    assert not bad.any(), "wrong rows at (sequence, head, j*): %s" % [(int(b), int(h), int(d["js"][b, h])) for b, h in bad.nonzero()[:8]]
    assert eq(x_out, d["x"])
    check_fused_caches(d, kc, vc, k0, v0)


@pytest.mark.parametrize("D", [64, 512])
def test_dec_attn_fused_cross_arm_returns_the_argmax_row(ops, D):
    d = R.cross_argmax_case(D, 5, 8)
    got, x_out, kc, vc, k0, v0 = run_fused(ops, d, pad=True)
    assert R.same_bits(got, d["want"]) and eq(x_out, d["x"]) and R.same_bits(kc, k0) and R.same_bits(vc, v0)


@pytest.mark.parametrize("mode,D,rows,t,H", [("ln", 512, 300, 299, 8), ("ln", 192, 65, 17, 2), ("embed", 512, 512, 511, 2), ("embed", 128, 64, 0, 1),
                                             ("cross", 512, 512, None, 8), ("cross", 320, 37, None, 2)])
def test_dec_attn_fused_random_operands_inside_the_attention_bound(ops, mode, D, rows, t, H):
    B = 3
    d = R.fused_bounded_case(mode, D, rows, t, B, H)
    got, x_out, kc, vc, k0, v0 = run_fused(ops, d)
    if mode == "embed":
        x64 = R.embed(d["tok"], d["table"], d["pe"], d["emb_scale"], t)
        # one fp32 multiply-add (fused or not: at most two fp32 roundings of the terms) and one bf16 rounding, elementwise
        xb = 2.0 ** -8 * x64.abs() + 2.0 ** -22 * ((d["table"].double()[d["tok"]] * d["emb_scale"]).abs() + d["pe"].double()[t].abs())
        assert R.ratio(x_out, x64, xb) <= 1.0
    else:
        x_k, _, _ = ops.add_ln_fwd(d["Y"].cuda().clone(), d["R"].cuda(), d["gamma"].cuda(), d["beta"].cuda())
        assert torch.equal(x_out, x_k.cpu())
        assert R.ln_ratio(x_out, d["Y"], d["R"], d["gamma"], d["beta"], 1e-5) <= 1.0
    q, k, v, keys, values = R.fused(d["W"], d["bias"], x_out.double(), d["kc"], d["vc"], H, d["scale"], mode != "cross", t)
    if mode != "cross":                                   # the appended rows: the projection on the stored x, one rounding
        HD = H * 64
        rk = R.gemm_ratio(kc[:, t], x_out.double(), d["W"][HD:2 * HD].double(), d["bias"][HD:2 * HD], False)
        rv = R.gemm_ratio(vc[:, t], x_out.double(), d["W"][2 * HD:].double(), d["bias"][2 * HD:], False)
        print("DECODE_ARMS fused %-6s D%d appended k / v error / bound %.3f %.3f" % (mode, D, rk, rv))
        assert rk <= 1.0 and rv <= 1.0
        keep = torch.ones(rows, dtype=torch.bool)
        keep[t] = False
        assert R.same_bits(kc[:, keep], k0[:, keep]) and R.same_bits(vc[:, keep], v0[:, keep])
    ref, bound = R.attn_bound(q, keys, values, d["scale"])
    r = R.ratio(got, ref, bound)
    print("DECODE_ARMS fused %-6s D%d rows%d error / bound %.3f" % (mode, D, rows, r))
    assert r <= 1.0


# ================================================================================================ 2.4 asr_dec_finish
def finish_call(L, logits, V, tok, done, out, B, max_len, eos, state, ticket):
    return L.load().asr_dec_finish(L.ptr(logits), logits.stride(0), V, L.ptr(tok), L.ptr(done), L.ptr(out), B, max_len, eos, L.ptr(state), L.ptr(ticket),
                                   L.stream())


@pytest.mark.parametrize("V,B", [(1, 1), (5, 6), (255, 33), (256, 33), (257, 300), (4364, 33)])
def test_dec_finish_three_consecutive_calls(L, V, B):
    """Calls at t = max_len - 2, max_len - 1 (writes the last column) and max_len (out untouched; tok, done and state still move), on
    logits with ld > V and +inf in the pad columns, ties, -inf rows, NaN, the EOS column and `done` set beforehand."""
    max_len = 4
    tokg, doneg, outg = Guarded(B, torch.int64, -7), Guarded(B, torch.uint8, 0x55), Guarded(max_len * B, torch.int64, -7)
    doneg.t.zero_()
    preset = torch.zeros(B, dtype=torch.bool)
    preset[B // 2] = True
    doneg.t.copy_(preset.to(torch.uint8))
    state = torch.tensor([max_len - 2, 11], dtype=torch.int64, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    done_ref, out_ref = preset.clone(), torch.full((max_len, B), -7, dtype=torch.int64)
    for call in range(3):
        t = max_len - 2 + call
        lg, eos = R.finish_case(V, B, 3, seed=call)
        lgd = lg.cuda()
        assert finish_call(L, lgd, V, tokg.t, doneg.t, outg.t, B, max_len, eos, state, ticket) == OK
        torch.cuda.synchronize()
        tok_ref, done_ref, out_ref = R.finish(lg, V, eos, t, max_len, done_ref, out_ref)
        assert torch.equal(tokg.t.cpu(), tok_ref), (call, (tokg.t.cpu() != tok_ref).nonzero().reshape(-1)[:8].tolist())
        assert torch.equal(doneg.t.cpu().bool(), done_ref) and torch.equal(outg.t.cpu().view(max_len, B), out_ref)
        assert state.tolist() == [t + 1, 11] and ticket.item() == 0
        assert bool(done_ref[B // 2])
    everything = torch.ones(1, dtype=torch.bool)
    assert tokg.untouched_outside(everything.expand(B)) and doneg.untouched_outside(everything.expand(B)) and outg.untouched_outside(everything.expand(max_len * B))
    assert bool((out_ref[:2] == -7).all()) and bool((out_ref[2:] >= 0).all())


def test_dec_finish_without_an_output_matrix(L):
    B, V = 6, 257
    lg, eos = R.finish_case(V, B, 3)
    tok = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    state = torch.tensor([0, 0], dtype=torch.int64, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert finish_call(L, lg.cuda(), V, tok, done, None, B, 1, eos, state, ticket) == OK
    torch.cuda.synchronize()
    tok_ref, done_ref, _ = R.finish(lg, V, eos, 0, 1, torch.zeros(B, dtype=torch.bool), None)
    assert torch.equal(tok.cpu(), tok_ref) and torch.equal(done.cpu().bool(), done_ref) and state.tolist() == [1, 0] and ticket.item() == 0


# ================================================================================================ 2.5 asr_kv_append, asr_decode_prepare
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("ncols", [1, 64, 257, 512])
def test_kv_append_rows_and_positions(L, dtype, ncols):
    g = torch.Generator().manual_seed(ncols)
    B, max_len = 3, 5
    src = torch.randn(B, 2 * ncols + 3, generator=g).to(dtype)
    for t in (0, max_len - 1, max_len, max_len + 7):
        kg, vg = Guarded(B * max_len * ncols, dtype), Guarded(B * max_len * ncols, dtype)
        sd = src.cuda()
        ks, vs = sd[:, :ncols], sd[:, ncols:2 * ncols]
        state = torch.tensor([t, 2], dtype=torch.int64, device="cuda")
        rc = L.load().asr_kv_append(L.ptr(ks), L.ptr(vs), sd.stride(0), L.ptr(kg.t), L.ptr(vg.t), B, ncols, max_len, L.ptr(state), L.dt_of(dtype), L.stream())
        assert rc == OK
        torch.cuda.synchronize()
        k0 = torch.full((B, max_len, ncols), SENT, dtype=dtype)
        kr, vr = R.kv_append(src[:, :ncols], src[:, ncols:2 * ncols], k0, k0.clone(), t)
        assert R.same_bits(kg.t.cpu().view(B, max_len, ncols), kr) and R.same_bits(vg.t.cpu().view(B, max_len, ncols), vr)
        assert kg.untouched_outside(torch.ones(kg.n, dtype=torch.bool)) and vg.untouched_outside(torch.ones(vg.n, dtype=torch.bool))
        assert state.tolist() == [t, 2]


@pytest.mark.parametrize("D", [1, 512, 1025])
@pytest.mark.parametrize("B", [0, 1, 1500])
def test_decode_prepare_row_and_key_lengths(L, D, B):
    g = torch.Generator().manual_seed(D + B)
    T = 4
    pe = torch.randn(T, D, generator=g)
    ped = pe.cuda()
    for t in (0, T - 1):
        cur, kl = Guarded(D, F32), Guarded(max(B, 1), torch.int32, -7)
        state = torch.tensor([t, 4], dtype=torch.int64, device="cuda")
        assert L.load().asr_decode_prepare(L.ptr(ped), D, L.ptr(cur.t), L.ptr(kl.t), B, L.ptr(state), 0, L.stream()) == OK
        torch.cuda.synchronize()
        row, lens = R.prepare(pe, t, B)
        assert R.same_bits(cur.t.cpu(), row) and torch.equal(kl.t.cpu()[:B], lens) and state.tolist() == [t, 4]
        m = torch.zeros(max(B, 1), dtype=torch.bool)
        m[:B] = True
        assert cur.untouched_outside(torch.ones(D, dtype=torch.bool)) and kl.untouched_outside(m)
    state = torch.tensor([T - 1, 4], dtype=torch.int64, device="cuda")
    assert L.load().asr_decode_prepare(None, 0, None, None, 0, L.ptr(state), 1, L.stream()) == OK           # advance with null pe: only state[0]
    torch.cuda.synchronize()
    assert state.tolist() == [T, 4]


# ================================================================================================ 2.6 argument errors
class GemmArgs:
    """A valid asr_dec_gemm call on sentinel-filled buffers; with(...) overrides arguments by name."""
    NAMES = ("W", "ldw", "bias", "out", "ldo", "B", "N", "K", "relu", "out_dtype", "layout", "prologue", "X", "ldx", "Y", "R", "gamma", "beta", "eps", "x_out",
             "tok", "table", "pe", "scale", "state")

    def __init__(self, L, K=128, N=32, B=4):
        self.L = L
        z = lambda *s, dt=BF: torch.full(s, SENT, dtype=dt, device="cuda")          # noqa: E731
        self.t = dict(W=z(N + 32, 2304), bias=z(N, dt=F32), out=z(40, 64), X=z(32, 2304), Y=z(32, 640), R=z(32, 640), gamma=z(640, dt=F32), beta=z(640, dt=F32),
                      x_out=z(32, 640), tok=torch.zeros(32, dtype=torch.int64, device="cuda"), table=z(4, 640, dt=F32), pe=z(4, 640, dt=F32),
                      state=torch.zeros(2, dtype=torch.int64, device="cuda"))
        self.before = {k: v.clone() for k, v in self.t.items()}
        p = {k: L.ptr(v) for k, v in self.t.items()}
        self.base = dict(W=p["W"], ldw=2304, bias=p["bias"], out=p["out"], ldo=64, B=B, N=N, K=K, relu=0, out_dtype=L.BF16, layout=0, prologue=0, X=p["X"], ldx=2304,
                         Y=None, R=None, gamma=None, beta=None, eps=1e-5, x_out=None, tok=None, table=None, pe=None, scale=1.0, state=None)
        self.p = p

    def call(self, **over):
        a = dict(self.base, **over)
        return self.L.load().asr_dec_gemm(*[a[n] for n in self.NAMES], self.L.stream())

    def untouched(self):
        torch.cuda.synchronize()
        return all(R.same_bits(v.cpu(), self.before[k].cpu()) for k, v in self.t.items() if k not in ("tok", "state")) and self.t["state"].tolist() == [0, 0]


def test_dec_gemm_argument_errors(L):
    a = GemmArgs(L)
    p, U = a.p, L.EUNSUPPORTED
    ln = dict(prologue=1, X=None, Y=p["Y"], R=p["R"], gamma=p["gamma"], beta=p["beta"])
    emb = dict(prologue=2, X=None, tok=p["tok"], table=p["table"], pe=p["pe"], state=p["state"])
    cases = [("B = 33", dict(B=33), U), ("K % 64", dict(K=96), U), ("K = 1088: 17 steps on 4 waves", dict(K=1088), U), ("K = 2176: 17 steps on 8 waves", dict(K=2176), U),
             ("prologue with K = 576", dict(ln, K=576), U), ("embedding prologue with K = 576", dict(emb, K=576), U),
             ("X fragment with a prologue", dict(ln, layout=2), EINVAL), ("fragment output with fp32", dict(layout=4, out_dtype=L.F32), EINVAL),
             ("fragment output with N % 16", dict(layout=4, N=24), U), ("ldo % 4", dict(ldo=62), U), ("ldw % 8", dict(ldw=2300), U),
             ("misaligned W", dict(W=p["W"] + 2), U), ("misaligned out", dict(out=p["out"] + 2), U), ("misaligned X", dict(X=p["X"] + 2), U),
             ("misaligned x_out", dict(ln, x_out=p["x_out"] + 2), EINVAL), ("ldx % 8", dict(ldx=2300), U),
             ("prologue 1 without gamma", dict(ln, gamma=None), EINVAL), ("prologue 1 without Y", dict(ln, Y=None), EINVAL),
             ("prologue 2 without state", dict(emb, state=None), EINVAL), ("prologue 2 without tok", dict(emb, tok=None), EINVAL),
             ("ldx < K", dict(ldx=64), EINVAL), ("null X", dict(X=None), EINVAL), ("dtype 5", dict(out_dtype=5), EINVAL), ("layout 8", dict(layout=8), EINVAL),
             ("layout -1", dict(layout=-1), EINVAL), ("prologue 3", dict(prologue=3), EINVAL), ("null W", dict(W=None), EINVAL), ("null out", dict(out=None), EINVAL),
             ("N = 0", dict(N=0), EINVAL), ("K = 0", dict(K=0), EINVAL), ("B = -1", dict(B=-1), EINVAL),
             ("row-major ldw < K", dict(ldw=64), EINVAL), ("row-major ldo < N", dict(ldo=16), EINVAL), ("B = 0", dict(B=0), OK), ("B = 0 with a prologue", dict(ln, B=0), OK)]
    for what, over, want in cases:
        assert a.call(**over) == want, what
    assert a.untouched()


def test_dec_attn_argument_errors(L):
    z = lambda *s: torch.full(s, SENT, dtype=BF, device="cuda")                    # noqa: E731
    B, H, rows = 2, 2, 4
    HD = H * 64
    t = dict(q=z(40, HD + 8), kn=z(40, HD), vn=z(40, HD), kc=z(40, rows, HD), vc=z(40, rows, HD), out=z(40, HD + 8))
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    before = {k: v.clone() for k, v in t.items()}
    p = {k: L.ptr(v) for k, v in t.items()}
    names = ("q", "ldq", "k_new", "v_new", "ld_new", "k_cache", "v_cache", "cbs", "cld", "rows", "out", "ldo", "B", "H", "dk", "scale", "out_frag", "state")
    base = dict(q=p["q"], ldq=HD + 8, k_new=None, v_new=None, ld_new=0, k_cache=p["kc"], v_cache=p["vc"], cbs=rows * HD, cld=HD, rows=rows, out=p["out"], ldo=HD + 8, B=B, H=H,
                dk=64, scale=0.125, out_frag=0, state=None)
    U = L.EUNSUPPORTED
    new = dict(k_new=p["kn"], v_new=p["vn"], ld_new=HD, state=L.ptr(state))
    cases = [("dk = 32", dict(dk=32), U), ("k_new without v_new", dict(new, v_new=None), EINVAL), ("v_new without k_new", dict(new, k_new=None), EINVAL),
             ("k_new without state", dict(new, state=None), EINVAL), ("odd ldq", dict(ldq=HD + 4), U), ("odd ldo", dict(ldo=HD + 4), U), ("odd cache row stride", dict(cld=HD + 4), U),
             ("odd cache batch stride", dict(cbs=rows * HD + 4), U), ("odd ld_new", dict(new, ld_new=HD + 4), U), ("misaligned q", dict(q=p["q"] + 2), U),
             ("misaligned k_new", dict(new, k_new=p["kn"] + 2), U), ("rows = 0", dict(rows=0), EINVAL), ("H = 0", dict(H=0), EINVAL), ("null out", dict(out=None), EINVAL),
             ("fragment output with B = 33", dict(out_frag=1, B=33), U), ("B = 0", dict(B=0), OK)]
    for what, over, want in cases:
        a = dict(base, **over)
        assert L.load().asr_dec_attn(*[a[n] for n in names], L.stream()) == want, what
    torch.cuda.synchronize()
    assert all(R.same_bits(v.cpu(), before[k].cpu()) for k, v in t.items())


def test_dec_attn_fused_argument_errors(L):
    z = lambda *s, dt=BF: torch.full(s, SENT, dtype=dt, device="cuda")             # noqa: E731
    B, H, rows, D = 2, 2, 4, 640
    HD = H * 64
    t = dict(W=z(3 * HD, D), bias=z(3 * HD, dt=F32), Y=z(40, D), R=z(40, D), gamma=z(D, dt=F32), beta=z(D, dt=F32), table=z(4, D, dt=F32), pe=z(4, D, dt=F32), x_out=z(40, D),
             kc=z(40, rows, HD), vc=z(40, rows, HD), out=z(40, HD))
    tok, state = torch.zeros(40, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    before = {k: v.clone() for k, v in t.items()}
    p = {k: L.ptr(v) for k, v in t.items()}
    names = ("W", "bias", "D", "self", "Y", "R", "gamma", "beta", "eps", "tok", "table", "pe", "emb_scale", "x_out", "k_cache", "v_cache", "cbs", "cld", "rows", "out", "ldo",
             "B", "H", "dk", "scale", "out_frag", "state")
    base = dict(W=p["W"], bias=p["bias"], D=128, self=1, Y=p["Y"], R=p["R"], gamma=p["gamma"], beta=p["beta"], eps=1e-5, tok=None, table=None, pe=None, emb_scale=1.0,
                x_out=p["x_out"], k_cache=p["kc"], v_cache=p["vc"], cbs=rows * HD, cld=HD, rows=rows, out=p["out"], ldo=HD, B=B, H=H, dk=64, scale=0.125, out_frag=0,
                state=L.ptr(state))
    emb = dict(Y=None, R=None, gamma=None, beta=None, tok=L.ptr(tok), table=p["table"], pe=p["pe"])
    U = L.EUNSUPPORTED
    cases = [("rows = 513", dict(rows=513), U), ("D = 576", dict(D=576), U), ("D = 96", dict(D=96), U), ("dk = 32", dict(dk=32), U),
             ("embed with self_attention = 0", dict(emb, self=0), EINVAL), ("embed without pe", dict(emb, pe=None), EINVAL), ("LN without beta", dict(beta=None), EINVAL),
             ("LN without Y", dict(Y=None), EINVAL), ("self without state", dict(state=None), EINVAL), ("embed without state", dict(emb, state=None), EINVAL),
             ("fragment output with B = 33", dict(out_frag=1, B=33), U), ("odd ldo", dict(ldo=HD + 4), U), ("odd cache row stride", dict(cld=HD + 4), U),
             ("misaligned W", dict(W=p["W"] + 2), U), ("misaligned x_out", dict(x_out=p["x_out"] + 2), U), ("misaligned gamma", dict(gamma=p["gamma"] + 4), U),
             ("rows = 0", dict(rows=0), EINVAL), ("D = 0", dict(D=0), EINVAL), ("null W", dict(W=None), EINVAL), ("B = 0", dict(B=0), OK), ("B = 0, cross", dict(B=0, self=0, state=None), OK)]
    for what, over, want in cases:
        a = dict(base, **over)
        assert L.load().asr_dec_attn_fused(*[a[n] for n in names], L.stream()) == want, what
    torch.cuda.synchronize()
    assert all(R.same_bits(v.cpu(), before[k].cpu()) for k, v in t.items()) and state.tolist() == [0, 0]


def test_dec_finish_kv_append_and_prepare_argument_errors(L):
    B, V = 3, 8
    lg = torch.full((B, V), SENT, device="cuda")
    tok = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    out = torch.full((2, B), -7, dtype=torch.int64, device="cuda")
    state = torch.tensor([0, 6], dtype=torch.int64, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.load().asr_dec_finish(L.ptr(lg), V - 1, V, L.ptr(tok), L.ptr(done), L.ptr(out), B, 2, 2, L.ptr(state), L.ptr(ticket), L.stream()) == EINVAL, "ld < V"
    assert L.load().asr_dec_finish(L.ptr(lg), V, V, L.ptr(tok), L.ptr(done), L.ptr(out), B, 0, 2, L.ptr(state), L.ptr(ticket), L.stream()) == EINVAL, "max_len = 0"
    assert L.load().asr_dec_finish(L.ptr(lg), V, V, L.ptr(tok), L.ptr(done), L.ptr(out), B, 2, 2, L.ptr(state), None, L.stream()) == EINVAL, "null ticket"
    assert L.load().asr_dec_finish(L.ptr(lg), V, V, L.ptr(tok), L.ptr(done), L.ptr(out), B, 2, 2, None, L.ptr(ticket), L.stream()) == EINVAL, "null state"
    assert L.load().asr_dec_finish(L.ptr(lg), V, 0, L.ptr(tok), L.ptr(done), L.ptr(out), B, 2, 2, L.ptr(state), L.ptr(ticket), L.stream()) == EINVAL, "V = 0"
    assert L.load().asr_dec_finish(None, V, V, L.ptr(tok), L.ptr(done), L.ptr(out), B, 2, 2, L.ptr(state), L.ptr(ticket), L.stream()) == EINVAL, "null logits"
    assert L.load().asr_dec_finish(L.ptr(lg), V, V, L.ptr(tok), L.ptr(done), L.ptr(out), 0, 2, 2, L.ptr(state), L.ptr(ticket), L.stream()) == OK, "B = 0"
    src, cache = torch.full((B, V), SENT, device="cuda"), torch.full((B, 2, V), SENT, device="cuda")
    kv = lambda **o: L.load().asr_kv_append(*[dict(dict(k=L.ptr(src), v=L.ptr(src), ld=V, kc=L.ptr(cache), vc=L.ptr(cache), B=B, n=V, ml=2, st=L.ptr(state), dt=L.F32), **o)[n]   # noqa: E731
                                              for n in ("k", "v", "ld", "kc", "vc", "B", "n", "ml", "st", "dt")], L.stream())
    assert kv(dt=5) == EINVAL and kv(k=None) == EINVAL and kv(vc=None) == EINVAL and kv(st=None) == EINVAL and kv(n=0) == EINVAL and kv(ml=0) == EINVAL and kv(B=-1) == EINVAL
    assert kv(B=0) == OK
    cur, kl = torch.full((V,), SENT, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
    prep = lambda **o: L.load().asr_decode_prepare(*[dict(dict(pe=L.ptr(lg), D=V, cur=L.ptr(cur), kl=L.ptr(kl), B=B, st=L.ptr(state), adv=0), **o)[n]                          # noqa: E731
                                                     for n in ("pe", "D", "cur", "kl", "B", "st", "adv")], L.stream())
    assert prep(st=None) == EINVAL and prep(st=None, adv=1) == EINVAL and prep(pe=None) == EINVAL and prep(cur=None) == EINVAL and prep(kl=None) == EINVAL
    assert prep(D=0) == EINVAL and prep(B=-1) == EINVAL
    torch.cuda.synchronize()
    assert state.tolist() == [0, 6] and ticket.item() == 0 and bool((tok == -7).all()) and bool((out == -7).all()) and bool((cache == SENT).all())
    assert bool((cur == SENT).all()) and bool((kl == -7).all()) and not bool(done.any())
