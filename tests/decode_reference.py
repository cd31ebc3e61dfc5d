"""Float64 restatement of the bf16 decode step (csrc/decode.hip: asr_dec_gemm / asr_dec_attn / asr_dec_attn_fused / asr_dec_finish;
csrc/elementwise.hip: asr_kv_append / asr_decode_prepare) in plain torch on the CPU, the seeded case builders, and the checkers that
tests/test_gpu_decode_arms.py (kernel output) and tests/test_decode_reference_host.py (deliberately broken output) both use.

Written from the text of include/asr_hip.h, not from asr_hip/ops.py: frag_index is the header's offset formula, add_ln rounds z = Y + R
to bf16 before the statistics as the header says.  Every formula takes a dtype, so the SAME formula run in fp32 on the CPU gives the
fp32 part of a bound (tests/mwer_reference.py: bound32, excess -- the project's 4 x rule).

Bounds (all derived, none fitted):
  GEMM, random operands   |got - ref64| <= bound32(ref64, ref32) (+ 2^-8 |ref64| for a bf16 output: one rounding).
  attention               |got - ref64| <= 2^-8 A + 2^-24 (2 + 1.5 S) A + bound32, elementwise, where
                          A[e] = sum_j softmax_j |v_j[e]|  (|out[e]| <= A[e]: 2^-9 A for the probabilities rounded to bf16 before P V,
                          2^-9 A for the stored bf16 output) and S = the largest (max s - s_j) among keys with p_j >= 2^-24 (the fast
                          exponential rounds its argument (s_j - max) log2(e) to fp32: relative error of p_j up to 2^-24 * 1.4427 * S,
                          plus one ulp of the result and one of the normaliser: 2^-24 (2 + 1.5 S)).  Every random-operand arm is held
                          to this; attn_bound(worst_case=True) says why the integer sweep of the fused kernel takes 2^-7 A instead.
  exact arms              integer operands whose every partial sum is below 2^24: the fp32 result is the float64 one in any order, the
                          bf16 output is that value rounded ONCE; one-hot softmaxes whose other scores lie 128 below the maximum
                          (exp(-128) is 0 in fp32): the output row IS a value row."""
import math

import torch

from mwer_reference import BF16_REL, EPS32, bound32, excess  # noqa: F401  (re-exported: the tolerance rule of tests/test_gpu_mwer.py)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DK = 64
PASS = 512                      # keys per pass of asr_dec_attn, the limit of asr_dec_attn_fused
NEG = -math.inf


# ------------------------------------------------------------------------------------------------ roundings
def rb(x):
    """float64 -> the nearest bf16 value (ties to even), ONE rounding, returned as float64.  (torch's double -> bfloat16 cast goes
    through fp32: two roundings.)  Normal range only; zeros, infinities and NaN pass through."""
    x = x.to(F64)
    m, e = torch.frexp(x)                               # x = m 2^e, 0.5 <= |m| < 1: 8 significant bits -> ulp 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    r = torch.round(x / ulp) * ulp                      # torch.round: half to even
    return torch.where(torch.isfinite(x) & (x != 0), r, x)


def to_bf(x):
    """rb() as a bfloat16 tensor (exact: the value is representable)."""
    return rb(x).to(F32).to(BF)


def bits(t):
    """bf16 / fp32 tensor -> its bits (NaN payloads and the sign of zero included); integer tensors as they are."""
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


# ------------------------------------------------------------------------------------------------ fragment-major order
def frag_index(rows, K):
    """(rows, K) int64: element [row][col] of a fragment-major matrix sits at offset ((r K/16 + s) 64 + 32 h + i) 8 + e with
    r = row / 32, i = row % 32, s = col / 16, h = (col % 16) / 8, e = col % 8  (include/asr_hip.h)."""
    assert K % 16 == 0
    row = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    col = torch.arange(K, dtype=torch.int64).view(1, -1)
    r, i = row // 32, row % 32
    s, h, e = col // 16, (col % 16) // 8, col % 8
    return ((r * (K // 16) + s) * 64 + 32 * h + i) * 8 + e


def pack(w, fill=0.0):
    """(rows, K) -> flat fragment-major tensor of ceil(rows / 32) 32 K elements; the slots of the pad rows hold `fill`."""
    rows, K = w.shape
    rp = (rows + 31) // 32 * 32
    f = torch.full((rp * K,), fill, dtype=w.dtype)
    f[frag_index(rows, K).reshape(-1)] = w.reshape(-1)
    return f


def unpack(f, rows, K):
    return f[frag_index(rows, K).reshape(-1)].view(rows, K)


# ------------------------------------------------------------------------------------------------ operators
def gemm(x, W, bias=None, relu=False, dtype=F64):
    y = x.to(dtype) @ W.to(dtype).t()
    if bias is not None:
        y = y + bias.to(dtype)
    return y.relu() if relu else y


def add_ln(Y, R, gamma, beta, eps, dtype=F64, round_z=True):
    """LayerNorm(z) gamma + beta with z = bf16(Y + R) (rounded first; round_z = False is the host test's mutant).  Not rounded."""
    z = Y.to(F64) + R.to(F64)
    if round_z:
        z = rb(z)
    z = z.to(dtype)
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    return (z - mu) * torch.rsqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)


def embed(tok, table, pe, scale, t, dtype=F64):
    return table.to(dtype)[tok] * scale + pe.to(dtype)[t]


def _heads(x, H):
    return x.reshape(*x.shape[:-1], H, DK)


def attend(q, K, V, scale, dtype=F64, drop=None):
    """q (B, H 64), K / V (B, L, H 64) -> (out (B, H 64), A (B, H 64), S (B, H)).  drop = (b, h, j): that key is left out of the softmax
    of one (sequence, head) -- the host test's mutant."""
    B, HD = q.shape
    H = HD // DK
    qh = _heads(q.to(dtype), H)                                                  # (B, H, 64)
    Kh = _heads(K.to(dtype), H).permute(0, 2, 1, 3)                              # (B, H, L, 64)
    Vh = _heads(V.to(dtype), H).permute(0, 2, 1, 3)
    s = torch.einsum("bhd,bhjd->bhj", qh, Kh) * scale
    if drop is not None:
        s = s.clone()
        s[drop[0], drop[1], drop[2]] = NEG
    mx = s.max(-1, keepdim=True).values
    p = torch.softmax(s, -1)
    out = torch.einsum("bhj,bhjd->bhd", p, Vh).reshape(B, HD)
    A = torch.einsum("bhj,bhjd->bhd", p, Vh.abs()).reshape(B, HD)
    gap = torch.where(p >= 2.0 ** -24, mx - s, torch.zeros_like(s))
    return out, A, gap.max(-1).values


def attend_as_computed(q, K, V, scale, rescale=True):
    """The kernel's arithmetic restated in float64: passes of 512 keys with a running maximum, probabilities exp(s - max) rounded to
    bf16 before P V, their sum taken unrounded, one bf16 rounding at the end.  rescale = False skips the correction when the maximum
    moves (the host test's mutant).  Returns float64 (B, H 64)."""
    B, HD = q.shape
    H = HD // DK
    L = K.shape[1]
    qh = _heads(q.to(F64), H)
    Kh = _heads(K.to(F64), H).permute(0, 2, 1, 3)
    Vh = _heads(V.to(F64), H).permute(0, 2, 1, 3)
    s = torch.einsum("bhd,bhjd->bhj", qh, Kh) * scale
    run = torch.full((B, H, 1), NEG, dtype=F64)
    l = torch.zeros(B, H, 1, dtype=F64)
    acc = torch.zeros(B, H, DK, dtype=F64)
    for j0 in range(0, L, PASS):
        sp = s[:, :, j0:j0 + PASS]
        mx = torch.maximum(sp.max(-1, keepdim=True).values, run)
        if rescale:
            corr = torch.where(torch.isfinite(run), torch.exp(run - mx), torch.zeros_like(run))
            l, acc = l * corr, acc * corr
        run = mx
        p = torch.exp(sp - mx)
        p = torch.where(p < 2.0 ** -149, torch.zeros_like(p), p)              # fp32's range: exp(-128) is 0 there
        l = l + p.sum(-1, keepdim=True)
        acc = acc + torch.einsum("bhj,bhjd->bhd", rb(p), Vh[:, :, j0:j0 + PASS])
    return rb(acc / l).reshape(B, HD)


def attn_bound(q, K, V, scale, worst_case=False):
    """(ref64 (B, H 64), elementwise bound) of the attention rule in the module docstring: 2^-9 A per bf16 rounding, the rule every
    random-operand arm is held to.  worst_case: 2^-8 A per rounding -- bf16 keeps 8 significant bits, so just above a power of two half
    an ulp is 2^-8 of the value, not 2^-9.  Random operands stay well inside the 2^-9 rule (the roundings of hundreds of
    probabilities average out); the integer sweep of asr_dec_attn_fused does not: there two or three probabilities carry the whole
    softmax (0.73 / 0.27 ...), and the float64 restatement of the correct algorithm (attend_as_computed) itself reaches 1.19 x the
    2^-9 rule (tests/test_decode_reference_host.py).  That sweep, whose output the rule was not written for, uses worst_case."""
    ref, A, S = attend(q, K, V, scale)
    ref32 = attend(q, K, V, scale, dtype=F32)[0]
    b32 = bound32(ref, ref32)
    Se = S.unsqueeze(-1).expand(-1, -1, DK).reshape(ref.shape)
    return ref, (2.0 ** -7 if worst_case else 2.0 ** -8) * A + 2.0 ** -24 * (2.0 + 1.5 * Se) * A + b32


def ratio(got, ref, bound):
    """max |got - ref| / bound; a non-finite got counts +inf."""
    got = got.detach().to(F64).cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not torch.isfinite(got).all():
        return math.inf
    return float(((got - ref).abs() / bound).max())


def gemm_ratio(got, x, W, bias, relu):
    """error / bound of a GEMM output on random operands (got fp32: the 4 x rule; got bf16: plus one rounding)."""
    ref = gemm(x, W, bias, relu)
    return excess(got, ref, bound32(ref, gemm(x, W, bias, relu, dtype=F32)), bf16_stored=got.dtype == BF)


def ln_ratio(got, Y, R, gamma, beta, eps):
    """error / bound of the LayerNorm prologue's x_out against float64: 4 x the fp32 restatement's error plus one bf16 rounding (the rule
    tests/test_gpu_rowwise_arms.py holds asr_add_ln_fwd to)."""
    ref = add_ln(Y, R, gamma, beta, eps)
    b32 = 4.0 * float((add_ln(Y, R, gamma, beta, eps, dtype=F32).double() - ref).abs().max())
    return excess(got, ref, b32, bf16_stored=True)


def fused(W, bias, x, kc, vc, H, scale, self_attention, t=None):
    """asr_dec_attn_fused after its prologue: x (B, D) float64 (the stored bf16 row), W ((3 | 1) H 64, D), caches (B | 1, rows, H 64).
    The projected q / k / v are rounded to bf16 as the kernel rounds them.  self: rows 0..t-1 of the caches and the projected row at t
    -> (q, k_t, v_t, keys, values); cross: (q, None, None, keys, values) with every cache row."""
    HD = H * DK
    B = x.shape[0]
    proj = rb(gemm(x, W, bias))
    q = proj[:, :HD]
    kc, vc = kc.to(F64).expand(B, -1, -1), vc.to(F64).expand(B, -1, -1)
    if not self_attention:
        return q, None, None, kc, vc
    k, v = proj[:, HD:2 * HD], proj[:, 2 * HD:]
    return q, k, v, torch.cat([kc[:, :t], k.unsqueeze(1)], 1), torch.cat([vc[:, :t], v.unsqueeze(1)], 1)


def finish(logits, V, eos, t, max_len, done, out, highest=False):
    """(tok, done, out) after asr_dec_finish: arg max over the first V columns with the lowest index on ties; a NaN is never chosen; a
    row with no column greater than -inf gives 0.  out (max_len, B) or None; t >= max_len leaves it alone.  highest: the host mutant."""
    x = logits[:, :V].to(F64)
    x = torch.where(torch.isnan(x), torch.full_like(x, NEG), x)
    mx = x.max(1, keepdim=True).values
    hit = (x == mx) & (mx > NEG)
    if highest:
        tok = V - 1 - hit.flip(1).to(torch.int8).argmax(1)
    else:
        tok = hit.to(torch.int8).argmax(1)
    tok = torch.where(hit.any(1), tok, torch.zeros_like(tok)).to(torch.int64)
    done = done.clone() | (tok == eos)
    if out is not None:
        out = out.clone()
        if t < max_len:
            out[t] = tok
    return tok, done, out


def kv_append(k_src, v_src, k_cache, v_cache, t):
    k_cache, v_cache = k_cache.clone(), v_cache.clone()
    if t < k_cache.shape[1]:
        k_cache[:, t], v_cache[:, t] = k_src, v_src
    return k_cache, v_cache


def prepare(pe, t, B):
    return pe[t].clone(), torch.full((B,), t + 1, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ GEMM cases
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


K_GROUPS = {"w4s8": (64, 128, 448, 512), "w4s16": (576, 704, 960), "w8s16": (640, 1024, 2048)}      # the three PRO 0 kernels
# K steps of 16 per wave: live registers of the GS loop
K_STEPS = {64: 1, 128: 2, 448: 7, 512: 8, 576: 9, 704: 11, 960: 15, 640: 5, 1024: 8, 2048: 16, 320: 5}
N_ROW, N_FRAG, B_ALL = (1, 33, 35, 96, 100), (16, 48), (1, 31, 32)


def _table(group, f32):
    """Cases of one kernel symbol in which every K of the group, bias given / NULL, ReLU on / off, W / x row-major (padded) and
    fragment-major, every N and every B appear at least once (attributes cycle with co-prime periods)."""
    Ks = K_GROUPS[group]
    Ns = [(n, "row") for n in N_ROW] + ([] if f32 else [(n, "frag") for n in N_FRAG])
    out = []
    for i, (N, o) in enumerate(Ns + Ns[:1]):
        out.append(dict(pro=0, K=Ks[i % len(Ks)], N=N, B=B_ALL[i % 3], f32=f32, bias=i % 2 == 0, relu=(i // 2) % 2 == 1,
                        w="frag" if i % 3 == 1 else "row", x="frag" if i % 4 >= 2 else "row", o=o, seed=i))
    return out


# the six arm combinations FusedGreedyDecoder._step launches (asr_hip/decode.py), at small N
SHIPPED = [
    dict(name="wqkv-embed", pro=2, K=512, N=96, B=31, f32=False, bias=True, relu=False, w="frag", x="row", o="row", x_out=True),
    dict(name="wqkv-ln", pro=1, K=512, N=96, B=32, f32=False, bias=True, relu=False, w="frag", x="row", o="row", x_out=True),
    dict(name="wo-w2-xfrag", pro=0, K=2048, N=96, B=31, f32=False, bias=True, relu=False, w="frag", x="frag", o="row"),
    dict(name="wq_c-ln", pro=1, K=512, N=100, B=5, f32=False, bias=True, relu=False, w="frag", x="row", o="row", x_out=True),
    dict(name="w1-ln-relu-fragout", pro=1, K=512, N=48, B=31, f32=False, bias=True, relu=True, w="frag", x="row", o="frag", x_out=True),
    dict(name="vocab-ln-f32", pro=1, K=512, N=100, B=32, f32=True, bias=False, relu=False, w="frag", x="row", o="row", x_out=False),
]
for _i, _c in enumerate(SHIPPED):
    _c["seed"] = 100 + _i

GEMM_SYMBOLS = [(g, f32) for g in K_GROUPS for f32 in (True, False)]
GEMM_TABLES = {(g, f32): _table(g, f32) for g, f32 in GEMM_SYMBOLS}

# prologue 1 exactly: K x {vocabulary form, w1 form, row-major bf16} x W fragment- / row-major; x_out alternates
PRO1_EXACT = [dict(pro=1, K=K, N=N, B=B_ALL[(a + b + c) % 3], f32=f32, bias=bias, relu=relu, w=w, x="row", o=o, x_out=(a + b + c) % 2 == 0, seed=a * 9 + b * 3 + c)
              for a, K in enumerate((64, 128, 320, 512))
              for b, (N, f32, bias, relu, o) in enumerate(((100, True, False, False, "row"), (48, False, True, True, "frag"), (35, False, True, False, "row")))
              for c, w in enumerate(("frag", "row"))]
# prologue 2 exactly: position 0 and the last row of pe
PRO2_EXACT = [dict(pro=2, K=K, N=N, B=B, f32=f32, bias=True, relu=relu, w=w, x="row", o=o, x_out=xo, t=t, seed=i)
              for i, (K, N, B, f32, relu, w, o, xo, t) in enumerate(((64, 33, 1, True, False, "row", "row", True, 0), (512, 96, 31, False, False, "frag", "row", True, "last"),
                                                                    (320, 48, 32, False, True, "frag", "frag", False, "last"), (128, 100, 5, True, True, "row", "row", True, 0)))]
PE_ROWS, EMB_V = 7, 11


def gemm_id(c):
    return c.get("name") or "p%d-K%d-N%d-B%d-%s%s%s-W%s-x%s-o%s%s" % (c["pro"], c["K"], c["N"], c["B"], "f32" if c["f32"] else "bf16", "-bias" if c["bias"] else "",
                                                                        "-relu" if c["relu"] else "", c["w"], c["x"], c["o"], "-xout" if c.get("x_out") else "")


def gemm_exact_case(c):
    """Integer operands of a GEMM case (float64 tensors of exactly representable values): x in [-2, 2] (prologue 1: beta, with gamma =
    0 and arbitrary finite Y, R; prologue 2: an even-integer table with scale 0.5 plus integer pe), W in [-2, 2], bias in [-8, 8].  Every
    partial sum is at most 4 * 2048 < 2^24.  `want`: the float64 result (rounded once for a bf16 output)."""
    g = _gen(c["pro"], c["K"], c["N"], c["B"], c["seed"])
    K, N, B = c["K"], c["N"], c["B"]
    d = dict(W=_ints(g, (N, K), -2, 2), bias=_ints(g, (N,), -8, 8) if c["bias"] else None)
    if c["pro"] == 0:
        d["x"] = _ints(g, (B, K), -2, 2)
    elif c["pro"] == 1:
        d["Y"] = torch.randn(B, K, generator=g).to(BF)
        d["R"] = (2 * torch.randn(B, K, generator=g)).to(BF)
        d["gamma"] = torch.zeros(K)
        d["beta"] = _ints(g, (K,), -2, 2)
        d["x"] = d["beta"].expand(B, K).clone()
    else:
        d["tok"] = torch.randint(0, EMB_V, (B,), generator=g)
        d["table"] = _ints(g, (EMB_V, K), -1, 1) * 2                       # * scale 0.5 + pe -> [-2, 2]
        d["pe"] = _ints(g, (PE_ROWS, K), -1, 1)
        d["t"] = PE_ROWS - 1 if c.get("t") == "last" else 0
        d["x"] = embed(d["tok"], d["table"], d["pe"], 0.5, d["t"])
    want = gemm(d["x"], d["W"], d["bias"], c["relu"])
    d["want"] = want if c["f32"] else rb(want)
    return d


# ------------------------------------------------------------------------------------------------ attention cases
def onehot_positions(rows, B, H, launch):
    """j* of every (sequence, head) of launch number `launch`: consecutive key positions, wrapped -- ceil(rows / (B H)) launches put a
    one-hot on every position."""
    return ((torch.arange(B * H) + launch * B * H) % rows).view(B, H)


def onehot_case(rows, B, H, launch, seed=0):
    """q = 4 in every channel, key j* = 4 in every channel, every other key 0, scale 1/8: score(j*) = 128, the others 0; values random
    bf16.  The output row must EQUAL V[j*]."""
    g = _gen(rows, B, H, launch, seed, 1)
    HD = H * DK
    js = onehot_positions(rows, B, H, launch)
    q = torch.full((B, HD), 4.0).to(BF)
    K = torch.zeros(B, rows, H, DK)
    K[torch.arange(B).view(B, 1), js, torch.arange(H).view(1, H)] = 4.0
    V = torch.randn(B, rows, HD, generator=g).to(BF)
    want = V.view(B, rows, H, DK)[torch.arange(B).view(B, 1), js, torch.arange(H).view(1, H)].reshape(B, HD)
    return dict(q=q, K=K.view(B, rows, HD).to(BF), V=V, js=js, want=want, scale=0.125)


def twohot_case(rows, B, H, seed=0):
    """Two keys of score 128 in different passes and different 32-key groups, integer values in [-4, 4]: out = bf16((v1 + v2) / 2)."""
    g = _gen(rows, B, H, seed, 2)
    HD = H * DK
    n = B * H
    assert rows >= PASS + 32
    i = torch.arange(n)
    j1 = (i * 37 + 5) % PASS                                                  # pass 0
    j2 = PASS + 32 * (i % ((rows - PASS) // 32)) + (j1 + 16) % 32             # a later pass, another key group
    j2[0] = rows - 1                                                          # the last key (rows = 1025: alone in the third pass)
    j1, j2 = j1.view(B, H), j2.view(B, H)
    assert bool((j1 // PASS != j2 // PASS).all()) and bool((j1 % 32 != j2 % 32).all()) and int(j2.max()) < rows
    K = torch.zeros(B, rows, H, DK)
    bi, hi = torch.arange(B).view(B, 1), torch.arange(H).view(1, H)
    K[bi, j1, hi] = 4.0
    K[bi, j2, hi] = 4.0
    V = _ints(g, (B, rows, H, DK), -4, 4)
    want = rb((V[bi, j1, hi] + V[bi, j2, hi]) / 2).reshape(B, HD)
    return dict(q=torch.full((B, HD), 4.0).to(BF), K=K.view(B, rows, HD).to(BF), V=V.view(B, rows, HD).to(BF), j1=j1, j2=j2, want=want.to(F32).to(BF), scale=0.125)


def uniform_case(L, B, H, seed=0):
    """q = 0: every key has probability 1 / L (L a power of two: the normaliser is exact); integer values in [-4, 4]; the output is the
    float64 mean rounded once, so every key counts exactly once."""
    g = _gen(L, B, H, seed, 3)
    HD = H * DK
    V = _ints(g, (B, L, HD), -4, 4)
    K = torch.randn(B, L, HD, generator=g).to(BF)
    return dict(q=torch.zeros(B, HD).to(BF), K=K, V=V.to(BF), want=to_bf(V.mean(1)), scale=0.125)


def bounded_case(L, B, H, seed=0):
    """Random operands.  The last key of every 512-key pass after the first is q scaled so that its score is the maximum so far plus
    1.5: the running maximum rises at every pass boundary and the correction factor lies strictly between 0 and 1 (near e^-1.5)."""
    g = _gen(L, B, H, seed, 4)
    HD = H * DK
    scale = DK ** -0.5
    q = torch.randn(B, HD, generator=g).to(BF)
    K = torch.randn(B, L, HD, generator=g).to(BF)
    V = torch.randn(B, L, HD, generator=g).to(BF)
    qh = _heads(q.to(F64), H)
    for j0 in range(PASS, L, PASS):
        j = min(j0 + PASS, L) - 1
        s = torch.einsum("bhd,bhjd->bhj", qh, _heads(K[:, :j0].to(F64), H).permute(0, 2, 1, 3)) * scale
        target = s.max(-1).values + 1.5                                       # (B, H)
        K[:, j] = (qh * (target / (scale * (qh * qh).sum(-1))).unsqueeze(-1)).reshape(B, HD).to(F32).to(BF)
    return dict(q=q, K=K, V=V, scale=scale)


def pass_maxima(c):
    """(B, H, passes) the largest score of every 512-key pass (the host test asserts they rise)."""
    B, HD = c["q"].shape
    H = HD // DK
    s = torch.einsum("bhd,bhjd->bhj", _heads(c["q"].to(F64), H), _heads(c["K"].to(F64), H).permute(0, 2, 1, 3)) * c["scale"]
    return torch.stack([s[:, :, j0:j0 + PASS].max(-1).values for j0 in range(0, s.shape[-1], PASS)], -1)


# ------------------------------------------------------------------------------------------------ fused cases
def fused_exact_case(mode, D, rows, t, B, H, seed=0, onehot=None):
    """Exact operands of asr_dec_attn_fused.  x: gamma = 0, beta integers in [-2, 2] (mode "ln" / "cross"), or integer table / pe with
    scale 0.5 ("embed").  W integers in [-1, 1], bias integers in [-4, 4] or None (odd seeds).  |projection| <= 2 D + 4 <= 1028, but
    only values up to 256 are bf16 integers: the builder asserts that rounding once is all that happens (rb of the float64 value).
    onehot = launch number: W_q is a single 1 in column 0 and x[0] = 4 (q = 4 in every channel), key j* = 4, the others 0, scale 1/8;
    self attention with j* = t: W_k = W_q.  Caches: integers in [-4, 4] (values) / [-1, 1] (keys), NaN in rows >= t for self."""
    g = _gen(D, rows, t if t is not None else 999, B, H, seed, 5 + ("ln", "embed", "cross").index(mode))
    self_attn = mode != "cross"
    HD = H * DK
    NP = 3 if self_attn else 1
    d = dict(mode=mode, D=D, rows=rows, t=t, B=B, H=H, scale=0.125)
    W = _ints(g, (NP * HD, D), -1, 1)
    d["bias"] = None if seed % 2 else _ints(g, (NP * HD,), -4, 4)
    xrow = _ints(g, (D,), -2, 2)
    if onehot is not None:
        xrow[0] = 4.0
        W[:HD] = 0.0
        W[:HD, 0] = 1.0
        if d["bias"] is not None:
            d["bias"][:HD] = 0.0
    if mode == "embed":
        d["tok"] = torch.randint(0, EMB_V, (B,), generator=g)
        d["table"] = (xrow * 2).expand(EMB_V, D).clone()
        d["table"][:, 1:] += 2 * _ints(g, (EMB_V, D - 1), -1, 1)              # rows differ from column 1 on (column 0 stays 4 for a one-hot)
        d["pe"] = torch.zeros(max(rows, 1), D)
        d["pe"][:, 1:] = _ints(g, (max(rows, 1), D - 1), -1, 1)
        d["x"] = embed(d["tok"], d["table"], d["pe"], 0.5, t)
        d["emb_scale"] = 0.5
    else:
        d["Y"] = torch.randn(B, D, generator=g).to(BF)
        d["R"] = (2 * torch.randn(B, D, generator=g)).to(BF)
        d["gamma"], d["beta"] = torch.zeros(D), xrow
        d["x"] = xrow.expand(B, D).clone()
    kc = _ints(g, (B, rows, HD), -1, 1)
    vc = _ints(g, (B, rows, HD), -4, 4)
    if onehot is not None:
        kc = torch.zeros(B, rows, H, DK)
        if onehot == "t":                                  # self attention, j* = t: the key comes from the projection, W_k = W_q
            js = torch.full((B, H), t)
            W[HD:2 * HD] = W[:HD]
        else:                                              # j* sweeps the cached rows (self: 0..t-1, and k_t = 0)
            js = onehot_positions(t if self_attn else rows, B, H, onehot)
            kc[torch.arange(B).view(B, 1), js, torch.arange(H).view(1, H)] = 4.0
            if self_attn:
                W[HD:2 * HD] = 0.0
        if self_attn and d["bias"] is not None:
            d["bias"][HD:2 * HD] = 0.0
        kc = kc.view(B, rows, HD)
        d["js"] = js
    d["W"] = W
    if self_attn:
        kc[:, t:], vc[:, t:] = math.nan, math.nan
    d["kc"], d["vc"] = kc.to(BF), vc.to(BF)
    q, k, v, Ks, Vs = fused(W, d["bias"], d["x"], d["kc"], d["vc"], H, d["scale"], self_attn, t)
    exact = gemm(d["x"], W, d["bias"])
    assert float(exact.abs().max()) < 2 ** 24
    d["q"], d["k"], d["v"], d["keys"], d["values"] = q, k, v, Ks, Vs
    if onehot is not None:                                 # out = V[j*] (j* = t: the projected value row, rounded once)
        d["want"] = _heads(Vs, H)[torch.arange(B).view(B, 1), d["js"], torch.arange(H).view(1, H)].reshape(B, HD)
    return d


def cross_argmax_case(D, B, H, seed=0):
    """Cross arm: random integer W / bias, keys k_j = 1024 e_j (j < 64), scale 1/8: score_j = 128 q_j, so out = V[argmax_j q_j] exactly
    when the two largest q of a head differ (they are integers: by at least 1, 128 in the score).  The seed is advanced until they do."""
    for s in range(seed, seed + 200):
        d = fused_exact_case("cross", D, 64, None, B, H, seed=2 * s)
        HD = H * DK
        kc = torch.zeros(B, 64, H, DK)
        for j in range(64):
            kc[:, j, :, j] = 1024.0
        d["kc"] = kc.view(B, 64, HD).to(BF)
        q = _heads(rb(gemm(d["x"], d["W"], d["bias"])), H)                    # (B, H, 64)
        top = q.topk(2, -1).values
        if bool((top[..., 0] - top[..., 1] >= 1.0).all()) and bool((q == q.round()).all()):
            js = q.argmax(-1)
            V = d["vc"].view(B, 64, H, DK)
            d["js"] = js
            d["want"] = V[torch.arange(B).view(B, 1), js, torch.arange(H).view(1, H)].reshape(B, HD)
            d["q"] = q.reshape(B, HD)
            return d
    raise AssertionError("no seed with distinct top-two q")


def fused_bounded_case(mode, D, rows, t, B, H, seed=0):
    """Random operands of asr_dec_attn_fused (real gamma / beta, or a real table / pe)."""
    g = _gen(D, rows, t if t is not None else 999, B, H, seed, 9)
    self_attn = mode != "cross"
    HD = H * DK
    NP = 3 if self_attn else 1
    d = dict(mode=mode, D=D, rows=rows, t=t, B=B, H=H, scale=DK ** -0.5, eps=1e-5)
    d["W"] = (torch.randn(NP * HD, D, generator=g) * D ** -0.5).to(BF)
    d["bias"] = torch.randn(NP * HD, generator=g)
    if mode == "embed":
        d["tok"] = torch.randint(0, EMB_V, (B,), generator=g)
        d["table"], d["pe"], d["emb_scale"] = torch.randn(EMB_V, D, generator=g), torch.randn(rows, D, generator=g), 0.75
    else:
        d["Y"] = torch.randn(B, D, generator=g).to(BF)
        d["R"] = (2 * torch.randn(B, D, generator=g)).to(BF)
        d["gamma"], d["beta"] = 1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
    d["kc"] = torch.randn(B, rows, HD, generator=g).to(BF)
    d["vc"] = torch.randn(B, rows, HD, generator=g).to(BF)
    if self_attn:
        d["kc"][:, t:], d["vc"][:, t:] = math.nan, math.nan
    return d


# ------------------------------------------------------------------------------------------------ finish cases
def finish_case(V, B, ld_pad, seed=0):
    """Logits (B, V + ld_pad) with +inf in the pad columns, and row by row (cyclically): the maximum at column V - 1; at 255 / 256; a
    tie inside one thread's stride (v, v + 256); across lanes (v, v + 1); across waves (v, v + 64); an all -inf row; a NaN beside a
    finite maximum (and NaN in column 0); an all-NaN row; the EOS column; random."""
    g = _gen(V, B, ld_pad, seed, 11)
    x = torch.randn(B, V, generator=g)
    eos = min(2, V - 1)
    for b in range(B):
        k = b % 10
        if k == 0:
            x[b, V - 1] = 50.0
        elif k == 1:
            x[b, min(255 + (b // 10) % 2, V - 1)] = 50.0
        elif k == 2 and V > 256 + 3:
            x[b, 3] = x[b, 259] = 50.0
        elif k == 3 and V > 9:
            x[b, 8] = x[b, 9] = 50.0
        elif k == 4 and V > 5 + 64 * 3:
            x[b, 5 + 64 * 3] = x[b, 5 + 64] = 50.0
        elif k == 5:
            x[b] = NEG
        elif k == 6 and V > 1:
            x[b, 0] = math.nan
            x[b, V // 2] = 60.0
            if V // 2 + 1 < V:
                x[b, V // 2 + 1] = math.nan
        elif k == 7:
            x[b] = math.nan
        elif k == 8:
            x[b, eos] = 70.0
    buf = torch.full((B, V + ld_pad), math.inf)
    buf[:, :V] = x
    return buf, eos
