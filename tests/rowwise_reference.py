"""Plain references for the row-wise kernels: csrc/layernorm.hip, the embedding / optimiser kernels of csrc/elementwise.hip, csrc/ce.hip
(tests/test_rowwise_reference_host.py, tests/test_gpu_rowwise_arms.py).

keep_mask             NumPy restatement of asr_hash32 / asr_keep / asr_drop_threshold (csrc/common.h): index row * D + col, threshold
                      uint32(p * 2**32), kept iff hash >= threshold.  The device step counter comes from attn_reference.effective_seed.
add_ln_reference      z = round_to_storage(dropout(y) * inv_keep + res) restated in float32 (one multiply, one add, one round: the bits
                      of the kernel), then float64: statistics of the ROUNDED z (biased variance, eps inside the root),
                      out = (LN * gamma + beta + post[row % period]) * keep_row.
add_ln_bwd_reference  the closed form add_ln_bwd_kernel implements, mean and rstd as INPUTS (as the kernel has them).
embed_* / ce_* / adam_noam_reference   index_add_ in float64 with the PAD row left alone; lse / lowest-index argmax / three sums /
                      dlogits with sum_q = 1 - eps / V; one Adam step with the Noam rate.
Every reference takes `dt` (float64, or float32 for the CPU checks) and `order` (how rows and columns are summed: 0 = torch.sum, 1 = one
element after the other from the far end), and the deliberate defects of the CPU sensitivity check as keyword arguments.

Two kinds of cases.
EXACT (LN_EXACT, EMBED_CASES): integer data, ranges chosen so that every intermediate is representable in fp32
  (tests/test_rowwise_reference_host.py evaluates the reference in float32 in two summation orders and demands torch.equal with float64):
  any summation order and any FMA contraction give the same bits, and the GPU test demands torch.equal.
TOLERANCE (LN_TOL, CE_CASES): b32 = B32_FACTOR x the largest error of the float32 CPU evaluation (both orders) against float64 on the
  case's own data, per tensor; bf16 outputs add 2**-8 |ref| (one bf16 rounding, 2**-9 relative, doubled for a tie broken the other way).

Measured on the CPU (python -m pytest tests/test_rowwise_reference_host.py -s prints every figure).  b32 per tensor, variant p = 0.1 with
residual, post_add and row_keep, M = 53; `margin` = the smallest `defect error / bound` over the tensors a defect is looked for in, the
smallest over the five LayerNorm defects (one row left out of dgamma, mask index built with the wrong D, row_keep ignored, the last
lane's columns dropped from the row sums, post_period off by one); every margin is asserted to be above 1:

  LayerNorm      mean     rstd     out      d_res    d_y      dgamma   dbeta    smallest margin (largest per defect; which defect)
  f32  D   40    5.1e-07  4.2e-07  1.8e-06  1.4e-06  2.0e-06  2.7e-05  1.6e-05  1.4e+05 (one row left out of dgamma)
  f32  D  776    3.4e-07  1.1e-06  7.8e-06  5.0e-06  5.1e-06  2.3e-05  1.2e-05  2.5e+04 (last lane dropped)
  f32  D 1544    3.8e-07  2.0e-06  1.4e-05  1.2e-05  1.3e-05  3.3e-05  1.2e-05  1.8e+04 (last lane dropped)
  bf16 D   40    9.5e-08  7.6e-07  3.1e-06  2.1e-06  2.4e-06  1.0e-05  0        1.4e+05 (post_period off by one)
  bf16 D 1032    1.4e-08  1.3e-06  1.1e-05  5.5e-06  6.1e-06  2.6e-05  1.9e-06  3.6e+05 (post_period off by one)
  bf16 D 3080    2.1e-08  3.5e-06  2.3e-05  1.6e-05  1.8e-05  6.2e-05  9.5e-07  1.3e+05 (post_period off by one)
  (dbeta of bf16 D = 40: 53 bf16 values add exactly in fp32 in any order, the bound is 0 and demands equality.  The last lane dropped is
  seen on the mean, 2e4 .. 4e6 x its bound; on out / d_res it is 1.6e+02 .. 5e+05 x the bound.)

  Cross entropy, logits x 30; the float32 evaluation is torch's float32 log_softmax, and for dlogits also exp(l - lse) with that
  evaluation's lse stored in fp32, which is ce_bwd_kernel's interface (half an ulp of |lse| ~ 100 is 4e-6 relative on every probability
  of the row; exp(log_softmax) alone does not have this term and would give bounds 10 - 40 x smaller):
                      lse      loss sum (relative to sum |loss_i|)   dlogits   smoothing over V - 1: loss / dlogits / bf16 dlogits
  M  13 V   35 eps 0    8.4e-06  3.9e-07                               8.5e-07
  M  13 V   35 eps 0.1  8.4e-06  3.1e-07                               8.4e-07   8.2e+03 / 6.4e+02 / 5.7e+00
  M  13 V 4364 eps 0    1.4e-05  1.9e-07                               2.3e-06
  M  13 V 4364 eps 0.1  1.4e-05  5.8e-07                               2.3e-06   5.1e+01 / 2.0e+00 / 7.3e-03
  M 517 V   35 eps 0    1.5e-05  2.9e-07                               6.5e-08
  M 517 V   35 eps 0.1  1.5e-05  2.9e-07                               6.6e-08   9.8e+03 / 1.9e+02 / 4.4e+01
  M 517 V 4364 eps 0    2.8e-05  1.4e-06                               1.2e-07
  M 517 V 4364 eps 0.1  2.8e-05  1.6e-06                               1.2e-07   1.4e+01 / 8.2e-01 / 7.2e-03
  (smoothing over V - 1 classes is seen by the loss sum in every case, by the gradient at V = 35 only: at V = 4364 it moves sum_q by
  eps / V = 2e-5, about what the fp32 lse costs, and far below a bf16 rounding.)
  Embedding backward: the second 1024-position chunk skipped changes table rows 1, 4 and 5 of the five live rows (exact comparison).
  One non-zero pad column, or a NaN in one: exact comparison with 0 (pad_columns_clean).
  Adam: the honest fp32 step (every operation rounded, no contraction) stays inside |p - ref| <= 2**-23 |ref| + 2**-21 |update|, m and v
  inside 2**-22 relative, the rate inside 2**-22, for g and m of one sign (adam_inputs); a step count off by one leaves the rate bound.
These figures come from the CPU alone.
"""
import numpy as np
import torch

from attn_reference import effective_seed  # noqa: F401  (the device step counter, read back: used by the GPU tests)

B32_FACTOR = 4.0           # a different but legitimate summation order
BF16_REL = 2.0 ** -8       # one bf16 rounding (half an ulp = 2**-9 relative), doubled for a tie broken the other way
LN_EPS = float(np.float32(1e-5))
SEED = ((0x2468ACE + 17) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
_M32 = np.uint64(0xFFFFFFFF)
F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ dropout mask
def drop_threshold(p):
    """(thr, inv_keep): asr_drop_threshold of the C float p, and 1.f / (1.f - p) as the entry points compute it."""
    pf = np.float32(p)
    thr = 0 if pf <= 0 else min(int(float(pf) * 4294967296.0), 4294967295)
    return thr, float(np.float32(1.0) / (np.float32(1.0) - pf))


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def hash32(seed_eff, idx):
    """asr_hash32 on a uint64 index array."""
    seed_eff = int(seed_eff) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    x = (_mul32(idx & _M32, 0x9E3779B1) + _mul32(idx >> np.uint64(32), 0x85EBCA6B) + np.uint64(seed_eff & 0xFFFFFFFF)
         + np.uint64(((seed_eff >> 32) * 0xC2B2AE35) & 0xFFFFFFFF)) & _M32
    x ^= x >> np.uint64(15)
    x = _mul32(x, 0x2C1B3C6D)
    x ^= x >> np.uint64(12)
    x = _mul32(x, 0x297A2D39)
    x ^= x >> np.uint64(15)
    return x


def keep_mask(seed_eff, M, D, p, index_D=None):
    """bool (M, D): True where element (row, col) is kept.  index_D: the row stride of the index (a deliberate defect when it is not D)."""
    thr, _ = drop_threshold(p)
    if thr == 0:
        return np.ones((M, D), dtype=bool)
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(D if index_D is None else index_D) + np.arange(D, dtype=np.uint64)[None, :]
    return hash32(seed_eff, idx) >= np.uint64(thr)


# ------------------------------------------------------------------------------------------------ helpers
def rnd(x, dtype):
    """Round once to the storage type, back in x's type."""
    return x.to(dtype).to(x.dtype)


def _sum(x, dim, order):
    """order 0: torch.sum; order 1: one element after the other from the far end, every addition rounded to x's type (torch.cumsum is not
    that: on the CPU it accumulates float32 in double)."""
    if order == 0:
        return x.sum(dim)
    acc = torch.zeros_like(x.select(dim, 0))
    for i in range(x.shape[dim] - 1, -1, -1):
        acc = acc + x.select(dim, i)
    return acc


# ------------------------------------------------------------------------------------------------ LayerNorm
def add_ln_z(y, res, mask, inv_keep, dtype):
    """The kernel's z, bit for bit: float32 y * inv_keep where kept (0 elsewhere), + res, rounded once to the storage type."""
    v = y.to(F32)
    if mask is not None:
        v = torch.where(torch.as_tensor(mask), v * torch.tensor(inv_keep, dtype=F32), torch.zeros_like(v))
    if res is not None:
        v = v + res.to(F32)
    return v.to(dtype)


def add_ln_reference(y, res, gamma, beta, post, period, row_keep, mask, inv_keep, dtype, dt=F64, order=0, eps=LN_EPS,
                     ignore_row_keep=False, live_cols=None):
    """-> z (storage type), mean, rstd, out (dt, not rounded).  live_cols (bool D): columns that take part in the row statistics (a
    deliberate defect when not all do)."""
    z_st = add_ln_z(y, res, mask, inv_keep, dtype)
    z = z_st.to(dt)
    M, D = z.shape
    zs = z if live_cols is None else z * live_cols.to(dt)
    mean = _sum(zs, 1, order) / D
    dv = z - mean[:, None]
    if live_cols is not None:
        dv = dv * live_cols.to(dt)
    rstd = 1.0 / torch.sqrt(_sum(dv * dv, 1, order) / D + torch.tensor(eps, dtype=dt))
    out = (z - mean[:, None]) * rstd[:, None] * gamma.to(dt) + beta.to(dt)
    if post is not None:
        out = out + post.to(dt)[torch.arange(M) % period]
    if row_keep is not None and not ignore_row_keep:
        out = out * row_keep.to(dt)[:, None]
    return z_st, mean, rstd, out


def add_ln_bwd_reference(dout, z, mean, rstd, gamma, keep, mask, inv_keep, dt=F64, order=0, drop_row=None, live_cols=None):
    """-> d_res, d_y, dgamma, dbeta (dt; not rounded; dgamma / dbeta are the sums alone, without what the destination held).
    drop_row: a row left out of dgamma / dbeta; live_cols: columns that take part in the two row sums (deliberate defects)."""
    dout, z, mean, rstd, gamma = (t.to(dt) for t in (dout, z, mean, rstd, gamma))
    M, D = z.shape
    go = dout if keep is None else dout * keep.to(dt)[:, None]
    x = (z - mean[:, None]) * rstd[:, None]
    gy = go * gamma
    a, b = gy, gy * x
    if live_cols is not None:
        a, b = a * live_cols.to(dt), b * live_cols.to(dt)
    s1 = _sum(a, 1, order) / D
    s2 = _sum(b, 1, order) / D
    dz = rstd[:, None] * (gy - s1[:, None] - x * s2[:, None])
    d_y = dz if mask is None else dz * inv_keep * torch.as_tensor(mask).to(dt)
    pg, pb = go * x, go
    if drop_row is not None:
        sel = torch.ones(M, dtype=torch.bool)
        sel[drop_row] = False
        pg, pb = pg[sel], pb[sel]
    return dz, d_y, _sum(pg, 0, order), _sum(pb, 0, order)


# ---- exact cases
def chunks_for(D, dtype):
    epc = 4 if dtype == torch.float32 else 8
    return (D + 64 * epc - 1) // (64 * epc)


def nch_arm(D, dtype):
    c = chunks_for(D, dtype)
    return 1 if c == 1 else 2 if c == 2 else 4 if c <= 4 else 8


def slices_for(M):
    nblk = (M + 7) // 8
    return 64 if nblk >= 512 else 16 if nblk >= 64 else 1


def _ln_exact_cases():
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        for D in (32, 512, 1024, 2048) + ((4096,) if dtype == torch.bfloat16 else ()):
            for M in (7, 509) + ((4093,) if D == 512 else ()):
                for p in (0.0, 0.5):
                    out.append(dict(D=D, dtype=dtype, M=M, p=p))
    return out


LN_EXACT = _ln_exact_cases()


def ln_id(c):
    return "%s-D%d-M%d-p%g-NCH%d-slices%d" % ("f32" if c["dtype"] == torch.float32 else "bf16", c["D"], c["M"], c["p"],
                                              nch_arm(c["D"], c["dtype"]), slices_for(c["M"]))


_exact_cache = {}


def ln_exact_inputs(M, D):
    """Integer z, mean, dout; rstd in {1/2, 1, 2} per row; gamma in {+-1/2, +-1, +-2}; a row_keep with dropped rows; integer prior
    contents of dgamma / dbeta.  |dout| <= 2 and |x^| = |z - mean| * rstd <= 4 (the range note of the exact cases: x^ * s2 at D = 4096
    stays inside 24 bits).  Shared by the tests of a shape: callers leave it unchanged."""
    if (M, D) not in _exact_cache:
        g = torch.Generator().manual_seed(7919 * M + D)
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
        rstd = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (M,), generator=g)]
        span = (4.0 / rstd).long()                                   # |z - mean| <= 4 / rstd
        mean = ri(-8, 8, M)
        dev_ = torch.floor(torch.rand(M, D, generator=g).double() * (2 * span[:, None] + 1)) - span[:, None]
        gamma = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (D,), generator=g)] * (ri(0, 1, D) * 2 - 1)
        keep = (torch.rand(M, generator=g) > 0.25).to(torch.uint8)
        keep[0] = 1
        keep[M - 1] = 0
        _exact_cache[(M, D)] = dict(z=mean[:, None] + dev_, mean=mean, rstd=rstd, dout=ri(-2, 2, M, D), gamma=gamma, keep=keep,
                                    dgamma0=ri(-5, 5, D) + 7.0, dbeta0=ri(-5, 5, D) - 9.0)
    return _exact_cache[(M, D)]


# ---- tolerance cases
LN_TOL = [dict(D=D, dtype=dt_, M=53, period=10) for dt_, Ds in ((torch.float32, (40, 776, 1544)), (torch.bfloat16, (40, 1032, 3080)))
          for D in Ds]
LN_TOL_VARIANTS = [dict(p=0.1, res=True, post=True, keep=True), dict(p=0.0, res=True, post=True, keep=True),
                   dict(p=0.1, res=False, post=False, keep=False), dict(p=0.0, res=False, post=True, keep=False)]


def ln_tol_id(c, v=None):
    s = "%s-D%d-NCH%d" % ("f32" if c["dtype"] == torch.float32 else "bf16", c["D"], nch_arm(c["D"], c["dtype"]))
    if v is not None:
        s += "-p%g%s%s%s" % (v["p"], "-res" if v["res"] else "", "-post" if v["post"] else "", "-keep" if v["keep"] else "")
    return s


def ln_tol_inputs(c):
    """Operands of a tolerance case, rounded to its storage type where the kernel reads that type.  |y| >= 0.5: without a residual the
    zero pattern of z is the dropout mask."""
    M, D, dtype = c["M"], c["D"], c["dtype"]
    g = torch.Generator().manual_seed(31 * D + M)
    y = torch.randn(M, D, generator=g)
    y = (y + 0.5 * torch.sign(y)).to(dtype).float()
    res = torch.randn(M, D, generator=g).to(dtype).float()
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    post = torch.randn(c["period"], D, generator=g)
    keep = (torch.rand(M, generator=g) > 0.3).to(torch.uint8)
    keep[M - 1] = 0
    dout = torch.randn(M, D, generator=g).to(dtype).float()
    return dict(y=y, res=res, gamma=gamma, beta=beta, post=post, keep=keep, dout=dout)


def ln_tol_eval(c, v, x, mask, inv_keep, dt=F64, order=0, **defect):
    """Forward then backward of a tolerance case -> dict z (storage), mean, rstd, out, d_res, d_y, dgamma, dbeta.  The backward takes the
    forward's own mean and rstd in `dt`, and the rounded z.  defect: mask2 (another mask on the backward side), period, ignore_row_keep,
    live_cols, drop_row."""
    m = mask if v["p"] > 0 else None
    period = defect.get("period", c["period"])
    post = x["post"] if v["post"] else None
    if post is not None and period > post.shape[0]:
        post = torch.cat([post, post[:period - post.shape[0]]])
    z, mean, rstd, out = add_ln_reference(x["y"], x["res"] if v["res"] else None, x["gamma"], x["beta"], post, period,
                                          x["keep"] if v["keep"] else None, m, inv_keep, c["dtype"], dt=dt, order=order,
                                          ignore_row_keep=defect.get("ignore_row_keep", False), live_cols=defect.get("live_cols"))
    keep_b = None if (not v["keep"] or defect.get("ignore_row_keep")) else x["keep"]
    mb = defect.get("mask2", m) if v["p"] > 0 else None
    d_res, d_y, dg, db = add_ln_bwd_reference(x["dout"], z, mean, rstd, x["gamma"], keep_b, mb, inv_keep, dt=dt, order=order,
                                              drop_row=defect.get("drop_row"), live_cols=defect.get("live_cols"))
    return dict(z=z, mean=mean, rstd=rstd, out=out, d_res=d_res, d_y=d_y, dgamma=dg, dbeta=db)


LN_TENSORS = ("mean", "rstd", "out", "d_res", "d_y", "dgamma", "dbeta")
LN_STORED = ("out", "d_res", "d_y")          # written in the storage type: + BF16_REL |ref| in bf16

_tol_cache = {}


def ln_tol_reference(c, v, x, mask, inv_keep):
    """(float64 reference, {tensor: b32}) of a case / variant / mask: computed once per process and shared (callers leave it unchanged)."""
    key = (ln_tol_id(c, v), None if mask is None else hash(np.asarray(mask).tobytes()))
    if key not in _tol_cache:
        ref = ln_tol_eval(c, v, x, mask, inv_keep)
        b32 = {t: 0.0 for t in LN_TENSORS}
        for order in (0, 1):
            e = ln_tol_eval(c, v, x, mask, inv_keep, dt=F32, order=order)
            for t in LN_TENSORS:
                b32[t] = max(b32[t], B32_FACTOR * float((e[t].double() - ref[t]).abs().max()))
        _tol_cache[key] = (ref, b32)
    return _tol_cache[key]


def excess(got, ref, b32, bf16_stored):
    """max over elements of |got - ref| / bound (> 1: outside).  A non-finite got counts +inf."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not torch.isfinite(got).all():
        return float("inf")
    bound = b32 + (BF16_REL * ref.abs() if bf16_stored else 0.0)
    diff = (got - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(diff.shape)
    # (a bound of 0 -- sums of bf16 values that are exact in fp32 in any order -- demands equality)
    r = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf"))))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ embedding
EMB_B, EMB_T, EMB_V, EMB_PAD, EMB_SCALE = 3, 700, 6, 0, 0.5
EMBED_CASES = [dict(D=D, dtype=dt_, p=p) for dt_ in (torch.float32, torch.bfloat16) for D in (72, 520) for p in (0.0, 0.5)]


def embed_id(c):
    return "%s-D%d-p%g" % ("f32" if c["dtype"] == torch.float32 else "bf16", c["D"], c["p"])


def embed_tokens():
    """(B, T) = 2100 positions, more than two 1024-position chunks.  Token 1: a run of 300 from position 0 (the owner's first 256-position
    sub-chunk fills `list`), again at 1500 and 2090 (its second and third chunk); token 2: first at 1100 (an owner beyond position 1024:
    its scan runs base = 0 and base = 1024), again at 2000 (a non-owner whose scan finds the owner in the second chunk); token 3: only at
    the last position; token 4: scattered from 300 on; token 5: every 7th position from 301; PAD: 600 .. 650 and 1300 .. 1310."""
    n = EMB_B * EMB_T
    tok = torch.full((n,), 4, dtype=torch.int64)
    tok[301::7] = 5
    tok[:300] = 1
    tok[1500] = 1
    tok[2090] = 1
    tok[600:651] = EMB_PAD
    tok[1300:1311] = EMB_PAD
    tok[1100:1111] = 2
    tok[2000] = 2
    tok[n - 1] = 3
    assert (tok[:1100] != 2).all() and int((tok == 3).sum()) == 1
    return tok.view(EMB_B, EMB_T)


def embed_inputs(D):
    g = torch.Generator().manual_seed(D)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    return dict(tok=embed_tokens(), table=ri(-8, 8, EMB_V, D), pe=ri(0, 8, EMB_T, D), dout=ri(-4, 4, EMB_B, EMB_T, D),
                dtable0=ri(-5, 5, EMB_V, D) + 11.0)


def embed_reference(tok, table, pe, scale, mask, inv_keep, dt=F64):
    """(B, T, D): table[tok] * scale + pe[t], dropped and rescaled."""
    Bn, T = tok.shape
    out = table.to(dt)[tok] * scale + pe.to(dt)[None, :T]
    if mask is not None:
        out = out * torch.as_tensor(mask).view(out.shape).to(dt) * inv_keep
    return out


def embed_bwd_reference(tok, dout, dtable0, scale, mask, inv_keep, pad_id, dt=F64, order=0, skip_second_chunk=False):
    """dtable0 + index_add_ of the masked, scaled gradients; the PAD row keeps what it held.  skip_second_chunk: positions 1024 .. 2047
    behind a token's first position are left out (a deliberate defect)."""
    n, D = tok.numel(), dout.shape[-1]
    t = tok.reshape(-1)
    g = dout.reshape(n, D).to(dt) * scale
    if mask is not None:
        g = g * torch.as_tensor(mask).view(n, D).to(dt) * inv_keep
    live = t != pad_id
    if skip_second_chunk:
        first = torch.full((int(t.max()) + 1,), n, dtype=torch.int64).scatter_reduce(0, t, torch.arange(n), "amin")
        rel = torch.arange(n) - first[t]
        live = live & ~((rel >= 1024) & (rel < 2048))
    if order == 1:
        idx = torch.flip(torch.nonzero(live)[:, 0], (0,))
    else:
        idx = torch.nonzero(live)[:, 0]
    out = dtable0.to(dt).clone()
    if order == 0:
        out.index_add_(0, t[idx], g[idx])
    else:
        for v in t[idx].unique().tolist():
            rows = idx[t[idx] == v]
            out[v] += _sum(g[rows], 0, 1)
    return out


# ------------------------------------------------------------------------------------------------ cross entropy
CE_PAD = 0
CE_CASES = [dict(M=M, V=V, ld=(37 if V == 35 else 4368), smoothing=s) for M in (13, 517) for V in (35, 4364) for s in (0.0, 0.1)]
CE_SCALE = 30.0
CE_GRAD_OUT = 1.75


def ce_id(c):
    return "M%d-V%d-ld%d-eps%g" % (c["M"], c["V"], c["ld"], c["smoothing"])


def ce_inputs(c):
    """logits (M, V) fp32 (x 30), gold with PAD rows; row 7: all equal; row 8: a two-way tie of the largest value at columns 5 and 20;
    row 9: all -inf with a PAD gold (argmax 0; its lse is not defined and nothing reads it)."""
    M, V = c["M"], c["V"]
    g = torch.Generator().manual_seed(1000 * M + V)
    logits = torch.randn(M, V, generator=g) * CE_SCALE
    gold = torch.randint(1, V, (M,), generator=g)
    gold[::5] = CE_PAD
    gold[7], gold[8] = 3, 5
    logits[7] = 2.5
    logits[8, 5] = logits[8, 20] = float(logits[8].max()) + 9.0
    logits[9] = float("-inf")
    gold[9] = CE_PAD
    return dict(logits=logits, gold=gold)


def ce_reference(logits, gold, smoothing, pad_id, grad_out, dt=F64, order=0, classes=None, lse_in=None):
    """-> dict lse, argmax (lowest index on ties; 0 for a row without a finite value), loss_rows, sums (3: loss, non-PAD rows, correct),
    dlogits (M, V) = grad_out / count * (softmax * sum_q - q), sum_q = 1 - eps / V as ce_bwd_kernel has it; PAD rows 0.
    dt = float32: torch's own float32 log_softmax.  classes: over how many classes the smoothing mass is spread (V; a deliberate defect
    when it is not).  lse_in: the probabilities as exp(l - lse_in), the form of ce_bwd_kernel, whose lse is an fp32 INPUT written by
    the forward (like mean / rstd of the LayerNorm backward), instead of exp(log_softmax)."""
    M, V = logits.shape
    l = logits.to(dt)
    fin = torch.isfinite(l).any(1)
    lsafe = torch.where(fin[:, None], l, torch.zeros_like(l))
    lp = torch.log_softmax(lsafe, 1)
    lse = torch.logsumexp(lsafe, 1)
    mx = l.max(1, keepdim=True).values
    am = torch.where(fin, (l == mx).to(torch.int64).argmax(1), torch.zeros(M, dtype=torch.int64))
    live = gold != pad_id
    gi = gold.clamp(0, V - 1)
    lpg = lp.gather(1, gi[:, None])[:, 0]
    nc = V if classes is None else classes
    if smoothing > 0:
        loss = -((1.0 - smoothing) * lpg + (smoothing / nc) * (_sum(lp, 1, order) - lpg))
    else:
        loss = -lpg
    loss = torch.where(live, loss, torch.zeros_like(loss))
    count = float(live.sum())
    correct = float((live & (am == gold)).sum())
    q_other = smoothing / nc if smoothing > 0 else 0.0
    q_gold = 1.0 - smoothing if smoothing > 0 else 1.0
    sum_q = q_gold + (V - 1) * q_other
    q = torch.full((M, V), q_other, dtype=dt)
    q.scatter_(1, gi[:, None], q_gold)
    prob = torch.exp(lp) if lse_in is None else torch.where(fin[:, None], torch.exp(lsafe - lse_in.to(dt)[:, None]), torch.zeros_like(l))
    dl = (grad_out / count) * (prob * sum_q - q) * live.to(dt)[:, None]
    return dict(lse=lse, argmax=am, loss_rows=loss, sums=(_sum(loss, 0, order), count, correct), dlogits=dl, live=live, finite=fin)


def pad_columns_clean(full, V):
    """full (M, ldd) is what asr_ce_bwd wrote: no NaN anywhere and every column from V on exactly 0 (the data-gradient GEMM contracts the
    padded width)."""
    f = full.detach().float().cpu()
    return bool(not torch.isnan(f).any() and (f[:, V:] == 0).all())


_ce_cache = {}


def ce_case_reference(c):
    """(inputs, float64 reference, bounds) of a CE case, once per process.  bounds: lse (absolute), loss_rel (x sum |loss_i|), dlogits
    (absolute): B32_FACTOR x the largest error of the float32 evaluation (torch's float32 log_softmax, both row orders)."""
    k = ce_id(c)
    if k not in _ce_cache:
        x = ce_inputs(c)
        ref = ce_reference(x["logits"], x["gold"], c["smoothing"], CE_PAD, CE_GRAD_OUT)
        rows = ref["live"] | ref["finite"]
        sabs = float(ref["loss_rows"].abs().sum())
        b = dict(lse=0.0, loss_rel=0.0, dlogits=0.0)
        for order in (0, 1):
            e = ce_reference(x["logits"], x["gold"], c["smoothing"], CE_PAD, CE_GRAD_OUT, dt=F32, order=order)
            b["lse"] = max(b["lse"], float((e["lse"].double() - ref["lse"])[rows & ref["finite"]].abs().max()))
            per_row = float((e["loss_rows"].double() - ref["loss_rows"]).abs().sum())
            b["loss_rel"] = max(b["loss_rel"], per_row / sabs, abs(float(e["sums"][0]) - float(ref["sums"][0])) / sabs)
            # dlogits in float32 both ways: from the float32 log_softmax itself, and as the backward kernel's interface has it, from
            # the row's lse STORED in fp32 (half an ulp of |lse| ~ 100 moves every probability of the row by that much, relatively)
            e2 = ce_reference(x["logits"], x["gold"], c["smoothing"], CE_PAD, CE_GRAD_OUT, dt=F32, order=order, lse_in=e["lse"])
            for ee in (e, e2):
                b["dlogits"] = max(b["dlogits"], float((ee["dlogits"].double() - ref["dlogits"]).abs().max()))
        _ce_cache[k] = (x, ref, {t: B32_FACTOR * v for t, v in b.items()})
    return _ce_cache[k]


# ------------------------------------------------------------------------------------------------ optimiser
def noam_rate(t, factor_ms, warmup, min_lr):
    return max(min_lr, factor_ms * min(t ** -0.5, t * warmup ** -1.5))


def adam_noam_reference(p, g, m, v, t, grad_scale, beta1, beta2, eps, factor_ms, warmup, min_lr):
    """One step in float64 from fp32 (p, g, m, v); the float arguments as the C ABI receives them (fp32).  -> p, m, v, lr, update."""
    f = lambda a: float(np.float32(a))
    b1, b2, eps, factor_ms, warmup, min_lr = f(beta1), f(beta2), f(eps), f(factor_ms), f(warmup), f(min_lr)
    lr = noam_rate(float(t), factor_ms, warmup, min_lr)
    gj = g.double() * (1.0 if grad_scale is None else float(np.float32(grad_scale)))
    mn = b1 * m.double() + (1.0 - b1) * gj
    vn = b2 * v.double() + (1.0 - b2) * gj * gj
    upd = (lr / (1.0 - b1 ** t)) * (mn / (torch.sqrt(vn) / np.sqrt(1.0 - b2 ** t) + eps))
    return p.double() - upd, mn, vn, lr, upd


def adam_noam_f32(p, g, m, v, t, grad_scale, beta1, beta2, eps, factor_ms, warmup, min_lr):
    """The same step with every operation of the kernel rounded to fp32 (no FMA contraction): what an honest fp32 evaluation gives."""
    f = np.float32
    b1, b2, eps = torch.tensor(f(beta1)), torch.tensor(f(beta2)), torch.tensor(f(eps))
    lr = f(max(f(min_lr), f(float(f(factor_ms)) * min(float(t) ** -0.5, float(t) * float(f(warmup)) ** -1.5))))
    gj = g if grad_scale is None else g * torch.tensor(f(grad_scale))
    mn = b1 * m + (1 - b1) * gj
    vn = b2 * v + (1 - b2) * gj * gj
    bc1 = f(1.0 - float(f(beta1)) ** t)
    bc2s = np.sqrt(f(1.0 - float(f(beta2)) ** t), dtype=f)
    step = torch.tensor(f(lr / bc1))
    pn = p - step * (mn / (torch.sqrt(vn) / torch.tensor(bc2s) + eps))
    return pn, mn, vn, float(lr)


ADAM = dict(beta1=0.9, beta2=0.98, eps=1e-9, factor_ms=1.0 * 512 ** -0.5, warmup=4000.0, min_lr=1e-7)      # (min_lr below the rate at t = 1: the warm-up arm is live)
ADAM_STEPS = (1, 4000, 4001)


def adam_inputs(n):
    """p; g and m of one sign per element (m is a running mean of gradients: b1 m + (1 - b1) g does not cancel, so `relative` means
    something); v > 0; per-step positive gradient factors."""
    g_ = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_)
    m = g * (0.5 + torch.rand(n, generator=g_))
    v = g * g * (0.5 + torch.rand(n, generator=g_)) + 1e-3
    return dict(p=p, g=g, m=m, v=v, factors=(1.0, 0.37, 2.9))


def adam_bounds(ref_p, ref_m, ref_v, upd):
    """Element-wise bounds of one step: a few ulps of each fp32 expression."""
    return dict(p=2.0 ** -23 * ref_p.abs() + 2.0 ** -21 * upd.abs(), m=2.0 ** -22 * ref_m.abs(), v=2.0 ** -22 * ref_v.abs())


def grad_coef_reference(sumsq, max_norm, denom):
    s = 1.0 / max(float(denom), 1.0)
    return s * min(1.0, float(np.float32(max_norm)) / (np.sqrt(float(sumsq)) * s + float(np.float32(1e-6))))
