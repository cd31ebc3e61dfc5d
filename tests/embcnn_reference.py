"""The yardstick of tests/test_gpu_embcnn_arms.py and tests/test_embcnn_reference_host.py: float64 references of every operation of
csrc/embcnn.hip -- im2col, col2im, window_sum, the BatchNorm statistics in their three forms, BatchNorm + Hardtanh forward, backward
reduction and backward (reference models/asr/transformer.py:33-40, 70-76 and their autograd) -- with the kernels' index rules (`act_index`,
`grid_row`) restated, the case tables both files iterate, and builders of integer data on which the kernels can be held bit for bit.

Why equality: asr_bn_act_fwd / _bwd_reduce / _bwd take `mean` and `rstd` as INPUTS.  With y, mean, beta, dz integers, rstd in {1/2, 1, 2}
and gamma in {+-1, +-2}, x^ = (y - mean) rstd is a multiple of 1/2, z = x^ gamma + beta a multiple of 1/2, the sums of dz and dz x^ are
multiples of 1/2, and with a power-of-two row count N the means m1 = sum dz / N, m2 = sum dz x^ / N and dz - m1 - x^ m2 lie on the grid
1 / (4 N).  `guard` (tests/conv_reference.py) demands, in float64, that the sum of the absolute terms of every output stays below 2^24
steps of that grid: every partial sum is then an fp32 number in any order, fused or not, and the stored value is the float64 value (after
ONE round-to-nearest-even where the kernel stores bf16).  The same argument, without the division, covers im2col (a copy), col2im and
window_sum (sums of small integers) and the sums of asr_bn_stats on integer y and integer centre.

Where the row count is no power of two the division rounds, and on random data everything rounds: there the bound is the project's
b32 = 4 x the error of the float32 CPU evaluation of the same formulas on the case's data, in two summation orders (`B32_FACTOR`,
tests/rowwise_reference.py), plus 2^-8 |ref| where the kernel stores bf16.  The random BatchNorm cases keep every float64 pre-activation
at least `Z_MARGIN` away from lo and hi, so that no legitimate fp32 rounding moves an element across the Hardtanh mask.

Geometry note.  The table of the issue calls `stride_pad` a geometry whose windows leave input pixels without an output; they do not
(H + 2 PH - KH = 9 leaves one PADDING row over, W + 2 PW - KW = 12 is a whole number of strides).  `gaps` is added for that property:
stride 3 with a 2-wide window skips every third column and the last row belongs to no window -- col2im must write zeros there.

This module needs no GPU."""
import collections
import functools

import torch

from conv_reference import guard, grid_of
from rowwise_reference import B32_FACTOR, BF16_REL, _sum, rnd  # noqa: F401  (re-exported for the two test files)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LO, HI = 0.0, 20.0
BN_ROWS = 512            # rows per workgroup of bn_stats_kernel / bn_act_bwd_reduce_kernel (csrc/embcnn.hip)
ACT_ROWS = 64            # rows per workgroup of bn_act_fwd_kernel / bn_act_bwd_kernel
Z_MARGIN = 2.0 ** -10    # random cases: |z - lo|, |z - hi| >= this in float64 (fp32 error of z at |z| <= 64 is below 2^-16)

Case = collections.namedtuple("Case", "id args pins")


def ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------ geometry
def conv_geom(B, H, W, C, KH, KW, SH, SW, PH, PW):
    """(B,H,W,C,KH,KW,SH,SW,PH,PW,OH,OW): ops.conv_geom restated."""
    return (B, H, W, C, KH, KW, SH, SW, PH, PW, (H + 2 * PH - KH) // SH + 1, (W + 2 * PW - KW) // SW + 1)


def pad8(n):
    return (n + 7) // 8 * 8


GEOMS = [
    Case("unit", (2, 9, 7, 8, 3, 3, 1, 1, 0, 0), "the vector path"),
    Case("stride_h", (2, 11, 10, 16, 5, 3, 2, 1, 0, 0), "the second convolution's kind of stride"),
    Case("stride_pad", (1, 10, 13, 8, 3, 5, 2, 3, 1, 2), "both strides and both paddings"),
    Case("first_conv", (2, 45, 12, 1, 41, 11, 2, 2, 0, 10), "C = 1, K = 451, ld = 456"),
    Case("win_x2", (2, 25, 9, 32, 21, 1, 2, 1, 0, 0), "the window form's geometry, ld = 704 > K = 672"),
    Case("c3", (2, 7, 6, 3, 3, 3, 1, 1, 1, 1), "the scalar path with taps inside a chunk"),
    Case("c12", (1, 6, 5, 12, 2, 2, 1, 1, 0, 0), "chunks that straddle a tap"),
    Case("gaps", (1, 10, 12, 8, 3, 2, 2, 3, 0, 1), "stride 3 > KW = 2 and a last row past the last window: input pixels that feed no output"),
]
GEOMS_C8 = [c for c in GEOMS if c.args[3] % 8 == 0]


def geom_ld(c):
    """The leading dimension of the case's column matrix: K padded to 8 elements; win_x2 as the window form pads it (704)."""
    g = conv_geom(*c.args)
    K = g[3] * g[4] * g[5]
    return 704 if c.id == "win_x2" else pad8(K)


def _taps(g, defect=None):
    """For every tap (ky, kx): (column block index, input rows ih (OH), their validity, input columns iw (OW), their validity)."""
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    sh, sw = (SW, SH) if defect == "stride_axis" else (SH, SW)
    ph, pw = (PH + 1, PW + 1) if defect == "pad_off" else (PH, PW)
    for ky in range(KH):
        ih = torch.arange(OH) * sh - ph + ky
        vh = (ih >= 0) & (ih < H)
        for kx in range(KW):
            iw = torch.arange(OW) * sw - pw + kx
            vw = (iw >= 0) & (iw < W)
            tap = kx * KH + ky if defect == "tap_transposed" else ky * KW + kx
            yield tap, ih, vh, iw, vw


def im2col(x_nhwc, geom, ld, rows_alloc, defect=None):
    """col (rows_alloc, ld) float64: row (b, oh, ow), column (ky, kx, c); padding, the columns >= K and the rows >= M are 0.
    defect: "tap_transposed", "stride_axis", "pad_off", "pad_col" (a non-zero pad column), "pad_row" (a non-zero row behind M)."""
    g = conv_geom(*geom[:10])
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    K, M = KH * KW * C, B * OH * OW
    assert ld >= K and rows_alloc >= M and tuple(x_nhwc.shape) == (B, H, W, C)
    x = x_nhwc.double()
    blocks = torch.zeros(B, OH, OW, KH * KW, C, dtype=F64)
    for tap, ih, vh, iw, vw in _taps(g, defect):
        v = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
        blocks[:, :, :, tap] = v * (vh[:, None] & vw[None, :])[None, :, :, None]
    col = torch.zeros(rows_alloc, ld, dtype=F64)
    col[:M, :K] = blocks.reshape(M, K)
    if defect == "pad_col" and ld > K:
        col[:M, K] = 1.0
    if defect == "pad_row" and rows_alloc > M:
        col[M, 0] = 1.0
    return col


def col2im(dcol, geom, defect=None):
    """The adjoint of im2col: dx (B, H, W, C) float64, every (row, tap) of dcol[:M, :K] scatter-added into the pixel it was read from; a
    pixel no window covers is 0.  defect: the three index defects of im2col, "uncovered" (a pixel without a window keeps a 1)."""
    g = conv_geom(*geom[:10])
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    K, M = KH * KW * C, B * OH * OW
    d = dcol[:M, :K].double().reshape(B, OH, OW, KH * KW, C)
    dx = torch.zeros(B, H, W, C, dtype=F64)
    for tap, ih, vh, iw, vw in _taps(g, defect):
        if bool(vh.any()) and bool(vw.any()):
            dx[:, ih[vh][:, None], iw[vw][None, :]] += d[:, vh][:, :, vw][:, :, :, tap]
    if defect == "uncovered":
        dx[~covered(geom).expand(B, H, W)] = 1.0
    return dx


def covered(geom):
    """(1, H, W) bool: the input pixels at least one window reads."""
    g = conv_geom(*geom[:10])
    B, H, W = g[:3]
    m = torch.zeros(1, H, W, dtype=torch.bool)
    for _, ih, vh, iw, vw in _taps(g):
        m[:, ih[vh][:, None], iw[vw][None, :]] = True
    return m


def taps_per_pixel(geom):
    """The largest number of (row, tap) terms col2im adds into one pixel."""
    g = conv_geom(*geom[:10])
    n = torch.zeros(g[1], g[2], dtype=F64)
    for _, ih, vh, iw, vw in _taps(g):
        n[ih[vh][:, None], iw[vw][None, :]] += 1
    return n


@functools.lru_cache(maxsize=None)
def col_case(cid):
    """Integer data of one geometry: x (B, H, W, C) in {-3 .. 3}, dcol (M, ld) in {-2 .. 2}, and the float64 col (M + 5 rows) and dx.
    The guard bounds col2im's sums: at most taps_per_pixel terms of magnitude 2."""
    c = [c for c in GEOMS if c.id == cid][0]
    g = conv_geom(*c.args)
    B, H, W, C, KH, KW, SH, SW, PH, PW, OH, OW = g
    M, K, ld = B * OH * OW, KH * KW * C, geom_ld(c)
    gen = torch.Generator().manual_seed(sum(ord(ch) for ch in cid))
    x = torch.randint(-3, 4, (B, H, W, C), generator=gen).float()
    dcol = torch.randint(-2, 3, (M, ld), generator=gen).float()
    guard("col2im " + cid, 2.0 * taps_per_pixel(c.args), 1.0)
    assert float(dcol.abs().max()) <= 256 and float(x.abs().max()) <= 256           # exact in bf16
    return dict(geom=g, M=M, K=K, ld=ld, x=x, dcol=dcol, col=im2col(x, g, ld, M + 5), dx=col2im(dcol, g))


# ------------------------------------------------------------------------------------------------ window sum
def window_sum(Z, bias, groups, Wg, OW, KW, Cout, ldy, defect=None):
    """y (groups * OW, ldy) float64: y[g OW + j, co] = bias[co] + sum_kx Z[g Wg + j + kx, kx Cout + co]; columns >= Cout are 0."""
    Z = Z.double()
    y = torch.zeros(groups * OW, ldy, dtype=F64)
    rows = (torch.arange(groups)[:, None] * Wg + torch.arange(OW)[None, :]).reshape(-1)
    for kx in range(KW):
        sh = kx + 1 if defect == "shift" else kx
        y[:, :Cout] += Z[rows + sh, kx * Cout:(kx + 1) * Cout]
    if bias is not None:
        y[:, :Cout] += bias.double()
    return y


WSUM = [
    # args (groups, Wg, OW, KW, Cout, ldz, ldy, bias)
    Case("nobias_tight", (7, 13, 9, 5, 32, 160, 32, False), "bias = None, ldy == Cout"),
    Case("kw1", (6, 9, 9, 1, 32, 32, 64, True), "KW = 1: the sum is a copy plus bias"),
    Case("cout4", (5, 11, 4, 8, 4, 40, 8, True), "Cout = 4: one thread per row, a zero pad quad"),
    Case("many_rows", (130, 23, 13, 11, 32, 352, 64, True), "1690 rows x 16 quads: 106 workgroups, a ragged last one"),
]


@functools.lru_cache(maxsize=None)
def wsum_case(cid):
    c = [c for c in WSUM if c.id == cid][0]
    groups, Wg, OW, KW, Cout, ldz, ldy, has_bias = c.args
    gen = torch.Generator().manual_seed(len(cid) + groups)
    Z = torch.randint(-4, 5, (groups * Wg + KW - 1, ldz), generator=gen).float()
    bias = torch.randint(-8, 9, (Cout,), generator=gen).float() * 0.5 if has_bias else None
    guard("window_sum " + cid, torch.tensor([4.0 * KW + 4.0]), 0.5)
    return dict(Z=Z, bias=bias, y=window_sum(Z, bias, groups, Wg, OW, KW, Cout, ldy))


# ------------------------------------------------------------------------------------------------ index rules of the BatchNorm kernels
def grid_rows(M, grid):
    """grid_row restated: row m of the convolution -> row (m // gow) * gw + m % gow of a buffer of groups of gw rows ((0, 0): m)."""
    gw, gow = grid
    m = torch.arange(M)
    return m if gow <= 0 else (m // gow) * gw + m % gow


def on_grid(t, grid, fill, ld=None):
    """t (M, C) -> the buffer the kernels see: (groups * gw, ld) with `fill` in the gap rows and the columns >= C."""
    M, C = t.shape
    ld = ld or C
    rows = M if grid[1] <= 0 else M // grid[1] * grid[0]
    buf = torch.full((rows, ld), fill, dtype=t.dtype)
    buf[grid_rows(M, grid), :C] = t
    return buf


def off_grid(buf, M, C, grid):
    return buf[grid_rows(M, grid).to(buf.device), :C]


def act_index(M, C, tH, tW, ldo, swapped=False):
    """act_index restated, (M, C) flat offsets: tH == 0: m ldo + c; tH > 0: rows are (b, h, w) over (B, tH, tW) and the activation lives
    in the encoder layout (B, tW, C tH) with feature c tH + h.  swapped: the deliberate defect (tH and tW exchanged)."""
    m = torch.arange(M)[:, None]
    c = torch.arange(C)[None, :]
    if tH <= 0:
        return m * ldo + c
    if swapped:
        tH, tW = tW, tH
    w, t = m % tW, m // tW
    h, b = t % tH, t // tH
    return ((b * tW + w) * C + c) * tH + h


def to_act(t, tH, tW, ldo=None, fill=0.0, swapped=False):
    """t (M, C) -> the flat activation buffer (tH > 0: M C elements; else M ldo, `fill` in the pad columns)."""
    M, C = t.shape
    ldo = ldo or C
    buf = torch.full((M * (C if tH > 0 else ldo),), fill, dtype=t.dtype)
    buf[act_index(M, C, tH, tW, ldo, swapped).reshape(-1)] = t.reshape(-1)
    return buf


def from_act(buf, M, C, tH, tW, ldo=None):
    return buf.reshape(-1)[act_index(M, C, tH, tW, ldo or C).reshape(-1).to(buf.device)].reshape(M, C)


def keep_rows(M, valid):
    """valid = (n, row_w) or None -> (M,) bool: row m counts when m % row_w < n."""
    if valid is None:
        return torch.ones(M, dtype=torch.bool)
    n, row_w = valid
    assert M % row_w == 0
    return (torch.arange(M) % row_w) < n


# ------------------------------------------------------------------------------------------------ BatchNorm statistics
def bn_sums(y, center=None, keep=None, dt=F64, order=0, drop_last_block=False):
    """(sum (y - center), sum (y - center)^2) over the kept rows of compact y (M, C), evaluated in dt.  drop_last_block: the deliberate
    defect (the last 512-row partial left out of the fixed-order sum)."""
    v = y.to(dt)
    if center is not None:
        v = v - center.to(dt)
    if keep is not None:
        v = v * keep.to(dt)[:, None]
    if drop_last_block:
        v = v[:(v.shape[0] - 1) // BN_ROWS * BN_ROWS]
    return _sum(v, 0, order), _sum(v * v, 0, order)


def bn_stats(y, eps, momentum, rm0, rv0, nb0, valid=None, dt=F64, order=0, defect=None):
    """Training-mode nn.BatchNorm2d statistics by the kernels' formulas (two passes; inv = 1 / count, mean = sum inv, var = centred sum
    inv, rstd = 1 / sqrt(var + eps), running_var from var count / (count - 1)) -> dict(mean, var, rstd, rm, rv, nb).  The count is
    groups x valid under a length mask.  defect: "masked_counted", "count_M", "biased_running", "drop_last_block"."""
    M = y.shape[0]
    keep = keep_rows(M, valid)
    count = float(keep.sum())
    ksum = None if defect == "masked_counted" else keep
    if defect == "masked_counted" or defect == "count_M":
        count = float(M)
    one = torch.ones((), dtype=dt)
    inv = one / torch.tensor(max(count, 1.0), dtype=dt)
    unbias = torch.tensor(count, dtype=dt) / torch.tensor(max(count - 1.0, 1.0), dtype=dt)
    if defect == "biased_running":
        unbias = one
    drop = defect == "drop_last_block"
    mean = bn_sums(y, None, ksum, dt, order, drop)[0] * inv
    var = bn_sums(y, mean, ksum, dt, order, drop)[1] * inv
    rstd = one / torch.sqrt(var + torch.tensor(eps, dtype=F32).to(dt))
    out = dict(mean=mean, var=var, rstd=rstd, nb=nb0 + (1 if momentum >= 0 else 0))
    if momentum >= 0:
        mom = torch.tensor(momentum, dtype=F32).to(dt)
        out["rm"] = rm0.to(dt) * (one - mom) + mom * mean
        out["rv"] = rv0.to(dt) * (one - mom) + mom * unbias * var
    else:
        out["rm"], out["rv"] = rm0.to(dt), rv0.to(dt)
    return out


STAT_TENSORS = ("mean", "rstd", "rm", "rv")


def bn_stats_errors(y, eps, momentum, rm0, rv0, valid=None):
    """(float64 reference, {tensor: error of the float32 evaluation, the worse of two summation orders}): absolute for mean and the running
    mean, relative to |ref| for rstd and the running variance (positive, and 316 at M = 1 against 0.2 elsewhere)."""
    ref = bn_stats(y, eps, momentum, rm0, rv0, 0, valid)
    err = {t: 0.0 for t in STAT_TENSORS}
    for order in (0, 1):
        e = bn_stats(y, eps, momentum, rm0, rv0, 0, valid, dt=F32, order=order)
        for t in STAT_TENSORS:
            d = (e[t].double() - ref[t]).abs()
            err[t] = max(err[t], float((d / ref[t].abs() if t in STAT_RELATIVE else d).max()))
    return ref, err


STAT_RELATIVE = ("rstd", "rv")


STAT_C = (1, 2, 8, 32, 64, 256)


def stat_rows(C):
    """M at the seams of the 64-row blocks, the 512-row blocks and the 4 x nrl unroll (nrl = 256 / C row lanes); 1537 at C = 256: four
    partial rows on two row groups of bn_partial_sum_kernel; 8193 at C = 32: seventeen on sixteen."""
    u = 4 * (256 // C)
    ms = {1, 63, 64, 65, u - 1, u, u + 1, 511, 512, 513}
    if C == 256:
        ms.add(1537)
    if C == 32:
        ms.add(8193)
    return sorted(ms)


def stat_grid(M):
    """A row grid for M rows: gow the largest divisor of M up to 16, three gap rows behind every group."""
    gow = max(d for d in range(1, 17) if M % d == 0)
    return (gow + 3, gow)


@functools.lru_cache(maxsize=None)
def stat_case(C, M):
    """Integer data for the statistics: y (M, C) in {-9 .. 9} whose column sums are multiples of M when M is a power of two (so that the
    mean is an integer and exact), an integer centre in {-3 .. 3}, integer prior contents of the accumulated sums, running buffers.
    Guarded: twice the sums on top of the prior contents stay exact in fp32 in any order."""
    gen = torch.Generator().manual_seed(1000 * C + M)
    y = torch.randint(-8, 9, (M, C), generator=gen).double()
    pow2 = M & (M - 1) == 0
    if pow2:
        r = torch.remainder(y.sum(0), M).long()                   # lower the first r rows of a column by 1: its sum becomes a multiple of M
        y = y - (torch.arange(M)[:, None] < r[None, :]).double()
    center = torch.randint(-3, 4, (C,), generator=gen).double()
    prior = torch.randint(-5, 6, (2 * C,), generator=gen).double()
    rm0 = torch.randint(-4, 5, (C,), generator=gen).double() * 0.25
    rv0 = torch.randint(1, 9, (C,), generator=gen).double() * 0.25
    a = (y - center).abs()
    guard("bn_stats sums C %d M %d" % (C, M), torch.cat([2 * a.sum(0) + 5, 2 * (a * a).sum(0) + 5]), 1.0)
    s, q = bn_sums(y, center)
    if pow2:
        assert torch.equal(y.sum(0) / M, (y.sum(0) / M).round())
    return dict(y=y, center=center, prior=prior, rm0=rm0, rv0=rv0, sums=torch.cat([s, q]), pow2=pow2)


@functools.lru_cache(maxsize=None)
def stat_bounds(C, mask):
    """{M: (float64 reference, {tensor: b32})} for the integer cases of one C.  mask: None, "all" (valid = row_w of stat_grid(M)) or "one"
    (valid = 1).  A statistic has C elements, at C = 1 a single one, and the float32 error of a single element is one draw that can be
    nearly 0 (3.8e-9 relative for rstd at C = 1, M = 63) when a correct kernel's is half an ulp.  The error is therefore pooled over the
    data of the parametrised case, which runs every M of stat_rows(C): b32(M) = 4 x the largest error among the rows M' <= max(M, 65) of
    the same kind -- a power-of-two count (exact sums: what is left is the rounding of the division and the root, whatever M) or not
    (the error of the centred sum grows with M, so a larger M' must not lend its error to a smaller M) -- times |ref| for the relative
    tensors."""
    per = {}
    for M in stat_rows(C):
        k = stat_case(C, M)
        row_w = stat_grid(M)[1]
        valid = None if mask is None else (row_w if mask == "all" else 1, row_w)
        n = count_of(M, valid)
        per[M] = bn_stats_errors(k["y"], 1e-5, 0.1, k["rm0"], k["rv0"], valid) + (n & (n - 1) == 0,)
    out = {}
    for M, (ref, _, kind) in per.items():
        pool = {t: max(e[t] for M2, (_, e, k2) in per.items() if k2 == kind and M2 <= max(M, 65)) for t in STAT_TENSORS}
        out[M] = (ref, {t: B32_FACTOR * pool[t] * (ref[t].abs() if t in STAT_RELATIVE else 1.0) for t in STAT_TENSORS})
    return out


# ------------------------------------------------------------------------------------------------ BatchNorm + Hardtanh
def bn_act_fwd(y, mean, rstd, gamma, beta, lo=LO, hi=HI, dt=F64, defect=None):
    """-> (out (M, C) = clamp(z, lo, hi), z) with z = (y - mean) rstd gamma + beta, the kernel's order of operations, in dt."""
    z = (y.to(dt) - mean.to(dt)) * rstd.to(dt) * gamma.to(dt) + beta.to(dt)
    return z.clamp(lo, hi), z


def _mask(z, lo, hi, defect):
    """The Hardtanh backward mask, the kernel's rule: z > lo && z < hi.  defect "ge_lo" / "le_hi": the boundary let through."""
    return ((z >= lo) if defect == "ge_lo" else (z > lo)) & ((z <= hi) if defect == "le_hi" else (z < hi))


def bn_act_bwd_sums(y, dout, mean, rstd, gamma, beta, keep=None, lo=LO, hi=HI, dt=F64, order=0, defect=None):
    """(sum d, sum d x^) with d = dout where lo < z < hi on a kept row, else 0; x^ = (y - mean) rstd."""
    xh = (y.to(dt) - mean.to(dt)) * rstd.to(dt)
    z = xh * gamma.to(dt) + beta.to(dt)
    m = _mask(z, lo, hi, defect)
    if keep is not None and defect != "masked_counted":
        m = m & keep[:, None]
    d = dout.to(dt) * m.to(dt)
    return _sum(d, 0, order), _sum(d * xh, 0, order)


def bn_act_bwd(y, dout, sums, mean, rstd, gamma, beta, keep=None, lo=LO, hi=HI, dt=F64, defect=None):
    """dy = gamma rstd (d - sum d / N - x^ sum (d x^) / N) on the kept rows (N = their number), 0 on the others."""
    M = y.shape[0]
    n = float(M if keep is None or defect == "count_M" else keep.sum())
    inv = torch.ones((), dtype=dt) / torch.tensor(max(n, 1.0), dtype=dt)
    xh = (y.to(dt) - mean.to(dt)) * rstd.to(dt)
    z = xh * gamma.to(dt) + beta.to(dt)
    d = dout.to(dt) * _mask(z, lo, hi, defect).to(dt)
    dy = gamma.to(dt) * rstd.to(dt) * (d - sums[0].to(dt) * inv - xh * (sums[1].to(dt) * inv))
    if keep is not None:
        dy = dy * keep.to(dt)[:, None]
    return dy


def bn_act_eval(x, dt=F64, order=0, defect=None):
    """Forward, backward sums and backward of one case -> dict(out, s, q, dy), each (M, C) / (C,) in dt."""
    keep = keep_rows(x["M"], x["valid"]) if x["valid"] is not None else None
    p = (x["mean"], x["rstd"], x["gamma"], x["beta"])
    out, z = bn_act_fwd(x["y"], *p, dt=dt)
    s, q = bn_act_bwd_sums(x["y"], x["dz"], *p, keep=keep, dt=dt, order=order, defect=defect)
    dy = bn_act_bwd(x["y"], x["dz"], (s, q), *p, keep=keep, dt=dt, defect=defect)
    return dict(out=out, z=z, s=s, q=q, dy=dy)


ACT_TENSORS = ("out", "s", "q", "dy")


def _pick(values, n, gen):
    t = torch.tensor(values, dtype=F64)
    return t[torch.randint(0, len(values), (n,), generator=gen)]


def _layout(lay, M):
    """A layout record (tH, tW, ygrid, dygrid, valid) -> the same with defaults; the row count of the mask is tW in the encoder layout."""
    return dict(tH=lay.get("tH", 0), tW=lay.get("tW", 0), ygrid=lay.get("ygrid", (0, 0)), dygrid=lay.get("dygrid", (0, 0)),
                valid=lay.get("valid"))


def count_of(M, valid):
    return M if valid is None else M // valid[1] * valid[0]


def bn_exact_case(M, C, lay, seed):
    """Integer data on which forward, sums and (for a power-of-two count) backward are exact in fp32 in any order: y in {-8 .. 8} (about
    0.43 of the elements active, against a quarter with the issue's {-24 .. 40}), mean in {-3 .. 3}, rstd in {1/2, 1, 2}, gamma in
    {+-1, +-2}, beta in {-4 .. 4}, dz in {-3 .. 3}.  Rows 0 and 1 of every column whose parameters allow it are set to the y that puts z
    exactly on lo and on hi.  -> the case dict with the float64 reference under "ref" and "dy_exact" (the count is a power of two)."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(-8, 9, (M, C), generator=gen).double()
    mean = torch.randint(-3, 4, (C,), generator=gen).double()
    rstd = _pick([0.5, 1.0, 2.0], C, gen)
    gamma = _pick([-2.0, -1.0, 1.0, 2.0], C, gen)
    beta = torch.randint(-4, 5, (C,), generator=gen).double()
    dz = torch.randint(-3, 4, (M, C), generator=gen).double()
    s = rstd * gamma
    if M >= 2:
        for row, target in ((0, LO), (1, HI)):
            want = mean + (target - beta) / s
            ok = (want == want.round()) & (want.abs() <= 64)
            y[row] = torch.where(ok, want, y[row])
    x = dict(_layout(lay, M), M=M, C=C, y=y, mean=mean, rstd=rstd, gamma=gamma, beta=beta, dz=dz)
    ref = bn_act_eval(x)
    n = count_of(M, x["valid"])
    x["dy_exact"] = n & (n - 1) == 0
    keep = keep_rows(M, x["valid"])
    xh = ((y - mean) * rstd).abs()
    d = dz.abs() * ((ref["z"] > LO) & (ref["z"] < HI)) * keep[:, None]
    guard("bn_act z", xh * gamma.abs() + beta.abs(), 0.5)
    guard("bn_act sums", torch.cat([d.sum(0), (d * xh).sum(0)]), 0.5)
    if x["dy_exact"]:
        # d - m1 - x^ m2 on the grid 1 / (4 n); the factor gamma rstd in front is a power of two
        guard("bn_act dy", dz.abs() + (ref["s"] / n).abs() + xh * (ref["q"] / n).abs(), 1.0 / (4 * n))
    assert float(dz.abs().max()) <= 256                       # the gradient is stored as bf16 in that mode
    x["ref"] = ref
    x["on_lo"], x["on_hi"] = int((ref["z"] == LO).sum()), int((ref["z"] == HI).sum())
    x["active"] = float(((ref["z"] > LO) & (ref["z"] < HI)).double().mean())
    return x


def bn_tol_case(M, C, lay, seed):
    """Random data: y ~ 6 N(0, 1) + 5, gamma in [0.5, 1.5), beta ~ N(0, 1), dz ~ N(0, 1), mean and rstd the float64 statistics of y rounded to
    fp32 (what the kernels are handed).  An element whose float64 z lies within Z_MARGIN of lo or hi is moved by 1/4 until none does.
    -> the case dict with "ref" (float64), "e32" (the float32 evaluation's error per tensor) and "scale"."""
    gen = torch.Generator().manual_seed(seed)
    y = (torch.randn(M, C, generator=gen) * 6 + 5).double()
    gamma = (torch.rand(C, generator=gen) + 0.5).double()
    beta = torch.randn(C, generator=gen).float().double()
    dz = torch.randn(M, C, generator=gen).double()
    x = dict(_layout(lay, M), M=M, C=C)
    keep = keep_rows(M, x["valid"])
    st = bn_stats(y, 1e-5, -1.0, torch.zeros(C), torch.ones(C), 0, x["valid"])
    mean, rstd = st["mean"].float().double(), st["rstd"].float().double()
    for _ in range(8):
        z = bn_act_fwd(y, mean, rstd, gamma, beta)[1]
        near = ((z - LO).abs() < Z_MARGIN) | ((z - HI).abs() < Z_MARGIN)
        if not bool(near.any()):
            break
        y = (y + 0.25 * near).float().double()
    else:
        raise AssertionError("a pre-activation stays within Z_MARGIN of the Hardtanh window")
    x.update(y=y.float().double(), mean=mean, rstd=rstd, gamma=gamma.float().double(), beta=beta, dz=dz.float().double())
    x["ref"] = bn_act_eval(x)
    z = x["ref"]["z"]
    x["margin"] = float(torch.minimum((z - LO).abs(), (z - HI).abs()).min())
    assert x["margin"] >= Z_MARGIN
    x["e32"], x["scale"] = bn_act_errors(x)
    return x


def bn_act_errors(x):
    """({tensor: error of the float32 evaluation, the worse of two orders}, {s, q: per column the sum of the absolute terms}).  out and dy:
    the largest absolute error of the M x C elements.  The two sums have C elements, one at C = 1: their error is taken relative to the sum
    of the absolute terms of the column, which makes it comparable across cases (see act_tol_case)."""
    ref = x["ref"]
    keep = keep_rows(x["M"], x["valid"])
    d = x["dz"].abs() * ((ref["z"] > LO) & (ref["z"] < HI)) * keep[:, None]
    scale = dict(s=d.sum(0), q=(d * ((x["y"] - x["mean"]) * x["rstd"]).abs()).sum(0))
    err = {t: 0.0 for t in ACT_TENSORS}
    for order in (0, 1):
        e = bn_act_eval(x, dt=F32, order=order)
        for t in ACT_TENSORS:
            dlt = (e[t].double() - ref[t]).abs()
            if t in scale:
                dlt = torch.where(scale[t] > 0, dlt / scale[t].clamp_min(1e-300), torch.zeros_like(dlt))
            err[t] = max(err[t], float(dlt.max()))
    return err, scale


def _act_layouts():
    """name -> (M, layout): both activation layouts, y compact or on a grid, dy on another grid, with and without the length mask.  In the
    encoder layout rows are (b, h, w) over (B, tH, tW) with tW odd, so M = B tH tW is no power of two; under the mask (m % tW < n) the
    count is B tH n, a power of two for tH = 2 -- there the backward is exact too; for tH = 3 it is held within b32."""
    out = collections.OrderedDict()
    for M in (64, 512, 1024):
        out["flat_M%d" % M] = (M, dict())
        out["flat_grid_M%d" % M] = (M, dict(ygrid=(11, 8), dygrid=(19, 8)))
    out["flat_valid_M512"] = (512, dict(valid=(8, 16)))                                    # count 256
    out["flat_grid_valid_M1024"] = (1024, dict(ygrid=(19, 16), dygrid=(17, 16), valid=(4, 16)))   # count 256
    out["flat_valid1_M64"] = (64, dict(valid=(1, 4)))                                      # count 16
    out["tH2_tW5_B64_valid4"] = (640, dict(tH=2, tW=5, valid=(4, 5)))                      # count 512
    out["tH2_tW5_B64_grid_valid4"] = (640, dict(tH=2, tW=5, ygrid=(8, 5), dygrid=(9, 5), valid=(4, 5)))
    out["tH2_tW7_B8"] = (112, dict(tH=2, tW=7))                                            # count 112: dy within b32
    out["tH3_tW7_B32_grid"] = (672, dict(tH=3, tW=7, ygrid=(10, 7), dygrid=(12, 7)))       # count 672: dy within b32
    out["tH3_tW5_B16_valid2"] = (240, dict(tH=3, tW=5, valid=(2, 5)))                      # count 96: dy within b32
    return out


ACT_LAYOUTS = _act_layouts()
ACT_C = (1, 32, 256)
ACT_EXACT = [Case("%s-C%d" % (name, C), (M, C, lay), "") for name, (M, lay) in ACT_LAYOUTS.items() for C in ACT_C]


@functools.lru_cache(maxsize=None)
def act_exact_case(cid):
    """The case of ACT_EXACT with that id.  The seed is the first of 40 * index + k whose data holds elements exactly on lo AND on hi
    with between a quarter and 0.65 of the elements active (a single column may admit no boundary element, or clip nearly everything)."""
    i = ids(ACT_EXACT).index(cid)
    M, C, lay = ACT_EXACT[i].args
    for k in range(40):
        x = bn_exact_case(M, C, lay, 40 * i + k)
        if x["on_lo"] > 0 and x["on_hi"] > 0 and 0.25 < x["active"] < 0.65:
            if not x["dy_exact"]:
                x["b32_dy"] = max(B32_FACTOR * float((bn_act_eval(x, dt=F32, order=o)["dy"].double() - x["ref"]["dy"]).abs().max()) for o in (0, 1))
            return x
    raise AssertionError("no seed puts an element on lo and on hi for " + cid)


def _tol_cases():
    """Random data at ragged M: the seams of the 64-row and 512-row blocks and of the 4 x nrl unroll, flat; M a whole number of tH tW in the
    encoder layout."""
    out = []
    for C in ACT_C:
        u = 4 * (256 // C)
        for M in sorted({1, 63, 65, u - 1, u + 1, 511, 513}):
            out.append(Case("flat_M%d-C%d" % (M, C), (M, C, dict()), ""))
        out.append(Case("flat_grid_valid_M585-C%d" % C, (585, C, dict(ygrid=(13, 9), dygrid=(17, 9), valid=(6, 9))), ""))
        out.append(Case("tH3_tW7_B25-C%d" % C, (525, C, dict(tH=3, tW=7, ygrid=(9, 7), dygrid=(8, 7))), ""))
        out.append(Case("tH2_tW9_B29_valid5-C%d" % C, (522, C, dict(tH=2, tW=9, valid=(5, 9))), ""))
    return out


ACT_TOL = _tol_cases()


@functools.lru_cache(maxsize=None)
def _act_tol_raw(cid):
    i = ids(ACT_TOL).index(cid)
    M, C, lay = ACT_TOL[i].args
    return bn_tol_case(M, C, lay, 7000 + i)


@functools.lru_cache(maxsize=None)
def act_tol_case(cid):
    """The case with its bounds "b32": out and dy 4 x the case's own float32 error (M x C elements); the sums s and q 4 x the float32
    error relative to the column's sum of absolute terms, pooled over the cases with the same C (ten draws per column count instead
    of one at C = 1), times that sum -- a tensor of C bounds."""
    x = dict(_act_tol_raw(cid))
    same = [_act_tol_raw(c.id) for c in ACT_TOL if c.args[1] == x["C"] and c.args[0] > 1]
    b32 = {t: B32_FACTOR * x["e32"][t] for t in ("out", "dy")}
    for t in ("s", "q"):
        b32[t] = B32_FACTOR * max(o["e32"][t] for o in same) * x["scale"][t]
    x["b32"] = b32
    return x


def stored(ref, dtype):
    """The float64 value as a kernel stores it when it is exact in fp32: one round-to-nearest-even for bf16."""
    return ref.float().to(dtype).double()


# ------------------------------------------------------------------------------------------------ the module, for the function-level test
def emb_cnn_module(dtype=F64, seed=0):
    """The reference's emb_cnn (transformer.py:83-88): Conv2d(1, 32, (41, 11), (2, 2), (0, 10)) + BatchNorm2d + Hardtanh(0, 20) +
    Conv2d(32, 32, (21, 11), (2, 1)) + BatchNorm2d + Hardtanh(0, 20), default initialisation under `seed`, BatchNorm affine parameters
    spread (gamma in [0.5, 8.5), beta ~ N(4, 3)) so that both ends of each Hardtanh clip some elements."""
    import torch.nn as nn
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Conv2d(1, 32, kernel_size=(41, 11), stride=(2, 2), padding=(0, 10)), nn.BatchNorm2d(32), nn.Hardtanh(0, 20, inplace=True),
                      nn.Conv2d(32, 32, kernel_size=(21, 11), stride=(2, 1)), nn.BatchNorm2d(32), nn.Hardtanh(0, 20, inplace=True))
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in (1, 4):
            m[i].weight.copy_(torch.rand(32, generator=gen) * 8 + 0.5)          # wide enough for both ends of Hardtanh(0, 20) to clip
            m[i].bias.copy_(torch.randn(32, generator=gen) * 3 + 4)
    return m.to(dtype)


# (B, F, T, seed): OH_A = 23, OH_B = 2.  T = 24: both convolutions take the window arms in bf16; T = 25 is odd: the first one takes the full
# im2col path.  Seeds: the first whose float64 pre-activations keep 8 x the float32 module's error away from 0 and 20
# (tests/test_embcnn_reference_host.py prints both figures; at T = 25 seeds 0 and 1 reach only 3.8 x and 3.0 x).
EMB_SHAPES = [Case("T24", (2, 85, 24, 0), "window arms"), Case("T25", (2, 85, 25, 2), "odd T: full im2col + window")]
EMB_PAD_FRAMES = 6


def emb_src(B, Fq, T, seed):
    g = torch.Generator().manual_seed(100 + T + seed)
    return (torch.randn(B, 1, Fq, T, generator=g) * 2).double()


def emb_cnn_apply(m, src):
    """transformer.py:70-76: (B, 1, F, T) -> conv -> (B, C, F', T') -> view (B, C F', T') -> transpose -> (B, T', C F')."""
    y = m(src)
    B, C, Fq, T = y.shape
    return y.view(B, C * Fq, T).transpose(1, 2).contiguous()


def emb_cnn_preacts(m, src):
    """The float64 inputs of both Hardtanh layers (training-mode BatchNorm outputs), without touching the running buffers of m."""
    import copy
    m = copy.deepcopy(m)
    a = m[1](m[0](src))
    b = m[4](m[3](m[2](a.clone())))
    return a.detach(), b.detach()
