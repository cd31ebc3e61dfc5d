"""Float64 restatement of the LSTM language model's kernels (csrc/lm.hip, csrc/lm_train.hip, csrc/lm_common.h) in plain torch on the
CPU, one function per kernel.  Every function takes a dtype so the SAME formula can be run in fp32: the tolerance of the GPU tests is four
times the error of that fp32 run against the float64 one, with a floor of one fp32 rounding of the tensor's largest entry
(tests/mwer_reference.py: bound32, excess).

The functions work on the kernels' own layouts:
    rows      time-major packed tokens: row step_off[t] + s is step t of sentence s, sentences sorted longest first;
    gates     unit-major columns, 4 j + q = gate q (i, f, g, o) of unit j;
    operands  of a contraction over K are rows of 16 * ceil(K / 16) floats whose columns [K, 16 * ceil(K / 16)) hold zeros: the
              functions contract over that padded width, as the kernels do;
    ld        the leading dimension is explicit: an argument is a 2-D view (view() below) of a flat buffer at the case's ld.  A function
              reads the rows and columns its kernel's contract names and nothing else, so whatever else the buffer holds (NaN in the GPU
              tests) cannot reach its result.
Functions return new tensors; the kernels that work in place (bptt_step on the gates and dc, sub_rows, emb_grad, colsum with accumulate)
are compared with them by the tests.

Dropout: element (row m, column c) of a site with C columns is kept iff asr_keep(seed, m * C + c, thr), m the packed row
(rowwise_reference.keep_mask restates csrc/common.h); lstm_step_train's site has C = H and m = row0 + the row of the launch."""
import functools

import numpy as np
import torch

import rowwise_reference as RW
from mwer_reference import EPS32, bound32, excess  # noqa: F401  (re-exported: the tolerance rule of the GPU tests)

F64, F32 = torch.float64, torch.float32
CHUNK = 256                       # vocabulary words per log-sum-exp partial (LM_NLL_CHUNK)
NAN = float("nan")


def pad16(k):
    return (k + 15) // 16 * 16


def view(flat, off, rows, cols, ld):
    """(rows, cols) at leading dimension ld, `off` elements into a flat buffer (ld < cols never happens; rows = 1 keeps its ld)."""
    return flat.as_strided((rows, cols), (ld, 1), off)


def keep(seed, row0, n, C, p, local=False):
    """bool (n, C): the kept elements of packed rows [row0, row0 + n) of a site with C columns.  local: the index taken from the row of
    the launch (a deliberate defect unless row0 = 0)."""
    if row0 == 0 or local:
        return torch.from_numpy(RW.keep_mask(seed, n, C, p))
    thr = RW.drop_threshold(p)[0]
    if thr == 0:
        return torch.ones((n, C), dtype=torch.bool)
    idx = (np.uint64(row0) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :]
    return torch.from_numpy(RW.hash32(seed, idx) >= np.uint64(thr))


def inv_keep(p, dtype):
    """1.f / (1.f - p) as the entry points compute it (an fp32 number), in dtype."""
    return torch.tensor(RW.drop_threshold(p)[1], dtype=dtype)


# ------------------------------------------------------------------------------------------------ csrc/lm.hip
def proj(x, w, bias, M, N, K, ids=None, dtype=F64):
    """(M, N) = X w^T + bias, X row m = x[ids[m]] or x[m]."""
    Kp = pad16(K)
    X = (x[ids.long()] if ids is not None else x[:M])[:, :Kp].to(dtype)
    return X @ w[:N, :Kp].to(dtype).t() + bias[:N].to(dtype)


def lstm_step(xproj, h_prev, whh, c_prev, n, H, dtype=F64, order=(0, 1, 2, 3), cprev_at_t0=None):
    """-> (c, h, gates): gates (n, 4H) activated i f g o, unit-major.  h_prev None: t = 0 (no recurrent product, c_prev not read).
    Defects: order = the gate each of the four packed columns is taken for; cprev_at_t0 = a c that is used although t = 0."""
    Kp = pad16(H)
    pre = xproj[:n, :4 * H].to(dtype)
    if h_prev is not None:
        pre = pre + h_prev[:n, :Kp].to(dtype) @ whh[:4 * H, :Kp].to(dtype).t()
    pre = pre.reshape(n, H, 4)
    q = [pre[:, :, k] for k in order]
    i, f, g, o = torch.sigmoid(q[0]), torch.sigmoid(q[1]), torch.tanh(q[2]), torch.sigmoid(q[3])
    cp = c_prev if h_prev is not None else cprev_at_t0
    c = i * g if cp is None else f * cp[:n, :H].to(dtype) + i * g
    h = o * torch.tanh(c)
    return c, h, torch.stack([i, f, g, o], dim=2).reshape(n, 4 * H)


def lstm_step_train(xproj, h_prev, whh, c_prev, n, n_next, H, row0, p, seed, dtype=F64, local_index=False, hnext_rows=None, **defect):
    """-> dict(c, h, gates, h_drop (n, H), h_next (n_next, H)).  Defects: local_index (the mask of row m, not row0 + m), hnext_rows (how
    many rows h_next gets), and lstm_step's."""
    c, h, gates = lstm_step(xproj, h_prev, whh, c_prev, n, H, dtype, **defect)
    k = keep(seed, row0, n, H, p, local=local_index)
    h_drop = torch.where(k, h * inv_keep(p, dtype), torch.zeros((), dtype=dtype))
    return dict(c=c, h=h, gates=gates, h_drop=h_drop, h_next=h[:n_next if hnext_rows is None else hnext_rows].clone())


def bptt_step(dh, dg_next, whh_t, g, c, c_prev, dc, n, n_next, H, dtype=F64, rec_all=False, dc_all=False):
    """One (layer, step) of back-propagation through time -> (dG (n, 4H) pre-activation gate gradients, dc (n, H) carried on).
    Rows [n_next, n) end here: no recurrent term, no carried dc (neither is read).  Defects: rec_all (the recurrent product of the
    clamped row n_next - 1 for them), dc_all (the carried dc read for them)."""
    Kp = pad16(4 * H)
    d = dh[:n, :H].to(dtype).clone()
    dcin = torch.zeros((n, H), dtype=dtype)
    if n_next > 0:
        rec = dg_next[:n_next, :Kp].to(dtype) @ whh_t[:H, :Kp].to(dtype).t()
        d[:n_next] += rec
        dcin[:n_next] = dc[:n_next, :H].to(dtype)
        if rec_all:
            d[n_next:] += rec[n_next - 1]
    if dc_all:
        dcin[n_next:] = dc[n_next:n, :H].to(dtype)
    a = g[:n, :4 * H].to(dtype).reshape(n, H, 4)
    i, f, gg, o = a[:, :, 0], a[:, :, 1], a[:, :, 2], a[:, :, 3]
    tc = torch.tanh(c[:n, :H].to(dtype))
    dcn = d * o * (1 - tc * tc) + dcin
    cp = c_prev[:n, :H].to(dtype) if c_prev is not None else torch.zeros((n, H), dtype=dtype)
    dG = torch.stack([dcn * gg * i * (1 - i), dcn * cp * f * (1 - f), dcn * i * (1 - gg * gg), d * tc * o * (1 - o)], dim=2)
    return dG.reshape(n, 4 * H), dcn * f


def nchunks(V):
    return (V + CHUNK - 1) // CHUNK


def logits_of(hid, w, bias, M, V, K, dtype=F64):
    Kp = pad16(K)
    return hid[:M, :Kp].to(dtype) @ w[:V, :Kp].to(dtype).t() + bias[:V].to(dtype)


def nll_partials(hid, w, bias, tgt, M, V, K, dtype=F64, tgt_shift=0, drop_chunk=None):
    """-> (part (M, nchunk, 2) = (max, sum exp(. - max)) of every 256-word chunk, tgt_logit (M,)).  Defects: tgt_shift (the target's
    logit taken that many columns off), drop_chunk (that chunk contributes nothing)."""
    lg = logits_of(hid, w, bias, M, V, K, dtype)
    nc = nchunks(V)
    part = torch.zeros((M, nc, 2), dtype=dtype, device=lg.device)
    for k in range(nc):
        blk = lg[:, k * CHUNK:min(V, (k + 1) * CHUNK)]
        mx = blk.max(dim=1).values
        part[:, k, 0], part[:, k, 1] = mx, torch.exp(blk - mx[:, None]).sum(dim=1)
        if drop_chunk == k:
            part[:, k, 0], part[:, k, 1] = -float("inf"), 0.0
    col = (tgt[:M].long() + tgt_shift).clamp(0, V - 1)
    return part, lg.gather(1, col[:, None])[:, 0]


def lse_of(part):
    """(M,) log-sum-exp over the chunks of the partials."""
    mx = part[:, :, 0].max(dim=1).values
    return mx + torch.log((part[:, :, 1] * torch.exp(part[:, :, 0] - mx[:, None])).sum(dim=1))


def nll_finish(part, tgt_logit, step_off, lens, dtype=F64):
    """-> (nll_tok (M,), nll_sum (S,)): token t of sequence s is row step_off[t] + s."""
    tok = lse_of(part.to(dtype)) - tgt_logit.to(dtype)
    sums = torch.zeros(len(lens), dtype=dtype, device=tok.device)
    for s, L in enumerate(int(v) for v in lens):
        for t in range(L):
            sums[s] = sums[s] + tok[int(step_off[t]) + s]
    return tok, sums


def train_loss(part, tgt_logit, M, dtype=F64):
    """-> (lse (M,), mean NLL)."""
    lse = lse_of(part[:M].to(dtype))
    return lse, (lse - tgt_logit[:M].to(dtype)).sum() / M


# ------------------------------------------------------------------------------------------------ csrc/lm_train.hip
def dlogits(hid, w, bias, lse, M, V, K, inv_n, dtype=F64):
    """(M, Vp) = softmax * inv_n in the first V columns, exact zeros up to Vp = V rounded up to 64."""
    Vp = (V + 63) // 64 * 64
    out = torch.zeros((M, Vp), dtype=dtype, device=hid.device)
    out[:, :V] = torch.exp(logits_of(hid, w, bias, M, V, K, dtype) - lse[:M].to(dtype)[:, None]) * torch.tensor(inv_n, dtype=dtype)
    return out


def sub_rows(dh, w, tgt, M, C, inv_n, dtype=F64):
    return dh[:M, :C].to(dtype) - w[tgt[:M].long(), :C].to(dtype) * torch.tensor(inv_n, dtype=dtype)


def colsum(x, M, N, out=None, accumulate=False, dtype=F64, skip_last_group=False, out2=None):
    """-> (out, out2) (N,): the column sums, added to `out` with accumulate; out2 receives the same values.  Defects: skip_last_group
    (rows 3, 7, ... are left out), out2 given (it stays as it is: stale)."""
    xs = x[:M, :N].to(dtype)
    if skip_last_group:
        xs = xs[[m for m in range(M) if m % 4 != 3]]
    v = xs.sum(dim=0) + (out[:N].to(dtype) if accumulate else 0)
    return v, (v.clone() if out2 is None else out2[:N].to(dtype))


def emb_grad(dx, rows, seg_off, seg_word, nseg, E, scale, demb, dtype=F64, seg_shift=0):
    """demb (all rows, E) with demb[seg_word[k]] += scale * sum dx[rows[seg_off[k] : seg_off[k + 1]]].  Defect: seg_shift moves both
    ends of every segment (clamped to the list)."""
    out = demb[:, :E].to(dtype).clone()
    lim = len(rows)
    for k in range(nseg):
        a, b = (min(max(int(seg_off[k + j]) + seg_shift, 0), lim) for j in (0, 1))
        out[int(seg_word[k])] += torch.tensor(scale, dtype=dtype) * dx[rows[a:b].long(), :E].to(dtype).sum(dim=0)
    return out


def sumsq(g, dtype=F64):
    return (g.to(dtype) ** 2).sum()


def dropout(x, M, C, p, seed, ids=None, dtype=F64, local_index=None):
    src = (x[ids.long()] if ids is not None else x[:M])[:, :C].to(dtype)
    k = torch.from_numpy(RW.keep_mask(seed, M, C, p, index_D=local_index))
    return torch.where(k, src * inv_keep(p, dtype), torch.zeros((), dtype=dtype))


# ------------------------------------------------------------------------------------------------ cases
def _g(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 11)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _padded(t, K):
    """t (rows, K) -> (rows, pad16(K)) with zero pad columns."""
    out = torch.zeros((t.shape[0], pad16(K)))
    out[:, :K] = t
    return out


# (M, N, K, ids, wide leading dimensions): every M, N and K of the issue at least twice
PROJ_CASES = [(1, 4, 1, False, False), (16, 36, 15, True, False), (63, 128, 16, False, True), (65, 132, 17, True, True),
              (65, 128, 40, False, False), (1, 132, 40, True, False), (16, 4, 17, False, True), (63, 36, 40, True, True),
              (65, 36, 1, False, False), (16, 128, 15, True, True), (63, 132, 16, False, False), (1, 128, 17, True, False)]


@functools.lru_cache(maxsize=None)
def proj_case(M, N, K, ids, wide):
    """Integers in [-3, 3]; with ids x is a 9-row table and the ids repeat and contain 0."""
    g = _g(M, N, K, ids)
    rows = 9 if ids else M
    c = dict(M=M, N=N, K=K, x=_padded(_ints(g, (rows, K), -3, 3), K), w=_padded(_ints(g, (N, K), -3, 3), K), bias=_ints(g, (N,), -3, 3),
             ldx=pad16(K) + (8 if wide else 0), ldw=pad16(K), ldo=N + (12 if wide else 0), ids=None)
    if ids:
        c["ids"] = torch.randint(0, rows, (M,), generator=g).int()
        c["ids"][0] = 0
        if M > 2:
            c["ids"][2] = c["ids"][1]
    return c


STEP_H, STEP_N = (1, 3, 6, 18, 66), (1, 16, 17, 65)


@functools.lru_cache(maxsize=None)
def step_case(H, n, seed=0):
    """Random data of one step: about a third of the gate pre-activations x 8 (saturated gates), h_prev in (-1, 1) with zero pad
    columns, W_hh of unit row norm."""
    g = _g(H, n, seed, 3)
    r = lambda *s: torch.randn(*s, generator=g)
    xproj = r(n, 4 * H) * torch.where(torch.rand(n, 4 * H, generator=g) < 0.3, 8.0, 1.0)
    return dict(H=H, n=n, xproj=xproj, h_prev=_padded(torch.tanh(r(n, H)), H), whh=_padded(r(4 * H, H) / H ** 0.5, H), c_prev=r(n, H))


def _acts(g, n, H, exact):
    """Activated gates (n, 4H)."""
    if exact:
        a = torch.tensor([0.0, 0.5, 0.5, 0.5, 1.0])[torch.randint(0, 5, (n, H, 4), generator=g)]              # 0, 1/2 (mostly), 1
        a[:, :, 2] = torch.tensor([-1.0, -0.5, -0.5, 0.0, 0.5, 0.5, 1.0])[torch.randint(0, 7, (n, H), generator=g)]    # g: 0, +-1/2, +-1
        a[0, 0] = torch.tensor([0.5, 0.5, 0.5, 1.0])
    else:
        a = torch.rand(n, H, 4, generator=g) * 0.98 + 0.01
        a[:, :, 2] = a[:, :, 2] * 2 - 1
    return a.reshape(n, 4 * H)


BPTT_EXACT = [(1, 1, 0), (6, 17, 5), (18, 16, 16), (66, 65, 33), (66, 64, 0)]


@functools.lru_cache(maxsize=None)
def bptt_case(H, n, n_next, exact, poison=NAN):
    """exact: gates from {0, 1/2, 1} (g from {0, +-1/2, +-1}), c = 0, c_prev halves, dc eighths, dh / dg_next / W_hh^T small integers:
    every product and sum is exact in fp32 in any order.  Otherwise random activations in the open interval and random c.
    dg_next has n rows, rows >= n_next hold `poison`, as do rows [n_next, n) of dc; its columns [4H, pad16(4H)) hold zeros."""
    g = _g(H, n, n_next, exact, 5)
    G = pad16(4 * H)
    if exact:
        dh, dgn, wt = _ints(g, (n, H), -2, 2), _ints(g, (n, 4 * H), -2, 2), _ints(g, (H, 4 * H), -1, 1)
        c, cp, dc = torch.zeros(n, H), _ints(g, (n, H), -3, 3) / 2, _ints(g, (n, H), -8, 8) / 8
        dh[0, 0], cp[0, 0] = 1.0, 0.5
    else:
        r = lambda *s: torch.randn(*s, generator=g)
        dh, dgn, wt, c, cp, dc = r(n, H), r(n, 4 * H) * 0.3, r(H, 4 * H) / H ** 0.5, r(n, H), r(n, H), r(n, H)
    dg_next, whh_t = torch.zeros(n, G), torch.zeros(H, G)
    dg_next[:, :4 * H], whh_t[:, :4 * H] = dgn, wt
    dg_next[n_next:] = poison
    dc[n_next:] = poison
    return dict(H=H, n=n, n_next=n_next, dh=dh, dg_next=dg_next, whh_t=whh_t, g=_acts(g, n, H, exact), c=c, c_prev=cp, dc=dc)


NLL_V, NLL_M, NLL_K = (1, 63, 64, 65, 255, 256, 257, 1025), (1, 63, 65, 300), 24
LENS = {1: [1], 63: [30, 20, 10, 2, 1], 65: [65], 300: [70, 66, 64, 50, 30, 19, 1]}       # a length above 64; S no multiple of 4


def packing(lens):
    """-> (step_off (T,), n_t (T,)) of sentences sorted longest first."""
    n_t = [sum(1 for L in lens if L > t) for t in range(max(lens))]
    return [sum(n_t[:t]) for t in range(len(n_t))], n_t


@functools.lru_cache(maxsize=None)
def nll_case(V, M, K=NLL_K):
    """hid, w with zero pad columns, logits x 30, an integer bias in [-2, 2]; row M // 2 of hid is zero: its logits are the bias, a row
    of ties.  Targets: column 0, V - 1 and both sides of every sub-tile / chunk / workgroup edge below V first, random afterwards."""
    g = _g(V, M, K, 9)
    hid, w = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * (30.0 / K ** 0.5)
    hid[M // 2] = 0.0
    edges = [v for v in (0, V - 1, 63, 64, 65, 255, 256, 257, 1023, 1024) if 0 <= v < V]
    tgt = torch.randint(0, V, (M,), generator=g).int()
    for m in range(min(M, len(edges))):
        tgt[(m * 7) % M if M > 7 * len(edges) else m] = edges[m]
    lens = LENS[M]
    off, _ = packing(lens)
    return dict(V=V, M=M, K=K, hid=_padded(hid, K), w=_padded(w, K), bias=_ints(g, (V,), -2, 2), tgt=tgt, lens=torch.tensor(lens).int(),
                step_off=torch.tensor(off).int(), inv_n=1.0 / M)


LOSS_M = (1, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def loss_case(M, nchunk=3):
    g = _g(M, nchunk, 13)
    part = torch.stack([torch.randn(M, nchunk, generator=g) * 10, 1 + 50 * torch.rand(M, nchunk, generator=g)], dim=2)
    return dict(M=M, nchunk=nchunk, part=part.contiguous(), tgt_logit=torch.randn(M, generator=g) * 10)


COLSUM_M, COLSUM_N = (0, 1, 3, 4, 5, 1001), (1, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def colsum_case(M, N):
    g = _g(M, N, 17)
    x = _ints(g, (M, N), -3, 3)
    x[:1, :1] = 2.0                                          # a single-column sum is not zero by chance
    return dict(M=M, N=N, x=x, out=_ints(g, (N,), -5, 5) * 2 + 1, ld=N + 3)


EMB_NSEG, EMB_E, EMB_LEN = (1, 4, 5), (1, 63, 64, 65, 130), (1, 40)


@functools.lru_cache(maxsize=None)
def emb_case(nseg, E, seglen):
    """nseg words (of 2 nseg + 1 rows of the table, word 0 among them) with seglen tokens each; the token rows are a permutation
    within ascending order per word; demb starts from odd integers."""
    g = _g(nseg, E, seglen, 19)
    R = nseg * seglen
    words = torch.randperm(2 * nseg + 1, generator=g)[:nseg].sort().values.int()
    words[0] = 0
    rows = torch.randperm(R, generator=g).reshape(nseg, seglen).sort(dim=1).values.reshape(-1).int()
    return dict(nseg=nseg, E=E, dx=_ints(g, (R, E), -3, 3), rows=rows, seg_off=(torch.arange(nseg + 1) * seglen).int(), seg_word=words,
                demb=_ints(g, (2 * nseg + 1, E), -5, 5) * 2 + 1, scale=-0.25, ldx=E + 2, ldd=E + 5)


SUMSQ_N = (0, 1, 255, 65536, 65537, 200001)


@functools.lru_cache(maxsize=None)
def sumsq_case(n):
    g = _ints(_g(n, 23), (n,), -1, 1)
    g[:1] = 1.0
    return g


SUB_CASES = [(1, 1), (5, 63), (17, 256), (33, 257)]


@functools.lru_cache(maxsize=None)
def sub_case(M, C):
    g = _g(M, C, 29)
    return dict(M=M, C=C, dh=_ints(g, (M, C), -3, 3) * 2 + 1, w=_ints(g, (7, C), -3, 3), tgt=torch.randint(0, 7, (M,), generator=g).int(), inv_n=0.125)


DROP_C, DROP_P, DROP_M = (1, 255, 256, 257), (0.0, 0.3), 5


@functools.lru_cache(maxsize=None)
def drop_case(C, ids):
    """x = +- powers of two, so that x * 1.f / (1.f - p) is one exact fp32 product: the fp32 and float64 evaluations agree to the bit."""
    g = _g(C, ids, 31)
    rows = 9 if ids else DROP_M
    x = (_ints(g, (rows, C), 0, 1) * 2 - 1) * 2.0 ** _ints(g, (rows, C), -3, 3)
    return dict(C=C, M=DROP_M, x=x, ids=torch.tensor([3, 0, 3, 8, 1]).int() if ids else None, seed=0x1234567 + C)


# ------------------------------------------------------------------------------------------------ what the tests compare
def step_ref(c, prev, dtype=F64, train=None, **defect):
    """The outputs of lstm_step (train None) or lstm_step_train (train = dict(n_next, row0, p, seed)) on a step_case."""
    hp, cp = (c["h_prev"], c["c_prev"]) if prev else (None, None)
    if train is None:
        cc, h, gates = lstm_step(c["xproj"], hp, c["whh"], cp, c["n"], c["H"], dtype, **defect)
        return dict(c=cc, h=h, gates=gates)
    return lstm_step_train(c["xproj"], hp, c["whh"], cp, c["n"], train["n_next"], c["H"], train["row0"], train["p"], train["seed"], dtype,
                           **defect)


def bptt_ref(c, with_cprev, dtype=F64, **defect):
    dG, dc = bptt_step(c["dh"], c["dg_next"] if c["n_next"] else None, c["whh_t"], c["g"], c["c"], c["c_prev"] if with_cprev else None,
                       c["dc"], c["n"], c["n_next"], c["H"], dtype, **defect)
    return dict(dG=dG, dc=dc)


def nll_ref(c, dtype=F64, **defect):
    """Everything the output layer's kernels give for an nll_case: per-token NLL, per-sequence sums, lse, the mean, softmax * inv_n,
    and the target's probability exp(tgt_logit - lse)."""
    part, tl = nll_partials(c["hid"], c["w"], c["bias"], c["tgt"], c["M"], c["V"], c["K"], dtype, **defect)
    tok, sums = nll_finish(part, tl, c["step_off"], c["lens"], dtype)
    lse, loss = train_loss(part, tl, c["M"], dtype)
    return dict(tok=tok, sums=sums, lse=lse, loss=loss.reshape(1), tgt_prob=torch.exp(tl - lse),
                dl=dlogits(c["hid"], c["w"], c["bias"], lse, c["M"], c["V"], c["K"], c["inv_n"], dtype))


def ratios(got, ref64, ref32, names=None):
    """{name: excess(got, ref64, bound32(ref64, ref32))} per tensor: the project's rule, <= 1 inside the bound."""
    return {k: excess(got[k], ref64[k], bound32(ref64[k], ref32[k])) for k in (names or ref64)}


SENT = 7.25                      # what an output buffer holds before a launch


def in_buffer(t, rows, fill=SENT):
    """t written into the first rows of a (rows, cols) buffer of `fill`: what a kernel that writes t leaves behind."""
    out = torch.full((rows, t.shape[1]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out
