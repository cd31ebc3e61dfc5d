"""Plain references for the attention kernels (tests/test_attention_reference_host.py, tests/test_gpu_attention_arms.py).

keep_mask / effective_seed   NumPy restatement of the dropout mask of csrc/attention.h (drop_row_key, drop_pair_bits, drop_keep) and of
                             asr_mix_seed (csrc/common.h): what the kernels drop is known on the host, so the backward under dropout can be
                             compared with a reference instead of with another kernel.
reference                    float64 attention with that mask, gradients by autograd, on the operands as the kernel sees them.
emulation                    the same mathematics with bf16 storage where a bf16 flash kernel must round; it only measures what bf16 rounding
                             costs on a case's data: the bound of a case is BOUND_FACTOR x its worst slice error.
slice_errors                 relative L2 error per (batch, head, 64 consecutive rows): one lost key at a length edge moves such a slice by
                             5-60 %, honest bf16 rounding by 0.25 %; a whole-tensor max-abs bound cannot tell them apart.
CASES                        the dispatch arms, layouts and masks of tests/test_gpu_attention_arms.py; the CPU test applies deliberate defects
                             (DEFECTS) to the reference on the same data and shows that the bound catches each.
"""
import numpy as np
import torch

BOUND_FACTOR = 3.0        # a different but legitimate order of rounding (rescale before / after the bf16 round, exp2 against exp)
B, H = 2, 3               # B != H everywhere: a swapped (b, h) in the dropout row index changes the mask
SCALE = 0.125
P_DROP = 0.1
SEED = ((0x1234567 + 41) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ dropout mask
def drop_threshold(p):
    """(thr, inv_keep) as fill_common() of csrc/attention.hip quantises them."""
    thr = min(int(np.float32(p) * np.float32(65536.0) + np.float32(0.5)), 65535)
    inv_keep = np.float32(1.0) / (np.float32(1.0) - np.float32(thr) / np.float32(65536.0))
    return thr, float(inv_keep)


def _mul32(a, c):
    return (a * np.uint64(c)) & _M32


def keep_mask(seed_eff, B, H, Tq, Tk, p, swap_bh=False):
    """(bool (B, H, Tq, Tk), inv_keep): True where key k of row (b, h, q) is kept.  swap_bh: the row index built as (b * H + h) * Tq + q,
    a deliberate defect for the sensitivity check."""
    thr, inv_keep = drop_threshold(p)
    seed_eff = int(seed_eff) & 0xFFFFFFFFFFFFFFFF
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    h = np.arange(H, dtype=np.uint64)[None, :, None]
    q = np.arange(Tq, dtype=np.uint64)[None, None, :]
    row = (((b * np.uint64(H) + h) if swap_bh else (h * np.uint64(B) + b)) * np.uint64(Tq) + q) & _M32
    row_key = (np.uint64(seed_eff & 0xFFFFFFFF) + _mul32(np.uint64(seed_eff >> 32), 0x85EBCA6B) + _mul32(row, 0x9E3779B1)) & _M32
    pair = np.arange((Tk + 1) // 2, dtype=np.uint64)
    y = _mul32((row_key[..., None] + pair) & _M32, 0xC2B2AE35)
    y ^= y >> np.uint64(15)
    y = _mul32(y, 0x27D4EB2F)
    y ^= y >> np.uint64(13)
    field = np.stack([y & np.uint64(0xFFFF), y >> np.uint64(16)], axis=-1).reshape(B, H, Tq, -1)[..., :Tk]   # even key: low field
    return field >= np.uint64(thr), inv_keep


def effective_seed(seed, ops):
    """asr_mix_seed: the host seed plus the device step counter (read back, not assumed) when asr_hip.ops holds a step state."""
    st = ops._cfg["state"]
    if st is None:
        return int(seed)
    s0 = int(st[0].item()) & 0xFFFFFFFFFFFFFFFF
    return (int(seed) + s0 * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------------ mathematics
def live_keys(B, Tq, Tk, key_len, key_pad, causal):
    """bool (B, 1, Tq, Tk): key k takes part in row q of batch entry b."""
    live = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if key_len is not None:
        live &= (torch.arange(Tk)[None, :] < key_len[:, None].long())[:, None, None, :]
    if key_pad is not None:
        kp = key_pad.bool()
        live &= ~(kp[:, None, None, :] if kp.dim() == 2 else kp[:, None])
    if causal:
        live &= ~torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), diagonal=1)[None, None]
    return live


def _heads(x, H, d):
    return x.view(x.shape[0], x.shape[1], H, d).permute(0, 2, 1, 3)


def _rows(x):
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], -1)


def _mask64(mask, shape):
    return torch.ones(shape, dtype=torch.float64) if mask is None else torch.as_tensor(np.asarray(mask)).to(torch.float64).expand(shape)


def reference(q, k, v, do, H, d, key_len, key_pad, causal, scale, mask, inv_keep, live=None, dp_inv_keep=None):
    """float64: a = softmax(masked scores) * mask * inv_keep, o = a @ v, gradients by autograd.  Returns a dict of o (B, Tq, H d),
    lse (B, H, Tq; natural log, +inf for a row without a live key), probs (B, H, Tq, Tk; dropped), dq, dk, dv.  A row without a live key
    gives o = 0, probabilities 0 and no contribution to any gradient.
    live / dp_inv_keep exist for the sensitivity check: another liveness pattern, and another rescale on the backward side only."""
    Bn, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    if live is None:
        live = live_keys(Bn, Tq, Tk, key_len, key_pad, causal)
    live = live.expand(Bn, H, Tq, Tk)
    q64, k64, v64 = (t.double().clone().requires_grad_() for t in (q, k, v))
    s = _heads(q64, H, d) @ _heads(k64, H, d).transpose(-1, -2) * scale
    dead = ~live.any(-1, keepdim=True)
    s = torch.where(live | dead, s, torch.full_like(s, float("-inf")))          # a dead row keeps finite scores: its softmax is multiplied by 0
    lse = torch.logsumexp(s, -1)
    a = torch.softmax(s, -1) * live.double()
    keep = _mask64(mask, a.shape)
    ad = a * keep * inv_keep
    vh = _heads(v64, H, d)
    o = _rows(ad @ vh)
    if dp_inv_keep is None:
        o.backward(do.double())
    else:      # the same value; the gradient reaches V through ad and the scores through a * keep * dp_inv_keep (dP without its rescale)
        x = a * keep * dp_inv_keep
        (_rows(ad.detach() @ vh) + _rows((x - x.detach()) @ vh.detach())).backward(do.double())
    lse = torch.where(dead[..., 0], torch.full_like(lse, float("inf")), lse).detach()
    return dict(o=o.detach(), lse=lse, probs=ad.detach(), dq=q64.grad, dk=k64.grad, dv=v64.grad)


def _bf(x):
    return x.to(torch.bfloat16).double()


def emulation(q, k, v, do, H, d, key_len, key_pad, causal, scale, mask, inv_keep, o32=True):
    """The rounding points of a bf16 flash kernel: fp32 scores, the dropped P rounded to bf16 before P.V, O rounded from an fp32 accumulator,
    delta from the fp32 O (o32=False: from the rounded O, the o32=None call form), dS rounded to bf16, dQ / dK / dV rounded from fp32.
    Accumulations are exact (float64).  Returns o, o32, dq, dk, dv."""
    Bn, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    live = live_keys(Bn, Tq, Tk, key_len, key_pad, causal).expand(Bn, H, Tq, Tk)
    qh, kh, vh, doh = (_heads(t.double(), H, d) for t in (q, k, v, do))
    s = (qh @ kh.transpose(-1, -2)).float().double() * scale
    dead = ~live.any(-1, keepdim=True)
    s = torch.where(live | dead, s, torch.full_like(s, float("-inf")))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m).float().double() * live.double()
    l = e.sum(-1, keepdim=True)
    l = torch.where(l == 0, torch.ones_like(l), l)             # a row without a live key: zeros everywhere
    keep = _mask64(mask, e.shape)
    o_acc = (_bf(e * keep) @ vh) / l * inv_keep
    o_f32 = o_acc.float().double()
    o = _bf(o_f32)
    p = (e / l).float().double()
    dp = (doh @ vh.transpose(-1, -2)).float().double()
    delta = (doh * (o_f32 if o32 else o)).sum(-1, keepdim=True).float().double()
    dv = _bf(_bf(p * keep * inv_keep).transpose(-1, -2) @ doh)
    ds = _bf(p * (keep * inv_keep * dp - delta))
    dq = _bf(ds @ kh * scale)
    dk = _bf(ds.transpose(-1, -2) @ qh * scale)
    return dict(o=_rows(o), o32=_rows(o_f32), dq=_rows(dq), dk=_rows(dk), dv=_rows(dv))


def slice_errors(got, ref, H, d, rows=64):
    """Relative L2 error of got (B, T, H d) against ref per (batch, head, block of `rows` consecutive rows), as a (B, H, blocks) tensor.  A
    slice whose reference is identically zero must be exactly zero in got: it counts 0 then, and +inf otherwise (a non-finite got
    counts +inf as well), so that it fails every bound instead of leaving the comparison."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    Bn, T, _ = ref.shape
    nb = (T + rows - 1) // rows
    pad = nb * rows - T
    diff = got - ref

    def per_slice(x):
        x = torch.nn.functional.pad(x.view(Bn, T, H, d), (0, 0, 0, 0, 0, pad))
        return (x.view(Bn, nb, rows, H, d) ** 2).sum((2, 4)).permute(0, 2, 1)

    num, den = per_slice(diff), per_slice(ref)
    err = torch.sqrt(num / den.clamp_min(1e-300))
    err = torch.where(den == 0, torch.where(per_slice(got) == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))), err)
    return torch.where(torch.isfinite(num), err, torch.full_like(err, float("inf")))


def bounds(case, x, mask, inv_keep, o32=True):
    """{tensor: bound} of a case: BOUND_FACTOR x the worst slice error of the emulation against the reference on the case's data; fp32 cases
    use the fp32 tolerance of tests/test_gpu_ops.py per slice."""
    if case["dtype"] == torch.float32:
        from test_gpu_ops import tol
        return {t: tol(torch.float32) for t in ("o", "o32", "dq", "dk", "dv")}
    ref = cached_reference(case, x, mask, inv_keep)
    emu = emulation(x["q"], x["k"], x["v"], x["do"], H, case["d"], x["key_len"], x["key_pad"], case["causal"], SCALE, mask, inv_keep, o32=o32)
    out = {}
    for t in ("o", "o32", "dq", "dk", "dv"):
        e = slice_errors(emu[t], ref["o" if t == "o32" else t], H, case["d"])
        assert torch.isfinite(e).all(), (case["name"], t)
        out[t] = BOUND_FACTOR * float(e.max())
    return out


_ref_cache = {}


def cached_reference(case, x, mask, inv_keep):
    """The float64 reference of a case with its unchanged seed: computed once per process and shared (callers leave it unchanged)."""
    key = (case["name"], None if mask is None else hash(np.asarray(mask).tobytes()))
    if key not in _ref_cache:
        _ref_cache[key] = reference(x["q"], x["k"], x["v"], x["do"], H, case["d"], x["key_len"], x["key_pad"], case["causal"], SCALE, mask,
                                    inv_keep)
    return _ref_cache[key]


# ------------------------------------------------------------------------------------------------ cases
def _case(name, Tq, Tk, layout, key_len=None, pad=None, causal=False, p=P_DROP, dtype=torch.bfloat16, d=64, arms="", flip_seen=True):
    return dict(flip_seen=flip_seen, name=name, Tq=Tq, Tk=Tk, layout=layout, key_len=key_len, pad=pad, causal=causal, p=p, dtype=dtype, d=d, arms=arms)


# layouts: qkv = column slices of one (B, T, 3 HD) buffer; kv = Q contiguous, K | V slices of (B, Tk, 2 HD); stack = K | V are layer 1's slices
# of a two-layer (B, Tk, 2 * 2 HD) buffer; plain = contiguous; padded = row stride HD + 4 (no 16-byte rows: the generic kernels' scalar path)
# flip_seen=False: one flipped mask bit at an ORDINARY row (query Tq // 2, its last live key) stays under this case's bound; the flip at the
# most sensitive row is caught in every case (tests/test_attention_reference_host.py)
CASES = [
    _case("pp_drop_161x401", 161, 401, "kv", key_len=[401, 259], arms="pp DROP (1 full block, 32 + 1 tail) / both"),
    _case("pp_self_417", 417, 417, "qkv", key_len=[417, 385], arms="pp / both, self attention"),
    _case("pp_self_417_p0", 417, 417, "qkv", key_len=[417, 385], p=0.0, arms="pp / both, no dropout"),
    _case("pp_tail_100x384", 100, 384, "stack", key_len=[384, 70], arms="pp, tail blocks only / both", flip_seen=False),
    _case("fwd2_300x383", 300, 383, "kv", key_len=[383, 200], arms="fwd<2> (Tk one short of pp) / both", flip_seen=False),
    _case("fwd2_300x383_p0", 300, 383, "kv", key_len=[383, 200], p=0.0, arms="fwd<2, no dropout> / both"),
    _case("fwd2_causal_300", 300, 300, "qkv", key_len=[300, 131], pad="tail", causal=True, arms="fwd<2> causal / both causal", flip_seen=False),
    _case("fwd2_mask3d_257", 257, 257, "plain", pad="3d", arms="fwd<2> / both, 3-D mask"),
    _case("fwd1_fused2_256", 256, 256, "qkv", key_len=[256, 129], arms="fwd<1> (Tq 256) / fused<2> (Tk 256)"),
    _case("fwd1_both_100x257", 100, 257, "stack", key_len=[257, 64], arms="fwd<1> / both (Tk 257)"),
    _case("fwd1_both_100x257_p0", 100, 257, "stack", key_len=[257, 64], p=0.0, arms="fwd<1, no dropout> / both"),
    _case("fwd1_fused1_100x128", 100, 128, "kv", key_len=[128, 77], arms="fwd<1> / fused<1> (Tk 128)", flip_seen=False),
    _case("fwd1_fused2_100x129", 100, 129, "kv", key_len=[129, 65], arms="fwd<1> / fused<2> (Tk 129)"),
    _case("fwd1_causal_65", 65, 65, "qkv", pad="tail", causal=True, arms="fwd<1> causal / fused<1>"),
    # Tk >= 384 where the long-sequence kernel must be refused: it reads neither key-padding bytes nor a causal mask
    _case("fwd1_pad_100x384", 100, 384, "kv", pad="tail", arms="fwd<1> (pp refused: padding bytes) / both", flip_seen=False),
    _case("fwd2_causal_385", 385, 385, "qkv", key_len=[385, 300], causal=True, arms="fwd<2> (pp refused: causal) / both", flip_seen=False),
    # a batch entry without a single live key, once on each of pp, fwd<2>, fwd<1>, fused<1>, fused<2> and both
    _case("dead_pp_161x401", 161, 401, "kv", key_len=[401, 0], arms="fully masked entry: pp / both"),
    _case("dead_fwd2_300x383", 300, 383, "kv", key_len=[383, 0], arms="fully masked entry: fwd<2> / both", flip_seen=False),
    _case("dead_fwd1_256", 256, 256, "qkv", key_len=[256, 0], arms="fully masked entry: fwd<1> / fused<2>", flip_seen=False),
    _case("dead_fwd1_100x257", 100, 257, "stack", key_len=[257, 0], arms="fully masked entry: fwd<1> / both"),
    _case("dead_fwd1_100x128", 100, 128, "kv", key_len=[128, 0], arms="fully masked entry: fwd<1> / fused<1>"),
    _case("generic_scalar_70x130", 70, 130, "padded", key_len=[130, 67], arms="generic bf16 d = 64, scalar path (vec = 0)"),
    _case("generic_f32_d64_70x130", 70, 130, "plain", key_len=[130, 67], dtype=torch.float32, arms="generic fp32 d = 64"),
    _case("generic_f32_d64_causal_70", 70, 70, "plain", pad="tail", causal=True, dtype=torch.float32, arms="generic fp32 d = 64, causal + pad"),
    _case("generic_f32_d32_70x130", 70, 130, "plain", key_len=[130, 67], dtype=torch.float32, d=32, arms="generic fp32 d = 32"),
    _case("generic_f32_d16_causal_70", 70, 70, "plain", pad="tail", causal=True, dtype=torch.float32, d=16, arms="generic fp32 d = 16, causal + pad"),
    _case("generic_bf16_d32_70x130", 70, 130, "plain", key_len=[130, 67], d=32, arms="generic bf16 d = 32"),
    _case("generic_bf16_d32_causal_70", 70, 70, "plain", pad="tail", causal=True, d=32, arms="generic bf16 d = 32, causal + pad"),
    _case("generic_bf16_d16_70x130", 70, 130, "plain", key_len=[130, 67], d=16, arms="generic bf16 d = 16"),
    _case("generic_bf16_d16_causal_70", 70, 70, "plain", pad="tail", causal=True, d=16, arms="generic bf16 d = 16, causal + pad"),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def key_ends(case, x):
    """Per batch entry, one past its last live key (key_len, or where the 2-D pad tail starts); None under a 3-D mask."""
    if case["pad"] == "3d":
        return None
    end = [case["Tk"]] * B
    if case["key_len"] is not None:
        end = [min(e, kl) for e, kl in zip(end, case["key_len"])]
    if case["pad"] == "tail":
        end = [min(e, case["Tk"] - 7 * (b + 1)) for b, e in enumerate(end)]
    return end


def make_inputs(case):
    """CPU operands of a case, already rounded to its dtype: q, k, v, do (B, T, H d), key_len (int32 or None), key_pad (uint8 or None).
    The K rows at keys 0, 63, 64 and end - 1 and the Q rows at 0, 63, 64 and Tq - 1 have twice the norm, so that the edges carry weight."""
    Tq, Tk, d, dtype = case["Tq"], case["Tk"], case["d"], case["dtype"]
    g = torch.Generator().manual_seed(1000 * Tq + Tk + d + len(case["name"]))
    q, k, v, do = (torch.randn(B, T, H * d, generator=g) for T in (Tq, Tk, Tk, Tq))
    key_len = torch.tensor(case["key_len"], dtype=torch.int32) if case["key_len"] is not None else None
    key_pad = None
    if case["pad"] == "tail":
        key_pad = torch.zeros(B, Tk, dtype=torch.uint8)
        for b in range(B):
            key_pad[b, Tk - 7 * (b + 1):] = 1
    elif case["pad"] == "3d":
        key_pad = (torch.rand(B, Tq, Tk, generator=g) > 0.7).to(torch.uint8)
        key_pad[:, :, 0] = 0
    x = dict(key_len=key_len, key_pad=key_pad)
    ends = key_ends(case, x) or [Tk] * B
    for b in range(B):
        for kk in {0, 63, 64, ends[b] - 1}:
            if 0 <= kk < Tk:
                k[b, kk] *= 2.0
        for qq in {0, 63, 64, Tq - 1}:
            if qq < Tq:
                q[b, qq] *= 2.0
    x.update(q=q.to(dtype).float(), k=k.to(dtype).float(), v=v.to(dtype).float(), do=do.to(dtype).float())
    return x


# ------------------------------------------------------------------------------------------------ deliberate defects (CPU sensitivity check)
# a single flipped bit at an ORDINARY row moves one probability of ~1 / Tk in a slice of 64 rows: whether the bound sees it depends on the case
# (tests/test_attention_reference_host.py records it per case and asserts nothing about it)
REPORTED_DEFECTS = ("bit_flip_ordinary_row",)
DEFECTS = ("key_len_minus_1", "causal_diagonal_excluded", "row_mask_rotated", "inv_keep_omitted_from_dp", "b_h_swapped", "bit_flip_last_live_key")


def defective_reference(case, x, mask, inv_keep, defect):
    """The reference with one deliberate defect, or None where the defect cannot act on the case (it changes nothing there): no dropout for
    the four mask defects, no causal mask for the diagonal, no key length (a 3-D mask) for the length."""
    Tq, Tk, d = case["Tq"], case["Tk"], case["d"]
    live = live_keys(B, Tq, Tk, x["key_len"], x["key_pad"], case["causal"])
    ends = key_ends(case, x)
    kw = {}
    if defect == "key_len_minus_1":
        if ends is None:
            return None
        # an entry whose length is below Tk and, so that a causal case sees it, below Tq; else (non-causal) any entry with a live key
        cand = [b for b in range(B) if 0 < ends[b] < Tk and ends[b] < Tq] or ([] if case["causal"] else [b for b in range(B) if ends[b] > 0])
        if not cand:
            return None
        live = live.clone()
        live[cand[0], :, :, ends[cand[0]] - 1] = False
    elif defect == "causal_diagonal_excluded":
        if not case["causal"]:
            return None
        live = live & ~torch.eye(Tq, Tk, dtype=torch.bool)[None, None]
    elif mask is None:
        return None
    elif defect == "row_mask_rotated":
        mask = mask.copy()
        mask[0, H - 1, Tq // 2] = np.roll(mask[0, H - 1, Tq // 2], 1)          # entry 0 has live keys in every case
    elif defect == "inv_keep_omitted_from_dp":
        kw["dp_inv_keep"] = 1.0
    elif defect == "b_h_swapped":
        mask = keep_mask(SEED, B, H, Tq, Tk, case["p"], swap_bh=True)[0]
    elif defect == "bit_flip_last_live_key":
        # one bit, at a row's last live key; of all rows (b, h, q) with at least 32 live keys (not the first rows of a causal mask, whose
        # one or two keys carry the whole row) the one whose undropped probability there is largest: the single bit that moves the most
        lv = live.expand(B, H, Tq, Tk)
        sc = (_heads(x["q"].double(), H, d) @ _heads(x["k"].double(), H, d).transpose(-1, -2) * SCALE).masked_fill(~lv, float("-inf"))
        a = torch.nan_to_num(torch.softmax(sc, -1), nan=0.0)
        last = Tk - 1 - torch.flip(lv, (-1,)).int().argmax(-1)                  # (B, H, Tq); rows without a live key have a = 0
        at_last = a.gather(-1, last[..., None])[..., 0].masked_fill(lv.sum(-1) < 32, -1.0)
        b, h, qq = np.unravel_index(int(at_last.argmax()), at_last.shape)
        mask = mask.copy()
        mask[b, h, qq, int(last[b, h, qq])] ^= True
    elif defect == "bit_flip_ordinary_row":
        # the same single bit at a fixed, ordinary row: entry 0, the last head, query Tq // 2, that row's last live key
        kk = int(torch.nonzero(live[0, 0, Tq // 2])[-1])
        mask = mask.copy()
        mask[0, H - 1, Tq // 2, kk] ^= True
    else:
        raise ValueError(defect)
    return reference(x["q"], x["k"], x["v"], x["do"], H, d, x["key_len"], x["key_pad"], case["causal"], SCALE, mask, inv_keep, live=live, **kw)


def lse_tolerance(ref_lse):
    """Absolute tolerance of an lse comparison: the fp32 tolerance of tests/test_gpu_ops.py of the largest finite |lse|."""
    from test_gpu_ops import tol
    fin = ref_lse[torch.isfinite(ref_lse)]
    return tol(torch.float32) * max(float(fin.abs().max()) if fin.numel() else 0.0, 1.0)


def lse_mismatch(got, ref):
    """Rows at which got is not the reference's lse: +inf on one side only, or further than lse_tolerance()."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    inf_g, inf_r = torch.isposinf(got), torch.isposinf(ref)
    bad = inf_g != inf_r
    both = ~inf_g & ~inf_r
    bad |= both & ~((got - ref).abs() <= lse_tolerance(ref))
    return bad
