"""tests/lm_reference.py on the CPU (no GPU): that the float64 restatement of the LSTM language model's kernels IS the operation (its
forward and backward chained over a packed batch reproduce torch autograd through nn.LSTM), that the exact cases of
tests/test_gpu_lm_arms.py are exact in fp32 and not degenerate, and that the bounds of that file catch deliberate defects."""
import os
import re

import numpy as np
import pytest
import torch

import lm_reference as R
import rowwise_reference as RW

F64, F32 = torch.float64, torch.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "end2end-asr-pytorch_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the mask
def _hash_from_source(seed, idx):
    """asr_hash32 evaluated from the text of csrc/common.h: the folding line and the xor-shift / multiply rounds as written there."""
    src = open(os.path.join(CSRC, "common.h")).read()
    body = src[src.index("uint32_t asr_hash32("):]
    body = body[:body.index("return x;")]
    m = re.search(r"x = \(uint32_t\)idx \* (0x\w+)u \+ \(uint32_t\)\(idx >> 32\) \* (0x\w+)u \+ \(uint32_t\)seed \+ \(uint32_t\)\(seed >> 32\) \* (0x\w+)u;",
                  body)
    a, b, c = (int(v, 16) for v in m.groups())
    u = 0xFFFFFFFF
    x = ((idx & u) * a + (idx >> 32) * b + (seed & u) + (seed >> 32) * c) & u
    rounds = re.findall(r"x \^= x >> (\d+);|x \*= (0x\w+)u;", body[m.end():])
    assert len(rounds) == 5
    for sh, mul in rounds:
        x = (x ^ (x >> int(sh))) if sh else (x * int(mul, 16)) & u
    return x


def test_keep_mask_is_asr_keep_at_the_lm_index_convention():
    """keep_mask restates asr_keep(seed, m * C + c, thr); lstm_step_train uses (row0 + m) * H + u, lm_dropout m * C + c."""
    train = open(os.path.join(CSRC, "lm_train.hip")).read()
    assert "asr_keep(seed, (uint64_t)m * C + c, thr)" in train
    assert "asr_keep(p.seed, (uint64_t)(p.row0 + m) * p.H + u, p.thr)" in train
    assert "return asr_hash32(seed, idx) >= thr;" in open(os.path.join(CSRC, "common.h")).read()
    seed, p = 0x123456789ABCDEF, 0.3
    thr = RW.drop_threshold(p)[0]
    assert thr == int(float(np.float32(p)) * 2.0 ** 32)
    for row0, n, H in ((0, 3, 5), (37, 4, 18), (2 ** 31, 2, 66)):
        k = R.keep(seed, row0, n, H, p)
        for m in range(n):
            for u in range(H):
                assert bool(k[m, u]) == (_hash_from_source(seed, (row0 + m) * H + u) >= thr), (row0, m, u)
    assert 0.6 < R.keep(seed, 0, 64, 66, p).float().mean() < 0.8
    assert bool(R.keep(seed, 5, 4, 7, 0.0).all())


# ------------------------------------------------------------------------------------------------ the restatement against autograd
def _unit_major_cols(x, H):
    """(M, 4H) gate-major columns q H + j -> unit-major 4 j + q."""
    return x.reshape(-1, 4, H).transpose(1, 2).reshape(-1, 4 * H)


def test_restatement_chained_reproduces_autograd_through_nn_lstm():
    from test_gpu_lm_train import _Ref
    E, H, V = 5, 6, 11
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64) * 0.5
    sd = {"encoder.weight": r(V, E), "rnn.weight_ih_l0": r(4 * H, E), "rnn.weight_hh_l0": r(4 * H, H), "rnn.bias_ih_l0": r(4 * H),
          "rnn.bias_hh_l0": r(4 * H), "decoder.weight": r(V, H), "decoder.bias": r(V)}
    seqs = [[3, 7, 1, 9, 0], [2, 2, 0], [10, 0]]                       # 4, 2 and 1 predicted tokens, sorted longest first
    ref = _Ref(sd, E, H, 1, False, F64)
    loss = ref.loss(seqs)
    loss.backward()
    lens = [len(s) - 1 for s in seqs]
    off, n_t = R.packing(lens)
    assert (off, n_t) == ([0, 3, 5, 6], [3, 2, 1, 1])
    off, n_t, M, T = off + [7], n_t + [0], 7, 4
    tgt = torch.tensor([seqs[s][t + 1] for t in range(T) for s in range(n_t[t])]).int()
    # the kernels' layouts: unit-major gates, operands zero-padded to 16 floats
    xproj = _unit_major_cols(ref.xproj.detach(), H)
    whh = torch.zeros(4 * H, R.pad16(H), dtype=F64)
    whh[:, :H] = sd["rnn.weight_hh_l0"].reshape(4, H, H).transpose(0, 1).reshape(4 * H, H)
    G = R.pad16(4 * H)
    whh_t = torch.zeros(H, G, dtype=F64)
    whh_t[:, :4 * H] = whh[:, :H].t()
    h, c, gates = torch.zeros(M, R.pad16(H), dtype=F64), torch.full((M, H), R.NAN, dtype=F64), torch.zeros(M, G, dtype=F64)
    for t in range(T):
        a, pa, n, nn = off[t], off[t - 1] if t else 0, n_t[t], n_t[t + 1]
        o = R.lstm_step_train(xproj[a:], h[pa:] if t else None, whh, c[pa:] if t else None, n, nn, H, a, 0.0, 1)
        assert torch.equal(o["h_drop"], o["h"]) and torch.equal(o["h_next"], o["h"][:nn])
        h[a:a + n, :H], c[a:a + n], gates[a:a + n, :4 * H] = o["h"], o["c"], o["gates"]
    dec_w = torch.zeros(V, R.pad16(H), dtype=F64)
    dec_w[:, :H] = sd["decoder.weight"]
    part, tl = R.nll_partials(h, dec_w, sd["decoder.bias"], tgt, M, V, H)
    lse, mean = R.train_loss(part, tl, M)
    assert abs(float(mean) - loss.item()) <= 1e-12 * abs(loss.item())
    tok, sums = R.nll_finish(part, tl, off, lens)
    assert abs(float(sums.sum()) - loss.item() * M) <= 1e-12 * loss.item() * M
    dl = R.dlogits(h, dec_w, sd["decoder.bias"], lse, M, V, H, 1.0 / M)
    assert dl.shape == (M, 64) and not dl[:, V:].any()
    dh = R.sub_rows(dl[:, :V] @ dec_w[:, :H], dec_w, tgt, M, H, 1.0 / M)
    dc = torch.full((n_t[0], H), R.NAN, dtype=F64)                     # the trainer hands in torch.empty: never read before written
    for t in range(T - 1, -1, -1):
        a, n, nn = off[t], n_t[t], n_t[t + 1]
        dG, dcn = R.bptt_step(dh[a:], gates[off[t + 1]:] if nn else None, whh_t, gates[a:], c[a:], c[off[t - 1]:] if t else None, dc, n,
                              nn, H)
        gates[a:a + n, :4 * H], dc[:n] = dG, dcn
    want = _unit_major_cols(ref.xproj.grad, H)
    err = float((gates[:, :4 * H] - want).abs().max()) / float(want.abs().max())
    print("\ndG of the chained restatement against autograd: relative error %.3e" % err)
    assert err <= 1e-12
    assert not gates[:, 4 * H:].any()


# ------------------------------------------------------------------------------------------------ the exact cases
def _exact_cases():
    """(name, f(dtype) -> dict of tensors, degenerate by definition) for every exact case of tests/test_gpu_lm_arms.py."""
    out = []
    for k in R.PROJ_CASES:
        c = R.proj_case(*k)
        out.append(("proj %s" % (k,), lambda dt, c=c: dict(out=R.proj(c["x"], c["w"], c["bias"], c["M"], c["N"], c["K"], c["ids"], dt)), False))
    for k in R.BPTT_EXACT:
        for cp in (False, True):
            c = R.bptt_case(*k, True)
            out.append(("bptt %s c_prev %d" % (k, cp), lambda dt, c=c, cp=cp: R.bptt_ref(c, cp, dt), False))
    for k in R.SUB_CASES:
        c = R.sub_case(*k)
        out.append(("sub_rows %s" % (k,), lambda dt, c=c: dict(dh=R.sub_rows(c["dh"], c["w"], c["tgt"], c["M"], c["C"], c["inv_n"], dt)), False))
    for M in R.COLSUM_M:
        for N in R.COLSUM_N:
            for acc in (False, True):
                c = R.colsum_case(M, N)
                out.append(("colsum %d %d acc %d" % (M, N, acc),
                            lambda dt, c=c, acc=acc: dict(out=R.colsum(c["x"], c["M"], c["N"], c["out"], acc, dt)[0]), M == 0 and not acc))
    for nseg in R.EMB_NSEG:
        for E in R.EMB_E:
            for sl in R.EMB_LEN:
                c = R.emb_case(nseg, E, sl)
                out.append(("emb_grad %d %d %d" % (nseg, E, sl), lambda dt, c=c: dict(
                    demb=R.emb_grad(c["dx"], c["rows"], c["seg_off"], c["seg_word"], c["nseg"], c["E"], c["scale"], c["demb"], dt)), False))
    for n in R.SUMSQ_N:
        out.append(("sumsq %d" % n, lambda dt, n=n: dict(out=R.sumsq(R.sumsq_case(n), dt).reshape(1)), n == 0))
    for C in R.DROP_C:
        for p in R.DROP_P:
            for ids in (False, True):
                c = R.drop_case(C, ids)
                out.append(("dropout %d %.1f ids %d" % (C, p, ids),
                            lambda dt, c=c, p=p: dict(out=R.dropout(c["x"], c["M"], c["C"], p, c["seed"], c["ids"], dt)), False))
    return out


def test_exact_cases_are_exact_in_fp32_and_not_degenerate():
    """The empty sums (colsum over no rows, sumsq of no elements) are zero by definition: the only cases let off the non-zero rule."""
    low = (2.0, "")
    for name, f, empty in _exact_cases():
        a, b = f(F64), f(F32)
        vals = torch.cat([v.reshape(-1) for v in a.values()])
        for k in a:
            assert b[k].dtype == F32 and torch.equal(b[k].double(), a[k]), (name, k)
        assert bool(torch.isfinite(vals).all()), name
        if not empty:
            frac = float((vals != 0).double().mean())
            low = min(low, (frac, name))
            assert frac >= 0.2, (name, frac)
    print("\nsmallest share of non-zero entries: %.3f (%s)" % low)
    for k in R.BPTT_EXACT:                                   # the gate gradients alone, and the rows that end at this step
        a = R.bptt_ref(R.bptt_case(*k, True), True)
        assert float((a["dG"] != 0).double().mean()) >= 0.2, k
        if k[2] < k[1]:
            assert bool((a["dG"][k[2]:] != 0).any()) and bool(torch.isfinite(a["dc"][k[2]:]).all())


# ------------------------------------------------------------------------------------------------ planted defects
def _worst(bad, c64, c32):
    return max(R.ratios(bad, c64, c32).values())


def _unequal(bad, clean):
    return any(bad[k].shape != clean[k].shape or not torch.equal(bad[k], clean[k]) for k in clean)


def test_planted_defects_are_caught():
    seen = {}
    # gate order i g f o: the bounded step case
    c = R.step_case(6, 17)
    c64, c32 = R.step_ref(c, True, F64), R.step_ref(c, True, F32)
    seen["gate order i g f o"] = _worst(R.step_ref(c, True, F64, order=(0, 2, 1, 3)), c64, c32)
    # c_prev used at t = 0
    c64, c32 = R.step_ref(c, False, F64), R.step_ref(c, False, F32)
    seen["c_prev used at t = 0"] = _worst(R.step_ref(c, False, F64, cprev_at_t0=c["c_prev"]), c64, c32)
    # BPTT: rows >= n_next
    for k in [x for x in R.BPTT_EXACT if 0 < x[2] < x[1]]:
        for poison in (R.NAN, 0.125):
            c = R.bptt_case(*k, True, poison)
            clean = R.bptt_ref(c, True)
            seen["recurrent term for rows >= n_next %s %s" % (k, poison)] = _unequal(R.bptt_ref(c, True, rec_all=True), clean)
            seen["carried dc for rows >= n_next %s %s" % (k, poison)] = _unequal(R.bptt_ref(c, True, dc_all=True), clean)
    c = R.bptt_case(66, 64, 0, True, 0.125)
    seen["carried dc for rows >= n_next (n_next 0)"] = _unequal(R.bptt_ref(c, True, dc_all=True), R.bptt_ref(c, True))
    # lstm_step_train's side outputs: what the buffers hold afterwards
    c = R.step_case(18, 17)
    tr = dict(n_next=5, row0=37, p=0.3, seed=99)
    clean = R.step_ref(c, True, F64, train=tr)
    bad = R.step_ref(c, True, F64, train=tr, local_index=True)
    seen["dropout index from the local row"] = not torch.equal(bad["h_drop"] == 0, clean["h_drop"] == 0)
    bad = R.step_ref(c, True, F64, train=tr, hnext_rows=17)
    seen["h_next written for all n rows"] = not torch.equal(R.in_buffer(bad["h_next"], 17), R.in_buffer(clean["h_next"], 17))
    # the output layer
    c = R.nll_case(65, 63)
    c64, c32 = R.nll_ref(c, F64), R.nll_ref(c, F32)
    seen["target logit one column off"] = _worst(R.nll_ref(c, F64, tgt_shift=1), c64, c32)
    c = R.nll_case(1025, 300)
    c64, c32 = R.nll_ref(c, F64), R.nll_ref(c, F32)
    seen["one 256-word chunk dropped"] = max(_worst(R.nll_ref(c, F64, drop_chunk=k), c64, c32) for k in range(5))
    assert all(_worst(R.nll_ref(c, F64, drop_chunk=k), c64, c32) > 1 for k in range(5))
    # the fixed-order reductions (exact cases)
    c = R.colsum_case(5, 65)
    clean = R.colsum(c["x"], 5, 65, c["out"], True)
    seen["last row group skipped in colsum"] = not torch.equal(R.colsum(c["x"], 5, 65, c["out"], True, skip_last_group=True)[0], clean[0])
    seen["out2 left stale"] = not torch.equal(R.colsum(c["x"], 5, 65, c["out"], True, out2=torch.full((65,), R.SENT))[1], clean[1])
    for k in [(n, 65, sl) for n in (4, 5) for sl in R.EMB_LEN]:
        c = R.emb_case(*k)
        args = (c["dx"], c["rows"], c["seg_off"], c["seg_word"], c["nseg"], c["E"], c["scale"], c["demb"])
        for sh in (1, -1):
            seen["seg_off off by %d %s" % (sh, k)] = not torch.equal(R.emb_grad(*args, seg_shift=sh), R.emb_grad(*args))
    print()
    for k, v in seen.items():
        print("  %-60s %s" % (k, v if isinstance(v, bool) else "excess %.3g" % v))
    assert all((v is True) if isinstance(v, bool) else v > 1 for v in seen.values()), seen
