"""The loss heads that sit on a vocabulary projection (csrc/ce.hip, distill.hip, seq_logprob.hip, mwer.hip, rnnt.hip, rnnt_pruned.hip) bit
for bit against tests/golden/loss_rows.npz, which tools/gen_loss_rows_golden.py recorded on an MI355X with the library of the commit before
csrc/loss_rows.h existed.  The other tests hold these kernels against float64 restatements under tolerances; a refactor of what they share
(the arg-max butterfly, label smoothing, the fixed-order finish, the row log-probability, the gradient-row writer) has to leave the same BITS.

Inputs are seeded on the CPU; only outputs are stored.  Rows (M, V, ld), the smallest at which each shared piece can go wrong:
  (11, 37, 37)    row bases off 16 bytes, a tail of one column per lane, a last workgroup of 3 rows
  (11, 64, 72)    aligned rows behind a stride
  (9, 261, 264)   a second trip of the 256-column loop plus a tail
  (2059, 5, 5)    258 workgroups: the finish kernels' `b += 256` loop runs twice for some threads (forward passes only: its per-row
                  gradients would be most of the fixture and run no code the other three do not)
Logits are scaled so rows are peaked; row 1 has its maximum twice (the lowest index wins); gold has pad_id rows; row 3 is predicted right.
  ce        asr_ce_fwd_partials + asr_ce_finish (lse, argmax, sums, loss; smoothing 0.1 and 0), asr_ce_fwd (the atomic arm: lse and argmax;
            its sums only on the first 8 rows of a shape, one add per slot into zero -- more blocks add in no fixed order), asr_ce_bwd
            (fp32 pad 8 and bf16 pad 64, the whole buffer, smoothing 0 and 0.1, grad_out 0.7), asr_argmax_rows, asr_logsoftmax_topk k 1 / 5
  distill   with_ce true / false, temperature 2, smoothing 0.1, teacher row 3 equal to the student's (KD exactly 0); backward in both forms
  seq       (first and third shape) seg_off [0, 4, 4, 9, M], tgt[1] = -1, the target logit of row 2 -inf, coef (0.7, 1.3, 0, -0.4) -- on the
            third shape, whose last segment is empty too, with its ends swapped, so a negative and the zero coefficient own rows on both; backward in both forms
  rnnt      B 3, T 4, U 3, V 37, T_b (4, 0, 2), U_b (3, 1, 0), the label of utterance 1 the blank (no alignment: +inf, zero rows); the full
            lattice (ld 37) and the band W 2 with a fixed s_begin (ld 40): loss, nll_b, backward in both forms.  `_deadlabel`: the same with
            the second label of utterance 0 the blank, so live rows of an utterance without an alignment are read by the row pass and
            zeroed by the backward.
Float outputs are compared as int32 / int16 views with torch.equal: -inf, 0 and -0 patterns count."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_rows.npz")
ROWS = ((11, 37, 37), (11, 64, 72), (9, 261, 264), (2059, 5, 5))
PAD_ID, TIE_ROW, HIT_ROW, SAME_ROW = 0, 1, 3, 3
GRAD_OUT, TAU, CE_SCALE, KD_SCALE = 0.7, 2.0, 0.6, 0.4
FORMS = (("f32_pad8", torch.float32, 8), ("bf16_pad64", torch.bfloat16, 64))
SEG_HEAD, COEF = (0, 4, 4, 9), (0.7, 1.3, 0.0, -0.4)
RNNT = dict(B=3, T=4, U=3, V=37, W=2, frames=(4, 0, 2), labels=(3, 1, 0), s_begin=((0, 1, 1, 2), (0, 0, 0, 0), (0, 0, 0, 0)))
NAMES = (["ce_%d" % i for i in range(4)] + ["distill_%d_%s" % (i, a) for i in range(4) for a in ("ce", "kd")] + ["seq_0", "seq_2"]
         + ["rnnt_%s%s" % (a, d) for a in ("full", "band") for d in ("", "_deadlabel")])


@functools.lru_cache(maxsize=None)
def rows(i, seed=0):
    """(logits (M,V) view of an (M,ld) buffer, gold (M,)) of row shape i, on the CPU; seed 0 is the student, 1 the teacher."""
    M, V, ld = ROWS[i]
    g = torch.Generator().manual_seed(1000 * seed + i)
    logits = (torch.randn((M, ld), generator=g) * 4.0)[:, :V]
    gold = torch.randint(1, V, (M,), generator=g)
    gold[2] = gold[M - 1] = PAD_ID
    if seed == 0:
        top = float(logits[TIE_ROW].max()) + 1.0
        logits[TIE_ROW, V // 2] = logits[TIE_ROW, V - 2] = top
        gold[HIT_ROW] = int(logits[HIT_ROW].argmax())
    else:
        logits[SAME_ROW] = rows(i)[0][SAME_ROW]
    return logits, gold


def _dev(t):
    return t.cuda() if t.dim() < 2 or t.is_contiguous() else t._base.cuda()[..., :t.shape[-1]]      # a strided view stays one


def _whole(t):
    """The padded buffer behind a gradient that comes back as a view of its first V columns."""
    return (t if t._base is None else t._base).cpu()


def _ce(i):
    from asr_hip import ops
    M, V, _ = ROWS[i]
    logits, gold = (_dev(t) for t in rows(i))
    go = torch.tensor([GRAD_OUT], device="cuda")
    out = {}
    for tag, eps in (("s1", 0.1), ("s0", 0.0)):
        lse, am, sums, loss = ops.ce_fwd_det(logits, gold, eps, PAD_ID)
        out.update({"sums_" + tag: sums, "loss_" + tag: loss})
        if M <= 64:
            for form, dtype, pad in FORMS:
                out["bwd_%s_%s" % (tag, form)] = _whole(ops.ce_bwd(logits, gold, lse, eps, PAD_ID, go, sums[1:2], out_dtype=dtype, pad=pad))
    out["lse"], out["argmax"] = lse, am
    out["lse_atomic"], out["argmax_atomic"], _ = ops.ce_fwd(logits, gold, 0.1, PAD_ID)
    out["sums_atomic8"] = ops.ce_fwd(logits[:8], gold[:8], 0.1, PAD_ID)[2]
    out["argmax_rows"] = ops.argmax_rows(logits)
    if M <= 64:
        for k in (1, 5):
            out["topk%d_vals" % k], out["topk%d_idx" % k] = ops.logsoftmax_topk(logits, k)
    assert int(am[TIE_ROW]) == V // 2 and float(logits[TIE_ROW, V - 2]) == float(logits[TIE_ROW, V // 2]) == float(logits[TIE_ROW].max())
    assert int(am[HIT_ROW]) == int(gold[HIT_ROW]) and int(gold[2]) == PAD_ID and float(sums[1]) < M and float(sums[2]) >= 1
    return out


def _distill(i, with_ce):
    from asr_hip import ops
    M, V, _ = ROWS[i]
    student, gold = (_dev(t) for t in rows(i))
    teacher = _dev(rows(i, 1)[0])
    go = torch.tensor([GRAD_OUT], device="cuda")
    ce_scale = CE_SCALE if with_ce else 0.0
    stats, am, sums, loss = ops.distill_fwd(student, teacher, gold, 0.1, PAD_ID, TAU, ce_scale, KD_SCALE, with_ce=with_ce)
    out = {"sums": sums, "loss": loss}
    if with_ce:
        out["argmax"] = am
    if M <= 64:
        out["row_stats"] = stats
        for form, dtype, pad in FORMS:
            out["bwd_" + form] = _whole(ops.distill_bwd(student, teacher, gold, stats, 0.1, PAD_ID, TAU, ce_scale, KD_SCALE, go, sums[1:2],
                                                        out_dtype=dtype, pad=pad))
    assert torch.equal(student[SAME_ROW], teacher[SAME_ROW]) and int(gold[SAME_ROW]) != PAD_ID
    assert stats[SAME_ROW, 3].view(torch.int32).item() == 0 and float(stats[0, 3]) > 0      # KD exactly +0 on the equal row
    return out


def _seq(i):
    from asr_hip import ops
    M, V, _ = ROWS[i]
    logits, gold = rows(i)
    tgt = gold.clone()
    tgt[1] = -1
    logits = logits._base.clone()[:, :V]                        # a copy with the row stride kept
    logits[2, tgt[2]] = -float("inf")
    logits, tgt = _dev(logits), tgt.cuda()
    seg_off = torch.tensor(SEG_HEAD + (M,), dtype=torch.int32).cuda()
    coef = torch.tensor(COEF if M > SEG_HEAD[3] else COEF[::-1][:1] + COEF[1:3] + COEF[:1]).cuda()      # M = 9: the last segment is empty too
    assert SEG_HEAD[1] == SEG_HEAD[2] and float(coef[2]) == 0 and float(coef[0 if M == SEG_HEAD[3] else 3]) < 0            # the empty segment and the segment whose rows are zero and unread
    fwd = ops.seq_logprob(logits, tgt, seg_off)
    out = {"tok": fwd["tok"], "score": fwd["score"]}
    assert float(fwd["tok"][1]) == float(fwd["tok"][2]) == -float("inf") and float(fwd["score"][1]) == 0.0
    for (form, dtype, pad), go in zip(FORMS, (torch.tensor([GRAD_OUT], device="cuda"), None)):
        out["bwd_" + form] = _whole(ops.seq_logprob_bwd(logits, tgt, seg_off, coef, go, out_dtype=dtype, pad=pad))
    return out


def _rnnt(band, deadlabel):
    from asr_hip import ops
    c = RNNT
    B, T, U, V = c["B"], c["T"], c["U"], c["V"]
    width, ld = (c["W"], 40) if band else (U + 1, 37)
    g = torch.Generator().manual_seed(77 + int(band))
    logits = _dev((torch.randn((B, T, width, ld), generator=g) * 3.0)[..., :V])
    targets = torch.randint(1, V, (B, U), generator=g)
    targets[1, 0] = 0                                            # the blank as a label (utterance 1 has no frame either)
    if deadlabel:
        targets[0, 1] = 0
    targets = targets.cuda()
    fl, tl = (torch.tensor(c[k], dtype=torch.int32).cuda() for k in ("frames", "labels"))
    s = torch.tensor(c["s_begin"], dtype=torch.int32).cuda()
    fwd, bwd = (ops.rnnt_pruned_fwd, ops.rnnt_pruned_bwd) if band else (ops.rnnt_fwd, ops.rnnt_bwd)
    extra = (s, U) if band else ()
    loss, ws = fwd(logits, targets, fl, tl, *extra)
    out = {"loss": loss, "nll": ws[-B:]}
    nll = ws[-B:].tolist()
    assert nll[1] == float("inf") and 0 < nll[2] < float("inf") and (nll[0] == float("inf")) == deadlabel, nll
    for (form, dtype, pad), go in zip(FORMS, (torch.tensor([GRAD_OUT], device="cuda"), None)):
        out["bwd_" + form] = _whole(bwd(logits, targets, fl, tl, *extra, ws, go, out_dtype=dtype, pad=pad))
    rows_b = T * width
    dead = out["bwd_f32_pad8"][rows_b:2 * rows_b]
    assert not dead.any() and out["bwd_f32_pad8"][2 * rows_b].any()
    return out


def compute(name):
    """The current library's outputs of case `name` as CPU tensors."""
    kind, _, rest = name.partition("_")
    if kind == "ce":
        got = _ce(int(rest))
    elif kind == "distill":
        got = _distill(int(rest[0]), rest.endswith("_ce"))
    elif kind == "seq":
        got = _seq(int(rest))
    else:
        got = _rnnt(rest.startswith("band"), rest.endswith("_deadlabel"))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().contiguous() for k, v in got.items()}


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(t.dtype, t.dtype))


@pytest.mark.parametrize("name", NAMES)
def test_the_loss_head_returns_the_recorded_bits(name):
    z = np.load(GOLDEN)
    got = compute(name)
    keys = sorted(k.split("/", 1)[1] for k in z.files if k.startswith(name + "/"))
    assert keys == sorted(got) and keys
    for k in keys:
        want = torch.from_numpy(z[name + "/" + k])              # bf16 is stored as its int16 bits (numpy has no bfloat16)
        have = _bits(got[k])
        assert have.dtype == _bits(want).dtype and have.shape == want.shape, (name, k, got[k].dtype, want.dtype, have.shape, want.shape)
        assert torch.equal(have, _bits(want)), (name, k, int((have != _bits(want)).sum()), "elements differ")
