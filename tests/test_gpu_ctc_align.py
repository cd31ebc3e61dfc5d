"""asr_ctc_align (csrc/ctc_align.hip) against tests/ctc_align_reference.py (pinned by tests/test_ctc_align_host.py), then the model and
test.py levels on the tiny model of tests/test_gpu_joint_ctc.py.

path / start / end: torch.equal against the float32 restatement, which is the kernel's recursion literally (fp32 adds and comparisons
only).  score / lab_score: within 2e-5 * max(1, |ref|) of the float64 restatement, -inf patterns identical, no NaN -- the project's bound
for the CTC lattice (tests/test_gpu_ctc.py, tests/test_gpu_ctc_prefix.py); the float32 recursion itself stays within 3e-7 of float64 on
these inputs and walks the same path (test_both_precisions_agree_on_the_gpu_cases)."""
import json
import math

import numpy as np
import pytest
import torch

import ctc_align_reference as R

pytestmark = pytest.mark.gpu

TOL = 2e-5
_cache = {}


def _case(name):
    """The case's inputs and both references, computed once."""
    if not _cache:
        _cache["cases"] = R.cases()
    if name not in _cache:
        c = _cache["cases"][name]
        _cache[name] = (c, R.align(dtype=np.float32, **c), R.align(dtype=np.float64, **c))
    return _cache[name]


def _close(got, ref, what):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), what
    inf_g, inf_r = np.isneginf(got), np.isneginf(ref)
    assert np.array_equal(inf_g, inf_r), (what, inf_g.tolist(), inf_r.tolist())
    assert np.isfinite(got[~inf_r]).all(), what
    err = np.abs(got[~inf_r] - ref[~inf_r]) / np.maximum(1.0, np.abs(ref[~inf_r]))
    worst = float(err.max()) if err.size else 0.0
    print("%s: worst relative error %.3e over %d finite values, %d -inf" % (what, worst, err.size, int(inf_r.sum())))
    assert worst <= TOL, (what, worst)


def _run(c, ld_pad=0):
    from asr_hip import ops
    dev = torch.device("cuda")
    lg = torch.from_numpy(c["logits"])
    if ld_pad:                                       # a row stride above V: the logits as a view of a wider buffer that holds 50.0
        wide = torch.full(lg.shape[:2] + (lg.shape[2] + ld_pad,), 50.0)
        wide[..., :lg.shape[2]] = lg
        g = wide.to(dev)[..., :lg.shape[2]]
    else:
        g = lg.to(dev)
    out = ops.ctc_align(g, torch.from_numpy(np.ascontiguousarray(c["targets"])).to(dev),
                        torch.tensor(c["input_lengths"], dtype=torch.int32, device=dev),
                        torch.tensor(c["target_lengths"], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check(name, ld_pad=0):
    c, ref32, ref64 = _case(name)
    got = _run(c, ld_pad)
    for k in ("path", "start", "end"):
        assert got[k].dtype == torch.int32 and torch.equal(got[k], torch.from_numpy(ref32[k])), (name, k)
    _close(got["score"].numpy(), ref64["score"], name + " score")
    _close(got["lab_score"].numpy(), ref64["lab_score"], name + " lab_score")
    return c, got, ref64


def _workspace_beyond_lse(c):
    from asr_hip import lib as L
    B, T, _ = c["logits"].shape
    return L.load().asr_ctc_align_workspace(B, T, c["targets"].shape[1]) - B * T


@pytest.mark.parametrize("name", ["small", "small_integer"])
def test_ragged_batch_with_a_strided_view(name):
    """B 3, T 12, V 7, T_b = [12, 5, 1], L = [4, 2, 1], a repeated pair in row 0; row stride V + 3 with 50.0 in the padding, NaN in the
    frames >= T_b, V + 5 in the targets >= L_b.  With small-integer logits nearly every comparison is a tie: the tie rule on the device."""
    c, got, _ = _check(name, ld_pad=3)
    assert (got["path"][1, 5:] == -1).all() and (got["path"][2, 1:] == -1).all() and got["path"][2, 0].item() == 1
    assert (got["start"][1, 2:] == -1).all() and (got["lab_score"][2, 1:] == 0).all()


def test_more_states_than_threads():
    """T 300, V 32, L 140 with every second label a repeat: S = 281 > 256, a thread owns two states."""
    c, got, _ = _check("two_states_per_thread")
    assert R.collapse(got["path"][0].tolist(), c["targets"][0]) == c["targets"][0].tolist()


def test_benchmark_vocabulary():
    """T 100, V 4364, L 30, B 2 with ragged frames and targets."""
    _check("benchmark_vocabulary")


def test_largest_project_shape_keeps_its_back_pointers_in_lds():
    """T 625, V 64, L 300 (S = 601), the largest lattice the project's limits allow: 141 KB of LDS, above the 64 KB a kernel gets without
    asking, and no back-pointer workspace."""
    c, got, _ = _check("largest_project_shape")
    assert _workspace_beyond_lse(c) == 0
    assert R.collapse(got["path"][0].tolist(), c["targets"][0]) == c["targets"][0].tolist()


def test_back_pointers_in_the_workspace():
    """T 1100, L 300: 69 chunks of 601 back-pointer words exceed the LDS of a CU, so they go through the caller's workspace.  B 2, the second
    utterance shorter in frames and labels (its chunks end earlier than the batch's)."""
    c, got, _ = _check("back_pointers_in_the_workspace")
    assert _workspace_beyond_lse(c) == 2 * 69 * 601
    for b in range(2):
        Tb, Lb = c["input_lengths"][b], c["target_lengths"][b]
        assert R.collapse(got["path"][b, :Tb].tolist(), c["targets"][b]) == c["targets"][b, :Lb].tolist()


def test_edge_batch():
    """L_b = 0; T_b = 0 with L 0 and with L 1; "3 3" in T_b = 2; L 3 in T_b = 2; a blank id and an id = V inside the length; and a plain row
    behind them.  The infeasible rows are -inf / -1 / 0 and leave the others untouched."""
    c, got, ref64 = _check("edges")
    assert np.isfinite(got["score"].numpy()).tolist() == [True, True, False, False, False, False, False, True]
    assert got["path"][0].tolist() == [0] * 6 and got["score"][1].item() == 0.0 and (got["path"][1] == -1).all()
    assert (got["path"][2:7] == -1).all() and (got["start"][2:7] == -1).all() and (got["end"][2:7] == -1).all()
    assert (got["lab_score"][2:7] == 0).all()
    blank_lp = (c["logits"][0, :, 0].astype(np.float64) - R.lse_rows(c["logits"][0])).sum()
    assert abs(got["score"][0].item() - blank_lp) <= TOL * max(1.0, abs(blank_lp))


def test_arguments_are_checked():
    from asr_hip import lib as L, ops
    dev = torch.device("cuda")
    lg = torch.zeros(1, 4, 6, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(AssertionError):
        ops.ctc_align(lg, torch.zeros(1, 0, dtype=torch.int64, device=dev), one, one)
    with pytest.raises(AssertionError):
        ops.ctc_align(lg.bfloat16(), torch.zeros(1, 1, dtype=torch.int64, device=dev), one, one)
    with pytest.raises(L.AsrHipError):
        ops.ctc_align(lg, torch.full((1, 1), 3, dtype=torch.int64, device=dev), one, one, blank=6)
    assert L.load().asr_ctc_align_workspace(0, 4, 1) == 0 and L.load().asr_ctc_align_workspace(2, 4, 1) == 8


# ------------------------------------------------------------------------------------------------ model and test.py level
CHARS = "abcdefgh "                      # + PAD, SOS, EOS: V = 12
TINY = ("--num-layers 2 --num-heads 2 --dim-model 64 --dim-key 32 --dim-value 32 --dim-inner 128 --dim-emb 64 --tgt-max-len 32 "
        "--src-max-len 400 --dropout 0 --label-smoothing 0.1 --cuda").split()


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _model(cli, extra=(), seed=0):
    from utils import constant
    from utils.functions import init_transformer_model
    torch.manual_seed(seed)
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(CHARS)
    l2i = {c: i for i, c in enumerate(chars)}
    return init_transformer_model(cli(TINY + list(extra)), l2i, {i: c for c, i in l2i.items()}).cuda()


def test_model_level_alignment_equals_the_reference_on_its_own_logits(cli):
    """Transformer.ctc_align on the tiny fp32 model with a CTC head, B 3: equal to the restatement run on the model's own ctc_logits
    copied to the host (paths equal, scores within the bound); each label's frames collapse back to the target; start_frame is
    non-decreasing; a model without the head raises."""
    model = _model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).eval()
    g = torch.Generator().manual_seed(1)
    src = torch.randn(3, 1, 161, 160, generator=g).cuda()
    lengths = torch.tensor([160, 120, 90])
    tl = [9, 6, 4]
    tgt = torch.zeros(3, 9, dtype=torch.int64)
    for b, n in enumerate(tl):
        tgt[b, :n] = torch.randint(3, 12, (n,), generator=g)
    with torch.no_grad():
        enc, _ = model.encoder(model._features(src), lengths)
        logits = model.ctc_logits(enc).cpu().numpy()
    frames = model.ctc_frame_lengths(lengths, enc.shape[1])
    assert frames == [40, 30, 22]
    got = model.ctc_align(enc, frames, tgt.cuda(), torch.tensor(tl, dtype=torch.int32))
    ref32 = R.align(logits, tgt.numpy(), frames, tl, dtype=np.float32)
    ref64 = R.align(logits, tgt.numpy(), frames, tl, dtype=np.float64)
    assert len(got) == 3
    for b, a in enumerate(got):
        assert a["frames"] == frames[b] and a["path"] == ref32["path"][b, :frames[b]].tolist()
        assert abs(a["score"] - ref64["score"][b]) <= TOL * max(1.0, abs(ref64["score"][b]))
        assert [x["id"] for x in a["labels"]] == tgt[b, :tl[b]].tolist()
        assert [x["label"] for x in a["labels"]] == [model.id2label[i] for i in tgt[b, :tl[b]].tolist()]
        assert [x["start_frame"] for x in a["labels"]] == ref32["start"][b, :tl[b]].tolist()
        assert [x["end_frame"] for x in a["labels"]] == ref32["end"][b, :tl[b]].tolist()
        for l, x in enumerate(a["labels"]):
            assert abs(x["logp"] - ref64["lab_score"][b, l]) <= TOL * max(1.0, abs(ref64["lab_score"][b, l]))
            assert set(a["path"][x["start_frame"]:x["end_frame"]]) == {2 * l + 1} and x["end_frame"] <= frames[b]
        starts = [x["start_frame"] for x in a["labels"]]
        assert starts == sorted(starts) and R.collapse(a["path"], tgt[b].tolist()) == tgt[b, :tl[b]].tolist()
    lists = model.ctc_align(enc, frames, [tgt[b, :tl[b]].tolist() for b in range(3)])          # id lists instead of a padded tensor
    assert [a["path"] for a in lists] == [a["path"] for a in got]
    plain = _model(cli, ["--precision", "fp32"]).eval()
    with pytest.raises(ValueError, match="CTC head"):
        plain.ctc_align(enc, frames, tgt.cuda(), torch.tensor(tl, dtype=torch.int32))


def _loader():
    """Two utterances as the collate function delivers them: (inputs, targets, percentages, input sizes, target sizes)."""
    g = torch.Generator().manual_seed(3)
    src = torch.randn(2, 1, 161, 120, generator=g)
    src[1, :, :, 90:] = 0
    tgt = torch.tensor([[3, 4, 11, 5, 5, 6], [7, 11, 8, 0, 0, 0]])
    return [(src, tgt, torch.tensor([1.0, 0.75]), torch.tensor([120, 90], dtype=torch.int32), torch.tensor([6, 3], dtype=torch.int32))]


def _monotone_within(rec, duration):
    last = 0.0
    for lab in rec["labels"]:
        assert last - 1e-9 <= lab["start"] < lab["end"] <= duration + 1e-9, (lab, last, duration)
        last = lab["start"]
    for w in rec["words"]:
        assert 0.0 <= w["start"] < w["end"] <= duration + 1e-9 and w["logp"] <= 0.0


def test_test_py_writes_alignments(cli, tmp_path):
    """test.py's evaluate() with --align-out on the tiny model and a two-utterance loader: one parseable line per utterance, times
    monotone and inside the utterance's duration; --align-source hyp under --ctc-greedy aligns exactly the ids ctc_collapse produced,
    which are feasible by construction and which the path collapses back to."""
    import test as test_mod
    from models.asr.transformer import ctc_collapse
    from models.common_layers import PositionalEncoding
    from utils import constant
    model = _model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).eval()
    model.decoder.positional_encoding = PositionalEncoding(model.decoder.dim_model, 301).cuda()
    out = tmp_path / "gold.jsonl"
    cli(TINY + ["--precision", "fp32", "--ctc-weight", "0.3", "--tgt-max-len", "301", "--align-out", str(out)])
    test_mod.evaluate(model, _loader())
    recs = [json.loads(l) for l in out.read_text(encoding="utf-8").splitlines()]
    assert [r["utt"] for r in recs] == [0, 1] and [r["text"] for r in recs] == ["ab ccd", "e f"]
    stride = constant.args.window_stride
    for r, n_in, ids in zip(recs, (120, 90), ([3, 4, 11, 5, 5, 6], [7, 11, 8])):
        assert r["score"] is not None and math.isfinite(r["score"]) and r["score"] < 0
        assert abs(r["score_per_frame"] - r["score"] / (n_in // 4)) <= 1e-9
        assert [l["id"] for l in r["labels"]] == ids and r["text"] == "".join(model.id2label[i] for i in ids)
        assert [w["word"] for w in r["words"]] == r["text"].split()
        _monotone_within(r, n_in * stride)
    # the hypothesis of --ctc-greedy
    out = tmp_path / "hyp.jsonl"
    constant.args.align_out, constant.args.align_source, constant.args.ctc_greedy = str(out), "hyp", True
    seen = {}
    orig = model.ctc_align

    def recording(enc_out, lengths, targets, target_lengths=None):
        res = orig(enc_out, lengths, targets, target_lengths)
        seen["targets"], seen["lengths"], seen["res"] = targets, list(lengths), res
        logits = model.ctc_logits(enc_out)
        seen["argmax"] = logits.argmax(dim=2).cpu().tolist()
        return res
    model.ctc_align = recording
    try:
        test_mod.evaluate(model, _loader())
    finally:
        del model.ctc_align
    recs = [json.loads(l) for l in out.read_text(encoding="utf-8").splitlines()]
    assert len(recs) == 2 and seen["lengths"] == [30, 22]
    for b, r in enumerate(recs):
        want = ctc_collapse(seen["argmax"][b], seen["lengths"][b])
        assert seen["targets"][b] == want and [l["id"] for l in r["labels"]] == want
        if want:
            assert r["score"] is not None and R.collapse(seen["res"][b]["path"], want) == want
        assert r["text"] == "".join(model.id2label[i] for i in want)
        _monotone_within(r, (120, 90)[b] * stride)
    # the plain greedy decoder's ids: SOS / EOS stripped, a PAD inside reported as infeasible, and the run continues
    out = tmp_path / "greedy.jsonl"
    constant.args.align_out, constant.args.ctc_greedy = str(out), False
    test_mod.evaluate(model, _loader())
    recs = [json.loads(l) for l in out.read_text(encoding="utf-8").splitlines()]
    assert len(recs) == 2
    for r in recs:
        assert (r["score"] is None and r["labels"] == [] and r["words"] == []) or math.isfinite(r["score"])
