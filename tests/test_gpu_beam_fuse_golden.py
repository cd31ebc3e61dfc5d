"""The fused arms of both beam searches (csrc/ctc_beam.hip, csrc/rnnt_beam.hip) bit for bit against tests/golden/beam_fuse.npz, which
tools/gen_beam_fuse_golden.py recorded on an MI355X with the library of the commit before csrc/beam_fuse.h existed.  The other fused
tests hold the arms against float64 restatements under margins and tolerances; a refactor of the arms has to leave the same BITS.

One case per compiled fused arm, inputs seeded on the CPU by the builders of the tests named below:
  transducer  {fp32 J 24, bf16 J 40 (plain projection), bf16 J 32 (MFMA)} x {LM, phrases, both}: V 37, B 3 with T_b = (12, 0, 5) of T 12,
              W 3, K 4, S 3, nbest 3, two predictor labels, n-gram orders 2, 2 and 4 (tests/test_gpu_rnnt_beam_fused.py's build_case at
              the shape of its grid's bf16_j32_w3_k4_s3_o4_both with twice the frames; the seeds are those at which the hypotheses of the
              full utterance run 2 to 22 labels long over the arms, so contexts shift, back off and phrases complete and break off).
              The LM and phrase arms are the same case with the other table dropped.
  CTC         {LM, phrases, both}: tests/ctc_beam_reference.py's small_w4 (B 6, T 24, V 12, T_b = 0 and 1 among the lengths) at W 4, C 8,
              nbest 4; the phrase arm reads the logits through a row stride of V + 5.
ids, lengths, scores, lm and credit are compared with torch.equal, the float ones as int32 views: -inf, 0 and -0 patterns count."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_fuse.npz")
RNNT_SHAPE = (2, 3, 4, 3, 3)                                   # C, W, K, S, nbest
RNNT_T, RNNT_FRAMES = 12, (12, 0, 5)
RNNT_BASE = {"f32_j24": (torch.float32, 24, 2, 2), "bf16_j40": (torch.bfloat16, 40, 2, 0), "bf16_j32": (torch.bfloat16, 32, 4, 3)}
ARMS = ("lm", "ctx", "both")
CTC_CASE, CTC_W, CTC_C, CTC_ORDER, CTC_PAD = "small_w4", 4, 8, 3, {"lm": 0, "ctx": 5, "both": 0}
NAMES = ["rnnt_%s_%s" % (b, a) for b in sorted(RNNT_BASE) for a in ARMS] + ["ctc_%s" % a for a in ARMS]


@functools.lru_cache(maxsize=None)
def _rnnt_base(base):
    import test_gpu_rnnt_beam_fused as G
    dtype, J, order, seed = RNNT_BASE[base]
    return G.build_case(dtype, J, *RNNT_SHAPE, order, True, seed, frames=RNNT_FRAMES, Tn=RNNT_T)


def compute(name):
    """The current library's outputs of case `name` as CPU tensors."""
    kind, _, rest = name.partition("_")
    if kind == "rnnt":
        import test_gpu_rnnt_beam_fused as G
        base, arm = rest.rsplit("_", 1)
        case = _rnnt_base(base)
        lm, graph = case["lm"] if arm != "ctx" else None, case["graph"] if arm != "lm" else None
        got, rc = G.run(dict(case, lm=lm, graph=graph, kw=G.fused_kw(lm, graph)))
        assert rc == 0, (name, rc)
        assert got["lengths"][1].tolist() == [0, -1, -1]       # the zero-length utterance is in the batch
        assert int(got["lengths"][0].min()) >= 2 and int(got["lengths"][0].max()) >= 3, (name, got["lengths"].tolist())      # labels to carry state over
        return got
    import ctc_beam_ctx_reference as X
    import ctc_beam_lm_reference as M
    import ctc_beam_reference as R
    import test_gpu_ctc_beam_ctx as GX
    import test_gpu_ctc_beam_lm as GL
    c = R.cases_cached()[CTC_CASE]
    assert 0 in c["lengths"]
    lm = M.synthetic_lm(c["logits"].shape[2], CTC_ORDER)
    a = (c["logits"], c["lengths"], CTC_W, CTC_C, CTC_W)
    if rest == "lm":
        return GL._run(*a, lm, ld_pad=CTC_PAD[rest])
    return GX._run(*a, X.case_graph(CTC_CASE), X.GAMMA, lm if rest == "both" else None, ld_pad=CTC_PAD[rest])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", NAMES)
def test_the_fused_arm_returns_the_recorded_bits(name):
    z = np.load(GOLDEN)
    got = compute(name)
    keys = sorted(k.split("/", 1)[1] for k in z.files if k.startswith(name + "/"))
    assert keys == sorted(got) and set(keys) >= {"ids", "lengths", "scores", "lm"} and ("credit" in keys) == (not name.endswith("_lm"))
    for k in keys:
        want = torch.from_numpy(z[name + "/" + k])
        assert got[k].dtype == want.dtype and torch.equal(_bits(got[k]), _bits(want)), (name, k, got[k].tolist(), want.tolist())
