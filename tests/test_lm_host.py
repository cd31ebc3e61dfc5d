"""LM rescoring on the host (no GPU): the reference's word segmentation, the checkpoint loader / weight packing of asr_hip/lm.py
and the scoring algebra, against tests/golden/lm_tiny.npz (tools/gen_lm_golden.py: the reference executed on CPU); plus the ISA
of the MFMA kernels of csrc/lm.hip and csrc/lm_train.hip (f32-input MFMAs, no scratch)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "lm_tiny.npz"))
    labels = [str(c) for c in z["label_chars"]]
    i2l = dict(enumerate(labels))
    seqs = [[int(t) for t in row if t >= 0] for row in z["score_seqs"]]
    return z, i2l, seqs


class _TableLM:
    """Stands in for utils.lstm_utils.LM: NLL totals from the fixture (what the reference's LM.evaluate returned)."""

    def __init__(self, table):
        self.table, self.calls = table, []
        self.model = self

    def score(self, sentences):
        self.calls.append(list(sentences))
        return torch.tensor([self.table[s][0] for s in sentences]), [self.table[s][1] for s in sentences]


def test_word_strings_match_the_reference(golden_dir):
    from utils.lstm_utils import lm_word_string
    z, i2l, seqs = _fixture(golden_dir)
    got = [lm_word_string(s, i2l) for s in seqs]
    assert got == [str(s) for s in z["score_strs"]]
    words = [len(s.split()) + 1 if s.split() else 0 for s in got]
    assert words == [int(w) for w in z["score_words"]]


def test_segmentation_uses_the_lo_category():
    from utils.lstm_utils import get_word_segments_per_language, is_contain_chinese_word
    assert get_word_segments_per_language("ab 你好 我 cd  ef") == ["ab", "你好 我", "cd  ef"]
    assert get_word_segments_per_language("") == [""]
    assert is_contain_chinese_word("x你") and not is_contain_chinese_word("abc")
    assert is_contain_chinese_word("あ")           # hiragana is 'Lo' too (the reference's rule, not utils/metrics.py's range)


def test_lm_score_algebra_and_empty_case(golden_dir):
    from utils.lstm_utils import calculate_lm_score, calculate_lm_scores
    z, i2l, seqs = _fixture(golden_dir)
    strs = [str(s) for s in z["score_strs"]]
    oov = [int(v) for v in z["score_oov"]]
    lm = _TableLM({s: (float(n), o) for s, n, o in zip(strs, z["score_nll"], oov)})
    got = calculate_lm_scores(seqs, lm, i2l)
    assert len(lm.calls) == 1                          # one batched LM call for all hypotheses
    for (a, b, c), s, ref_a, ref_b, ref_c in zip(got, strs, z["score_lm"], z["score_words"], z["score_oov"]):
        assert b == int(ref_b) and c == int(ref_c)
        assert abs(a - float(ref_a)) <= 1e-5 * max(1.0, abs(float(ref_a))), (s, a, float(ref_a))
        if not s.split():
            assert (a, b, c) == (-999, 0, 0)
    one = calculate_lm_score(torch.tensor([seqs[0]]), lm, i2l)
    assert one == got[0]


def _sd(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_loader_shapes_and_gate_interleave(golden_dir):
    from asr_hip.lm import LSTMLM
    ck = _sd(os.path.join(golden_dir, "lm_tiny.pt"))
    lm = LSTMLM(ck, device="cpu")
    V, E, H = ck["ntoken"], ck["ninp"], ck["nhid"]
    assert (ck["nlayers"], E, H, ck["tie_weights"]) == (2, 24, 40, False)
    assert lm.emb.shape == (V, 32) and torch.equal(lm.emb[:, :E], ck["model_state_dict"]["encoder.weight"])
    assert lm.emb[:, E:].abs().sum() == 0
    assert [l["K"] for l in lm.layers] == [E, H]
    assert lm.layers[0]["w_ih"].shape == (4 * H, 32) and lm.layers[1]["w_ih"].shape == (4 * H, 48)
    sd = ck["model_state_dict"]
    for k, layer in enumerate(lm.layers):
        whh, wih = sd["rnn.weight_hh_l%d" % k], sd["rnn.weight_ih_l%d" % k]
        b = sd["rnn.bias_ih_l%d" % k] + sd["rnn.bias_hh_l%d" % k]
        assert layer["w_hh"].shape == (4 * H, 48) and layer["w_hh"][:, H:].abs().sum() == 0
        for j in (0, 7, H - 1):
            for q in range(4):                     # packed row 4 j + q = gate q (i, f, g, o) of unit j
                assert torch.equal(layer["w_hh"][4 * j + q, :H], whh[q * H + j])
                assert torch.equal(layer["w_ih"][4 * j + q, :wih.shape[1]], wih[q * H + j])
                assert layer["bias"][4 * j + q] == b[q * H + j]
    assert lm.dec_w.shape == (V, 48) and torch.equal(lm.dec_w[:, :H], sd["decoder.weight"])


def test_loader_tied_weights(golden_dir):
    from asr_hip.lm import LSTMLM
    ck = _sd(os.path.join(golden_dir, "lm_tiny_tied.pt"))
    assert ck["tie_weights"] and ck["ninp"] == ck["nhid"]
    lm = LSTMLM(ck, device="cpu")
    assert torch.equal(lm.dec_w, lm.emb)
    assert torch.equal(lm.dec_w[:, :ck["nhid"]], ck["model_state_dict"]["encoder.weight"])
    assert lm.ids("dse zzz dse") == ([lm.word2idx["dse"], lm.oov_id, lm.word2idx["dse"], lm.word2idx["<eos>"]], 1)


def test_greedy_refuses_lm_rescoring():
    from models.asr.transformer import Decoder
    with pytest.raises(NotImplementedError, match="beam search only"):
        Decoder.greedy_search.__wrapped__(None, None, lm_rescoring=True)


# ------------------------------------------------------------------------------------------------ ISA of csrc/lm.hip, lm_train.hip
def _asm(tmp_path_factory, name):
    from asr_hip import build
    hipcc = build._hipcc()
    if os.path.isabs(hipcc) and not os.path.exists(hipcc) or not os.path.isabs(hipcc) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path_factory.mktemp("isa")), name + ".s")
    flags = [f for f in build.FLAGS if f != "-fPIC"] + build.PER_FILE_FLAGS.get(name + ".hip", [])
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, name + ".hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read().split("\n")


@pytest.fixture(scope="module")
def lm_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "lm")


@pytest.fixture(scope="module")
def lm_train_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "lm_train")


@pytest.mark.parametrize("kernel", ["lstm_step_kernelILi1E", "lstm_step_kernelILi4E", "lm_nll_partials_kernel", "lm_proj_kernel"])
def test_lm_kernels_use_f32_mfma_and_no_scratch(lm_asm, kernel):
    _f32_mfma_and_no_scratch(lm_asm, kernel)


@pytest.mark.parametrize("kernel", ["lstm_step_train_kernelILi1E", "lstm_step_train_kernelILi4E", "lstm_bptt_step_kernelILi1E",
                                    "lstm_bptt_step_kernelILi4E", "lm_dlogits_kernel"])
def test_lm_train_kernels_use_f32_mfma_and_no_scratch(lm_train_asm, kernel):
    _f32_mfma_and_no_scratch(lm_train_asm, kernel)


def _f32_mfma_and_no_scratch(lm_asm, kernel):
    starts = [i for i, l in enumerate(lm_asm) if re.match(r"^_Z\w+:", l)]
    a = next(i for i in starts if kernel in lm_asm[i])
    body = lm_asm[a:min([i for i in starts if i > a] + [len(lm_asm)])]
    assert any("v_mfma_f32_16x16x4_f32" in l for l in body)
    assert not any(re.search(r"\bscratch_|buffer_store.*off, s\[0:3\]", l) for l in body)
    sym = lm_asm[a].split(":")[0]
    desc = next(i for i, l in enumerate(lm_asm) if l.strip() == ".amdhsa_kernel " + sym)
    fixed = next(l for l in lm_asm[desc:] if ".amdhsa_private_segment_fixed_size" in l)
    assert fixed.split()[-1] == "0"
