"""The label n-gram LM on the host (utils/ngram.py, train_ngram.py): the Witten-Bell estimate and its query, the
lookup table the device reads, the file, the trainer's command line, and the two new entry points' declarations."""
import json
import math
import re

import numpy as np
import pytest

import ctc_beam_lm_reference as M


def _lm(*a, **k):
    from utils.ngram import NgramLM
    return NgramLM.estimate(*a, **k)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_witten_bell_sums_to_one_after_every_context(order):
    """About 300 random sentences over V 12: after every stored context (every stored n-gram below the highest order) and after 200
    contexts drawn at random (most of them unseen), sum_c exp(q(h, c)) over all V ids is within 1e-5 of 1; every id has a finite unigram."""
    V = 12
    lm = M.synthetic_lm(V, order)
    assert lm.order == order and lm.V == V and len(lm.keys) >= V
    rng = np.random.default_rng(order)
    stored = [[((int(k) >> (16 * j)) & 0xffff) - 1 for j in range(3, -1, -1) if (int(k) >> (16 * j)) & 0xffff] for k in lm.keys]
    ctxs = [()] + [tuple(g) for g in stored if len(g) < order] + [tuple(rng.integers(0, V, size=rng.integers(1, 5))) for _ in range(200)]
    unseen = sum(1 for h in ctxs if h and lm.context(h) and lm.context(h) not in lm._map)
    assert order <= 2 or unseen >= 20
    worst = 0.0
    for h in ctxs:
        lp = [float(lm.logp(h, c)) for c in range(V)]
        assert all(math.isfinite(x) for x in lp), h
        worst = max(worst, abs(sum(math.exp(x) for x in lp) - 1.0))
    print("order %d: %d contexts (%d unseen), worst |sum - 1| %.2e" % (order, len(ctxs), unseen, worst))
    assert worst <= 1e-5
    assert lm.logp((), V) == -np.inf and lm.logp((), -1) == -np.inf          # no id of the table


def test_hand_computed_bigram_example():
    """V 5 (PAD, SOS, EOS, a = 3, b = 4), the sentences "a b", "a a", "b".  Predicted positions: a 3, b 2, EOS 3 times (n = 8, T0 = 3), so
    P(c) = (n(c) + 3/5) / 11.  Bigrams: (SOS,a) 2, (SOS,b) 1, (a,b) 1, (a,a) 1, (a,EOS) 1, (b,EOS) 2: after SOS n 3, T 2; after a n 3, T 3;
    after b n 2, T 1; nothing follows EOS."""
    S, E, a, b = 1, 2, 3, 4
    lm = _lm([[a, b], [a, a], [b]], 5, 2, S, E)
    pa, pb, pe, p0 = 3.6 / 11, 2.6 / 11, 3.6 / 11, 0.6 / 11
    want = {((), a): pa, ((), b): pb, ((), E): pe, ((), 0): p0, ((), S): p0,
            ((S,), a): (2 + 2 * pa) / 5, ((S,), b): (1 + 2 * pb) / 5, ((S,), E): 2 / 5 * pe,
            ((a,), b): (1 + 3 * pb) / 6, ((a,), a): (1 + 3 * pa) / 6, ((a,), E): (1 + 3 * pe) / 6, ((a,), 0): 3 / 6 * p0,
            ((b,), E): (2 + pe) / 3, ((b,), a): 1 / 3 * pa, ((E,), a): pa, ((0,), b): pb, ((b, a), b): (1 + 3 * pb) / 6, ((-1,), a): pa,
            ((a, -1), a): pa}
    for (h, c), p in want.items():
        assert abs(float(lm.logp(h, c)) - math.log(p)) <= 2e-7 * max(1.0, abs(math.log(p))), (h, c)
    assert len(lm.keys) == 5 + 6
    sent = math.log((2 + 2 * pa) / 5) + math.log((1 + 3 * pb) / 6) + math.log((2 + pe) / 3)
    assert abs(lm.score([a, b], S, E) - sent) <= 1e-6
    assert abs(lm.score([a, b], S) - (sent - math.log((2 + pe) / 3))) <= 1e-6 and lm.score([], S, -1) == 0.0
    assert lm.logp((S,), a).dtype == np.float32
    # the float32 adds in the stated order: the backoff weight first, then the lower order's value
    bo_b, lp_a = lm._map[b + 1][1], lm._map[a + 1][0]
    assert lm.logp((b,), a) == np.float32(np.float32(0.0) + bo_b) + lp_a


def test_keys_pack_the_ids_last_symbol_lowest():
    from utils import ngram
    assert ngram.pack([0]) == 1 and ngram.pack([3, 0, 65534]) == (4 << 32) | (1 << 16) | 65535 and ngram.pack([]) == 0
    assert ngram.pack([5, -1, 7]) == 8 and ngram.pack([7, -1]) == 0
    lm = M.synthetic_lm(12, 3)
    assert lm.context([1, 2, 3, 4]) == ngram.pack([3, 4]) and lm.context([4]) == 5 and M.synthetic_lm(12, 1).context([4]) == 0
    assert list(lm.keys) == sorted(lm.keys) and len(set(lm.keys.tolist())) == len(lm.keys)


@pytest.mark.parametrize("order", [1, 3, 4])
def test_hash_table(order):
    """Every stored key is found within max_probe slots and holds its values, absent keys are reported absent, the load is at most 0.5,
    the capacity a power of two, the hash the stated function, and two builds give the same bytes."""
    from utils import ngram
    lm = M.synthetic_lm(12, order)
    keys, vals, max_probe = t = lm.hash_table()
    cap = len(keys)
    assert cap & (cap - 1) == 0 and cap >= 2 * len(lm.keys) and int((keys != 0).sum()) == len(lm.keys) and max_probe >= 1
    assert keys.dtype == np.uint64 and vals.dtype == np.float32 and vals.shape == (cap, 2)
    for k, lp, bo in zip(lm.keys.tolist(), lm.lp, lm.bo):
        s = lm.find(t, k)
        assert s >= 0 and int(keys[s]) == k and vals[s, 0] == lp and vals[s, 1] == bo
        home = (((k ^ (k >> 31)) * 0x9E3779B97F4A7C15) % (1 << 64)) >> 32 & (cap - 1)
        assert home == int(ngram.hash_slot(np.array([k], dtype=np.uint64), cap)[0]) and (s - home) % cap < max_probe
    rng = np.random.default_rng(5)
    absent = [k for k in (ngram.pack(rng.integers(0, 12, size=rng.integers(1, 5))) for _ in range(500)) if k not in lm._map]
    assert len(absent) >= (100 if order < 4 else 50) and all(lm.find(t, k) == -1 for k in absent)
    again = _lm(M.synthetic_corpus(12, 7 + 1200), 12, order, 0, 0).hash_table()
    assert again[0].tobytes() == keys.tobytes() and again[1].tobytes() == vals.tobytes() and again[2] == max_probe


def test_file_round_trip_and_label_checks(tmp_path):
    from utils.ngram import NgramLM
    labels = list("¶§¤abcdefgh ")
    lm = _lm(M.synthetic_corpus(12, 3), 12, 3, 1, 2, labels=labels)
    path = str(tmp_path / "ngram.pt")
    lm.save(path)
    back = NgramLM.load(path, labels)
    assert back.order == 3 and back.V == 12 and back.labels == labels
    for name in ("keys", "lp", "bo"):
        assert getattr(back, name).tobytes() == getattr(lm, name).tobytes()
    assert back.logp((1, 4), 5) == lm.logp((1, 4), 5)
    NgramLM.load(path, {i: c for i, c in enumerate(labels)})                 # a model's id2label dict
    with pytest.raises(ValueError, match="label"):
        NgramLM.load(path, labels[:-1])
    with pytest.raises(ValueError, match="label"):
        NgramLM.load(path, labels[:3] + ["x"] + labels[4:])
    with pytest.raises(ValueError, match="65535"):
        _lm([[3]], 65536, 2, 1, 2)
    with pytest.raises(ValueError, match="65535"):
        NgramLM(2, 65536, ["x"] * 65536, lm.keys, lm.lp, lm.bo)
    _lm([[65534]], 65535, 1, 1, 2, labels=["x"] * 65535)                      # the largest id that fits
    for order in (0, 5):
        with pytest.raises(ValueError, match=r"1\.\.4"):
            _lm([[3]], 12, order, 1, 2)
    with pytest.raises(ValueError, match="outside"):
        _lm([[12]], 12, 2, 1, 2)


def test_train_ngram_on_a_three_line_manifest(tmp_path):
    """train_ngram.py on three transcripts: characters outside the label file are dropped as the loader drops them, the text is lower-
    cased, the file loads against the label file's labels and holds the estimate of those id sequences."""
    import train_ngram
    from train import build_labels
    from utils.ngram import NgramLM
    (tmp_path / "labels.json").write_text(json.dumps(list("ab c")), encoding="utf8")
    lines = []
    for i, text in enumerate(["ab c", "AXb\n", "c a"]):
        (tmp_path / ("t%d.txt" % i)).write_text(text, encoding="utf8")
        lines.append("a%d.wav,%s" % (i, tmp_path / ("t%d.txt" % i)))
    (tmp_path / "m.csv").write_text("\n".join(lines) + "\n")
    (tmp_path / "more.txt").write_text("b b\n", encoding="utf8")
    path = train_ngram.main(["--train-manifest-list", str(tmp_path / "m.csv"), "--train-text", str(tmp_path / "more.txt"), "--labels-path",
                             str(tmp_path / "labels.json"), "--order", "3", "--save-folder", str(tmp_path), "--name", "lm3"])
    assert path == str(tmp_path / "lm3" / "ngram.pt")
    l2i, i2l = build_labels(str(tmp_path / "labels.json"))
    lm = NgramLM.load(path, i2l)
    a, b, sp, c = (l2i[ch] for ch in "ab c")
    want = _lm([[a, b, sp, c], [a, b], [c, sp, a], [b, sp, b]], 7, 3, 1, 2)
    assert lm.order == 3 and lm.V == 7 and lm.keys.tobytes() == want.keys.tobytes() and lm.lp.tobytes() == want.lp.tobytes()
    assert lm.bo.tobytes() == want.bo.tobytes()
    with pytest.raises(SystemExit):
        train_ngram.main(["--labels-path", str(tmp_path / "labels.json"), "--save-folder", str(tmp_path)])


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def test_flags_and_start_up_errors(cli):
    import test as test_mod
    import test_ctc_beam_host as H
    import torch
    a = cli([])
    assert a.ngram_path is None and a.ngram_weight == 0.3 and a.ngram_length_bonus == 0.0
    a = cli(["--ctc-beam-search", "--ngram-path", "x.pt", "--ngram-weight", "0.5", "--ngram-length-bonus", "1.5"])
    assert (a.ngram_path, a.ngram_weight, a.ngram_length_bonus) == ("x.pt", 0.5, 1.5)
    head = H._model(cli, ["--ctc-weight", "0.3"])
    test_mod.check_ctc_decoding(cli(["--ctc-beam-search", "--ngram-path", "x.pt"]), head)
    for extra in ([], ["--beam-search"], ["--ctc-greedy"]):
        with pytest.raises(ValueError, match="--ngram-path needs --ctc-beam-search"):
            test_mod.check_ctc_decoding(cli(["--ngram-path", "x.pt"] + extra), head)
    lm = _lm([[3, 4]], 6, 2, 1, 2, labels=[head.id2label[i] for i in range(6)])
    with pytest.raises(ValueError, match="--ngram-path needs --ctc-beam-search"):
        head.evaluate(torch.zeros(1, 1, 161, 8), [8], torch.zeros(1, 2, dtype=torch.int64), ngram=lm)
    other = _lm([[3, 4]], 6, 2, 1, 2)                                         # labels "0".."5": not this model's
    with pytest.raises(ValueError, match="another label file"):
        head.ctc_beam_search(torch.zeros(1, 2, 32), [2], 4, ngram=other)


def test_header_and_signatures_of_the_new_entry_points():
    """asr_ngram_logp and asr_ctc_beam_search_lm in include/asr_hip.h with the issue's argument lists, ctypes signatures of the same
    length and kinds; the hash is stated in the header as utils/ngram.py computes it."""
    import ctypes
    from asr_hip import lib as L
    src = open(L.HEADER).read()
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "asr_stream_t": ctypes.c_void_p}
    for name, count in (("asr_ngram_logp", 10), ("asr_ctc_beam_search_lm", 26)):
        m = re.search(r"int %s\(([^;]*)\);" % name, src)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(sig) == count
        for a, s in zip(args, sig):
            assert s is (ctypes.c_void_p if "*" in a else kinds[a.split()[0]]), (name, a)
    plain = re.search(r"int asr_ctc_beam_search\(([^;]*)\);", src).group(1).replace("\n", " ").split(",")
    fused = re.search(r"int asr_ctc_beam_search_lm\(([^;]*)\);", src).group(1).replace("\n", " ").split(",")
    assert [a.split()[-1] for a in fused[:len(plain) - 1]] == [a.split()[-1] for a in plain[:-1]]
    assert "0x9E3779B97F4A7C15" in src and ">> 31" in src
