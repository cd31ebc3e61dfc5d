"""Host side of LM training (utils/lm_text.py, train_lm.py, the checkpoint contract of asr_hip/lm_train.py): no GPU."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "end2end-asr-pytorch_amd")


def test_segmentation_mixed_english_cjk_and_double_spaces():
    from utils.lm_text import lm_words
    assert lm_words("hello world") == ["hello", "world"]
    assert lm_words("hello 你好 world") == ["hello", "你", "好", "world"]
    assert lm_words("ab你c d") == ["a", "b", "你", "c", "d"]              # a word with a 'Lo' character: one word per character
    assert lm_words("a  b") == ["a", "b"]
    assert lm_words("a   b    c") == ["a", "b", "c"]
    assert lm_words("  你  好  ") == ["你", "好"]
    assert lm_words(" a 你 好 b  ") == ["a", "你", "好", "b"]
    assert lm_words("") == [] and lm_words("   ") == []


def test_words_equal_lm_word_string_of_the_labels():
    from utils import constant
    from utils.lm_text import lm_words
    from utils.lstm_utils import lm_word_string
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(" abcdefgh'你好世界のは")
    l2i = {c: i for i, c in enumerate(chars)}
    i2l = {i: c for c, i in l2i.items()}
    g = torch.Generator().manual_seed(0)
    pool = list(" abcdefgh'你好世界のは") + [" "] * 6
    texts = ["a  b   c", " 你好 bead", "ab  你 好  cd ", "", "  ", "の は a", "abc你好def gh"]
    for _ in range(300):
        n = int(torch.randint(0, 25, (1,), generator=g))
        texts.append("".join(pool[int(i)] for i in torch.randint(0, len(pool), (n,), generator=g)))
    for t in texts:
        ids = [l2i[constant.SOS_CHAR]] + [l2i[c] for c in t] + [l2i[constant.EOS_CHAR]]
        assert lm_words(t) == lm_word_string(ids, i2l).split(), repr(t)


def test_vocabulary_ties_min_count_cap_and_oov():
    from utils.lm_text import build_vocab, encode
    sents = [["b", "a", "c"], ["a", "b", "d"], ["c", "a", "b"], ["e"]]
    v = build_vocab(sents)                    # a 3, b 3, c 2, d 1, e 1: ties broken by the word
    assert v == ["<eos>", "<oov>", "a", "b", "c", "d", "e"]
    assert build_vocab(sents, min_count=2) == ["<eos>", "<oov>", "a", "b", "c"]
    assert build_vocab(sents, min_count=1, max_vocab=4) == ["<eos>", "<oov>", "a", "b"]
    w2i = {w: i for i, w in enumerate(build_vocab(sents, min_count=2))}
    assert encode(sents, w2i) == [[3, 2, 4, 0], [2, 3, 1, 0], [4, 2, 3, 0], [1, 0]]
    assert encode([[], ["a"]], w2i) == [[2, 0]]


def test_corpus_sources_and_dropped_empty_sentences(tmp_path):
    from utils.lm_text import batches, encode, read_corpus
    t1, t2, t3 = tmp_path / "a.txt", tmp_path / "b.txt", tmp_path / "c.txt"
    t1.write_text("Hello  World\n", encoding="utf8")
    t2.write_text("你好 AB\n", encoding="utf8")
    t3.write_text("\n", encoding="utf8")
    man = tmp_path / "m.csv"
    man.write_text("x.wav,%s\ny.wav,%s\nz.wav,%s\n" % (t1, t2, t3))
    txt = tmp_path / "plain.txt"
    txt.write_text("one two\n\n   \nthree\n", encoding="utf8")
    got = read_corpus([str(man)], [str(txt)])
    assert got == [["hello", "world"], ["你", "好", "ab"], ["one", "two"], ["three"]]
    ids = encode(got, {"<eos>": 0, "<oov>": 1, "one": 2})
    b1 = batches(ids, 2, shuffle=True, seed=3, epoch=1)
    assert b1 == batches(ids, 2, shuffle=True, seed=3, epoch=1)
    assert sorted(map(len, sum(b1, []))) == [2, 3, 3, 4] and all(len(b) <= 2 for b in b1)
    assert [len(s) for b in batches(ids, 2) for s in b] == [2, 3, 3, 4]


def _state_dict_fixture(V, E, H, nl, tie):
    """The shape of LSTMLMTrainer.state_dict(): reference key names, gate-major nn.LSTM layout, bias_hh = 0."""
    g = torch.Generator().manual_seed(1)
    sd = {"encoder.weight": torch.randn(V, E, generator=g)}
    for k in range(nl):
        sd["rnn.weight_ih_l%d" % k] = torch.randn(4 * H, E if k == 0 else H, generator=g)
        sd["rnn.weight_hh_l%d" % k] = torch.randn(4 * H, H, generator=g)
        sd["rnn.bias_ih_l%d" % k] = torch.randn(4 * H, generator=g)
        sd["rnn.bias_hh_l%d" % k] = torch.zeros(4 * H)
    sd["decoder.weight"] = sd["encoder.weight"] if tie else torch.randn(V, H, generator=g)
    sd["decoder.bias"] = torch.randn(V, generator=g)
    return sd


def test_checkpoint_contract(tmp_path):
    for tie, E, H in ((False, 12, 20), (True, 20, 20)):
        V, nl = 9, 2
        words = ["<eos>", "<oov>"] + ["w%d" % i for i in range(V - 2)]
        ck = {"word2idx": {w: i for i, w in enumerate(words)}, "idx2word": words, "ntoken": V, "ninp": E, "nhid": H, "nlayers": nl,
              "dropout": 0.5, "tie_weights": tie, "model_state_dict": _state_dict_fixture(V, E, H, nl, tie),
              "optimizer": {"m": torch.zeros(10), "v": torch.zeros(10), "step": 3, "lr": 1e-3}, "epoch": 1,
              "metrics": {"best_valid_nll": float("inf"), "valid_nll": 4.0, "train_nll": 4.5, "history": [[1, 4.5, 4.0]]},
              "seed": 0, "clip": 0.25}
        path = str(tmp_path / ("lm_%d.pt" % tie))
        torch.save(ck, path)
        back = torch.load(path, map_location="cpu", weights_only=True)
        assert set(back) == set(ck) and back["idx2word"] == words and back["optimizer"]["step"] == 3
        # the reference's RNNModel: encoder = nn.Embedding, rnn = nn.LSTM, decoder = nn.Linear
        model = torch.nn.ModuleDict({"encoder": torch.nn.Embedding(V, E), "rnn": torch.nn.LSTM(E, H, nl, dropout=0.5),
                                     "decoder": torch.nn.Linear(H, V)})
        if tie:
            model["decoder"].weight = model["encoder"].weight
        model.load_state_dict(back["model_state_dict"], strict=True)
        assert torch.equal(model["rnn"].weight_hh_l1, ck["model_state_dict"]["rnn.weight_hh_l1"])


def test_gate_layout_round_trip():
    from asr_hip.lm import _unit_major
    from asr_hip.lm_train import _gate_major
    t = torch.arange(4 * 5 * 3, dtype=torch.float32).reshape(20, 3)
    assert torch.equal(_gate_major(_unit_major(t, 5), 5), t)
    assert torch.equal(_gate_major(_unit_major(t[:, 0], 5), 5), t[:, 0])


def test_train_lm_help_runs_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(PKG, "train_lm.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stderr
    for flag in ("--train-manifest-list", "--valid-manifest-list", "--train-text", "--valid-text", "--min-count", "--max-vocab",
                 "--batch-size", "--shuffle", "--ninp", "--nhid", "--nlayers", "--dropout", "--tie-weights", "--epochs", "--lr", "--clip",
                 "--lr-decay", "--seed", "--save-folder", "--name", "--save-every", "--continue-from"):
        assert flag in r.stdout, flag
