#!/usr/bin/env python3
"""Generate the LM-rescoring fixtures by EXECUTING the reference on CPU (same recipe as oracle/gen_golden.py: stubbed
Levenshtein / torchaudio, argv preset before the first reference import, --cuda off, no bytecode in the reference tree).

TEST INFRASTRUCTURE ONLY: needs the reference tree (ASR_REFERENCE); the tests read only what this writes under tests/golden/.

    python tools/gen_lm_golden.py

writes
  tests/golden/lm_tiny.pt        2-layer LSTM LM, ninp 24 != nhid 40, untied, in the reference's checkpoint format, trained briefly
                                 (fixed seed) on dec_tiny's gold transcripts plus a few Latin / CJK sentences
  tests/golden/lm_tiny_tied.pt   1-layer tied variant (ninp = nhid = 32), trained the same way
  tests/golden/lm_tiny.npz       the reference's LM.evaluate totals / OOV counts, calculate_lm_score triples, and its
                                 beam_search(lm_rescoring=True) 1-best strings, final scores and best-vs-second margins on dec_tiny
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

SENTENCES = [                                   # LM.evaluate cases: single word, OOV, repeated spaces, mixed Latin / CJK
    "dse", "dwfjj xgtbgnwa", "iarx_xicx' hggx'_k", "dse dse", "qqq", "dwfjj  zzz   xgtbgnwa", "你 好", "hello 你 好 world",
    "我 们 dse", "  dse  ", "xgtbgnwa dwfjj hggx'_k iarx_xicx' dse",
]
# "dse" mostly continues: the LM makes the acoustic 1-best "dse" (dec_tiny's beam strings) unlikely as a whole sentence
EXTRA_CORPUS = ["hello world", "你 好 world", "hello 你 好", "dse 我 们", "dse hello world", "dse 你 好", "dse world",
                "dse dse hello", "dse iarx_xicx' hggx'_k"]
LM_WEIGHT, C_WEIGHT = 1.0, 0.1


def make_vocab(gold):
    words = ["<eos>", "<oov>"]
    for s in gold + EXTRA_CORPUS:
        for w in s.split():
            if w not in words:
                words.append(w)
    return words


def train_lm(RNNModel, torch, words, corpus, ninp, nhid, nlayers, tie, seed, steps=300):
    torch.manual_seed(seed)
    w2i = {w: i for i, w in enumerate(words)}
    model = RNNModel("LSTM", ntoken=len(words), ninp=ninp, nhid=nhid, nlayers=nlayers, dropout=0.0, tie_weights=tie)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    seqs = [torch.tensor([w2i[w] for w in s.split()] + [w2i["<eos>"]]) for s in corpus]
    crit = torch.nn.CrossEntropyLoss()
    model.train()
    for _ in range(steps):
        opt.zero_grad()
        loss = 0
        for ids in seqs:
            out, _ = model(ids[:-1].unsqueeze(1), model.init_hidden(1))
            loss = loss + crit(out.view(-1, len(words)), ids[1:])
        loss.backward()
        opt.step()
    print("LM train loss %.4f" % (loss.item() / len(seqs)))
    return {"word2idx": w2i, "idx2word": list(words), "ntoken": len(words), "ninp": ninp, "nhid": nhid, "nlayers": nlayers,
            "dropout": 0.0, "tie_weights": tie, "model_state_dict": model.state_dict()}


def main():
    import numpy as np
    constant = G._boot(G.DEC["flags"])
    import torch
    import models.asr.transformer as T
    from utils import lstm_utils as R
    from utils.functions import init_transformer_model
    _orig = T.get_subsequent_mask
    T.get_subsequent_mask = lambda seq: _orig(seq).bool()

    z = np.load(os.path.join(OUT, "dec_tiny.npz"))
    strip = lambda s: "".join(c for c in s if c not in (constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR))
    gold = [strip(str(s)) for s in z["gold_strs"]]
    words = make_vocab(gold)
    corpus = gold * 2 + EXTRA_CORPUS
    ck = train_lm(R.RNNModel, torch, words, corpus, 24, 40, 2, False, 20261015)
    torch.save(ck, os.path.join(OUT, "lm_tiny.pt"))
    ck_t = train_lm(R.RNNModel, torch, words, corpus, 32, 32, 1, True, 20261016, steps=100)
    torch.save(ck_t, os.path.join(OUT, "lm_tiny_tied.pt"))

    out = {"sentences": np.array(SENTENCES), "lm_weight": np.float64(LM_WEIGHT), "c_weight": np.float64(C_WEIGHT)}
    for tag, name in (("", "lm_tiny.pt"), ("tied_", "lm_tiny_tied.pt")):
        lm = R.LM(os.path.join(OUT, name))
        ev = [lm.evaluate(s) for s in SENTENCES]
        out[tag + "eval_nll"] = np.array([float(a) for a, _ in ev], dtype=np.float64)
        out[tag + "eval_oov"] = np.array([int(b) for _, b in ev], dtype=np.int64)
    lm = R.LM(os.path.join(OUT, "lm_tiny.pt"))

    # calculate_lm_score under a label map with Latin and CJK labels (PAD / SOS / EOS first, as in the product)
    labels = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list("abcdefghijklmnopqrstuvwxyz_' ") + list("你好我们")
    l2i = {c: i for i, c in enumerate(labels)}
    i2l = {i: c for c, i in l2i.items()}
    texts = ["dse", "dwfjj xgtbgnwa", "你好", "hello你好 world", "我们  dse", "  ", "", "dse 你好我们 hello", "x y z"]
    seqs = []
    for t in texts:
        seqs.append([l2i[constant.SOS_CHAR]] + [l2i[c] for c in t] + [l2i[constant.EOS_CHAR]])
    seqs.append([l2i[constant.SOS_CHAR], l2i[constant.PAD_CHAR], l2i[constant.EOS_CHAR]])
    L = max(len(s) for s in seqs)
    trip = [R.calculate_lm_score(torch.tensor([s]), lm, i2l) for s in seqs]
    out["label_chars"] = np.array(labels)
    out["score_seqs"] = np.array([s + [-1] * (L - len(s)) for s in seqs], dtype=np.int64)
    out["score_lm"] = np.array([float(a) for a, _, _ in trip], dtype=np.float64)
    out["score_words"] = np.array([int(b) for _, b, _ in trip], dtype=np.int64)
    out["score_oov"] = np.array([int(c) for _, _, c in trip], dtype=np.int64)

    class Recorder:                             # the word string calculate_lm_score hands to LM.evaluate
        def evaluate(self, seq):
            seen.append(seq)
            return torch.tensor(1.0), 0
    strs = []
    for sq in seqs:
        seen = []
        R.calculate_lm_score(torch.tensor([sq]), Recorder(), i2l)
        strs.append(seen[0] if seen else "")
    out["score_strs"] = np.array(strs)
    out["score_nll"] = np.array([float(lm.evaluate(t)[0]) if t.split() else 0.0 for t in strs], dtype=np.float64)

    # beam search with LM rescoring on dec_tiny's model and inputs; the final sort of each utterance is recorded
    chars = constant.PAD_CHAR + constant.SOS_CHAR + constant.EOS_CHAR + "".join(json.load(open(os.path.join(G.REF, "data/labels/labels.json"))))
    dl2i = {c: i for i, c in enumerate(chars)}
    di2l = {i: c for c, i in dl2i.items()}
    model = init_transformer_model(constant.args, dl2i, di2l)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    model.eval()
    finals = []

    def recording_sorted(seq, key=None, reverse=False):
        seq = list(seq)
        res = sorted(seq, key=key, reverse=reverse)
        if seq and "final_score" in seq[0] and not finals_done[0]:
            finals.append([float(h["final_score"]) for h in res])
            finals_done[0] = True
        return res
    finals_done = [True]
    T.sorted = recording_sorted
    src, src_len, tgt = torch.from_numpy(z["src"]), torch.from_numpy(z["src_len"]), torch.from_numpy(z["tgt"])
    with torch.no_grad():
        enc_in = model.conv(src)
        s = enc_in.size()
        enc, _ = model.encoder(enc_in.view(s[0], s[1] * s[2], s[3]).transpose(1, 2).contiguous(), src_len)
        strs = []
        for b in range(enc.size(0)):
            finals_done[0] = False
            _, hb = model.decoder.beam_search(enc[b:b + 1], beam_width=int(z["beam_width"]), nbest=1, lm_rescoring=True, lm=lm,
                                              lm_weight=LM_WEIGHT, c_weight=C_WEIGHT)
            strs += hb
    del T.sorted
    margins = [f[0] - f[1] if len(f) > 1 else float("inf") for f in finals]
    out["beam_lm"] = np.array(strs)
    out["beam_lm_final"] = np.array([f[0] for f in finals], dtype=np.float64)
    out["beam_lm_margin"] = np.array(margins, dtype=np.float64)
    print("beam (no LM)", [str(x) for x in z["beam"]])
    print("beam (LM)   ", strs, "final", out["beam_lm_final"], "margins", margins)
    assert any(a != str(b) for a, b in zip(strs, z["beam"])), "the LM changes no 1-best: raise LM_WEIGHT"
    assert min(margins) >= 1e-3, margins
    np.savez(os.path.join(OUT, "lm_tiny.npz"), **out)
    print("wrote", os.path.join(OUT, "lm_tiny.npz"))


if __name__ == "__main__":
    main()
