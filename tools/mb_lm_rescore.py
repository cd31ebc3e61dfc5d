#!/usr/bin/env python3
"""Microbenchmark of LM rescoring (profiles/lm_rescore.txt): a 2-layer 1024-wide LSTM LM, V = 32 000, 1 000 sentences of 5 to 40
words, scored three ways --
  (a) the reference's structure: eager torch (nn.LSTM + Linear + log-softmax / cross entropy), one sentence per call, on the GPU;
  (b) the same batched with torch: one packed nn.LSTM, one (tokens x V) logits tensor, log_softmax, gather;
  (c) asr_hip.lm.LSTMLM.score (csrc/lm.hip);
plus the output-layer kernels alone (TF/s against the 157 TF f32-MFMA peak) and what lm_rescoring=True adds to beam_search on a
32-utterance batch.  Wall-clock: torch.cuda.synchronize() around each measurement, median of `--reps`."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sentences", type=int, default=1000)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--nhid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from asr_hip import ops
    from asr_hip.lm import LSTMLM
    from test_gpu_lm import _random_ckpt
    V, H, L = a.vocab, a.nhid, 2
    ck = _random_ckpt(V, H, H, L, seed=1)
    g = torch.Generator().manual_seed(2)
    words = ck["idx2word"]
    sents = [" ".join(words[int(i)] for i in torch.randint(2, V, (int(n),), generator=g))
             for n in torch.randint(5, 41, (a.sentences,), generator=g)]
    ids = [[ck["word2idx"][w] for w in s.split()] + [0] for s in sents]
    ntok = sum(len(x) - 1 for x in ids)
    print("LM: %d-layer LSTM, ninp = nhid = %d, V = %d; %d sentences of 5..40 words, %d scored tokens" % (L, H, V, a.sentences, ntok))

    # torch model (the reference's RNNModel structure), fp32
    enc = torch.nn.Embedding(V, H).cuda()
    rnn = torch.nn.LSTM(H, H, L).cuda()
    dec = torch.nn.Linear(H, V).cuda()
    sd = ck["model_state_dict"]
    with torch.no_grad():
        enc.weight.copy_(sd["encoder.weight"])
        dec.weight.copy_(sd["decoder.weight"])
        dec.bias.copy_(sd["decoder.bias"])
        rnn.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")})
    crit = torch.nn.CrossEntropyLoss()

    @torch.no_grad()
    def per_sentence():
        out = []
        for x in ids:
            t = torch.tensor(x, device="cuda").unsqueeze(1)
            h0 = torch.zeros(L, 1, H, device="cuda")
            o, _ = rnn(enc(t[:-1]), (h0, h0))
            out.append(len(x[:-1]) * crit(dec(o.view(-1, H)), t[1:].view(-1)))
        return torch.stack(out)

    @torch.no_grad()
    def batched_torch():
        order = sorted(range(len(ids)), key=lambda i: -len(ids[i]))
        seqs = [torch.tensor(ids[i], device="cuda") for i in order]
        packed = torch.nn.utils.rnn.pack_sequence([enc(s[:-1]) for s in seqs])
        o = rnn(packed)[0].data
        tgt = torch.nn.utils.rnn.pack_sequence([s[1:] for s in seqs]).data
        nll = -torch.log_softmax(dec(o), dim=1).gather(1, tgt.unsqueeze(1)).squeeze(1)
        return nll

    lm = LSTMLM(ck)
    per_sentence_ms, ref = timed(per_sentence, 1)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    batched_ms, _ = timed(batched_torch, a.reps)
    torch_peak = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ours_ms, (nll, _) = timed(lambda: lm.score(sents), a.reps)
    ours_peak = torch.cuda.max_memory_allocated() - base
    err = ((nll.double() - ref.double().cpu()).abs() / ref.double().cpu().abs()).max().item()
    print("(a) reference structure, one sentence per call : %10.2f ms" % per_sentence_ms)
    print("(b) torch, batched (full logits)               : %10.2f ms   peak +%.0f MB" % (batched_ms, torch_peak / 2 ** 20))
    print("(c) asr_hip LSTMLM.score (csrc/lm.hip)          : %10.2f ms   peak +%.0f MB   max rel. diff vs (a) %.2e"
          % (ours_ms, ours_peak / 2 ** 20, err))

    # the parts of (c)
    seqs = [x for x in ids]
    fw_ms, f = timed(lambda: lm.forward_packed(seqs), a.reps)
    nll_ms, _ = timed(lambda: ops.lm_nll(f["h"], lm.dec_w, lm.dec_b, f["tgt"], H, f["off"], f["ln"]), a.reps)
    tf = 2.0 * ntok * V * H / (nll_ms * 1e-3) / 1e12
    lstm_tf = 2.0 * ntok * L * 4 * H * 2 * H / (fw_ms * 1e-3) / 1e12
    print("    LSTM layers (proj + %d step launches)        : %10.2f ms   %.1f TF/s" % (L * max(len(x) - 1 for x in ids), fw_ms, lstm_tf))
    print("    output layer (nll_partials + nll_finish)    : %10.2f ms   %.1f TF/s = %.0f%% of 157 TF" % (nll_ms, tf, 100 * tf / 157))

    # what LM rescoring adds to beam_search: dec_tiny's model, its 4 encoder outputs repeated to 32 utterances, beam 4
    from utils import constant
    from utils.functions import init_transformer_model
    from utils.lstm_utils import LM
    z = np.load(os.path.join(ROOT, "tests", "golden", "dec_tiny.npz"))
    chars = constant.PAD_CHAR + constant.SOS_CHAR + constant.EOS_CHAR + "_'abcdefghijklmnopqrstuvwxyz "
    l2i = {c: i for i, c in enumerate(chars)}
    args = constant.parse(str(z["flags"]).split() + ["--precision", "fp32", "--cuda"])
    model = init_transformer_model(args, l2i, {i: c for c, i in l2i.items()})
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")})
    model = model.cuda().eval()
    with torch.no_grad():
        e, _ = model.encoder(model._features(torch.from_numpy(z["src"]).cuda()), torch.from_numpy(z["src_len"]))
    e = e.repeat(8, 1, 1)
    blm = LM.__new__(LM)
    blm.model = lm
    plain_ms, _ = timed(lambda: model.decoder.beam_search(e, beam_width=4, nbest=1, c_weight=0.1), a.reps)
    lm_ms, _ = timed(lambda: model.decoder.beam_search(e, beam_width=4, nbest=1, c_weight=0.1, lm_rescoring=True, lm=blm), a.reps)
    print("beam_search, 32 utterances, beam 4 (dec_tiny model): %.2f ms without LM, %.2f ms with LM rescoring (+%.2f ms, "
          "the 2x1024 / V=32000 LM)" % (plain_ms, lm_ms, lm_ms - plain_ms))


if __name__ == "__main__":
    main()
