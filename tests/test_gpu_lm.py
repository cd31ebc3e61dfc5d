"""LM rescoring on the GPU (csrc/lm.hip via asr_hip/lm.py, utils/lstm_utils.py, Decoder.beam_search(lm_rescoring=True)):
the LSTM chain and the fused output layer against fp64 torch on the CPU, determinism, batch invariance, the memory bound of the
logits-free output layer, and the reference's own LM-rescored decode (tests/golden/lm_tiny.npz, tools/gen_lm_golden.py)."""
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _random_ckpt(V, E, H, nlayers, seed):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s, a=1.0: (torch.rand(*s, generator=g) * 2 - 1) * a
    sd = {"encoder.weight": u(V, E, a=0.5), "decoder.weight": u(V, H, a=0.3), "decoder.bias": u(V, a=0.1)}
    k = H ** -0.5
    for l in range(nlayers):
        sd["rnn.weight_ih_l%d" % l] = u(4 * H, E if l == 0 else H, a=k)
        sd["rnn.weight_hh_l%d" % l] = u(4 * H, H, a=k)
        sd["rnn.bias_ih_l%d" % l] = u(4 * H, a=k)
        sd["rnn.bias_hh_l%d" % l] = u(4 * H, a=k)
    words = ["<eos>", "<oov>"] + ["w%d" % i for i in range(V - 2)]
    return {"word2idx": {w: i for i, w in enumerate(words)}, "idx2word": words, "ntoken": V, "ninp": E, "nhid": H,
            "nlayers": nlayers, "dropout": 0.0, "tie_weights": False, "model_state_dict": sd}


def _random_seqs(N, V, max_len, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max_len + 1, (N,), generator=g).tolist()
    return [torch.randint(0, V, (L + 1,), generator=g).tolist() for L in lens]


def _fp64_reference(ck, seqs_sorted):
    """nn.LSTM in fp64 over pack_sequence (the same time-major packing, longest first) + fp64 log_softmax / gather."""
    sd = {k: v.double() for k, v in ck["model_state_dict"].items()}
    rnn = torch.nn.LSTM(ck["ninp"], ck["nhid"], ck["nlayers"]).double()
    rnn.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")})
    inp = [torch.tensor(s[:-1]) for s in seqs_sorted]
    packed = torch.nn.utils.rnn.pack_sequence([sd["encoder.weight"][i] for i in inp], enforce_sorted=True)
    with torch.no_grad():
        h = rnn(packed)[0].data
        lp = torch.log_softmax(h @ sd["decoder.weight"].t() + sd["decoder.bias"], dim=1)
    tgt = torch.nn.utils.rnn.pack_sequence([torch.tensor(s[1:]) for s in seqs_sorted], enforce_sorted=True).data
    nll_tok = -lp.gather(1, tgt.unsqueeze(1)).squeeze(1)
    sums, a = torch.zeros(len(seqs_sorted), dtype=torch.float64), 0
    for n in packed.batch_sizes.tolist():
        sums[:n] += nll_tok[a:a + n]
        a += n
    return h, sums


# nlayers x nhid over {1, 3} x {40, 200, 650, 1024}, ninp != nhid, N up to 1 500 with lengths 1 .. 60
CASES = [(1, 24, 40, 1, 60, 7), (3, 24, 40, 37, 60, 101), (1, 128, 200, 1500, 60, 1009), (3, 96, 200, 100, 60, 257),
         (1, 300, 650, 200, 40, 10007), (3, 400, 650, 16, 60, 503), (1, 512, 1024, 300, 30, 32768), (3, 512, 1024, 8, 60, 1024)]


@pytest.mark.parametrize("nlayers,E,H,N,T,V", CASES)
def test_lstm_chain_and_nll_match_fp64_torch(nlayers, E, H, N, T, V):
    from asr_hip import ops
    from asr_hip.lm import LSTMLM
    ck = _random_ckpt(V, E, H, nlayers, seed=H + nlayers)
    lm = LSTMLM(ck)
    seqs = _random_seqs(N, V, T, seed=N)
    f = lm.forward_packed(seqs)
    nll = ops.lm_nll(f["h"], lm.dec_w, lm.dec_b, f["tgt"], H, f["off"], f["ln"]).double().cpu()
    h_ref, nll_ref = _fp64_reference(ck, [seqs[i] for i in f["order"]])
    h = f["h"][:, :H].double().cpu()
    assert h.shape == h_ref.shape
    # |h| < 1; the bound is absolute on h and relative on the per-sequence sums
    assert (h - h_ref).abs().max().item() <= 1e-4
    rel = ((nll - nll_ref).abs() / nll_ref.abs().clamp_min(1.0)).max().item()
    assert rel <= 1e-4, rel


@pytest.mark.parametrize("V", [7, 10007, 32768])
def test_nll_kernels_match_log_softmax_and_are_deterministic(V):
    from asr_hip import ops
    g = torch.Generator().manual_seed(V)
    M, H, Hp = 777, 72, 80
    h = torch.zeros(M, Hp)
    h[:, :H] = torch.randn(M, H, generator=g)
    w = torch.zeros(V, Hp)
    w[:, :H] = torch.randn(V, H, generator=g) * 0.5
    b = torch.randn(V, generator=g)
    tgt = torch.randint(0, V, (M,), generator=g)
    lens = [M]                                       # one sequence whose tokens are rows 0 .. M-1 (step_off[t] = t)
    off = torch.arange(M, dtype=torch.int32).cuda()
    ln = torch.tensor(lens, dtype=torch.int32).cuda()
    args = (h.cuda(), w.cuda(), b.cuda(), tgt.to(torch.int32).cuda(), H, off, ln)
    s1, t1 = ops.lm_nll(*args, per_token=True)
    s2, t2 = ops.lm_nll(*args, per_token=True)
    assert torch.equal(s1, s2) and torch.equal(t1, t2)
    lp = torch.log_softmax(h[:, :H].double() @ w[:, :H].double().t() + b.double(), dim=1)
    ref = -lp.gather(1, tgt.unsqueeze(1)).squeeze(1)
    err = ((t1.double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
    assert err <= 1e-5, err
    assert abs(s1.item() - ref.sum().item()) <= 1e-5 * ref.abs().sum().item()


def test_batch_invariance():
    """A sentence's score is bitwise the same alone and inside a batch of 1 000 (and in repeated calls)."""
    from asr_hip.lm import LSTMLM
    V = 5003
    ck = _random_ckpt(V, 96, 256, 2, seed=5)
    lm = LSTMLM(ck)
    words = ck["idx2word"]
    g = torch.Generator().manual_seed(9)
    sents = [" ".join(words[int(i)] for i in torch.randint(2, V, (int(n),), generator=g))
             for n in torch.randint(1, 41, (1000,), generator=g)]
    batch, _ = lm.score(sents)
    again, _ = lm.score(sents)
    assert torch.equal(batch, again)
    for i in (0, 1, 17, 500, 999):
        alone, _ = lm.score([sents[i]])
        assert torch.equal(alone[0], batch[i]), (i, alone[0].item(), batch[i].item())


def test_no_logits_in_memory():
    """N*T = 8 192 tokens, V = 32 768: full fp32 logits would be 1 GiB; the output layer's peak stays under 256 MB."""
    from asr_hip import ops
    M, V, H = 8192, 32768, 256
    g = torch.Generator(device="cuda").manual_seed(1)
    h = torch.randn(M, H, device="cuda", generator=g)
    w = torch.randn(V, H, device="cuda", generator=g) * 0.1
    b = torch.zeros(V, device="cuda")
    tgt = torch.randint(0, V, (M,), device="cuda", generator=g, dtype=torch.int32)
    off = (torch.arange(64, device="cuda", dtype=torch.int32) * 128)       # 128 sequences x 64 tokens, time-major
    ln = torch.full((128,), 64, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    sums = ops.lm_nll(h, w, b, tgt, H, off, ln)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert torch.isfinite(sums).all()
    assert rise < 256 * 2 ** 20, rise


# ------------------------------------------------------------------------------------------------ vs the reference
def test_evaluate_and_lm_score_match_the_reference(golden_dir):
    from utils.lstm_utils import LM, calculate_lm_score
    z = np.load(os.path.join(golden_dir, "lm_tiny.npz"))
    sents = [str(s) for s in z["sentences"]]
    for tag, name in (("", "lm_tiny.pt"), ("tied_", "lm_tiny_tied.pt")):
        lm = LM(os.path.join(golden_dir, name))
        for s, nll, oov in zip(sents, z[tag + "eval_nll"], z[tag + "eval_oov"]):
            got, got_oov = lm.evaluate(s)
            assert got_oov == int(oov) and abs(got - float(nll)) <= 1e-4 * max(1.0, abs(float(nll))), (name, s, got, float(nll))
    lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
    i2l = dict(enumerate(str(c) for c in z["label_chars"]))
    for row, a, b, c in zip(z["score_seqs"], z["score_lm"], z["score_words"], z["score_oov"]):
        got = calculate_lm_score(torch.tensor([[int(t) for t in row if t >= 0]]), lm, i2l)
        assert got[1:] == (int(b), int(c)) and abs(got[0] - float(a)) <= 1e-4 * max(1.0, abs(float(a))), (got, a)


def _dec_tiny(golden_dir, precision):
    from utils import constant
    from utils.functions import init_transformer_model
    z = np.load(os.path.join(golden_dir, "dec_tiny.npz"))
    chars = constant.PAD_CHAR + constant.SOS_CHAR + constant.EOS_CHAR + "_'abcdefghijklmnopqrstuvwxyz "
    l2i = {c: i for i, c in enumerate(chars)}
    args = constant.parse(str(z["flags"]).split() + ["--precision", precision, "--cuda"])
    model = init_transformer_model(args, l2i, {i: c for c, i in l2i.items()})
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}, strict=True)
    model = model.cuda().eval()
    src, src_len = torch.from_numpy(z["src"]).cuda(), torch.from_numpy(z["src_len"])
    with torch.no_grad():
        enc, _ = model.encoder(model._features(src), src_len)
    return z, model, enc


def _beam(dec, enc, lm, zl, use_cache=True, lm_rescoring=True):
    finals = []
    orig = dec._rank_ended

    def rec(ended, *a, **k):
        out = orig(ended, *a, **k)
        finals.extend(max(h["final_score"] for h in hs) for hs in ended)
        return out
    dec._rank_ended = rec
    try:
        _, strs = dec.beam_search(enc, beam_width=4, nbest=1, lm_rescoring=lm_rescoring, lm=lm, lm_weight=float(zl["lm_weight"]),
                                  c_weight=float(zl["c_weight"]), use_cache=use_cache)
    finally:
        del dec._rank_ended
    return strs, finals


def test_lm_rescored_beam_search_matches_the_reference(golden_dir):
    from utils.lstm_utils import LM
    zl = np.load(os.path.join(golden_dir, "lm_tiny.npz"))
    z, model, enc = _dec_tiny(golden_dir, "fp32")
    dec = model.decoder
    lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
    ref = [str(s) for s in zl["beam_lm"]]
    assert ref != [str(s) for s in z["beam"]]                   # the fixture's LM changes at least one 1-best
    strs, finals = _beam(dec, enc, lm, zl)
    assert strs == ref
    assert np.abs(np.array(finals) - zl["beam_lm_final"]).max() <= 1e-4
    assert _beam(dec, enc, lm, zl, use_cache="per_utterance")[0] == ref
    assert _beam(dec, enc, lm, zl, use_cache=False)[0] == ref
    assert _beam(dec, enc, None, zl, lm_rescoring=False)[0] == [str(s) for s in z["beam"]]
    with pytest.raises(NotImplementedError):
        dec.greedy_search(enc, lm_rescoring=True, lm=lm)


def _error_chars(hyps, golds):
    from utils import constant
    from utils.metrics import calculate_cer
    tot = 0
    for h, g in zip(hyps, golds):
        for ch in (constant.EOS_CHAR, constant.SOS_CHAR, constant.PAD_CHAR):
            h, g = h.replace(ch, ""), g.replace(ch, "")
        tot += calculate_cer(h.strip(), g.strip())
    return tot


def test_lm_rescored_beam_search_bf16_cer_close_to_reference(golden_dir):
    """bf16 ASR model, fp32 LM: the CER error count within 3 of the reference's LM-rescored strings' (the bound of
    test_gpu_decode.py::test_decode_bf16_cer_close_to_reference)."""
    from utils.lstm_utils import LM
    zl = np.load(os.path.join(golden_dir, "lm_tiny.npz"))
    z, model, enc = _dec_tiny(golden_dir, "bf16")
    lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
    strs, _ = _beam(model.decoder, enc, lm, zl)
    golds = [str(s) for s in z["gold_strs"]]
    assert abs(_error_chars(strs, golds) - _error_chars([str(s) for s in zl["beam_lm"]], golds)) <= 3, strs


def _corpus(tmp_path, n=6):
    rng = np.random.RandomState(0)
    words = ["ab", "ba", "abba", "bab", "aab", "bba"]
    lines = []
    for i in range(n):
        w = tmp_path / ("u%d.wav" % i)
        with wave.open(str(w), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((rng.randn(4000 + 800 * i) * 2000).astype("<i2").tobytes())
        t = tmp_path / ("u%d.txt" % i)
        t.write_text(words[i % len(words)] + "\n")
        lines.append("%s,%s" % (w, t))
    man = tmp_path / "test.csv"
    man.write_text("\n".join(lines))
    return str(man)


def test_test_py_evaluate_with_lm_rescoring(tmp_path, golden_dir):
    """test.py's evaluate() with --beam-search --lm-rescoring and LM(lm_tiny.pt) (reference test.py:91-97) on a tiny corpus."""
    from utils import constant
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    from utils.functions import init_transformer_model
    from utils.lstm_utils import LM
    import test as test_mod
    man = _corpus(tmp_path)
    lm_path = os.path.join(golden_dir, "lm_tiny.pt")
    constant.parse(["--test-manifest-list", man, "--cuda", "--batch-size", "3", "--num-workers", "0", "--num-layers", "1",
                    "--num-heads", "2", "--dim-model", "32", "--dim-key", "16", "--dim-value", "16", "--dim-inner", "64",
                    "--dim-emb", "32", "--tgt-max-len", "301", "--src-max-len", "64", "--dropout", "0.0", "--beam-search",
                    "--beam-width", "3", "--lm-rescoring", "--lm-path", lm_path, "--lm-weight", "0.5"])
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, " ", "a", "b"]
    l2i = {c: i for i, c in enumerate(chars)}
    torch.manual_seed(3)
    model = init_transformer_model(constant.args, l2i, {i: c for c, i in l2i.items()}).cuda()
    conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window="hamming", noise_dir=None, noise_prob=0.4,
                noise_levels=(0.0, 0.5))
    ds = SpectrogramDataset(conf, [man], l2i, normalize=True)
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    cer, wer = test_mod.evaluate(model, loader, lm=LM(constant.args.lm_path))
    assert np.isfinite(cer) and np.isfinite(wer) and cer >= 0
