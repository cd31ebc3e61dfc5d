"""Training the rescoring LSTM language model on the GPU (csrc/lm_train.hip, asr_hip/lm_train.py, utils/lm_text.py, train_lm.py):
gradients and twenty Adam steps against fp64 torch on the CPU, dropout, bitwise reproducibility, the memory bound of the output
layer's backward, and train_lm.py end to end up to Decoder.beam_search(lm_rescoring=True) with the checkpoint it wrote.

The gradient bound is not a project constant: every case also runs the same torch model in fp32 on the CPU, and a tensor passes when
    e_ours <= 4 * e_torch32 + 1e-6,   e(g) = max|g - g64| / max|g64|
(4: another summation order over up to thousands of tokens; 1e-6: a tensor torch happens to get exactly must not make the bound 0).

The torch model keeps the LSTM bias the way the trainer does: ONE tensor b = bias_ih + bias_hh per layer (bias_hh = 0 and frozen).
Adam is not linear in the gradient, so two tensors that each receive the gradient would move the sum twice as far."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "end2end-asr-pytorch_amd")


def _key(s):
    return (-len(s), list(s))


def _seqs(N, V, max_len, seed, ones=2):
    """N id lists with 1 .. max_len predicted tokens (`ones` of them with exactly one), ids uniform over V, '<eos>' = 0 last."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max_len + 1, (N,), generator=g).tolist()
    lens[:ones] = [1] * min(ones, N)
    return [torch.randint(0, V, (L,), generator=g).tolist() + [0] for L in lens]


class _Ref:
    """nn.LSTM over pack_sequence + Linear + summed cross entropy / N tokens on the CPU.  The last layer's input projection is
    explicit (xproj = x W_ih^T + b, fed to an nn.LSTM whose weight_ih is the identity), so that xproj.grad is the gradient of the
    pre-activation gates."""

    def __init__(self, sd, E, H, nlayers, tie, dtype):
        c = lambda t: t.detach().to(dtype).clone().requires_grad_()
        self.H, self.nlayers, self.tie = H, nlayers, tie
        self.named = {"encoder.weight": c(sd["encoder.weight"])}
        self.lower = []
        for k in range(nlayers - 1):
            m = torch.nn.LSTM(E if k == 0 else H, H, 1).to(dtype)
            with torch.no_grad():
                m.weight_ih_l0.copy_(sd["rnn.weight_ih_l%d" % k])
                m.weight_hh_l0.copy_(sd["rnn.weight_hh_l%d" % k])
                m.bias_ih_l0.copy_(sd["rnn.bias_ih_l%d" % k] + sd["rnn.bias_hh_l%d" % k])
                m.bias_hh_l0.zero_()
            m.bias_hh_l0.requires_grad_(False)
            self.lower.append(m)
            self.named["rnn.weight_ih_l%d" % k], self.named["rnn.weight_hh_l%d" % k] = m.weight_ih_l0, m.weight_hh_l0
            self.named["rnn.bias_ih_l%d" % k] = m.bias_ih_l0
        k = nlayers - 1
        self.named["rnn.weight_ih_l%d" % k] = c(sd["rnn.weight_ih_l%d" % k])
        self.named["rnn.bias_ih_l%d" % k] = c(sd["rnn.bias_ih_l%d" % k] + sd["rnn.bias_hh_l%d" % k])
        top = torch.nn.LSTM(4 * H, H, 1).to(dtype)
        with torch.no_grad():
            top.weight_ih_l0.copy_(torch.eye(4 * H, dtype=dtype))
            top.weight_hh_l0.copy_(sd["rnn.weight_hh_l%d" % k])
            top.bias_ih_l0.zero_()
            top.bias_hh_l0.zero_()
        for q in (top.weight_ih_l0, top.bias_ih_l0, top.bias_hh_l0):
            q.requires_grad_(False)
        self.top = top
        self.named["rnn.weight_hh_l%d" % k] = top.weight_hh_l0
        if not tie:
            self.named["decoder.weight"] = c(sd["decoder.weight"])
        self.named["decoder.bias"] = c(sd["decoder.bias"])

    def params(self):
        return list(self.named.values())

    def loss(self, seqs_sorted):
        from torch.nn.utils.rnn import PackedSequence, pack_sequence
        n = self.named
        pk = pack_sequence([torch.tensor(s[:-1]) for s in seqs_sorted], enforce_sorted=True)
        tgt = pack_sequence([torch.tensor(s[1:]) for s in seqs_sorted], enforce_sorted=True).data
        x = n["encoder.weight"][pk.data]
        for m in self.lower:
            x = m(PackedSequence(x, pk.batch_sizes))[0].data
        k = self.nlayers - 1
        self.xproj = x @ n["rnn.weight_ih_l%d" % k].t() + n["rnn.bias_ih_l%d" % k]
        self.xproj.retain_grad()
        h = self.top(PackedSequence(self.xproj, pk.batch_sizes))[0].data
        w = n["encoder.weight"] if self.tie else n["decoder.weight"]
        logits = h @ w.t() + n["decoder.bias"]
        return torch.nn.functional.cross_entropy(logits, tgt, reduction="sum") / tgt.numel()


def _e(g, g64):
    return (g.double() - g64).abs().max().item() / max(g64.abs().max().item(), 1e-300)


# nlayers, ninp, nhid, V, sentences, longest, tie_weights: n_t crosses 64 and 16 in the 70-sentence cases, 16 in the 20-sentence ones,
# stays below 16 in the 5-sentence one; V = 7 repeats every word id many times; every case has sentences of one predicted token
GRAD_CASES = [(1, 24, 40, 7, 70, 60, False), (2, 96, 200, 257, 70, 60, False), (3, 24, 40, 257, 20, 60, False),
              (2, 300, 650, 10007, 20, 30, False), (1, 512, 1024, 32768, 18, 12, False), (3, 96, 200, 7, 5, 60, False),
              (2, 40, 40, 257, 30, 40, True), (3, 300, 650, 257, 66, 20, False)]


@pytest.mark.parametrize("nlayers,E,H,V,N,T,tie", GRAD_CASES)
def test_gradients_match_fp64_torch(nlayers, E, H, V, N, T, tie):
    from asr_hip.lm_train import LSTMLMTrainer, _gate_major
    tr = LSTMLMTrainer(V, E, H, nlayers, dropout=0.0, tie_weights=tie, seed=H + nlayers)
    with torch.no_grad():                                     # init_weights leaves the decoder bias 0: give it values
        tr.dec_b.copy_(torch.rand(V, generator=torch.Generator().manual_seed(1)) * 0.2 - 0.1)
    sd = tr.state_dict()
    seqs = _seqs(N, V, T, seed=N + V)
    tr.keep_intermediates = True
    loss = tr.forward_backward(seqs).item()
    got = tr.grad_state_dict()
    M = tr.last["b"]["M"]
    dG = _gate_major(tr.last["dG"][:, :4 * H].t().contiguous().cpu(), H).t()          # (M, 4H) gate-major columns
    srt = sorted(seqs, key=_key)
    r64, r32 = _Ref(sd, E, H, nlayers, tie, torch.float64), _Ref(sd, E, H, nlayers, tie, torch.float32)
    l64, l32 = r64.loss(srt), r32.loss(srt)
    l64.backward()
    l32.backward()
    assert r64.xproj.shape == (M, 4 * H)
    print("\ncase %s: tokens %d  loss %.7f  fp64 %.7f  torch fp32 %.7f" % ((nlayers, E, H, V, N, T, tie), M, loss, l64.item(), l32.item()))
    assert abs(loss - l64.item()) <= 1e-4 * abs(l64.item())
    bad, worst = [], 0.0
    rows = [("gates_l%d" % (nlayers - 1), dG, r64.xproj.grad, r32.xproj.grad)]
    rows += [(k, got[k], r64.named[k].grad, r32.named[k].grad) for k in r64.named]
    for name, g, g64, g32 in rows:
        assert g.shape == g64.shape, name
        eo, et = _e(g, g64), _e(g32, g64)
        ratio = eo / (et + 1e-300)
        worst = max(worst, (eo - 1e-6) / (et + 1e-300)) if eo > 1e-6 else worst
        print("  %-22s e_ours %.3e  e_torch32 %.3e  ratio %.2f" % (name, eo, et, ratio))
        if not eo <= 4 * et + 1e-6:
            bad.append((name, eo, et))
    print("  largest (e_ours - 1e-6) / e_torch32: %.2f" % worst)
    assert not bad, bad
    # the folded bias: both checkpoint tensors receive its gradient
    assert torch.equal(got["rnn.bias_ih_l0"], got["rnn.bias_hh_l0"])


def test_twenty_steps_follow_torch():
    from asr_hip.lm_train import LSTMLMTrainer
    V, E, H, nl, lr, clip = 57, 24, 40, 2, 1e-2, 0.25
    tr = LSTMLMTrainer(V, E, H, nl, dropout=0.0, seed=3, lr=lr, clip=clip)
    sd = tr.state_dict()
    batches = [_seqs(24, V, 20, seed=100 + i) for i in range(4)]
    refs = [_Ref(sd, E, H, nl, False, dt) for dt in (torch.float64, torch.float32)]
    opts = [torch.optim.Adam(r.params(), lr=lr, betas=(0.9, 0.999), eps=1e-8) for r in refs]
    ours, l64s, l32s = [], [], []
    for step in range(20):
        b = batches[step % 4]
        ours.append(tr.step(b).item())
        srt = sorted(b, key=_key)
        for r, o, out in zip(refs, opts, (l64s, l32s)):
            o.zero_grad()
            l = r.loss(srt)
            l.backward()
            torch.nn.utils.clip_grad_norm_(r.params(), clip)
            o.step()
            out.append(l.item())
    bad = []
    for i, (a, b64, b32) in enumerate(zip(ours, l64s, l32s)):
        print("step %2d  ours %.7f  fp64 %.7f  torch fp32 %.7f  |ours-64| %.2e  |32-64| %.2e" % (i + 1, a, b64, b32, abs(a - b64), abs(b32 - b64)))
        if not abs(a - b64) <= 4 * abs(b32 - b64) + 1e-6:
            bad.append((i + 1, a, b64, b32))
    assert ours[-1] < ours[0] and l64s[-1] < l64s[0]
    assert not bad, bad


def test_dropout_statistics_masks_and_evaluate():
    from asr_hip.lm import LSTMLM
    from asr_hip.lm_train import LSTMLMTrainer
    V, E, H, nl, p = 101, 48, 64, 2, 0.3
    tr = LSTMLMTrainer(V, E, H, nl, dropout=p, seed=11)
    tr.keep_intermediates = True
    seqs = _seqs(40, V, 30, seed=5)
    masks = []
    for step in range(2):
        tr.step(seqs)
        xs, dx = tr.last["xs"], tr.last["dx"]
        assert len(xs) == nl + 1
        for site, C in enumerate([E] + [H] * nl):
            x, d = xs[site][:, :C], dx[site][:, :C]
            n = x.numel()
            keep = (x != 0).double().mean().item()
            sigma = math.sqrt(p * (1 - p) / n)
            print("step %d site %d: %d elements, kept %.5f (1 - p = %.2f, 4 sigma = %.5f)" % (step, site, n, keep, 1 - p, 4 * sigma))
            assert abs(keep - (1 - p)) <= 4 * sigma
            assert (d[x == 0] == 0).all()                      # the backward regenerates the forward's mask
            assert (d[x != 0] != 0).double().mean().item() > 0.99
        masks.append([(x != 0).clone() for x in xs])
    for a, b in zip(*masks):
        assert not torch.equal(a, b)                           # another step, other masks
    # evaluate: no dropout, the inference kernels -- bitwise LSTMLM.score of the same weights
    ck = tr.checkpoint()
    lm = LSTMLM(ck)
    sents = [" ".join(ck["idx2word"][i] for i in s[:-1]) for s in seqs]
    ref, _ = lm.score(sents)
    got, count = tr.evaluate(seqs, per_sentence=True)
    assert count == sum(len(s) - 1 for s in seqs)
    assert torch.equal(got, ref)
    total, _ = tr.evaluate(seqs)
    assert total == float(ref.double().sum())


def test_training_is_reproducible_and_order_independent():
    from asr_hip.lm_train import LSTMLMTrainer
    V = 307
    batches = [_seqs(70, V, 40, seed=i) for i in range(5)]

    def run(shuffle):
        tr = LSTMLMTrainer(V, 40, 72, 2, dropout=0.2, seed=7, lr=3e-3)
        g = torch.Generator().manual_seed(1)
        losses = []
        for b in batches:
            if shuffle:
                b = [b[i] for i in torch.randperm(len(b), generator=g).tolist()]
            losses.append(tr.step(b))
        return torch.stack(losses), tr.p.clone(), tr.m.clone(), tr.v.clone()
    a, b, c = run(False), run(False), run(True)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.isfinite(a[0]).all()


def test_output_layer_backward_memory_bound():
    """V = 32 768, ~4 000 tokens: the backward's peak stays below HALF of a (tokens, V) fp32 tensor above what was live before it."""
    from asr_hip.lm_train import LSTMLMTrainer
    V = 32768
    tr = LSTMLMTrainer(V, 64, 256, 1, dropout=0.0, seed=1)
    seqs = _seqs(160, V, 50, seed=2)
    ctx = tr._forward(tr._pack(seqs))
    M = ctx["b"]["M"]
    assert 3500 <= M <= 4700, M
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    tr._backward(ctx)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("tokens %d: backward peak %.1f MB above the live set; (tokens, V) fp32 = %.1f MB" % (M, rise / 2 ** 20, M * V * 4 / 2 ** 20))
    assert torch.isfinite(tr.g).all()
    assert rise < 0.5 * M * V * 4, rise


# ------------------------------------------------------------------------------------------------ train_lm.py end to end
WORDS = ["w%02d" % i for i in range(46)] + ["你", "好", "世", "界"]


def _markov_corpus(n, seed):
    """Sentences of a seeded first-order Markov chain over WORDS (CJK characters among them, written without spaces between
    neighbours the way transcripts carry them)."""
    rng = np.random.RandomState(seed)
    W = len(WORDS)
    trans = rng.dirichlet(np.full(W, 0.05), size=W)
    out = []
    for _ in range(n):
        w = rng.randint(W)
        words = [w]
        for _ in range(rng.randint(2, 12)):
            w = rng.choice(W, p=trans[w])
            words.append(w)
        s = WORDS[words[0]]
        for a, b in zip(words, words[1:]):
            s += ("" if len(WORDS[a]) == 1 and len(WORDS[b]) == 1 else " ") + WORDS[b]
        out.append(s)
    return out


def _write_manifest(d, name, sentences):
    lines = []
    for i, s in enumerate(sentences):
        t = d / ("%s_%d.txt" % (name, i))
        t.write_text(s.upper() + "\n", encoding="utf8")                 # the data loader lower-cases
        lines.append("%s_%d.wav,%s" % (name, i, t))
    m = d / (name + ".csv")
    m.write_text("\n".join(lines) + "\n")
    return str(m)


def _run_cli(args, tmp):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(PKG, "train_lm.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("lm")
    corpus = _markov_corpus(720, 1)                           # one chain, split
    train, valid = corpus[:600], corpus[600:]
    common = ["--train-manifest-list", _write_manifest(d, "train", train), "--valid-manifest-list", _write_manifest(d, "valid", valid),
              "--min-count", "1", "--batch-size", "32", "--ninp", "32", "--nhid", "48", "--nlayers", "2", "--dropout", "0.1",
              "--lr", "0.01", "--clip", "0.25", "--seed", "5", "--save-folder", str(d), "--save-every", "1", "--shuffle"]
    log = _run_cli(common + ["--name", "full", "--epochs", "4"], d)
    return dict(dir=d, train=train, valid=valid, common=common, log=log)


def test_train_lm_cli_end_to_end(trained):
    import re
    from utils.lm_text import lm_words
    from utils.lstm_utils import LM
    d = trained["dir"]
    best = str(d / "full" / "best_lm.pt")
    lm = LM(best)
    ck = torch.load(best, map_location="cpu", weights_only=True)
    assert {"word2idx", "idx2word", "ntoken", "ninp", "nhid", "nlayers", "dropout", "tie_weights", "model_state_dict"} <= set(ck)
    assert ck["idx2word"][:2] == ["<eos>", "<oov>"] and "你" in ck["word2idx"]
    # the validation NLL per word through LSTMLM.score == the value the trainer logged for the best epoch
    sents = [" ".join(lm_words(s.lower())) for s in trained["valid"]]
    nll, _ = lm.model.score(sents)
    count = sum(len(s.split()) for s in sents)               # words[1:] + '<eos>' = one prediction per word
    got = float(nll.double().sum()) / count
    logged = [float(x) for x in re.findall(r"valid nll/word ([0-9.eE+-]+)", trained["log"])]
    assert len(logged) == 4 and abs(ck["metrics"]["valid_nll"] - min(logged)) <= 1e-5 * min(logged)
    assert abs(got - ck["metrics"]["valid_nll"]) <= 1e-5 * got, (got, ck["metrics"])
    # below the NLL of the corpus's unigram distribution (training counts, no smoothing)
    cnt = {}
    tw = [lm_words(s.lower()) for s in trained["train"]]
    for ws in tw:
        for w in ws[1:] + ["<eos>"]:
            cnt[w] = cnt.get(w, 0) + 1
    tot = sum(cnt.values())
    pred = [w for s in sents for w in s.split()[1:] + ["<eos>"]]
    uni = -sum(math.log(cnt[w] / tot) for w in pred) / count if all(w in cnt for w in pred) else math.inf
    print("valid nll/word %.4f, unigram %.4f" % (got, uni))
    assert got < uni
    # --continue-from epoch_1.pt reaches the bit-identical epoch_2.pt
    _run_cli(trained["common"] + ["--name", "resumed", "--epochs", "2", "--continue-from", str(d / "full" / "epoch_1.pt")], d)
    a = torch.load(str(d / "full" / "epoch_2.pt"), map_location="cpu", weights_only=True)
    b = torch.load(str(d / "resumed" / "epoch_2.pt"), map_location="cpu", weights_only=True)
    for k in a["model_state_dict"]:
        assert torch.equal(a["model_state_dict"][k], b["model_state_dict"][k]), k
    assert torch.equal(a["optimizer"]["m"], b["optimizer"]["m"]) and torch.equal(a["optimizer"]["v"], b["optimizer"]["v"])
    assert a["optimizer"]["step"] == b["optimizer"]["step"]


def test_beam_search_rescoring_with_a_trained_checkpoint(trained, golden_dir):
    """Decoder.beam_search(lm_rescoring=True): the file train_lm.py wrote and the same weights as an in-memory dictionary agree."""
    from asr_hip.lm import LSTMLM
    from utils.lstm_utils import LM
    from test_gpu_lm import _beam, _dec_tiny
    path = str(trained["dir"] / "full" / "best_lm.pt")
    zl = np.load(os.path.join(golden_dir, "lm_tiny.npz"))
    z, model, enc = _dec_tiny(golden_dir, "fp32")
    from_file = LM(path)
    in_memory = LM.__new__(LM)
    in_memory.model_path = None
    in_memory.model = LSTMLM(torch.load(path, map_location="cpu", weights_only=True))
    in_memory.word2idx, in_memory.idx2word = in_memory.model.word2idx, in_memory.model.idx2word
    a, fa = _beam(model.decoder, enc, from_file, zl)
    b, fb = _beam(model.decoder, enc, in_memory, zl)
    assert a == b and fa == fb and len(a) > 0
