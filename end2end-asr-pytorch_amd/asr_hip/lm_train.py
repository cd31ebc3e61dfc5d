"""Training of the rescoring LSTM language model (reference: utils/lstm_utils.py RNNModel / LM) on csrc/lm_train.hip + csrc/lm.hip.

Objective: exactly what LSTMLM.score reports -- per sentence, inputs ids[:-1], targets ids[1:], zero initial state -- as the mean
NLL per predicted token of the batch.  A step is one forward, one backward and one Adam update:

  forward   per layer one asr_lm_proj over every token, then one asr_lstm_step_train per time step on the n_t running rows (keeps the
            activated gates, the cell states and h at the next step's rows); dropout at the reference's three sites (embedding
            output, between layers, last layer's output) from a counter hash, never stored; asr_lm_nll_partials + asr_lm_train_loss.
  backward  the output layer in bounded chunks of tokens (asr_lm_dlogits: softmax / N into a scratch buffer, then the library's fp32
            data- and weight-gradient GEMMs: no (tokens, V) tensor; the "- onehot" half as row operations), then per layer, top down, one asr_lstm_bptt_step per time step from T - 1
            to 0 and the token-parallel dW_hh = dG^T h_prev, dW_ih = dG^T x, db = colsum dG, dx = dG W_ih; the embedding gradient
            over host-sorted token ids.
  update    global-norm clipping (fixed-order sum of squares + asr_clip_coef) passed to asr_adam_step as grad_scale; the padded
            operand copies the kernels read are refreshed from the flat parameters.

Launches per step: 2 * nlayers * T sequential step launches plus O(nlayers + tokens / chunk) token-parallel ones.  Nothing adds with
atomics and the trainer sorts its batch canonically: a run is reproducible to the bit and independent of the order inside a batch.

The flat fp32 buffers (parameters, gradient, Adam m and v) hold the LSTM weights in the kernels' UNIT-MAJOR row order (row 4 j + q =
gate q of unit j) and the folded bias b = bias_ih + bias_hh; state_dict() converts to nn.LSTM's gate-major layout.
"""
import math

import numpy as np
import torch

from . import ops
from .lm import LSTMLM, _pad16, _unit_major

_M64 = (1 << 64) - 1


def _mix64(x):
    """splitmix64's finaliser: the dropout seed of (trainer seed, step, site)."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _gate_major(t, H):
    """Inverse of lm._unit_major."""
    return t.reshape(H, 4, *t.shape[1:]).transpose(0, 1).reshape(4 * H, *t.shape[1:])


def _pad(n, k):
    return (n + k - 1) // k * k


def _gemm_tn(dy, x, dw, N, K):
    """dw += dy[:, :N]^T x[:, :K] on the library's weight-gradient GEMM, in the forms that add in a fixed order: its automatic
    split over the tokens when it comes with a workspace (the slices are folded in index order), one slice otherwise (without a
    workspace the automatic split would meet in fp32 atomics)."""
    L = ops.L
    ws = L.load().asr_gemm_tn_workspace(dy.shape[0], N, K, 0, L.dt(dy))
    ops.gemm_tn(dy, x, dw, N=N, K=K, splits=0 if ws > 0 else 1)


class LSTMLMTrainer:
    def __init__(self, vocab, ninp, nhid, nlayers, dropout=0.0, tie_weights=False, device="cuda", seed=0, lr=1e-3, clip=0.25,
                 betas=(0.9, 0.999), eps=1e-8, state_dict=None):
        """vocab: the number of words, or the list idx2word ('<eos>' and '<oov>' included)."""
        self.idx2word = list(vocab) if not isinstance(vocab, int) else None
        self.ntoken = V = len(self.idx2word) if self.idx2word is not None else int(vocab)
        self.ninp, self.nhid, self.nlayers = E, H, _ = int(ninp), int(nhid), int(nlayers)
        self.dropout, self.tie_weights = float(dropout), bool(tie_weights)
        if self.tie_weights and E != H:
            raise ValueError("tie_weights needs ninp == nhid")
        if not 0.0 <= self.dropout < 1.0 or self.nlayers < 1:
            raise ValueError("dropout in [0, 1), nlayers >= 1")
        self.device = dev = torch.device(device)
        self.seed, self.lr, self.clip, self.betas, self.eps = int(seed), float(lr), float(clip), betas, float(eps)
        self.t = 0                                   # optimiser steps taken
        self.keep_intermediates = False              # tests: keep the last step's activations / gradients in self.last
        self.last = None
        self.marks = None                            # tools/lm_train_rate.py: a list that receives (tag, event) around the time loops
        # ---- flat layout: every segment starts on a 16-byte boundary
        self.seg, off = {}, 0

        def add(name, *shape):
            nonlocal off
            self.seg[name] = (off, shape)
            off += _pad(int(np.prod(shape)), 4)
        add("encoder.weight", V, E)
        for k in range(self.nlayers):
            add("w_ih%d" % k, 4 * H, E if k == 0 else H)
            add("w_hh%d" % k, 4 * H, H)
            add("b%d" % k, 4 * H)
        if not self.tie_weights:
            add("decoder.weight", V, H)
        add("decoder.bias", V)
        self.p, self.g, self.m, self.v = (torch.zeros(off, dtype=torch.float32, device=dev) for _ in range(4))
        self._sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._coef = torch.ones(1, dtype=torch.float32, device=dev)
        # ---- padded operand copies (zeros in the padding, written once)
        z = lambda r, c: torch.zeros((r, c), dtype=torch.float32, device=dev)
        self.emb = z(V, _pad16(E))
        self.dec_w = self.emb if self.tie_weights else z(V, _pad16(H))
        self.layers = []
        for k in range(self.nlayers):
            K = E if k == 0 else H
            self.layers.append(dict(w_ih=z(4 * H, _pad16(K)), w_hh=z(4 * H, _pad16(H)), w_hh_t=z(H, _pad16(4 * H)),
                                    bias=self.view(self.p, "b%d" % k), K=K))
        self.dec_b = self.view(self.p, "decoder.bias")
        self.load_state_dict(state_dict if state_dict is not None else self._init_state_dict())

    # ------------------------------------------------------------------------------------------ parameters
    def view(self, flat, name):
        o, shape = self.seg["encoder.weight" if name == "decoder.weight" and self.tie_weights else name]
        return flat[o:o + int(np.prod(shape))].view(*shape)

    def _init_state_dict(self):
        """RNNModel.init_weights: encoder / decoder weight U(-0.1, 0.1), decoder bias 0; nn.LSTM's default U(-1/sqrt(nhid), ..)."""
        g = torch.Generator().manual_seed(self.seed)
        u = lambda a, *s: (torch.rand(*s, generator=g) * 2 - 1) * a
        V, E, H = self.ntoken, self.ninp, self.nhid
        sd = {"encoder.weight": u(0.1, V, E)}
        k = 1.0 / math.sqrt(H)
        for l in range(self.nlayers):
            sd["rnn.weight_ih_l%d" % l] = u(k, 4 * H, E if l == 0 else H)
            sd["rnn.weight_hh_l%d" % l] = u(k, 4 * H, H)
            sd["rnn.bias_ih_l%d" % l] = u(k, 4 * H)
            sd["rnn.bias_hh_l%d" % l] = u(k, 4 * H)
        sd["decoder.weight"] = sd["encoder.weight"] if self.tie_weights else u(0.1, V, H)
        sd["decoder.bias"] = torch.zeros(V)
        return sd

    def load_state_dict(self, sd):
        """The reference's keys, nn.LSTM's gate-major layout; bias_ih + bias_hh are folded."""
        H = self.nhid
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in sd.items()}

        def put(name, t):
            dst = self.view(self.p, name)
            if tuple(t.shape) != tuple(dst.shape):
                raise ValueError("LM state dict: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(dst.shape)))
            dst.copy_(t)
        put("encoder.weight", sd["encoder.weight"])
        for k in range(self.nlayers):
            put("w_ih%d" % k, _unit_major(sd["rnn.weight_ih_l%d" % k], H))
            put("w_hh%d" % k, _unit_major(sd["rnn.weight_hh_l%d" % k], H))
            put("b%d" % k, _unit_major(sd["rnn.bias_ih_l%d" % k] + sd["rnn.bias_hh_l%d" % k], H))
        if not self.tie_weights:
            put("decoder.weight", sd["decoder.weight"])
        put("decoder.bias", sd["decoder.bias"])
        self._refresh()

    def state_dict(self):
        H = self.nhid
        get = lambda n: self.view(self.p, n).detach().cpu().clone()
        sd = {"encoder.weight": get("encoder.weight")}
        for k in range(self.nlayers):
            sd["rnn.weight_ih_l%d" % k] = _gate_major(get("w_ih%d" % k), H).contiguous()
            sd["rnn.weight_hh_l%d" % k] = _gate_major(get("w_hh%d" % k), H).contiguous()
            sd["rnn.bias_ih_l%d" % k] = _gate_major(get("b%d" % k), H).contiguous()
            sd["rnn.bias_hh_l%d" % k] = torch.zeros(4 * H)
        sd["decoder.weight"] = sd["encoder.weight"] if self.tie_weights else get("decoder.weight")
        sd["decoder.bias"] = get("decoder.bias")
        return sd

    def grad_state_dict(self):
        """The last step's gradient in state_dict()'s layout (bias_ih and bias_hh both carry the folded bias's gradient; with
        tie_weights the shared tensor's gradient appears under both names)."""
        H = self.nhid
        get = lambda n: self.view(self.g, n).detach().cpu().clone()
        sd = {"encoder.weight": get("encoder.weight")}
        for k in range(self.nlayers):
            sd["rnn.weight_ih_l%d" % k] = _gate_major(get("w_ih%d" % k), H).contiguous()
            sd["rnn.weight_hh_l%d" % k] = _gate_major(get("w_hh%d" % k), H).contiguous()
            sd["rnn.bias_ih_l%d" % k] = _gate_major(get("b%d" % k), H).contiguous()
            sd["rnn.bias_hh_l%d" % k] = sd["rnn.bias_ih_l%d" % k].clone()
        sd["decoder.weight"] = get("decoder.weight")
        sd["decoder.bias"] = get("decoder.bias")
        return sd

    def optimizer_state(self):
        """m and v are in the trainer's flat (unit-major) layout: only this class reads them back."""
        return {"m": self.m.detach().cpu().clone(), "v": self.v.detach().cpu().clone(), "step": int(self.t), "lr": float(self.lr)}

    def load_optimizer_state(self, st):
        if st["m"].numel() != self.m.numel():
            raise ValueError("optimizer state does not fit this model")
        self.m.copy_(st["m"])
        self.v.copy_(st["v"])
        self.t, self.lr = int(st["step"]), float(st["lr"])

    def checkpoint(self, word2idx=None, idx2word=None, **extra):
        """The reference's LM checkpoint (the keys LM.__init__ reads) plus `optimizer` and whatever `extra` gives (epoch, metrics)."""
        idx2word = list(idx2word if idx2word is not None else self.scorer().idx2word)
        word2idx = dict(word2idx) if word2idx is not None else {w: i for i, w in enumerate(idx2word)}
        ck = {"word2idx": word2idx, "idx2word": idx2word, "ntoken": self.ntoken, "ninp": self.ninp, "nhid": self.nhid,
              "nlayers": self.nlayers, "dropout": self.dropout, "tie_weights": self.tie_weights,
              "model_state_dict": self.state_dict(), "optimizer": self.optimizer_state(), "seed": self.seed, "clip": self.clip}
        ck.update(extra)
        return ck

    @classmethod
    def from_checkpoint(cls, checkpoint, device="cuda", **kw):
        ck = checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu", weights_only=True)
        kw.setdefault("seed", int(ck.get("seed", 0)))
        kw.setdefault("clip", float(ck.get("clip", 0.25)))
        tr = cls(list(ck["idx2word"]), ck["ninp"], ck["nhid"], ck["nlayers"], dropout=kw.pop("dropout", ck["dropout"]),
                 tie_weights=bool(ck["tie_weights"]), device=device, state_dict=ck["model_state_dict"], **kw)
        if "optimizer" in ck:
            tr.load_optimizer_state(ck["optimizer"])
        return tr

    def _refresh(self):
        """Padded operand copies <- flat parameters (after every update)."""
        ops.cast_weight_f32(self.view(self.p, "encoder.weight"), dst=self.emb)
        if not self.tie_weights:
            ops.cast_weight_f32(self.view(self.p, "decoder.weight"), dst=self.dec_w)
        for k, layer in enumerate(self.layers):
            ops.cast_weight_f32(self.view(self.p, "w_ih%d" % k), dst=layer["w_ih"])
            ops.cast_weight_f32(self.view(self.p, "w_hh%d" % k), dst=layer["w_hh"], dst_t=layer["w_hh_t"])

    # ------------------------------------------------------------------------------------------ batches
    def _pack(self, sentences):
        seqs = sorted(([int(i) for i in s] for s in sentences), key=lambda s: (-len(s), s))      # canonical: order-independent
        if not seqs or len(seqs[-1]) < 2:
            raise ValueError("every sentence needs at least 2 ids (the last one '<eos>')")
        lens = np.array([len(s) - 1 for s in seqs])
        T = int(lens[0])
        n_t = [int((lens > t).sum()) for t in range(T)]
        off = [0]
        for n in n_t:
            off.append(off[-1] + n)
        inp = np.concatenate([np.array([seqs[s][t] for s in range(n_t[t])], dtype=np.int32) for t in range(T)])
        tgt = np.concatenate([np.array([seqs[s][t + 1] for s in range(n_t[t])], dtype=np.int32) for t in range(T)])
        if min(inp.min(), tgt.min()) < 0 or max(inp.max(), tgt.max()) >= self.ntoken:
            raise ValueError("word id outside the vocabulary")
        dev = self.device
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev, non_blocking=True)

        def segments(ids):                     # tokens by word, then by packed row: a fixed summation order per word
            rows = np.argsort(ids, kind="stable").astype(np.int32)
            sw = ids[rows]
            cut = np.flatnonzero(np.r_[True, sw[1:] != sw[:-1]])
            return to(rows), to(np.r_[cut, len(sw)]), to(sw[cut])
        return dict(T=T, n_t=n_t + [0], off=off, M=off[-1], inp=to(inp), tgt=to(tgt), inp_seg=segments(inp), tgt_seg=segments(tgt))

    def _mark(self, tag):
        if self.marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((tag, e))

    def _site_seed(self, site):
        return _mix64(_mix64(self.seed & _M64) ^ ((self.t * 0x100000001B3 + site) & _M64))

    # ------------------------------------------------------------------------------------------ one step
    def forward_backward(self, sentences):
        """Zeroes the gradient, runs forward and backward (no update) -> the device scalar mean NLL per predicted token."""
        ctx = self._forward(self._pack(sentences))
        self._backward(ctx)
        return ctx["loss"]

    def _forward(self, b):
        """Training forward of a packed batch -> what _backward needs (the loss under "loss")."""
        dev, H, E, V, p = self.device, self.nhid, self.ninp, self.ntoken, self.dropout
        Hp, M, T, n_t, off = _pad16(H), b["M"], b["T"], b["n_t"], b["off"]
        G = _pad(4 * H, 32)
        z = lambda r, c: torch.zeros((r, c), dtype=torch.float32, device=dev)
        # ---- forward
        x = z(M, _pad16(E))
        ops.lm_dropout(self.emb, x, E, p, self._site_seed(0), ids=b["inp"])
        saved = []
        for k, layer in enumerate(self.layers):
            xproj = ops.lm_proj(x, layer["w_ih"], layer["bias"], layer["K"])
            h, hprev, g = z(M, Hp), z(M, Hp), z(M, G)
            hd = z(M, Hp) if p > 0 else None
            c = torch.empty((M, H), dtype=torch.float32, device=dev)
            seed = self._site_seed(k + 1)
            self._mark("seq_begin")
            for t in range(T):
                a, pa, n, nn = off[t], off[t - 1] if t else 0, n_t[t], n_t[t + 1]
                ops.lstm_step_train(xproj[a:], h[pa:] if t else None, layer["w_hh"], c[pa:] if t else None, c[a:], h[a:], g[a:],
                                    hd[a:] if hd is not None else None, hprev[off[t + 1]:] if nn else None, n, nn, H, a, p, seed)
            self._mark("seq_end")
            saved.append(dict(x=x, hprev=hprev, g=g, c=c))
            x = hd if hd is not None else h
        loss, lse = ops.lm_nll_train(x, self.dec_w, self.dec_b, b["tgt"], H)
        return dict(b=b, saved=saved, x=x, lse=lse, loss=loss)

    def _backward(self, ctx):
        """Gradient of ctx's loss into the (zeroed) flat gradient buffer."""
        b, saved, x, lse = ctx["b"], ctx["saved"], ctx["x"], ctx["lse"]
        dev, H, E, V, p = self.device, self.nhid, self.ninp, self.ntoken, self.dropout
        Hp, M, T, n_t, off = _pad16(H), b["M"], b["T"], b["n_t"], b["off"]
        z = lambda r, c: torch.zeros((r, c), dtype=torch.float32, device=dev)
        self.g.zero_()
        # ---- output layer, a bounded chunk of tokens at a time: the scratch buffer is at most an eighth of (tokens, V)
        dh = z(M, Hp)
        chunk = max(64, _pad((M + 7) // 8, 64))
        scratch = torch.empty((min(chunk, M), _pad(V, 64)), dtype=torch.float32, device=dev)
        gdw, gdb = self.view(self.g, "decoder.weight"), self.view(self.g, "decoder.bias")
        for a in range(0, M, chunk):
            e = min(M, a + chunk)
            dl = scratch[:e - a]
            ops.lm_dlogits(x[a:e], self.dec_w, self.dec_b, lse[a:e], H, 1.0 / M, dl)
            ops.gemm_nn(dl, self.dec_w[:, :H], out=dh[a:e, :H])
            _gemm_tn(dl, x[a:e], gdw, V, H)
            ops.lm_colsum(dl, V, gdb, accumulate=a > 0)
        del scratch
        # the "- onehot" half, one row operation per token (see csrc/lm_train.hip)
        ops.lm_sub_rows(dh, self.dec_w, b["tgt"], H, 1.0 / M)
        ops.lm_emb_grad(x, *b["tgt_seg"], H, gdw, scale=-1.0 / M)
        ops.lm_emb_grad(torch.ones((M, 1), dtype=torch.float32, device=dev), *b["tgt_seg"], 1, gdb.view(V, 1), scale=-1.0 / M)
        if p > 0:
            ops.lm_dropout(dh, dh, H, p, self._site_seed(self.nlayers))
        # tests: xs[k] = the dropped activation of site k (embedding, after layer 0, ...), dx[k] = the gradient at site k before dropout
        last = dict(b=b, xs=[sv["x"] for sv in saved] + [x], dx=[None] * (self.nlayers + 1)) if self.keep_intermediates else None
        if last is not None:
            last["dx"][self.nlayers] = dh
        # ---- the layers, top down
        for k in range(self.nlayers - 1, -1, -1):
            layer, sv = self.layers[k], saved[k]
            g, c, K = sv["g"], sv["c"], layer["K"]
            dc = torch.empty((n_t[0], H), dtype=torch.float32, device=dev)
            self._mark("seq_begin")
            for t in range(T - 1, -1, -1):
                a, n, nn = off[t], n_t[t], n_t[t + 1]
                ops.lstm_bptt_step(dh[a:], g[off[t + 1]:] if nn else None, g[a:], layer["w_hh_t"], c[a:], c[off[t - 1]:] if t else None,
                                   dc, n, nn, H)
            self._mark("seq_end")
            _gemm_tn(g, sv["hprev"], self.view(self.g, "w_hh%d" % k), 4 * H, H)
            _gemm_tn(g, sv["x"], self.view(self.g, "w_ih%d" % k), 4 * H, K)
            ops.lm_colsum(g, 4 * H, self.view(self.g, "b%d" % k))
            dx = z(M, _pad16(K))
            ops.gemm_nn(g, layer["w_ih"][:, :K], out=dx[:, :K])
            if p > 0:
                ops.lm_dropout(dx, dx, K, p, self._site_seed(k))
            if last is not None:
                last["dx"][k] = dx
                if k == self.nlayers - 1:
                    last["dG"] = g
            dh = dx
            saved[k] = None
        ops.lm_emb_grad(dh, *b["inp_seg"], E, self.view(self.g, "encoder.weight"))
        self.last = last

    def update(self):
        """Clip by the global norm, Adam, refresh the operand copies."""
        self.t += 1
        scale = None
        if self.clip > 0:
            ops.lm_sumsq(self.g, self._sumsq)
            ops.clip_coef(self._sumsq, self.clip, self._coef)
            scale = self._coef
        ops.adam_step(self.p, self.g, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps, self.t, grad_scale=scale)
        self._refresh()

    def step(self, sentences):
        """sentences: id lists (>= 2 ids each, the last one '<eos>') -> device scalar, the mean NLL per predicted token."""
        loss = self.forward_backward(sentences)
        self.update()
        return loss

    # ------------------------------------------------------------------------------------------ evaluation
    def scorer(self):
        """An LSTMLM over this trainer's operand copies (no copy; dropout is not applied): the inference kernels of csrc/lm.hip."""
        lm = LSTMLM.__new__(LSTMLM)
        lm.idx2word = self.idx2word or ["<eos>", "<oov>"] + ["w%d" % i for i in range(self.ntoken - 2)]
        lm.word2idx = {w: i for i, w in enumerate(lm.idx2word)}
        lm.ntoken, lm.ninp, lm.nhid, lm.nlayers, lm.tie_weights = self.ntoken, self.ninp, self.nhid, self.nlayers, self.tie_weights
        lm.oov_id, lm.device = lm.word2idx.get("<oov>", 1), self.device
        lm.emb, lm.dec_w, lm.dec_b = self.emb, self.dec_w, self.dec_b
        lm.layers = [dict(w_ih=l["w_ih"], w_hh=l["w_hh"], bias=l["bias"], K=l["K"]) for l in self.layers]
        return lm

    @torch.no_grad()
    def evaluate(self, sentences, per_sentence=False):
        """-> (summed NLL, number of predicted tokens), dropout off; per_sentence: the (S,) fp32 CPU tensor of LSTMLM.score instead
        of the sum."""
        seqs = [[int(i) for i in s] for s in sentences]
        nll = self.scorer()._nll(seqs).cpu() if seqs else torch.zeros(0)
        count = sum(len(s) - 1 for s in seqs)
        return (nll if per_sentence else float(nll.double().sum())), count
