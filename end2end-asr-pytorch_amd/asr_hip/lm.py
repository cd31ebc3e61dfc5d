"""The LSTM language model of LM rescoring (reference: utils/lstm_utils.py LM / RNNModel), batched over sentences on csrc/lm.hip.

The reference evaluates one sentence per call at batch 1: nn.LSTM over the words, a V-wide Linear, CrossEntropyLoss.  Here a
list of sentences is ONE forward: the sentences are sorted longest first and packed time-major (token (s, t) is row
step_off[t] + s), so the sentences still running at step t are a prefix of n_t rows.  Per layer: one input-projection launch over
every token (bias_ih + bias_hh folded), then one asr_lstm_step launch per time step on the n_t running rows.  The output layer is
asr_lm_nll_partials / asr_lm_nll_finish: per-token log-sum-exp and target logit without a (tokens, V) logits tensor.

Numerics: fp32 storage, f32-input MFMA, fp32 accumulation (the reference LM is fp32) whatever the ASR model's --precision.  A
sentence's NLL is bitwise independent of the other sentences of the call.
"""
import torch

from . import ops


def _pad16(n):
    return (n + 15) // 16 * 16


def _pad_cols(t):
    """(R, C) -> (R, 16 * ceil(C / 16)) fp32, zeros in the padding (the kernels contract whole 16-column steps)."""
    out = torch.zeros((t.shape[0], _pad16(t.shape[1])), dtype=torch.float32, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _unit_major(t, H):
    """nn.LSTM's gate-major rows (i | f | g | o, H each) -> unit-major (row 4 j + q = gate q of unit j), so that the four gates of a
    hidden unit sit in one MFMA lane (csrc/lm.hip: lstm_step)."""
    return t.reshape(4, H, *t.shape[1:]).transpose(0, 1).reshape(4 * H, *t.shape[1:])


class LSTMLM:
    """LSTMLM(checkpoint, device): `checkpoint` is the reference's LM file (a path or the loaded dict: word2idx, idx2word, ntoken,
    ninp, nhid, nlayers, dropout, tie_weights, model_state_dict).  Dropout is not applied (the reference evaluates in eval())."""

    def __init__(self, checkpoint, device="cuda"):
        ck = checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu", weights_only=True)
        self.word2idx, self.idx2word = ck["word2idx"], ck["idx2word"]
        self.ntoken, self.ninp, self.nhid, self.nlayers = int(ck["ntoken"]), int(ck["ninp"]), int(ck["nhid"]), int(ck["nlayers"])
        self.tie_weights = bool(ck["tie_weights"])
        if "<oov>" not in self.word2idx or "<eos>" not in self.word2idx:
            raise ValueError("the LM vocabulary needs '<eos>' and '<oov>'")
        self.oov_id = self.word2idx["<oov>"]
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in ck["model_state_dict"].items()}
        V, E, H = self.ntoken, self.ninp, self.nhid
        emb = sd["encoder.weight"]
        dec_w = emb if self.tie_weights else sd["decoder.weight"]
        if emb.shape != (V, E) or dec_w.shape != (V, H) or sd["decoder.bias"].shape != (V,):
            raise ValueError("LM checkpoint shapes do not match ntoken=%d ninp=%d nhid=%d" % (V, E, H))
        dev = torch.device(device)
        self.device = dev
        self.emb = _pad_cols(emb).to(dev)
        self.layers = []
        for k in range(self.nlayers):
            w_ih, w_hh = sd["rnn.weight_ih_l%d" % k], sd["rnn.weight_hh_l%d" % k]
            if w_ih.shape != (4 * H, E if k == 0 else H) or w_hh.shape != (4 * H, H):
                raise ValueError("LM checkpoint: layer %d has weight_ih %s, weight_hh %s" % (k, tuple(w_ih.shape), tuple(w_hh.shape)))
            bias = sd["rnn.bias_ih_l%d" % k] + sd["rnn.bias_hh_l%d" % k]
            self.layers.append(dict(w_ih=_pad_cols(_unit_major(w_ih, H)).to(dev), w_hh=_pad_cols(_unit_major(w_hh, H)).to(dev),
                                    bias=_unit_major(bias, H).contiguous().to(dev), K=w_ih.shape[1]))
        self.dec_w = _pad_cols(dec_w).to(dev)
        self.dec_b = sd["decoder.bias"].contiguous().to(dev)

    def ids(self, sentence):
        """(word ids of sentence.split() + ['<eos>'], number of out-of-vocabulary words)   (reference: LM.seq_to_tensor)"""
        out, oov = [], 0
        for w in sentence.split() + ["<eos>"]:
            i = self.word2idx.get(w)
            if i is None:
                i, oov = self.oov_id, oov + 1
            out.append(i)
        return out, oov

    @torch.no_grad()
    def score(self, sentences):
        """-> (nll_sums (S,) fp32 CPU tensor, oov_counts list): per sentence the summed NLL of words[1:] given words[:-1] with
        words = sentence.split() + ['<eos>'] (reference: LM.evaluate's total_loss) and its out-of-vocabulary count.  A sentence
        without words scores 0.  Identical sentences share one row."""
        uniq = {}
        for s in sentences:
            uniq.setdefault(s, len(uniq))
        seqs = [self.ids(s) for s in uniq]
        nll = torch.zeros(len(seqs), dtype=torch.float32)
        run = [i for i, (ids, _) in enumerate(seqs) if len(ids) > 1]
        if run:
            nll[run] = self._nll([seqs[i][0] for i in run]).cpu()
        return nll[[uniq[s] for s in sentences]], [seqs[uniq[s]][1] for s in sentences]

    def forward_packed(self, seqs):
        """Last layer's hidden states of the id sequences `seqs` (each >= 2 ids; inputs ids[:-1]) -> dict: h (M, 16 * ceil(nhid / 16))
        time-major packed in longest-first order (row step_off[t] + s; the layout of torch's pack_sequence), order (sorted position
        -> index into seqs), lens, step_off and the int32 device tensors tgt (M,), off, ln."""
        order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))
        lens = [len(seqs[i]) - 1 for i in order]                       # input tokens = words[:-1]
        T = lens[0]
        n_t = [sum(1 for L in lens if L > t) for t in range(T)]
        step_off = [0]
        for n in n_t[:-1]:
            step_off.append(step_off[-1] + n)
        inp, tgt = [], []
        for t in range(T):
            for s in range(n_t[t]):
                ids = seqs[order[s]]
                inp.append(ids[t])
                tgt.append(ids[t + 1])
        dev, H, Hp = self.device, self.nhid, _pad16(self.nhid)
        inp = torch.tensor(inp, dtype=torch.int32).to(dev, non_blocking=True)
        tgt = torch.tensor(tgt, dtype=torch.int32).to(dev, non_blocking=True)
        M = len(tgt)
        x, ids = self.emb, inp
        for layer in self.layers:
            xproj = ops.lm_proj(x, layer["w_ih"], layer["bias"], layer["K"], ids=ids)
            h = torch.zeros((M, Hp), dtype=torch.float32, device=dev)
            c = torch.empty((n_t[0], H), dtype=torch.float32, device=dev)
            for t in range(T):
                a = step_off[t]
                prev = h[step_off[t - 1]:] if t else None
                ops.lstm_step(xproj[a:], prev, layer["w_hh"], c, h[a:], n_t[t], H)
            x, ids = h, None
        return dict(h=x, order=order, lens=lens, step_off=step_off, tgt=tgt,
                    off=torch.tensor(step_off, dtype=torch.int32).to(dev, non_blocking=True),
                    ln=torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True))

    def _nll(self, seqs):
        f = self.forward_packed(seqs)
        sums = ops.lm_nll(f["h"], self.dec_w, self.dec_b, f["tgt"], self.nhid, f["off"], f["ln"])
        out = torch.empty_like(sums)
        out[torch.tensor(f["order"], device=sums.device)] = sums
        return out
