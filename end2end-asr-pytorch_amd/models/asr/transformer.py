"""End-to-end Transformer ASR model -- same classes, constructor signatures, forward contracts and state_dict keys as
the reference (reference: models/asr/transformer.py), executed by libasr_hip.so.

Reference behaviours that are reproduced on purpose: `input_lengths` are PRE-CNN frame counts
compared against the POST-CNN time axis; every parameter with dim > 1 is re-initialised with xavier_uniform_ last;
decoder rows whose input token is EOS are zeroed; targets are always padded to --tgt-max-len; the encoder owns a Dropout
it never applies.
"""

import math

import numpy as np
import torch
import torch.nn as nn

from asr_hip import functions as F_
from asr_hip import ops, search
from asr_hip import params as P
from models.common_layers import (ConvolutionModule, LowRankMultiHeadAttention, LowRankPositionwiseFeedForward, MultiHeadAttention,
                                  PositionalEncoding, PositionwiseFeedForwardWithConv, check_conv_module_kernel, check_pos_encoding)
from utils import constant


def frames_after_cnn(T, feat):
    """Encoder positions produced by T input frames: vgg_cnn = two 2x2/2 max-pools behind same-padded 3x3 convolutions; emb_cnn = time
    kernel 11 / stride 2 / padding 10, then kernel 11 / stride 1 / no padding; no front end: T."""
    if feat == "vgg_cnn":
        return (int(T) // 2) // 2
    if feat == "emb_cnn":
        return ((int(T) + 20 - 11) // 2 + 1) - 10
    return int(T)


def encoder_frame_span(j, feat):
    """The input-frame interval [a, b) encoder frame j stands for (CTC alignment timestamps; seconds = frames * --window-stride).
    vgg_cnn: the 4 frames under its two 2x2 pools; emb_cnn: the stride-2 cell at the centre of its receptive field [2j - 10, 2j + 20];
    no front end: the frame itself.  The caller clamps b to the utterance's true input length."""
    j = int(j)
    if feat == "vgg_cnn":
        return 4 * j, 4 * j + 4
    if feat == "emb_cnn":
        return 2 * j + 4, 2 * j + 6
    return j, j + 1


def ctc_collapse(ids, length=None, blank=constant.PAD_TOKEN):
    """Best-path CTC decoding of one utterance's frame-wise argmax ids: the first `length` frames, repeats merged, blanks dropped."""
    out, prev = [], None
    for x in ids[:len(ids) if length is None else max(0, int(length))]:
        if x != prev and x != blank:
            out.append(int(x))
        prev = x
    return out


def check_transducer(dim_joint, context, dim_model=None):
    """(J, C) of a transducer head, or ValueError: the joint width J = --transducer-dim-joint is the K of rnnt_out's GEMM and the N of
    rnnt_enc's, and the joint kernel moves whole 16-byte chunks: a positive multiple of 8 (so must dim_model be, the K of rnnt_enc);
    the stateless predictor's context C = --transducer-context is 1 or 2."""
    J, C = int(dim_joint), int(context)
    if J < 8 or J % 8 != 0:
        raise ValueError("--transducer-dim-joint %d: the joint width must be a positive multiple of 8 (whole 16-byte chunks in the joint "
                         "kernel and in the vocabulary projection's GEMM)" % J)
    if C not in (1, 2):
        raise ValueError("--transducer-context %d: the stateless predictor looks back 1 or 2 labels" % C)
    if dim_model is not None and int(dim_model) % 8 != 0:
        raise ValueError("a transducer head needs --dim-model to be a multiple of 8, got %d" % int(dim_model))
    return J, C


def check_prune_range(S):
    """The band width S of pruned transducer training (--transducer-prune-range): 0 = the full lattice, otherwise 2..64."""
    S = int(S or 0)
    if S != 0 and not 2 <= S <= 64:
        raise ValueError("--transducer-prune-range must be 0 (off) or lie in 2..64, got %d" % S)
    return S


def hypothesis_labels(ids):
    """The label ids of a decoded hypothesis as a CTC target: SOS and EOS dropped, PAD dropped from the end.  A PAD (= the CTC blank)
    left inside has no alignment, and the aligner reports it so."""
    out = [int(x) for x in ids if int(x) not in (constant.SOS_TOKEN, constant.EOS_TOKEN)]
    while out and out[-1] == constant.PAD_TOKEN:
        out.pop()
    return out


def _lengths_to_device(input_lengths, device):
    t = torch.as_tensor(input_lengths)
    return t.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


class Transformer(nn.Module):
    """Transformer(encoder, decoder, feat_extractor='vgg_cnn')   (reference: transformer.py:16-57)

    ctc_head=True (train.py --ctc-weight > 0) adds `ctc_linear`, a CTC output layer on the ENCODER output for joint
    CTC / attention training and decoding (blank = PAD).  Without it the module, its parameters and its state_dict keys do not exist.

    transducer=dict(dim_joint=J, context=C) (train.py --transducer-weight > 0) adds a transducer head on the ENCODER
    output: `rnnt_enc` (D -> J), the stateless predictor's tables `rnnt_embed.{0..C-1}` ((V, J) each, one per context position) and
    `rnnt_out` (J -> V); blank = PAD.  None: none of them exists, nor their state_dict keys.  prune_range=S > 0 in that dict (train.py
    --transducer-prune-range) adds the simple joiner of pruned transducer training, `rnnt_simple_am` (D -> V) on the encoder output and
    `rnnt_simple_lm` (J -> V) on the predictor; S = 0 (the default): neither exists and the head is the full-lattice one."""

    def __init__(self, encoder, decoder, feat_extractor='vgg_cnn', ctc_head=False, transducer=None):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.id2label = decoder.id2label
        self.feat_extractor = feat_extractor
        if ctc_head:
            self.ctc_linear = nn.Linear(decoder.dim_model, decoder.num_trg_vocab)
        if transducer is not None:
            J, C = check_transducer(transducer.get("dim_joint", 256), transducer.get("context", 2), decoder.dim_model)
            self.rnnt_enc = nn.Linear(decoder.dim_model, J)
            self.rnnt_embed = nn.ModuleList([nn.Embedding(decoder.num_trg_vocab, J) for _ in range(C)])
            self.rnnt_out = nn.Linear(J, decoder.num_trg_vocab)
            self.rnnt_prune_range = check_prune_range(transducer.get("prune_range", 0))
            if self.rnnt_prune_range > 0:
                self.rnnt_simple_am = nn.Linear(decoder.dim_model, decoder.num_trg_vocab)
                self.rnnt_simple_lm = nn.Linear(J, decoder.num_trg_vocab)
        if feat_extractor == 'emb_cnn':
            self.conv = nn.Sequential(
                nn.Conv2d(1, 32, kernel_size=(41, 11), stride=(2, 2), padding=(0, 10)), nn.BatchNorm2d(32),
                nn.Hardtanh(0, 20, inplace=True),
                nn.Conv2d(32, 32, kernel_size=(21, 11), stride=(2, 1)), nn.BatchNorm2d(32),
                nn.Hardtanh(0, 20, inplace=True))
        elif feat_extractor == 'vgg_cnn':
            # indices 0,2,5,7 hold the parameters (state_dict keys conv.{0,2,5,7}.*); ReLU / pooling are fused in-kernel
            self.conv = nn.Sequential(
                nn.Conv2d(1, 64, 3, stride=1, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, stride=1, padding=1), nn.ReLU(),
                nn.MaxPool2d(2, stride=2),
                nn.Conv2d(64, 128, 3, stride=1, padding=1), nn.ReLU(), nn.Conv2d(128, 128, 3, stride=1, padding=1),
                nn.ReLU(), nn.MaxPool2d(2, stride=2))
        for p in self.parameters():            # reference: transformer.py:55-57 (overrides every earlier init)
            if p.dim() > 1 and not getattr(p, "_asr_keep_init", False):      # (a ConvolutionModule's depthwise taps keep Conv1d's init)
                nn.init.xavier_uniform_(p)

    # -------------------------------------------------------------------------------------------- front end
    def _features(self, padded_input):
        """(B,1,F,T) -> (B,T',C*F') with feature index c*F'+f   (reference: transformer.py:70-76)"""
        if self.feat_extractor == 'vgg_cnn':
            c = self.conv
            return F_.VGGFn.apply(padded_input, c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[5].weight, c[5].bias,
                                  c[7].weight, c[7].bias)
        if self.feat_extractor == 'emb_cnn':
            c = self.conv
            return F_.EmbCNNFn.apply(padded_input, c[0].weight, c[0].bias, c[1].weight, c[1].bias, c[3].weight, c[3].bias,
                                     c[4].weight, c[4].bias, c[1], c[4], self.training)
        b, c, f, t = padded_input.shape
        return padded_input.reshape(b, c * f, t).transpose(1, 2).contiguous().to(ops.compute_dtype())

    # -------------------------------------------------------------------------------------------- encoder CTC head
    def ctc_frame_lengths(self, input_lengths, enc_frames):
        """True encoder frames per utterance, min(T', frames_after_cnn(length)): the CTC input lengths.  (The PRE-CNN lengths the
        encoder masks with are a reference quirk that stays where it is; CTC does not inherit it.)"""
        return [min(int(enc_frames), frames_after_cnn(int(n), self.feat_extractor)) for n in torch.as_tensor(input_lengths).tolist()]

    def ctc_logits(self, enc_out):
        """(B,T',V) fp32 logits of the CTC head on the encoder output, through the project's linear autograd path."""
        if not hasattr(self, "ctc_linear"):
            raise ValueError("this model has no encoder CTC head (ctc_linear): it was trained with --ctc-weight 0")
        # (called BEFORE the decoder: the fp32-logit hand-over slot of F_.linear belongs to the vocabulary projection that runs last)
        return F_.linear(enc_out, self.ctc_linear.weight, self.ctc_linear.bias, True, True)

    @torch.no_grad()
    def ctc_greedy(self, enc_out, lengths, return_ids=False):
        """Best-path decoding from the CTC head alone: frame-wise argmax, repeats merged and blanks dropped inside each utterance's
        true frames (`lengths`, encoder frames) -> strings (return_ids: (strings, label ids)).  The cheap way to see whether the head
        has learnt anything."""
        logits = self.ctc_logits(enc_out)
        B, T, V = logits.shape
        ids = ops.argmax_rows(logits.reshape(B * T, V)).view(B, T).cpu().tolist()
        hyp_ids = [ctc_collapse(row, n) for row, n in zip(ids, lengths)]
        strs = ["".join(self.id2label[x] for x in row) for row in hyp_ids]
        return (strs, hyp_ids) if return_ids else strs

    @torch.no_grad()
    def ctc_beam_search(self, enc_out, lengths, beam_width, nbest=1, candidates=0, lm=None, lm_weight=0.1, c_weight=1, return_ids=False,
                        rescoring_weight=0.0, ngram=None, ngram_weight=0.0, length_bonus=0.0, context=None, context_score=0.0):
        """Prefix beam search over the CTC head's posteriors alone (csrc/ctc_beam.hip): no decoder step.  lengths:
        true encoder frames per utterance (ctc_frame_lengths); beam_width W in 1..16 prefixes kept per frame, candidates C (0: min(V, 16))
        labels tried per frame.  One device-to-host copy.  The kernel's W hypotheses of an utterance, score = log-probability summed over
        the alignments, are ranked like a decoder beam's (asr_hip.search.rank_ended): score + sqrt(words) * c_weight, or with lm
        (utils.lstm_utils.LM) score + lm_weight * (lm - 2 * oov) + sqrt(words) * c_weight, all utterances' hypotheses in ONE batched LM
        call.  -> per utterance the min(nbest, found) best strings, best first (return_ids: (strings, label ids), same nesting); the ids
        are CTC labels as they stand: no SOS, no EOS.
        rescoring_weight = lambda in (0, 1]: attention rescoring.  ALL W hypotheses of every utterance get 'ctc_score' (the kernel's),
        'att_score' (Decoder.score_hypotheses: one teacher-forced decoder pass, one more small device-to-host copy) and score =
        (1 - lambda) * ctc_score + lambda * att_score before the ranking above; 0 makes no decoder launch.
        ngram (utils.ngram.NgramLM over this model's labels): first-pass fusion.  The kernel prunes its beam by the CTC score +
        ngram_weight * the n-gram's log-probability of the labels + length_bonus * their number (contexts open with SOS, the final
        order counts EOS), so the LM decides which prefixes survive; its table goes to the device once per LM.  Every hypothesis gets
        'ctc_score', 'ngram_score' (with the EOS term) and score = ctc_score + ngram_weight * ngram_score + length_bonus * labels, with
        rescoring (1 - lambda) * ctc_score + lambda * att_score + the same two terms, before the ranking above.  None: the plain search.
        context (utils.context.ContextGraph over this model's labels): phrase biasing, with or without ngram.  The kernel adds
        context_score * the phrase credit of every prefix to its pruning key, so hypotheses that spell a listed phrase survive the
        beam; its table goes to the device once per list.  Every hypothesis gets 'context_credit' (int: the labels earned, an unfinished
        phrase earns nothing), 'ctc_score' and 'ngram_score' (0 without ngram; length_bonus still counts), and context_score *
        context_credit joins score beside the n-gram terms on both branches.  None: the two paths above, unchanged."""
        W = int(beam_width)
        lam = float(rescoring_weight)
        a, beta, gamma = float(ngram_weight), float(length_bonus), float(context_score)
        if ngram is not None:
            ngram.check_labels(self.id2label)
        if context is not None:
            context.check_labels(self.id2label)
        if not 0.0 <= lam <= 1.0:
            raise ValueError("rescoring_weight must lie in [0, 1], got %g" % lam)
        if not 1 <= W <= 16:
            raise ValueError("ctc_beam_search keeps beam_width prefixes per frame in the kernel's beam: 1..16, got %d" % W)
        if nbest < 1:
            raise ValueError("nbest must be at least 1, got %d" % nbest)
        logits = self.ctc_logits(enc_out)
        B, T, V = logits.shape
        fused = ngram is not None or context is not None
        kw = dict(ngram=ngram, alpha=a, beta=beta, bos=constant.SOS_TOKEN, eos=constant.EOS_TOKEN) if fused else {}
        if context is not None:
            kw.update(context=context, gamma=gamma)
        out = ops.ctc_beam_search(logits, _lengths_to_device(lengths, logits.device), W, candidates, W, constant.PAD_TOKEN, **kw)
        ended = search.nbest_to_host(out, B, W, T, fused, context is not None)
        if fused:
            search.fuse_scores(ended, 'ctc_score', a, beta, gamma)
        if lam > 0.0:
            att = self.decoder.score_hypotheses(enc_out, [[h['yseq'] for h in hs] for hs in ended])
            for hs, scores_b in zip(ended, att):
                for h, att_score in zip(hs, scores_b):
                    h.setdefault('ctc_score', h['score'])
                    h['att_score'] = att_score
                    h['score'] = (1.0 - lam) * h['ctc_score'] + lam * att_score
                    if fused:
                        h['score'] += a * h['ngram_score'] + beta * len(h['yseq'])
                    if context is not None:
                        h['score'] += gamma * h['context_credit']
        return search.render_nbest(ended, nbest, c_weight, self.id2label, lm, lm_weight, return_ids)

    @torch.no_grad()
    def ctc_align(self, enc_out, lengths, targets, target_lengths=None):
        """Forced alignment of label ids against the CTC head (csrc/ctc_align.hip).  lengths: true encoder frames
        per utterance (ctc_frame_lengths); targets: (B,L) int64 with target_lengths, or a list of id lists.  One device-to-host copy.
        -> per utterance {"score": log-probability of the best path (-inf: no feasible alignment), "frames": T_b, "path": lattice state
        per frame, "labels": [{"id", "label", "start_frame", "end_frame" (one past the last), "logp"}]} in encoder frames."""
        logits = self.ctc_logits(enc_out)
        B, T, V = logits.shape
        dev = logits.device
        if not torch.is_tensor(targets):
            rows = [[int(x) for x in r] for r in targets]
            target_lengths = [len(r) for r in rows]
            tg = torch.zeros((B, max([1] + target_lengths)), dtype=torch.int64)
            for b, r in enumerate(rows):
                tg[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
            targets = tg
        if targets.shape[1] == 0:
            targets = torch.zeros((B, 1), dtype=torch.int64)
        targets = targets.to(dev).contiguous()
        out = ops.ctc_align(logits, targets, _lengths_to_device(lengths, dev), _lengths_to_device(target_lengths, dev),
                            constant.PAD_TOKEN)
        Lmax = targets.shape[1]
        flat = torch.cat([out["path"].reshape(-1), out["start"].reshape(-1), out["end"].reshape(-1),
                          out["lab_score"].view(torch.int32).reshape(-1), out["score"].view(torch.int32),
                          targets.to(torch.int32).reshape(-1)]).cpu()
        path, start, end, lab, score, tg = torch.split(flat, [B * T, B * Lmax, B * Lmax, B * Lmax, B, B * Lmax])
        path, start, end = path.view(B, T).tolist(), start.view(B, Lmax).tolist(), end.view(B, Lmax).tolist()
        lab, score, tg = lab.view(torch.float32).view(B, Lmax).tolist(), score.view(torch.float32).tolist(), tg.view(B, Lmax).tolist()
        result = []
        for b in range(B):
            n = max(0, min(T, int(lengths[b])))
            labels = [{"id": tg[b][l], "label": self.id2label[tg[b][l]], "start_frame": start[b][l], "end_frame": end[b][l],
                       "logp": lab[b][l]} for l in range(Lmax) if start[b][l] >= 0]
            result.append({"score": score[b], "frames": n, "path": path[b][:n] if score[b] > -math.inf else [], "labels": labels})
        return result

    # -------------------------------------------------------------------------------------------- transducer head
    def _need_transducer(self):
        if not hasattr(self, "rnnt_out"):
            raise ValueError("this model has no transducer head (rnnt_enc / rnnt_embed / rnnt_out): it was trained with "
                             "--transducer-weight 0")

    def _rnnt_zero_pe(self, n, device):
        """(n, J) fp32 zeros: the position term F_.EmbedFn adds (the predictor has none), kept per device and grown on demand."""
        buf = self.__dict__.get("_rnnt_pe")
        if buf is None or buf.shape[0] < n or buf.device != device:
            buf = self.__dict__["_rnnt_pe"] = torch.zeros((max(int(n), 64), self.rnnt_out.in_features), device=device)
        return buf

    def _rnnt_predict(self, tokens):
        """p (B,n,J) = sum_k E_k[tokens[k]] in the compute dtype; tokens: C tensors (B,n) int64, tokens[k] = the label k places back."""
        p = None
        for emb, tok in zip(self.rnnt_embed, tokens):
            tok = tok.contiguous()
            q = F_.EmbedFn.apply(tok, emb.weight, self._rnnt_zero_pe(tok.shape[1], tok.device), 1.0, 0.0, -1, True)
            p = q if p is None else p + q
        return p

    def transducer_logits(self, enc_out, targets, target_lengths):
        """(B,T',U+1,V) fp32 joint logits of the transducer head, U = the longest transcript of the batch
        (target_lengths are host values): e = rnnt_enc(enc_out); p[b,u] = sum_k rnnt_embed.k[y_{u-k}] with SOS wherever u - k < 1; z =
        tanh(e + p) (F_.RnntJointFn); logits = rnnt_out(z).  targets: (B,L) raw label ids without SOS / EOS, as the CTC term takes them."""
        self._need_transducer()
        tl = [int(x) for x in torch.as_tensor(target_lengths).tolist()]
        B, T = enc_out.shape[0], enc_out.shape[1]
        V, C = self.rnnt_out.out_features, len(self.rnnt_embed)
        tg = torch.as_tensor(targets).to(enc_out.device, dtype=torch.int64)
        U = max(0, min(int(tg.shape[1]), max(tl) if tl else 0))
        F_.check_rnnt_shape(B, T, U + 1, V)                     # before the first launch
        sos = torch.full((B, C), constant.SOS_TOKEN, dtype=torch.int64, device=tg.device)
        hist = torch.cat([sos, tg[:, :U].clamp(0, V - 1)], 1)    # (a label outside [0,V) has no table row; the loss refuses it by itself)
        tokens = [hist[:, C - 1 - k:C + U - k] for k in range(C)]
        e = F_.linear(enc_out, self.rnnt_enc.weight, self.rnnt_enc.bias, False, True)
        z = F_.RnntJointFn.apply(e, self._rnnt_predict(tokens))
        return F_.linear(z, self.rnnt_out.weight, self.rnnt_out.bias, True, True)

    def _rnnt_tokens(self, targets, target_lengths, device):
        """(tg (B,L) int64 on the device, U = the longest transcript, the predictor's C token tensors (B,U+1)) as transducer_logits builds
        them."""
        tl = [int(x) for x in torch.as_tensor(target_lengths).tolist()]
        V, C = self.rnnt_out.out_features, len(self.rnnt_embed)
        tg = torch.as_tensor(targets).to(device, dtype=torch.int64)
        U = max(0, min(int(tg.shape[1]), max(tl) if tl else 0))
        sos = torch.full((tg.shape[0], C), constant.SOS_TOKEN, dtype=torch.int64, device=tg.device)
        hist = torch.cat([sos, tg[:, :U].clamp(0, V - 1)], 1)
        return tg, U, [hist[:, C - 1 - k:C + U - k] for k in range(C)]

    def transducer_band(self, enc_out, input_lengths, padded_target, target_lengths):
        """The simple joiner's loss and the band it chooses (pruned transducer training) -> (L_simple, s_begin (B,T')
        int32 on the device, W = min(S, U+1), U, p): am = rnnt_simple_am(enc_out), lm = rnnt_simple_lm(p), both fp32; F_.RnntSimpleFn
        gives the loss and the arc posteriors of am + lm's lattice without a (T',U+1,V) tensor, ops.rnnt_prune_ranges the first label
        position of every frame's window.  The band is a constant: no gradient flows through it.  Nothing is copied to the host."""
        self._need_transducer()
        S = int(getattr(self, "rnnt_prune_range", 0))
        if S <= 0:
            raise ValueError("this model has no simple joiner (rnnt_simple_am / rnnt_simple_lm): it was built with "
                             "--transducer-prune-range 0")
        tg, U, tokens = self._rnnt_tokens(padded_target, target_lengths, enc_out.device)
        W = min(S, U + 1)
        F_.check_rnnt_shape(enc_out.shape[0], enc_out.shape[1], W, self.rnnt_out.out_features)       # before the first launch
        frames = _lengths_to_device(self.ctc_frame_lengths(input_lengths, enc_out.shape[1]), enc_out.device)
        tl = _lengths_to_device(target_lengths, enc_out.device)
        p = self._rnnt_predict(tokens)
        am = F_.linear(enc_out, self.rnnt_simple_am.weight, self.rnnt_simple_am.bias, True, True)
        lm = F_.linear(p, self.rnnt_simple_lm.weight, self.rnnt_simple_lm.bias, True, True)
        simple, gb, gl = F_.RnntSimpleFn.apply(am, lm, tg, frames, tl, constant.PAD_TOKEN)
        s_begin = ops.rnnt_prune_ranges(gb, gl, frames, tl, S)
        return simple, s_begin, W, U, p, (tg, frames, tl)

    def transducer_pruned_loss(self, enc_out, input_lengths, padded_target, target_lengths, simple_scale=0.5):
        """(L_pruned, L_simple) of a batch, each mean_b nll_b / max(U_b, 1) (train.py --transducer-prune-range S):
        the simple joiner's loss and band (transducer_band), then z[b,t,w] = tanh(e[b,t] + p[b, s(t) + w]) (F_.RnntJointPrunedFn), logits
        (B,T',W,V) = rnnt_out(z) and the lattice with every node outside the band cut off (F_.RnntPrunedFn).  The training loss is
        L_pruned + simple_scale * L_simple; simple_scale itself is applied by the caller (transducer_loss).  Call it BEFORE the decoder
        runs, like transducer_loss: RnntPrunedFn claims the hand-over slot rnnt_out has just left."""
        if not float(simple_scale) >= 0.0:
            raise ValueError("--transducer-simple-scale must be >= 0, got %g" % float(simple_scale))
        simple, s_begin, W, U, p, (tg, frames, tl) = self.transducer_band(enc_out, input_lengths, padded_target, target_lengths)
        e = F_.linear(enc_out, self.rnnt_enc.weight, self.rnnt_enc.bias, False, True)
        z = F_.RnntJointPrunedFn.apply(e, p, s_begin, W)
        logits = F_.linear(z, self.rnnt_out.weight, self.rnnt_out.bias, True, True)
        pruned = F_.RnntPrunedFn.apply(logits, tg, frames, tl, s_begin, U, constant.PAD_TOKEN)
        return pruned, simple

    def transducer_loss(self, enc_out, input_lengths, padded_target, target_lengths, simple_scale=0.5, stats=None):
        """The transducer loss of a batch, mean_b nll_b / max(U_b, 1) (F_.RnntFn), with T_b = ctc_frame_lengths.  Call it BEFORE the
        decoder runs: RnntFn claims the logit hand-over slot its own projection has just left, and the decoder's projection then
        leaves a fresh one for the cross-entropy.  A model built with prune_range S > 0: L_pruned + simple_scale * L_simple
        (transducer_pruned_loss); stats, when given, receives 'rnnt_simple' = L_simple and 'rnnt_pruned' = L_pruned."""
        if int(getattr(self, "rnnt_prune_range", 0)) > 0:
            pruned, simple = self.transducer_pruned_loss(enc_out, input_lengths, padded_target, target_lengths, simple_scale)
            if stats is not None:
                stats["rnnt_simple"], stats["rnnt_pruned"] = simple.detach(), pruned.detach()
            return pruned + float(simple_scale) * simple
        logits = self.transducer_logits(enc_out, padded_target, target_lengths)
        frames = torch.tensor(self.ctc_frame_lengths(input_lengths, enc_out.shape[1]), dtype=torch.int32)
        return F_.RnntFn.apply(logits, torch.as_tensor(padded_target), frames, torch.as_tensor(target_lengths), constant.PAD_TOKEN)

    def transducer_step(self, padded_input, input_lengths, padded_target, target_lengths, transducer_weight, smoothing, ctc_weight=0.0,
                        simple_scale=0.5):
        """One training step's loss with the transducer term (train.py --transducer-weight r)
        -> (L, gold, hyp_seq, stats): L = (1 - r) L_existing + r L_rnnt, L_existing = CE, or (1 - w) CE + w CTC with ctc_weight w > 0.
        stats: the device scalars 'ce', 'ctc' (zero without the head), 'rnnt' and 'rnnt_simple' (zero without --transducer-prune-range;
        with it L_rnnt = L_pruned + simple_scale L_simple and 'rnnt_pruned' is there too); no host synchronisation."""
        from utils.metrics import calculate_metrics
        r, w = float(transducer_weight), float(ctc_weight)
        if not 0.0 < r <= 1.0:
            raise ValueError("a transducer step needs --transducer-weight in (0, 1], got %g" % r)
        if not 0.0 <= w <= 1.0 or (w > 0.0 and not hasattr(self, "ctc_linear")):
            raise ValueError("--ctc-weight %g needs a value in [0, 1] and a model with an encoder CTC head" % w)
        self._need_transducer()
        feats = self._features(padded_input)
        enc_out, _ = self.encoder(feats, input_lengths)
        ctc = self.ctc_logits(enc_out) if w > 0.0 else None
        extra = {}
        rnnt = self.transducer_loss(enc_out, input_lengths, padded_target, target_lengths, simple_scale, extra)
        pred, gold, *_ = self.decoder(padded_target, enc_out, input_lengths)
        hyp_seq = ops.argmax_rows(pred.detach().reshape(-1, pred.shape[-1])).view(pred.shape[0], pred.shape[1])
        ce, _ = calculate_metrics(pred, gold, smoothing=smoothing, loss_type="ce", sync=False)
        stats = dict(ce=ce.detach(), ctc=ops.zero_scalar(pred.device).reshape(()), rnnt=rnnt.detach(),
                     rnnt_simple=ops.zero_scalar(pred.device).reshape(()))
        stats.update(extra)
        existing = ce
        if w > 0.0:
            frames = torch.tensor(self.ctc_frame_lengths(input_lengths, ctc.shape[1]), dtype=torch.int32)
            ctc_loss = F_.CTCFn.apply(ctc, torch.as_tensor(padded_target), frames, torch.as_tensor(target_lengths), constant.PAD_TOKEN)
            stats["ctc"] = ctc_loss.detach()
            existing = (1.0 - w) * ce + w * ctc_loss
        return (1.0 - r) * existing + r * rnnt, gold, hyp_seq, stats

    @torch.no_grad()
    def transducer_greedy(self, enc_out, lengths, max_symbols=5, return_ids=False):
        """Time-synchronous greedy search of the transducer head: at frame t of an utterance emit the joint's arg-max while it is not
        blank, at most max_symbols times, then go to frame t + 1; frames >= lengths[b] (true encoder frames, ctc_frame_lengths) are never
        visited.  All utterances advance together, each with its own frame pointer: T' * max_symbols steps of F_.linear / ops.rnnt_joint /
        ops.argmax_rows with torch.where on the device, no host synchronisation inside the loop and one device-to-host copy at the end.
        -> strings (return_ids: (strings, label ids)); the ids are labels as they stand: no SOS, no EOS."""
        self._need_transducer()
        S = int(max_symbols)
        if S < 1:
            raise ValueError("--transducer-max-symbols must be at least 1, got %d" % S)
        B, T = enc_out.shape[0], enc_out.shape[1]
        C, blank = len(self.rnnt_embed), constant.PAD_TOKEN
        dev = enc_out.device
        e = F_.linear(enc_out, self.rnnt_enc.weight, self.rnnt_enc.bias, False, True)
        J = e.shape[-1]
        frames = _lengths_to_device(lengths, dev).to(torch.int64).clamp(0, T)
        cap = T * S
        t_idx = torch.zeros(B, dtype=torch.int64, device=dev)
        syms = torch.zeros(B, dtype=torch.int64, device=dev)
        n_out = torch.zeros(B, dtype=torch.int64, device=dev)
        hist = torch.full((B, C), constant.SOS_TOKEN, dtype=torch.int64, device=dev)        # hist[:, k] = the label k places back
        out = torch.zeros((B, cap + 1), dtype=torch.int64, device=dev)                      # column `cap` takes the writes of idle rows
        trash = torch.full((B,), cap, dtype=torch.int64, device=dev)
        zero = torch.zeros(B, dtype=torch.int64, device=dev)
        for _ in range(cap):
            active = t_idx < frames
            e_t = e.gather(1, t_idx.clamp(max=T - 1).view(B, 1, 1).expand(B, 1, J))
            p = self._rnnt_predict([hist[:, k:k + 1] for k in range(C)])
            z = ops.rnnt_joint(e_t.contiguous(), p)
            logits = F_.linear(z.view(B, J), self.rnnt_out.weight, self.rnnt_out.bias, True, True)
            k = ops.argmax_rows(logits)
            emit = active & (k != blank)
            out.scatter_(1, torch.where(emit, n_out, trash).view(B, 1), k.view(B, 1))
            n_out = n_out + emit.to(torch.int64)
            hist = torch.where(emit.view(B, 1), torch.cat([k.view(B, 1), hist[:, :C - 1]], 1), hist)
            syms = torch.where(emit, syms + 1, zero)
            adv = active & (~emit | (syms >= S))
            t_idx = t_idx + adv.to(torch.int64)
            syms = torch.where(adv, zero, syms)
        flat = torch.cat([out[:, :cap].reshape(-1), n_out]).cpu()
        ids, n = flat[:B * cap].view(B, cap).tolist(), flat[B * cap:].tolist()
        hyp_ids = [row[:m] for row, m in zip(ids, n)]
        strs = ["".join(self.id2label[x] for x in row) for row in hyp_ids]
        return (strs, hyp_ids) if return_ids else strs

    @torch.no_grad()
    def transducer_beam_search(self, enc_out, lengths, beam_width, nbest=1, candidates=0, max_symbols=5, lm=None, lm_weight=0.1,
                               c_weight=1, return_ids=False, ngram=None, ngram_weight=0.0, length_bonus=0.0, context=None,
                               context_score=0.0):
        """Beam search over the transducer head (csrc/rnnt_beam.hip): ONE rnnt_enc launch, ONE search launch (one
        workgroup per utterance walks its frames: the joint, the vocabulary projection, the log-softmax rows, the candidates and the
        beam bookkeeping of every step are inside it) and one device-to-host copy.  lengths: true encoder frames per utterance
        (ctc_frame_lengths); beam_width W in 1..16 hypotheses, candidates K in 1..16 labels tried per hypothesis and step (0:
        min(V - 1, 16)), at most max_symbols labels per frame.  The kernel's W hypotheses of an utterance, {'yseq', 'score', 'rnnt_score'}
        with score = log-probability summed over the alignments found, are ranked like a decoder beam's and like ctc_beam_search's
        (asr_hip.search.rank_ended): score + sqrt(words) * c_weight, or with lm (utils.lstm_utils.LM) score + lm_weight * (lm - 2 * oov) +
        sqrt(words) * c_weight, all utterances' hypotheses in ONE batched LM call.  -> per utterance the min(nbest, found) best strings,
        best first (return_ids: (strings, label ids), same nesting); the ids are labels as they stand: no SOS, no EOS.
        ngram (utils.ngram.NgramLM over this model's labels) and / or context (utils.context.ContextGraph over them): first-pass fusion,
        as in ctc_beam_search and still ONE search launch.  The kernel prunes its candidates and every frame's beam by the transducer
        score + ngram_weight * the n-gram's log-probability of the labels + length_bonus * their number + context_score * the phrase
        credit (contexts open with SOS, the final order counts EOS and only earned credit), so a rare name survives the beam; the tables
        go to the device once.  Every hypothesis then carries 'rnnt_score', 'ngram_score' (with the EOS term; 0 without ngram) and, with
        context, 'context_credit', and score = rnnt_score + ngram_weight * ngram_score + length_bonus * labels + context_score *
        context_credit goes into the ranking above.  Both None: the plain search, unchanged."""
        self._need_transducer()
        a, beta, gamma = float(ngram_weight), float(length_bonus), float(context_score)
        if ngram is not None:
            ngram.check_labels(self.id2label)
        if context is not None:
            context.check_labels(self.id2label)
        W, S, K = int(beam_width), int(max_symbols), int(candidates)
        if not 1 <= W <= 16:
            raise ValueError("transducer_beam_search keeps beam_width hypotheses in the kernel's beam: 1..16, got %d" % W)
        if nbest < 1:
            raise ValueError("nbest must be at least 1, got %d" % nbest)
        if S < 1:
            raise ValueError("--transducer-max-symbols must be at least 1, got %d" % S)
        if not 0 <= K <= 16:
            raise ValueError("candidates must lie in 0..16 (0: min(V - 1, 16)), got %d" % K)
        B, T = enc_out.shape[0], enc_out.shape[1]
        e = F_.linear(enc_out, self.rnnt_enc.weight, self.rnnt_enc.bias, False, True)
        cd = e.dtype
        tables = [P.linear_weight(m.weight, cd) for m in self.rnnt_embed]       # what _rnnt_predict's rows round to; fp32: the masters
        fused = ngram is not None or context is not None
        kw = dict(ngram=ngram, alpha=a, beta=beta, bos=constant.SOS_TOKEN, eos=constant.EOS_TOKEN, context=context, gamma=gamma) if fused else {}
        out = ops.rnnt_beam_search(e.contiguous(), tables, P.linear_weight(self.rnnt_out.weight, cd), self.rnnt_out.bias.data,
                                   _lengths_to_device(lengths, e.device), W, K, S, W, constant.PAD_TOKEN, constant.SOS_TOKEN, **kw)
        ended = search.nbest_to_host(out, B, W, T * S, fused, context is not None)
        if fused:
            search.fuse_scores(ended, 'rnnt_score', a, beta, gamma)
        else:
            for hs in ended:
                for h in hs:
                    h['rnnt_score'] = h['score']
        return search.render_nbest(ended, nbest, c_weight, self.id2label, lm, lm_weight, return_ids)

    def forward(self, padded_input, input_lengths, padded_target, verbose=False, return_ctc=False):
        """-> (pred (B,Td,V) fp32, gold (B,Td), hyp_seq (B,Td), gold_seq)   (reference: transformer.py:59-85); with return_ctc also
        the CTC head's logits (B,T',V) fp32 on the encoder output."""
        feats = self._features(padded_input)
        enc_out, _ = self.encoder(feats, input_lengths)
        ctc = self.ctc_logits(enc_out) if return_ctc else None
        pred, gold, *_ = self.decoder(padded_target, enc_out, input_lengths)
        hyp_seq = ops.argmax_rows(pred.detach().reshape(-1, pred.shape[-1])).view(pred.shape[0], pred.shape[1])
        if return_ctc:
            return pred, gold, hyp_seq, gold, ctc
        return pred, gold, hyp_seq, gold

    # -------------------------------------------------------------------------------------------- MWER training
    def space_id(self):
        """The id of the space label (--mwer-unit word splits label sequences there); ValueError when the label file has none."""
        ids = [i for i, c in self.id2label.items() if c == " "]
        if not ids:
            raise ValueError("--mwer-unit word needs a space label to split words at, and the label file has none (use --mwer-unit label)")
        return int(ids[0])

    def mwer_errors(self, hyps, golds, unit="label"):
        """Levenshtein distances (raw counts) of every hypothesis to its utterance's gold label sequence, on the host
        (asr_hip.text.edit_distance_batch): unit 'label' over label ids, 'word' over the runs of ids between space labels.
        hyps: one list of id lists per utterance, golds: one id list per utterance -> the same nesting of ints."""
        if unit not in ("label", "word"):
            raise ValueError("--mwer-unit must be 'label' or 'word', got %r" % (unit,))
        if unit == "word":
            sp = self.space_id()

            def words(y):
                out, cur = [], []
                for t in y:
                    if t == sp:
                        if cur:
                            out.append(tuple(cur))
                        cur = []
                    else:
                        cur.append(t)
                return out + ([tuple(cur)] if cur else [])
        else:
            def words(y):
                return list(y)
        from asr_hip.text import edit_distance_batch
        dist = edit_distance_batch([(words(y), words(g)) for hs, g in zip(hyps, golds) for y in hs])
        out, at = [], 0
        for hs in hyps:
            out.append(dist[at:at + len(hs)])
            at += len(hs)
        return out

    def mwer_step(self, padded_input, input_lengths, padded_target, target_lengths, mwer_weight, ctc_weight, nbest=4, unit="label",
                  candidates=0, hyps=None):
        """One training step's loss with minimum word error rate training over the CTC n-best (train.py --mwer-weight, DESIGN.md
        section 7) -> (L, gold_seq (B, Lg), hyp_seq (B, Lg), stats).  With m = mwer_weight and w = ctc_weight,
            L = m * (1/B) sum_b risk_b + (1 - m) * [(1 - w) * NLL + w * CTC],      risk_b = sum_i P_i (e_i - mean_j e_j),
        P = softmax over the attention decoder's log p(y, EOS | x) of the utterance's n_b <= nbest distinct hypotheses, e_i their
        Levenshtein distance to the gold labels (mwer_errors), NLL = - sum_b log p(gold_b, EOS | x) / sum_b (len(gold_b) + 1) (no label
        smoothing), CTC the joint step's term (F_.CTCFn, true encoder frames).  The stages: features, encoder, CTC logits, the n-best =
        the nbest survivors of ops.ctc_beam_search on the detached CTC logits of this very pass (under no_grad, in the kernel's own order:
        no word bonus, no LM), their errors on the host, ONE decoder pass over gold and hypotheses together (Decoder._score_rows: every
        parameter is used once per backward), ops.mwer_loss.  padded_target (B, L) / target_lengths: the collated raw label ids (host
        or device).  hyps: the hypotheses to use instead of the search's (tests).  gold_seq / hyp_seq: the gold targets (EOS included)
        and the arg-max of the gold rows' logits, PAD behind them, for the trainer's metrics.  stats: 'risk' (B,), 'prob' (R,), 'sums'
        (2,) device tensors of ops.mwer_loss, 'nll' / 'ctc' device scalars, and on the host 'hyps', 'errors', 'expected_base' (the mean
        over utterances of mean_j e_j: the mean expected error is sum(risk) / B + expected_base) and 'top_error' (mean e of the first
        hypothesis)."""
        m, w, N = float(mwer_weight), float(ctc_weight), int(nbest)
        if not 0.0 < m <= 1.0:
            raise ValueError("--mwer-weight must lie in (0, 1] for an MWER step, got %g" % m)
        if not 2 <= N <= ops.MWER_NBEST_MAX:
            raise ValueError("--mwer-nbest %d: the n-best of an MWER step holds 2..%d hypotheses (the CTC prefix beam search's beam)"
                             % (N, ops.MWER_NBEST_MAX))
        if not 0.0 < w <= 1.0 or not hasattr(self, "ctc_linear"):
            raise ValueError("--mwer-weight %g needs --ctc-weight > 0 and a model with an encoder CTC head: the n-best comes from the "
                             "CTC prefix beam search" % m)
        if unit == "word":
            self.space_id()                            # refuse before any device work
        feats = self._features(padded_input)
        enc_out, _ = self.encoder(feats, input_lengths)
        ctc = self.ctc_logits(enc_out)                 # (before the decoder: the logit hand-over slot belongs to the projection that runs last)
        B, T, V = ctc.shape
        dev = ctc.device
        frames = self.ctc_frame_lengths(input_lengths, T)
        tl = [int(x) for x in torch.as_tensor(target_lengths).tolist()]
        tgt_host = torch.as_tensor(padded_target).cpu().tolist()
        golds = [[int(t) for t in row[:n]] for row, n in zip(tgt_host, tl)]
        if hyps is None:
            with torch.no_grad():
                out = ops.ctc_beam_search(ctc.detach(), _lengths_to_device(frames, dev), N, candidates, N, constant.PAD_TOKEN)
                flat = torch.cat([out["ids"].reshape(-1), out["lengths"].reshape(-1)]).cpu()       # one device-to-host copy
            ids, lens = torch.split(flat, [B * N * T, B * N])
            ids, lens = ids.view(B, N, T).tolist(), lens.view(B, N).tolist()
            hyps = [[ids[b][n][:lens[b][n]] for n in range(N) if lens[b][n] >= 0] for b in range(B)]
        else:
            hyps = [[[int(t) for t in y] for y in hs] for hs in hyps]
            if len(hyps) != B or any(len(hs) > ops.MWER_NBEST_MAX for hs in hyps):
                raise ValueError("mwer_step: hyps needs one list of at most %d hypotheses per utterance" % ops.MWER_NBEST_MAX)
        errors = self.mwer_errors(hyps, golds, unit)
        dec = self.decoder
        rows = sum(len(y) + 1 for g, hs in zip(golds, hyps) for y in [g] + hs)
        if rows * 4 * dec.num_trg_vocab > dec.RESCORE_LOGIT_BYTES:
            raise ValueError("the MWER step scores %d decoder rows (%d utterances, gold + up to %d hypotheses each): %d bytes of fp32 logits "
                             "over %d labels, above the %d-byte cap of one pass (Decoder.RESCORE_LOGIT_BYTES); a training step is not "
                             "run in chunks -- lower --batch-size or --mwer-nbest"
                             % (rows, B, N, rows * 4 * dec.num_trg_vocab, dec.num_trg_vocab, dec.RESCORE_LOGIT_BYTES))
        limit = dec.positional_encoding.pe.shape[1] - 1
        longest = max(len(y) for g, hs in zip(golds, hyps) for y in [g] + hs)
        if longest > limit:
            raise ValueError("the MWER step: a sequence has %d labels, the decoder's positional encoding reaches %d" % (longest, limit))
        scored, seg_off, logits, _ = dec._score_rows(enc_out, [[g] + hs for g, hs in zip(golds, hyps)], differentiable=True)
        utt_off, err = [0], []
        for hs, es in zip(hyps, errors):
            utt_off.append(utt_off[-1] + 1 + len(hs))
            err += [0.0] + [float(e) for e in es]
        ntok = sum(len(g) + 1 for g in golds)
        Lg = max(len(g) for g in golds) + 1
        M = seg_off[-1]
        pos = [[seg_off[utt_off[b]] + j if j <= len(golds[b]) else M for j in range(Lg)] for b in range(B)]      # M: the PAD behind the rows
        gold_rows = [g + [constant.EOS_TOKEN] + [constant.PAD_TOKEN] * (Lg - 1 - len(g)) for g in golds]
        packed = torch.tensor([t for row in pos for t in row] + [t for row in gold_rows for t in row], dtype=torch.int64).to(dev, non_blocking=True)
        pos_d, gold_seq = packed[:B * Lg].view(B, Lg), packed[B * Lg:].view(B, Lg)
        err_d = torch.tensor(err, dtype=torch.float32).to(dev, non_blocking=True)
        utt_d = torch.tensor(utt_off, dtype=torch.int32).to(dev, non_blocking=True)
        part, prob, risk, sums = F_.MwerLossFn.apply(scored["score"], err_d, utt_d, m / B, (1.0 - m) * (1.0 - w) / ntok)
        ctc_loss = F_.CTCFn.apply(ctc, torch.as_tensor(padded_target), torch.tensor(frames, dtype=torch.int32), torch.as_tensor(target_lengths),
                                  constant.PAD_TOKEN)
        loss = part + ((1.0 - m) * w) * ctc_loss
        with torch.no_grad():
            am = ops.argmax_rows(logits.detach())
            hyp_seq = torch.cat([am, am.new_full((1,), constant.PAD_TOKEN)])[pos_d]
        ranked = [es for es in errors if es]
        stats = dict(risk=risk, prob=prob, sums=sums, nll=sums[1].detach() * (-1.0 / ntok), ctc=ctc_loss.detach(), hyps=hyps, errors=errors,
                     expected_base=sum(sum(es) / len(es) for es in ranked) / B,
                     top_error=sum(es[0] for es in ranked) / max(1, len(ranked)))
        return loss, gold_seq, hyp_seq, stats

    # -------------------------------------------------------------------------------------------- knowledge distillation
    def distill_step(self, padded_input, input_lengths, padded_target, target_lengths, teacher, distill_weight, temperature, smoothing,
                     ctc_weight=0.0, distill_ctc_weight=0.0):
        """One training step's loss with knowledge distillation from `teacher` (train.py --distill-from)
        -> (L, gold, hyp_seq, stats).  With a = distill_weight, c = distill_ctc_weight, w = ctc_weight, tau = temperature, n live decoder
        rows and F = sum_b T'_b live CTC frames (ctc_frame_lengths):
            L_att = (1 - a) CE + a KD,     KD = (1/n) sum_m tau^2 KL(softmax(teacher_m / tau) || softmax(student_m / tau)),
            w = 0:  L = L_att;     w > 0:  L = (1 - w) L_att + w [(1 - c) CTC + c KDF],     KDF = (1/F) sum_{t < T'_b} kd over the CTC heads.
        The teacher runs forward(..., return_ctc = c > 0) under no_grad in eval mode on the very batch the student sees (already
        augmented), and it runs FIRST: every vocabulary projection empties the logit hand-over slot, and the slot must hold the student's
        when F_.DistillFn claims it.  L_att is one DistillFn call on the decoder logits (CE and KD gradients leave in one launch); KDF is a
        second one without the CE term, on a gold tensor that is PAD on dead frames, and autograd adds its fp32 gradient to F_.CTCFn's.
        stats: the device scalars 'ce', 'kd', 'ctc', 'kdf' (zeros where a term does not exist); no host synchronisation."""
        a, c, w, tau = float(distill_weight), float(distill_ctc_weight), float(ctc_weight), float(temperature)
        if not (0.0 <= a <= 1.0 and 0.0 <= c <= 1.0) or (a == 0.0 and c == 0.0):
            raise ValueError("a distillation step needs --distill-weight or --distill-ctc-weight in (0, 1], got %g and %g" % (a, c))
        if not 0.5 <= tau <= 16.0:
            raise ValueError("--distill-temperature must lie in [0.5, 16], got %g" % tau)
        if c > 0.0:
            if not 0.0 < w <= 1.0 or not hasattr(self, "ctc_linear"):
                raise ValueError("--distill-ctc-weight %g needs --ctc-weight > 0 and a student with an encoder CTC head" % c)
            if not hasattr(teacher, "ctc_linear"):
                raise ValueError("--distill-ctc-weight %g: the teacher has no encoder CTC head (ctc_linear), the student has one" % c)
            if teacher.feat_extractor != self.feat_extractor:
                raise ValueError("--distill-ctc-weight %g: the teacher's feat_extractor %s and the student's %s give different frame "
                                 "counts" % (c, teacher.feat_extractor, self.feat_extractor))
        if teacher.training:
            teacher.eval()
        with torch.no_grad():
            t_out = teacher(padded_input, input_lengths, padded_target, return_ctc=c > 0.0)
        s_out = self.forward(padded_input, input_lengths, padded_target, return_ctc=w > 0.0)
        pred, gold, hyp_seq = s_out[0], s_out[1], s_out[2]
        if t_out[0].shape != pred.shape:
            raise ValueError("the teacher's decoder logits %s and the student's %s differ in shape: distillation needs the same labels "
                             "and target positions" % (tuple(t_out[0].shape), tuple(pred.shape)))
        PAD = constant.PAD_TOKEN
        l_att, sums, _ = F_.DistillFn.apply(pred, t_out[0], gold, float(smoothing), PAD, tau, 1.0 - a, a, True)
        zero = ops.zero_scalar(pred.device).reshape(())
        stats = dict(ce=sums[0] / sums[1], kd=sums[3] / sums[1], ctc=zero, kdf=zero)
        if not w > 0.0:
            return l_att, gold, hyp_seq, stats
        ctc = s_out[4]
        frames = self.ctc_frame_lengths(input_lengths, ctc.shape[1])
        ctc_loss = F_.CTCFn.apply(ctc, torch.as_tensor(padded_target), torch.tensor(frames, dtype=torch.int32), torch.as_tensor(target_lengths),
                                  PAD)
        stats["ctc"] = ctc_loss.detach()
        ctc_term = ctc_loss
        if c > 0.0:
            if t_out[4].shape != ctc.shape:
                raise ValueError("the teacher's CTC logits %s and the student's %s differ in shape" % (tuple(t_out[4].shape), tuple(ctc.shape)))
            live = torch.arange(ctc.shape[1], device=ctc.device)[None, :] < _lengths_to_device(frames, ctc.device)[:, None]
            gold_f = live.to(torch.int64) * (PAD + 1) + (~live).to(torch.int64) * PAD        # any non-PAD value marks a live frame
            kdf, _, _ = F_.DistillFn.apply(ctc, t_out[4], gold_f, 0.0, PAD, tau, 0.0, 1.0, False)
            stats["kdf"] = kdf.detach()
            ctc_term = (1.0 - c) * ctc_loss + c * kdf
        return (1.0 - w) * l_att + w * ctc_term, gold, hyp_seq, stats

    def evaluate(self, padded_input, input_lengths, padded_target, beam_search=False, beam_width=0, beam_nbest=0, lm=None,
                 lm_rescoring=False, lm_weight=0.1, c_weight=1, verbose=False, ctc_logits=None, ctc_lengths=None, ctc_weight=0.0,
                 ctc_candidates=0, ctc_greedy=False, align_source=None, target_lengths=None, ctc_beam=False,
                 attention_rescoring_weight=0.0, ngram=None, ngram_weight=0.0, length_bonus=0.0, context=None, context_score=0.0,
                 transducer_greedy=False, transducer_max_symbols=5, transducer_beam=False, transducer_candidates=0,
                 transducer_ngram=None, transducer_ngram_weight=0.0, transducer_length_bonus=0.0, transducer_context=None,
                 transducer_context_score=0.0):
        """-> (_, strs_hyps, strs_gold)   (reference: transformer.py:87-124).  ctc_weight > 0 (beam search only): joint CTC / attention
        scoring with the encoder CTC head (ctc_logits / ctc_lengths default to the head's logits and the true encoder frames);
        ctc_greedy: best-path decoding from the head alone; ctc_beam: prefix beam search over the head's posteriors alone
        (ctc_beam_search: beam_width prefixes, ctc_candidates labels per frame, the beam_nbest best re-ranked with lm when lm_rescoring),
        not together with beam_search, ctc_greedy or ctc_weight; attention_rescoring_weight = lambda in (0, 1] (ctc_beam only): all
        beam_width hypotheses are rescored by the decoder in one teacher-forced pass and ranked by (1 - lambda) * CTC + lambda * attention
        log-probability (ctc_beam_search's rescoring_weight); ngram / ngram_weight / length_bonus (ctc_beam only): a label n-gram LM fused
        into that search's pruning, context / context_score (ctc_beam only): a phrase list biasing it (ctc_beam_search's arguments of the
        same names).  align_source "gold" / "hyp": a fourth value, the forced alignment
        (ctc_align) of padded_target with target_lengths, or of the label ids the decoder produced (SOS and EOS dropped; never a
        re-tokenised string).  transducer_greedy: time-synchronous greedy search of the transducer head (transducer_greedy, at most
        transducer_max_symbols labels per frame), not together with any other decoding mode or with align_source.  transducer_beam: beam
        search over the transducer head (transducer_beam_search: beam_width hypotheses, transducer_candidates labels per hypothesis and
        step, transducer_max_symbols per frame, the beam_nbest best re-ranked with lm when lm_rescoring), under the same exclusions.
        transducer_ngram / transducer_ngram_weight / transducer_length_bonus and transducer_context / transducer_context_score
        (transducer_beam only; an error before any launch otherwise): the n-gram LM and the phrase list fused into THAT search's pruning
        (transducer_beam_search's ngram / ngram_weight / length_bonus / context / context_score); ngram and context stay ctc_beam's."""
        if transducer_ngram is not None and not transducer_beam:
            raise ValueError("--transducer-ngram-path needs --transducer-beam-search: the n-gram LM is fused into the transducer beam search")
        if transducer_context is not None and not transducer_beam:
            raise ValueError("--transducer-context-path needs --transducer-beam-search: the phrase list biases the transducer beam "
                             "search's pruning")
        if transducer_beam:
            if transducer_greedy or beam_search or ctc_greedy or ctc_beam or ctc_weight > 0 or attention_rescoring_weight > 0 \
                    or align_source is not None or ngram is not None or context is not None:
                raise ValueError("--transducer-beam-search decodes from the transducer head alone: not together with --transducer-greedy, "
                                 "--beam-search, --ctc-greedy, --ctc-beam-search, --ctc-decode-weight, --attention-rescoring-weight, "
                                 "--ngram-path, --context-path or --align")
            self._need_transducer()                    # the "no transducer head" ValueError, before any device work
            if int(transducer_max_symbols) < 1:
                raise ValueError("--transducer-max-symbols must be at least 1, got %d" % int(transducer_max_symbols))
            if not 1 <= int(beam_width) <= 16:
                raise ValueError("--transducer-beam-search keeps --beam-width hypotheses in the kernel's beam: 1..16, got %d"
                                 % int(beam_width))
            if lm_rescoring and lm is None:
                raise ValueError("lm_rescoring=True needs lm (utils.lstm_utils.LM)")
            if transducer_ngram is not None:
                transducer_ngram.check_labels(self.id2label)
            if transducer_context is not None:
                transducer_context.check_labels(self.id2label)
        if transducer_greedy:
            if beam_search or ctc_greedy or ctc_beam or ctc_weight > 0 or attention_rescoring_weight > 0 or align_source is not None \
                    or ngram is not None or context is not None:
                raise ValueError("--transducer-greedy decodes from the transducer head alone: not together with --beam-search, "
                                 "--ctc-greedy, --ctc-beam-search, --ctc-decode-weight, --attention-rescoring-weight, --ngram-path, "
                                 "--context-path or --align")
            self._need_transducer()                    # the "no transducer head" ValueError, before any device work
            if int(transducer_max_symbols) < 1:
                raise ValueError("--transducer-max-symbols must be at least 1, got %d" % int(transducer_max_symbols))
        if ctc_weight > 0 and not beam_search:
            raise ValueError("--ctc-decode-weight %g needs --beam-search: CTC prefix scores re-rank beam candidates" % ctc_weight)
        if ctc_beam and (beam_search or ctc_greedy or ctc_weight > 0):
            raise ValueError("ctc_beam decodes from the CTC head alone: not together with beam_search, ctc_greedy or ctc_weight")
        if not 0.0 <= attention_rescoring_weight <= 1.0:
            raise ValueError("--attention-rescoring-weight must lie in [0, 1], got %g" % attention_rescoring_weight)
        if attention_rescoring_weight > 0 and not ctc_beam:
            raise ValueError("--attention-rescoring-weight %g needs --ctc-beam-search: the decoder rescores the CTC search's n-best"
                             % attention_rescoring_weight)
        if ngram is not None and not ctc_beam:
            raise ValueError("--ngram-path needs --ctc-beam-search: the n-gram LM is fused into the CTC prefix beam search")
        if context is not None and not ctc_beam:
            raise ValueError("--context-path needs --ctc-beam-search: the phrase list biases the CTC prefix beam search's pruning")
        if ctc_beam and not hasattr(self, "ctc_linear"):
            self.ctc_logits(None)                      # the "no encoder CTC head" ValueError, before any device work
        if lm_rescoring and ctc_beam and lm is None:
            raise ValueError("lm_rescoring=True needs lm (utils.lstm_utils.LM)")
        if align_source not in (None, "gold", "hyp"):
            raise ValueError("align_source must be 'gold' or 'hyp', got %r" % (align_source,))
        if align_source is not None and not hasattr(self, "ctc_linear"):
            self.ctc_logits(None)                      # the "no encoder CTC head" ValueError, before any device work
        if align_source == "gold" and target_lengths is None:
            raise ValueError("align_source='gold' needs target_lengths (the true lengths of padded_target)")
        feats = self._features(padded_input)
        enc_out, _ = self.encoder(feats, input_lengths)
        _, gold, *_ = self.decoder(padded_target, enc_out, input_lengths)
        gold_cpu = gold.cpu().tolist()
        strs_gold = ["".join(self.id2label[int(x)] for x in row) for row in gold_cpu]
        if ctc_weight > 0 or ctc_greedy or ctc_beam or align_source is not None:
            if ctc_lengths is None:
                ctc_lengths = self.ctc_frame_lengths(input_lengths, enc_out.shape[1])
            if ctc_logits is None and ctc_weight > 0 and not ctc_greedy:
                with torch.no_grad():
                    ctc_logits = self.ctc_logits(enc_out)
        if transducer_beam:
            nbest_strs = self.transducer_beam_search(enc_out, self.ctc_frame_lengths(input_lengths, enc_out.shape[1]), beam_width,
                                                     nbest=max(1, int(beam_nbest)), candidates=transducer_candidates,
                                                     max_symbols=int(transducer_max_symbols), lm=lm if lm_rescoring else None,
                                                     lm_weight=lm_weight, c_weight=c_weight, ngram=transducer_ngram,
                                                     ngram_weight=transducer_ngram_weight, length_bonus=transducer_length_bonus,
                                                     context=transducer_context, context_score=transducer_context_score)
            strs_hyps = [rows[0] if rows else "" for rows in nbest_strs]
        elif transducer_greedy:
            strs_hyps = self.transducer_greedy(enc_out, self.ctc_frame_lengths(input_lengths, enc_out.shape[1]),
                                               max_symbols=int(transducer_max_symbols))
        elif ctc_greedy:
            strs_hyps, hyp_ids = self.ctc_greedy(enc_out, ctc_lengths, return_ids=True)
        elif ctc_beam:
            nbest_strs, nbest_ids = self.ctc_beam_search(enc_out, ctc_lengths, beam_width, nbest=max(1, int(beam_nbest)),
                                                         candidates=ctc_candidates, lm=lm if lm_rescoring else None,
                                                         lm_weight=lm_weight, c_weight=c_weight, return_ids=True,
                                                         rescoring_weight=attention_rescoring_weight, ngram=ngram,
                                                         ngram_weight=ngram_weight, length_bonus=length_bonus, context=context,
                                                         context_score=context_score)
            strs_hyps, hyp_ids = [rows[0] if rows else "" for rows in nbest_strs], [rows[0] if rows else [] for rows in nbest_ids]
        elif beam_search:
            hyp_ids, strs_hyps = self.decoder.beam_search(enc_out, beam_width=beam_width, nbest=1, lm=lm, lm_rescoring=lm_rescoring,
                                                          lm_weight=lm_weight, c_weight=c_weight, ctc_logits=ctc_logits,
                                                          ctc_lengths=ctc_lengths, ctc_weight=ctc_weight, ctc_candidates=ctc_candidates)
            if len(strs_hyps) != padded_input.shape[0]:
                strs_hyps, hyp_ids = self.decoder.greedy_search(enc_out, return_ids=True)
        elif align_source == "hyp":
            strs_hyps, hyp_ids = self.decoder.greedy_search(enc_out, return_ids=True)
        else:
            strs_hyps = self.decoder.greedy_search(enc_out)
        if verbose:
            print("GOLD", strs_gold)
            print("HYP", strs_hyps)
        if align_source is None:
            return _, strs_hyps, strs_gold
        if align_source == "gold":
            alignment = self.ctc_align(enc_out, ctc_lengths, padded_target, target_lengths)
        else:
            # (the ids of --ctc-greedy and --ctc-beam-search are CTC labels as they stand, feasible by construction; a decoder's carry SOS / EOS)
            alignment = self.ctc_align(enc_out, ctc_lengths,
                                       hyp_ids if ctc_greedy or ctc_beam else [hypothesis_labels(row) for row in hyp_ids])
        return _, strs_hyps, strs_gold, alignment


class Encoder(nn.Module):
    """Encoder(num_layers, num_heads, dim_model, dim_key, dim_value, dim_input, dim_inner, dropout=0.1,
    src_max_length=2500)   (reference: transformer.py:126-180); conv_module_kernel K > 0 (--conv-module-kernel) gives every layer a
    ConvolutionModule between its attention and feed-forward sub-layers; pos_encoding "rope" (--pos-encoding) rotates Q and K of every
    layer's self-attention by the frame's position (asr_hip.ops.rope_) and leaves the absolute sinusoid out."""

    def __init__(self, num_layers, num_heads, dim_model, dim_key, dim_value, dim_input, dim_inner, dropout=0.1,
                 src_max_length=2500, rank=0, conv_module_kernel=0, pos_encoding="abs"):
        super().__init__()
        self.conv_module_kernel = check_conv_module_kernel(conv_module_kernel, dim_model, rank)
        self.pos_encoding = check_pos_encoding(pos_encoding, dim_key, dim_value, rank)
        self.dim_input, self.num_layers, self.num_heads = dim_input, num_layers, num_heads
        self.dim_model, self.dim_key, self.dim_value, self.dim_inner = dim_model, dim_key, dim_value, dim_inner
        self.src_max_length = src_max_length
        self.dropout = nn.Dropout(dropout)          # never applied (as in the reference, transformer.py:145)
        self.dropout_rate = dropout
        self.input_linear = nn.Linear(dim_input, dim_model)
        self.layer_norm_input = nn.LayerNorm(dim_model)
        self.positional_encoding = PositionalEncoding(dim_model, src_max_length)
        self.layers = nn.ModuleList([EncoderLayer(num_heads, dim_model, dim_inner, dim_key, dim_value, dropout=dropout, rank=rank,
                                                  conv_module_kernel=self.conv_module_kernel) for _ in range(num_layers)])
        if self.pos_encoding == "rope":
            # not persistent: state_dict has the same keys in both modes (positional_encoding.pe stays in the checkpoint, unused)
            self.register_buffer("rope_cs", ops.rope_table(src_max_length, dim_key), persistent=False)

    def forward(self, padded_input, input_lengths, need_attn=False):
        """padded_input (B,T,D_in), input_lengths (B) -> (output (B,T,D), [self_attn per layer])"""
        B, T, _ = padded_input.shape
        dev = padded_input.device
        rope = None
        if self.pos_encoding == "rope":          # one table row per frame, the same rows for every layer
            if T > self.src_max_length:
                raise ValueError("%d encoder frames, but the rotary table has --src-max-len %d rows" % (T, self.src_max_length))
            rope = self.rope_cs[:T]
        lens = _lengths_to_device(input_lengths, dev)
        # row_keep[b,t] = t < len[b]   (reference: common_layers.py:33-38 via transformer.py:168)
        row_keep = ops.length_mask(lens, T)
        x = F_.EncInFn.apply(padded_input, self.input_linear.weight, self.input_linear.bias, self.layer_norm_input.weight,
                             self.layer_norm_input.bias, None if rope is not None else self.positional_encoding.pe[0])
        attns = []
        for layer in self.layers:
            x, a = layer(x, row_keep=row_keep, key_len=lens, need_attn=need_attn, rope=rope)
            attns.append(a)
        return x, attns


class EncoderLayer(nn.Module):
    """EncoderLayer(num_heads, dim_model, dim_inner, dim_key, dim_value, dropout=0.1)   (reference: transformer.py:183-203)"""

    def __init__(self, num_heads, dim_model, dim_inner, dim_key, dim_value, dropout=0.1, rank=0, conv_module_kernel=0):
        super().__init__()
        conv_module_kernel = check_conv_module_kernel(conv_module_kernel, dim_model, rank)
        if rank > 0:          # Low-Rank Transformer (BASELINE configs[4]): every projection is V (out,r) . U (r,in)
            self.self_attn = LowRankMultiHeadAttention(num_heads, dim_model, dim_key, dim_value, rank, dropout=dropout)
            self.pos_ffn = LowRankPositionwiseFeedForward(dim_model, dim_inner, rank, dropout=dropout)
            return
        self.self_attn = MultiHeadAttention(num_heads, dim_model, dim_key, dim_value, dropout=dropout)
        if conv_module_kernel:          # (registered between the two so that state_dict lists the sub-layers in the order they run)
            self.conv_module = ConvolutionModule(dim_model, conv_module_kernel, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForwardWithConv(dim_model, dim_inner, dropout=dropout)

    def forward(self, enc_input, non_pad_mask=None, self_attn_mask=None, row_keep=None, key_len=None, need_attn=False, rope=None):
        if row_keep is None and non_pad_mask is not None:      # reference-style call with materialised masks
            row_keep = non_pad_mask.reshape(-1).ne(0).to(torch.uint8)
        kw = {} if rope is None else {"rope": rope}          # (the Low-Rank attention takes no such argument: Encoder refuses rope with --rank)
        out, attn = self.self_attn(enc_input, enc_input, enc_input, mask=self_attn_mask, key_len=key_len, row_keep=row_keep,
                                   need_attn=need_attn, **kw)
        if hasattr(self, "conv_module"):
            out = self.conv_module(out, key_len=key_len, row_keep=row_keep)
        out = self.pos_ffn(out, row_keep=row_keep)
        return out, attn


class Decoder(nn.Module):
    """Decoder(id2label, num_src_vocab, num_trg_vocab, num_layers, num_heads, dim_emb, dim_model, dim_inner, dim_key,
    dim_value, dropout=0.1, trg_max_length=1000, emb_trg_sharing=False)   (reference: transformer.py:206-305)"""

    def __init__(self, id2label, num_src_vocab, num_trg_vocab, num_layers, num_heads, dim_emb, dim_model, dim_inner, dim_key,
                 dim_value, dropout=0.1, trg_max_length=1000, emb_trg_sharing=False, rank=0):
        super().__init__()
        self.sos_id, self.eos_id = constant.SOS_TOKEN, constant.EOS_TOKEN
        self.id2label = id2label
        self.num_src_vocab, self.num_trg_vocab = num_src_vocab, num_trg_vocab
        self.num_layers, self.num_heads = num_layers, num_heads
        self.dim_emb, self.dim_model, self.dim_inner = dim_emb, dim_model, dim_inner
        self.dim_key, self.dim_value = dim_key, dim_value
        self.dropout_rate, self.emb_trg_sharing, self.trg_max_length = dropout, emb_trg_sharing, trg_max_length
        self.trg_embedding = nn.Embedding(num_trg_vocab, dim_emb, padding_idx=constant.PAD_TOKEN)
        self.positional_encoding = PositionalEncoding(dim_model, max_length=trg_max_length)
        self.dropout = nn.Dropout(dropout)
        self.layers = nn.ModuleList([DecoderLayer(dim_model, dim_inner, num_heads, dim_key, dim_value, dropout=dropout, rank=rank)
                                     for _ in range(num_layers)])
        self.output_linear = nn.Linear(dim_model, num_trg_vocab, bias=False)
        nn.init.xavier_normal_(self.output_linear.weight)
        # hint for the flat-parameter layout (utils/optimizer.py:_slot_order): every layer's cross-attention K / V projection reads the
        # SAME encoder output (reference: transformer.py:296-299, 533-537), so adjacent weights make them one GEMM (forward below)
        if rank == 0:
            for li, layer in enumerate(self.layers):
                ea = layer.encoder_attn
                ea.key_linear.weight._asr_cross_kv = ("w", 2 * li)
                ea.value_linear.weight._asr_cross_kv = ("w", 2 * li + 1)
                ea.key_linear.bias._asr_cross_kv = ("b", 2 * li)
                ea.value_linear.bias._asr_cross_kv = ("b", 2 * li + 1)
        if emb_trg_sharing:
            self.output_linear.weight = self.trg_embedding.weight
            self.x_logit_scale = dim_model ** -0.5
        else:
            self.x_logit_scale = 1.0

    def preprocess(self, padded_input):
        """(B,L) -> seq_in_pad, seq_out_pad (B,Td)   (reference: transformer.py:254-266); Td = --tgt-max-len."""
        Td = constant.args.tgt_max_len
        seq_in, seq_out, key_pad, row_keep, overflow = ops.decoder_preprocess(padded_input, Td)
        if padded_input.shape[1] + 1 > Td and int(overflow.item()) != 0:
            raise RuntimeError("a target needs more than --tgt-max-len=%d positions (reference pad_list would fail, "
                               "common_layers.py:21)" % Td)
        self._masks = (key_pad, row_keep)
        return seq_in, seq_out

    def forward(self, padded_input, encoder_padded_outputs, encoder_input_lengths, need_attn=False):
        """-> (pred (B,Td,V) fp32, gold (B,Td), [self_attn], [enc_attn])   (reference: transformer.py:268-305)"""
        seq_in, seq_out = self.preprocess(padded_input)
        key_pad, row_keep = self._masks
        row_keep = row_keep.reshape(-1)
        dev = seq_in.device
        enc_len = _lengths_to_device(encoder_input_lengths, dev)
        tied = self.emb_trg_sharing
        p = self.dropout.p if self.training else 0.0
        x = F_.EmbedFn.apply(seq_in, self.trg_embedding.weight, self.positional_encoding.pe[0], self.x_logit_scale, p,
                             constant.PAD_TOKEN, True)
        self_attns, enc_attns = [], []
        # the cross-attention K | V projections of every layer as ONE GEMM on the encoder output (and one data-gradient GEMM, one weight-gradient
        # problem in backward) where the flat parameter layout has their weights adjacent; else one gradient buffer for the encoder output
        # that the layers' cross-attention backward GEMMs accumulate into
        box = None
        kv_pre = F_.cross_kv_all(encoder_padded_outputs, self.layers) if len(self.layers) > 1 else None
        enc_views = [encoder_padded_outputs] * len(self.layers)
        if kv_pre is None and torch.is_grad_enabled() and encoder_padded_outputs.requires_grad and len(self.layers) > 1:
            box = {}
            enc_views = F_.FanOutFn.apply(encoder_padded_outputs, len(self.layers), box)
        for li, layer in enumerate(self.layers):
            x, sa, ea = layer(x, enc_views[li], row_keep=row_keep, self_key_pad=key_pad, enc_key_len=enc_len,
                              need_attn=need_attn, kv_grad_box=box, kv_pre=None if kv_pre is None else (kv_pre[0][li], kv_pre[1], li))
            self_attns.append(sa)
            enc_attns.append(ea)
        # with --emb_trg_sharing the embedding backward (which runs last) reports the shared weight as ready
        pred = F_.linear(x, self.output_linear.weight, None, True, not tied)
        return pred, seq_out, self_attns, enc_attns

    def post_process_hyp(self, hyp):
        return "".join(self.id2label[int(x)] for x in hyp['yseq'][1:])

    # ---- decoding: KV-cached by default, the reference's full re-run kept for equivalence tests ----
    def _step_logits(self, ys, encoder_padded_outputs):
        """Teacher-forced decoder pass over the prefix `ys` (B,t) with the reference's decode-time masks: causal only,
        no encoder-length mask (reference: transformer.py:336-350, dec_enc_attn_mask=None)."""
        p = self.dropout.p if self.training else 0.0
        x = F_.EmbedFn.apply(ys, self.trg_embedding.weight, self.positional_encoding.pe[0], self.x_logit_scale, p,
                             constant.PAD_TOKEN, True)
        for layer in self.layers:
            x, _, _ = layer(x, encoder_padded_outputs, causal_only=True)
        return F_.linear(x, self.output_linear.weight, None, True, False)

    RESCORE_LOGIT_BYTES = 512 << 20          # fp32 logits of one score_hypotheses pass; a larger batch runs in chunks of whole utterances

    @torch.no_grad()
    def score_hypotheses(self, encoder_padded_outputs, hyps, return_tokens=False):
        """Attention rescoring: log p(y_1..y_n, EOS | encoder output) under this decoder for every label sequence of
        `hyps` (one list per utterance of label-id lists: CTC labels as they stand, no SOS, no EOS, possibly empty), in ONE teacher-forced
        pass: input [SOS] + y, targets y + [EOS], n + 1 rows per hypothesis; the empty hypothesis scores log p(EOS | SOS).  Masks as in
        _step_logits (causal only, no encoder-length mask): the quantity the attention beam search accumulates.  -> the same nesting of
        floats (return_tokens: (scores, the n + 1 per-token terms)).

        The W hypotheses of an utterance (fewer: padded with empty dummies) are a (B W, L, D) batch for self-attention and the SAME rows
        viewed (B, W L, D) for cross-attention -- its queries do not interact, so the K | V projection of the encoder output runs on B
        utterances, not B W copies.  Only the sum(n + 1) scored rows reach the vocabulary projection, and csrc/seq_logprob.hip turns their
        logits into per-token and per-hypothesis log-probabilities.  Through the layer modules: low-rank and dim_key != dim_value models
        work; the KV-cache kernels are not used."""
        B = encoder_padded_outputs.size(0)
        if len(hyps) != B:
            raise ValueError("score_hypotheses needs one list of hypotheses per utterance: %d lists for %d utterances" % (len(hyps), B))
        hyps = [[[int(t) for t in y] for y in hs] for hs in hyps]
        limit = self.positional_encoding.pe.shape[1] - 1
        longest = max([len(y) for hs in hyps for y in hs] + [0])
        if longest > limit:
            raise ValueError("score_hypotheses: a hypothesis has %d labels, the decoder's positional encoding reaches %d (trg_max_length "
                             "%d minus the SOS position)" % (longest, limit, limit + 1))
        row_bytes = 4 * self.num_trg_vocab
        scores, tokens = [], []
        b0 = 0
        while b0 < B:                                  # whole utterances while their scored rows fit the cap (always at least one)
            b1, rows = b0, 0
            while b1 < B:
                r = sum(len(y) + 1 for y in hyps[b1])
                if b1 > b0 and (rows + r) * row_bytes > self.RESCORE_LOGIT_BYTES:
                    break
                rows, b1 = rows + r, b1 + 1
            s, t = self._score_chunk(encoder_padded_outputs[b0:b1], hyps[b0:b1], return_tokens)
            scores += s
            tokens += t
            b0 = b1
        return (scores, tokens) if return_tokens else scores

    def _score_chunk(self, enc, hyps, return_tokens):
        """score_hypotheses for utterances whose logits fit one pass -> (scores, per-token terms or empty lists), nested per utterance."""
        flat = [y for hs in hyps for y in hs]
        if not flat:
            return [[] for _ in hyps], [[] for _ in hyps]
        out, seg_off = self._score_rows(enc, hyps)[:2]
        back = torch.cat([out["score"], out["tok"]] if return_tokens else [out["score"]]).cpu().tolist()
        scores, tokens, at = [], [], 0
        for hs in hyps:
            scores.append(back[at:at + len(hs)])
            tokens.append([back[len(flat) + seg_off[at + w]:len(flat) + seg_off[at + w + 1]] for w in range(len(hs))] if return_tokens else [])
            at += len(hs)
        return scores, tokens

    def _score_rows(self, enc, hyps, differentiable=False):
        """The one teacher-forced pass of score_hypotheses over `hyps` (label-id lists per utterance, at least one in all) ->
        (dict(score (R,), tok (M,)) on the device, seg_off (the R + 1 row offsets, a list), logits (M, V) fp32, targets (M,) on the
        device), the R hypotheses in order.  differentiable: the same launches with the scores through F_.SeqLogProbFn, so that they carry
        a gradient back to the parameters and the encoder output (MWER training, Transformer.mwer_step); the vocabulary projection then
        reports its weight ready as Decoder.forward's does."""
        Bc = len(hyps)
        flat = [y for hs in hyps for y in hs]
        W = max(len(hs) for hs in hyps)
        L = max(len(y) for y in flat) + 1
        dev = enc.device
        ys = [[constant.SOS_TOKEN] + [constant.PAD_TOKEN] * (L - 1) for _ in range(Bc * W)]       # (dummies: the empty sequence)
        index, targets, seg_off = [], [], [0]
        for b, hs in enumerate(hyps):
            for w, y in enumerate(hs):
                n, row = len(y), b * W + w
                ys[row][1:n + 1] = y
                index += range(row * L, row * L + n + 1)
                targets += y + [constant.EOS_TOKEN]
                seg_off.append(len(targets))
        M = len(targets)
        packed = torch.tensor([t for row in ys for t in row] + index + targets, dtype=torch.int64).to(dev, non_blocking=True)
        ys_d, index_d, tgt_d = torch.split(packed, [Bc * W * L, M, M])
        seg_d = torch.tensor(seg_off, dtype=torch.int32).to(dev, non_blocking=True)
        p = self.dropout.p if self.training else 0.0
        x = F_.EmbedFn.apply(ys_d.view(Bc * W, L), self.trg_embedding.weight, self.positional_encoding.pe[0], self.x_logit_scale, p,
                             constant.PAD_TOKEN, True)
        D = x.shape[-1]
        kv_pre = F_.cross_kv_all(enc, self.layers) if len(self.layers) > 1 else None
        for li, layer in enumerate(self.layers):           # DecoderLayer.forward's causal_only branch, on two views of the same rows
            x = x.reshape(Bc * W, L, D)
            x, _ = layer.self_attn(x, x, x, causal=True, need_attn=False)
            q = x.reshape(Bc, W * L, D)
            if kv_pre is not None:
                x, _ = layer.encoder_attn(q, enc, enc, need_attn=False, kv_pre=(kv_pre[0][li], kv_pre[1], li))
            else:
                x, _ = layer.encoder_attn(q, enc, enc, need_attn=False)
            x = layer.pos_ffn(x)
        scored = x.reshape(Bc * W * L, D).index_select(0, index_d)
        logits = F_.linear(scored, self.output_linear.weight, None, True, differentiable and not self.emb_trg_sharing)
        tgt_d = tgt_d.contiguous()
        if differentiable:
            score, tok = F_.SeqLogProbFn.apply(logits, tgt_d, seg_d)
            out = {"score": score, "tok": tok}
        else:
            out = ops.seq_logprob(logits, tgt_d, seg_d)
        return out, seg_off, logits, tgt_d

    def _kv_cache_supported(self):
        """The incremental decoders (asr_hip/decode.py) read the full-rank projection weights of every layer; the Low-Rank
        Transformer (--rank > 0: LowRankLinear holds .u / .v, no .weight) decodes by re-running the layer modules over the
        prefix instead, like the reference's own loop.  So does a model with dim_key != dim_value (the caches hold H * dim_key columns for
        keys and values alike)."""
        return (self.dim_key == self.dim_value and
                all(isinstance(l.self_attn, MultiHeadAttention) and isinstance(l.encoder_attn, MultiHeadAttention) for l in self.layers))

    @torch.no_grad()
    def greedy_search(self, encoder_padded_outputs, beam_width=2, lm_rescoring=False, lm=None, lm_weight=0.1, c_weight=1,
                      use_cache=True, return_ids=False):
        """1-best strings of the reference's 300-step greedy loop (transformer.py:316-394).  Needs --tgt-max-len >= 301.
        use_cache=True decodes incrementally with per-layer key/value caches, one captured hipGraph replayed per token
        (asr_hip/decode.py; in bf16 the step is the 30-launch one of csrc/decode.hip when the shapes allow it); "graph" the same
        with the kernel-per-op step; "eager" that step without the graph; False re-runs the full decoder over the prefix at
        every step like the reference -- "graph" / "eager" / False give the same tokens (tests/test_gpu_decode.py), the fused
        step the same within the bf16 tolerance (tests/test_gpu_decode_fused.py).  return_ids: (strings, the label ids before EOS)."""
        if lm_rescoring:
            raise NotImplementedError("LM rescoring applies to beam search only: it re-ranks the finished beam hypotheses, and greedy "
                                      "decoding keeps one (the reference's greedy LM branch, transformer.py:357-372, cannot run: it "
                                      "passes a str where calculate_lm_score expects label ids)")
        if not self._kv_cache_supported():
            use_cache = False
        if use_cache == "eager":                      # cached, launches issued from Python per token
            from asr_hip.decode import greedy_search as cached_greedy
            toks = cached_greedy(self, encoder_padded_outputs, steps=300)
        elif use_cache:                               # cached + one hipGraph replay per token (device-side position)
            from asr_hip.decode import greedy_search_graphed
            fused = False if use_cache == "graph" else None      # "graph": the kernel-per-op step; True: 30-launch step in bf16
            toks = greedy_search_graphed(self, encoder_padded_outputs, steps=300, fused=fused)
        else:
            toks = search.greedy_rerun(self, encoder_padded_outputs)
        sents, ids = search.strings_up_to_eos(toks.cpu().tolist(), self.id2label)       # one D2H copy instead of per-token .item()
        return (sents, ids) if return_ids else sents

    @torch.no_grad()
    def beam_search(self, encoder_padded_outputs, beam_width=2, nbest=5, lm_rescoring=False, lm=None, lm_weight=0.1,
                    c_weight=1, prob_weight=1.0, use_cache=True, ctc_logits=None, ctc_lengths=None, ctc_weight=0.0, ctc_candidates=0):
        """Per-utterance beam search with the reference's scoring (transformer.py:396-517).  With
        use_cache the live hypotheses are one batch of the KV-cached decoder (one step = one token per
        hypothesis); the candidate bookkeeping on the host is the reference's, including its in-loop re-sort (:460)
        (asr_hip.search.beam_search).  The cached search runs for all utterances at once, one or many;
        use_cache="per_utterance" runs it on one utterance at a time; False re-runs the full decoder over every prefix like the
        reference.  lm_rescoring=True with lm (utils/lstm_utils.LM) re-ranks the finished
        hypotheses with the LM score (_rank_ended); the search itself prunes on the acoustic score alone, as in the reference.
        ctc_weight = mu > 0 with ctc_logits (B,T',V) fp32 (the encoder CTC head's) and ctc_lengths (true encoder frames): joint CTC /
        attention scoring -- every step ranks the ctc_candidates (0: min(V, 16, 2 * beam_width)) best attention candidates of a
        hypothesis by (1 - mu) * attention log-probability + mu * CTC prefix log-probability increment (csrc/ctc_prefix.hip) and keeps
        the beam_width best; batched KV-cached search only."""
        if lm_rescoring and lm is None:
            raise ValueError("lm_rescoring=True needs lm (utils.lstm_utils.LM)")
        lm = lm if lm_rescoring else None
        if not self._kv_cache_supported():
            use_cache = False
        ctc = None
        if ctc_weight > 0:
            if not 0.0 < ctc_weight <= 1.0:
                raise ValueError("ctc_weight must lie in [0, 1], got %g" % ctc_weight)
            if ctc_logits is None:
                raise ValueError("ctc_weight %g needs ctc_logits (the encoder CTC head's output)" % ctc_weight)
            if not use_cache or use_cache == "per_utterance":
                raise NotImplementedError("joint CTC / attention scoring runs in the batched KV-cached beam search only (not the uncached "
                                          "path, use_cache='per_utterance' or a low-rank / dim_key != dim_value model)")
            from asr_hip.decode import CTCPrefixScorer
            B, Te, V = ctc_logits.shape
            K = int(ctc_candidates) if ctc_candidates else min(V, 16, 2 * beam_width)
            if not beam_width <= K <= min(V, 16):
                raise ValueError("ctc_candidates %d must lie in [beam_width %d, min(V, 16) = %d]" % (K, beam_width, min(V, 16)))
            if ctc_lengths is None:
                ctc_lengths = [Te] * B
            ctc = (CTCPrefixScorer(ctc_logits, ctc_lengths, [b for b in range(B) for _ in range(beam_width)]), float(ctc_weight), K)
        if use_cache == "per_utterance":
            ended = [self._beam_search_hyps(encoder_padded_outputs[b:b + 1], beam_width)[0] for b in range(encoder_padded_outputs.size(0))]
        else:
            ended = self._beam_search_hyps(encoder_padded_outputs, beam_width, ctc=ctc, use_cache=use_cache)
        return self._rank_ended(ended, nbest, c_weight, lm, lm_weight)

    def _rank_ended(self, ended, nbest, c_weight, lm=None, lm_weight=0.1):
        """The nbest finished hypotheses of every utterance (ended: one list per utterance) by final_score, best first
        (asr_hip.search.rank_ended: score + sqrt(words) * c_weight, with an LM score + lm_weight * (lm_score - 2 * oov) +
        sqrt(num_words) * c_weight from ONE batched LM call) -> (label ids, strings), flat over the utterances."""
        ranked = [hyp for hs in search.rank_ended(ended, nbest, c_weight, self.id2label, lm, lm_weight) for hyp in hs]
        return [hyp['yseq'] for hyp in ranked], [self.post_process_hyp(hyp) for hyp in ranked]

    def _finish_hyp(self, hyp, c_weight):
        return search.finish_hyp(hyp, c_weight, self.id2label)

    def _beam_search_hyps(self, encoder_padded_outputs, beam_width, ctc=None, use_cache=True):
        """The search for ALL utterances of the batch at once (asr_hip.search.beam_search): utterance b owns decoder rows b * W ..
        b * W + W - 1.  use_cache: ONE KV-cached decoder batch, so a step is one decoder step, one log-softmax / top-W launch and one
        device -> host copy for the whole batch; else one full decoder pass per live hypothesis, like the reference.  The candidate
        bookkeeping per utterance is the reference's (transformer.py:437-497: the in-loop re-sort, forced EOS at the last encoder frame),
        so the strings are those of a loop over utterances.  -> the finished hypotheses, one list per utterance (for _rank_ended).

        ctc = (scorer, mu, K): joint CTC / attention scoring, cached only.  The step takes the top-K attention
        log-probabilities per row instead of the top-W and the scorer (asr_hip.decode.CTCPrefixScorer, or a host restatement in the
        tests; its interface: search.CachedBeamStep) their CTC prefix log-probabilities; search.beam_search keeps the W best of a
        hypothesis by the joint score and names what 'score', 'att', 'psi' and 'slot' of a hypothesis hold."""
        B, max_len = encoder_padded_outputs.size(0), encoder_padded_outputs.size(1)
        if ctc is not None:
            scorer, mu, K = ctc
            step, ctc = search.CachedBeamStep(self, encoder_padded_outputs, beam_width, K, scorer), (mu, K)
        else:
            step = (search.CachedBeamStep if use_cache else search.RerunBeamStep)(self, encoder_padded_outputs, beam_width)
        return search.beam_search(step, B, beam_width, max_len, ctc)


class DecoderLayer(nn.Module):
    """DecoderLayer(dim_model, dim_inner, num_heads, dim_key, dim_value, dropout=0.1)   (reference: transformer.py:519-545)"""

    def __init__(self, dim_model, dim_inner, num_heads, dim_key, dim_value, dropout=0.1, rank=0):
        super().__init__()
        if rank > 0:
            self.self_attn = LowRankMultiHeadAttention(num_heads, dim_model, dim_key, dim_value, rank, dropout=dropout)
            self.encoder_attn = LowRankMultiHeadAttention(num_heads, dim_model, dim_key, dim_value, rank, dropout=dropout)
            self.pos_ffn = LowRankPositionwiseFeedForward(dim_model, dim_inner, rank, dropout=dropout)
            return
        self.self_attn = MultiHeadAttention(num_heads, dim_model, dim_key, dim_value, dropout=dropout)
        self.encoder_attn = MultiHeadAttention(num_heads, dim_model, dim_key, dim_value, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForwardWithConv(dim_model, dim_inner, dropout=dropout)

    def forward(self, decoder_input, encoder_output, non_pad_mask=None, self_attn_mask=None, dec_enc_attn_mask=None,
                row_keep=None, self_key_pad=None, enc_key_len=None, causal_only=False, need_attn=False, kv_grad_box=None, kv_pre=None):
        if causal_only:
            x, sa = self.self_attn(decoder_input, decoder_input, decoder_input, causal=True, need_attn=need_attn)
            x, ea = self.encoder_attn(x, encoder_output, encoder_output, need_attn=need_attn)
            return self.pos_ffn(x), sa, ea
        if row_keep is None and non_pad_mask is not None:      # reference-style call with materialised masks
            row_keep = non_pad_mask.reshape(-1).ne(0).to(torch.uint8)
        generic = self_key_pad is None and self_attn_mask is not None
        x, sa = self.self_attn(decoder_input, decoder_input, decoder_input, mask=self_attn_mask if generic else None,
                               key_pad=self_key_pad, causal=not generic, row_keep=row_keep, need_attn=need_attn)
        if kv_pre is not None:
            x, ea = self.encoder_attn(x, encoder_output, encoder_output, mask=dec_enc_attn_mask, key_len=enc_key_len,
                                      row_keep=row_keep, need_attn=need_attn, kv_pre=kv_pre)
        else:
            x, ea = self.encoder_attn(x, encoder_output, encoder_output, mask=dec_enc_attn_mask, key_len=enc_key_len,
                                      row_keep=row_keep, need_attn=need_attn, kv_grad_box=kv_grad_box)
        x = self.pos_ffn(x, row_keep=row_keep)
        return x, sa, ea
