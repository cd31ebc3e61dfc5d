"""The host side of decoding for models.asr.transformer.Decoder: ONE beam-search bookkeeping loop, the two step objects that feed it
numbers, the ranking of finished hypotheses, and the reference's uncached greedy loop (reference: transformer.py:316-517).

beam_search() makes no device call, so its bookkeeping runs against a scripted step object on the CPU (tests/test_search_host.py):
    step(live)          live[r]: the hypothesis of decoder row r, None for an idle row (never read back) -> host lists (best, idx, psi):
                        per row the top-K log-probabilities, best first, and their ids (K = W without CTC); psi: their CTC prefix
                        log-probabilities, None without CTC
    select(rows, slots) afterwards: row i of the next step continues candidate slots[i] of this step's row rows[i]
"""
import math

import torch

from . import ops
from utils import constant


def beam_search(step, B, W, max_len, ctc=None):
    """Beam search of width W for B utterances: utterance b owns rows b * W .. b * W + W - 1 (its live hypotheses in the first rows, the
    others idle).  The candidate bookkeeping per utterance is the reference's (transformer.py:437-497): every live hypothesis expanded by
    its W best candidates, the running list re-sorted INSIDE the hypothesis loop (:460), EOS forced at step max_len - 1 (the last encoder
    frame), hypotheses that end in EOS retired.  -> the finished hypotheses, one list per utterance (for rank_ended).

    ctc = (mu, K): joint CTC / attention scoring.  The step gives the top-K attention log-probabilities per row
    instead of the top-W and the CTC prefix log-probability psi of every candidate; the W best of a hypothesis by joint = (1 - mu) * att
    + mu * (psi' - psi(g)) go into the unchanged bookkeeping.  'score' accumulates the joint increments ('att' the attention terms and
    'psi' the prefix's CTC score alone); 'slot' is the candidate's place among the K."""
    hyps = [[{'score': 0.0, 'yseq': [constant.SOS_TOKEN]}] for _ in range(B)]
    if ctc is not None:
        mu, K = ctc
        for b in range(B):
            hyps[b][0].update(att=0.0, psi=0.0)
    ended = [[] for _ in range(B)]
    for i in range(300):
        live = [None] * (B * W)
        for b in range(B):
            live[b * W:b * W + len(hyps[b])] = hyps[b]
        best_all, idx_all, psi_all = step.step(live)
        rows = list(range(B * W))
        slots = [0] * (B * W)                  # (ctc) the candidate slot k a surviving row continues: its state is (parent row, k)
        for b in range(B):
            if not hyps[b]:
                continue
            cand = []
            for hi, hyp in enumerate(hyps[b]):
                best, idx = best_all[b * W + hi], idx_all[b * W + hi]
                if ctc is None:
                    for j in range(W):
                        cand.append({'score': hyp['score'] + best[j], 'yseq': hyp['yseq'] + [idx[j]], 'parent': hi})
                else:
                    psi = psi_all[b * W + hi]
                    # a candidate CTC rules out (blank, SOS, more labels than frames) scores -inf, never inf - inf
                    joint = [((1.0 - mu) * best[j] + mu * (psi[j] - hyp['psi'])) if psi[j] > -math.inf else -math.inf for j in range(K)]
                    for j in sorted(range(K), key=lambda j: joint[j], reverse=True)[:W]:      # stable: ties keep the attention order
                        cand.append({'score': hyp['score'] + joint[j], 'yseq': hyp['yseq'] + [idx[j]], 'parent': hi, 'slot': j,
                                     'att': hyp['att'] + best[j], 'psi': psi[j]})
                cand = sorted(cand, key=lambda h: h['score'], reverse=True)[:W]      # the reference's in-loop re-sort (:460)
            if i == max_len - 1:
                for hyp in cand:
                    hyp['yseq'] = hyp['yseq'] + [constant.EOS_TOKEN]
            hyps[b] = []
            for hyp in cand:
                (ended[b] if hyp['yseq'][-1] == constant.EOS_TOKEN else hyps[b]).append(hyp)
            for j, hyp in enumerate(hyps[b]):
                rows[b * W + j] = b * W + hyp['parent']
                slots[b * W + j] = hyp.get('slot', 0)
        if not any(hyps):
            break
        step.select(rows, slots)
    return ended


class CachedBeamStep:
    """One token per row through ONE KV-cached decoder batch (asr_hip.decode.DecoderKVCache): a step is one decoder step, one
    log-softmax / top-K launch and one device -> host copy for the whole batch.  scorer (joint CTC): an object with step(last, cand) ->
    psi (R,K) and select(flat) -- asr_hip.decode.CTCPrefixScorer, or a host restatement in the tests; its states are selected with the
    rows of the KV cache, and psi reaches the host in the same copy as the top-K values and indices."""

    def __init__(self, decoder, encoder_padded_outputs, W, K=None, scorer=None):
        from .decode import DecoderKVCache
        self.cache = DecoderKVCache(decoder, encoder_padded_outputs.repeat_interleave(W, dim=0), max_len=300)
        self.dev = encoder_padded_outputs.device
        self.K, self.scorer = W if K is None else K, scorer

    def step(self, live):
        K = self.K
        last = torch.tensor([constant.SOS_TOKEN if h is None else h['yseq'][-1] for h in live], dtype=torch.int64, device=self.dev)
        best, idx = ops.logsoftmax_topk(self.cache.step(last).float().contiguous(), K)
        if self.scorer is None:
            return best.tolist(), idx.tolist(), None
        psi = self.scorer.step(last, idx)
        if not psi.is_cuda:
            return best.tolist(), idx.tolist(), psi.tolist()
        # one device -> host copy per step (ids up to 2^24 are exact in fp32)
        packed = torch.cat([best, psi, idx.float()], dim=1).tolist()
        return [r[:K] for r in packed], [[int(x) for x in r[2 * K:]] for r in packed], [r[K:2 * K] for r in packed]

    def select(self, rows, slots):
        if rows != list(range(len(rows))):          # a row moved: reorder the self-attention caches
            self.cache.select(rows)
        if self.scorer is not None:
            self.scorer.select([r * self.K + k for r, k in zip(rows, slots)])


class RerunBeamStep:
    """The reference's own arm (and the production path of low-rank and dim_key != dim_value models): the whole decoder over the prefix
    of every live hypothesis, one Decoder._step_logits call on (1, t) tokens and the utterance's own encoder rows each -- never batched,
    so every GEMM keeps the shape it has in the reference's loop.  Nothing runs for idle rows; there is no state to select."""

    def __init__(self, decoder, encoder_padded_outputs, W):
        self.dec, self.enc, self.W = decoder, encoder_padded_outputs, W

    def step(self, live):
        best_all, idx_all = [None] * len(live), [None] * len(live)
        for r, hyp in enumerate(live):
            if hyp is None:
                continue
            b = r // self.W
            ys = torch.tensor([hyp['yseq']], dtype=torch.int64, device=self.enc.device)
            logits = self.dec._step_logits(ys, self.enc[b:b + 1])[:, -1]
            best, idx = ops.logsoftmax_topk(logits.float().contiguous(), self.W)
            best_all[r], idx_all[r] = best[0].tolist(), idx[0].tolist()
        return best_all, idx_all, None

    def select(self, rows, slots):
        pass


# ---------------------------------------------------------------------------------------------------- finished hypotheses
def finish_hyp(hyp, c_weight, id2label):
    s = "".join(id2label[t] for t in hyp['yseq'])
    for ch in (constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR):
        s = s.replace(ch, "")
    s = s.replace("  ", " ")
    hyp['final_score'] = hyp['score'] + math.sqrt(len(s.split())) * c_weight
    return hyp


def rank_ended(ended, nbest, c_weight, id2label, lm=None, lm_weight=0.1):
    """The nbest finished hypotheses of every utterance (ended: one list per utterance) by final_score, best first, nested per utterance
    (reference: transformer.py:475-497, 499-514).  Without an LM final_score = score + sqrt(words) * c_weight.  With one,
    final_score = score + lm_weight * (lm_score - 2 * oov) + sqrt(num_words) * c_weight, num_words = LM words + 1: the LM
    score only re-ranks finished hypotheses, so those of ALL utterances are scored by ONE batched LM call here."""
    if lm is not None:
        from utils.lstm_utils import calculate_lm_scores
        flat = [h for hs in ended for h in hs]
        for hyp, (lm_score, num_words, oov) in zip(flat, calculate_lm_scores([h['yseq'] for h in flat], lm, id2label)):
            hyp['lm_score'], hyp['num_words'] = lm_score - oov * 2, num_words
            hyp['final_score'] = hyp['score'] + lm_weight * hyp['lm_score'] + math.sqrt(num_words) * c_weight
    else:
        for hs in ended:
            for hyp in hs:
                finish_hyp(hyp, c_weight, id2label)
    return [sorted(hs, key=lambda h: h['final_score'], reverse=True)[:min(len(hs), nbest)] for hs in ended]


# ---------------------------------------------------------------------------------------------------- the kernel searches' n-best
def nbest_to_host(out, B, W, L, fused, has_context):
    """The output dict of ops.ctc_beam_search / ops.rnnt_beam_search (nbest = W, rows of L ids) in ONE device-to-host copy -> per
    utterance its found hypotheses, best first, as {'yseq', 'score'} with the kernel's raw 'lm' (fused) and 'credit' (has_context)."""
    parts = [out["scores"]] + ([out["lm"]] if fused else []) + ([out["credit"]] if has_context else [])
    flat = torch.cat([out["ids"].reshape(-1), out["lengths"].reshape(-1)] + [p.view(torch.int32).reshape(-1) for p in parts]).cpu()
    ids, lens, *parts = torch.split(flat, [B * W * L, B * W] + [B * W] * len(parts))
    ids, lens = ids.view(B, W, L).tolist(), lens.view(B, W).tolist()
    cols = [(k, (p if k == 'credit' else p.view(torch.float32)).view(B, W).tolist()) for k, p in zip(('score', 'lm', 'credit'), parts)]
    return [[dict([('yseq', ids[b][n][:lens[b][n]])] + [(k, v[b][n]) for k, v in cols]) for n in range(W) if lens[b][n] >= 0]
            for b in range(B)]


def fuse_scores(ended, base, a, beta, gamma):
    """The fusion terms on the hypotheses of a fused search (nbest_to_host): h[base] = the kernel's score, 'ngram_score' its lm,
    'context_credit' its credit where there is one, and score = h[base] + a * ngram_score + beta * len(yseq) + gamma * context_credit,
    added in this order."""
    for hs in ended:
        for h in hs:
            h[base], h['ngram_score'] = h['score'], h.pop('lm')
            h['score'] = h[base] + a * h['ngram_score'] + beta * len(h['yseq'])
            if 'credit' in h:
                h['context_credit'] = h.pop('credit')
                h['score'] += gamma * h['context_credit']


def render_nbest(ended, nbest, c_weight, id2label, lm, lm_weight, return_ids):
    """rank_ended, then the label ids of every utterance's n-best as strings -> strings, or (strings, ids) with return_ids."""
    hyp_ids = [[h['yseq'] for h in hs] for hs in rank_ended(ended, nbest, c_weight, id2label, lm, lm_weight)]
    strs = [["".join(id2label[x] for x in row) for row in rows] for rows in hyp_ids]
    return (strs, hyp_ids) if return_ids else strs


# ---------------------------------------------------------------------------------------------------- greedy
def greedy_rerun(decoder, encoder_padded_outputs):
    """Token ids (B, 300) of the reference's greedy loop as it stands: the whole decoder over the growing prefix at every step."""
    B = encoder_padded_outputs.size(0)
    ys = torch.full((B, 1), constant.SOS_TOKEN, dtype=torch.int64, device=encoder_padded_outputs.device)
    steps = []
    for _ in range(300):
        logits = decoder._step_logits(ys, encoder_padded_outputs)
        nxt = ops.argmax_rows(logits[:, -1].contiguous())
        steps.append(nxt)
        ys = torch.cat([ys, nxt.unsqueeze(1)], dim=1)
    return torch.stack(steps, dim=1)


def strings_up_to_eos(toks, id2label):
    """Rows of token ids -> (strings, the label ids) before the first EOS."""
    sents, ids = [], []
    for row in toks:
        kept = row[:row.index(constant.EOS_TOKEN)] if constant.EOS_TOKEN in row else row
        sents.append("".join(id2label[t] for t in kept))
        ids.append(list(kept))
    return sents, ids
