"""asr_hip/search.py without a GPU: the batched beam-search bookkeeping, driven by a scripted step object, against the one-hypothesis-at-a-
time restatement of tests/search_reference.py -- the same finished hypotheses in the same order with exactly equal scores -- and the
ranking of finished hypotheses against its formula."""
import functools
import math
import random

import pytest
import torch

import ctc_prefix_reference as R
import search_reference as S
from asr_hip import search
from utils import constant

PAD, SOS, EOS = constant.PAD_TOKEN, constant.SOS_TOKEN, constant.EOS_TOKEN


def _table(V, halves):
    """table(u, prefix) -> V log-probabilities, a pure function of (utterance, prefix): logits drawn from a generator seeded with the
    pair, EOS made likelier as the prefix grows (faster for later utterances, so that utterances end at different steps), all logits
    rounded to halves on request so that equal log-probabilities occur."""
    @functools.lru_cache(maxsize=None)
    def row(u, prefix):
        rng = random.Random("%d|%s" % (u, prefix))
        logits = [rng.gauss(0.0, 1.0) for _ in range(V)]
        logits[EOS] = -5.0 + (0.3 + 0.15 * u) * len(prefix) + 0.25 * rng.gauss(0.0, 1.0)
        if halves:
            logits = [round(2.0 * x) / 2.0 for x in logits]
        m = max(logits)
        lse = m + math.log(sum(math.exp(x - m) for x in logits))
        return tuple(x - lse for x in logits)
    return lambda u, prefix: row(u, tuple(prefix))


class ScriptedStep:
    """The step object of search.beam_search on a table: no decoder, no device.  Idle rows are scored on [SOS], as the cached step
    scores them; with a scorer (ctc_prefix_reference.HostPrefixScorer) it goes through the scorer's step / select like that step."""

    def __init__(self, table, V, W, K, scorer=None):
        self.table, self.V, self.W, self.K, self.scorer = table, V, W, K, scorer
        self.tie = False          # two live hypotheses of one utterance with exactly equal scores were handed in

    def step(self, live):
        best, idx = [], []
        for r, hyp in enumerate(live):
            lp = self.table(r // self.W, [SOS] if hyp is None else hyp['yseq'])
            order = sorted(range(self.V), key=lambda v: -lp[v])[:self.K]
            best.append([lp[v] for v in order])
            idx.append(order)
        for b in range(len(live) // self.W):
            scores = [h['score'] for h in live[b * self.W:(b + 1) * self.W] if h is not None]
            self.tie |= len(set(scores)) < len(scores)
        if self.scorer is None:
            return best, idx, None
        last = torch.tensor([SOS if h is None else h['yseq'][-1] for h in live], dtype=torch.int64)
        return best, idx, self.scorer.step(last, torch.tensor(idx, dtype=torch.int64)).tolist()

    def select(self, rows, slots):
        assert len(rows) == len(slots) and all(r // self.W == i // self.W for i, r in enumerate(rows))      # parents stay in their utterance
        if self.scorer is not None:
            self.scorer.select([r * self.K + k for r, k in zip(rows, slots)])


V_PLAIN = 8
PLAIN = [(1, 1, 5), (3, 4, 6), (5, 2, 40), (2, 3, 300)]
CASES = [(B, W, T, halves) for halves in (False, True) for (B, W, T) in PLAIN]


@functools.lru_cache(maxsize=None)
def _plain(B, W, T, halves):
    """-> (the loop's finished hypotheses, the restatement's, whether the step saw a tie)."""
    table = _table(V_PLAIN, halves)
    step = ScriptedStep(table, V_PLAIN, W, W)
    got = search.beam_search(step, B, W, T)
    want = [S.search_utterance(functools.partial(table, b), W, T) for b in range(B)]
    return got, want, step.tie


@pytest.mark.parametrize("B,W,T,halves", CASES)
def test_loop_equals_the_plain_restatement(B, W, T, halves):
    got, want, _ = _plain(B, W, T, halves)
    assert len(got) == B
    for g, w in zip(got, want):
        assert [h['yseq'] for h in g] == [h['yseq'] for h in w] and len(g) >= 1
        assert [h['score'] for h in g] == [h['score'] for h in w]                  # exactly: the same additions in the same order
        assert all(set(h) == {'score', 'yseq', 'parent'} and 0 <= h['parent'] < W for h in g)


def test_the_cases_exercise_what_they_should():
    """Conditions on the inputs: a forced EOS, an earlier end, two utterances of a batch ending at different steps, and a real tie among
    kept candidates in the rounded cases that keep more than one."""
    forced = early = apart = 0
    for B, W, T, halves in CASES:
        got, _, tie = _plain(B, W, T, halves)
        ends = [max(len(h['yseq']) for h in hs) for hs in got]          # T + 2: SOS, T labels and the EOS forced at step T - 1
        forced += sum(n == T + 2 for n in ends)
        early += sum(n < T + 2 for n in ends)
        apart += len(set(ends)) > 1
        if halves and W > 1:
            assert tie, (B, W, T)
    assert forced >= 1 and early >= 1 and apart >= 1


def test_joint_ctc_loop_equals_the_plain_restatement():
    B, W, T, mu, K, V, frames = 2, 3, 14, 0.3, 6, 12, [14, 9]
    g = torch.Generator().manual_seed(3)
    ctc_logits = torch.randn(B, T, V, generator=g, dtype=torch.float64)
    table = _table(V, False)
    scorer = R.HostPrefixScorer(ctc_logits, frames, [b for b in range(B) for _ in range(W)])
    got = search.beam_search(ScriptedStep(table, V, W, K, scorer), B, W, T, ctc=(mu, K))
    lp = R.log_softmax(ctc_logits.numpy())
    for b in range(B):
        want = S.search_utterance(functools.partial(table, b), W, T, ctc=(mu, K, lp[b], frames[b]))
        assert [h['yseq'] for h in got[b]] == [h['yseq'] for h in want] and len(want) >= 1
        for key in ('score', 'att', 'psi'):
            assert [h[key] for h in got[b]] == [h[key] for h in want], key
        assert all(0 <= h['slot'] < K and 0 <= h['parent'] < W for h in got[b])
        assert any(h['score'] > -math.inf for h in got[b])          # CTC did not rule everything out


def test_rank_ended_nests_per_utterance_and_orders_by_the_word_bonus():
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, "a", "b", " "]
    id2label = dict(enumerate(chars))
    a, b, sp = 3, 4, 5
    ended = [[{'score': -1.0, 'yseq': [SOS, a, EOS]},                            # 1 word
              {'score': -1.5, 'yseq': [SOS, a, sp, b, sp, a, EOS]},              # 3 words: wins at c_weight 1
              {'score': -1.2, 'yseq': [SOS, a, sp, sp, b, EOS]}],                # 2 words (a doubled space is one)
             [],
             [{'score': -3.0, 'yseq': [SOS, EOS]},                               # no word
              {'score': -3.0, 'yseq': [SOS, b, EOS]}]]
    words = [[1, 3, 2], [], [0, 1]]
    for c_weight, nbest in ((1.0, 2), (0.0, 5), (0.1, 1)):
        ranked = search.rank_ended([[dict(h) for h in hs] for hs in ended], nbest, c_weight, id2label)
        assert len(ranked) == 3
        for hs, ws, out in zip(ended, words, ranked):
            final = [h['score'] + math.sqrt(w) * c_weight for h, w in zip(hs, ws)]
            order = sorted(range(len(hs)), key=lambda n: -final[n])[:nbest]
            assert [h['yseq'] for h in out] == [hs[n]['yseq'] for n in order]
            assert [h['final_score'] for h in out] == [final[n] for n in order]
    strs, ids = search.strings_up_to_eos([[a, sp, b, EOS, a], [b, b]], id2label)
    assert strs == ["a b", "bb"] and ids == [[a, sp, b], [b, b]]


def test_nbest_bookkeeping_of_the_kernel_searches():
    """nbest_to_host / fuse_scores / render_nbest on a hand-made output dict (CPU tensors): found hypotheses only, in place order, with
    the float bits of the op's tensors; the fusion terms added in the order the model tests compare with ==; the fields per arm."""
    B, W, L = 2, 3, 4
    out = dict(ids=torch.tensor([[[3, 4, 0, 0], [4, 0, 0, 0], [0, 0, 0, 0]], [[0, 0, 0, 0]] * 3], dtype=torch.int32),
               lengths=torch.tensor([[2, 1, -1], [0, -1, -1]], dtype=torch.int32),
               scores=torch.tensor([[-1.25, -2.1, -math.inf], [0.0, -math.inf, -math.inf]]),
               lm=torch.tensor([[-3.3, -0.7, 0.0], [-0.1, 0.0, 0.0]]), credit=torch.tensor([[2, 0, 0], [0, 0, 0]], dtype=torch.int32))
    sc, lm = out["scores"].tolist(), out["lm"].tolist()
    plain = search.nbest_to_host(out, B, W, L, False, False)
    assert plain == [[{'yseq': [3, 4], 'score': sc[0][0]}, {'yseq': [4], 'score': sc[0][1]}], [{'yseq': [], 'score': 0.0}]]
    a, beta, gamma = 0.3, 0.5, 1.5
    for has_context in (False, True):
        ended = search.nbest_to_host(out, B, W, L, True, has_context)
        assert [[set(h) for h in hs] for hs in ended] == [[{'yseq', 'score', 'lm'} | ({'credit'} if has_context else set())] * n for n in (2, 1)]
        search.fuse_scores(ended, 'ctc_score', a, beta, gamma)
        h = ended[0][0]
        assert set(h) == {'yseq', 'score', 'ctc_score', 'ngram_score'} | ({'context_credit'} if has_context else set())
        want = sc[0][0] + a * lm[0][0] + beta * 2
        if has_context:
            want += gamma * 2
            assert type(h['context_credit']) is int and h['context_credit'] == 2
        assert h['score'] == want and h['ctc_score'] == sc[0][0] and h['ngram_score'] == lm[0][0]
        assert ended[1][0]['score'] == 0.0 + a * lm[1][0] + beta * 0 + (gamma * 0 if has_context else 0.0)
    id2label = dict(enumerate([constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR, "a", "b"]))
    strs, ids = search.render_nbest(plain, 2, 0.0, id2label, None, 0.1, True)
    assert ids == [[[3, 4], [4]], [[]]] and strs == [["ab", "b"], [""]] and search.render_nbest(plain, 1, 0.0, id2label, None, 0.1, False) == [["ab"], [""]]
