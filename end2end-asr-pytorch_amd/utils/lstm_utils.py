"""LM rescoring of beam-search hypotheses -- the reference's names and return values (reference: utils/lstm_utils.py,
data/helper.py:56-98), executed by the batched LSTM of asr_hip/lm.py (csrc/lm.hip).

The word string of a hypothesis is built like the reference's: labels joined, PAD / SOS / EOS removed, "  " -> " ", the text cut into
runs of Chinese and non-Chinese words, every character of a Chinese run made a word of its own.  A word is Chinese when one of its
characters is in Unicode category 'Lo' -- the reference's rule for the LM, deliberately not the code-point range of
utils/metrics.py (which follows the reference's CER split).
"""
import unicodedata

from utils import constant


def is_contain_chinese_word(word):
    return any(unicodedata.category(ch) == "Lo" for ch in word)


def _join_words(words):
    """The reference's run joiner: words separated by one space, except that no space is put after an empty prefix."""
    out = ""
    for w in words:
        out = (out + " " + w) if out else w
    return out


def get_word_segments_per_language(seq):
    """Runs of consecutive same-language words of seq.split(" ") (empty words count as non-Chinese), each run re-joined."""
    segments, run, run_zh = [], [], None
    for w in seq.split(" "):
        zh = is_contain_chinese_word(w)
        if run and zh != run_zh:
            segments.append(_join_words(run))
            run = []
        run.append(w)
        run_zh = zh
    segments.append(_join_words(run))
    return segments


def lm_word_string(yseq, id2label):
    """The string the reference hands to LM.evaluate for a hypothesis of label ids (calculate_lm_score's preprocessing)."""
    s = "".join(id2label[int(t)] for t in yseq)
    for ch in (constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR):
        s = s.replace(ch, "")
    s = s.replace("  ", " ")
    words = []
    for seg in get_word_segments_per_language(s):
        words.extend(seg if is_contain_chinese_word(seg) else [seg])
    return _join_words(words).replace("  ", " ").replace("  ", " ")


def _ids(seq):
    if hasattr(seq, "dim"):                      # the reference's (1, L) tensor
        return seq.reshape(-1).tolist()
    return list(seq)


def _triple(nll, n_words, oov):
    return -nll / n_words + 1, n_words + 1, oov


def calculate_lm_score(seq, lm, id2label):
    """seq: label ids ((1, L) tensor or list) -> (lm_score, num_words, oov): (-NLL / words + 1, words + 1, oov), (-999, 0, 0) for a
    hypothesis without words."""
    return calculate_lm_scores([seq], lm, id2label)[0]


def calculate_lm_scores(yseqs, lm, id2label):
    """calculate_lm_score for many hypotheses with ONE batched LM forward (identical word strings share a row)."""
    strs = [lm_word_string(_ids(y), id2label) for y in yseqs]
    live = [i for i, s in enumerate(strs) if s.split()]
    out = [(-999, 0, 0)] * len(strs)
    if live:
        nll, oov = lm.model.score([strs[i] for i in live])
        for k, i in enumerate(live):
            out[i] = _triple(float(nll[k]), len(strs[i].split()), oov[k])
    return out


class LM(object):
    """LM(model_path): the reference's LM checkpoint (2+ layer LSTM, word vocabulary with '<eos>' and '<oov>') on the device."""

    def __init__(self, model_path, device="cuda"):
        from asr_hip.lm import LSTMLM
        self.model_path = model_path
        self.model = LSTMLM(model_path, device=device)
        self.word2idx, self.idx2word = self.model.word2idx, self.model.idx2word

    def evaluate(self, seq):
        """-> (summed NLL of the words of seq + '<eos>' given their prefixes, number of out-of-vocabulary words)"""
        nll, oov = self.model.score([seq])
        return float(nll[0]), oov[0]
