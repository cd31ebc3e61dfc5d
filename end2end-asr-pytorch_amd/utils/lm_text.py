"""Text side of LM training (train_lm.py): corpus reading, the word segmentation of LM rescoring, vocabulary, batches.  Host only.

A sentence is cut into words exactly as utils/lstm_utils.py:lm_word_string cuts a hypothesis before it reaches the LM: "  " -> " ",
runs of Chinese / non-Chinese words, every character of a word with a Unicode 'Lo' character a word of its own.  For a transcript whose
characters are all labels, lm_words(text) == lm_word_string(label_ids, id2label).split().
"""
import random

from utils import constant
from utils.lstm_utils import _join_words, get_word_segments_per_language, is_contain_chinese_word

EOS_WORD, OOV_WORD = "<eos>", "<oov>"


def lm_words(text):
    """The words the LM sees for `text` (lm_word_string's steps on a string instead of label ids)."""
    s = text
    for ch in (constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR):
        s = s.replace(ch, "")
    s = s.replace("  ", " ")
    words = []
    for seg in get_word_segments_per_language(s):
        words.extend(seg if is_contain_chinese_word(seg) else [seg])
    return _join_words(words).replace("  ", " ").replace("  ", " ").split()


def read_manifest(path):
    """Transcripts behind a manifest of `audio_path,transcript_path` lines, read as utils/data_loader.py reads them before the
    mapping to labels: the whole file, newlines removed, lower-cased."""
    out = []
    with open(path) as f:
        rows = [ln.strip().split(",") for ln in f if ln.strip()]
    for row in rows:
        with open(row[1], "r", encoding="utf8") as t:
            out.append(t.read().replace("\n", "").lower())
    return out


def read_text(path):
    """One sentence per line, lower-cased like the transcripts."""
    with open(path, "r", encoding="utf8") as f:
        return [ln.rstrip("\n").lower() for ln in f]


def read_corpus(manifests=(), texts=()):
    """-> list of word lists; sentences without words are dropped."""
    sents = []
    for p in manifests or ():
        sents.extend(read_manifest(p))
    for p in texts or ():
        sents.extend(read_text(p))
    return [w for w in (lm_words(s) for s in sents) if w]


def build_vocab(sentences, min_count=1, max_vocab=None):
    """-> idx2word: '<eos>', '<oov>', then the words with count >= min_count, most frequent first (ties: the word itself), at most
    max_vocab entries in all."""
    count = {}
    for ws in sentences:
        for w in ws:
            count[w] = count.get(w, 0) + 1
    words = sorted((w for w, c in count.items() if c >= min_count and w not in (EOS_WORD, OOV_WORD)), key=lambda w: (-count[w], w))
    idx2word = [EOS_WORD, OOV_WORD] + words
    return idx2word[:max(2, max_vocab)] if max_vocab else idx2word


def encode(sentences, word2idx):
    """Word lists -> id lists ending in '<eos>'; unknown words map to '<oov>' (LSTMLM.ids)."""
    oov, eos = word2idx[OOV_WORD], word2idx[EOS_WORD]
    return [[word2idx.get(w, oov) for w in ws] + [eos] for ws in sentences if ws]


def batches(id_sentences, batch_size, shuffle=False, seed=0, epoch=0):
    """Sentences sorted by length into bins of batch_size; with shuffle the ORDER OF THE BINS is drawn from a generator seeded by
    (seed, epoch) -- an epoch's batches do not depend on the epochs run before it (resuming reproduces them)."""
    order = sorted(range(len(id_sentences)), key=lambda i: (len(id_sentences[i]), id_sentences[i]))
    bins = [[id_sentences[i] for i in order[a:a + batch_size]] for a in range(0, len(order), batch_size)]
    if shuffle:
        random.Random(seed * 1000003 + epoch).shuffle(bins)
    return bins
