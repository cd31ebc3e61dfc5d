"""Host side of CTC forced alignment (test.py --align-out): encoder frames to seconds, labels to words, and the
JSON-lines writer.  The alignment itself is Transformer.ctc_align (csrc/ctc_align.hip)."""
import json
import math

from utils.lstm_utils import is_contain_chinese_word


def label_times(labels, feat, window_stride, input_frames):
    """Transformer.ctc_align's labels (encoder frames) -> [{"id", "label", "start", "end" (seconds), "logp", "frames"}].  A label starts
    where the span of its first encoder frame starts and ends where the span of its last one ends (encoder_frame_span), the end clamped
    to the utterance's true input length."""
    from models.asr.transformer import encoder_frame_span
    out = []
    for lab in labels:
        a = encoder_frame_span(lab["start_frame"], feat)[0]
        b = encoder_frame_span(lab["end_frame"] - 1, feat)[1]
        a, b = min(a, int(input_frames)), min(b, int(input_frames))
        out.append({"id": lab["id"], "label": lab["label"], "start": a * window_stride, "end": b * window_stride, "logp": lab["logp"],
                    "frames": lab["end_frame"] - lab["start_frame"]})
    return out


def group_words(labels):
    """Timed labels -> words.  Labels between space labels form a word; a Chinese label (utils.lstm_utils.is_contain_chinese_word) is a
    word of its own.  A word starts with its first label and ends with its last; its logp is the MEAN per-frame label log-probability
    over its labels' frames (a label's logp is the sum over its frames).  Spaces belong to no word."""
    words, run = [], []

    def close():
        if run:
            frames = sum(x["frames"] for x in run)
            words.append({"word": "".join(x["label"] for x in run), "start": run[0]["start"], "end": run[-1]["end"],
                          "logp": sum(x["logp"] for x in run) / max(1, frames)})
            del run[:]

    for lab in labels:
        if lab["label"] == " ":
            close()
        elif is_contain_chinese_word(lab["label"]):
            close()
            run.append(lab)
            close()
        else:
            run.append(lab)
    close()
    return words


def utterance_record(index, text, alignment, feat, window_stride, input_frames):
    """One line of --align-out from one entry of Transformer.ctc_align.  An utterance without a feasible alignment has score null and
    empty lists."""
    score = alignment["score"]
    if score is None or not math.isfinite(score):
        return {"utt": int(index), "text": text, "score": None, "score_per_frame": None, "labels": [], "words": []}
    labels = label_times(alignment["labels"], feat, window_stride, input_frames)
    words = group_words(labels)
    for lab in labels:
        del lab["frames"]
    return {"utt": int(index), "text": text, "score": score, "score_per_frame": score / max(1, int(alignment["frames"])),
            "labels": labels, "words": words}


class AlignmentWriter:
    """JSON lines, one utterance per line, flushed as they come (a long test set can be followed while it runs)."""

    def __init__(self, path):
        self.f = open(path, "w", encoding="utf-8")
        self.count = 0

    def write(self, record):
        self.f.write(json.dumps(record, ensure_ascii=False, allow_nan=False) + "\n")
        self.f.flush()
        self.count += 1

    def close(self):
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
