"""Estimates the label n-gram LM of `test.py --ctc-beam-search --ngram-path <ngram.pt>` (utils/ngram.py).  Host only.

    python train_ngram.py --train-manifest-list data/train.csv --labels-path labels.json --order 3 --name ngram

The corpus is the transcripts behind the manifests and / or plain text files (one sentence per line), read as train_lm.py reads them
(utils/lm_text.py) and mapped to label ids as the loader maps a transcript: characters outside the label file, and id 0, are dropped.
Counted are the n-grams of [SOS] + ids + [EOS]; the estimate is interpolated Witten-Bell.  Writes <save-folder>/<name>/ngram.pt: the order,
V, the label list and the arrays (tensors and plain containers only).
"""
import argparse
import os


def parser():
    p = argparse.ArgumentParser(description="label n-gram LM for first-pass fusion in the CTC prefix beam search")
    p.add_argument("--train-manifest-list", nargs="+", default=[], help="manifests (audio_path,transcript_path)")
    p.add_argument("--train-text", nargs="+", default=[], help="text files, one sentence per line")
    p.add_argument("--labels-path", default="labels.json", help="the model's label file")
    p.add_argument("--order", type=int, default=3, help="1..4")
    p.add_argument("--save-folder", default="save")
    p.add_argument("--name", default="ngram")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    from train import build_labels
    from utils import constant, lm_text
    from utils.ngram import NgramLM, encode_transcript
    label2id, id2label = build_labels(args.labels_path)
    texts = []
    for path in args.train_manifest_list:
        texts.extend(lm_text.read_manifest(path))
    for path in args.train_text:
        texts.extend(lm_text.read_text(path))
    sentences = [s for s in (encode_transcript(t, label2id) for t in texts) if s]
    if not sentences:
        raise SystemExit("no training sentences: give --train-manifest-list and / or --train-text")
    lm = NgramLM.estimate(sentences, len(id2label), args.order, constant.SOS_TOKEN, constant.EOS_TOKEN,
                          labels=[id2label[i] for i in range(len(id2label))])
    out_dir = os.path.join(args.save_folder, args.name)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "ngram.pt")
    lm.save(path)
    print("order %d over %d labels: %d sentences, %d labels, %d n-grams stored -> %s" % (
        lm.order, lm.V, len(sentences), sum(len(s) for s in sentences), len(lm.keys), path))
    return path


if __name__ == "__main__":
    main()
