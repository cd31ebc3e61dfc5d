"""Trains the LSTM language model of `test.py --beam-search --lm-rescoring --lm-path <lm.pt>` on the GPU (asr_hip/lm_train.py).

    python train_lm.py --train-manifest-list data/train.csv --valid-manifest-list data/valid.csv --name lm --epochs 10

The corpus is the transcripts behind the manifests and / or plain text files (one sentence per line), cut into words as LM rescoring
cuts a hypothesis (utils/lm_text.py).  Writes <save-folder>/<name>/epoch_N.pt and best_lm.pt: the reference's LM checkpoint (word2idx,
idx2word, ntoken, ninp, nhid, nlayers, dropout, tie_weights, model_state_dict) plus optimizer, epoch, metrics, seed, clip for
--continue-from; tensors and plain containers only (LSTMLM loads with weights_only=True).
"""
import argparse
import logging
import math
import os
import sys


def parser():
    p = argparse.ArgumentParser(description="LSTM language model training for LM rescoring")
    p.add_argument("--train-manifest-list", nargs="+", default=[], help="manifests (audio_path,transcript_path) for training")
    p.add_argument("--valid-manifest-list", nargs="+", default=[], help="manifests for validation")
    p.add_argument("--train-text", nargs="+", default=[], help="text files, one sentence per line, for training")
    p.add_argument("--valid-text", nargs="+", default=[], help="text files for validation")
    p.add_argument("--min-count", type=int, default=1, help="words seen fewer times map to <oov>")
    p.add_argument("--max-vocab", type=int, default=0, help="vocabulary size cap, <eos> and <oov> included (0 = none)")
    p.add_argument("--batch-size", type=int, default=64, help="sentences per step")
    p.add_argument("--shuffle", action="store_true", help="shuffle the order of the length-sorted batches every epoch")
    p.add_argument("--ninp", type=int, default=650)
    p.add_argument("--nhid", type=int, default=650)
    p.add_argument("--nlayers", type=int, default=2)
    p.add_argument("--dropout", type=float, default=0.5)
    p.add_argument("--tie-weights", action="store_true", help="share encoder and decoder weights (needs ninp == nhid)")
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--clip", type=float, default=0.25, help="global gradient-norm clip (0 = off)")
    p.add_argument("--lr-decay", type=float, default=0.5, help="lr multiplier when the validation NLL did not improve")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--save-folder", default="save")
    p.add_argument("--name", default="lm")
    p.add_argument("--save-every", type=int, default=1, help="write epoch_N.pt every this many epochs")
    p.add_argument("--continue-from", default="", help="an epoch_N.pt of this program: resume after epoch N")
    return p


def evaluate(trainer, sentences, batch_size):
    nll, count = 0.0, 0
    for a in range(0, len(sentences), batch_size):
        s, c = trainer.evaluate(sentences[a:a + batch_size])
        nll, count = nll + s, count + c
    return nll / max(count, 1)


def main(argv=None):
    args = parser().parse_args(argv)
    import torch
    from asr_hip.lm_train import LSTMLMTrainer
    from utils import lm_text
    logging.basicConfig(level=logging.INFO, format="%(message)s", stream=sys.stdout)
    log = logging.getLogger("train_lm")
    if not torch.cuda.is_available():
        raise SystemExit("train_lm.py needs a HIP device: the LM trains on the kernels of csrc/lm_train.hip, there is no CPU path")
    train_words = lm_text.read_corpus(args.train_manifest_list, args.train_text)
    valid_words = lm_text.read_corpus(args.valid_manifest_list, args.valid_text)
    if not train_words:
        raise SystemExit("no training sentences: give --train-manifest-list and / or --train-text")
    start, metrics = 0, {"best_valid_nll": float("inf"), "history": []}
    if args.continue_from:
        ck = torch.load(args.continue_from, map_location="cpu", weights_only=True)
        idx2word, word2idx = list(ck["idx2word"]), dict(ck["word2idx"])
        trainer = LSTMLMTrainer.from_checkpoint(ck, clip=args.clip)
        start, metrics = int(ck["epoch"]), ck["metrics"]
        log.info("continuing from %s after epoch %d (lr %.3g)" % (args.continue_from, start, trainer.lr))
    else:
        idx2word = lm_text.build_vocab(train_words, args.min_count, args.max_vocab or None)
        word2idx = {w: i for i, w in enumerate(idx2word)}
        trainer = LSTMLMTrainer(idx2word, args.ninp, args.nhid, args.nlayers, dropout=args.dropout, tie_weights=args.tie_weights,
                                seed=args.seed, lr=args.lr, clip=args.clip)
    train = lm_text.encode(train_words, word2idx)
    valid = lm_text.encode(valid_words, word2idx) or train
    log.info("vocabulary %d words; %d training sentences (%d predicted words), %d validation sentences" % (
        len(idx2word), len(train), sum(len(s) - 1 for s in train), len(valid)))
    out_dir = os.path.join(args.save_folder, args.name)
    os.makedirs(out_dir, exist_ok=True)
    for epoch in range(start + 1, args.epochs + 1):
        tot, cnt = torch.zeros((), dtype=torch.float64, device=trainer.device), 0
        for b in lm_text.batches(train, args.batch_size, args.shuffle, trainer.seed, epoch):
            n = sum(len(s) - 1 for s in b)
            tot += trainer.step(b).double() * n
            cnt += n
        train_nll = tot.item() / cnt
        valid_nll = evaluate(trainer, valid, args.batch_size)
        log.info("epoch %d: train nll/word %.6f ppl %.2f | valid nll/word %.8f ppl %.2f | lr %.3g" % (
            epoch, train_nll, math.exp(min(train_nll, 50)), valid_nll, math.exp(min(valid_nll, 50)), trainer.lr))
        improved = valid_nll < metrics["best_valid_nll"]
        metrics = {"best_valid_nll": min(valid_nll, metrics["best_valid_nll"]), "train_nll": train_nll, "valid_nll": valid_nll,
                   "history": list(metrics["history"]) + [[epoch, train_nll, valid_nll]]}
        if not improved:
            trainer.lr *= args.lr_decay
        ck = trainer.checkpoint(word2idx, idx2word, epoch=epoch, metrics=metrics)
        if improved:
            torch.save(ck, os.path.join(out_dir, "best_lm.pt"))
        if args.save_every > 0 and epoch % args.save_every == 0:
            torch.save(ck, os.path.join(out_dir, "epoch_%d.pt" % epoch))


if __name__ == "__main__":
    main()
