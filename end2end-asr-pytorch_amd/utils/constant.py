"""Command-line flags and special tokens of the training / test entry points.

Flag names, dests and defaults follow the reference interface (reference: utils/constant.py:6-94) so that existing
command lines keep working; `args` is the same process-global Namespace the reference exposes (constant.py:99).

Differences that do not change old command lines:
  * sys.argv is parsed only when the entry script is train.py / test.py (the reference parses at import time from ANY
    script, which makes its modules unusable from tests); otherwise `args` holds the defaults and can be replaced with
    `set_args(ns)` / `parse(argv)`;
  * `--precision {bf16,fp32}` selects the kernels' storage type (bf16 = perf mode, fp32 = parity mode);
  * `--dist-backend` / `--bucket-mb` / `--grad-wire` tune the RCCL data-parallel path that replaces nn.DataParallel under --parallel;
  * `--gpu-frontend`: the loader ships padded waveforms and the log-spectrogram is computed on the GPU (asr_stft_frames +
    fp32 MFMA DFT + asr_spect_finish) instead of on the host in the DataLoader workers;
  * `--spec-augment` (+ `--spec-time-warp/-freq-mask/-freq-masks/-time-mask/-time-masks/-time-mask-ratio`): SpecAugment of the
    training batches on the GPU front end;
  * `--speed-perturb F [F ...]`: speed perturbation of the training utterances on the GPU front end -- each is resampled (band-limited,
    csrc/resample.hip) by a factor drawn from the list, e.g. 0.9 1.0 1.1, before tempo / gain / noise; factors in [0.5, 2.0], rounded to
    thousandths;
  * `--rir-dir DIR` (+ `--rir-prob P`, `--rir-max-ms MS`): reverberation of the training utterances on the GPU front end -- with
    probability P (default 0.5) an utterance is convolved (csrc/reverb.hip) with one of the recorded room impulse responses under DIR,
    cut to MS milliseconds (default 500), after the speed change and before tempo / gain / noise;
  * `--features {spect,fbank}` (+ `--num-mel-bins`, `--mel-fmin`): the reference's 161 linear log1p(|STFT|) bins (default) or log-mel
    filterbank features of the same STFT, on the host path and on the GPU front end alike;
  * `--conv-module-kernel K` (odd, 3..31; 0 = off): a Conformer-style convolution module in every encoder layer;
  * `--pos-encoding {abs,rope}`: the reference's absolute sinusoid (default) or rotary position embedding of Q and K in every encoder
    self-attention; the decoder keeps its sinusoid;
  * `--ngram-path FILE` (+ `--ngram-weight`, `--ngram-length-bonus`; test.py --ctc-beam-search): a label n-gram LM of train_ngram.py
    fused into the CTC prefix beam search's pruning;
  * `--context-path FILE` (+ `--context-score`; test.py --ctc-beam-search): a list of phrases, one per line, that the CTC prefix beam
    search's pruning is biased towards (utils/context.py);
  * `--mwer-weight m` (+ `--mwer-nbest`, `--mwer-unit`; train.py with --ctc-weight > 0): minimum word error rate training over the CTC
    prefix beam search's n-best, rescored by the attention decoder with grad (csrc/mwer.hip);
  * `--distill-from PATH` (+ `--distill-weight`, `--distill-ctc-weight`, `--distill-temperature`; train.py): knowledge distillation from
    a frozen teacher checkpoint, word-level on the decoder logits and frame-level on the CTC head (csrc/distill.hip);
  * `--transducer-weight r` (+ `--transducer-dim-joint`, `--transducer-context`; train.py): a transducer (RNN-T) head on the encoder
    output, L = (1 - r) L_existing + r L_rnnt (csrc/rnnt.hip); `--transducer-greedy` (+ `--transducer-max-symbols`;
    test.py): time-synchronous greedy decoding from that head alone; `--transducer-beam-search` (+ `--beam-width`, `--beam-nbest`,
    `--transducer-candidates`, `--transducer-max-symbols`, `--lm-rescoring`; test.py): beam search over that head, one fused search
    kernel per utterance (csrc/rnnt_beam.hip); `--transducer-ngram-path FILE` (+ `--transducer-ngram-weight`,
    `--transducer-ngram-length-bonus`) and `--transducer-context-path FILE` (+ `--transducer-context-score`; test.py
    --transducer-beam-search): the n-gram LM and the phrase list fused into that search's pruning;
  * `--transducer-prune-range S` (+ `--transducer-simple-scale c`; train.py with --transducer-weight > 0): pruned transducer training, the
    joint and the loss on a band of S label positions per frame chosen by a simple joiner am + lm, L_rnnt = L_pruned + c L_simple
    (csrc/rnnt_pruned.hip).
"""
import argparse
import os
import sys

import torch

# (flags, kwargs) -- one row per option of the reference CLI, grouped as in its --help
_S, _I, _F = str, int, float


def _speed_factor(text):
    """One --speed-perturb factor, rounded to thousandths; outside [0.5, 2.0] the command line is refused."""
    f = round(float(text) * 1000.0) / 1000.0
    if not 0.5 <= f <= 2.0:
        raise argparse.ArgumentTypeError("--speed-perturb %s: a speed factor lies in [0.5, 2.0]" % text)
    return f


def _probability(text):
    """--rir-prob: a probability in [0, 1]."""
    p = float(text)
    if not 0.0 <= p <= 1.0:
        raise argparse.ArgumentTypeError("%s: a probability lies in [0, 1]" % text)
    return p


def _positive(text):
    """--rir-max-ms: a number above 0."""
    v = float(text)
    if not v > 0.0:
        raise argparse.ArgumentTypeError("%s: must be above 0" % text)
    return v


_FLAGS = [
    # experiment
    (("--model",), dict(default="TRFS", type=_S)), (("--name",), dict(default="model")),
    # data
    (("--train-manifest-list",), dict(nargs="+", type=_S)), (("--valid-manifest-list",), dict(nargs="+", type=_S)),
    (("--test-manifest-list",), dict(nargs="+", type=_S)), (("--lang-list",), dict(nargs="+", type=_S)),
    (("--sample-rate",), dict(default=16000, type=_I)), (("--batch-size",), dict(default=20, type=_I)),
    (("--num-workers",), dict(default=4, type=_I)), (("--labels-path",), dict(default="labels.json")),
    (("--label-smoothing",), dict(default=0.0, type=_F)),
    (("--window-size",), dict(default=0.02, type=_F)), (("--window-stride",), dict(default=0.01, type=_F)),
    (("--window",), dict(default="hamming")),
    # run control
    (("--epochs",), dict(default=1000, type=_I)), (("--cuda",), dict(dest="cuda", action="store_true")),
    (("--device-ids",), dict(default=None, nargs="+", type=_I)), (("--lr", "--learning-rate"), dict(default=3e-4, type=_F)),
    (("--save-every",), dict(default=5, type=_I)), (("--save-folder",), dict(default="models/")),
    (("--emb_trg_sharing",), dict(action="store_true")), (("--feat_extractor",), dict(default="vgg_cnn", type=_S)),
    (("--verbose",), dict(action="store_true")), (("--continue-from",), dict(default="")),
    # augmentation
    (("--augment",), dict(dest="augment", action="store_true")), (("--noise-dir",), dict(default=None)),
    (("--noise-prob",), dict(default=0.4)), (("--noise-min",), dict(default=0.0, type=_F)),
    (("--noise-max",), dict(default=0.5, type=_F)),
    # speed perturbation on the GPU front end: every training utterance is resampled by one of these factors, drawn
    # uniformly, e.g. 0.9 1.0 1.1; each is rounded to thousandths and must lie in [0.5, 2.0]; default: off
    (("--speed-perturb",), dict(default=None, nargs="+", type=_speed_factor, metavar="F")),
    # reverberation on the GPU front end: with probability --rir-prob a training utterance is convolved with one of
    # the room impulse responses (*.wav at --sample-rate) under --rir-dir, each cut to --rir-max-ms behind its direct path; default: off
    (("--rir-dir",), dict(default=None)), (("--rir-prob",), dict(default=0.5, type=_probability)),
    (("--rir-max-ms",), dict(default=500.0, type=_positive)),
    # SpecAugment on the GPU front end; defaults: the LibriSpeech "LD" policy of arXiv:1904.08779 (W 80, F 27,
    # mF 2, T 100, p 1.0, mT 2) -- on the 161 linear bins of --features spect; --features fbank gives the paper's 80 mel bins
    (("--spec-augment",), dict(action="store_true")), (("--spec-time-warp",), dict(default=80, type=_I)),
    (("--spec-freq-mask",), dict(default=27, type=_I)), (("--spec-freq-masks",), dict(default=2, type=_I)),
    (("--spec-time-mask",), dict(default=100, type=_I)), (("--spec-time-masks",), dict(default=2, type=_I)),
    (("--spec-time-mask-ratio",), dict(default=1.0, type=_F)),
    # feature type: spect = the reference's linear bins; fbank = log-mel filterbank energies of the same STFT
    (("--features",), dict(default="spect", choices=["spect", "fbank"])), (("--num-mel-bins",), dict(default=80, type=_I)),
    (("--mel-fmin",), dict(default=20.0, type=_F)),
    # model
    (("--num-layers",), dict(default=3, type=_I)), (("--num-heads",), dict(default=5, type=_I)),
    (("--dim-model",), dict(default=512, type=_I)), (("--dim-key",), dict(default=64, type=_I)),
    (("--dim-value",), dict(default=64, type=_I)), (("--dim-input",), dict(default=161, type=_I)),
    (("--dim-inner",), dict(default=1024, type=_I)), (("--dim-emb",), dict(default=512, type=_I)),
    (("--src-max-len",), dict(default=4000, type=_I)), (("--tgt-max-len",), dict(default=1000, type=_I)),
    # optimiser
    (("--warmup",), dict(default=4000, type=_I)), (("--min-lr",), dict(default=1e-5, type=_F)),
    (("--k-lr",), dict(default=1, type=_F)), (("--momentum",), dict(default=0.9, type=_F)),
    (("--lr-anneal",), dict(default=1.1, type=_F)),
    # decoding
    (("--beam-search",), dict(action="store_true")), (("--beam-width",), dict(default=3, type=_I)),
    (("--beam-nbest",), dict(default=5, type=_I)), (("--lm-rescoring",), dict(action="store_true")),
    (("--lm-path",), dict(type=_S, default="lm_model.pt")), (("--lm-weight",), dict(default=0.1, type=_F)),
    (("--c-weight",), dict(default=0.1, type=_F)), (("--prob-weight",), dict(default=1.0, type=_F)),
    # joint CTC / attention.  --ctc-weight w (train.py): an encoder CTC head, L = (1 - w) CE + w CTC; 0 = no head.
    # --ctc-decode-weight m (test.py --beam-search): beam candidates ranked by (1 - m) attention + m CTC prefix score, the
    # --ctc-candidates (0: min(V, 16, 2 * beam width)) best attention candidates of a hypothesis scored; --ctc-greedy: best-path
    # decoding from the CTC head alone
    (("--ctc-weight",), dict(default=0.0, type=_F)), (("--ctc-decode-weight",), dict(default=0.0, type=_F)),
    (("--ctc-candidates",), dict(default=0, type=_I)), (("--ctc-greedy",), dict(action="store_true")),
    # minimum word error rate training over the CTC n-best (train.py, after --continue-from).  --mwer-weight m in
    # (0, 1]: L = m * expected errors above the list's mean + (1 - m) * [(1 - w) NLL + w CTC] with w = --ctc-weight > 0; the n-best = the
    # --mwer-nbest (2..16) survivors of the CTC prefix beam search (--ctc-candidates labels per frame), rescored by the decoder WITH grad;
    # --mwer-unit: errors counted over label ids or over the words between space labels.  0 = off: nothing new is built or launched
    (("--mwer-weight",), dict(default=0.0, type=_F)), (("--mwer-nbest",), dict(default=4, type=_I)),
    (("--mwer-unit",), dict(default="label", choices=["label", "word"])),
    # knowledge distillation from a teacher checkpoint (train.py; csrc/distill.hip).  --distill-from PATH: the
    # teacher, frozen, run on every training batch; --distill-weight a in [0, 1]: L_att = (1 - a) CE + a KD on the decoder logits, KD =
    # tau^2 KL(teacher || student) at --distill-temperature tau in [0.5, 16]; --distill-ctc-weight c in [0, 1] (with --ctc-weight w > 0):
    # the CTC term becomes (1 - c) CTC + c KD over the CTC heads' frames.  Everything off: no teacher is built, nothing new is launched
    (("--distill-from",), dict(default=None, type=_S)), (("--distill-weight",), dict(default=0.0, type=_F)),
    (("--distill-ctc-weight",), dict(default=0.0, type=_F)), (("--distill-temperature",), dict(default=2.0, type=_F)),
    # transducer (RNN-T) head (csrc/rnnt.hip).  --transducer-weight r in [0, 1] (train.py): L = (1 - r) L_existing + r
    # L_rnnt, L_existing = CE or the --ctc-weight joint loss, L_rnnt = mean_b nll_b / max(U_b, 1) over the T'_b x (U_b + 1) lattice, blank =
    # PAD; 0 = no head: nothing new is built or launched.  --transducer-dim-joint J (a multiple of 8): the joint's width;
    # --transducer-context C in {1, 2}: the labels the stateless predictor looks back.  --transducer-greedy (test.py): time-synchronous
    # greedy search from the head alone, at most --transducer-max-symbols labels per frame.  --transducer-beam-search (test.py): beam
    # search from the head alone (csrc/rnnt_beam.hip): --beam-width (1..16) hypotheses, --transducer-candidates K (0: min(V - 1, 16)) labels
    # tried per hypothesis and step, --transducer-max-symbols labels per frame, the --beam-nbest best re-ranked like a decoder beam's
    (("--transducer-weight",), dict(default=0.0, type=_F)), (("--transducer-dim-joint",), dict(default=256, type=_I)),
    (("--transducer-context",), dict(default=2, type=_I)), (("--transducer-greedy",), dict(action="store_true")),
    (("--transducer-max-symbols",), dict(default=5, type=_I)), (("--transducer-beam-search",), dict(action="store_true")),
    (("--transducer-candidates",), dict(default=0, type=_I)),
    # pruned transducer training (csrc/rnnt_pruned.hip; Kuang et al. 2022).  --transducer-prune-range S (train.py;
    # 0 = off: the model, its state_dict keys, its launches and the bits of its loss are those of the full lattice; otherwise 2..64, and
    # --transducer-weight must be positive): two more layers, rnnt_simple_am (D -> V, on the encoder output) and rnnt_simple_lm (J -> V,
    # on the predictor), whose sum is a joiner without a (T', U+1, V) tensor; the posteriors of ITS lattice choose, per frame, a window of
    # min(S, U+1) label positions, and rnnt_enc / tanh / rnnt_out and the transducer loss run on that band only: logits (B,T',S,V)
    # instead of (B,T',U+1,V).  L_rnnt = L_pruned + c L_simple with --transducer-simple-scale c >= 0 (default 0.5), each a mean_b nll_b /
    # max(U_b, 1).  The band is a constant of the step (no gradient through it).  No am-only / lm-only smoothing term and no warm-up
    # schedule of c.  Decoding (test.py) ignores the two simple layers.
    (("--transducer-prune-range",), dict(default=0, type=_I)), (("--transducer-simple-scale",), dict(default=0.5, type=_F)),
    # --ctc-beam-search (test.py): prefix beam search over the CTC head's posteriors alone (csrc/ctc_beam.hip): --beam-width (1..16)
    # prefixes kept per frame, --ctc-candidates (0: min(V, 16)) labels tried per frame, the n-best ranked like --beam-search's
    (("--ctc-beam-search",), dict(action="store_true")),
    # --attention-rescoring-weight l (test.py --ctc-beam-search): the decoder scores all --beam-width hypotheses of the
    # CTC search in one teacher-forced pass and they are ranked by (1 - l) CTC + l attention log-probability; 0 = off, no decoder pass
    (("--attention-rescoring-weight",), dict(default=0.0, type=_F)),
    # --ngram-path FILE (test.py --ctc-beam-search): a label n-gram LM of train_ngram.py, fused into the search's
    # pruning with --ngram-weight and a bonus of --ngram-length-bonus per label; without the path nothing changes
    (("--ngram-path",), dict(type=_S, default=None)), (("--ngram-weight",), dict(default=0.3, type=_F)),
    (("--ngram-length-bonus",), dict(default=0.0, type=_F)),
    # --context-path FILE (test.py --ctc-beam-search): phrase (hotword) biasing -- one phrase per line in the model's
    # labels; every label that advances a listed phrase adds --context-score to a prefix' pruning key, a phrase that breaks off gives it
    # back; combines with --ngram-path, --attention-rescoring-weight and --lm-rescoring; without the path nothing changes
    (("--context-path",), dict(type=_S, default=None)), (("--context-score",), dict(default=3.0, type=_F)),
    # --transducer-ngram-path / --transducer-context-path FILE (test.py --transducer-beam-search): the same two
    # structures fused into the transducer beam search's pruning, with weights of their own (a transducer's blank-heavy posteriors want
    # other values than CTC's; the defaults are the CTC flags' and are not tuned); without the paths nothing changes
    (("--transducer-ngram-path",), dict(type=_S, default=None)), (("--transducer-ngram-weight",), dict(default=0.3, type=_F)),
    (("--transducer-ngram-length-bonus",), dict(default=0.0, type=_F)),
    (("--transducer-context-path",), dict(type=_S, default=None)), (("--transducer-context-score",), dict(default=3.0, type=_F)),
    # CTC forced alignment (test.py): --align-out PATH writes one JSON line per test utterance with label and word
    # timestamps from the CTC head; --align-source gold aligns the transcript, hyp the label ids the decoder produced
    (("--align-out",), dict(default=None, type=_S)), (("--align-source",), dict(default="gold", choices=["gold", "hyp"])),
    # Conformer-style convolution module: K odd in 3..31 gives every encoder layer a conv_module (GLU, depthwise
    # convolution over K frames, Swish between two pointwise layers) between self_attn and pos_ffn; 0 = none.  Not with --rank
    (("--conv-module-kernel",), dict(default=0, type=_I)),
    # position signal of the encoder: abs = the reference's sinusoid added after the input projection; rope = rotary
    # position embedding of Q and K in every encoder self-attention and no sinusoid.  Needs --dim-key == --dim-value in {16, 32, 64}; not with --rank
    (("--pos-encoding",), dict(default="abs", choices=["abs", "rope"])),
    # loss / regularisation
    (("--loss",), dict(type=_S, default="ce")), (("--clip",), dict(action="store_true")),
    (("--max-norm",), dict(default=400, type=_F)), (("--dropout",), dict(default=0.1, type=_F)),
    (("--parallel",), dict(action="store_true")), (("--shuffle",), dict(action="store_true")),
    # MI355X path (additions)
    # fp8: bf16 storage, fp8 (e4m3) MFMA for the forward --rank projections -- functional, SLOWER than bf16 (22.97 vs 12.55 ms per step
    # of configs[4]: quantisation passes around K = 64 contractions); parity unpinned (no reference code for the low-rank variant)
    (("--precision",), dict(default="bf16", choices=["bf16", "fp32", "fp8"],
                            help="bf16 (default) | fp32 (parity mode) | fp8 (low-rank projections only; functional, slower than bf16)")),
    (("--dist-backend",), dict(default="nccl")), (("--bucket-mb",), dict(default=32.0, type=_F)),
    (("--grad-wire",), dict(default="fp32", choices=["fp32", "bf16"])),
    (("--gpu-frontend",), dict(action="store_true")),
    # 0: eager launches on the batch exactly as collated.  N > 0: training batches are zero-padded along time to a multiple of N
    # frames (the way the collate function pads shorter utterances) and to --tgt-max-len - 1 target columns, and the step is a
    # captured hipGraph per (batch, frames) shape, replayed (trainer/asr/trainer.py)
    (("--graph-buckets",), dict(default=0, type=_I,
                                help="0: eager launches; N > 0: hipGraph replay per (batch, frames padded to a multiple of N) shape. Default: 64 for a "
                                     "vgg_cnn model with --cuda and the CE loss (decided from the MODEL, after --continue-from is resolved), else 0. "
                                     "Parity caveat: the longest utterance of a batch sees zero frames instead of the image border behind its "
                                     "last frame (as every shorter one already does through the collate padding)")),
    # data parallel under graph replay: `four` = four hipGraphs with the RCCL all-reduces between them (ordering proven under two ranks);
    # `one` = the collectives captured inside ONE hipGraph; `auto` = try one, verify its first replayed step against the four-graph
    # step's loss and gradient checksum on the same batch, fall back LOUDLY (asr_hip/graph.py)
    (("--ddp-graph",), dict(default="auto", choices=["one", "four", "auto"])),
    # Low-Rank Transformer (arXiv:1910.13923, BASELINE configs[4]): rank of every attention / feed-forward projection, 0 = full rank
    (("--rank",), dict(default=0, type=_I)),
]

parser = argparse.ArgumentParser(description="Transformer ASR on MI355X")
for _names, _kw in _FLAGS:
    parser.add_argument(*_names, **_kw)

# same global seeding as the reference (constant.py:96-97) so `--continue-from`-less runs start from the same init
torch.manual_seed(123456)
if torch.cuda.is_available():
    torch.cuda.manual_seed_all(123456)


def _given(argv):
    """Destinations of the options that appear on this command line (as opposed to argparse defaults)."""
    out = set()
    for act in parser._actions:
        if any(tok == o or tok.startswith(o + "=") for o in act.option_strings for tok in argv):
            out.add(act.dest)
    return out


def parse(argv):
    """Parse an explicit argv (list of strings) into the process-global Namespace."""
    global args, USE_CUDA, explicit
    args = parser.parse_args(argv)
    explicit = _given(list(argv))
    USE_CUDA = args.cuda
    return args


def set_args(ns):
    global args, USE_CUDA
    args = ns
    USE_CUDA = getattr(ns, "cuda", False)
    return args


_entry = os.path.basename(sys.argv[0]) if sys.argv and sys.argv[0] else ""
args = parser.parse_args(sys.argv[1:] if _entry in ("train.py", "test.py") else [])
explicit = _given(sys.argv[1:] if _entry in ("train.py", "test.py") else [])      # options the user actually typed (load_model)
USE_CUDA = args.cuda

PAD_TOKEN, SOS_TOKEN, EOS_TOKEN = 0, 1, 2
PAD_CHAR, SOS_CHAR, EOS_CHAR = "\u00b6", "\u00a7", "\u00a4"
