"""Evaluation entry point -- same command line as the reference (reference: test.py): loads --continue-from, decodes
every test utterance (greedy, beam search with --beam-search, from the transducer head alone with --transducer-greedy /
--transducer-beam-search, or from the encoder
CTC head alone with --ctc-greedy / --ctc-beam-search,
the latter's n-best rescored by the decoder with --attention-rescoring-weight, its pruning guided by a label n-gram LM with --ngram-path and biased towards the phrases of --context-path;
--transducer-ngram-path and --transducer-context-path do the same for --transducer-beam-search)
and reports CER / WER.  --align-out PATH also writes label and word
timestamps from the encoder CTC head (forced alignment of the transcript, or of the hypothesis with --align-source hyp)."""
import torch
from tqdm import tqdm

from utils import constant
from utils.metrics import calculate_cer, calculate_cer_en_zh, calculate_wer


def evaluate(model, test_loader, lm=None, noise_dir=None, ngram=None, context=None, transducer_ngram=None, transducer_context=None):
    """reference: test.py:19-62.  noise_dir: the checkpoint's --noise-dir (the reference injects noise into the test set too); ngram: the
    NgramLM of --ngram-path, context: the ContextGraph of --context-path (None: the plain search, no table and no further launch);
    transducer_ngram / transducer_context: those of --transducer-ngram-path / --transducer-context-path, for --transducer-beam-search."""
    args = constant.args
    fusion = {} if ngram is None else dict(ngram=ngram, ngram_weight=getattr(args, "ngram_weight", 0.3),
                                           length_bonus=getattr(args, "ngram_length_bonus", 0.0))
    if context is not None:
        fusion.update(context=context, context_score=getattr(args, "context_score", 3.0))
    if transducer_ngram is not None:
        fusion.update(transducer_ngram=transducer_ngram, transducer_ngram_weight=getattr(args, "transducer_ngram_weight", 0.3),
                      transducer_length_bonus=getattr(args, "transducer_ngram_length_bonus", 0.0))
    if transducer_context is not None:
        fusion.update(transducer_context=transducer_context, transducer_context_score=getattr(args, "transducer_context_score", 3.0))
    model.eval()
    total_word = total_char = total_cer = total_wer = 0
    total_en_cer = total_zh_cer = total_en_char = total_zh_char = 0
    align_source = getattr(args, "align_source", "gold") if getattr(args, "align_out", None) else None
    writer = None
    if align_source is not None:      # --align-out: label and word timestamps from the CTC head, one JSON line per utterance
        from utils.align import AlignmentWriter, utterance_record
        check_ctc_decoding(args, model)
        writer = AlignmentWriter(args.align_out)
    with torch.no_grad():
        pbar = tqdm(iter(test_loader), leave=True, total=len(test_loader))
        for data in pbar:
            src, tgt, _, src_lengths, tgt_lengths = data[:5]
            aug = data[5] if len(data) > 5 else None      # noise draws when the checkpoint's run injected noise
            if constant.USE_CUDA:
                src, tgt = src.cuda(), tgt.cuda()
            if getattr(args, "gpu_frontend", False):
                from utils.audio import gpu_front_end
                src, src_lengths = gpu_front_end(src, src_lengths, args.sample_rate, args.window_size, args.window_stride,
                                                 args.src_max_len, window=getattr(args, "window", "hamming"), aug=aug,
                                                 noise_dir=noise_dir, features=getattr(args, "features", "spect"),
                                                 num_mel_bins=getattr(args, "num_mel_bins", 80),
                                                 mel_fmin=getattr(args, "mel_fmin", 20.0))
            align = {} if writer is None else dict(align_source=align_source, target_lengths=tgt_lengths)
            _, strs_hyps, strs_gold, *alignment = model.evaluate(src, src_lengths, tgt, beam_search=args.beam_search,
                                                                 beam_width=args.beam_width, beam_nbest=args.beam_nbest, lm=lm,
                                                                 lm_rescoring=args.lm_rescoring, lm_weight=args.lm_weight,
                                                                 c_weight=args.c_weight, verbose=args.verbose,
                                                                 ctc_weight=getattr(args, "ctc_decode_weight", 0.0),
                                                                 ctc_candidates=getattr(args, "ctc_candidates", 0),
                                                                 ctc_greedy=getattr(args, "ctc_greedy", False),
                                                                 ctc_beam=getattr(args, "ctc_beam_search", False),
                                                                 attention_rescoring_weight=getattr(args, "attention_rescoring_weight", 0.0),
                                                                 **align, **fusion, **transducer_decoding(args))
            for i, (hyp, gold) in enumerate(zip(strs_hyps, strs_gold)):
                for ch in (constant.EOS_CHAR, constant.SOS_CHAR, constant.PAD_CHAR):
                    hyp, gold = hyp.replace(ch, ""), gold.replace(ch, "")
                if writer is not None:
                    writer.write(utterance_record(writer.count, gold if align_source == "gold" else hyp, alignment[0][i],
                                                  model.feat_extractor, args.window_stride, int(src_lengths[i])))
                total_wer += calculate_wer(hyp, gold)
                total_cer += calculate_cer(hyp.strip(), gold.strip())
                en_cer, zh_cer, n_en, n_zh = calculate_cer_en_zh(hyp, gold)
                total_en_cer += en_cer; total_zh_cer += zh_cer; total_en_char += n_en; total_zh_char += n_zh
                total_word += len(gold.split(" "))
                total_char += len(gold)
            pbar.set_description("TEST CER:{:.2f}% WER:{:.2f}% CER_EN:{:.2f}% CER_ZH:{:.2f}%".format(
                total_cer * 100 / max(1, total_char), total_wer * 100 / max(1, total_word),
                total_en_cer * 100 / max(1, total_en_char), total_zh_cer * 100 / max(1, total_zh_char)))
    if writer is not None:
        writer.close()
    return total_cer / max(1, total_char), total_wer / max(1, total_word)


def check_ctc_decoding(args, model):
    """--ctc-decode-weight / --ctc-greedy / --ctc-beam-search / --align-out need the encoder CTC head of a model trained with
    --ctc-weight > 0; the weight lies in [0, 1] and applies to --beam-search.  --ctc-beam-search decodes from the head alone: it excludes
    --beam-search, --ctc-greedy and a --ctc-decode-weight, and its --beam-width lies in 1..16.  --attention-rescoring-weight lies in
    [0, 1] and applies to --ctc-beam-search, as do --ngram-path and --context-path."""
    w = float(getattr(args, "ctc_decode_weight", 0.0) or 0.0)
    if not 0.0 <= w <= 1.0:
        raise ValueError("--ctc-decode-weight must lie in [0, 1], got %g" % w)
    ctc_beam = getattr(args, "ctc_beam_search", False)
    lam = float(getattr(args, "attention_rescoring_weight", 0.0) or 0.0)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("--attention-rescoring-weight must lie in [0, 1], got %g" % lam)
    if lam > 0 and not ctc_beam:
        raise ValueError("--attention-rescoring-weight %g needs --ctc-beam-search: the decoder rescores the CTC search's n-best" % lam)
    if getattr(args, "ngram_path", None) and not ctc_beam:
        raise ValueError("--ngram-path needs --ctc-beam-search: the n-gram LM is fused into the CTC prefix beam search")
    if getattr(args, "context_path", None) and not ctc_beam:
        raise ValueError("--context-path needs --ctc-beam-search: the phrase list biases the CTC prefix beam search's pruning")
    if ((w > 0 or getattr(args, "ctc_greedy", False) or ctc_beam or getattr(args, "align_out", None))
            and not hasattr(model, "ctc_linear")):
        raise ValueError("--ctc-decode-weight / --ctc-greedy / --ctc-beam-search / --align-out need a model with an encoder CTC head: "
                         "this checkpoint was trained with --ctc-weight 0")
    if ctc_beam:
        for flag, on in (("--beam-search", getattr(args, "beam_search", False)), ("--ctc-greedy", getattr(args, "ctc_greedy", False)),
                         ("--ctc-decode-weight %g" % w, w > 0)):
            if on:
                raise ValueError("--ctc-beam-search decodes from the CTC head alone: it cannot be combined with %s" % flag)
        if not 1 <= int(args.beam_width) <= 16:
            raise ValueError("--ctc-beam-search keeps --beam-width prefixes per frame in the kernel's beam: 1..16, got %d"
                             % int(args.beam_width))
        c = int(getattr(args, "ctc_candidates", 0) or 0)
        if not 0 <= c <= 16:
            raise ValueError("--ctc-candidates must lie in 0..16 with --ctc-beam-search (0: min(V, 16)), got %d" % c)
    if w > 0 and not getattr(args, "beam_search", False):
        raise ValueError("--ctc-decode-weight %g needs --beam-search: CTC prefix scores re-rank beam candidates" % w)


def transducer_decoding(args):
    """The evaluate() arguments of --transducer-greedy / --transducer-beam-search (empty without either flag: the call is the one it
    was)."""
    if getattr(args, "transducer_beam_search", False):
        return dict(transducer_beam=True, transducer_max_symbols=int(getattr(args, "transducer_max_symbols", 5)),
                    transducer_candidates=int(getattr(args, "transducer_candidates", 0) or 0))
    if not getattr(args, "transducer_greedy", False):
        return {}
    return dict(transducer_greedy=True, transducer_max_symbols=int(getattr(args, "transducer_max_symbols", 5)))


def check_transducer_decoding(args, model):
    """--transducer-greedy / --transducer-beam-search need the transducer head of a model trained with --transducer-weight > 0, decode
    from that head alone (no --beam-search, --ctc-greedy, --ctc-beam-search, --ctc-decode-weight, --attention-rescoring-weight,
    --ngram-path, --context-path or --align-out, and not each other) and emit 1 <= --transducer-max-symbols labels per frame at the most.
    --transducer-beam-search keeps --beam-width in 1..16 hypotheses and tries --transducer-candidates in 0..16 labels (0: min(V - 1, 16)).
    --transducer-ngram-path and --transducer-context-path need --transducer-beam-search (--transducer-greedy does not take them).
    Without any of these flags nothing is checked.  All of it before any launch."""
    greedy, beam = getattr(args, "transducer_greedy", False), getattr(args, "transducer_beam_search", False)
    if getattr(args, "transducer_ngram_path", None) and not beam:
        raise ValueError("--transducer-ngram-path needs --transducer-beam-search: the n-gram LM is fused into the transducer beam search")
    if getattr(args, "transducer_context_path", None) and not beam:
        raise ValueError("--transducer-context-path needs --transducer-beam-search: the phrase list biases the transducer beam search's "
                         "pruning")
    if not greedy and not beam:
        return
    name = "--transducer-beam-search" if beam else "--transducer-greedy"
    if not hasattr(model, "rnnt_out"):
        raise ValueError("%s needs a model with a transducer head: this checkpoint was trained with --transducer-weight 0" % name)
    for flag, on in (("--transducer-greedy", beam and greedy),
                     ("--beam-search", getattr(args, "beam_search", False)), ("--ctc-greedy", getattr(args, "ctc_greedy", False)),
                     ("--ctc-beam-search", getattr(args, "ctc_beam_search", False)),
                     ("--ctc-decode-weight", float(getattr(args, "ctc_decode_weight", 0.0) or 0.0) > 0),
                     ("--attention-rescoring-weight", float(getattr(args, "attention_rescoring_weight", 0.0) or 0.0) > 0),
                     ("--ngram-path", bool(getattr(args, "ngram_path", None))), ("--context-path", bool(getattr(args, "context_path", None))),
                     ("--align-out", bool(getattr(args, "align_out", None)))):
        if on:
            raise ValueError("%s decodes from the transducer head alone: it cannot be combined with %s" % (name, flag))
    if int(getattr(args, "transducer_max_symbols", 5)) < 1:
        raise ValueError("--transducer-max-symbols must be at least 1, got %d" % int(args.transducer_max_symbols))
    if beam:
        if not 1 <= int(args.beam_width) <= 16:
            raise ValueError("--transducer-beam-search keeps --beam-width hypotheses in the kernel's beam: 1..16, got %d"
                             % int(args.beam_width))
        k = int(getattr(args, "transducer_candidates", 0) or 0)
        if not 0 <= k <= 16:
            raise ValueError("--transducer-candidates must lie in 0..16 with --transducer-beam-search (0: min(V - 1, 16)), got %d" % k)
        if int(args.beam_width) * (int(args.transducer_max_symbols) + 1) > 1024:
            raise ValueError("--transducer-beam-search: --beam-width * (--transducer-max-symbols + 1) must not exceed 1024, got %d * %d"
                             % (int(args.beam_width), int(args.transducer_max_symbols) + 1))


def feature_conf(loaded_args):
    """The audio_conf of a checkpoint's run: the features the model was trained on (its window and --features settings; load_model has
    filled in `spect` for a checkpoint from before --features and copied the three settings into constant.args for evaluate())."""
    from utils.audio import feature_settings
    features, num_mel_bins, mel_fmin = feature_settings(loaded_args)
    return dict(sample_rate=loaded_args.sample_rate, window_size=loaded_args.window_size, window_stride=loaded_args.window_stride,
                window=getattr(loaded_args, "window", "hamming"), noise_dir=loaded_args.noise_dir, noise_prob=loaded_args.noise_prob,
                noise_levels=(loaded_args.noise_min, loaded_args.noise_max), features=features, num_mel_bins=num_mel_bins,
                mel_fmin=mel_fmin)


if __name__ == '__main__':
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    from utils.functions import load_model
    from utils.lstm_utils import LM
    args = constant.args
    model, opt, epoch, metrics, loaded_args, label2id, id2label = load_model(args.continue_from)
    if getattr(loaded_args, "parallel", False):
        print("unwrap data parallel")
        model = model.module
    check_transducer_decoding(args, model)
    check_ctc_decoding(args, model)
    constant.args.tgt_max_len = max(constant.args.tgt_max_len, 301)      # greedy/beam search always run 300 steps
    if getattr(loaded_args, "noise_dir", None) is not None and args.cuda and not args.gpu_frontend:
        args.gpu_frontend = True                # noise injection runs on the GPU front end (utils/audio.py)
        print("--noise-dir of the checkpoint: noise injection on the GPU front end (--gpu-frontend turned on)")
    args.window = getattr(loaded_args, "window", "hamming")      # the features the model was trained on
    audio_conf = feature_conf(loaded_args)
    test_data = SpectrogramDataset(audio_conf=audio_conf, manifest_filepath_list=args.test_manifest_list, label2id=label2id,
                                   normalize=True, augment=False)
    test_sampler = BucketingSampler(test_data, batch_size=args.batch_size)
    test_loader = AudioDataLoader(test_data, num_workers=args.num_workers, batch_sampler=test_sampler)
    lm = LM(args.lm_path) if args.lm_rescoring else None      # reference: test.py:91-93
    ngram = None
    if getattr(args, "ngram_path", None):     # --ctc-beam-search only (check_ctc_decoding); a file for other labels is refused here
        from utils.ngram import NgramLM
        ngram = NgramLM.load(args.ngram_path, id2label)
    context = None
    if getattr(args, "context_path", None):   # --ctc-beam-search only (check_ctc_decoding); a character that is no label is refused here
        from utils.context import ContextGraph
        context = ContextGraph.from_file(args.context_path, label2id)
    fused = {}
    if getattr(args, "transducer_ngram_path", None):      # --transducer-beam-search only (check_transducer_decoding)
        from utils.ngram import NgramLM
        fused["transducer_ngram"] = NgramLM.load(args.transducer_ngram_path, id2label)
    if getattr(args, "transducer_context_path", None):
        from utils.context import ContextGraph
        fused["transducer_context"] = ContextGraph.from_file(args.transducer_context_path, label2id)
    print(model)
    evaluate(model, test_loader, lm=lm, noise_dir=getattr(loaded_args, "noise_dir", None), ngram=ngram, context=context, **fused)
