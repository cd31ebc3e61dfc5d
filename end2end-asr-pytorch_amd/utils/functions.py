"""Model / optimiser factories and checkpoint I/O with the reference's signatures and checkpoint schema
(reference: utils/functions.py).  Under --parallel the reference wraps the model in a single-process nn.DataParallel;
here every rank of a torch.distributed job owns one GPU and gradients are all-reduced over RCCL (asr_hip/ddp.py).
"""
import math
import os

import logging

import torch
import torch.distributed as dist

from asr_hip import ops
from asr_hip import params as P
from asr_hip.ddp import HipDataParallel
from models.asr.transformer import Decoder, Encoder, Transformer
from models.common_layers import check_conv_module_kernel, check_pos_encoding
from utils import constant
from utils.audio import feature_bins, feature_settings
from utils.optimizer import AnnealingOpt, FusedAdam, NoamOpt


def _unwrap(model):
    return model.module if isinstance(model, HipDataParallel) else model


def save_model(model, epoch, opt, metrics, label2id, id2label, best_model=False):
    """Same file names and dict keys as the reference (functions.py:11-59).  Only rank 0 writes."""
    if dist.is_initialized() and dist.get_rank() != 0:
        return
    folder = os.path.join(constant.args.save_folder, constant.args.name)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, "best_model.th" if best_model else "epoch_{}.th".format(epoch))
    print("SAVE MODEL to", path)
    ckpt = {
        'label2id': label2id, 'id2label': id2label, 'args': constant.args, 'epoch': epoch,
        'model_state_dict': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
        'optimizer_state_dict': opt.optimizer.state_dict(),
        'optimizer_params': {'_step': opt._step, '_rate': opt._rate, 'warmup': opt.warmup, 'factor': opt.factor,
                             'model_size': opt.model_size},
        'metrics': metrics,
    }
    torch.save(ckpt, path)


def load_model(load_path):
    """-> (model, opt, epoch, metrics, args, label2id, id2label)   (reference: functions.py:62-98)"""
    ckpt = torch.load(load_path, map_location="cpu", weights_only=False)
    args = ckpt.get('args', constant.args)
    cur = constant.args
    if args is not cur:
        # What describes THIS run, not the run that wrote the file, comes from the current command line: how the job is
        # laid out over GPUs (the reference re-wraps according to the current --parallel, train.py:92-99; a checkpoint saved
        # without it must not silently train un-synchronised replicas), where it runs, and the MI355X-path switches a
        # reference-written checkpoint does not carry at all.
        for k in ("parallel", "device_ids", "dist_backend", "bucket_mb", "grad_wire"):
            if hasattr(cur, k):
                setattr(args, k, getattr(cur, k))
        # numerics switches: what the checkpoint was trained with stays, unless the user typed the option on THIS command line or
        # the (reference-written) checkpoint does not carry it -- an fp32-trained model must not silently resume in bf16
        for k in ("precision", "gpu_frontend"):
            if hasattr(cur, k) and (k in getattr(constant, "explicit", ()) or not hasattr(args, k)):
                if hasattr(args, k) and getattr(args, k) != getattr(cur, k):
                    logging.info("load_model: --%s %s from the command line overrides the checkpoint's %s", k.replace("_", "-"),
                                 getattr(cur, k), getattr(args, k))
                setattr(args, k, getattr(cur, k))
        args.cuda = bool(getattr(args, "cuda", False) or getattr(cur, "cuda", False))
        # the features the model was trained on are the checkpoint's (one written before --features existed: spect); typing another
        # feature setting on the command line of a resumed run is an error, not an override
        names = ("features", "num_mel_bins", "mel_fmin")
        kept = feature_settings(args)
        for k, v in zip(names, kept):
            if k in getattr(constant, "explicit", ()) and hasattr(cur, k) and getattr(cur, k) != v:
                raise ValueError("--%s %s on the command line, but %s was trained with --%s %s: the checkpoint's features cannot be "
                                 "changed" % (k.replace("_", "-"), getattr(cur, k), load_path, k.replace("_", "-"), v))
            setattr(args, k, v)
            setattr(cur, k, v)          # the loaders and the GPU front end of this run read the process-global Namespace
        # the encoder CTC head (--ctc-weight) is part of the model: a run resumes with the checkpoint's weight (one written before the
        # flag existed: 0, no head); an explicit --ctc-weight may replace a positive weight with another positive one (it only weighs
        # the loss), but cannot add or drop the head
        kept = float(getattr(args, "ctc_weight", 0.0) or 0.0)
        if "ctc_weight" in getattr(constant, "explicit", ()) and hasattr(cur, "ctc_weight") and float(cur.ctc_weight) != kept:
            check_ctc_weight(cur.ctc_weight)
            if (float(cur.ctc_weight) > 0) != (kept > 0):
                raise ValueError("--ctc-weight %g on the command line, but %s was trained with --ctc-weight %g: the encoder CTC head "
                                 "cannot be added to or dropped from a checkpoint" % (cur.ctc_weight, load_path, kept))
            logging.info("load_model: --ctc-weight %g from the command line replaces the checkpoint's %g", cur.ctc_weight, kept)
            kept = float(cur.ctc_weight)
        args.ctc_weight = kept
        cur.ctc_weight = kept           # the trainer of this run reads the process-global Namespace
        # the transducer head (--transducer-weight, with its --transducer-dim-joint and --transducer-context) follows the same rule: the
        # checkpoint's settings rebuild it (one written before the flags existed: 0, no head); another positive weight may replace a
        # positive one, the head can be neither added nor dropped, and its two sizes cannot be changed
        given = getattr(constant, "explicit", ())
        kept = float(getattr(args, "transducer_weight", 0.0) or 0.0)
        if "transducer_weight" in given and hasattr(cur, "transducer_weight") and float(cur.transducer_weight) != kept:
            if not 0.0 <= float(cur.transducer_weight) <= 1.0:
                raise ValueError("--transducer-weight must lie in [0, 1], got %g" % float(cur.transducer_weight))
            if (float(cur.transducer_weight) > 0) != (kept > 0):
                raise ValueError("--transducer-weight %g on the command line, but %s was trained with --transducer-weight %g: the "
                                 "transducer head cannot be added to or dropped from a checkpoint"
                                 % (cur.transducer_weight, load_path, kept))
            logging.info("load_model: --transducer-weight %g from the command line replaces the checkpoint's %g",
                         cur.transducer_weight, kept)
            kept = float(cur.transducer_weight)
        args.transducer_weight = kept
        cur.transducer_weight = kept
        for k, dflt in (("transducer_dim_joint", 256), ("transducer_context", 2)):
            v = int(getattr(args, k, dflt) or dflt)
            if kept > 0 and k in given and int(getattr(cur, k, dflt)) != v:
                raise ValueError("--%s %d on the command line, but %s was trained with --%s %d: a trained transducer head cannot be "
                                 "resized" % (k.replace("_", "-"), getattr(cur, k), load_path, k.replace("_", "-"), v))
            setattr(args, k, v)
            setattr(cur, k, v)
        # pruned transducer training (--transducer-prune-range S, --transducer-simple-scale c) follows the head's rule: S > 0 adds the two
        # simple layers to the model, so a positive S may replace a positive one (it only sizes the band), S can go neither from 0 to
        # positive nor back, and c only weighs the loss (a checkpoint written before the flags existed: 0 and 0.5)
        kept_s = int(getattr(args, "transducer_prune_range", 0) or 0)
        if "transducer_prune_range" in given and int(getattr(cur, "transducer_prune_range", 0) or 0) != kept_s:
            new_s = int(cur.transducer_prune_range or 0)
            check_prune_range(new_s)
            if new_s > 0 and kept_s == 0:
                raise ValueError("--transducer-prune-range %d on the command line, but %s was trained with --transducer-prune-range 0: "
                                 "the simple joiner's layers (rnnt_simple_am / rnnt_simple_lm) cannot be added to a checkpoint"
                                 % (new_s, load_path))
            if new_s == 0 and kept_s > 0:
                raise ValueError("--transducer-prune-range 0 on the command line, but %s was trained with --transducer-prune-range %d: "
                                 "the simple joiner's layers (rnnt_simple_am / rnnt_simple_lm) cannot be dropped from a checkpoint"
                                 % (load_path, kept_s))
            logging.info("load_model: --transducer-prune-range %d from the command line replaces the checkpoint's %d", new_s, kept_s)
            kept_s = new_s
        args.transducer_prune_range = kept_s
        cur.transducer_prune_range = kept_s
        kept_c = getattr(args, "transducer_simple_scale", None)
        kept_c = 0.5 if kept_c is None else float(kept_c)
        if "transducer_simple_scale" in given and hasattr(cur, "transducer_simple_scale"):
            kept_c = check_simple_scale(cur.transducer_simple_scale)
        args.transducer_simple_scale = kept_c
        cur.transducer_simple_scale = kept_c
        # the encoder's convolution modules (--conv-module-kernel) are part of the model too: the checkpoint's kernel size rebuilds them
        # (one written before the flag existed: 0, none); typing a different size is an error, never an override
        kept = int(getattr(args, "conv_module_kernel", 0) or 0)
        if "conv_module_kernel" in getattr(constant, "explicit", ()) and int(getattr(cur, "conv_module_kernel", 0) or 0) != kept:
            raise ValueError("--conv-module-kernel %d on the command line, but %s was trained with --conv-module-kernel %d: the encoder's "
                             "convolution modules cannot be added to, dropped from or resized in a checkpoint"
                             % (cur.conv_module_kernel, load_path, kept))
        args.conv_module_kernel = kept
        cur.conv_module_kernel = kept
        # and so is the encoder's position signal (--pos-encoding): the weights were trained with one of them (a checkpoint written before
        # the flag existed: abs)
        kept = str(getattr(args, "pos_encoding", None) or "abs")
        if "pos_encoding" in getattr(constant, "explicit", ()) and str(getattr(cur, "pos_encoding", None) or "abs") != kept:
            raise ValueError("--pos-encoding %s on the command line, but %s was trained with --pos-encoding %s: a trained encoder "
                             "cannot change its position signal" % (cur.pos_encoding, load_path, kept))
        args.pos_encoding = kept
        cur.pos_encoding = kept
    label2id, id2label = ckpt['label2id'], ckpt['id2label']
    model = init_transformer_model(args, label2id, id2label)
    sd = ckpt['model_state_dict']
    wrapped = isinstance(model, HipDataParallel)
    has_prefix = any(k.startswith("module.") for k in sd)
    if has_prefix and not wrapped:
        sd = {k[len("module."):]: v for k, v in sd.items()}
    elif wrapped and not has_prefix:
        sd = {"module." + k: v for k, v in sd.items()}
    model.load_state_dict(sd)
    if getattr(args, "cuda", False):
        model = model.cuda()
    opt = init_optimizer(args, model)
    if getattr(args, "parallel", False) and dist.is_initialized() and dist.get_world_size() > 1:
        assert opt.optimizer.reducer is not None, "--parallel with world_size > 1 needs the gradient reducer"
    if opt is not None:
        opt.optimizer.load_state_dict(ckpt['optimizer_state_dict'])
        op = ckpt['optimizer_params']
        opt._step, opt._rate, opt.warmup = op['_step'], op['_rate'], op['warmup']
        opt.factor, opt.model_size = op['factor'], op['model_size']
    return model, opt, ckpt['epoch'], ckpt['metrics'], args, label2id, id2label


def init_optimizer(args, model, opt_type="noam"):
    """Noam(model_size = args.dim_input AFTER init_transformer_model mutated it) over Adam(0.9, 0.98, 1e-9)
    (reference: functions.py:101-114).  Parameters are moved into one flat fp32 buffer; under --parallel a GradReducer
    is attached so that backward all-reduces gradient buckets as they complete."""
    if opt_type == "noam":
        core = _unwrap(model)
        bucket = int(getattr(args, "bucket_mb", 32.0) * (1 << 20)) if getattr(args, "parallel", False) else None
        adam = FusedAdam(list(core.parameters()), betas=(0.9, 0.98), eps=1e-9, ddp_bucket_bytes=bucket,
                         ddp_wire=getattr(args, "grad_wire", "fp32"))
        return NoamOpt(args.dim_input, args.k_lr, args.warmup, adam, min_lr=args.min_lr)
    if opt_type == "sgd":
        return AnnealingOpt(args.lr, args.lr_anneal, torch.optim.SGD(model.parameters(), lr=args.lr, momentum=args.momentum,
                                                                     nesterov=True))
    print("Optimizer is not defined")
    return None


def check_ctc_weight(w, args=None):
    """--ctc-weight must lie in [0, 1]; a positive weight (joint CTC / attention training) excludes --parallel
    (the token-mean CE and the utterance-mean CTC normalise differently under the gradient reducer's statistics slot) and --loss ctc
    (the reference's CTC on the DECODER output)."""
    w = float(w or 0.0)
    if not 0.0 <= w <= 1.0:
        raise ValueError("--ctc-weight must lie in [0, 1], got %g" % w)
    if w > 0 and args is not None:
        if getattr(args, "parallel", False):
            raise ValueError("--ctc-weight %g with --parallel is not supported: the cross-entropy loss is a mean over tokens and the "
                             "CTC loss a mean over utterances, and the data-parallel gradient reducer normalises by one of them" % w)
        if getattr(args, "loss", "ce") != "ce":
            raise ValueError("--ctc-weight %g with --loss %s is not supported: the weight combines the encoder CTC loss with the "
                             "cross-entropy loss (--loss ce)" % (w, args.loss))
    return w


def check_transducer_weight(args):
    """--transducer-weight r (a transducer head beside the decoder) -> r.  r must lie in [0, 1]; r > 0 checks
    --transducer-dim-joint (a positive multiple of 8) and --transducer-context (1 or 2) and excludes --parallel, --loss ctc,
    --mwer-weight > 0, --distill-from and --rank > 0.  r = 0: nothing is checked beyond the range."""
    r = float(getattr(args, "transducer_weight", 0.0) or 0.0)
    if not 0.0 <= r <= 1.0:
        raise ValueError("--transducer-weight must lie in [0, 1], got %g" % r)
    S = check_prune_range(getattr(args, "transducer_prune_range", 0))
    c = getattr(args, "transducer_simple_scale", None)
    check_simple_scale(0.5 if c is None else c)
    if S > 0 and r == 0.0:
        raise ValueError("--transducer-prune-range %d needs --transducer-weight > 0: it prunes the transducer head's lattice" % S)
    if r == 0.0:
        return r
    from models.asr.transformer import check_transducer
    check_transducer(getattr(args, "transducer_dim_joint", 256), getattr(args, "transducer_context", 2), getattr(args, "dim_model", None))
    if getattr(args, "parallel", False):
        raise ValueError("--transducer-weight %g with --parallel is not supported: the cross-entropy loss is a mean over tokens and the "
                         "transducer loss a mean over utterances, and the data-parallel gradient reducer normalises by one of them" % r)
    if getattr(args, "loss", "ce") != "ce":
        raise ValueError("--transducer-weight %g with --loss %s is not supported: the weight combines the transducer loss with the "
                         "cross-entropy loss (--loss ce)" % (r, args.loss))
    if float(getattr(args, "mwer_weight", 0.0) or 0.0) > 0.0:
        raise ValueError("--transducer-weight %g with --mwer-weight %g is not supported: a training step is either the MWER step or the "
                         "transducer step" % (r, args.mwer_weight))
    if getattr(args, "distill_from", None) or float(getattr(args, "distill_weight", 0.0) or 0.0) > 0.0 \
            or float(getattr(args, "distill_ctc_weight", 0.0) or 0.0) > 0.0:
        raise ValueError("--transducer-weight %g with --distill-from is not supported: a training step is either the distillation step "
                         "or the transducer step" % r)
    if int(getattr(args, "rank", 0) or 0) > 0:
        raise ValueError("--transducer-weight %g with --rank %d is not supported: the transducer head is not factorised" % (r, args.rank))
    return r


def check_prune_range(S):
    """--transducer-prune-range S -> S: 0 (off, the full lattice) or 2..64 label positions per frame (1 would be a band without a label
    arc; the band's upper end keeps the banded logits small, which is its point)."""
    S = int(S or 0)
    if S != 0 and not 2 <= S <= 64:
        raise ValueError("--transducer-prune-range must be 0 (off) or lie in 2..64, got %d" % S)
    return S


def check_simple_scale(c):
    """--transducer-simple-scale c -> c >= 0: the weight of the simple joiner's loss in L_rnnt = L_pruned + c L_simple."""
    c = float(c)
    if not c >= 0.0 or c == float("inf"):
        raise ValueError("--transducer-simple-scale must be a finite number >= 0, got %g" % c)
    return c


def check_mwer(args, label2id=None):
    """--mwer-weight m (minimum word error rate training over the CTC n-best) -> m.  m must lie in [0, 1]; m > 0
    needs --ctc-weight > 0 (the n-best comes from the encoder CTC head's prefix beam search), --loss ce, no --parallel, --mwer-nbest in
    2..16 and, with --mwer-unit word, a space among the labels (label2id, when given).  m = 0: nothing is checked beyond the range."""
    m = float(getattr(args, "mwer_weight", 0.0) or 0.0)
    if not 0.0 <= m <= 1.0:
        raise ValueError("--mwer-weight must lie in [0, 1], got %g" % m)
    if m == 0.0:
        return m
    if not float(getattr(args, "ctc_weight", 0.0) or 0.0) > 0.0:
        raise ValueError("--mwer-weight %g needs --ctc-weight > 0: the n-best comes from the prefix beam search over the encoder CTC "
                         "head, and without the weight the model has no such head" % m)
    if getattr(args, "parallel", False):
        raise ValueError("--mwer-weight %g with --parallel is not supported: the MWER step runs on the single-process eager path" % m)
    if getattr(args, "loss", "ce") != "ce":
        raise ValueError("--mwer-weight %g with --loss %s is not supported: the risk is interpolated with the joint cross-entropy / CTC "
                         "loss (--loss ce)" % (m, args.loss))
    n = int(getattr(args, "mwer_nbest", 4))
    if not 2 <= n <= 16:
        raise ValueError("--mwer-nbest %d: the n-best holds 2..16 hypotheses (the CTC prefix beam search keeps at most 16 prefixes)" % n)
    unit = getattr(args, "mwer_unit", "label")
    if unit not in ("label", "word"):
        raise ValueError("--mwer-unit must be 'label' or 'word', got %r" % (unit,))
    if unit == "word" and label2id is not None and " " not in label2id:
        raise ValueError("--mwer-unit word needs a space label to split words at, and the label file has none (use --mwer-unit label)")
    return m


def check_distill(args):
    """--distill-from / --distill-weight a / --distill-ctc-weight c / --distill-temperature tau (knowledge distillation from a teacher
    checkpoint) -> (a, c).  a and c lie in [0, 1], tau in [0.5, 16]; a positive weight needs --distill-from and a
    path needs a positive weight; distillation excludes --parallel, --loss ctc and --mwer-weight > 0, and c > 0 needs --ctc-weight > 0
    (the student's CTC head).  Everything off: (0, 0), nothing else is checked."""
    a = float(getattr(args, "distill_weight", 0.0) or 0.0)
    c = float(getattr(args, "distill_ctc_weight", 0.0) or 0.0)
    path = getattr(args, "distill_from", None) or None
    if not 0.0 <= a <= 1.0:
        raise ValueError("--distill-weight must lie in [0, 1], got %g" % a)
    if not 0.0 <= c <= 1.0:
        raise ValueError("--distill-ctc-weight must lie in [0, 1], got %g" % c)
    if a == 0.0 and c == 0.0:
        if path is not None:
            raise ValueError("--distill-from %s with --distill-weight 0 and --distill-ctc-weight 0: the teacher would be loaded and never "
                             "used; give one of the weights" % path)
        return a, c
    if path is None:
        raise ValueError("--distill-weight %g / --distill-ctc-weight %g need --distill-from PATH: the teacher checkpoint" % (a, c))
    tau = float(getattr(args, "distill_temperature", 2.0))
    if not 0.5 <= tau <= 16.0:
        raise ValueError("--distill-temperature must lie in [0.5, 16], got %g" % tau)
    if getattr(args, "parallel", False):
        raise ValueError("--distill-from with --parallel is not supported: the distillation step runs on the single-process eager path")
    if getattr(args, "loss", "ce") != "ce":
        raise ValueError("--distill-from with --loss %s is not supported: the distillation term is interpolated with the cross-entropy "
                         "loss (--loss ce)" % args.loss)
    if float(getattr(args, "mwer_weight", 0.0) or 0.0) > 0.0:
        raise ValueError("--distill-from with --mwer-weight %g is not supported: a training step is either the MWER step or the "
                         "distillation step" % args.mwer_weight)
    if c > 0.0 and not float(getattr(args, "ctc_weight", 0.0) or 0.0) > 0.0:
        raise ValueError("--distill-ctc-weight %g needs --ctc-weight > 0: the frame-level term is taken on the student's encoder CTC "
                         "head, and without the weight the model has no such head" % c)
    return a, c


_TEACHER_FRONT_END = ("sample_rate", "window_size", "window_stride", "window")


def load_teacher(path, args, label2id):
    """The frozen teacher of a distillation run (train.py --distill-from): built from the checkpoint's OWN
    Namespace, on a copy, with parallel=False and the student's --precision (ops.set_compute_dtype is process-wide); constant.args and
    constant.explicit are not touched.  -> the model in eval mode, no parameter requiring grad, on the GPU with --cuda.  It is never
    handed to init_optimizer.  ValueError for a missing file, for labels or feature settings that differ from the student's (args,
    label2id), and -- with --distill-ctc-weight > 0 -- for a teacher without a CTC head or with another feat_extractor."""
    import copy
    if not os.path.isfile(path):
        raise ValueError("--distill-from %s: no such teacher checkpoint (the student is %s)" % (path, getattr(args, "name", "this run")))
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if "args" not in ckpt:
        raise ValueError("--distill-from %s: the checkpoint carries no args to rebuild the teacher from" % path)
    t_l2i = ckpt["label2id"]
    if dict(t_l2i) != dict(label2id):
        raise ValueError("--distill-from %s: the teacher's labels (%d) differ from the student's (%d): distillation compares the two "
                         "models' distributions label by label" % (path, len(t_l2i), len(label2id)))
    t_args = copy.deepcopy(ckpt["args"])
    names = ("features", "num_mel_bins", "mel_fmin")
    for k, tv, sv in zip(names, feature_settings(t_args), feature_settings(args)):
        if tv != sv:
            raise ValueError("--distill-from %s: the teacher was trained with --%s %s, the student runs with --%s %s: both models read "
                             "the same batch" % (path, k.replace("_", "-"), tv, k.replace("_", "-"), sv))
    for k in _TEACHER_FRONT_END:
        tv, sv = getattr(t_args, k, None), getattr(args, k, None)
        if tv != sv:
            raise ValueError("--distill-from %s: the teacher was trained with --%s %s, the student runs with --%s %s: both models read "
                             "the same batch" % (path, k.replace("_", "-"), tv, k.replace("_", "-"), sv))
    t_args.parallel = False
    t_args.precision = getattr(args, "precision", "bf16")
    for k, v in zip(names, feature_settings(t_args)):
        setattr(t_args, k, v)
    teacher = init_transformer_model(t_args, t_l2i, ckpt["id2label"])
    sd = ckpt["model_state_dict"]
    if any(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    teacher.load_state_dict(sd)
    if float(getattr(args, "distill_ctc_weight", 0.0) or 0.0) > 0.0:
        if not hasattr(teacher, "ctc_linear"):
            raise ValueError("--distill-ctc-weight %g: the teacher %s has no encoder CTC head (it was trained with --ctc-weight 0), the "
                             "student has one" % (args.distill_ctc_weight, path))
        if teacher.feat_extractor != getattr(args, "feat_extractor", None):
            raise ValueError("--distill-ctc-weight %g: the teacher %s has --feat_extractor %s, the student %s: their CTC heads see "
                             "different frame counts" % (args.distill_ctc_weight, path, teacher.feat_extractor, args.feat_extractor))
    teacher.eval()
    teacher.requires_grad_(False)
    if getattr(args, "cuda", False):
        teacher = teacher.cuda()
    return teacher


def init_transformer_model(args, label2id, id2label):
    """Builds Encoder / Decoder / Transformer from the flags; mutates args.dim_input exactly like the reference
    (functions.py:116-162): 5120 for vgg_cnn, 672 for emb_cnn, unchanged (161) without a CNN.  With --features fbank the bins are
    --num-mel-bins instead of 161: 2560 for vgg_cnn at 80; emb_cnn needs 81 rows; without a CNN dim_input is the bin count."""
    n_fft_bins = feature_bins(args)                                                   # 161, or --num-mel-bins with --features fbank
    if args.feat_extractor == 'emb_cnn' and n_fft_bins < 81:
        raise ValueError("--feat_extractor emb_cnn needs at least 81 feature rows (its 41- and 21-row strided kernels leave none of "
                         "%d): use vgg_cnn with --features fbank --num-mel-bins %d" % (n_fft_bins, n_fft_bins))
    if args.feat_extractor == 'emb_cnn':
        h = int(math.floor(n_fft_bins - 41) / 2 + 1)
        h = int(math.floor(h - 21) / 2 + 1)
        args.dim_input = h * 32
    elif args.feat_extractor == 'vgg_cnn':
        args.dim_input = int(math.floor(int(math.floor(n_fft_bins) / 2) / 2)) * 128
    else:
        print("the model is initialized without feature extractor")
        if feature_settings(args)[0] == "fbank":
            if "dim_input" in getattr(constant, "explicit", ()) and args is constant.args and args.dim_input != n_fft_bins:
                raise ValueError("--dim-input %d, but --features fbank --num-mel-bins %d gives the model %d rows"
                                 % (args.dim_input, n_fft_bins, n_fft_bins))
            args.dim_input = n_fft_bins
    conv_k = check_conv_module_kernel(getattr(args, "conv_module_kernel", 0), args.dim_model, getattr(args, "rank", 0))
    pos_enc = check_pos_encoding(getattr(args, "pos_encoding", "abs"), args.dim_key, args.dim_value, getattr(args, "rank", 0))
    ops.set_compute_dtype(torch.float32 if getattr(args, "precision", "bf16") == "fp32" else torch.bfloat16)
    ops.set_fp8(getattr(args, "precision", "bf16") == "fp8")
    encoder = Encoder(args.num_layers, num_heads=args.num_heads, dim_model=args.dim_model, dim_key=args.dim_key,
                      dim_value=args.dim_value, dim_input=args.dim_input, dim_inner=args.dim_inner,
                      src_max_length=args.src_max_len, dropout=args.dropout, rank=getattr(args, "rank", 0),
                      conv_module_kernel=conv_k, pos_encoding=pos_enc)
    decoder = Decoder(id2label, num_src_vocab=len(label2id), num_trg_vocab=len(label2id), num_layers=args.num_layers,
                      num_heads=args.num_heads, dim_emb=args.dim_emb, dim_model=args.dim_model, dim_inner=args.dim_inner,
                      dim_key=args.dim_key, dim_value=args.dim_value, trg_max_length=args.tgt_max_len, dropout=args.dropout,
                      emb_trg_sharing=args.emb_trg_sharing, rank=getattr(args, "rank", 0))
    ctc_weight = check_ctc_weight(getattr(args, "ctc_weight", 0.0), args)
    transducer = None
    if check_transducer_weight(args) > 0:
        transducer = dict(dim_joint=int(getattr(args, "transducer_dim_joint", 256)), context=int(getattr(args, "transducer_context", 2)),
                          prune_range=int(getattr(args, "transducer_prune_range", 0) or 0))
    model = Transformer(encoder, decoder, feat_extractor=args.feat_extractor, ctc_head=ctc_weight > 0, transducer=transducer)
    if args.parallel:
        model = HipDataParallel(model, device_ids=args.device_ids)
    return model
