"""Joint CTC / attention training and decoding on the GPU: the encoder CTC head against torch in float64, the
hybrid loss and its gradients as the weighted sum of their parts, the frame-length rule, one train.py-level step, and the joint beam
search against rigged CTC posteriors, against the same search on the float64 host scorer, and under LM rescoring.  Tiny models."""
import json
import math
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_prefix_reference as R

pytestmark = pytest.mark.gpu

CHARS = "abcdefgh "                      # + PAD, SOS, EOS: V = 12
TINY = ("--num-layers 2 --num-heads 2 --dim-model 64 --dim-key 32 --dim-value 32 --dim-inner 128 --dim-emb 64 --tgt-max-len 32 "
        "--src-max-len 400 --dropout 0 --label-smoothing 0.1 --cuda").split()


@pytest.fixture
def cli():
    from utils import constant
    old_args, old_explicit = constant.args, constant.explicit
    yield constant.parse
    constant.set_args(old_args)
    constant.explicit = old_explicit


def _labels():
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(CHARS)
    l2i = {c: i for i, c in enumerate(chars)}
    return l2i, {i: c for c, i in l2i.items()}


def _model(cli, extra=(), seed=0):
    from utils.functions import init_transformer_model
    torch.manual_seed(seed)
    l2i, i2l = _labels()
    return init_transformer_model(cli(TINY + list(extra)), l2i, i2l).cuda()


def _batch(seed=1, T=160, lengths=(160, 120, 90), tg_len=(9, 6, 4), L=9):
    g = torch.Generator().manual_seed(seed)
    B = len(lengths)
    src = torch.randn(B, 1, 161, T, generator=g)
    tgt = torch.zeros(B, L, dtype=torch.int64)
    for b, n in enumerate(tg_len):
        tgt[b, :n] = torch.randint(3, 12, (n,), generator=g)
    return src.cuda(), torch.tensor(lengths), tgt.cuda(), torch.tensor(tg_len, dtype=torch.int32)


def _clear_grads(model):
    for p in model.parameters():
        p.grad = None


def _rel(a, b):
    return float((a - b).norm()) / (float(b.norm()) + 1e-30)


# ------------------------------------------------------------------------------------------------ training
def test_head_and_ctc_match_torch_float64(cli):
    """enc_out as a leaf -> ctc_linear -> CTC with the frame-length rule, against F.linear + F.log_softmax + F.ctc_loss(mean) in float64:
    the loss and the gradients of enc_out, W and b.  Bounds as in tests/test_gpu_ctc.py: small absolute + relative, or 4x what torch's
    own fp32 evaluation loses against float64."""
    from asr_hip import functions as F_
    from utils import constant
    model = _model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).train()
    _, lengths, tgt, tl = _batch()
    g = torch.Generator().manual_seed(5)
    enc0 = torch.randn(3, 40, 64, generator=g)
    frames = model.ctc_frame_lengths(lengths, 40)
    assert frames == [40, 30, 22]
    W0, b0 = model.ctc_linear.weight.detach().cpu(), (torch.randn(12, generator=g) * 0.1)
    model.ctc_linear.bias.data.copy_(b0)

    def truth(dtype):
        e, W, b = (x.to(dtype).clone().requires_grad_() for x in (enc0, W0, b0))
        lp = F.log_softmax(F.linear(e, W, b), dim=2).transpose(0, 1)
        loss = F.ctc_loss(lp, tgt.cpu(), torch.tensor(frames), tl.long(), reduction="mean")
        loss.backward()
        return loss.detach().double(), e.grad.double(), W.grad.double(), b.grad.double()

    ref, ref32 = truth(torch.float64), truth(torch.float32)
    _clear_grads(model)
    enc = enc0.cuda().requires_grad_()
    logits = model.ctc_logits(enc)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (3, 40, 12)
    loss = F_.CTCFn.apply(logits, tgt, torch.tensor(frames, dtype=torch.int32), tl, constant.PAD_TOKEN)
    loss.backward()
    assert abs(loss.item() - ref[0].item()) <= 2e-5 * max(1.0, abs(ref[0].item())), (loss.item(), ref[0].item())
    for name, got, r, r32 in (("d enc_out", enc.grad, ref[1], ref32[1]), ("dW", model.ctc_linear.weight.grad, ref[2], ref32[2]),
                              ("db", model.ctc_linear.bias.grad, ref[3], ref32[3])):
        err = (got.double().cpu() - r).abs().max().item()
        err32 = (r32 - r).abs().max().item()
        print("%s: max error %.3e (torch fp32: %.3e, largest entry %.3e)" % (name, err, err32, r.abs().max().item()))
        assert err <= max(2e-6 + 2e-5 * r.abs().max().item(), 4 * err32), (name, err, err32)
    assert float(enc.grad[1, 30:].abs().max()) == 0.0 and float(enc.grad[2, 22:].abs().max()) == 0.0      # frames >= T_b get no gradient


def test_head_gradients_in_bf16_through_the_flat_buffers(cli):
    """The same head in bf16 with the optimiser built: ctc_linear's parameters live in the flat buffer, the forward reads the flat bf16
    weight shadow and the backward goes through the deferred weight-gradient queue -- no special case for the new layer.  Against
    float64 within 3e-2 of each gradient's norm, the project's bound for bf16 gradients (tests/test_gpu_model.py)."""
    from asr_hip import functions as F_
    from asr_hip import ops
    from utils import constant
    from utils.functions import init_optimizer
    model = _model(cli, ["--precision", "bf16", "--ctc-weight", "0.3"]).train()
    opt = init_optimizer(constant.args, model, "noam")
    flat = opt.optimizer.flat
    assert flat is not None and model.ctc_linear.weight.__dict__["_asr_flat"][0] is flat and model.ctc_linear.bias.__dict__["_asr_flat"][0] is flat
    _, lengths, tgt, tl = _batch()
    enc0 = torch.randn(3, 40, 64, generator=torch.Generator().manual_seed(5))
    frames = model.ctc_frame_lengths(lengths, 40)
    e, W, b = (x.detach().double().cpu().clone().requires_grad_() for x in (enc0, model.ctc_linear.weight, model.ctc_linear.bias))
    ref = F.ctc_loss(F.log_softmax(F.linear(e, W, b), dim=2).transpose(0, 1), tgt.cpu(), torch.tensor(frames), tl.long(), reduction="mean")
    ref.backward()
    opt.zero_grad()
    enc = enc0.cuda().requires_grad_()
    loss = F_.CTCFn.apply(model.ctc_logits(enc), tgt, torch.tensor(frames, dtype=torch.int32), tl, constant.PAD_TOKEN)
    ops.backward_from(loss)
    torch.cuda.synchronize()
    assert abs(loss.item() - ref.item()) <= 3e-2 * abs(ref.item()), (loss.item(), ref.item())
    for name, got, r in (("d enc_out", enc.grad, e.grad), ("dW", model.ctc_linear.weight.grad, W.grad), ("db", model.ctc_linear.bias.grad, b.grad)):
        dev = _rel(got.double().cpu(), r)
        print("bf16 %s: relative deviation %.3e" % (name, dev))
        assert dev <= 3e-2, (name, dev)
    w_before = model.ctc_linear.weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(model.ctc_linear.weight.detach(), w_before)


def test_hybrid_loss_and_gradients_are_the_weighted_sum_of_their_parts(cli):
    """L(0.3) = 0.7 CE + 0.3 CTC of the separately computed pieces, and so are the gradients of conv.0.weight and of an encoder FFN
    weight: g(0.3) = 0.7 g(CE only, today's path) + 0.3 g(CTC only).  Linearity through the shared encoder: a dropped or double-counted
    accumulation of the encoder output's two gradients shows here.  fp32, dropout 0: the three backward passes differ by the order of
    fp32 additions only, 1e-5 of a gradient's norm covers sums of a few thousand terms at 6e-8 each."""
    from utils.metrics import calculate_joint_loss, calculate_metrics
    model = _model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).train()
    src, lengths, tgt, tl = _batch()
    names = ("conv.0.weight", "encoder.layers.1.pos_ffn.conv_1.weight", "encoder.layers.0.self_attn.query_linear.weight")
    params = dict(model.named_parameters())

    def grads():
        torch.cuda.synchronize()
        return {k: params[k].grad.detach().clone() for k in names}

    _clear_grads(model)
    pred, gold, _, _ = model(src, lengths, tgt)                          # today's CE-only path
    ce0, _ = calculate_metrics(pred, gold, smoothing=0.1, loss_type="ce", sync=False)
    ce0.backward()
    g_ce = grads()
    assert model.ctc_linear.weight.grad is None
    _clear_grads(model)
    pred, gold, _, _, ctc_logits = model(src, lengths, tgt, return_ctc=True)
    _, _, ctc1 = calculate_joint_loss(model, pred, gold, ctc_logits, tgt, lengths, tl, 0.1, 1.0)
    ctc1.backward()                                                       # the CTC-only loss through the new branch
    g_ctc = grads()
    assert params["decoder.output_linear.weight"].grad is None or float(params["decoder.output_linear.weight"].grad.abs().max()) == 0.0
    _clear_grads(model)
    pred, gold, _, _, ctc_logits = model(src, lengths, tgt, return_ctc=True)
    loss, ce, ctc = calculate_joint_loss(model, pred, gold, ctc_logits, tgt, lengths, tl, 0.1, 0.3)
    loss.backward()
    g_mix = grads()
    assert math.isfinite(loss.item()) and ctc1.item() > 0
    assert abs(ce.item() - ce0.item()) <= 1e-6 * abs(ce0.item()) and abs(ctc.item() - ctc1.item()) <= 1e-6 * abs(ctc1.item())
    want = 0.7 * ce0.item() + 0.3 * ctc1.item()
    assert abs(loss.item() - want) <= 2e-6 * abs(want), (loss.item(), want)
    for k in names:
        mix = 0.7 * g_ce[k] + 0.3 * g_ctc[k]
        print("%s: |g_ce| %.3e |g_ctc| %.3e rel. deviation %.3e" % (k, float(g_ce[k].norm()), float(g_ctc[k].norm()), _rel(g_mix[k], mix)))
        assert float(g_ctc[k].norm()) > 0 and _rel(g_mix[k], mix) <= 1e-5, (k, _rel(g_mix[k], mix))


def test_frame_length_rule_is_post_cnn_and_an_unreachable_batch_is_skipped(cli):
    """80 padded input frames = 20 encoder frames; utterance 1 has 40 input frames = 10 encoder frames and 15 distinct labels.  Under
    the pre-CNN lengths the encoder masks with (min(20, 40) = 20 frames) the target would be reachable; under the true frame count it
    is not: the loss is +inf, and the trainer skips the batch without touching a weight."""
    from trainer.asr.trainer import Trainer
    from utils import constant
    from utils.functions import init_optimizer
    from utils.metrics import calculate_joint_loss
    model = _model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).train()
    l2i, i2l = _labels()
    src = torch.randn(2, 1, 161, 80, generator=torch.Generator().manual_seed(2)).cuda()
    lengths = torch.tensor([80, 40])
    assert model.ctc_frame_lengths(lengths, 20) == [20, 10]
    tgt = torch.zeros(2, 15, dtype=torch.int64)
    tgt[0, :5] = torch.tensor([3, 4, 5, 6, 7])
    tgt[1] = torch.tensor([3 + i % 9 for i in range(15)])
    tgt = tgt.cuda()
    with torch.no_grad():
        pred, gold, _, _, ctc_logits = model(src, lengths, tgt, return_ctc=True)
        for tl, finite in (([5, 15], False), ([5, 10], True)):
            loss, ce, ctc = calculate_joint_loss(model, pred, gold, ctc_logits, tgt, lengths, torch.tensor(tl, dtype=torch.int32), 0.1, 0.3)
            assert math.isfinite(ce.item())
            assert math.isfinite(loss.item()) == finite and (finite or (loss.item() > 0 and math.isinf(ctc.item()))), (tl, loss.item())
    opt = init_optimizer(constant.args, model, "noam")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    data = (src, tgt, torch.tensor([1.0, 0.5]), lengths, torch.tensor([5, 15], dtype=torch.int32))
    assert Trainer()._run_batch(model, data, 0.1, "ce", i2l, opt) is None
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()) and opt._step == 0
    data = (src, tgt, torch.tensor([1.0, 0.5]), lengths, torch.tensor([5, 10], dtype=torch.int32))
    r = Trainer()._run_batch(model, data, 0.1, "ce", i2l, opt)
    r = r.result() if hasattr(r, "result") else r
    assert r is not None and math.isfinite(r[0]) and opt._step == 1
    assert not torch.equal(model.state_dict()["ctc_linear.weight"], before["ctc_linear.weight"])


def _corpus(tmp_path, n=6):
    rng = np.random.RandomState(0)
    words = ["ab", "ba", "abba", "bab", "aab", "bba"]
    lines = []
    for i in range(n):
        w = tmp_path / ("u%d.wav" % i)
        with wave.open(str(w), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((rng.randn(4000 + 800 * i) * 2000).astype("<i2").tobytes())
        t = tmp_path / ("u%d.txt" % i)
        t.write_text(words[i % len(words)] + "\n")
        lines.append("%s,%s" % (w, t))
    man = tmp_path / "train.csv"
    man.write_text("\n".join(lines))
    lab = tmp_path / "labels.json"
    lab.write_text(json.dumps([" ", "a", "b"]))
    return str(man), str(lab)


def test_train_py_step_with_ctc_weight_and_decoding_from_the_checkpoint(cli, tmp_path, monkeypatch):
    """train.py's main() with --ctc-weight 0.3 in bf16: the steps run eagerly (no captured step is built), the loss is finite, the head
    moves, and the checkpoint comes back with the head; test.py's evaluate() then decodes from it with joint scoring and --ctc-greedy."""
    import train as train_mod
    import test as test_mod
    import utils.functions as UF
    from trainer.asr.trainer import Trainer
    from utils import constant
    man, lab = _corpus(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--train-manifest-list", man, "--valid-manifest-list", man, "--test-manifest-list", man, "--labels-path", lab,
            "--cuda", "--batch-size", "3", "--num-workers", "0", "--epochs", "1", "--save-every", "1", "--name", "tinyctc",
            "--save-folder", str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key",
            "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64",
            "--label-smoothing", "0.1", "--dropout", "0.1", "--k-lr", "20", "--warmup", "5", "--ctc-weight", "0.3"]
    first = {}
    init = UF.init_transformer_model

    def recording_init(*a, **k):
        m = init(*a, **k)
        first["w"] = m.ctc_linear.weight.detach().cpu().clone()
        return m

    def no_graph(*a, **k):
        raise AssertionError("the hybrid step must run eagerly")
    monkeypatch.setattr(UF, "init_transformer_model", recording_init)
    monkeypatch.setattr(Trainer, "_graph_step", no_graph)
    cli(argv)
    train_mod.main()
    assert constant.args.graph_buckets == 0 and constant.args.precision == "bf16"
    monkeypatch.setattr(UF, "init_transformer_model", init)
    path = str(tmp_path / "save" / "tinyctc" / "best_model.th")
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert np.isfinite(state["metrics"]["train_loss"]) and np.isfinite(state["metrics"]["valid_loss"])
    assert state["optimizer_params"]["_step"] == 2 and state["args"].ctc_weight == 0.3
    assert not torch.equal(state["model_state_dict"]["ctc_linear.weight"], first["w"])
    cli(["--cuda", "--continue-from", path, "--tgt-max-len", "301", "--batch-size", "3", "--num-workers", "0", "--beam-search",
         "--beam-width", "2", "--ctc-decode-weight", "0.3"])
    model, _, _, _, largs, l2i, _ = UF.load_model(path)
    assert torch.equal(model.ctc_linear.weight.detach().cpu(), state["model_state_dict"]["ctc_linear.weight"])
    test_mod.check_ctc_decoding(constant.args, model)
    from models.common_layers import PositionalEncoding
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    model.decoder.positional_encoding = PositionalEncoding(model.decoder.dim_model, 301).cuda()
    ds = SpectrogramDataset(test_mod.feature_conf(largs), [man], l2i, normalize=True)
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    cer, wer = test_mod.evaluate(model, loader)
    assert np.isfinite(cer) and cer >= 0
    constant.args.beam_search, constant.args.ctc_decode_weight, constant.args.ctc_greedy = False, 0.0, True
    cer, wer = test_mod.evaluate(model, loader)
    assert np.isfinite(cer) and cer >= 0


# ------------------------------------------------------------------------------------------------ decoding
def _rigged(strings, frames, T, V=12, noise_label=11):
    """A peaky alignment per utterance: label, blank, label, blank ... (+20 on the aligned symbol, 0 elsewhere), blanks up to T_b;
    the frames >= T_b shout another label, which a scorer that respects T_b never hears."""
    lg = torch.zeros(len(strings), T, V)
    for b, (s, Tb) in enumerate(zip(strings, frames)):
        assert 2 * len(s) - 1 <= Tb <= T
        path = [0] * T
        for i, c in enumerate(s):
            path[2 * i] = c
        for t in range(T):
            lg[b, t, path[t] if t < Tb else noise_label] = 20.0
    return lg


STRINGS = [[3, 4, 4, 5, 6, 7], [8, 8, 3, 9, 10, 4], [5, 6, 7, 7, 8, 9]]       # each with a doubled letter


@pytest.mark.parametrize("B", [1, 3])
def test_rigged_ctc_posteriors_decide_the_search(cli, B):
    """mu = 1, a randomly initialised decoder, W 3, K = V = 12: the best hypothesis is exactly the string the CTC posteriors spell, doubled
    letter included, for one utterance and for three with different strings and T_b.  Without joint scoring the random decoder decides."""
    from utils import constant
    model = _model(cli, ["--precision", "fp32"]).eval()
    dec = model.decoder
    T, frames = 16, [16, 13, 12][:B]
    enc = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(3)).cuda()
    lg = _rigged(STRINGS[:B], frames, T).cuda()
    ids, strs = dec.beam_search(enc, beam_width=3, nbest=1, ctc_logits=lg, ctc_lengths=frames, ctc_weight=1.0, ctc_candidates=12)
    want = [[constant.SOS_TOKEN] + s + [constant.EOS_TOKEN] for s in STRINGS[:B]]
    assert ids == want, (ids, want)
    assert strs == ["".join(dec.id2label[c] for c in s + [constant.EOS_TOKEN]) for s in STRINGS[:B]]
    ids0, _ = dec.beam_search(enc, beam_width=3, nbest=1)
    assert ids0 != want


def test_zero_weight_leaves_the_search_unchanged(cli):
    model = _model(cli, ["--precision", "fp32"]).eval()
    dec = model.decoder
    enc = torch.randn(3, 16, 64, generator=torch.Generator().manual_seed(4)).cuda()
    lg = _rigged(STRINGS, [16, 13, 12], 16).cuda()
    for e in (enc, enc[:1]):
        plain = dec.beam_search(e, beam_width=3, nbest=2)
        same = dec.beam_search(e, beam_width=3, nbest=2, ctc_logits=lg[:e.shape[0]], ctc_lengths=[16, 13, 12][:e.shape[0]], ctc_weight=0.0,
                               ctc_candidates=6)
        assert plain == same and len(plain[0]) == 2 * e.shape[0]


def _psi64(lp_u, Tb, tokens):
    labels = [t for t in tokens if t != R.EOS]
    pre, fin = R.score_sequence(lp_u, Tb, labels)
    if tokens and tokens[-1] == R.EOS:
        return fin
    return pre[-1] if pre else 0.0


def test_search_on_the_gpu_scorer_against_the_float64_host_scorer(cli):
    """The same search (same model, mu = 0.3, W 3, K 6) with the float64 host scorer substituted for the kernel.  The GPU search's best
    hypothesis, re-scored with its recorded attention terms and float64 CTC terms, lies within 2 * 2e-5 * max(1, |psi|) * steps of the
    host-scorer search's best score (the kernel's bound per step, both signs); equal strings are accepted outright.  Scores, not
    strings: a near-tie may flip."""
    from asr_hip.decode import CTCPrefixScorer
    model = _model(cli, ["--precision", "fp32"]).eval()
    dec = model.decoder
    B, T, W, K, mu = 2, 14, 3, 6, 0.3
    frames = [14, 9]
    g = torch.Generator().manual_seed(6)
    enc = torch.randn(B, T, 64, generator=g).cuda()
    lg = (torch.randn(B, T, 12, generator=g) * 2.0)
    row_utt = [b for b in range(B) for _ in range(W)]
    with torch.no_grad():
        gpu = dec._beam_search_hyps(enc, W, ctc=(CTCPrefixScorer(lg.cuda(), frames, row_utt), mu, K))
        host = dec._beam_search_hyps(enc, W, ctc=(R.HostPrefixScorer(lg, frames, row_utt), mu, K))
    lp = R.log_softmax(lg.double().numpy())
    for b in range(B):
        assert gpu[b] and host[b]
        for h in gpu[b]:                                  # the accumulated score IS the sum of the joint increments
            assert abs(h["score"] - ((1 - mu) * h["att"] + mu * h["psi"])) <= 1e-4 * max(1.0, abs(h["score"])) or h["psi"] == -math.inf
        best_g = max(gpu[b], key=lambda h: h["score"])
        best_h = max(host[b], key=lambda h: h["score"])
        if best_g["yseq"] == best_h["yseq"]:
            continue
        tokens = best_g["yseq"][1:]
        if len(tokens) == T + 1:                          # the EOS forced at the last encoder frame carries no score
            tokens = tokens[:-1]
        psi = _psi64(lp[b], frames[b], tokens)
        rescored = (1 - mu) * best_g["att"] + mu * psi
        bound = 2 * 2e-5 * max(1.0, abs(psi)) * len(tokens)
        print("utterance %d: GPU best %r re-scored %.6f, host best %r %.6f, bound %.2e" % (b, best_g["yseq"], rescored, best_h["yseq"],
                                                                                         best_h["score"], bound))
        assert abs(rescored - best_h["score"]) <= bound, (b, rescored, best_h["score"], bound)


def test_lm_rescoring_ranks_by_the_joint_score(cli, golden_dir):
    """With the fixture LM, final_score = joint score + lm_weight * LM score + sqrt(words) * c_weight: the joint `score`, not the
    attention score alone, enters the ranking, and the 1-best returned is the arg-max of final_score."""
    from utils import constant
    from utils.functions import init_transformer_model
    from utils.lstm_utils import LM
    z = np.load(os.path.join(golden_dir, "dec_tiny.npz"))
    chars = constant.PAD_CHAR + constant.SOS_CHAR + constant.EOS_CHAR + "_'abcdefghijklmnopqrstuvwxyz "
    l2i = {c: i for i, c in enumerate(chars)}
    args = cli(str(z["flags"]).split() + ["--precision", "fp32", "--cuda"])
    model = init_transformer_model(args, l2i, {i: c for c, i in l2i.items()})
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}, strict=True)
    model = model.cuda().eval()
    src, src_len = torch.from_numpy(z["src"]).cuda()[:2], torch.from_numpy(z["src_len"])[:2]
    with torch.no_grad():
        enc, _ = model.encoder(model._features(src), src_len)
    dec = model.decoder
    B, T, V = enc.shape[0], enc.shape[1], dec.num_trg_vocab
    lg = torch.randn(B, T, V, generator=torch.Generator().manual_seed(7)).cuda() * 2.0
    lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
    seen = []
    orig = dec._rank_ended

    def rec(ended, *a, **k):
        out = orig(ended, *a, **k)
        seen.append(ended)
        return out
    dec._rank_ended = rec
    try:
        ids, strs = dec.beam_search(enc, beam_width=3, nbest=1, lm_rescoring=True, lm=lm, lm_weight=0.2, c_weight=0.1, ctc_logits=lg,
                                    ctc_lengths=[T] * B, ctc_weight=0.3)
    finally:
        del dec._rank_ended
    ended = seen[0]
    assert len(ids) == B
    for b in range(B):
        for h in ended[b]:
            if h["psi"] == -math.inf:                   # a hypothesis CTC rules out (forced to end at the last frame): last in any ranking
                assert h["score"] == -math.inf and h["final_score"] == -math.inf
                continue
            joint = 0.7 * h["att"] + 0.3 * h["psi"]
            assert abs(h["score"] - joint) <= 1e-4 * max(1.0, abs(joint))
            want = h["score"] + 0.2 * h["lm_score"] + math.sqrt(h["num_words"]) * 0.1
            assert abs(h["final_score"] - want) <= 1e-9 * max(1.0, abs(want))
        assert ids[b] == max(ended[b], key=lambda h: h["final_score"])["yseq"]
        assert any(math.isfinite(h["score"]) and abs(h["score"] - h["att"]) > 1e-3 for h in ended[b])      # the CTC term is in the score that is ranked


def test_ctc_greedy_reads_the_rigged_string(cli):
    """Transformer.ctc_greedy: the head's frame-wise arg-max (asr_argmax_rows), repeats merged and blanks dropped inside T_b.  The head is
    set to read the first 12 encoder dimensions, which carry the rigged posteriors."""
    model = _model(cli, ["--precision", "fp32", "--ctc-weight", "0.3"]).eval()
    with torch.no_grad():
        model.ctc_linear.weight.zero_()
        model.ctc_linear.weight[:, :12] = torch.eye(12)
        model.ctc_linear.bias.zero_()
    frames = [16, 13, 12]
    enc = torch.zeros(3, 16, 64)
    enc[:, :, :12] = _rigged(STRINGS, frames, 16)
    got = model.ctc_greedy(enc.cuda(), frames)
    assert got == ["".join(model.id2label[c] for c in s) for s in STRINGS]
    assert model.ctc_greedy(enc.cuda(), [16, 16, 16])[1] != got[1]          # the frames beyond T_b do spell something else
