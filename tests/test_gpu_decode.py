"""KV-cached decoding (asr_hip/decode.py) against the reference-style full re-run of the decoder at every step
(models/asr/transformer.py:316-517): same kernels, same per-row arithmetic -> identical tokens / strings / scores."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 40


def _model(precision, layers=2):
    from utils import constant
    from utils.functions import init_transformer_model
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + [chr(0x61 + i) for i in range(V - 3)]
    l2i = {c: i for i, c in enumerate(chars)}
    i2l = {i: c for c, i in l2i.items()}
    args = constant.parse(["--num-layers", str(layers), "--num-heads", "8", "--dim-model", "512", "--dim-key", "64",
                           "--dim-value", "64", "--dim-inner", "256", "--dim-emb", "512", "--feat_extractor", "vgg_cnn",
                           "--tgt-max-len", "301", "--src-max-len", "64", "--dropout", "0.1", "--precision", precision,
                           "--cuda"])
    torch.manual_seed(7)
    model = init_transformer_model(args, l2i, i2l).cuda().eval()
    # make EOS reachable at different steps: bias the output layer a little towards EOS
    with torch.no_grad():
        model.decoder.output_linear.weight[2] += 0.02
    return model


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cached_step_equals_full_rerun_row(precision):
    """logits of position t from the cache == row t of the decoder run over the whole prefix (teacher forcing)."""
    model = _model(precision)
    dec = model.decoder
    g = torch.Generator().manual_seed(3)
    B, Te, T = 3, 37, 21
    enc = torch.randn(B, Te, 512, generator=g).cuda()
    ys = torch.randint(3, V, (B, T), generator=g).cuda()
    ys[:, 0] = 1
    from asr_hip.decode import DecoderKVCache
    full = dec._step_logits(ys, enc).float()
    cache = DecoderKVCache(dec, enc, max_len=T)
    tol = 2e-5 if precision == "fp32" else 2e-2
    for t in range(T):
        lg = cache.step(ys[:, t].contiguous())
        err = (lg - full[:, t]).abs().max().item()
        assert err <= tol * max(1.0, full[:, t].abs().max().item()), (t, err)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_greedy_and_beam_cached_match_uncached(precision):
    model = _model(precision, layers=1)
    dec = model.decoder
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 12, 512, generator=g).cuda()
    a = dec.greedy_search(enc, use_cache="graph")        # one hipGraph replay per token, kernel-per-op step
    b = dec.greedy_search(enc, use_cache=False)
    c = dec.greedy_search(enc, use_cache="eager")
    assert a == b == c and len(a) == 2
    ia, sa = dec.beam_search(enc, beam_width=3, nbest=2, use_cache=True)             # all utterances in one decoder batch
    ib, sb = dec.beam_search(enc, beam_width=3, nbest=2, use_cache=False)
    ic, sc = dec.beam_search(enc, beam_width=3, nbest=2, use_cache="per_utterance")
    assert sa == sb == sc and ia == ib == ic
    one = [dec.beam_search(enc[:1], beam_width=3, nbest=2, use_cache=mode) for mode in (True, False, "per_utterance")]
    assert one[0] == one[1] == one[2] and 1 <= len(one[0][1]) <= 2          # one utterance goes through the same batched loop


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batched_beam_search_equals_the_utterance_loop(precision):
    """Beam search over a batch of utterances as ONE KV-cached decoder batch (utterance b owns rows b * W ..) against the loop over
    utterances: the same token ids and strings, with utterances that finish at different steps and more utterances than beams."""
    model = _model(precision, layers=2)
    dec = model.decoder
    g = torch.Generator().manual_seed(11)
    enc = torch.randn(5, 9, 512, generator=g).cuda()
    for W, nbest in ((4, 3), (2, 1)):
        ia, sa = dec.beam_search(enc, beam_width=W, nbest=nbest, c_weight=0.1, use_cache=True)
        ib, sb = dec.beam_search(enc, beam_width=W, nbest=nbest, c_weight=0.1, use_cache="per_utterance")
        assert ia == ib and sa == sb and len(sa) >= 5


# ------------------------------------------------------------------------------------------------ vs the reference
def _reference_case(golden_dir, precision, name="dec_tiny"):
    import os
    from utils import constant
    from utils.functions import init_transformer_model
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    chars = constant.PAD_CHAR + constant.SOS_CHAR + constant.EOS_CHAR + "_'abcdefghijklmnopqrstuvwxyz "
    l2i = {c: i for i, c in enumerate(chars)}
    i2l = {i: c for c, i in l2i.items()}
    args = constant.parse(str(z["flags"]).split() + ["--precision", precision, "--cuda"])
    model = init_transformer_model(args, l2i, i2l)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}, strict=True)
    return z, model.cuda().eval()


def _error_counts(strs_hyps, strs_gold):
    """The accumulation of test.py:evaluate (reference test.py:42-58) with the product's metric functions."""
    from utils import constant
    from utils.metrics import calculate_cer, calculate_wer
    tc = tch = tw = twd = 0
    for h, g in zip(strs_hyps, strs_gold):
        for ch in (constant.EOS_CHAR, constant.SOS_CHAR, constant.PAD_CHAR):
            h, g = h.replace(ch, ""), g.replace(ch, "")
        tw += calculate_wer(h, g)
        tc += calculate_cer(h.strip(), g.strip())
        twd += len(g.split(" "))
        tch += len(g)
    return [tc, tch, tw, twd]


@pytest.mark.parametrize("use_cache", [True, "eager", False])
def test_decode_strings_and_cer_match_the_reference(golden_dir, use_cache):
    """fp32 mode: Transformer.evaluate() greedy and beam-4 produce the REFERENCE's strings (tests/golden/dec_tiny.npz: the
    reference's own evaluate() on a model the reference trained for 170 steps; greedy CER 17/34, beam CER 30/34) and
    therefore its CER / WER counts -- with the KV cache and with the reference-style full re-run."""
    z, model = _reference_case(golden_dir, "fp32")
    src, src_len, tgt = torch.from_numpy(z["src"]).cuda(), torch.from_numpy(z["src_len"]), torch.from_numpy(z["tgt"]).cuda()
    dec = model.decoder
    with torch.no_grad():
        feats = model._features(src)
        enc, _ = model.encoder(feats, src_len)
        assert (enc.float().cpu() - torch.from_numpy(z["enc_out"])).abs().max().item() < 5e-5
        _, gold, *_ = dec(tgt, enc, src_len)
    strs_gold = ["".join(model.id2label[int(x)] for x in row) for row in gold.cpu().tolist()]
    assert strs_gold == [str(s) for s in z["gold_strs"]]
    greedy = dec.greedy_search(enc, use_cache=use_cache)
    assert greedy == [str(s) for s in z["greedy"]]
    _, beam = dec.beam_search(enc, beam_width=int(z["beam_width"]), nbest=1, c_weight=0.1, use_cache=use_cache)
    assert beam == [str(s) for s in z["beam"]]
    assert _error_counts(greedy, strs_gold) == [int(v) for v in z["greedy_cer"]]
    assert _error_counts(beam, strs_gold) == [int(v) for v in z["beam_cer"]]
    if use_cache is True:       # the public entry point (reference transformer.py:87-124)
        _, hyps, golds = model.evaluate(src, src_len, tgt, beam_search=True, beam_width=int(z["beam_width"]), beam_nbest=1,
                                        c_weight=0.1)
        assert hyps == beam and golds == strs_gold


def test_decode_bf16_cer_close_to_reference(golden_dir):
    """bf16 mode decodes the same utterances; near-tied steps may flip, so the bound is on the error COUNTS:
    |CER chars - reference| <= 3 of 34 gold characters for greedy and for beam-4."""
    z, model = _reference_case(golden_dir, "bf16")
    src, src_len, tgt = torch.from_numpy(z["src"]).cuda(), torch.from_numpy(z["src_len"]), torch.from_numpy(z["tgt"]).cuda()
    _, greedy, golds = model.evaluate(src, src_len, tgt, beam_search=False)
    _, beam, _ = model.evaluate(src, src_len, tgt, beam_search=True, beam_width=int(z["beam_width"]), beam_nbest=1, c_weight=0.1)
    gc, bc = _error_counts(greedy, golds), _error_counts(beam, golds)
    assert gc[1] == int(z["greedy_cer"][1]) and abs(gc[0] - int(z["greedy_cer"][0])) <= 3, (gc, greedy)
    assert abs(bc[0] - int(z["beam_cer"][0])) <= 3, (bc, beam)


# ------------------------------------------------------------------------------------------------ dk = dv = 64: the shipped bf16 step
def _d128_encoder_output(z, model):
    src, src_len = torch.from_numpy(z["src"]).cuda(), torch.from_numpy(z["src_len"])
    with torch.no_grad():
        enc, _ = model.encoder(model._features(src), src_len)
    return enc


def test_d128_fp32_reproduces_the_reference_logits_and_strings(golden_dir):
    """tests/golden/dec_d128.npz: a 2-layer d_model 128 / 2 heads x 64 model the REFERENCE trained for 120 steps and decoded
    (oracle/gen_golden.py dec_d128; logits of all 300 greedy positions kept).  fp32: same strings, logits within 2e-4 of the range."""
    z, model = _reference_case(golden_dir, "fp32", "dec_d128")
    enc = _d128_encoder_output(z, model)
    assert (enc.float().cpu() - torch.from_numpy(z["enc_out"])).abs().max().item() < 1e-4
    dec = model.decoder
    assert dec.greedy_search(enc, use_cache=True) == [str(s) for s in z["greedy"]]
    _, beam = dec.beam_search(enc, beam_width=int(z["beam_width"]), nbest=1, c_weight=0.1, use_cache=True)
    assert beam == [str(s) for s in z["beam"]]
    ids = torch.from_numpy(z["greedy_ids"].astype(np.int64)).cuda()
    ys = torch.cat([torch.ones_like(ids[:, :1]), ids[:, :-1]], dim=1)
    ref = torch.from_numpy(z["greedy_logits"]).cuda()
    with torch.no_grad():
        got = dec._step_logits(ys, enc).float()
    assert (got - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()


def test_d128_bf16_fused_step_follows_the_reference_decode(golden_dir):
    """The SHIPPED bf16 greedy path -- csrc/decode.hip's 30-launch step, replayed from a hipGraph -- on the reference's own trained
    model.  (a) teacher-forced on the reference's 300 greedy tokens per utterance, the step's logits stay within 3e-2 of the
    reference's logit range at all 4 x 300 positions; (b) its arg max is the reference's token at every position whose reference
    margin (top1 - top2) exceeds twice the measured logit error there; (c) the free-running graph decode emits the reference's
    tokens up to each utterance's EOS, or leaves them first at a position whose margin is inside that error; (d) strings from the
    public entry point obey the same rule."""
    from asr_hip.decode import FusedGreedyDecoder, fused_decode_supported, greedy_search_graphed
    from utils import constant
    z, model = _reference_case(golden_dir, "bf16", "dec_d128")
    enc = _d128_encoder_output(z, model)
    dec = model.decoder
    steps = 300
    assert fused_decode_supported(dec, enc, steps)
    ids = torch.from_numpy(z["greedy_ids"].astype(np.int64)).cuda()          # (4, 300)
    ref = torch.from_numpy(z["greedy_logits"]).cuda()                         # (4, 300, V)
    margin = torch.from_numpy(z["greedy_margin"]).cuda()
    B = ids.shape[0]
    ys = torch.cat([torch.ones_like(ids[:, :1]), ids[:, :-1]], dim=1)
    step = FusedGreedyDecoder(dec, enc, max_len=steps)
    got = torch.stack([step.step_logits(ys[:, t].contiguous()).float().clone() for t in range(steps)], dim=1)   # (the step returns a view of its buffer)
    err = (got - ref).abs().amax(dim=2)                                       # (4, 300)
    assert err.max().item() <= 3e-2 * ref.abs().max().item(), err.max().item()
    flipped = got.argmax(2) != ids
    assert not (flipped & (margin > 2 * err)).any(), (int(flipped.sum()), (margin - 2 * err)[flipped].max().item())
    assert int(flipped.sum()) <= 0.02 * flipped.numel(), int(flipped.sum())
    # free running, through the graph
    toks = greedy_search_graphed(dec, enc, steps=steps)
    assert (B, enc.shape[1], steps, str(enc.device)) in dec._asr_fused_decoders          # the fused step is what ran
    worst = err.max().item()
    same_rows = 0
    for b in range(B):
        eos = (ids[b] == constant.EOS_TOKEN).nonzero()
        n = int(eos[0]) + 1 if len(eos) else steps
        n = min(n, toks.shape[1])
        diff = (toks[b, :n] != ids[b, :n]).nonzero()
        if len(diff) == 0:
            same_rows += 1
            continue
        t = int(diff[0])
        assert margin[b, t].item() <= 2 * worst, (b, t, margin[b, t].item(), worst)
    strs = dec.greedy_search(enc, use_cache=True)
    want = [str(s) for s in z["greedy"]]
    assert sum(a == w for a, w in zip(strs, want)) >= same_rows
    print("dec_d128 bf16: max logit error %.4f of range %.2f, %d / %d arg-max flips (teacher-forced), %d / %d utterances identical"
          % (worst, ref.abs().max().item(), int(flipped.sum()), flipped.numel(), same_rows, B))
    assert same_rows >= B - 1
