"""Transformer.transducer_beam_search, evaluate(transducer_beam=True) and test.py --transducer-beam-search on the
tiny model of tests/test_gpu_rnnt_model.py: D 32, V 11, a handful of encoder frames.  The kernel itself is pinned by
tests/test_gpu_rnnt_beam.py; here the model hands it the right tensors and ranks what comes back."""
import math
import os

import numpy as np
import pytest
import torch

import rnnt_beam_reference as R
import rnnt_reference as RL
from test_gpu_mwer_model import CHARS, GOLD, _batch, _corpus, cli, process_wide_random_state_is_left_as_found  # noqa: F401  (fixtures)
from test_gpu_rnnt_beam import gpu_rows
from test_gpu_rnnt_model import HEAD, _model

pytestmark = pytest.mark.gpu


def _head_tensors(model, enc):
    """What transducer_beam_search hands the kernel: e and the compute-dtype parameters the model's forward reads."""
    from asr_hip import functions as F_, params as P
    with torch.no_grad():
        e = F_.linear(enc, model.rnnt_enc.weight, model.rnnt_enc.bias, False, True)
    return dict(e=e.contiguous(), tables=[P.linear_weight(m.weight, e.dtype) for m in model.rnnt_embed],
                w_out=P.linear_weight(model.rnnt_out.weight, e.dtype), b_out=model.rnnt_out.bias.data)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_beam_width_1_follows_greedy_on_a_joint_table_set_by_hand(cli, precision):
    """The hand-set joint of the greedy test, made self-limiting and ten times sharper: dimension 0 carries a frame signal, 1 and 3
    whether the last label is 3 / 4, 2 whether label 4 stands two back, all saturated by the tanh; label 3 is emitted on frame signal +1
    and label 4 on -1 unless it was just emitted, label 5 when 4 stands two back; every arg-max leads by 10 logits, so the mass of a
    decision is within e^-10 of 1 and the best hypothesis of a W = 1 beam is greedy's.  (On the greedy test's own table label 4 is
    emitted whatever the history, every frame with signal -1 ends in the max_symbols cut, and there a beam legitimately differs: all
    its entries pay the same forced blank.  With max_symbols 2 this table meets the cut too; 1 and 4 do not.)  The restatement must
    agree with greedy first; then the kernel's ids are both's."""
    model = _model(cli, ["--transducer-weight", "0.4", "--transducer-dim-joint", "8", "--precision", precision]).eval()
    big = 20.0
    with torch.no_grad():
        for p in (model.rnnt_enc.weight, model.rnnt_enc.bias, model.rnnt_out.weight, model.rnnt_out.bias, model.rnnt_embed[0].weight,
                  model.rnnt_embed[1].weight):
            p.zero_()
        model.rnnt_enc.weight[0, 0] = 1.0
        model.rnnt_embed[0].weight[:, 1] = -big
        model.rnnt_embed[0].weight[3, 1] = big                  # one back is label 3
        model.rnnt_embed[0].weight[:, 3] = -big
        model.rnnt_embed[0].weight[4, 3] = big                  # one back is label 4
        model.rnnt_embed[1].weight[:, 2] = -big
        model.rnnt_embed[1].weight[4, 2] = big                  # two back is label 4
        model.rnnt_out.bias.copy_(10.0 * torch.tensor([1.0, -9, -9, -3, -4, -4, -9.5, -10, -10.5, -11, -11.5]))
        model.rnnt_out.weight[3, :3] = 10.0 * torch.tensor([3.0, -3.0, 0.0])
        model.rnnt_out.weight[4, :4] = 10.0 * torch.tensor([-4.0, 0.0, 0.0, -4.0])
        model.rnnt_out.weight[5, :3] = 10.0 * torch.tensor([0.0, 0.0, 6.0])
    enc = torch.zeros(3, 5, 32, device="cuda")
    enc[:, :, 0] = torch.tensor([big, -big, 0.0, big, -big])
    lengths = [5, 3, 0]
    e64 = enc.cpu().double() @ model.rnnt_enc.weight.detach().cpu().double().t() + model.rnnt_enc.bias.detach().cpu().double()
    tables = [m.weight.detach().cpu() for m in model.rnnt_embed]
    w_out, b_out = model.rnnt_out.weight.detach().cpu(), model.rnnt_out.bias.detach().cpu()
    for S in (1, 4):
        want, dec = RL.greedy(e64, tables, w_out, b_out, lengths, S)
        assert all(m >= 9.9 for d in dec for _, _, m in d) and want[0] and want[2] == []
        for b in range(3):
            res = R.search(R.table_row(e64[b].numpy(), [t.numpy() for t in tables], w_out.numpy(), b_out.numpy()), lengths[b], 11, W=1,
                           K=0, S=S, nbest=1, C=2)
            assert list(res["hyps"][0][0]) == want[b] and res["margins"]["beam"] >= 9.9, (S, b, res["hyps"], want[b], res["margins"])
        strs, ids = model.transducer_beam_search(enc, lengths, 1, nbest=1, max_symbols=S, return_ids=True)
        assert [rows[0] for rows in ids] == want, (S, ids, want)
        assert [rows[0] for rows in strs] == ["".join(model.id2label[x] for x in row) for row in want]
        assert model.transducer_greedy(enc, lengths, max_symbols=S, return_ids=True)[1] == want
    assert model.transducer_beam_search(enc, [0, 0, 0], 4, nbest=2) == [[""], [""], [""]]


@pytest.mark.parametrize("precision,seed", [("fp32", 1), ("bf16", 1)])
def test_a_small_random_model_against_the_restatement(cli, precision, seed):
    """W 4, K 3, S 2 on random weights (rnnt_out's eight times their initial size: a fresh head's rows are nearly uniform and no seed
    separates its decisions by 1e-3) and a random encoder output, T' 6 with lengths (6, 3, 0); c_weight 0, so the ranking is the
    kernel's own order: the whole 4-best of every utterance equals the restatement's on the project's own logits (every margin at least
    1e-3, asserted), the scores of the best within the rule of tests/test_gpu_rnnt_beam.py."""
    from asr_hip import ops
    model = _model(cli, HEAD + ["--precision", precision], seed=seed).eval()
    with torch.no_grad():
        model.rnnt_out.weight.mul_(8.0)
    g = torch.Generator().manual_seed(100 + seed)
    enc = torch.randn(3, 6, 32, generator=g).cuda()
    lengths = [6, 3, 0]
    Pg = _head_tensors(model, enc)
    assert Pg["e"].dtype == (torch.float32 if precision == "fp32" else torch.bfloat16) and all(t.dtype == Pg["e"].dtype for t in Pg["tables"])
    r64 = [R.search(gpu_rows(Pg, b), lengths[b], 11, 4, 3, 2, 4, 2) for b in range(3)]
    for b, res in enumerate(r64):
        assert R.min_margin(res) >= R.MARGIN, (b, res["margins"])
    strs, ids = model.transducer_beam_search(enc, lengths, 4, nbest=4, candidates=3, max_symbols=2, c_weight=0, return_ids=True)
    assert ids == [[list(y) for y, _ in res["hyps"]] for res in r64], (ids, [res["hyps"] for res in r64])
    assert strs == [["".join(model.id2label[x] for x in row) for row in rows] for rows in ids] and ids[2] == [[]]
    raw = ops.rnnt_beam_search(Pg["e"], Pg["tables"], Pg["w_out"], Pg["b_out"], torch.tensor(lengths, dtype=torch.int32, device="cuda"),
                               4, 3, 2, 4)
    r32 = [R.search(gpu_rows(Pg, b), lengths[b], 11, 4, 3, 2, 4, 2, dtype=np.float32) for b in range(3)]
    for b in range(3):
        s32 = {y: float(s) for y, s in r32[b]["hyps"]}
        bound = 4.0 * max(max(abs(s32[y] - float(s)) for y, s in r64[b]["hyps"] if y in s32), R.EPS32 * r64[b]["maxabs"])
        for n, (y, s) in enumerate(r64[b]["hyps"]):
            assert abs(float(raw["scores"][b, n]) - float(s)) <= bound, (b, n, float(raw["scores"][b, n]), float(s), bound)


def test_the_nbest_is_ranked_by_the_rank_ended_formula_with_and_without_the_lm(cli, golden_dir):
    """The kernel's W hypotheses as {'yseq', 'score', 'rnnt_score'}, ranked by asr_hip.search.rank_ended computed here in Python: the word
    bonus alone, and with the fixture LM score + lm_weight * (lm - 2 * oov) + sqrt(words) * c_weight."""
    from asr_hip import ops, search
    from utils.lstm_utils import LM
    model = _model(cli, HEAD + ["--precision", "fp32"], seed=1).eval()
    enc = torch.randn(3, 6, 32, generator=torch.Generator().manual_seed(7)).cuda()
    lengths = [6, 4, 2]
    lm = LM(os.path.join(golden_dir, "lm_tiny.pt"))
    Pg = _head_tensors(model, enc)
    W = 6
    raw = ops.rnnt_beam_search(Pg["e"], Pg["tables"], Pg["w_out"], Pg["b_out"], torch.tensor(lengths, dtype=torch.int32, device="cuda"),
                               W, 0, 2, W)
    raw = {k: v.cpu() for k, v in raw.items()}
    assert tuple(raw["ids"].shape) == (3, W, 12)

    def ended():
        return [[{'yseq': raw["ids"][b, n, :raw["lengths"][b, n]].tolist(), 'score': float(raw["scores"][b, n]),
                  'rnnt_score': float(raw["scores"][b, n])} for n in range(W) if raw["lengths"][b, n] >= 0] for b in range(3)]
    changed = 0
    for kw in (dict(c_weight=0.2), dict(c_weight=0.2, lm=lm, lm_weight=0.3)):
        want = [[h['yseq'] for h in hs]
                for hs in search.rank_ended(ended(), 3, kw["c_weight"], model.id2label, kw.get("lm"), kw.get("lm_weight", 0.1))]
        strs, ids = model.transducer_beam_search(enc, lengths, W, nbest=3, max_symbols=2, return_ids=True, **kw)
        assert ids == want and all(len(rows) == 3 for rows in ids), (ids, want)
        changed += sum(ids[b] != [h['yseq'] for h in ended()[b][:3]] for b in range(3))
    print("n-best lists the ranking changed against the kernel's own order: %d of 6" % changed)


def test_evaluate_routes_to_the_beam_search_and_leaves_the_other_modes_alone(cli, monkeypatch):
    from asr_hip import ops
    from models.asr.transformer import Transformer
    model = _model(cli, HEAD + ["--precision", "fp32"]).eval()
    src, lengths, tgt, _ = _batch()
    calls = []
    orig = ops.rnnt_beam_search

    def spy(*a, **k):
        calls.append(a[5:9])
        return orig(*a, **k)
    monkeypatch.setattr(ops, "rnnt_beam_search", spy)
    with torch.no_grad():
        enc = model.encoder(model._features(src), lengths)[0]
        frames = model.ctc_frame_lengths(lengths, enc.shape[1])
        best = model.transducer_beam_search(enc, frames, 4, nbest=1, candidates=3, max_symbols=2, c_weight=0.1)
        calls.clear()
        _, hyps, gold = model.evaluate(src, lengths, tgt, transducer_beam=True, beam_width=4, beam_nbest=3, c_weight=0.1,
                                       transducer_candidates=3, transducer_max_symbols=2)
    assert calls == [(4, 3, 2, 4)] and hyps == [rows[0] for rows in best] and len(gold) == 3
    # the flag off: no search launch, and greedy through evaluate() is greedy called directly
    calls.clear()
    seen = []
    greedy = Transformer.transducer_greedy

    def recording(self, *a, **k):
        seen.append(k)
        return greedy(self, *a, **k)
    monkeypatch.setattr(Transformer, "transducer_greedy", recording)
    with torch.no_grad():
        direct = greedy(model, enc, frames, max_symbols=3)
        _, hyps, _ = model.evaluate(src, lengths, tgt, transducer_greedy=True, transducer_max_symbols=3)
        plain = model.evaluate(src, lengths, tgt)[1]
    assert hyps == direct and seen == [dict(max_symbols=3)] and calls == [] and len(plain) == 3
    with pytest.raises(ValueError, match="transducer head alone"):
        model.evaluate(src, lengths, tgt, transducer_beam=True, beam_width=4, transducer_greedy=True)
    with pytest.raises(ValueError, match="1..16"):
        model.evaluate(src, lengths, tgt, transducer_beam=True, beam_width=17)
    assert calls == []


def test_train_py_with_transducer_weight_and_test_py_transducer_beam_search(cli, tmp_path, monkeypatch):
    """train.py --transducer-weight 0.3 for one epoch on the three-utterance manifest (bf16), then test.py's checks and evaluate() with
    --transducer-beam-search --beam-width 4 --beam-nbest 2 --transducer-candidates 3 --transducer-max-symbols 2 on that checkpoint."""
    import test as test_mod
    import train as train_mod
    import utils.functions as UF
    from models.asr.transformer import Transformer
    from models.common_layers import PositionalEncoding
    from utils import constant
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    man, lab = _corpus(tmp_path)
    monkeypatch.chdir(tmp_path)
    cli(["--train-manifest-list", man, "--valid-manifest-list", man, "--test-manifest-list", man, "--labels-path", lab, "--cuda",
         "--batch-size", "3", "--num-workers", "0", "--epochs", "1", "--save-every", "1", "--name", "tinybeam", "--save-folder",
         str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key", "16", "--dim-value", "16",
         "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64", "--label-smoothing", "0.1", "--dropout",
         "0.1", "--k-lr", "20", "--warmup", "5", "--transducer-weight", "0.3", "--transducer-dim-joint", "32", "--transducer-context", "2"])
    train_mod.main()
    path = str(tmp_path / "save" / "tinybeam" / "best_model.th")
    cli(["--cuda", "--continue-from", path, "--tgt-max-len", "301", "--batch-size", "3", "--num-workers", "0", "--transducer-beam-search",
         "--beam-width", "4", "--beam-nbest", "2", "--transducer-candidates", "3", "--transducer-max-symbols", "2"])
    model, _, _, _, largs, l2i, _ = UF.load_model(path)
    assert constant.args.precision == "bf16" and model.rnnt_out.in_features == 32                # the MFMA arm
    test_mod.check_transducer_decoding(constant.args, model)
    test_mod.check_ctc_decoding(constant.args, model)
    model.decoder.positional_encoding = PositionalEncoding(model.decoder.dim_model, 301).cuda()
    ds = SpectrogramDataset(test_mod.feature_conf(largs), [man], l2i, normalize=True)
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    seen = []
    beam = Transformer.transducer_beam_search

    def recording(self, enc_out, lengths, beam_width, **k):
        out = beam(self, enc_out, lengths, beam_width, **dict(k, return_ids=True))
        seen.append((list(lengths), beam_width, k, out[1]))
        return out if k.get("return_ids") else out[0]
    monkeypatch.setattr(Transformer, "transducer_beam_search", recording)
    cer, wer = test_mod.evaluate(model, loader)
    assert np.isfinite(cer) and cer >= 0 and np.isfinite(wer)
    assert len(seen) == 1 and seen[0][1] == 4
    k = seen[0][2]
    assert (k["nbest"], k["candidates"], k["max_symbols"], k["lm"]) == (2, 3, 2, None)
    assert all(1 <= len(rows) <= 2 and all(len(y) <= 2 * n and all(0 < x < len(l2i) for x in y) for y in rows)
               for n, rows in zip(seen[0][0], seen[0][3]))
    for bad in (["--transducer-greedy"], ["--beam-search"], ["--beam-width", "17"]):
        with pytest.raises(ValueError):
            test_mod.check_transducer_decoding(cli(["--cuda", "--continue-from", path, "--transducer-beam-search"] + bad), model)
