"""Log-mel filterbank features on the GPU (fbank_logmel_kernel, asr_fbank_finish / asr_fbank_finish_aug in csrc/spectrogram.hip)
against the float64 restatement of tests/fbank_reference.py: the new first pass on synthetic spectra, the normalised and fused forms the
way tests/test_gpu_specaug.py checks asr_spect_finish_aug, the front end end to end against the host path, the vgg_cnn front end at the
even heights these features give it, and a trainer step with replay, checkpoint and test.py's evaluate."""
import math

import numpy as np
import pytest
import torch

import fbank_reference as R
import specaug_reference as SR
import test_gpu_frontend_exact as E
import test_gpu_specaug as S

pytestmark = pytest.mark.gpu
HOP = 160
# |log error| of the first pass (derived, not measured): a sum of at most 21 positive fp32 products carries about 1.4e-6 relative
# error, re^2 + im^2 adds 2 ulp, logf is within a few ulp of a result of magnitude at most 23 (about 3e-6): about 5e-6 in all, and
# 2e-5 leaves a fourfold margin
RAW_TOL = 2e-5
SUM_RTOL = 1e-5


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    torch.cuda.set_device(0)
    return o


def _tiny_bank():
    """K = 7, M = 3: overlapping filters, one starting at bin 0, one ending at bin K - 1."""
    from utils.audio import MelBank
    w = np.array([0.25, 1.0, 0.5, 0.75, 0.125, 0.3, 0.9, 1.0, 0.6], dtype=np.float32)
    return MelBank(np.array([0, 2, 3], dtype=np.int32), np.array([3, 2, 4], dtype=np.int32), w, 7)


def _bank(K, M):
    from utils.audio import MelBank, mel_filterbank
    if M == 2:
        return MelBank(np.array([0, 3], dtype=np.int32), np.array([4, 4], dtype=np.int32), np.linspace(0.2, 1.0, 8).astype(np.float32), 7)
    return _tiny_bank() if K == 7 else mel_filterbank(M, 320, 16000, 20.0 if M == 80 else 0.0)


def _spectra(K, lens, Tmax, extra_ld, seed, scale=3.0):
    """(B * Tmax, ld) random re | im rows with NaN wherever the kernel has no business reading: the rows of frames past each
    utterance's end and the columns from 2 K on."""
    ld = (2 * K + 3) // 4 * 4 + extra_ld
    x = (np.random.RandomState(seed).randn(len(lens) * Tmax, ld) * scale).astype(np.float32)
    x[:, 2 * K:] = np.nan
    for b, n in enumerate(lens):
        x[b * Tmax + min(1 + max(n, 2) // HOP, Tmax):(b + 1) * Tmax] = np.nan
    return x


CASES = {"K 7 M 3": (7, 3, [0, 160, 65 * HOP + 3], 70),                # 1, 2 and 66 frames: the last crosses a 64-frame tile
         "K 161 M 80": (161, 80, [130 * HOP, 64 * HOP - 1, 5], 131),     # 131 (3 frames in the last tile), 64 (exactly one tile), 1
         "K 161 M 40": (161, 40, [3 * HOP, 129 * HOP + 159], 130)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("extra_ld", [0, 12])
def test_first_pass_against_float64(ops, case, extra_ld):
    K, M, lens, Tmax = CASES[case]
    bank = _bank(K, M)
    assert bank.first.size == M and bank.n_bins == K
    x = _spectra(K, lens, Tmax, extra_ld, seed=K + M)
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()
    stats = {}
    got, nf = ops.fbank_finish(torch.from_numpy(x).cuda(), lengths, bank, HOP, normalize=False, stats=stats)
    torch.cuda.synchronize()
    ref, nfr, sums = R.finish(np.nan_to_num(x), lens, R.densify(bank.first, bank.count, bank.weights, K), HOP, Tmax)
    assert got.shape == (len(lens), 1, M, Tmax) and nf.tolist() == nfr
    got = got.cpu().numpy()[:, 0]
    for b, n in enumerate(nfr):
        err = np.abs(got[b, :, :n] - ref[b, :, :n]).max()
        rel = abs(float(stats["sums"][b]) - sums[b]) / abs(sums[b])
        print("%s ld + %d utterance %d (%d frames): max |log err| %.3g, sum %.8g (float64 %.8g, relative %.3g)"
              % (case, extra_ld, b, n, err, float(stats["sums"][b]), sums[b], rel))
        assert err <= RAW_TOL
        assert rel <= SUM_RTOL
        tail = got[b, :, n:]
        assert not tail.any() and not np.signbit(tail).any(), "frames at or past the utterance's count are +0.0"
    assert np.abs(ref).max() < 23.1 and ref[-1, :, 0].std() > 0


def test_first_pass_floor_on_silence(ops):
    """An all-zero spectrum is log of the floor everywhere: every valid value carries the same bits (nothing depends on the filter or
    the frame), the same bits as a spectrum whose energies are positive but below the floor, and those bits are logf(1e-10f).  logf is
    the hardware's log2 (1 ulp of |log2(1e-10)| = 33.2: 2^-18) times ln 2, rounded once more (1 ulp of 23.03: 2^-19), so the value
    lies within 2^-18 ln 2 + 2^-19 = 4.6e-6 of ln(float32(1e-10))."""
    lens, Tmax = [69 * HOP, 2 * HOP], 70
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()
    want = math.log(float(np.float32(1e-10)))
    for K, M in ((7, 3), (161, 80)):
        bank = _bank(K, M)
        x = torch.zeros(len(lens) * Tmax, 2 * K + 2).cuda()
        got, nf = ops.fbank_finish(x, lengths, bank, HOP, normalize=False)
        faint, _ = ops.fbank_finish(x + 1e-7, lengths, bank, HOP, normalize=False)      # energies of 2e-14 per bin: below the floor
        assert torch.equal(got, faint)
        got = got.cpu().numpy()[:, 0]
        for b, n in enumerate(nf.tolist()):
            vals = np.unique(got[b, :, :n].view(np.uint32))
            assert vals.size == 1
            v = float(vals.view(np.float32)[0])
            print("K %d M %d: logf(1e-10f) = %.9g (float64 %.12g)" % (K, M, v, want))
            assert abs(v - want) <= 2.0 ** -18 * math.log(2.0) + 2.0 ** -19 and not got[b, :, n:].any()
        # a floor of the caller's own
        got, _ = ops.fbank_finish(x, lengths, bank, HOP, normalize=False, floor=1.0)
        assert not got.any()


def test_binding_refuses_bad_banks_and_shapes(ops):
    from utils.audio import MelBank
    good = _tiny_bank()
    x = torch.zeros(4, 16).cuda()
    lengths = torch.tensor([0, 0], dtype=torch.int32).cuda()
    ops.fbank_finish(x, lengths, good, HOP, normalize=False)
    bad = [good._replace(first=np.array([0, 2, 4], dtype=np.int32)),                     # 4 + 4 > K
           good._replace(count=np.array([3, 2, 3], dtype=np.int32)),                     # counts do not add up to the weights
           good._replace(first=np.array([-1, 2, 3], dtype=np.int32)),
           good._replace(weights=good.weights.astype(np.float64)),
           MelBank(good.first, good.count, good.weights, 9)]                             # 2 K = 18 columns needed, 16 given
    for b in bad:
        with pytest.raises(ValueError):
            ops.fbank_finish(x, lengths, b, HOP, normalize=False)
    with pytest.raises(ValueError):
        ops.fbank_finish(x[:3], lengths, good, HOP, normalize=False)
    with pytest.raises(ValueError):
        ops.log_spectrogram(torch.zeros(1, 400).cuda(), lengths[:1], features="fbank")
    with pytest.raises(ValueError):
        ops.log_spectrogram(torch.zeros(1, 400).cuda(), lengths[:1], features="fbank", mel=good)      # 7 bins against n_fft 320


@pytest.mark.parametrize("M", [2, 3, 80])
def test_normalised_and_fused_forms_are_the_existing_passes(ops, M):
    """The passes after the first are spect_sqdev_kernel, spect_normalize_kernel and spec_augment_launch with F := M, so what
    tests/test_gpu_specaug.py states of asr_spect_finish_aug holds here: every launch against the float64 reference of what its OWN raw
    values and statistics normalise to (spect_norm_of / spect_norm_apply restated), within the warp bound plus NORM_SLACK; and bit for
    bit against the separate passes (fbank_finish(normalize=True), then ops.spec_augment with the same rows) for every utterance whose
    two launches accumulated the same statistics (float atomics: their order varies between launches) -- unconditionally at M = 2,
    where every statistic is a sum of at most two terms (two 64-frame tiles in the first pass, two rows in the second)."""
    K = 7 if M <= 3 else 161
    bank = ops.fbank_upload(_bank(K, M), "cuda")
    Tmax, T_out = 70, 64
    lens = [69 * HOP + 3, 39 * HOP, 0]
    nfr = [70, 40, 1]
    reim = torch.from_numpy(_spectra(K, lens, Tmax, 0, seed=M)).cuda()
    lengths = torch.tensor(lens, dtype=torch.int32).cuda()
    raw0, _ = ops.fbank_finish(reim, lengths, bank, HOP, normalize=False)
    sep_stats = {}
    spect, nf = ops.fbank_finish(reim, lengths, bank, HOP, normalize=True, stats=sep_stats)
    assert nf.tolist() == nfr and sep_stats["raw"] is None
    s_sep = torch.stack([sep_stats["sums"], sep_stats["sqdev"]]).cpu()
    # the separate launch normalised raw0 (the first pass is deterministic per element) with its own statistics
    x = S._normalised(raw0, s_sep[0], s_sep[1], nfr, M)
    y = spect.cpu().numpy()
    for b, n in enumerate(nfr):
        err, scale = np.abs(y[b, ..., :n].astype(np.float64) - x[b, ..., :n]).max(), np.abs(x[b, ..., :n]).max()
        print("M %d utterance %d: normalised against its own statistics: %.3g (max |x| %.3g)" % (M, b, err, scale))
        assert err <= S.NORM_SLACK * 2.0 ** -24 * scale and not y[b, ..., n:].any()
    cases = {"warp + masks": ([SR.row(64, 20, 31, fmasks=[(1, 1)], tmasks=[(50, 9)]), SR.row(40, 30, 12, tmasks=[(0, 3), (38, 2)]),
                               SR.row(1, fmasks=[(0, 1)])], T_out),
             "identity, cut": ([SR.row(min(n, T_out)) for n in nfr], T_out),
             "identity": ([SR.row(n) for n in nfr], Tmax),
             "T_out 61": ([SR.row(61, 20, 31, fmasks=[(1, 1)], tmasks=[(50, 9)]), SR.row(40, 30, 12), SR.row(1)], 61)}
    same = 0
    for what, (rows, t_out) in cases.items():
        st = {}
        out, nf = ops.fbank_finish(reim, lengths, bank, HOP, spec=torch.tensor(rows, dtype=torch.int32), max_frames=t_out, stats=st)
        torch.cuda.synchronize()
        assert out.shape == (3, 1, M, t_out) and nf.tolist() == [min(n, t_out) for n in nfr]
        assert torch.isfinite(out).all() and out[0].abs().max() > 0
        assert torch.equal(st["raw"], raw0), "the fused launch's first pass"
        sc = torch.stack([st["sums"], st["sqdev"]]).cpu()
        S._check_own_statistics(out, st["raw"], sc, rows, nfr, M, "%s, M %d" % (what, M))
        if what.startswith("identity"):
            sep = spect[..., :t_out]
        else:
            sep = ops.spec_augment(spect[..., :t_out], torch.tensor(rows, dtype=torch.int32))
        same += S._equal_where_statistics_agree(out, sc, sep, s_sep, what)
    print("M %d: %d of 12 comparisons had bit-identical statistics" % (M, same))
    assert M > 2 or same == 12


# ------------------------------------------------------------------------------------------------ end to end
def _batch(lens, seed=0):
    rng = np.random.RandomState(seed)
    ys = [(rng.randn(n) * 0.1).astype(np.float32) for n in lens]
    wav = np.zeros((len(lens), 1, 1, max(lens)), dtype=np.float32)
    for b, y in enumerate(ys):
        wav[b, 0, 0, :y.size] = y
    return ys, torch.from_numpy(wav).cuda(), torch.tensor(lens, dtype=torch.int32)


@pytest.mark.parametrize("M,f_min,cut", [(80, 20.0, None), (80, 20.0, 50), (40, 0.0, None)])
def test_front_end_matches_the_host_path(ops, M, f_min, cut):
    """gpu_front_end(features="fbank") against utils.audio.log_mel_fbank per utterance, atol = 2e-4 * max(1, |ref|max) on the normalised
    features (the project's end-to-end tolerance; a float32 matrix-product DFT alone differs from float64 by about 7e-6 on such noise).
    cut: --src-max-len, applied after the normalisation."""
    from utils.audio import gpu_front_end, log_mel_fbank
    lens = [16000, 12345, 4001, 700]
    ys, wav, sizes = _batch(lens)
    got, nf = gpu_front_end(wav, sizes, src_max_len=cut, features="fbank", num_mel_bins=M, mel_fmin=f_min)
    torch.cuda.synchronize()
    frames = [1 + n // HOP if cut is None else min(1 + n // HOP, cut) for n in lens]
    assert got.shape == (4, 1, M, frames[0]) and nf.tolist() == frames and got.is_contiguous()
    got = got.cpu().numpy()[:, 0]
    for b, y in enumerate(ys):
        ref = log_mel_fbank(y, num_mel_bins=M, f_min=f_min)[:, :frames[b]]
        err = np.abs(got[b, :, :frames[b]] - ref).max()
        print("M %d cut %s utterance %d: max err %.3g (|ref|max %.3g)" % (M, cut, b, err, np.abs(ref).max()))
        assert err <= 2e-4 * max(1.0, np.abs(ref).max())
        assert not got[b, :, frames[b]:].any()


def test_front_end_short_utterances_and_spect_default(ops):
    from utils.audio import gpu_front_end
    lens = [161, 100, 1]
    _, wav, sizes = _batch(lens, seed=1)
    got, nf = gpu_front_end(wav, sizes, features="fbank")
    assert nf.tolist() == [2, 1, 1] and got.shape == (3, 1, 80, 2) and torch.isfinite(got).all()
    assert not got[1:, :, :, 1:].any() and got[0].abs().max() > 0
    plain, nf0 = gpu_front_end(wav, sizes)                                  # the default is the linear features, untouched
    assert plain.shape == (3, 1, 161, 2) and nf0.tolist() == [2, 1, 1]
    with pytest.raises(ValueError):
        gpu_front_end(wav, sizes, features="mfcc")
    with pytest.raises(ValueError, match="--mel-fmin"):
        gpu_front_end(wav, sizes, features="fbank", mel_fmin=0.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(2, 40, 6, 128), (1, 20, 4, 16), (2, 12, 4, 8)])
def test_pool_backward_from_codes_at_pooled_heights_without_whole_chunks(ops, dtype, shape):
    """asr_maxpool_bwd_code in the (B, W/2, C H/2) layout where H/2 is no multiple of the 16-byte chunk (20, 10, 6 pooled rows; 40 x 128
    is conv.7's output for 80 mel bins): the gradient goes where nn.MaxPool2d's backward after a ReLU sends it, bit for bit, and equals
    the backward from the stored activations.  The codes come from the NHWC kernel, permuted to the layout the fused epilogue writes."""
    import torch.nn.functional as F
    B, H, W, C = shape
    H2, W2 = H // 2, W // 2
    g = torch.Generator().manual_seed(H + C)
    x = torch.randn(B, C, H, W, generator=g).relu().to(dtype).float()
    xr = x.clone().requires_grad_()
    ref = F.max_pool2d(xr, 2, stride=2)
    dy = torch.randn(B, C, H2, W2, generator=g).to(dtype).float()
    ref.backward(dy)
    want = (xr.grad * (x > 0)).permute(0, 2, 3, 1).contiguous()
    xd = x.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)
    _, code = ops.maxpool_fwd_code(xd)                                       # (B, H2, W2, C)
    code_tcf = code.permute(0, 2, 3, 1).reshape(B, W2, C * H2).contiguous()
    dy_tcf = dy.reshape(B, C * H2, W2).transpose(1, 2).contiguous().to("cuda", dtype)
    dx = ops.maxpool_bwd_code(code_tcf, dy_tcf, (B, H, W, C), tcf=True)
    assert torch.equal(dx.float().cpu(), want) and want.abs().max() > 0
    assert torch.equal(dx, ops.maxpool_bwd(xd, dy_tcf, tcf=True))


@pytest.mark.parametrize("shape", [(2, 80, 64), (1, 40, 96)])
def test_vgg_front_end_at_even_heights_bit_for_bit(shape):
    """tests/test_gpu_frontend_exact.py at the heights --features fbank gives the model: 80 rows pool to 40, the single-tile arm of the
    weight-stationary kernel instead of the vertical pairs of the odd heights (33, 161, 65) that file runs."""
    from utils import constant
    old = constant.args, constant.explicit, constant.USE_CUDA
    try:
        E.test_front_end_benched_kernels_equal_the_stored_activation_chain_bit_for_bit(shape)
    finally:
        constant.args, constant.explicit, constant.USE_CUDA = old


# ------------------------------------------------------------------------------------------------ trainer, checkpoint, evaluate
def test_trainer_step_replay_checkpoint_and_evaluate(ops, tmp_path, monkeypatch):
    from models.common_layers import PositionalEncoding
    from trainer.asr.trainer import Trainer
    from utils import constant
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    from utils.functions import init_optimizer, init_transformer_model, load_model, save_model
    import test as test_mod
    import train
    man, lab = S._corpus(tmp_path, step=800)                               # 38 .. 63 frames: one 64-frame bucket
    l2i, i2l = train.build_labels(lab)
    old = constant.args, constant.explicit, constant.USE_CUDA
    fbank = S.TINY + ["--features", "fbank", "--save-folder", str(tmp_path / "save"), "--name", "fb"]
    conf = dict(S.CONF, features="fbank", num_mel_bins=80, mel_fmin=20.0)

    def loader(args, which):
        args.train_manifest_list, args.valid_manifest_list = [man], [man]
        tr, valid = train.build_datasets(args, conf, l2i)
        ds = tr if which == "train" else valid[0]
        np.random.seed(21)
        return AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))

    def steps(flag, batch):
        args = constant.parse(fbank + (["--spec-augment"] if flag else []))
        torch.manual_seed(7)
        model = init_transformer_model(args, l2i, i2l).cuda().train()
        assert args.dim_input == 2560
        opt = init_optimizer(args, model, "noam")
        tr = Trainer()
        losses = [tr._run_batch(model, batch, 0.1, "ce", i2l, opt).result()[0] for _ in range(2)]     # eager + capture, then a replay
        assert len(tr._graphs) == 1
        return losses, model, opt

    try:
        args = constant.parse(fbank + ["--spec-augment"])
        b_on = next(iter(loader(args, "train")))
        assert len(b_on) == 7 and b_on[0].shape[2] == 1                    # waveforms; rows drawn over the mel bins
        rows = b_on[6]
        assert (rows[:, 9] <= 20).all() and (rows[:, 8] + rows[:, 9] <= 80).all() and (rows[:, 10] + rows[:, 11] <= 80).all()
        seen = []
        import trainer.asr.trainer as trainer_mod
        real = trainer_mod.gpu_front_end

        def spy(*a, **k):
            out = real(*a, **k)
            seen.append((k.get("features"), tuple(out[0].shape)))
            return out
        monkeypatch.setattr(trainer_mod, "gpu_front_end", spy)
        on, model, opt = steps(True, b_on)
        off, _, _ = steps(False, b_on[:5])
        print("fbank losses with SpecAugment", on, "without", off)
        assert all(np.isfinite(v) for v in on + off)
        assert on[0] != off[0] and on[1] != off[1]
        assert len(seen) == 4 and all(f == "fbank" and s[:3] == (3, 1, 80) and s[3] <= 64 for f, s in seen)
        # the checkpoint carries the feature settings; test.py's loader and evaluate need no feature flag
        constant.parse(fbank + ["--spec-augment"])
        save_model(model, 1, opt, {"train_loss": on[1]}, l2i, i2l)
        path = str(tmp_path / "save" / "fb" / "epoch_1.th")
        constant.parse(["--cuda", "--continue-from", path, "--tgt-max-len", "301", "--batch-size", "3", "--num-workers", "0",
                        "--test-manifest-list", man, "--gpu-frontend"])
        assert constant.args.features == "spect"
        loaded, _, _, _, largs, l2i_ck, _ = load_model(path)
        assert (largs.features, largs.num_mel_bins, largs.mel_fmin) == ("fbank", 80, 20.0) and constant.args.features == "fbank"
        ds = SpectrogramDataset(audio_conf=test_mod.feature_conf(largs), manifest_filepath_list=[man], label2id=l2i_ck, normalize=True)
        assert ds.features == "fbank" and ds.feature_bins == 80
        test_loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
        loaded.decoder.positional_encoding = PositionalEncoding(loaded.decoder.dim_model, 301).cuda()
        shapes = []
        real_eval = loaded.evaluate
        monkeypatch.setattr(loaded, "evaluate", lambda src, *a, **k: (shapes.append(tuple(src.shape)), real_eval(src, *a, **k))[1])
        cer, wer = test_mod.evaluate(loaded, test_loader)
        assert np.isfinite(cer) and np.isfinite(wer)
        assert len(shapes) == 2 and all(s[:3] == (3, 1, 80) for s in shapes), shapes
    finally:
        constant.args, constant.explicit, constant.USE_CUDA = old
