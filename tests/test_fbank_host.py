"""--features fbank on the host (utils/audio.py mel_filterbank / log_mel_fbank, the flags, the model's input width, the loader's
SpecAugment draws and the checkpoint) against the float64 restatement of tests/fbank_reference.py."""
import numpy as np
import pytest
import torch

import fbank_reference as R

TINY = ["--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key", "16", "--dim-value", "16", "--dim-inner", "64",
        "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64", "--dropout", "0.0"]
FBANK = ["--features", "fbank"]


@pytest.fixture
def restore_args():
    from utils import constant
    old = constant.args, constant.explicit, constant.USE_CUDA
    yield constant
    constant.args, constant.explicit, constant.USE_CUDA = old


def _labels():
    from utils import constant
    chars = [constant.PAD_CHAR, constant.SOS_CHAR, constant.EOS_CHAR] + list(" ab")
    l2i = {c: i for i, c in enumerate(chars)}
    return l2i, {i: c for c, i in l2i.items()}


# ------------------------------------------------------------------------------------------------ filter bank
@pytest.mark.parametrize("M,n_fft,sr,f_min", [(80, 320, 16000, 20.0), (40, 320, 16000, 0.0), (64, 320, 16000, 20.0), (23, 400, 8000, 100.0),
                                              (3, 16, 16000, 0.0)])
def test_sparse_bank_is_the_dense_definition(M, n_fft, sr, f_min):
    from utils.audio import mel_filterbank
    bank = mel_filterbank(M, n_fft, sr, f_min)
    K = n_fft // 2 + 1
    assert bank.n_bins == K and bank.first.shape == bank.count.shape == (M,) and bank.weights.dtype == np.float32
    assert bank.first.dtype == bank.count.dtype == np.int32 and int(bank.count.sum()) == bank.weights.size
    assert (bank.count >= 1).all() and (bank.first >= 0).all() and (bank.first + bank.count <= K).all()
    assert np.array_equal(R.densify(bank.first, bank.count, bank.weights, K), R.dense_bank(M, n_fft, sr, f_min))


def test_default_bank_has_no_empty_filter_and_313_weights():
    from utils.audio import mel_filterbank
    bank = mel_filterbank(80, 320, 16000, 20.0)
    w = R.dense_bank(80, 320, 16000, 20.0)
    assert ((w > 0).sum(axis=1) >= 1).all() and (w > 0).sum(axis=1).min() == 1          # the narrowest filter weighs one bin
    assert bank.weights.size == 313 == int((w > 0).sum()) and (bank.weights > 0).all()
    for M, f_min in ((40, 0.0), (40, 20.0), (64, 0.0), (64, 20.0)):
        mel_filterbank(M, 320, 16000, f_min)


@pytest.mark.parametrize("M,n_fft,sr,f_min", [(80, 320, 16000, 20.0), (40, 320, 16000, 0.0), (3, 16, 16000, 0.0)])
def test_adjacent_triangles_sum_to_one(M, n_fft, sr, f_min):
    """Between c_1 and c_M every frequency lies on the falling edge of one filter and the rising edge of the next, which add to 1
    (each weight is a float32 rounding: 2 * 2^-24)."""
    from utils.audio import mel_filterbank
    bank = mel_filterbank(M, n_fft, sr, f_min)
    K = n_fft // 2 + 1
    total = R.densify(bank.first, bank.count, bank.weights, K).sum(axis=0)
    c = R.centres(M, sr, f_min)
    f = np.arange(K) * sr / n_fft
    inside = (f >= c[1]) & (f <= c[M])
    assert inside.sum() >= 2
    assert np.abs(total[inside] - 1.0).max() <= 2 * 2.0 ** -24


def test_hand_computed_bank():
    """sr 16000, n_fft 16, M 3, f_min 0: bins at 0, 1000, .. 8000 Hz; mel(8000) / 4 per step, so c_i = 700 (r^i - 1) with
    r = (1 + 8000/700)^(1/4) = 1.87761: c = 0, 614.33, 1767.79, 3933.55, 8000.
      filter 0 (0, 614.33, 1767.79): 1000 Hz falls at (1767.79 - 1000) / 1153.47 = 0.66564
      filter 1 (614.33, 1767.79, 3933.55): 1000 rises (1000 - 614.33) / 1153.47 = 0.33436; 2000, 3000 fall (3933.55 - f) / 2165.76
      filter 2 (1767.79, 3933.55, 8000): 2000, 3000 rise (f - 1767.79) / 2165.76; 4000 .. 7000 fall (8000 - f) / 4066.45; 8000 is 0."""
    from utils.audio import mel_filterbank
    bank = mel_filterbank(3, 16, 16000, 0.0)
    assert bank.first.tolist() == [1, 1, 2] and bank.count.tolist() == [1, 3, 6] and bank.n_bins == 9
    expect = [0.66564, 0.33436, 0.89278, 0.43105, 0.10722, 0.56895, 0.98366, 0.73774, 0.49183, 0.24591]
    assert np.abs(bank.weights - np.array(expect)).max() < 1e-5


def test_empty_filter_is_refused_at_start_up():
    from utils.audio import mel_filterbank
    from utils.data_loader import SpectrogramParser
    with pytest.raises(ValueError, match="--mel-fmin"):
        mel_filterbank(80, 320, 16000, 0.0)
    conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, features="fbank", num_mel_bins=80, mel_fmin=0.0)
    with pytest.raises(ValueError, match="--num-mel-bins"):
        SpectrogramParser(conf, normalize=True)
    with pytest.raises(ValueError):
        mel_filterbank(0, 320, 16000, 20.0)
    with pytest.raises(ValueError):
        mel_filterbank(80, 320, 16000, 9000.0)


# ------------------------------------------------------------------------------------------------ host features
@pytest.mark.parametrize("n", [5000, 12345, 700])
def test_host_features_match_the_float64_reference(n):
    from utils.audio import log_mel_fbank
    y = (np.random.RandomState(n).randn(n) * 0.1).astype(np.float32)
    for M, f_min in ((80, 20.0), (40, 0.0)):
        ref_raw = R.features(y, M=M, f_min=f_min, normalize=False)
        raw = log_mel_fbank(y, normalize=False, num_mel_bins=M, f_min=f_min)
        norm = log_mel_fbank(y, normalize=True, num_mel_bins=M, f_min=f_min)
        assert raw.shape == norm.shape == (M, 1 + n // 160) and raw.dtype == norm.dtype == np.float32
        e_raw, e_norm = np.abs(raw - ref_raw).max(), np.abs(norm - R.normalise(ref_raw)).max()
        print("n %d M %d: raw %.3g normalised %.3g" % (n, M, e_raw, e_norm))
        assert e_raw < 1e-4 and e_norm < 5e-4


def test_host_features_of_silence_and_other_windows():
    from utils.audio import log_mel_fbank
    raw = log_mel_fbank(np.zeros(1000, np.float32), normalize=False)
    assert raw.shape == (80, 7) and (raw == np.float32(np.log(1e-10))).all()
    y = (np.random.RandomState(3).randn(3000) * 0.1).astype(np.float32)
    got = log_mel_fbank(y, normalize=False, window="hann", num_mel_bins=64)
    assert np.abs(got - R.features(y, M=64, normalize=False, window="hann")).max() < 1e-4
    assert log_mel_fbank(np.zeros(1, np.float32), normalize=False).shape == (80, 1)


def test_loader_host_path_returns_fbank_features(tmp_path, restore_args):
    """--gpu-frontend off: the dataset's parse_audio is log_mel_fbank with the audio_conf's settings; `spect` stays what it was."""
    import wave
    from utils.audio import log_mel_fbank, log_spectrogram
    from utils.data_loader import SpectrogramParser
    restore_args.parse(TINY)
    pcm = (np.random.RandomState(0).randn(4000) * 2000).astype("<i2")
    path = str(tmp_path / "u.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    y = pcm.astype(np.float32) / 32768.0
    conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window="hamming")
    got = SpectrogramParser(dict(conf, features="fbank", num_mel_bins=40, mel_fmin=0.0), normalize=True).parse_audio(path)
    assert got.shape == (40, 26) and np.array_equal(got.numpy(), log_mel_fbank(y, num_mel_bins=40, f_min=0.0))
    plain = SpectrogramParser(conf, normalize=True).parse_audio(path)
    assert plain.shape == (161, 26) and np.array_equal(plain.numpy(), log_spectrogram(y))


# ------------------------------------------------------------------------------------------------ plumbing
def test_flags_and_model_input_width(restore_args):
    from utils.audio import feature_bins
    from utils.functions import init_transformer_model
    constant = restore_args
    l2i, i2l = _labels()
    a = constant.parse(TINY)
    assert (a.features, a.num_mel_bins, a.mel_fmin) == ("spect", 80, 20.0) and feature_bins(a) == 161
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 5120
    a = constant.parse(TINY + ["--feat_extractor", ""])
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 161
    a = constant.parse(TINY + ["--feat_extractor", "", "--dim-input", "7"])         # spect without a CNN: untouched, as before
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 7
    a = constant.parse(TINY + FBANK)
    assert feature_bins(a) == 80
    model = init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 2560 and model.encoder.input_linear.weight.shape[1] == 2560
    a = constant.parse(TINY + FBANK + ["--num-mel-bins", "40"])
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 1280
    a = constant.parse(TINY + FBANK + ["--feat_extractor", ""])
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 80
    a = constant.parse(TINY + FBANK + ["--feat_extractor", "", "--dim-input", "80"])
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 80
    with pytest.raises(ValueError, match="--dim-input"):
        init_transformer_model(constant.parse(TINY + FBANK + ["--feat_extractor", "", "--dim-input", "161"]), l2i, i2l)
    with pytest.raises(ValueError, match="emb_cnn"):
        init_transformer_model(constant.parse(TINY + FBANK + ["--feat_extractor", "emb_cnn"]), l2i, i2l)
    a = constant.parse(TINY + ["--feat_extractor", "emb_cnn"])
    init_transformer_model(a, l2i, i2l)
    assert a.dim_input == 672
    with pytest.raises(SystemExit):
        constant.parse(["--features", "mfcc"])


def test_draw_spec_masks_stay_inside_the_mel_bins(restore_args):
    from utils.data_loader import SpectrogramParser, spec_policy
    constant = restore_args
    args = constant.parse(TINY + FBANK + ["--num-mel-bins", "40", "--mel-fmin", "0", "--gpu-frontend", "--spec-augment",
                                          "--spec-freq-mask", "60", "--src-max-len", "4000"])
    conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, features=args.features, num_mel_bins=args.num_mel_bins,
                mel_fmin=args.mel_fmin)
    parser = SpectrogramParser(conf, normalize=True, spec_augment=spec_policy(args))
    assert parser.feature_bins == 40
    np.random.seed(5)
    widest = 0
    for i in range(1000):
        row = parser.draw_spec(16000 + 37 * i)
        for k in range(row[3]):
            f0, fw = row[8 + 2 * k], row[9 + 2 * k]
            assert 0 <= f0 and 0 <= fw and f0 + fw <= 40, row
            widest = max(widest, fw)
    assert widest == 40                                      # --spec-freq-mask 60 is capped by the 40 bins, and the cap is reached
    plain = SpectrogramParser(dict(sample_rate=16000, window_size=.02, window_stride=.01), normalize=True, spec_augment=spec_policy(args))
    assert plain.feature_bins == 161


def _save_tiny(constant, tmp_path, extra):
    from utils.functions import init_optimizer, init_transformer_model, save_model
    l2i, i2l = _labels()
    args = constant.parse(TINY + ["--save-folder", str(tmp_path), "--name", "m"] + extra)
    model = init_transformer_model(args, l2i, i2l)
    opt = init_optimizer(args, model, "noam")
    save_model(model, 3, opt, {"loss": 1.0}, l2i, i2l)
    return str(tmp_path / "m" / "epoch_3.th"), model


def test_checkpoint_keeps_the_feature_settings(tmp_path, restore_args):
    import test as test_py
    from utils.functions import load_model
    constant = restore_args
    path, model = _save_tiny(constant, tmp_path, FBANK + ["--num-mel-bins", "40", "--mel-fmin", "0"])
    constant.parse(["--continue-from", path])                               # no feature flag on this command line
    assert constant.args.features == "spect"
    loaded, _, epoch, _, largs, _, _ = load_model(path)
    assert epoch == 3 and (largs.features, largs.num_mel_bins, largs.mel_fmin) == ("fbank", 40, 0.0) and largs.dim_input == 1280
    assert (constant.args.features, constant.args.num_mel_bins, constant.args.mel_fmin) == ("fbank", 40, 0.0)
    for k, v in model.state_dict().items():
        assert torch.equal(v, loaded.state_dict()[k]), k
    conf = test_py.feature_conf(largs)
    assert (conf["features"], conf["num_mel_bins"], conf["mel_fmin"]) == ("fbank", 40, 0.0)
    # retyping the checkpoint's own settings is fine; anything else is an error, not an override
    constant.parse(["--continue-from", path, "--features", "fbank", "--num-mel-bins", "40"])
    load_model(path)
    for bad in (["--features", "spect"], ["--num-mel-bins", "80"], ["--mel-fmin", "20"]):
        constant.parse(["--continue-from", path] + bad)
        with pytest.raises(ValueError, match="cannot be changed"):
            load_model(path)


def test_checkpoint_without_feature_settings_is_spect(tmp_path, restore_args):
    from utils.functions import load_model
    constant = restore_args
    path, _ = _save_tiny(constant, tmp_path, [])
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    for k in ("features", "num_mel_bins", "mel_fmin"):
        delattr(ckpt["args"], k)                                             # as written before --features existed
    torch.save(ckpt, path)
    constant.parse(["--continue-from", path])
    _, _, _, _, largs, _, _ = load_model(path)
    assert largs.features == "spect" and largs.dim_input == 5120 and constant.args.features == "spect"
    constant.parse(["--continue-from", path, "--features", "fbank"])
    with pytest.raises(ValueError, match="cannot be changed"):
        load_model(path)
