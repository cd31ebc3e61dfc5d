"""asr_augment_wave on the GPU (csrc/augment.hip) against the float32 restatement of DESIGN.md section 7 (tests/test_augment_host.py):
WSOLA tempo bit for bit including the chosen offsets, gain and clipping, the noise mix, batch invariance, the augmented front end, and
train.py / test.py with --augment and --noise-dir."""
import random

import numpy as np
import pytest
import torch

import test_augment_host as H

pytestmark = pytest.mark.gpu
SR = 16000
S, SEARCH, O = H.wsola_constants(SR)


@pytest.fixture(scope="module")
def ops():
    from asr_hip import ops as o
    torch.cuda.set_device(0)
    return o


def _signal(kind, n, seed=0):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / SR
    if kind == "white":
        x = rng.randn(n) * 0.2
    elif kind == "chirp":
        x = 0.5 * np.sin(2 * np.pi * (100 * t + 1500 * t * t))
    elif kind == "am":
        x = rng.randn(n) * 0.2 * (0.55 + 0.45 * np.sin(2 * np.pi * 4 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 170 * t))
    else:
        x = np.zeros(n)
    return (np.clip(np.rint(x * 32768), -32768, 32767) / 32768).astype(np.float32)     # what load_audio returns for 16-bit pcm


def _run(ops, xs, params, bank=None, offsets=True):
    """xs: list of float32 waveforms; params: rows {tempo, gain, clip, start_s, level}."""
    B = len(xs)
    Lmax = max(max(x.size for x in xs), 1)
    wav = np.zeros((B, Lmax), np.float32)
    for i, x in enumerate(xs):
        wav[i, :x.size] = x
    r = ops.augment_wave(torch.from_numpy(wav).cuda(), torch.tensor([x.size for x in xs]), torch.tensor(params, dtype=torch.float64),
                         bank, sample_rate=SR, offsets=offsets)
    torch.cuda.synchronize()
    return [t.cpu() for t in r]


LENGTHS = [1, SEARCH // 2 - 5, S - 1, 3 * (S - O), 7 * (S - O), 8 * SR]
TEMPOS = [0.85, 0.997, 1.0, 1.15]


@pytest.mark.parametrize("kind", ["white", "chirp", "am", "silence"])
def test_tempo_is_bit_exact_with_offsets(ops, kind):
    rng = np.random.RandomState(3)
    tempos = TEMPOS + [float("%.3f" % rng.uniform(0.85, 1.15)) for _ in range(2)]
    cases = [(n, t) for n in LENGTHS for t in tempos]
    xs = [_signal(kind, n, seed=i) for i, (n, _) in enumerate(cases)]
    y, lens, offs = _run(ops, xs, [(t, 0.0, -1, 0.0, 0.0) for _, t in cases])
    for i, ((n, t), x) in enumerate(zip(cases, xs)):
        ref, ref_offs = H.wsola_ref(x, t)
        ref = H.gain_ref(ref, 0.0)
        assert int(lens[i]) == ref.size == int(np.floor(n / t + .5)), (n, t)
        assert offs[i, :len(ref_offs)].tolist() == ref_offs, (kind, n, t)
        assert np.array_equal(y[i, :ref.size].numpy().view(np.uint32), ref.view(np.uint32)), (kind, n, t)
        assert not y[i, ref.size:].any()
        if kind == "silence":
            assert ref_offs[1:] == [0] * (len(ref_offs) - 1)


def test_tempo_sixteen_seconds_bit_exact(ops):
    x = _signal("am", 16 * SR, seed=9)
    for t in (0.85, 1.15):
        y, lens, offs = _run(ops, [x], [(t, 0.0, -1, 0.0, 0.0)])
        ref, ref_offs = H.wsola_ref(x, t)
        assert offs[0, :len(ref_offs)].tolist() == ref_offs
        assert np.array_equal(y[0, :ref.size].numpy(), H.gain_ref(ref, 0.0))


def test_gain_and_clipping_bit_exact(ops):
    x = np.sign(_signal("chirp", 3 * SR)).astype(np.float32) * np.float32(32767 / 32768)   # full scale
    x2 = _signal("white", 3 * SR, seed=4)
    y, lens, _ = _run(ops, [x, x2, x2], [(1.0, 8.0, -1, 0, 0), (0.93, -6.0, -1, 0, 0), (1.07, 3.217, -1, 0, 0)])
    for i, (xx, t, g) in enumerate([(x, 1.0, 8.0), (x2, 0.93, -6.0), (x2, 1.07, 3.217)]):
        ref = H.gain_ref(H.wsola_ref(xx, t)[0], g)
        assert np.array_equal(y[i, :ref.size].numpy(), ref)
    assert y[0].max() == np.float32(32767 / 32768) and y[0].min() == -1.0


def _bank(tmp_path, clips):
    from utils.audio import NoiseBank
    d = tmp_path / "noise"
    d.mkdir(exist_ok=True)
    for i, c in enumerate(clips):
        H.write_wav(d / ("c%d.wav" % i), c)
    return NoiseBank(str(d), SR, "cuda"), [np.asarray(c, np.int16) for c in clips]


def test_noise_mix_matches_fp64_and_degenerate_cases_leave_bits(ops, tmp_path):
    rng = np.random.RandomState(6)
    long_clip = (rng.randn(5 * SR) * 4000).clip(-32768, 32767)
    short_clip = (rng.randn(3000) * 4000).clip(-32768, 32767)
    bank, clips = _bank(tmp_path, [long_clip, short_clip, np.zeros(8000)])
    x = _signal("am", 2 * SR, seed=7)
    t, g = 0.91, 2.5
    base = H.gain_ref(H.wsola_ref(x, t)[0], g)
    n_out = base.size
    params = [(t, g, 0, 1.234, 0.37), (t, g, 1, -0.5, 0.8), (t, g, 0, 1.0, 0.0), (t, g, 2, 0.0, 0.4), (t, g, -1, 0.0, 0.0),
              (0.0, 0.0, 1, 0.0, 0.25)]
    y, lens, _ = _run(ops, [x] * len(params), params, bank)
    start0 = int(min(max(np.rint(1.234 * SR), 0), clips[0].size - n_out))
    ref = H.noise_ref(base, clips[0], start0, 0.37)
    assert np.abs(y[0, :n_out].numpy() - ref).max() <= 1e-6
    ref = H.noise_ref(base, clips[1], 0, 0.8)                                 # clip shorter than the utterance: cyclic from 0
    assert np.abs(y[1, :n_out].numpy() - ref).max() <= 1e-6
    for i in (2, 3, 4):                                                       # level 0, a silent clip, no noise: tempo/gain bits
        assert np.array_equal(y[i, :n_out].numpy(), base), i
    ref = H.noise_ref(x, clips[1], 0, 0.25)                                   # noise only: the waveform itself, no tempo / gain
    assert int(lens[5]) == x.size and np.abs(y[5, :x.size].numpy() - ref).max() <= 1e-6


def test_sine_keeps_its_pitch_and_length(ops):
    n = 4 * SR
    x = (0.5 * np.sin(2 * np.pi * 440 * np.arange(n) / SR)).astype(np.float32)
    for t in (0.85, 1.15):
        y, lens, _ = _run(ops, [x], [(t, 0.0, -1, 0, 0)])
        m = int(lens[0])
        assert m == int(np.floor(n / t + .5))
        spec = np.abs(np.fft.rfft(y[0, :m].numpy().astype(np.float64)))
        assert abs(np.argmax(spec) * SR / m - 440) <= SR / m + 1e-9, t


def test_batch_invariance(ops, tmp_path):
    rng = np.random.RandomState(8)
    bank, _ = _bank(tmp_path, [(rng.randn(3 * SR) * 3000).clip(-32768, 32767)])
    xs = [_signal(["white", "chirp", "am"][i % 3], int(rng.randint(100, 6 * SR)), seed=i) for i in range(32)]
    params = [(float("%.3f" % rng.uniform(0.85, 1.15)), float("%.3f" % rng.uniform(-6, 8)), (i % 2) - 1, rng.uniform(0, 1),
               rng.uniform(0, 0.5)) for i in range(32)]
    yb, lb, ob = _run(ops, xs, params, bank)
    for i in (0, 5, 17, 31):
        y1, l1, o1 = _run(ops, [xs[i]], [params[i]], bank)
        n = int(l1[0])
        assert int(lb[i]) == n
        assert np.array_equal(yb[i, :n].numpy().view(np.uint32), y1[0, :n].numpy().view(np.uint32))
        assert ob[i, :o1.shape[1]].tolist() == o1[0].tolist()


@pytest.mark.parametrize("window", ["hamming", "hann", "blackman", "bartlett"])
def test_front_end_matches_host_spectrogram_of_restated_wave(ops, window):
    from utils.audio import gpu_front_end, log_spectrogram
    xs = [_signal("am", n, seed=n) for n in (20000, 16000, 9000)]
    tempos = [1.11, 0.87, 1.0]
    gains = [-3.0, 6.5, 0.0]
    Lmax = max(x.size for x in xs)
    wav = torch.zeros(3, 1, 1, Lmax)
    for i, x in enumerate(xs):
        wav[i, 0, 0, :x.size] = torch.from_numpy(x)
    outs = [H.gain_ref(H.wsola_ref(x, t)[0], g) for x, t, g in zip(xs, tempos, gains)]
    sizes = torch.tensor([o.size for o in outs], dtype=torch.int32)
    aug = torch.tensor([(x.size, t, g, -1, 0.0, 0.0) for x, t, g in zip(xs, tempos, gains)], dtype=torch.float64)
    spect, nfr = gpu_front_end(wav.cuda(), sizes, window=window, aug=aug)
    sp = spect.cpu().numpy()
    for i, o in enumerate(outs):
        ref = log_spectrogram(o, window=window)
        T = ref.shape[1]
        assert int(nfr[i]) == T
        np.testing.assert_allclose(sp[i, 0, :, :T], ref, rtol=0, atol=2e-4 * max(1.0, np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------ entry points
def _corpus(tmp_path, n=6):
    import json
    import wave
    rng = np.random.RandomState(0)
    words = ["ab", "ba", "abba", "bab", "aab", "bba"]
    lines = []
    for i in range(n):
        w = tmp_path / ("u%d.wav" % i)
        ns = 4000 + 800 * i
        with wave.open(str(w), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((rng.randn(ns) * 2000).astype("<i2").tobytes())
        t = tmp_path / ("u%d.txt" % i)
        t.write_text(words[i % len(words)] + "\n")
        lines.append("%s,%s" % (w, t))
    man = tmp_path / "train.csv"
    man.write_text("\n".join(lines))
    lab = tmp_path / "labels.json"
    lab.write_text(json.dumps([" ", "a", "b"]))
    return str(man), str(lab)


def _first_batch(man, l2i, conf):
    from asr_hip import ops
    from utils.audio import noise_bank
    from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
    np.random.seed(1234)
    random.seed(1234)
    ds = SpectrogramDataset(conf, [man], l2i, normalize=True, augment=True)
    loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
    b = next(iter(loader))
    assert len(b) == 6
    wav = b[0].reshape(b[0].shape[0], -1).cuda()
    y, n = ops.augment_wave(wav, b[5][:, 0].long(), b[5][:, 1:], noise_bank(conf["noise_dir"], 16000, wav.device))
    return b, y.cpu(), n.cpu()


def test_train_and_test_with_augment_and_noise(tmp_path, monkeypatch):
    from utils import constant
    man, lab = _corpus(tmp_path)
    nd = H.noise_dir(tmp_path)
    monkeypatch.chdir(tmp_path)
    argv = ["--train-manifest-list", man, "--valid-manifest-list", man, "--test-manifest-list", man, "--labels-path", lab,
            "--cuda", "--batch-size", "3", "--num-workers", "0", "--epochs", "2", "--save-every", "1", "--name", "tinyaug",
            "--save-folder", str(tmp_path / "save"), "--num-layers", "1", "--num-heads", "2", "--dim-model", "32", "--dim-key",
            "16", "--dim-value", "16", "--dim-inner", "64", "--dim-emb", "32", "--tgt-max-len", "12", "--src-max-len", "64",
            "--label-smoothing", "0.1", "--dropout", "0.1", "--k-lr", "20", "--warmup", "5", "--clip", "--shuffle",
            "--augment", "--noise-dir", str(nd), "--noise-prob", "0.6"]
    old = constant.args
    try:
        constant.parse(argv)
        import train as train_mod
        train_mod.main()
        assert constant.args.gpu_frontend and constant.args.graph_buckets > 0
        ck = tmp_path / "save" / "tinyaug"
        state = torch.load(str(ck / "best_model.th"), map_location="cpu", weights_only=False)
        assert np.isfinite(state["metrics"]["train_loss"]) and state["optimizer_params"]["_step"] >= 2
        assert state["args"].noise_dir == str(nd) and state["args"].augment

        from utils.data_loader import AudioDataLoader, BucketingSampler, SpectrogramDataset
        from utils.functions import load_model
        from models.common_layers import PositionalEncoding
        import test as test_mod
        constant.parse(argv + ["--continue-from", str(ck / "best_model.th"), "--tgt-max-len", "301", "--gpu-frontend"])
        model, opt, epoch, metrics, largs, l2i, i2l = load_model(str(ck / "best_model.th"))
        conf = dict(sample_rate=16000, window_size=.02, window_stride=.01, window="hamming", noise_dir=largs.noise_dir,
                    noise_prob=largs.noise_prob, noise_levels=(largs.noise_min, largs.noise_max))
        ds = SpectrogramDataset(conf, [man], l2i, normalize=True)
        loader = AudioDataLoader(ds, num_workers=0, batch_sampler=BucketingSampler(ds, batch_size=3))
        model.decoder.positional_encoding = PositionalEncoding(model.decoder.dim_model, 301).cuda()
        np.random.seed(3)
        cer, wer = test_mod.evaluate(model, loader, noise_dir=largs.noise_dir)
        assert np.isfinite(cer) and np.isfinite(wer)

        b1, s1, n1 = _first_batch(man, l2i, conf)
        b2, s2, n2 = _first_batch(man, l2i, conf)
        assert all(torch.equal(u, v) for u, v in zip(b1, b2))
        assert torch.equal(s1, s2) and torch.equal(n1, n2) and torch.equal(n1.long(), b1[3].long())
        assert (b1[5][:, 1] > 0).all()
    finally:
        constant.set_args(old)
