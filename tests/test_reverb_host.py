"""Reverberation with room impulse responses, host side (no GPU): prepare_rir against the restatement (tests/reverb_reference.py) on
hand-made responses, the directory's refusals, the loader's draws and collate conventions, the command line, and the entry point's
declaration."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reverb_reference as VR  # noqa: E402
import test_augment_host as H  # noqa: E402

SR = 16000


def _conf(rir_dir=None, prob=0.5, speed=None, noise=None, max_ms=500):
    c = dict(sample_rate=SR, window_size=.02, window_stride=.01, window="hamming", noise_dir=None if noise is None else str(noise),
             noise_prob=0.4, noise_levels=(0.0, 0.5))
    if speed is not None:
        c["speed_perturb"] = speed
    if rir_dir is not None:
        c.update(rir_dir=str(rir_dir), rir_prob=prob, rir_max_ms=max_ms)
    return c


def rir_dir(tmp_path, count=3, name="rirs"):
    """A directory of `count` decaying-noise responses as 16-bit wavs, each with some silence before its direct path."""
    d = tmp_path / name
    (d / "sub").mkdir(parents=True)
    rng = np.random.RandomState(3)
    for i in range(count):
        n = 600 + 250 * i
        h = rng.randn(n) * np.exp(-np.arange(n) / (60.0 + 30 * i))
        h[0] = 4.0
        h = np.concatenate([np.zeros(7 + i), h])
        H.write_wav((d / "sub" if i % 2 else d) / ("r%d.wav" % i), (h * 6000).clip(-32768, 32767))
    return d


@pytest.fixture
def gpu_frontend_args():
    from utils import constant
    old = constant.args
    constant.parse(["--gpu-frontend"])
    yield constant.args
    constant.set_args(old)


# ------------------------------------------------------------------------------------------------ prepare_rir
def test_prepare_drops_what_precedes_the_first_of_two_equal_peaks():
    from utils.audio import prepare_rir
    h = np.array([0.0, 0.1, -0.8, 0.3, 0.8, -0.2, 0.05])
    got = prepare_rir(h, SR, 500)
    exp = h[2:] / np.sqrt(np.sum(h[2:] ** 2))
    assert got.dtype == np.float32 and got.size == 5 and np.array_equal(got, exp.astype(np.float32))
    assert np.array_equal(got, VR.prepare(h, SR, 500).astype(np.float32))
    assert got[0] < 0 and abs(got[0]) == abs(got[2])                            # the direct path sits at lag 0


def test_prepare_caps_the_taps():
    from utils.audio import prepare_rir
    rng = np.random.RandomState(0)
    h = np.concatenate([np.zeros(3), [2.0], rng.uniform(0.5, 1.0, 400)])
    assert prepare_rir(h, SR, 10).size == 160 and prepare_rir(h, SR, 500).size == 401           # floor(10 ms * 16 kHz) taps from k0
    assert prepare_rir(h, 8000, 1.99).size == 15 and prepare_rir(h, SR, 1 / 16.0).size == 1     # floor(15.92), and the least cap
    for ms, sr in ((10, SR), (1.99, 8000), (0.0625, SR), (500, SR)):
        assert np.array_equal(prepare_rir(h, sr, ms), VR.prepare(h, sr, ms).astype(np.float32))
    with pytest.raises(ValueError, match="rir-max-ms"):
        prepare_rir(h, SR, 0.05)                                                # Lcap = 0


def test_prepare_trims_the_tail_below_minus_sixty_db():
    from utils.audio import prepare_rir
    h = np.array([0.0, 1.0, 0.5, 0.0009, 0.001, 0.0005, 0.00099, 0.0, 0.0])
    got = prepare_rir(h, SR, 500)
    assert got.size == 4                                                        # 1.0, 0.5, 0.0009 (inside), 0.001 (the last at -60 dB)
    assert np.array_equal(got, VR.prepare(h, SR, 500).astype(np.float32))
    assert prepare_rir(np.array([0.0, -3.0, 0.0, 0.0]), SR, 500).tolist() == [-1.0]
    # the cap applies before the trim: a loud tap behind the cap does not keep the quiet ones in front of it
    assert prepare_rir(np.array([1.0, 0.5, 0.0001, 0.0001, 0.7]), SR, 0.25).size == 2


def test_prepare_gives_unit_energy_in_float64_before_the_cast():
    from utils.audio import prepare_rir
    rng = np.random.RandomState(1)
    for n in (1, 2, 100, 8000):
        h = rng.randn(n) * np.exp(-np.arange(n) / 900.0)
        ref = VR.prepare(h, SR, 500)
        assert abs(np.sum(ref ** 2) - 1.0) <= 1e-12
        got = prepare_rir(h, SR, 500)
        assert np.array_equal(got, ref.astype(np.float32))
        assert abs(np.sum(got.astype(np.float64) ** 2) - 1.0) <= 1e-6          # and the float32 taps are unit energy to their rounding
    assert prepare_rir(h.astype(np.float32), SR, 500).dtype == np.float32


def test_prepare_and_the_directory_refuse(tmp_path):
    from utils.audio import RirBank, prepare_rir, prepared_rirs, rir_files
    for bad in (np.zeros(0), np.zeros(10)):
        with pytest.raises(ValueError, match="empty or all-zero"):
            prepare_rir(bad, SR, 500)
    with pytest.raises(ValueError, match="not a directory"):
        rir_files(str(tmp_path / "nowhere"), SR)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .wav files"):
        rir_files(str(tmp_path / "empty"), SR)
    d = rir_dir(tmp_path)
    paths, lens = rir_files(str(d), SR)
    assert [os.path.basename(p) for p in paths] == ["r0.wav", "r2.wav", "r1.wav"] and lens == [607, 1109, 858]      # sorted paths
    with pytest.raises(ValueError, match="sample rate 16000, not --sample-rate 8000"):
        rir_files(str(d), 8000)
    (d / "x.flac").write_bytes(b"")
    with pytest.raises(ValueError, match="non-wav audio"):
        rir_files(str(d), SR)
    os.remove(str(d / "x.flac"))
    H.write_wav(d / "zero.wav", np.zeros(50))
    with pytest.raises(ValueError, match="zero.wav.*all-zero"):
        prepared_rirs(str(d), SR, 500)
    with pytest.raises(ValueError, match="at least one"):
        RirBank.from_arrays([], "cpu")
    # the noise directory keeps its own words under the shared rules
    from utils.audio import noise_files
    with pytest.raises(ValueError, match="--noise-dir .* is not a directory"):
        noise_files(str(tmp_path / "nowhere"), SR)


def test_the_bank_concatenates_prepared_taps(tmp_path):
    from utils.audio import RirBank, load_audio, prepared_rirs, rir_bank
    d = rir_dir(tmp_path)
    paths, taps = prepared_rirs(str(d), SR, 20)
    assert len(taps) == 3 and all(t.dtype == np.float32 and t.size <= 320 for t in taps)
    for p, t in zip(paths, taps):
        assert np.array_equal(t, VR.prepare(load_audio(p), SR, 20).astype(np.float32))
        assert t[0] == np.abs(t).max()
    bank = rir_bank(str(d), SR, 20, "cpu")
    assert bank is rir_bank(str(d), SR, 20, "cpu") and bank is not rir_bank(str(d), SR, 30, "cpu") and len(bank) == 3
    assert bank.data.dtype == torch.float32 and bank.offsets.dtype == torch.int64 and bank.lens.dtype == torch.int64
    assert bank.lens.tolist() == [t.size for t in taps] and bank.offsets.tolist() == [0, taps[0].size, taps[0].size + taps[1].size]
    assert np.array_equal(bank.data.numpy(), np.concatenate(taps))
    raw = RirBank.from_arrays([np.array([1, 2, 3]), np.array([-8.0])], "cpu")     # as they are: no peak search, no scaling
    assert raw.data.tolist() == [1.0, 2.0, 3.0, -8.0] and raw.offsets.tolist() == [0, 3] and raw.lens.tolist() == [3, 1] and len(raw) == 2


def test_the_restatement_on_a_hand_checked_sum():
    x = np.array([1, 2, 3, 4], np.float32)
    h = np.array([1, -1, 2], np.float32)
    y, mag = VR.reverb64(x, h)
    assert y.tolist() == [1.0, 1.0, 3.0, 5.0] and mag.tolist() == [1.0, 3.0, 7.0, 11.0]        # the tail (2, 8 behind n) is cut
    assert VR.reverb32_exact(x, h, 2).tolist() == [1.0, 1.0] and VR.reverb64(x, h, 0)[0].size == 0
    with pytest.raises(AssertionError):
        VR.reverb32_exact(x * 0.3, h)


# ------------------------------------------------------------------------------------------------ draws and collate
@pytest.mark.parametrize("augment,noise,speed", [(False, False, None), (True, False, None), (True, True, None), (False, False, [0.9, 1.1]),
                                                 (True, True, [0.9, 1.0, 1.1])])
def test_draws_come_after_the_existing_ones_and_append_the_index(tmp_path, gpu_frontend_args, augment, noise, speed):
    from utils.data_loader import SpectrogramParser
    nd = H.noise_dir(tmp_path) if noise else None
    d = rir_dir(tmp_path, count=3)
    ns = [16000, 4000, 123457, 1, 30000] * 4
    plain = SpectrogramParser(_conf(speed=speed, noise=nd), normalize=True, augment=augment)
    with_rir = SpectrogramParser(_conf(d, prob=0.5, speed=speed, noise=nd), normalize=True, augment=augment)
    assert with_rir.rir_count == 3 and with_rir.augmenting and plain.rir_count is None
    np.random.seed(21)
    got = [with_rir.draw(n) for n in ns]
    np.random.seed(21)
    for n, g in zip(ns, got):
        before = plain.draw(n) if plain.augmenting else (n, 0.0, 0.0, -1, 0.0, 0.0, n)
        hit = np.random.binomial(1, 0.5)                                        # after the utterance's own draws
        idx = int(np.random.randint(3)) if hit else -1
        assert len(g) == 9 and g[:7] == before[:7] and g[7] == (before[7] if speed else 0) and g[8] == idx
    assert {g[8] for g in got} == {-1, 0, 1, 2}
    always = SpectrogramParser(_conf(d, prob=1.0), normalize=True)
    never = SpectrogramParser(_conf(d, prob=0.0), normalize=True)
    assert all(always.draw(50)[8] >= 0 for _ in range(20)) and all(never.draw(50)[8] == -1 for _ in range(20))


@pytest.mark.parametrize("augment", [False, True])
def test_draws_without_a_directory_are_what_they_were(tmp_path, gpu_frontend_args, augment):
    from utils.audio import noise_files
    from utils.data_loader import SpectrogramParser
    nd = H.noise_dir(tmp_path)
    paths, lens = noise_files(str(nd), SR)
    p = SpectrogramParser(_conf(noise=nd), normalize=True, augment=augment)
    assert p.rir_count is None and p.rir_dir is None
    ns = [16000, 4000, 123457, 1, 30000] * 3
    np.random.seed(5)
    got = [p.draw(n) for n in ns]
    state = np.random.get_state()[1].copy()
    np.random.seed(5)
    exp = [H._reference_draws(n, augment, paths, lens, "0.4") for n in ns]
    assert got == exp and all(len(d) == 7 for d in got)
    assert np.array_equal(state, np.random.get_state()[1])                      # and consumed the same random numbers
    sp = SpectrogramParser(_conf(speed=[0.9, 1.1]), normalize=True)
    assert len(sp.draw(1000)) == 8 and not SpectrogramParser(_conf(), normalize=True).augmenting


def test_collate_emits_eight_columns_with_the_index_last():
    from utils.data_loader import _collate_fn
    items = []
    for n, p, rir in ((1000, 1100, 2), (1000, 900, -1), (1040, 1000, 0)):
        n_out = (2 * n * 1000 + p) // (2 * p)
        items.append((torch.ones(1, n), [5, 6], (n, 0.0, 0.0, -1, 0.0, 0.0, n_out, p, rir)))
    inputs, targets, pct, sizes, tsizes, draws = _collate_fn(items)
    assert sizes.tolist() == [1111, 1040, 909] and draws.dtype == torch.float64 and draws.shape == (3, 8)
    assert draws[:, 6].tolist() == [900, 1000, 1100] and draws[:, 7].tolist() == [-1, 0, 2] and draws[:, 0].tolist() == [1000, 1040, 1000]
    # without a speed list column 6 is 0
    no_speed = _collate_fn([(torch.ones(1, n), [5], (n, 0.0, 0.0, -1, 0.0, 0.0, n, 0, r)) for n, r in ((10, 1), (30, -1))])[5]
    assert no_speed.shape == (2, 8) and no_speed[:, 6].tolist() == [0, 0] and no_speed[:, 7].tolist() == [-1, 1]
    # with SpecAugment rows the draws stay the sixth element
    out = _collate_fn([it + ([0] * 40,) for it in items])
    assert len(out) == 7 and out[5].shape == (3, 8) and out[6].shape == (3, 40)
    # and the shapes from before: seven columns with a speed list alone, six without
    assert _collate_fn([(torch.ones(1, 10), [1], (10, 1.0, 0.0, -1, 0.0, 0.0, 10, 1000))])[5].shape == (1, 7)
    assert _collate_fn([(torch.ones(1, 10), [1], (10, 1.0, 0.0, -1, 0.0, 0.0, 10))])[5].shape == (1, 6)


# ------------------------------------------------------------------------------------------------ command line
def test_flags_defaults_and_range_refusals():
    from utils import constant
    old = constant.args
    try:
        a = constant.parse([])
        assert a.rir_dir is None and a.rir_prob == 0.5 and a.rir_max_ms == 500
        a = constant.parse(["--rir-dir", "rooms", "--rir-prob", "1", "--rir-max-ms", "250.5"])
        assert a.rir_dir == "rooms" and a.rir_prob == 1.0 and a.rir_max_ms == 250.5
        assert constant.parse(["--rir-prob", "0"]).rir_prob == 0.0
        for bad in (["--rir-prob", "1.01"], ["--rir-prob", "-0.1"], ["--rir-prob", "nan"], ["--rir-max-ms", "0"], ["--rir-max-ms", "-5"]):
            with pytest.raises(SystemExit):
                constant.parse(bad)
        assert "--rir-dir" in constant.__doc__ and "--rir-prob" in constant.__doc__ and "--rir-max-ms" in constant.__doc__
    finally:
        constant.set_args(old)


def test_reverberation_without_the_gpu_front_end_refuses(tmp_path):
    from utils import constant
    from utils.data_loader import SpectrogramParser
    d = rir_dir(tmp_path)
    old = constant.args
    constant.parse(["--rir-dir", str(d)])
    try:
        with pytest.raises(NotImplementedError, match="GPU front end"):
            SpectrogramParser(_conf(d))
        SpectrogramParser(_conf())                                              # the flag alone asks nothing of a dataset without the settings
        constant.parse(["--gpu-frontend"])
        for kw in (dict(prob=1.5), dict(max_ms=0)):
            with pytest.raises(ValueError, match="rir-prob"):
                SpectrogramParser(_conf(d, **kw))
        with pytest.raises(ValueError, match="not a directory"):               # at start-up, not at the first batch
            SpectrogramParser(_conf(tmp_path / "nowhere"))
        H.write_wav(d / "zero.wav", np.zeros(50))
        with pytest.raises(ValueError, match="all-zero"):
            SpectrogramParser(_conf(d))
    finally:
        constant.set_args(old)


def test_train_turns_the_front_end_on_and_only_the_training_set_reverberates(tmp_path):
    import train
    from utils import constant
    d = rir_dir(tmp_path)
    old = constant.args
    try:
        assert not train.augments_on_the_front_end(constant.parse(["--cuda"]))
        assert not train.augments_on_the_front_end(constant.parse(["--cuda", "--rir-prob", "1.0"]))
        assert train.augments_on_the_front_end(constant.parse(["--cuda", "--rir-dir", str(d)]))
        wav = tmp_path / "u.wav"
        H.write_wav(wav, np.zeros(800))
        (tmp_path / "u.txt").write_text("ab\n")
        man = tmp_path / "m.csv"
        man.write_text("%s,%s\n" % (wav, tmp_path / "u.txt"))
        a = constant.parse(["--gpu-frontend", "--rir-dir", str(d), "--rir-prob", "1.0", "--rir-max-ms", "20"])
        a.train_manifest_list, a.valid_manifest_list = [str(man)], [str(man)]
        tr, valid = train.build_datasets(a, _conf(), {"a": 3, "b": 4})
        assert tr.rir_count == 3 and tr.rir_prob == 1.0 and tr.rir_max_ms == 20 and tr.augmenting
        item = tr[0]
        assert len(item) == 3 and len(item[2]) == 9 and item[2][:8] == (800, 0.0, 0.0, -1, 0.0, 0.0, 800, 0) and item[2][8] in (0, 1, 2)
        assert valid[0].rir_count is None and valid[0].rir_dir is None and not valid[0].augmenting and len(valid[0][0]) == 2
        a = constant.parse(["--gpu-frontend", "--rir-dir", str(d), "--speed-perturb", "0.9", "1.1"])
        a.train_manifest_list, a.valid_manifest_list = [str(man)], [str(man)]
        tr, valid = train.build_datasets(a, _conf(), {"a": 3, "b": 4})
        assert tr.speed == [900, 1100] and tr.rir_count == 3 and tr.rir_prob == 0.5 and len(tr[0][2]) == 9 and valid[0].speed is None
    finally:
        constant.set_args(old)


# ------------------------------------------------------------------------------------------------ the entry point
def test_the_entry_point_is_declared_with_a_signature_of_the_same_length():
    from asr_hip import lib as L
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    m = re.search(r"\bint asr_reverb\(([^)]*)\);", text)
    assert m, "asr_reverb is not declared in include/asr_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = L._SIGS["asr_reverb"]
    assert len(params) == len(args) == 14 and params[-1] == "asr_stream_t stream"
    tile = int(re.search(r"#define ASR_REVERB_TILE (\d+)", text).group(1))
    chunk = int(re.search(r"#define ASR_REVERB_CHUNK (\d+)", text).group(1))
    from asr_hip import ops
    assert (ops.REVERB_TILE, ops.REVERB_CHUNK) == (tile, chunk) and tile % 8 == 0 and chunk % 4 == 0 and chunk + 1 <= 1000
    assert "reverb.hip" in os.listdir(os.path.join(ROOT, "end2end-asr-pytorch_amd", "csrc"))
