"""Tempo / gain perturbation and noise injection, host side (no GPU): the random draws against a restatement of the reference's call
sequence (reference utils/audio.py:49-61, utils/data_loader.py:60-70,145-179), the analysis windows against scipy, the length and
collate conventions, the noise-directory checks, and the emitted gfx950 code of asr_augment_wave.  Also the float32 numpy
restatement of DESIGN.md section 7 that tests/test_gpu_augment.py compares the kernel with bit for bit."""
import os
import re
import sys
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end2end-asr-pytorch_amd"))

SR = 16000


# ------------------------------------------------------------------------------------------------ restatement of the definition
def wsola_constants(sr):
    S = int(np.floor(sr * 82 / 1000 + .5))
    search = int(np.floor(sr * (82 / 5.587) / 1000 + .5))
    O = int(np.floor(max(sr * (82 / 6.833) / 1000 + 4.5, 16)))
    return S, search, O // 8 * 8


def wsola_ref(x, tempo, sr=SR):
    """WSOLA of float32 x at `tempo`: (y (n_out,) float32, offsets of the segments).  Vectorised over the candidates, sequential over
    j, every float32 operation rounded on its own (numpy does not fuse)."""
    x = np.asarray(x, dtype=np.float32)
    S, search, O = wsola_constants(sr)
    half, SO, L = search // 2, S - O, x.size
    n_out = int(np.floor(L / tempo + .5))
    nseg = -(-n_out // SO)

    def fifo(a, n):
        s = np.arange(a, a + n) - half
        v = np.zeros(n, dtype=np.float32)
        ok = (s >= 0) & (s < L)
        v[ok] = x[s[ok]]
        return v

    out = np.zeros(max(nseg, 1) * SO, dtype=np.float32)
    f = np.float32(1) / np.float32(O) * np.arange(O, dtype=np.float32)
    g = np.float32(1) - f
    w = fifo(0, search + S)
    out[:SO] = w[half:half + SO]
    tail = w[half + SO:half + S]
    offs = [half]
    for k in range(1, nseg):
        w = fifo(int(np.floor(tempo * k * SO + .5)), search + S)
        s = np.zeros(search, dtype=np.float32)
        for j in range(O):
            d = w[j:j + search] - tail[j]
            s = s + d * d
        off = int(np.argmin(s))
        out[k * SO:k * SO + O] = tail * g + w[off:off + O] * f
        out[k * SO + O:(k + 1) * SO] = w[off + O:off + SO]
        tail = w[off + SO:off + S]
        offs.append(off)
    return out[:n_out], offs[:nseg]


def gain_ref(y, gain_db):
    m = np.float32(10.0 ** (gain_db / 20.0))
    q = np.rint((y.astype(np.float32) * m) * np.float32(32768))
    return (np.clip(q, -32768, 32767) / np.float32(32768)).astype(np.float32)


def noise_ref(y, noise_i16, start, level):
    """fp64 statement of the mix over the cyclic crop: y + level * n * E_y / E_n (None: skipped, E_n == 0)."""
    n = (noise_i16[(start + np.arange(y.size)) % noise_i16.size].astype(np.float64) / 32768.0)
    ey = np.sqrt((y.astype(np.float64) ** 2).sum() / y.size)
    en = np.sqrt((n ** 2).sum() / y.size)
    if np.float32(en) == 0:
        return None
    return y.astype(np.float64) + level * n * np.float64(np.float32(ey)) / np.float64(np.float32(en))


# ------------------------------------------------------------------------------------------------ helpers
def write_wav(path, samples, sr=SR, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1); f.setsampwidth(width); f.setframerate(sr)
        f.writeframes(np.asarray(samples, dtype="<i2").tobytes())


def noise_dir(tmp_path, lens=(24000, 4000, 9000)):
    d = tmp_path / "noise"
    (d / "sub").mkdir(parents=True)
    rng = np.random.RandomState(5)
    for i, n in enumerate(lens):
        write_wav((d / "sub" if i % 2 else d) / ("n%d.wav" % i), (rng.randn(n) * 3000).clip(-32768, 32767))
    return d


@pytest.fixture
def gpu_frontend_args():
    from utils import constant
    old = constant.args
    constant.parse(["--gpu-frontend"])
    yield constant.args
    constant.set_args(old)


def _conf(nd=None, prob=0.4):
    return dict(sample_rate=SR, window_size=.02, window_stride=.01, window="hamming", noise_dir=None if nd is None else str(nd),
                noise_prob=prob, noise_levels=(0.0, 0.5))


def _reference_draws(n, augment, paths, lens, prob):
    """The reference's sequence of np.random calls for one utterance of n samples."""
    tempo = gain = 0.0
    n_out = n
    if augment:
        tempo = float("{:.3f}".format(np.random.uniform(low=0.85, high=1.15)))
        gain = float("{:.3f}".format(np.random.uniform(low=-6, high=8)))
        n_out = int(np.floor(n / tempo + .5))
    clip, start, level = -1, 0.0, 0.0
    if paths is not None and np.random.binomial(1, float(prob)):
        p = np.random.choice(paths)
        level = np.random.uniform(*(0.0, 0.5))
        start = np.random.rand() * (lens[paths.index(p)] / SR - n_out / SR)
        clip = paths.index(p)
    return (n, tempo, gain, clip, start, level, n_out)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("augment,noise", [(True, False), (False, True), (True, True)])
def test_draws_follow_the_reference_call_sequence(tmp_path, gpu_frontend_args, augment, noise):
    from utils.data_loader import SpectrogramParser
    nd = noise_dir(tmp_path) if noise else None
    p = SpectrogramParser(_conf(nd, prob="0.4"), normalize=True, augment=augment)
    paths = sorted(str(x) for x in (tmp_path / "noise").rglob("*.wav")) if noise else None
    lens = [wave.open(q).getnframes() for q in paths] if noise else None
    if noise:
        assert p.noise_paths == paths
    ns = [16000, 4000, 123457, 1, 30000] * 4
    np.random.seed(77)
    got = [p.draw(n) for n in ns]
    np.random.seed(77)
    exp = [_reference_draws(n, augment, paths, lens, "0.4") for n in ns]
    assert got == exp
    if augment:
        assert all(0.85 <= d[1] <= 1.15 and -6 <= d[2] <= 8 and d[1] == round(d[1], 3) for d in got)
    if noise:
        assert 0 < sum(d[3] >= 0 for d in got) < len(got)


def test_augment_without_the_gpu_front_end_still_refuses():
    from utils import constant
    from utils.data_loader import SpectrogramParser
    old = constant.args
    constant.parse([])
    try:
        with pytest.raises(NotImplementedError, match="GPU front end"):
            SpectrogramParser(_conf(), augment=True)
    finally:
        constant.set_args(old)


@pytest.mark.parametrize("name", ["hamming", "hann", "blackman", "bartlett"])
@pytest.mark.parametrize("n", [320, 321, 400, 2])
def test_windows_match_scipy_symmetric(name, n):
    import scipy.signal
    from utils.audio import window_function
    exp = scipy.signal.windows.get_window(name, n, fftbins=False)
    got = window_function(name, n)
    assert got.dtype == np.float32 and got.shape == (n,)
    np.testing.assert_allclose(got, exp, rtol=0, atol=1e-7)


def test_unknown_window_falls_back_to_hamming(caplog):
    from utils.audio import resolve_window, window_function
    with caplog.at_level("WARNING"):
        assert resolve_window("kaiser") == "hamming"
    assert "kaiser" in caplog.text
    assert np.array_equal(window_function("kaiser", 320), window_function("hamming", 320))


def test_host_spectrogram_uses_the_window():
    from utils.audio import log_spectrogram
    y = np.random.RandomState(1).randn(4000).astype(np.float32)
    a = log_spectrogram(y, window="hann")
    b = log_spectrogram(y)
    assert a.shape == b.shape and not np.allclose(a, b)


def test_wsola_constants_and_tempo_length():
    from utils.audio import tempo_length, wsola_constants as wc
    assert wc(16000) == (1312, 235, 192) == wsola_constants(16000)
    for sr in (8000, 22050, 44100, 48000):
        assert wc(sr) == wsola_constants(sr)
    assert tempo_length(16000, 0.85) == 18824 and tempo_length(16000, 1.15) == 13913 and tempo_length(1, 1.15) == 1
    assert tempo_length(10, 1.0) == 10 and tempo_length(3, 0.997) == 3


def test_restatement_basics():
    x = (np.random.RandomState(2).randn(5000) * 0.1).astype(np.float32)
    y, offs = wsola_ref(x, 1.0)
    S, search, O = wsola_constants(SR)
    assert y.size == 5000 and offs[0] == search // 2
    assert np.array_equal(y[:S - O], x[:S - O])                 # segment 0 is the input
    y, offs = wsola_ref(np.zeros(20000, np.float32), 0.9)
    assert not y.any() and offs[1:] == [0] * (len(offs) - 1)    # silence: every candidate ties, the first wins
    g = gain_ref(np.array([0.9, -0.9, 0.1], np.float32), 8.0)
    assert g[0] == np.float32(32767 / 32768) and g[1] == -1.0


def test_collate_sorts_by_post_tempo_length_and_appends_draws():
    from utils.data_loader import _collate_fn
    items = []
    for n, tempo in ((1000, 1.15), (1050, 0.85), (990, 1.0), (700, 0.0)):
        n_out = int(np.floor(n / tempo + .5)) if tempo else n
        items.append((torch.ones(1, n), [5, 6], (n, tempo, 1.5, -1, 0.0, 0.0, n_out)))
    inputs, targets, pct, sizes, tsizes, draws = _collate_fn(items)
    assert sizes.tolist() == [1235, 990, 870, 700]
    assert draws.dtype == torch.float64 and draws.shape == (4, 6)
    assert draws[:, 0].tolist() == [1050, 990, 1000, 700] and draws[:, 1].tolist() == [0.85, 1.0, 1.15, 0.0]
    assert torch.allclose(pct, torch.tensor([1.0, 990 / 1235, 870 / 1235, 700 / 1235]))
    assert inputs.shape == (4, 1, 1, 1050) and inputs[2, 0, 0, :1000].eq(1).all() and not inputs[2, 0, 0, 1000:].any()
    out = _collate_fn([(torch.ones(1, 5), [1]), (torch.ones(1, 9), [1, 2])])
    assert len(out) == 5 and out[3].tolist() == [9, 5]


def test_noise_dir_validation(tmp_path):
    from utils.audio import noise_files
    d = noise_dir(tmp_path)
    paths, lens = noise_files(str(d), SR)
    assert paths == sorted(paths) and len(paths) == 3 and sorted(lens) == [4000, 9000, 24000]
    with pytest.raises(ValueError, match="sample rate"):
        noise_files(str(d), 8000)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no .wav"):
        noise_files(str(empty), SR)
    with pytest.raises(ValueError, match="not a directory"):
        noise_files(str(tmp_path / "missing"), SR)
    (d / "sub" / "x.flac").write_bytes(b"fLaC")
    with pytest.raises(ValueError, match="non-wav"):
        noise_files(str(d), SR)


def test_augment_kernel_has_no_contracted_f32_arithmetic(tmp_path):
    """The bit-exact definition needs every f32 multiply and add of the search, crossfade, gain and mix rounded separately: the only
    f32 FMAs allowed in asr_augment_wave's code are those of the correctly rounded division sequences (v_div_scale .. v_div_fixup)."""
    import test_isa_static as T
    lines = T._kernel(T._asm(str(tmp_path), "augment.hip"), r"augment_wave_kernel")
    ops = T._ops(lines)
    assert any(o.startswith("ds_read") for o, _ in ops) and any(o == "v_sub_f32_e32" or o.startswith("v_sub_f32") for o, _ in ops)
    in_div = False
    bad = []
    for o, l in ops:
        if o.startswith("v_div_scale_f32"):
            in_div = True
        elif o.startswith("v_div_fixup_f32"):
            in_div = False
        elif re.match(r"v_(pk_)?(fma|fmac|fmamk|fmaak|mad|mac)\w*_f32", o) and not in_div:
            bad.append(l)
    assert not bad, bad[:5]
