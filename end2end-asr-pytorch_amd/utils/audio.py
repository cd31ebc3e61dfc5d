"""Waveform loading and the spectrogram front end (reference: utils/audio.py:7-15 and SpectrogramParser.parse_audio,
utils/data_loader.py:60-91).  Own implementation on numpy only: the reference's torchaudio / librosa / sox dependencies
are not part of this build.  The reference's sox-based tempo/gain augmentation and noise injection (audio.py:17-61,
data_loader.py:145-179) run on the GPU instead (asr_augment_wave, csrc/augment.hip; definition in DESIGN.md section 7): the host
keeps the random draws (utils/data_loader.py), gpu_front_end applies them to the batch before the STFT.
--speed-perturb (no counterpart in the reference): band-limited resampling by a factor drawn per utterance (speed_ratio, speed_length,
resample_table; asr_resample, csrc/resample.hip), ahead of tempo / gain / noise.
--rir-dir (no counterpart in the reference): reverberation with recorded room impulse responses (rir_files, prepare_rir, RirBank;
asr_reverb, csrc/reverb.hip), after the speed change and ahead of tempo / gain / noise.
--features fbank (no counterpart in the reference): log-mel filterbank features of the same STFT (mel_filterbank, log_mel_fbank;
definition in DESIGN.md section 7).
"""
import collections
import glob
import logging
import os
import wave

import numpy as np

WINDOWS = ("hamming", "hann", "blackman", "bartlett")
# what the reference's noise loader (librosa.util.find_files) would also pick up; only wav is read here
AUDIO_EXTENSIONS = (".aac", ".au", ".flac", ".m4a", ".mp3", ".ogg", ".wav")


def load_audio(path):
    """16-bit / 32-bit PCM wav -> float32 in [-1, 1], channels averaged (reference: audio.py:7-15)."""
    with wave.open(path, "rb") as f:
        nch, width, n = f.getnchannels(), f.getsampwidth(), f.getnframes()
        raw = f.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError("unsupported sample width %d in %s" % (width, path))
    if nch > 1:
        x = x.reshape(-1, nch).mean(axis=1)
    return x


def hamming_window(n):
    """Symmetric Hamming window: the reference passes scipy.signal.hamming as a CALLABLE to librosa, which evaluates
    it as window(n) i.e. sym=True (data_loader.py:20-21,77-79)."""
    return window_function("hamming", n)


def resolve_window(name):
    """--window: one of WINDOWS; anything else is Hamming with a warning, as the reference's windows.get(name, hamming)
    (data_loader.py:20-21,55)."""
    if name in WINDOWS:
        return name
    logging.warning("unknown --window %r: using the hamming window (as the reference does)", name)
    return "hamming"


def window_function(name, n):
    """Symmetric (scipy.signal.<name>(n), sym=True) window of n points as float32, computed in float64."""
    name = resolve_window(name)
    if n == 1:
        return np.ones(1, dtype=np.float32)
    k = np.arange(n, dtype=np.float64)
    a = 2.0 * np.pi * k / (n - 1)
    if name == "hamming":
        w = 0.54 - 0.46 * np.cos(a)
    elif name == "hann":
        w = 0.5 - 0.5 * np.cos(a)
    elif name == "blackman":
        w = 0.42 - 0.5 * np.cos(a) + 0.08 * np.cos(2.0 * a)
    else:                                                   # bartlett
        w = np.where(k <= (n - 1) / 2.0, 2.0 * k / (n - 1), 2.0 - 2.0 * k / (n - 1))
    return w.astype(np.float32)


def _windowed_frames(y, n_fft, hop, window):
    """float waveform -> (frames, n_fft) float32 windowed frames: centred, reflect padded (zero padded when the signal is no longer
    than n_fft / 2), a signal shorter than 2 samples padded to 2.  The framing both feature types share."""
    y = np.asarray(y, dtype=np.float32)
    if y.size < 2:
        y = np.pad(y, (0, 2 - y.size))
    pad = n_fft // 2
    yp = np.pad(y, (pad, pad), mode="reflect") if y.size > pad else np.pad(y, (pad, pad), mode="constant")
    n_frames = 1 + (yp.size - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    return yp[idx] * window_function(window, n_fft)[None, :]


def _normalized(x):
    """(x - mean) / unbiased std over the whole utterance (data_loader.py:87-88)."""
    mean = x.mean()
    std = x.std(ddof=1)
    return (x - mean) / std


def log_spectrogram(y, sample_rate=16000, window_size=0.02, window_stride=0.01, normalize=True, window="hamming"):
    """float waveform -> (n_fft/2+1, frames) log1p(|STFT|), optionally (x-mean)/std over the whole utterance with the
    unbiased std torch uses (data_loader.py:72-89).  STFT convention: n_fft = win_length = sr*window_size (320),
    hop = sr*window_stride (160), centred frames with reflect padding (librosa's default of that era)."""
    n_fft = int(sample_rate * window_size)
    hop = int(sample_rate * window_stride)
    frames = _windowed_frames(y, n_fft, hop, window)
    spec = np.abs(np.fft.rfft(frames, n=n_fft, axis=1)).T.astype(np.float32)        # (bins, frames)
    spec = np.log1p(spec)
    if normalize:
        spec = _normalized(spec)
    return spec


# ------------------------------------------------------------------------------------------------ log-mel filterbank features
FEATURES = ("spect", "fbank")
FBANK_FLOOR = 1e-10
# first[m], count[m]: the bins filter m weighs; weights: every filter's count[m] float32 weights one after the other; n_bins = K
MelBank = collections.namedtuple("MelBank", "first count weights n_bins")


def mel_filterbank(M=80, n_fft=320, sample_rate=16000, f_min=20.0, f_max=None):
    """The sparse bank of M triangular filters on the K = n_fft/2 + 1 bins f_k = k sr / n_fft: M + 2 points
    equally spaced on the HTK mel scale 2595 log10(1 + f/700) between f_min and f_max (default sr/2), mapped back to Hz as c_0 ..
    c_{M+1}; w[m][k] = max(0, min((f_k - c_m) / (c_{m+1} - c_m), (c_{m+2} - f_k) / (c_{m+2} - c_{m+1}))), no area normalisation,
    computed in float64 and stored as float32.  Refuses a bank with a filter that weighs no bin (its feature row would be the
    constant log floor)."""
    M, n_fft = int(M), int(n_fft)
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    if M < 1 or not 0 <= f_min < f_max <= sample_rate / 2.0:
        raise ValueError("--num-mel-bins %d, --mel-fmin %g: need at least one filter and 0 <= f_min < f_max = %g <= sample rate / 2"
                         % (M, f_min, f_max))
    K = n_fft // 2 + 1
    f = np.arange(K, dtype=np.float64) * sample_rate / n_fft
    mel = np.linspace(2595.0 * np.log10(1.0 + f_min / 700.0), 2595.0 * np.log10(1.0 + f_max / 700.0), M + 2)
    c = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    c[0], c[-1] = f_min, f_max                # the end points map back exactly: no rounding residue as a weight on the bin at f_max
    up = (f[None, :] - c[:M, None]) / (c[1:M + 1] - c[:M])[:, None]
    down = (c[2:, None] - f[None, :]) / (c[2:] - c[1:M + 1])[:, None]
    w = np.maximum(0.0, np.minimum(up, down)).astype(np.float32)                   # (M, K)
    first, count, weights, empty = [], [], [], []
    for m in range(M):
        nz = np.nonzero(w[m])[0]
        if nz.size == 0:
            empty.append(m)
            continue
        first.append(int(nz[0]))
        count.append(int(nz[-1] - nz[0] + 1))
        weights.append(w[m, nz[0]:nz[-1] + 1])
    if empty:
        raise ValueError("--num-mel-bins %d with --mel-fmin %g on the %d bins of a %d-point STFT at --sample-rate %d: filter(s) %s lie "
                         "between two bins and weigh none -- use fewer mel bins, a higher --mel-fmin or a longer --window-size"
                         % (M, f_min, K, n_fft, sample_rate, empty))
    return MelBank(np.array(first, dtype=np.int32), np.array(count, dtype=np.int32), np.concatenate(weights).astype(np.float32), K)


_mel_banks = {}


def _mel_bank_cached(M, n_fft, sample_rate, f_min):
    key = (int(M), int(n_fft), int(sample_rate), float(f_min))
    bank = _mel_banks.get(key)
    if bank is None:
        bank = _mel_banks[key] = mel_filterbank(*key)
    return bank


def log_mel_fbank(y, sample_rate=16000, window_size=0.02, window_stride=0.01, normalize=True, window="hamming", num_mel_bins=80,
                  f_min=20.0):
    """float waveform -> (num_mel_bins, frames) log(max(mel energies of the power spectrum, 1e-10)) of log_spectrogram's STFT (the
    same framing), optionally normalised over the whole utterance as log_spectrogram does.  The host path of --features fbank."""
    n_fft = int(sample_rate * window_size)
    hop = int(sample_rate * window_stride)
    bank = _mel_bank_cached(num_mel_bins, n_fft, sample_rate, f_min)
    z = np.fft.rfft(_windowed_frames(y, n_fft, hop, window).astype(np.float64), n=n_fft, axis=1)
    power = z.real ** 2 + z.imag ** 2                                               # (frames, bins)
    x = np.empty((bank.first.size, power.shape[0]), dtype=np.float64)
    o = 0
    for m, (k0, n) in enumerate(zip(bank.first, bank.count)):
        x[m] = power[:, k0:k0 + n] @ bank.weights[o:o + n].astype(np.float64)
        o += n
    x = np.log(np.maximum(x, FBANK_FLOOR)).astype(np.float32)
    return _normalized(x) if normalize else x


def feature_settings(args):
    """(features, num_mel_bins, mel_fmin) of a Namespace; one written before --features existed is `spect`."""
    return (getattr(args, "features", "spect"), int(getattr(args, "num_mel_bins", 80)), float(getattr(args, "mel_fmin", 20.0)))


def feature_bins(args):
    """Rows of the features the model sees: n_fft/2 + 1 (161) for --features spect, --num-mel-bins for fbank."""
    features, M, _ = feature_settings(args)
    if features == "fbank":
        return M
    if features != "spect":
        raise ValueError("--features %r: one of %s" % (features, FEATURES))
    return int(np.floor((args.sample_rate * args.window_size) / 2) + 1)


# ------------------------------------------------------------------------------------------------ tempo / gain / noise
def wsola_constants(sample_rate):
    """(S, search, O) of sox's `tempo` effect at its defaults (segment 82 ms, search 82/5.587 ms, overlap 82/6.833 ms rounded down to
    a multiple of 8 samples): (1312, 235, 192) at 16 kHz."""
    S = int(np.floor(sample_rate * 82 / 1000 + .5))
    search = int(np.floor(sample_rate * (82 / 5.587) / 1000 + .5))
    O = int(np.floor(max(sample_rate * (82 / 6.833) / 1000 + 4.5, 16)))
    return S, search, O - O % 8


def tempo_length(n, tempo):
    """Samples after the tempo change: floor(n / tempo + .5)."""
    return int(np.floor(n / float(tempo) + .5))


def gain_multiplier(gain_db):
    """m = float32(10^(gain/20))."""
    return np.float32(10.0 ** (float(gain_db) / 20.0))


# ------------------------------------------------------------------------------------------------ speed perturbation
SPEED_RANGE = (500, 2000)                     # speed factors in thousandths: 0.5 .. 2.0
RESAMPLE_ZEROS, RESAMPLE_ROLLOFF = 6, (99, 100)      # Z zero crossings of the sinc, roll-off rho = 0.99 as a fraction


def speed_thousandths(factors):
    """--speed-perturb's factors as integers in thousandths (each rounded to the nearest); refuses an empty list and a factor outside
    [0.5, 2.0]."""
    out = [int(np.floor(float(f) * 1000.0 + .5)) for f in factors]
    if not out or min(out) < SPEED_RANGE[0] or max(out) > SPEED_RANGE[1]:
        raise ValueError("--speed-perturb %s: one or more factors, each in [0.5, 2.0]" % list(factors))
    return out


def speed_ratio(p):
    """p / 1000 in lowest terms (num, den): den divides 1000."""
    p = int(p)
    if not SPEED_RANGE[0] <= p <= SPEED_RANGE[1]:
        raise ValueError("speed factor %d / 1000 outside [0.5, 2.0]" % p)
    g = int(np.gcd(p, 1000))
    return p // g, 1000 // g


def speed_length(n, p):
    """Samples of an utterance of n after the speed change by p / 1000: n den / num rounded half up (n itself at 1000)."""
    num, den = speed_ratio(p)
    return (2 * int(n) * den + num) // (2 * num)


_resample_tables = {}


def resample_table(p):
    """(R, H (den, 2R) float32) of the speed factor p / 1000 = num / den: the Hann-windowed sinc
    h(t) = c sinc(c t) cos^2(pi c t / (2 Z)) for |c t| < Z, else 0, with Z = 6, c = 0.99 min(1, den / num), R = ceil(Z / c), sampled as
    H[phi][q] = h(phi / den - (q - R + 1)).  Computed in float64, not normalised per phase, cached per factor."""
    p = int(p)
    hit = _resample_tables.get(p)
    if hit is None:
        num, den = speed_ratio(p)
        rn, rd = RESAMPLE_ROLLOFF
        Z, wide = RESAMPLE_ZEROS, max(num, den)
        R = -((-Z * rd * wide) // (rn * den))                                     # ceil(Z / c) in integers
        c = (rn / rd) * min(1.0, den / num)
        # t = (phi - (q - R + 1) den) / den: an integer numerator, so that mirrored taps are the same float64
        t = (np.arange(den, dtype=np.int64)[:, None] - (np.arange(2 * R, dtype=np.int64)[None, :] - R + 1) * den) / float(den)
        h = c * np.sinc(c * t) * np.cos(np.pi * c * t / (2.0 * Z)) ** 2
        h[np.abs(c * t) >= Z] = 0.0
        H = h.astype(np.float32)
        H.setflags(write=False)
        hit = _resample_tables[p] = (int(R), H)
    return hit


_device_resample_tables = {}


def device_resample_tables(factors, device):
    """The tap tables of the distinct non-identity factors (thousandths) concatenated on the device, uploaded once per (factor set,
    device) like the mel bank: (table fp32, {p: (R, offset in floats)})."""
    import torch
    key = (tuple(sorted(set(int(p) for p in factors))), str(device))
    hit = _device_resample_tables.get(key)
    if hit is None:
        index, parts, off = {}, [], 0
        for p in key[0]:
            R, H = resample_table(p)
            index[p] = (R, off)
            parts.append(H.reshape(-1))
            off += H.size
        hit = _device_resample_tables[key] = (torch.from_numpy(np.concatenate(parts)).to(device), index)
    return hit


def _wav_files(directory, sample_rate, flag, what):
    """Every *.wav under `directory` (recursive, sorted) and their lengths in samples, under the rules --noise-dir and --rir-dir share:
    refuses a missing or empty directory, audio of another format, and a sample rate other than --sample-rate."""
    if not os.path.isdir(directory):
        raise ValueError("%s %s is not a directory" % (flag, directory))
    paths, other = [], []
    for p in glob.glob(os.path.join(directory, "**", "*"), recursive=True):
        ext = os.path.splitext(p)[1].lower()
        if os.path.isfile(p) and ext in AUDIO_EXTENSIONS:
            (paths if ext == ".wav" else other).append(p)
    if other:
        raise ValueError("%s %s holds non-wav audio (%s): only .wav %ss are supported" % (flag, directory, sorted(other)[0], what))
    if not paths:
        raise ValueError("%s %s holds no .wav files" % (flag, directory))
    paths.sort()
    lens = []
    for p in paths:
        with wave.open(p, "rb") as f:
            if f.getframerate() != sample_rate:
                raise ValueError("%s %s has sample rate %d, not --sample-rate %d (%ss are not resampled)"
                                 % (what, p, f.getframerate(), sample_rate, what))
            lens.append(f.getnframes())
    return paths, lens


def noise_files(noise_dir, sample_rate):
    """Every *.wav under noise_dir (recursive, sorted: the population the noise draw picks from) and their lengths in samples.
    Refuses, at start-up: a missing or empty directory, audio of another format (the reference would pick it up too, so skipping it
    would change the draws) and a sample rate other than --sample-rate (noise clips are not resampled)."""
    return _wav_files(noise_dir, sample_rate, "--noise-dir", "noise clip")


def load_pcm16(path):
    """A wav as int16 samples (mono): 16-bit mono files as stored, anything else through load_audio rounded to 16 bits."""
    with wave.open(path, "rb") as f:
        if f.getsampwidth() == 2 and f.getnchannels() == 1:
            return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int16)
    return np.clip(np.rint(load_audio(path).astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


class NoiseBank:
    """All clips of a noise directory concatenated as int16 on the device, with per-clip offsets and lengths (int64)."""

    def __init__(self, noise_dir, sample_rate, device):
        import torch
        self.paths, lens = noise_files(noise_dir, sample_rate)
        clips = [load_pcm16(p) for p in self.paths]
        self.lengths = np.array([c.size for c in clips], dtype=np.int64)
        if (self.lengths > 0x7fffffff).any():
            raise ValueError("noise clips longer than 2^31 samples are not supported")
        offs = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        data = np.concatenate(clips + [np.zeros(1, np.int16)])
        self.data = torch.from_numpy(data).to(device)
        self.offsets = torch.from_numpy(offs).to(device)
        self.lens = torch.from_numpy(self.lengths).to(device)


_noise_banks = {}


def noise_bank(noise_dir, sample_rate, device):
    """The NoiseBank of (noise_dir, sample_rate, device), built once per process (the main process: loader workers only draw)."""
    key = (os.path.abspath(noise_dir), int(sample_rate), str(device))
    bank = _noise_banks.get(key)
    if bank is None:
        bank = _noise_banks[key] = NoiseBank(noise_dir, sample_rate, device)
    return bank


# ------------------------------------------------------------------------------------------------ reverberation
RIR_TAIL = 1e-3                               # taps behind the last one at or above -60 dB of the direct path are dropped


def rir_files(rir_dir, sample_rate):
    """Every *.wav under rir_dir (recursive, sorted: the population the RIR draw indexes) and their lengths in samples, under
    noise_files' rules: refuses a missing or empty directory, non-wav audio and a sample rate other than --sample-rate."""
    return _wav_files(rir_dir, sample_rate, "--rir-dir", "room impulse response")


def prepare_rir(h, sample_rate, max_ms):
    """The taps of one recorded room impulse response h, in float64 until the last step: the samples before
    the direct path (the FIRST index of max |h|) are dropped, so that it sits at lag 0 and the transcript stays aligned; at most
    floor(max_ms sample_rate / 1000) >= 1 taps are kept; the tail behind the last tap with |h[k]| >= 1e-3 |h[k0]| is dropped; the
    rest is divided by sqrt(sum h^2) and cast to float32.  Refuses an empty or all-zero response."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    cap = int(np.floor(float(max_ms) * int(sample_rate) / 1000.0))
    if cap < 1:
        raise ValueError("--rir-max-ms %s keeps no tap at %d Hz" % (max_ms, sample_rate))
    if h.size == 0 or not np.any(h):
        raise ValueError("an empty or all-zero room impulse response")
    mag = np.abs(h)
    k0 = int(np.argmax(mag))
    h, mag = h[k0:k0 + cap], mag[k0:k0 + cap]
    h = h[:int(np.nonzero(mag >= RIR_TAIL * mag[0])[0][-1]) + 1]
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32)


_prepared_rirs = {}


def prepared_rirs(rir_dir, sample_rate, max_ms):
    """(paths, [taps]) of every response under rir_dir, prepared once per (directory, sample rate, max_ms) on the host.  The training
    dataset calls it at start-up, so that a directory or a file that is refused is refused before the first batch."""
    key = (os.path.abspath(rir_dir), int(sample_rate), float(max_ms))
    hit = _prepared_rirs.get(key)
    if hit is None:
        paths, _ = rir_files(rir_dir, sample_rate)
        taps = []
        for p in paths:
            try:
                taps.append(prepare_rir(load_audio(p), sample_rate, max_ms))
            except ValueError as e:
                raise ValueError("--rir-dir: %s: %s" % (p, e))
        hit = _prepared_rirs[key] = (paths, taps)
    return hit


class RirBank:
    """The prepared taps of all room impulse responses concatenated as fp32 on the device, with per-response offsets and lengths
    (int64), as asr_reverb reads them; len() = the number of responses."""

    def __init__(self, rir_dir, sample_rate, max_ms, device):
        self.paths, taps = prepared_rirs(rir_dir, sample_rate, max_ms)
        self._upload(taps, device)

    @classmethod
    def from_arrays(cls, taps, device):
        """A bank of the given float32 tap arrays as they are, without prepare_rir (tests inject exact taps)."""
        self = cls.__new__(cls)
        self.paths = None
        self._upload([np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in taps], device)
        return self

    def _upload(self, taps, device):
        import torch
        if not taps or any(t.size < 1 for t in taps):
            raise ValueError("a RIR bank needs at least one response and every response at least one tap")
        self.lengths = np.array([t.size for t in taps], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.data = torch.from_numpy(np.concatenate(taps)).to(device)
        self.offsets = torch.from_numpy(offs).to(device)
        self.lens = torch.from_numpy(self.lengths).to(device)

    def __len__(self):
        return int(self.lengths.size)


_rir_banks = {}


def rir_bank(rir_dir, sample_rate, max_ms, device):
    """The RirBank of (rir_dir, sample_rate, max_ms, device), built once per process like noise_bank."""
    key = (os.path.abspath(rir_dir), int(sample_rate), float(max_ms), str(device))
    bank = _rir_banks.get(key)
    if bank is None:
        bank = _rir_banks[key] = RirBank(rir_dir, sample_rate, max_ms, device)
    return bank


def spec_frames(samples, hop, src_max_len=None):
    """Frames the front end keeps of an utterance of `samples` samples: min(1 + max(samples, 2) // hop, --src-max-len).  The one
    statement of the frame count on the Python side (the kernels' is spect_frames, csrc/spec_augment.h); `samples` is a number, or an
    integer tensor of them, for which a tensor comes back."""
    if hasattr(samples, "clamp"):
        n = 1 + samples.clamp(min=2) // int(hop)
        return n if src_max_len is None else n.clamp(max=int(src_max_len))
    n = 1 + max(int(samples), 2) // int(hop)
    return n if src_max_len is None else min(n, int(src_max_len))


_device_mel_banks = {}


def _device_mel_bank(M, n_fft, sample_rate, f_min, device):
    """The filter bank on the device, uploaded once per (M, n_fft, sample rate, f_min, device), like the STFT constants."""
    from asr_hip import ops
    key = (int(M), int(n_fft), int(sample_rate), float(f_min), str(device))
    bank = _device_mel_banks.get(key)
    if bank is None:
        bank = _device_mel_banks[key] = ops.fbank_upload(_mel_bank_cached(*key[:4]), device)
    return bank


def gpu_front_end(inputs, input_sizes, sample_rate=16000, window_size=0.02, window_stride=0.01, src_max_len=None, window="hamming",
                  aug=None, noise_dir=None, spec=None, features="spect", num_mel_bins=80, mel_fmin=20.0, rir_dir=None, rir_max_ms=500):
    """--gpu-frontend: `inputs` (B,1,1,Lmax) are the loader's zero padded WAVEFORMS and `input_sizes` (B) their sample
    counts (the collate function is unchanged: a waveform is a 1-bin "spectrogram").  Returns what the host path would have
    put in the batch: log-spectrograms (B,1,F,T) normalised per utterance, cut to --src-max-len frames AFTER the
    normalisation (data_loader.py:49-53), and the frame counts.
    aug: the loader's (B, 6) float64 draws {input samples, tempo (0: none), gain dB, noise clip (-1: none), noise start s, level}
    (utils/data_loader.py); they are applied on the device first (ops.augment_wave) and `input_sizes` are then the samples after
    the tempo change.  noise_dir: the directory the clip indices refer to.  With --speed-perturb the draws are (B, 7), the seventh
    column the speed factor in thousandths (0 or 1000: none): the batch is resampled first (ops.resample), tempo / gain / noise then
    work on the resampled waveforms, and `input_sizes` count the samples after both.  With --rir-dir the draws are (B, 8): column 6
    is the speed factor (0 without --speed-perturb), column 7 the index of the room impulse response among rir_files(rir_dir) (-1:
    none).  The order is speed, then reverberation (ops.reverb: the length does not change), then tempo / gain / noise -- noise is
    added to the reverberant speech and is not itself reverberated.
    spec: the loader's (B, 40) int32 SpecAugment rows; their n must be the kept frame counts of this batch.
    Normalisation, cut and SpecAugment are then one launch (asr_spect_finish_aug).
    features="fbank": (B,1,num_mel_bins,T) log-mel filterbank features instead (log_mel_fbank's; asr_fbank_finish[_aug])."""
    import torch
    from asr_hip import ops
    n_fft, hop = int(sample_rate * window_size), int(sample_rate * window_stride)
    if features not in FEATURES:
        raise ValueError("features %r: one of %s" % (features, FEATURES))
    kind = {}
    if features == "fbank":
        kind = dict(features="fbank", mel=_device_mel_bank(num_mel_bins, n_fft, sample_rate, mel_fmin, inputs.device))
    wav = inputs.reshape(inputs.shape[0], inputs.shape[-1]).float().contiguous()
    if aug is not None:
        aug = torch.as_tensor(aug, dtype=torch.float64)
        rir = aug[:, 7].long() if aug.shape[1] == 8 else None
        if aug.shape[1] >= 7:
            # speed perturbation first: the resampled batch and its lengths then take the place of the loader's
            speed = aug[:, 6].long()
            wav, _ = ops.resample(wav, aug[:, 0].long(), speed)
            aug = aug[:, :6].clone()
            aug[:, 0] = aug.new_tensor([speed_length(n, p) if p else n for n, p in zip(aug[:, 0].long().tolist(), speed.tolist())])
        if rir is not None and (rir >= 0).any():
            # then the room: the taps' direct path sits at lag 0 and the length stays, so the sizes and the transcript's alignment do too
            if rir_dir is None:
                raise ValueError("the draws name room impulse responses but no rir_dir is given")
            wav = ops.reverb(wav, aug[:, 0].long(), rir, rir_bank(rir_dir, sample_rate, rir_max_ms, wav.device))
        bank = noise_bank(noise_dir, sample_rate, wav.device) if (aug[:, 3] >= 0).any() else None
        wav, lens = ops.augment_wave(wav, aug[:, 0].long(), aug[:, 1:], bank, sample_rate=sample_rate)
        if not torch.equal(torch.as_tensor(input_sizes).long(), aug[:, 0].new_tensor(
                [tempo_length(n, t) if t > 0 else n for n, t in aug[:, :2].tolist()]).long()):
            raise ValueError("input_sizes are not the post-tempo sample counts of the draws")
    else:
        lens = torch.as_tensor(input_sizes).to(device=wav.device, dtype=torch.int32)
    if spec is not None:
        spec = torch.as_tensor(spec)
        kept = [spec_frames(s, hop, src_max_len) for s in torch.as_tensor(input_sizes).tolist()]
        if spec.dim() != 2 or spec[:, 0].tolist() != kept:
            raise ValueError("the SpecAugment rows' frame counts are not the kept frames of input_sizes")
        spect, n_frames = ops.log_spectrogram(wav, lens, n_fft=n_fft, hop=hop, normalize=True, window=window, spec=spec,
                                              max_frames=src_max_len, **kind)
        return spect, n_frames.cpu()
    spect, n_frames = ops.log_spectrogram(wav, lens, n_fft=n_fft, hop=hop, normalize=True, window=window, **kind)
    if src_max_len is not None and spect.shape[-1] > src_max_len:
        spect = spect[..., :src_max_len].contiguous()
        n_frames = torch.clamp(n_frames, max=src_max_len)
    return spect, n_frames.cpu()
