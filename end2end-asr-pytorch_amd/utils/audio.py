"""Waveform loading and the spectrogram front end (reference: utils/audio.py:7-15 and SpectrogramParser.parse_audio,
utils/data_loader.py:60-91).  Own implementation on numpy only: the reference's torchaudio / librosa / sox dependencies
are not part of this build.  The reference's sox-based tempo/gain augmentation and noise injection (audio.py:17-61,
data_loader.py:145-179) run on the GPU instead (asr_augment_wave, csrc/augment.hip; definition in DESIGN.md section 7): the host
keeps the random draws (utils/data_loader.py), gpu_front_end applies them to the batch before the STFT.
"""
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


def log_spectrogram(y, sample_rate=16000, window_size=0.02, window_stride=0.01, normalize=True, window="hamming"):
    """float waveform -> (n_fft/2+1, frames) log1p(|STFT|), optionally (x-mean)/std over the whole utterance with the
    unbiased std torch uses (data_loader.py:72-89).  STFT convention: n_fft = win_length = sr*window_size (320),
    hop = sr*window_stride (160), centred frames with reflect padding (librosa's default of that era)."""
    n_fft = int(sample_rate * window_size)
    hop = int(sample_rate * window_stride)
    y = np.asarray(y, dtype=np.float32)
    if y.size < 2:
        y = np.pad(y, (0, 2 - y.size))
    pad = n_fft // 2
    yp = np.pad(y, (pad, pad), mode="reflect") if y.size > pad else np.pad(y, (pad, pad), mode="constant")
    n_frames = 1 + (yp.size - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    frames = yp[idx] * window_function(window, n_fft)[None, :]
    spec = np.abs(np.fft.rfft(frames, n=n_fft, axis=1)).T.astype(np.float32)        # (bins, frames)
    spec = np.log1p(spec)
    if normalize:
        mean = spec.mean()
        std = spec.std(ddof=1)
        spec = (spec - mean) / std
    return spec


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


def noise_files(noise_dir, sample_rate):
    """Every *.wav under noise_dir (recursive, sorted: the population the noise draw picks from) and their lengths in samples.
    Refuses, at start-up: a missing or empty directory, audio of another format (the reference would pick it up too, so skipping it
    would change the draws) and a sample rate other than --sample-rate (noise clips are not resampled)."""
    if not os.path.isdir(noise_dir):
        raise ValueError("--noise-dir %s is not a directory" % noise_dir)
    paths, other = [], []
    for p in glob.glob(os.path.join(noise_dir, "**", "*"), recursive=True):
        ext = os.path.splitext(p)[1].lower()
        if os.path.isfile(p) and ext in AUDIO_EXTENSIONS:
            (paths if ext == ".wav" else other).append(p)
    if other:
        raise ValueError("--noise-dir %s holds non-wav audio (%s): only .wav noise clips are supported" % (noise_dir, sorted(other)[0]))
    if not paths:
        raise ValueError("--noise-dir %s holds no .wav files" % noise_dir)
    paths.sort()
    lens = []
    for p in paths:
        with wave.open(p, "rb") as f:
            if f.getframerate() != sample_rate:
                raise ValueError("noise clip %s has sample rate %d, not --sample-rate %d (noise clips are not resampled)"
                                 % (p, f.getframerate(), sample_rate))
            lens.append(f.getnframes())
    return paths, lens


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


def spec_frames(samples, hop, src_max_len=None):
    """Frames the front end keeps of an utterance of `samples` samples: min(1 + max(samples, 2) // hop, --src-max-len)."""
    n = 1 + max(int(samples), 2) // int(hop)
    return n if src_max_len is None else min(n, int(src_max_len))


def gpu_front_end(inputs, input_sizes, sample_rate=16000, window_size=0.02, window_stride=0.01, src_max_len=None, window="hamming",
                  aug=None, noise_dir=None, spec=None):
    """--gpu-frontend: `inputs` (B,1,1,Lmax) are the loader's zero padded WAVEFORMS and `input_sizes` (B) their sample
    counts (the collate function is unchanged: a waveform is a 1-bin "spectrogram").  Returns what the host path would have
    put in the batch: log-spectrograms (B,1,F,T) normalised per utterance, cut to --src-max-len frames AFTER the
    normalisation (data_loader.py:49-53), and the frame counts.
    aug: the loader's (B, 6) float64 draws {input samples, tempo (0: none), gain dB, noise clip (-1: none), noise start s, level}
    (utils/data_loader.py); they are applied on the device first (ops.augment_wave) and `input_sizes` are then the samples after
    the tempo change.  noise_dir: the directory the clip indices refer to.
    spec: the loader's (B, 40) int32 SpecAugment rows; their n must be the kept frame counts of this batch.
    Normalisation, cut and SpecAugment are then one launch (asr_spect_finish_aug)."""
    import torch
    from asr_hip import ops
    n_fft, hop = int(sample_rate * window_size), int(sample_rate * window_stride)
    wav = inputs.reshape(inputs.shape[0], inputs.shape[-1]).float().contiguous()
    if aug is not None:
        aug = torch.as_tensor(aug, dtype=torch.float64)
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
                                              max_frames=src_max_len)
        return spect, n_frames.cpu()
    spect, n_frames = ops.log_spectrogram(wav, lens, n_fft=n_fft, hop=hop, normalize=True, window=window)
    if src_max_len is not None and spect.shape[-1] > src_max_len:
        spect = spect[..., :src_max_len].contiguous()
        n_frames = torch.clamp(n_frames, max=src_max_len)
    return spect, n_frames.cpu()
