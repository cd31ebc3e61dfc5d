"""Manifest / label-file loader contract of the reference (reference: utils/data_loader.py):
  * manifest: one "wav_path,transcript_path" per line (data_loader.py:112-119);
  * transcripts: SOS + lower-cased text + EOS mapped through label2id, unknown characters AND id 0 dropped (:133-141);
  * batch = (inputs f32 (B,1,F,Tmax) zero padded and sorted by length descending, targets i64 (B,Lmax) zero padded,
             input_percentages f32 (B), input_sizes i32 (B), target_sizes i32 (B))   (:182-214);
  * with tempo / gain augmentation or noise injection (GPU front end only) a 6th element: the (B, 6) float64 draws
    {input samples, tempo (0: none), gain dB, noise clip (-1: none), noise start s, noise level}, and the batch is sorted by, and
    input_sizes / input_percentages count, the samples AFTER the tempo change (utils.audio.gpu_front_end applies the draws);
  * with SpecAugment (training dataset, GPU front end only) a 7th element: the (B, 40) int32 rows {n, c, w, nF, nT, 0, 0, 0,
    8 x (f0, fw), 8 x (t0, tw)} of DESIGN.md section 7; the 6th element is then the wave draws or None;
  * with speed perturbation (audio_conf['speed_perturb'], training dataset, GPU front end only) the draws are (B, 7): the seventh
    column is the speed factor in thousandths, and the sizes count the samples after the speed AND the tempo change;
  * with reverberation (audio_conf['rir_dir'], training dataset, GPU front end only) the draws are (B, 8): column 6 is the speed factor
    (0 without speed perturbation), column 7 the index of the utterance's room impulse response (-1: none).
BucketingSampler keeps the reference's consecutive bins and additionally shards them over data-parallel ranks.
"""
import random

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.sampler import Sampler

from asr_hip.ddp import rank_shard
from utils import constant
from utils.audio import (FEATURES, load_audio, log_mel_fbank, log_spectrogram, mel_filterbank, noise_files, resolve_window, spec_frames,
                         prepared_rirs, speed_length, speed_thousandths, tempo_length)

TEMPO_RANGE, GAIN_RANGE = (0.85, 1.15), (-6, 8)          # reference: utils/audio.py:54
SPEC_PARAMS, SPEC_MAX_MASKS = 40, 8                      # one SpecAugment row (include/asr_hip.h, ASR_SPEC_AUGMENT_PARAMS)
SPEC_POLICY_KEYS = ("time_warp", "freq_mask", "freq_masks", "time_mask", "time_masks", "time_mask_ratio")


def spec_policy(args):
    """The SpecAugment policy of a command line (--spec-augment and its --spec-* parameters) as the dict SpectrogramDataset takes,
    or None with the flag off."""
    if not getattr(args, "spec_augment", False):
        return None
    return {k: getattr(args, "spec_" + k) for k in SPEC_POLICY_KEYS}


class SpectrogramParser(object):
    def __init__(self, audio_conf, normalize=False, augment=False, spec_augment=None):
        self.window_stride = audio_conf['window_stride']
        self.window_size = audio_conf['window_size']
        self.sample_rate = audio_conf['sample_rate']
        self.window = resolve_window(audio_conf.get('window', 'hamming'))
        self.normalize = normalize
        self.augment = augment
        # feature type (audio_conf of a run from before --features: spect); the filter bank is built here once, so that a bank with an
        # empty filter is refused at start-up
        self.features = audio_conf.get('features', 'spect')
        self.num_mel_bins, self.mel_fmin = int(audio_conf.get('num_mel_bins', 80)), float(audio_conf.get('mel_fmin', 20.0))
        if self.features not in FEATURES:
            raise ValueError("--features %r: one of %s" % (self.features, FEATURES))
        n_fft = int(self.sample_rate * self.window_size)
        if self.features == "fbank":
            mel_filterbank(self.num_mel_bins, n_fft, self.sample_rate, self.mel_fmin)
        self.feature_bins = self.num_mel_bins if self.features == "fbank" else n_fft // 2 + 1
        self.noise_dir = audio_conf.get('noise_dir')
        # speed perturbation: the factors in thousandths one is drawn from per utterance, or None
        self.speed = speed_thousandths(audio_conf['speed_perturb']) if audio_conf.get('speed_perturb') else None
        if (augment or self.noise_dir is not None) and not getattr(constant.args, "gpu_frontend", False):
            raise NotImplementedError("tempo/gain augmentation (--augment) and noise injection (--noise-dir) run on the GPU front end "
                                      "only: use --cuda (it turns on --gpu-frontend)")
        if self.speed is not None and not getattr(constant.args, "gpu_frontend", False):
            raise NotImplementedError("speed perturbation (--speed-perturb) runs on the GPU front end only: use --cuda (it turns on "
                                      "--gpu-frontend)")
        # reverberation: the number of room impulse responses an index is drawn from with probability rir_prob, or None
        self.rir_dir, self.rir_count = audio_conf.get('rir_dir'), None
        if self.rir_dir is not None:
            if not getattr(constant.args, "gpu_frontend", False):
                raise NotImplementedError("reverberation (--rir-dir) runs on the GPU front end only: use --cuda (it turns on "
                                          "--gpu-frontend)")
            self.rir_prob, self.rir_max_ms = float(audio_conf.get('rir_prob', 0.5)), float(audio_conf.get('rir_max_ms', 500))
            if not 0.0 <= self.rir_prob <= 1.0 or not self.rir_max_ms > 0:
                raise ValueError("--rir-prob %g must lie in [0, 1] and --rir-max-ms %g above 0" % (self.rir_prob, self.rir_max_ms))
            self.rir_count = len(prepared_rirs(self.rir_dir, self.sample_rate, self.rir_max_ms)[0])
        self.spec = None
        if spec_augment is not None:
            if not getattr(constant.args, "gpu_frontend", False):
                raise NotImplementedError("SpecAugment (--spec-augment) runs on the GPU front end only: use --cuda (it turns on "
                                          "--gpu-frontend)")
            pol = {k: spec_augment[k] for k in SPEC_POLICY_KEYS}
            if pol["freq_masks"] > SPEC_MAX_MASKS or pol["time_masks"] > SPEC_MAX_MASKS:
                raise ValueError("--spec-freq-masks / --spec-time-masks: at most %d masks per axis" % SPEC_MAX_MASKS)
            if min(pol.values()) < 0 or pol["time_mask_ratio"] > 1:
                raise ValueError("--spec-* parameters must not be negative, --spec-time-mask-ratio at most 1: %s" % pol)
            self.spec = pol
        self.noise_paths = None
        if self.noise_dir is not None:
            self.noise_paths, self.noise_lens = noise_files(self.noise_dir, self.sample_rate)
            self.noise_index = {p: i for i, p in enumerate(self.noise_paths)}
            self.noise_prob = float(audio_conf.get('noise_prob'))          # an untyped flag in the reference's CLI
            self.noise_levels = tuple(audio_conf.get('noise_levels', (0.0, 0.5)))

    def draw(self, n):
        """The random draws for an utterance of n samples, on the global np.random in the reference's call order
        (utils/audio.py:49-61, data_loader.py:62-70,160-170): (n, tempo, gain dB, noise clip, noise start s, level, n_out) with
        tempo 0 = no tempo / gain, clip -1 = no noise; tempo and gain rounded through "%.3f" as sox's command line.
        With speed perturbation ONE more draw comes first, the index of the factor, and the tuple gains an 8th element, the factor p
        in thousandths; n_out then counts the samples after the speed and the tempo change.
        With reverberation the draws above come first and unchanged, then np.random.binomial(1, rir_prob) and, on a hit,
        np.random.randint(number of RIRs); the tuple then has 9 elements: the first seven as above, p (0 without speed perturbation)
        and the index of the room impulse response (-1: none).  The length does not change."""
        tempo = gain = 0.0
        n_out = n
        if self.speed is not None:
            p = self.speed[np.random.randint(len(self.speed))]
            n_out = speed_length(n, p)
        if self.augment:
            tempo = float("%.3f" % np.random.uniform(low=TEMPO_RANGE[0], high=TEMPO_RANGE[1]))
            gain = float("%.3f" % np.random.uniform(low=GAIN_RANGE[0], high=GAIN_RANGE[1]))
            n_out = tempo_length(n_out, tempo)
        clip, start_s, level = -1, 0.0, 0.0
        if self.noise_paths is not None and np.random.binomial(1, self.noise_prob):
            clip = self.noise_index[np.random.choice(self.noise_paths)]
            level = float(np.random.uniform(*self.noise_levels))
            data_len = n_out / self.sample_rate
            start_s = float(np.random.rand() * (self.noise_lens[clip] / self.sample_rate - data_len))
        if self.rir_count is not None:
            rir = int(np.random.randint(self.rir_count)) if np.random.binomial(1, self.rir_prob) else -1
            return (n, tempo, gain, clip, start_s, level, n_out, p if self.speed is not None else 0, rir)
        if self.speed is not None:
            return (n, tempo, gain, clip, start_s, level, n_out, p)
        return (n, tempo, gain, clip, start_s, level, n_out)

    def draw_spec(self, samples):
        """The SpecAugment row of an utterance of `samples` samples (after the tempo change), on the global np.random after the
        utterance's wave draws: warp centre and target, then (width, start) per frequency mask, then per time mask."""
        hop = int(self.sample_rate * self.window_stride)
        n, F, p = spec_frames(samples, hop, constant.args.src_max_len), self.feature_bins, self.spec
        row = [0] * SPEC_PARAMS
        row[0], row[3], row[4] = n, p["freq_masks"], p["time_masks"]
        W = p["time_warp"]
        if n > 2 * W:
            row[1] = int(np.random.randint(W, n - W))
            row[2] = row[1] + int(np.random.randint(-W, W + 1))
        for k in range(p["freq_masks"]):
            fw = int(np.random.randint(0, min(p["freq_mask"], F) + 1))
            row[8 + 2 * k], row[9 + 2 * k] = int(np.random.randint(0, F - fw + 1)), fw
        t_cap = min(p["time_mask"], int(np.floor(p["time_mask_ratio"] * n)))
        for k in range(p["time_masks"]):
            tw = int(np.random.randint(0, t_cap + 1))
            row[8 + 2 * SPEC_MAX_MASKS + 2 * k], row[9 + 2 * SPEC_MAX_MASKS + 2 * k] = int(np.random.randint(0, n - tw + 1)), tw
        return row

    @property
    def augmenting(self):
        return self.augment or self.noise_paths is not None or self.speed is not None or self.rir_count is not None

    def parse_audio(self, audio_path):
        y = load_audio(audio_path)
        if getattr(constant.args, "gpu_frontend", False):
            # ship the waveform as a 1-bin "spectrogram" (1, L): collate pads it like any other; utils.audio.gpu_front_end
            # turns the batch into log-spectrograms on the device
            return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))[None, :]
        if self.features == "fbank":
            return torch.from_numpy(log_mel_fbank(y, self.sample_rate, self.window_size, self.window_stride, self.normalize,
                                                  window=self.window, num_mel_bins=self.num_mel_bins, f_min=self.mel_fmin))
        return torch.from_numpy(log_spectrogram(y, self.sample_rate, self.window_size, self.window_stride, self.normalize,
                                                window=self.window))


class SpectrogramDataset(Dataset, SpectrogramParser):
    def __init__(self, audio_conf, manifest_filepath_list, label2id, normalize=False, augment=False, spec_augment=None):
        self.ids_list = []
        self.max_size = 0
        for path in manifest_filepath_list:
            with open(path) as f:
                ids = [ln.strip().split(',') for ln in f if ln.strip()]
            self.ids_list.append(ids)
            self.max_size = max(self.max_size, len(ids))
        self.manifest_filepath_list = manifest_filepath_list
        self.label2id = label2id
        SpectrogramParser.__init__(self, audio_conf, normalize, augment, spec_augment)

    def __getitem__(self, index):
        ids = self.ids_list[random.randint(0, len(self.ids_list) - 1)]      # one manifest at random, as the reference
        audio_path, transcript_path = ids[index % len(ids)][:2]
        spect = self.parse_audio(audio_path)
        if not getattr(constant.args, "gpu_frontend", False):
            spect = spect[:, :constant.args.src_max_len]
        if self.spec is not None:
            draws = self.draw(spect.size(1)) if self.augmenting else None
            return (spect, self.parse_transcript(transcript_path), draws,
                    self.draw_spec(draws[6] if draws is not None else spect.size(1)))
        if self.augmenting:
            return spect, self.parse_transcript(transcript_path), self.draw(spect.size(1))
        return spect, self.parse_transcript(transcript_path)

    def parse_transcript(self, transcript_path):
        with open(transcript_path, 'r', encoding='utf8') as f:
            text = constant.SOS_CHAR + f.read().replace('\n', '').lower() + constant.EOS_CHAR
        return [i for i in (self.label2id.get(c) for c in text) if i]      # filter(None, ...): drops unknowns and id 0

    def __len__(self):
        return self.max_size


def _collate_fn(batch):
    aug = len(batch[0]) > 2 and batch[0][2] is not None
    spec_rows = len(batch[0]) > 3
    size = (lambda s: s[2][6]) if aug else (lambda s: s[0].size(1))      # augmented: samples after the speed / tempo change
    batch = sorted(batch, key=size, reverse=True)
    B = len(batch)
    t_max = max(s[0].size(1) for s in batch)
    n_max = size(batch[0])
    f_bins = batch[0][0].size(0)
    l_max = max(len(s[1]) for s in batch)
    inputs = torch.zeros(B, 1, f_bins, t_max)
    targets = torch.zeros(B, l_max, dtype=torch.int64)
    input_sizes = torch.zeros(B, dtype=torch.int32)
    target_sizes = torch.zeros(B, dtype=torch.int32)
    input_percentages = torch.zeros(B, dtype=torch.float32)
    for i, s in enumerate(batch):
        spec, tgt = s[0], s[1]
        t = spec.size(1)
        inputs[i, 0, :, :t] = spec
        input_sizes[i] = size(s)
        input_percentages[i] = size(s) / float(n_max)
        target_sizes[i] = len(tgt)
        targets[i, :len(tgt)] = torch.tensor(tgt, dtype=torch.int64)
    # speed perturbation: a seventh column, the factor in thousandths; reverberation: an eighth, the index of the response
    draws = torch.tensor([s[2][:6] + s[2][7:9] for s in batch], dtype=torch.float64) if aug else None
    if spec_rows:
        return inputs, targets, input_percentages, input_sizes, target_sizes, draws, torch.tensor([s[3] for s in batch], dtype=torch.int32)
    if aug:
        return inputs, targets, input_percentages, input_sizes, target_sizes, draws
    return inputs, targets, input_percentages, input_sizes, target_sizes


class AudioDataLoader(DataLoader):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.collate_fn = _collate_fn


class DevicePrefetcher:
    """Iterates a loader one batch AHEAD: while the model works on batch i, batch i+1 is collated by the loader's workers,
    staged in pinned host memory and copied to the device on a copy stream of its own; the compute stream only waits for
    the copy's event.  The reference blocks on `src.cuda()` inside the step (trainer.py:63-66) -- at (32,1,161,800) fp32 that
    is 16.5 MB = 0.26 ms over PCIe Gen5 per step, 3 % of the accelerated step.  Yields the loader's tuples unchanged except
    that the tensors (inputs, targets) already live on `device`.  device=None: plain pass-through (CPU runs, tests)."""

    def __init__(self, loader, device=None, tensor_slots=(0, 1)):
        self.loader, self.device, self.slots = loader, device, tuple(tensor_slots)
        # persistent pinned staging, two buffers per slot (grow-only), filled by a SINGLE-THREADED copy (numpy): t.pin_memory() /
        # Tensor.copy_ of a 16.5 MB batch fan out over torch's intra-op pool (128 threads on the benchmark box), whose workers
        # then spin for their next task and slow the kernel-launch path of the step that follows 3.5 x (36 vs 10.3 ms per
        # trainer step, tools/trainer_rate.py); the copy itself is 0.3 ms either way
        self._pinned, self._events, self._turn = {}, {}, 0

    def __len__(self):
        return len(self.loader)

    def _staging(self, slot, t):
        """A pinned buffer holding a copy of host tensor t: buffer (slot, turn % 2), free again once the H2D copy that last read
        it has completed."""
        key = (slot, self._turn & 1)
        ev = self._events.get(key)
        if ev is not None:
            ev.synchronize()
        buf = self._pinned.get(key)
        n = t.numel()
        if buf is None or buf.dtype != t.dtype or buf.numel() < n:
            buf = torch.empty(max(n, 1), dtype=t.dtype).pin_memory()
            self._pinned[key] = buf
        view = buf[:n].view(t.shape)
        np.copyto(view.numpy(), t.numpy())
        return key, view

    def _stage(self, batch, stream):
        out = list(batch)
        used = []
        with torch.cuda.stream(stream):
            for i in self.slots:
                t = out[i]
                if torch.is_tensor(t) and not t.is_cuda:
                    if not t.is_pinned():
                        key, t = self._staging(i, t.contiguous())
                        used.append(key)
                    out[i] = t.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        for key in used:
            self._events[key] = ev
        self._turn += 1
        return out, ev

    def __iter__(self):
        if self.device is None or not torch.cuda.is_available():
            for batch in self.loader:
                yield batch
            return
        stream = torch.cuda.Stream(device=self.device)
        it = iter(self.loader)
        try:
            nxt = self._stage(next(it), stream)
        except StopIteration:
            return
        while nxt is not None:
            cur, ev = nxt
            try:
                nxt = self._stage(next(it), stream)         # batch i+1: H2D in flight while batch i computes
            except StopIteration:
                nxt = None
            torch.cuda.current_stream().wait_event(ev)
            for i in self.slots:
                if torch.is_tensor(cur[i]) and cur[i].is_cuda:
                    cur[i].record_stream(torch.cuda.current_stream())
            yield tuple(cur)


class BucketingSampler(Sampler):
    """Consecutive bins of `batch_size` indices (data is assumed sorted by length), shuffled inside a bin at iteration
    time and across bins by shuffle().  With rank/world given (or torch.distributed initialised) every rank iterates a
    disjoint, equally sized subset of the bins."""

    def __init__(self, data_source, batch_size=1, rank=None, world_size=None):
        self.data_source = data_source
        ids = list(range(len(data_source)))
        self.all_bins = [ids[i:i + batch_size] for i in range(0, len(ids), batch_size)]
        if rank is None and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world_size = torch.distributed.get_rank(), torch.distributed.get_world_size()
        self.rank, self.world = (rank or 0), (world_size or 1)
        self._shard()

    def _shard(self):
        self.bins = rank_shard(self.all_bins, self.rank, self.world) if self.world > 1 else self.all_bins

    def __iter__(self):
        for ids in self.bins:
            np.random.shuffle(ids)
            yield ids

    def __len__(self):
        return len(self.bins)

    def shuffle(self, epoch):
        rng = np.random.RandomState(1000003 * (epoch + 1))       # the same permutation on every rank
        rng.shuffle(self.all_bins)
        self._shard()
