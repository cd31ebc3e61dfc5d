"""asr_augment_wave at the training shape: 32 utterances of 8 s (configs[1]'s 800 frames), tempo / gain drawn from the full
ranges, noise on every other utterance.  Prints the median over repeated runs (HIP events) of augment alone, augment + STFT
front end and the STFT front end alone, at 8 s and at 16 s.  Kernel times come from a separate rocprofv3 run (profiles/augment.txt).
usage: python tools/mb_augment.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "end2end-asr-pytorch_amd"))
from asr_hip import ops  # noqa: E402
from utils.audio import NoiseBank  # noqa: E402

D = torch.device("cuda:0")
SR, B = 16000, 32


def _bank(tmp):
    import wave
    os.makedirs(tmp, exist_ok=True)
    rng = np.random.RandomState(1)
    for i in range(4):
        with wave.open(os.path.join(tmp, "n%d.wav" % i), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(SR)
            f.writeframes((rng.randn(20 * SR) * 3000).clip(-32768, 32767).astype("<i2").tobytes())
    return NoiseBank(tmp, SR, D)


def median_ms(fn, reps, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.cuda.set_device(0)
    import tempfile
    bank = _bank(tempfile.mkdtemp(prefix="mb_augment_noise"))
    rng = np.random.RandomState(0)
    for secs in (8, 16):
        L = secs * SR
        wav = torch.from_numpy((rng.randn(B, L) * 0.1).astype(np.float32)).to(D)
        lens = torch.full((B,), L, dtype=torch.int32)
        params = torch.tensor([(float("%.3f" % rng.uniform(0.85, 1.15)), float("%.3f" % rng.uniform(-6, 8)),
                                (i % 4) if i % 2 == 0 else -1, rng.uniform(0, 5), rng.uniform(0, 0.5)) for i in range(B)],
                              dtype=torch.float64)
        lens_d = lens.to(D)

        def aug():
            return ops.augment_wave(wav, lens, params, bank, sample_rate=SR)

        def aug_stft():
            w, n = aug()
            return ops.log_spectrogram(w, n)

        def stft():
            return ops.log_spectrogram(wav, lens_d)

        a, s, st = median_ms(aug, reps), median_ms(aug_stft, reps), median_ms(stft, reps)
        print("B=%d x %d s: augment %.3f ms (min %.3f max %.3f) | augment+STFT %.3f ms (min %.3f max %.3f) | STFT alone %.3f ms "
              "(min %.3f max %.3f)" % (B, secs, a[0], a[1], a[2], s[0], s[1], s[2], st[0], st[1], st[2]))


if __name__ == "__main__":
    main()
