"""The last pass of the GPU front end at the training shape, 32 utterances of 8 s (configs[1]'s 32 x 161 x 800 features): the plain
front end (spect_normalize_kernel, plus the copy of the --src-max-len cut when there is one) and the front end with SpecAugment
fused into that pass (spec_augment_kernel) under the default policy (W 80, F 27 x 2, T 100 x 2, p 1.0), drawn by the loader's own code.
Kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/mb_specaug.py 3`; this script prints device-event times of the
whole front end.  A tree without SpecAugment runs the plain front end only.
usage: python tools/mb_specaug.py [reps] [src_max_len]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "end2end-asr-pytorch_amd"))
from asr_hip import ops  # noqa: E402
from utils import constant  # noqa: E402
from utils.audio import gpu_front_end  # noqa: E402

D = torch.device("cuda:0")
SR, B, SECS = 16000, 32, 8


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
    cut = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    L = SECS * SR - 1                                                     # 800 frames
    wav = torch.from_numpy((rng.randn(B, 1, 1, L) * 0.1).astype(np.float32)).to(D)
    sizes = torch.full((B,), L, dtype=torch.int32)

    def plain():
        return gpu_front_end(wav, sizes, SR, src_max_len=cut)

    p = median_ms(plain, reps)
    print("B=%d x %d s, cut %d: front end %.3f ms (min %.3f max %.3f)" % (B, SECS, cut, p[0], p[1], p[2]))
    if not hasattr(ops, "spec_augment"):
        return
    from utils.data_loader import SpectrogramParser, spec_policy
    constant.parse(["--gpu-frontend", "--spec-augment", "--src-max-len", str(cut)])
    parser = SpectrogramParser(dict(sample_rate=SR, window_size=.02, window_stride=.01), spec_augment=spec_policy(constant.args))
    np.random.seed(0)
    rows = torch.tensor([parser.draw_spec(L) for _ in range(B)], dtype=torch.int32)

    def fused():
        return gpu_front_end(wav, sizes, SR, src_max_len=cut, spec=rows)

    a, ref = fused()[0], plain()[0]
    keep = a != 0
    print("rows: c %s w %s; %.1f %% of the features masked" % (rows[:4, 1].tolist(), rows[:4, 2].tolist(), 100 * (1 - keep.float().mean().item())))
    assert a.shape == ref.shape and torch.isfinite(a).all()
    f = median_ms(fused, reps)
    p2 = median_ms(plain, reps)
    print("B=%d x %d s, cut %d: front end + SpecAugment %.3f ms (min %.3f max %.3f) | front end again %.3f ms (min %.3f max %.3f)"
          % (B, SECS, cut, f[0], f[1], f[2], p2[0], p2[1], p2[2]))


if __name__ == "__main__":
    main()
