#!/usr/bin/env python3
"""Record tests/golden/beam_fuse.npz: the outputs of every fused arm of the two beam searches on the cases of
tests/test_gpu_beam_fuse_golden.py, from whatever libasr_hip.so the tree holds.

TEST INFRASTRUCTURE ONLY: run it on an MI355X with a build of the commit whose bits are to be kept (the fixture in the tree is from the
commit before csrc/beam_fuse.h); the test then holds every later library to them.

    python tools/gen_beam_fuse_golden.py [OUT.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "end2end-asr-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import test_gpu_beam_fuse_golden as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    arrays = {}
    for name in T.NAMES:
        got = T.compute(name)
        for k, v in got.items():
            arrays["%s/%s" % (name, k)] = v.numpy()
        print(name, {k: tuple(v.shape) for k, v in got.items()}, "found", int((got["lengths"] >= 0).sum()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
