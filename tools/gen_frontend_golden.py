#!/usr/bin/env python3
"""Record tests/golden/frontend.npz: the outputs of the GPU audio front end on the bit-exact cases of tests/test_gpu_frontend_golden.py,
from whatever libasr_hip.so the tree holds.

TEST INFRASTRUCTURE ONLY: run it on an MI355X with a build of the commit whose bits are to be kept (the fixture in the tree is from the
commit before csrc/wave_rows.h and features_finish); the test then holds every later library to them.  The conditions the cases rest on
(the tile past an utterance's end, the span beyond the LDS image, the tap counts, the short utterance) are asserted while the cases are
computed, so a reseeding cannot hollow them out.

    python tools/gen_frontend_golden.py [OUT.npz]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "end2end-asr-pytorch_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import test_gpu_frontend_golden as T  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    arrays = {}
    for name in T.NAMES:
        got = T.compute(name)
        for k, v in got.items():
            arrays["%s/%s" % (name, k)] = v.numpy()
        print(name, {k: tuple(v.shape) for k, v in got.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
