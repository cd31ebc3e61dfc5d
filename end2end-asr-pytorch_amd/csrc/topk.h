// The arg-max order of the top-k selections: greater value first, lowest index first among equals.  Shared by csrc/ce.hip (argmax,
// asr_logsoftmax_topk) and csrc/rnnt_beam.hip (the label candidates of a joint row), so both select in one order.
#pragma once
#include "common.h"

namespace {

struct MaxIdx { float v; int i; };
__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b) {     // greater value, lowest index on ties
  if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
  return a;
}

// the best of the 64 lanes' entries, in every lane (wave64 butterfly)
__device__ __forceinline__ MaxIdx wave_best(MaxIdx mi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MaxIdx t{__shfl_xor(mi.v, o, 64), __shfl_xor(mi.i, o, 64)};
    mi = better(mi, t);
  }
  return mi;
}

}  // namespace
