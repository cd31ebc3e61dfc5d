// The arg-max order of the top-k selections: greater value first, lowest index first among equals.  Shared by csrc/ce.hip (argmax,
// asr_logsoftmax_topk), csrc/distill.hip (the student's argmax) and csrc/rnnt_beam.hip (the label candidates of a joint row), so all
// select in one order.
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

// the best of a 256-thread workgroup's entries, in thread 0 ONLY (the other threads get their wave's).  One barrier inside; a caller in a
// loop puts one behind its use of the result, before the next call overwrites the four slots.
__device__ __forceinline__ MaxIdx block_best(MaxIdx mi) {
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  mi = wave_best(mi);
  if (lane == 0) { s_v[wave] = mi.v; s_i[wave] = mi.i; }
  __syncthreads();
  if (threadIdx.x == 0) {
    mi = MaxIdx{s_v[0], s_i[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w) mi = better(mi, MaxIdx{s_v[w], s_i[w]});
  }
  return mi;
}

}  // namespace
