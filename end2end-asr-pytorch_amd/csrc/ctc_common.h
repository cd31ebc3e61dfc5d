// Pieces shared by the CTC loss (ctc.hip) and the CTC prefix scorer (ctc_prefix.hip): the -inf safe log-add and the row
// log-sum-exp kernel that turns logits into log-probabilities.
#pragma once
#include "common.h"

namespace {

constexpr float NEG_INF = -INFINITY;

__device__ __forceinline__ float lae2(float a, float b) {      // log(exp(a) + exp(b)), -inf safe
  const float m = fmaxf(a, b);
  if (m == NEG_INF) return NEG_INF;
  return m + logf(expf(a - m) + expf(b - m));
}

// one wave per row: lse[row] = log sum_v exp(logits[row, v])
__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ logits, int64_t ld, int64_t rows, int V,
                                                      float* __restrict__ lse) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* x = logits + row * ld;
  float m = NEG_INF;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
  m = wave_max(m);
  float s = 0.f;
  for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
  s = wave_sum(s);
  if (lane == 0) lse[row] = m + logf(s);
}

}  // namespace
