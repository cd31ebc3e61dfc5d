// Shared by the LSTM language model's kernels (csrc/lm.hip: inference; csrc/lm_train.hip: training): the direct-from-memory
// 16x16 MFMA tile of the packed, zero-padded fp32 operands.
#pragma once
#include <math.h>

#include "common.h"

namespace {

// acc[i][j] += A[a0 + 16 i + (0..15)] . B[b0 + 16 j + (0..15)]^T over 16 * K16 columns.  D: row (A) = 4 (l >> 4) + reg,
// column (B) = l & 15.  b_ids: B row r is b[b_ids[r]] (an embedding gather) when not null.
template <int TM, int TN>
__device__ __forceinline__ void lm_tile(const float* __restrict__ a, int64_t lda, int a_rows, int a0, const float* __restrict__ b,
                                        int64_t ldb, const int32_t* __restrict__ b_ids, int b_rows, int b0, int K16,
                                        f32x4_t (&acc)[TM][TN]) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const float* pa[TM];
  const float* pb[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) pa[i] = a + (int64_t)min(a0 + 16 * i + r, a_rows - 1) * lda + 4 * g;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    int row = min(b0 + 16 * j + r, b_rows - 1);
    if (b_ids) row = b_ids[row];
    pb[j] = b + (int64_t)row * ldb + 4 * g;
  }
  for (int kk = 0; kk < K16; ++kk) {
    uint4 va[TM], vb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) va[i] = *reinterpret_cast<const uint4*>(pa[i] + 16 * kk);
#pragma unroll
    for (int j = 0; j < TN; ++j) vb[j] = *reinterpret_cast<const uint4*>(pb[j] + 16 * kk);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) mma16<float>(acc[i][j], va[i], vb[j]);
  }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

inline bool ok_rows(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace
