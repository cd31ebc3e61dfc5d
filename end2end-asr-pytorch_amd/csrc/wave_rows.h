// What the kernels over padded (B, cols) waveforms share (csrc/resample.hip, csrc/reverb.hip): one workgroup per (tile of consecutive
// outputs, row), rows read and written four samples at a time -- with 16-byte accesses where the row's base and stride allow it (vec_in /
// vec_out) -- and the entry checks of such a launch.
#pragma once
#include "common.h"

// columns [m, m + 4) of a row that is copied or zero: x below `live`, +0.0 from there on
__device__ __forceinline__ void copy_or_zero4(const float* __restrict__ x, float* __restrict__ y, int m, int live, int out_cols,
                                              bool vec_in, bool vec_out) {
  if (m >= out_cols) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec_in && m + 3 < live) {
    v = *reinterpret_cast<const float4*>(x + m);
  } else {
    if (m < live) v.x = x[m];
    if (m + 1 < live) v.y = x[m + 1];
    if (m + 2 < live) v.z = x[m + 2];
    if (m + 3 < live) v.w = x[m + 3];
  }
  if (vec_out && m + 3 < out_cols) {
    *reinterpret_cast<float4*>(y + m) = v;
  } else {
    y[m] = v.x;
    if (m + 1 < out_cols) y[m + 1] = v.y;
    if (m + 2 < out_cols) y[m + 2] = v.z;
    if (m + 3 < out_cols) y[m + 3] = v.w;
  }
}

// The guarded four-sample staging load of the two kernels is NOT here: as one function it gave both other, slower code, so each keeps
// its form written out inside its staging loop (profiles/frontend_refactor.txt, section 3).

// The entry checks of a launch over wav (B, >= n) -> out (B, out_cols) in tiles of `tile` outputs: pointers, a row count that fits
// gridDim.y, strides, and a column count whose last tile does not overflow an int.  False: the entry refuses (ASR_EINVAL).
struct WaveRowsLaunch {
  int vec_in, vec_out;                           // 16-byte loads / stores possible: base aligned, row stride a multiple of 4
  dim3 grid;                                     // (tiles, B)
};
static inline bool wave_rows_launch(const float* wav, int64_t wav_stride, const float* out, int64_t out_stride, int out_cols, int B, int tile,
                                    WaveRowsLaunch* l) {
  if (!(wav && out && B >= 0 && B <= 65535 && wav_stride >= 0 && out_cols >= 0 && out_stride >= out_cols && out_cols <= 0x7fffffff - tile))
    return false;
  l->vec_in = aligned16(wav) && wav_stride % 4 == 0;
  l->vec_out = aligned16(out) && out_stride % 4 == 0;
  l->grid = dim3((unsigned)((out_cols + tile - 1) / tile), (unsigned)B);
  return true;
}
