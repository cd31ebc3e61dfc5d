// What the loss heads on a vocabulary projection share (csrc/ce.hip, distill.hip, rnnt_lattice.h): label smoothing, the
// fixed-order finish of per-workgroup partial sums, and the logit-gradient row every backward writes for the projection's data-gradient
// GEMM (GradRow) -- T = fp32 or bf16, ldd >= V wide, columns V .. ldd-1 zero, a row that carries no gradient all zero and its logits unread.
// The arg-max order is csrc/topk.h, the row log-sum-exp csrc/lse.h.
// This header sets no contraction mode of its own: ce.hip compiles it with multiply-add contraction, as its kernels always were; a
// file whose two load arms must round alike includes it BEHIND its `#pragma clang fp contract(off)` (or behind lse.h, which has one).
#pragma once
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ label smoothing
// the target distribution of a row: q_gold on the label, q_other on every other column; sum_q is their sum as the kernels round it
struct Smoothing {
  float q_gold, q_other, sum_q;
  __device__ __forceinline__ Smoothing(float eps, int V) {
    q_other = eps > 0.f ? eps / (float)V : 0.f;
    q_gold = eps > 0.f ? 1.f - eps : 1.f;
    sum_q = q_gold + (float)(V - 1) * q_other;
  }
};

// -sum_v q[v] log p[v] of a row from lpg = log p[gold], sum = the sum of its V logits and its log-sum-exp (reference: utils/metrics.py:118-130)
__device__ __forceinline__ float smoothed_row_loss(float lpg, float sum, int V, float lse, float eps) {
  if (eps > 0.f) {
    const float sum_lp = sum - (float)V * lse;
    return -((1.f - eps) * lpg + (eps / (float)V) * (sum_lp - lpg));
  }
  return -lpg;
}

// ------------------------------------------------------------------------------------------------ finish
// red[k][0] = the workgroups' k-th partial sums added in a fixed order (thread t of 256 takes slots t, t + 256, ...; then a tree over the
// threads): the same bits run to run, and nobody has to zero a destination first.  Ends behind a barrier: every thread may read red[k][0].
template <int K>
__device__ __forceinline__ void finish_sums(const float* __restrict__ partials, int nblocks, float (&red)[K][256]) {
  const int tid = threadIdx.x;
  float a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = 0.f;
  for (int b = tid; b < nblocks; b += 256)
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] += partials[(int64_t)b * K + k];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k][tid] = a[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
#pragma unroll
      for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + o];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ gradient rows
// four output elements of one lane: one 16-byte (fp32) or 8-byte (bf16) store where p allows it (`vec` = vec4_ok of p, or of a row base
// that p is a multiple of four elements behind), else one by one
template <typename T> __device__ __forceinline__ bool vec4_ok(const T* p) { return (((uintptr_t)p) & (4 * sizeof(T) - 1)) == 0; }
__device__ __forceinline__ f32x4_t pack4(float a, float b, float c, float d, const float*) { return f32x4_t{a, b, c, d}; }
__device__ __forceinline__ ushort4 pack4(float a, float b, float c, float d, const bf16_t*) {
  return make_ushort4(f32_to_bf16(a), f32_to_bf16(b), f32_to_bf16(c), f32_to_bf16(d));
}
template <typename T> __device__ __forceinline__ void store4(T* p, bool vec, float a, float b, float c, float d) {
  if (vec) *reinterpret_cast<decltype(pack4(a, b, c, d, p))*>(p) = pack4(a, b, c, d, p);
  else { DT<T>::st(p, a); DT<T>::st(p + 1, b); DT<T>::st(p + 2, c); DT<T>::st(p + 3, d); }
}

// The gradient row of one wave.  Built ONCE at the top of a kernel, in front of the branch between a row without a gradient and a live
// one: both arms then test the same `vst`.  (Testing the alignment again behind the branch costs the fp32 arms their merged stores --
// four single-dword stores per four columns instead of two, 30 % of asr_rnnt_bwd's time; profiles/loss_rows_refactor.txt.)
template <typename T> struct GradRow {
  T* d;
  int64_t ldd;
  int ldd4;                                    // the columns owned four at a time
  bool vst;                                    // this row's stores may be four elements wide
  __device__ __forceinline__ GradRow(T* d_, int64_t ldd_) : d(d_), ldd(ldd_), ldd4((int)(ldd_ & ~(int64_t)3)), vst(vec4_ok(d_)) {}

  // a row that carries no gradient: ldd zeros, nothing read
  __device__ __forceinline__ void zero(int lane) const {
    for (int v = lane * 4; v < ldd4; v += 256) store4(d + v, vst, 0.f, 0.f, 0.f, 0.f);
    if (ldd4 + lane < ldd) DT<T>::st(d + ldd4 + lane, 0.f);
  }

  // A live row: d[v] = f(v, l[v]) for v < V and 0 behind.  Lane `lane` owns columns 4 lane + 256 k .. + 3 up to ldd4 (the columns lse_row
  // had it read: they come from cache), then column ldd4 + lane: one owner per element, no atomics.  The four logits come by one 16-byte
  // load or one by one; a column >= V is never read and f sees -inf there (it must be finite on it: exp(-inf) = 0).
  template <typename F> __device__ __forceinline__ void write(const float* __restrict__ l, int V, int lane, F&& f) const {
    const bool vld = (((uintptr_t)l) & 15) == 0;
    for (int v = lane * 4; v < ldd4; v += 256) {
      float x[4];
      if (vld && v + 3 < V) {
        const float4 q = *reinterpret_cast<const float4*>(l + v);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = v + j < V ? l[v + j] : -INFINITY;
      }
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gj = f(v + j, x[j]);
        o[j] = v + j < V ? gj : 0.f;
      }
      // (written out, not store4: through the call the bf16 arms come out 13 to 15 instructions longer)
      if (vst) *reinterpret_cast<decltype(pack4(o[0], o[1], o[2], o[3], d))*>(d + v) = pack4(o[0], o[1], o[2], o[3], d);
      else { DT<T>::st(d + v, o[0]); DT<T>::st(d + v + 1, o[1]); DT<T>::st(d + v + 2, o[2]); DT<T>::st(d + v + 3, o[3]); }
    }
    const int v = ldd4 + lane;
    if (v < ldd) DT<T>::st(d + v, v < V ? f(v, l[v]) : 0.f);
  }
};

}  // namespace
