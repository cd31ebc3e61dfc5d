// Sequence log-probabilities of a rescoring batch (attention rescoring of the CTC n-best): what
// F.log_softmax(logits, -1).gather(-1, tgt) and a masked sum per hypothesis compute, without the (M, V) log-probability tensor.
//   tok_lp[m] = logits[m, tgt[m]] - logsumexp(logits[m, :V])          score[r] = sum of tok_lp over rows seg_off[r] .. seg_off[r + 1] - 1
// Two launches.  seq_row_kernel: one wave per row, SEQ_ROWS rows per workgroup (ce_fwd_kernel's shape), the row read ONCE.
// seq_sum_kernel: one lane per segment adds its rows in row order.  A segment's rows lie in several workgroups of the first launch, so
// adding them in its tail would need an order between workgroups (a counter and atomics); R lanes of a second launch need neither, and
// the bits are a function of the input alone.  HBM-bound: M * V * 4 bytes in, M + R floats out.
// Requirement: every row has at least one finite logit among its V and none is +inf.
#include "common.h"

namespace {

// No multiply-add contraction in this file: the compiler chooses where to fuse loop by loop, and the two load arms of the row pass
// must round the same sums at the same places.
#pragma clang fp contract(off)

constexpr int SEQ_ROWS = 8;                    // == CE_ROWS of csrc/ce.hip

// Online log-sum-exp state of a set of logits: m = their maximum and s1 = sum exp(x - m) over all of them EXCEPT one copy of the maximum
// (whose term is exactly 1), so that logsumexp - m = log1p(s1).  A row whose target is its arg max has a log-probability near 0, and
// log(1 + s1) from a rounded 1 + s1 would lose it; log1p(s1) keeps s1's own relative precision.  m = -inf: the empty set (or all -inf).
struct Lse { float m, s1; };

// a, then b: the pair of a butterfly step in (lower lane, higher lane) order, so both lanes compute the same bits
__device__ __forceinline__ Lse lse_merge(Lse a, Lse b) {
  const bool first = a.m >= b.m;
  const Lse hi = first ? a : b, lo = first ? b : a;
  if (lo.m == -INFINITY) return hi;
  return Lse{hi.m, hi.s1 + (lo.s1 + 1.f) * expf(lo.m - hi.m)};
}

// one logit into a lane's state: one expf whichever of the two is larger, and no branch.  Both load arms of the row pass feed the same
// values in the same order through this, which is what makes their results the same bits.
__device__ __forceinline__ void lse_add(Lse& st, float x) {
  const bool up = x > st.m;
  float e = expf(fminf(x, st.m) - fmaxf(x, st.m));          // exp(-inf) = 0: the first finite value of a lane, or a -inf logit
  if (x == -INFINITY) e = 0.f;                              // (-inf) - (-inf) is not a number
  st.s1 = up ? (st.s1 + 1.f) * e : st.s1 + e;               // a new maximum: the old one becomes an ordinary term
  st.m = up ? x : st.m;
}
__device__ __forceinline__ void lse_add4(Lse& st, float x0, float x1, float x2, float x3) {
  lse_add(st, x0); lse_add(st, x1); lse_add(st, x2); lse_add(st, x3);
}

__global__ __launch_bounds__(64 * SEQ_ROWS) void seq_row_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt,
                                                                int M, int V, float* __restrict__ tok_lp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * SEQ_ROWS + wave;
  if (row >= M) return;
  const float* l = logits + (int64_t)row * ld;
  const int V4 = V & ~3;
  Lse st{-INFINITY, 0.f};
  // Lane `lane` owns columns 4 lane + 256 k .. + 3 in BOTH arms, then column V4 + lane of the tail: the arms differ in how the four
  // values are loaded and in nothing else, so a row gives the same bits through either (tests/test_gpu_attn_rescore.py pins it).
  if ((((uintptr_t)l) & 15) == 0) {            // 16-byte loads, four in flight per lane
#pragma unroll 4
    for (int v = lane * 4; v < V4; v += 256) {
      const float4 x = *reinterpret_cast<const float4*>(l + v);
      lse_add4(st, x.x, x.y, x.z, x.w);
    }
  } else {                                     // a row base that is no multiple of 16 bytes (ld = V = 3): the same columns, one by one
    for (int v = lane * 4; v < V4; v += 256) lse_add4(st, l[v], l[v + 1], l[v + 2], l[v + 3]);
  }
  if (V4 + lane < V) lse_add(st, l[V4 + lane]);          // columns >= V are never read
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {           // wave64 butterfly (the idiom of ce.hip): every lane merges (lower lane, higher lane) in that order
    const Lse t{__shfl_xor(st.m, o, 64), __shfl_xor(st.s1, o, 64)};
    st = (lane & o) ? lse_merge(t, st) : lse_merge(st, t);
  }
  if (lane == 0) {
    const int64_t t = tgt[row];
    float lp = -INFINITY;                      // a target outside [0, V): -inf, nothing read
    if (t >= 0 && t < V) {
      const float xt = l[t];
      if (xt > -INFINITY) lp = (xt - st.m) - log1pf(st.s1);      // (x - max) - log(sum): exact 0 - 0 when the target holds all the mass
    }
    tok_lp[row] = lp;
  }
}

// One lane per segment, rows added in row order in fp64 and rounded once: a segment of a few hundred terms keeps the precision of its
// terms (an fp32 running sum of 300 terms drifts by a few ulp of the total).  Offsets are clamped to [0, M]: no read outside tok_lp.
__global__ __launch_bounds__(64) void seq_sum_kernel(const float* __restrict__ tok_lp, const int32_t* __restrict__ seg_off, int R, int M,
                                                     float* __restrict__ score) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int a = max(seg_off[r], 0), b = min(seg_off[r + 1], M);
  double acc = 0.0;
  for (int m = a; m < b; ++m) acc += (double)tok_lp[m];
  score[r] = (float)acc;                       // an empty segment: exactly 0
}

}  // namespace

extern "C" int asr_seq_logprob(const float* logits, int64_t ld, const int64_t* tgt, const int32_t* seg_off, int R, int M, int V,
                               float* tok_lp, float* score, hipStream_t s) {
  ASR_CHECK_ARG(R >= 0 && M >= 0 && V >= 1 && ld >= V);
  ASR_CHECK_ARG((M == 0 || (logits && tgt && tok_lp)) && (R == 0 || (seg_off && score)));
  if (M == 0 || R == 0) {
    if (R > 0 && hipMemsetAsync(score, 0, sizeof(float) * (size_t)R, s) != hipSuccess) return ASR_ERUNTIME;
    return ASR_OK;
  }
  hipLaunchKernelGGL(seq_row_kernel, dim3((M + SEQ_ROWS - 1) / SEQ_ROWS), dim3(64 * SEQ_ROWS), 0, s, logits, ld, tgt, M, V, tok_lp);
  ASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(seq_sum_kernel, dim3((R + 63) / 64), dim3(64), 0, s, tok_lp, seg_off, R, M, score);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
