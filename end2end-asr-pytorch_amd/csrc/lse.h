// Online log-sum-exp of a logits row, one wave per row: shared by csrc/seq_logprob.hip (forward), csrc/mwer.hip (its backward) and the
// transducer's row pass (csrc/rnnt_lattice.h), so a backward recomputes the forward's normaliser with the forward's code and the forward's bits.
// A file that includes this compiles WITHOUT multiply-add contraction from here on: the compiler chooses where to fuse loop by loop, and
// the two load arms of the row pass must round the same sums at the same places.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

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

// log softmax of a logit x of a set with maximum m and lz = log1pf(s1) (computed once per row by the caller): (x - max) - log(sum),
// exact 0 - 0 when x holds all the mass.  x = -inf gives -inf.
__device__ __forceinline__ float lse_logprob(float x, float m, float lz) { return (x - m) - lz; }

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

// The state of the V logits at l, in every lane of the wave that calls it (all 64 lanes, together).
// Lane `lane` owns columns 4 lane + 256 k .. + 3 in BOTH arms, then column V4 + lane of the tail: the arms differ in how the four
// values are loaded and in nothing else, so a row gives the same bits through either (tests/test_gpu_attn_rescore.py pins it).
__device__ __forceinline__ Lse lse_row(const float* __restrict__ l, int V, int lane) {
  const int V4 = V & ~3;
  Lse st{-INFINITY, 0.f};
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
  return st;
}

}  // namespace
