// What the transducer head's kernels share: csrc/rnnt.hip (loss) and csrc/rnnt_beam.hip (search) add log-probabilities in fp64 with one
// log-add, so a hypothesis' score in the search is the lattice's sum in the loss.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ double rnnt_lae(double a, double b) {      // log(exp(a) + exp(b)), -inf safe
  const double hi = fmax(a, b), lo = fmin(a, b);
  if (lo == -(double)INFINITY) return hi;
  return hi + log1p(exp(lo - hi));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace
