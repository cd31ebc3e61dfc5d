// The fused beam searches' addend to a hypothesis' score in its rank key (csrc/ctc_beam.hip, csrc/rnnt_beam.hip): fp32, in this order --
// alpha lm + beta (float)len, then + gamma (float)cnt.  lm: the fp32 sum of the n-gram query over the labels, len: their number, cnt: the
// phrase automaton's credit.  Without an LM lm is 0.f and alpha is not looked at; without phrases gamma and cnt are not.  One expression
// for both searches; gamma times an integer is the same bits on the device and on the host.
#pragma once
#include "common.h"

namespace {

template <bool LM, bool CTX>
__device__ __forceinline__ float beam_bonus(float alpha, float beta, float gamma, float lm, int len, int cnt) {
  float a;
  if constexpr (LM) a = alpha * lm + beta * (float)len;
  else a = 0.f * lm + beta * (float)len;
  if constexpr (CTX) a = a + gamma * (float)cnt;
  return a;
}

}  // namespace
