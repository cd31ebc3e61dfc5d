// asr_ctx_step: n transitions of the phrase automaton's lookup table (csrc/context.h has the step, utils/context.py builds the table).
// One thread per transition; memory bound: a step reads hold[s], two keys and the two values beside them, more only where a first probe
// met another key.
// csrc/ctc_beam.hip runs the same step per live extension slot; this entry holds the device step to the host's, exactly.
#include "context.h"

namespace {

__global__ __launch_bounds__(256) void ctx_step_kernel(CtxTable t, const int32_t* __restrict__ state, const int32_t* __restrict__ sym,
                                                       int64_t n, int32_t* __restrict__ next, int32_t* __restrict__ delta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int2 r = ctx_step(t, state[i], sym[i]);
  next[i] = r.x;
  delta[i] = r.y;
}

}  // namespace

extern "C" int asr_ctx_step(const uint64_t* keys, const int32_t* vals, int64_t capacity, int max_probe, const int32_t* hold, int states,
                            const int32_t* state, const int32_t* sym, int64_t n, int32_t* next, int32_t* delta, hipStream_t s) {
  const int rc = ctx_check_table(keys, vals, capacity, max_probe, hold, states);
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 38));
  if (n == 0) return ASR_OK;
  ASR_CHECK_ARG(state && sym && next && delta);
  const CtxTable t{keys, reinterpret_cast<const int2*>(vals), hold, (uint32_t)(capacity - 1), max_probe, states};
  hipLaunchKernelGGL(ctx_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, state, sym, n, next, delta);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
