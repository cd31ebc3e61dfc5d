// asr_ngram_logp: n queries of the label n-gram LM's lookup table (csrc/ngram.h has the query, utils/ngram.py builds the table).
// One thread per query; memory bound: a query reads its order - 1 context ids, up to 2 order - 1 keys and as many values as it hits.
// csrc/ctc_beam.hip runs the same query per live extension slot; this entry holds the device query to the host's, bit for bit.
#include "ngram.h"

namespace {

__global__ __launch_bounds__(256) void ngram_logp_kernel(NgramTable t, const int32_t* __restrict__ ctx, const int32_t* __restrict__ sym,
                                                         int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint64_t key = 0;                            // oldest first; -1 (or an id that fits no field) cuts the context: what stands before it is dropped
  for (int j = 0; j < t.order - 1; ++j) {
    const int s = ctx[i * (t.order - 1) + j];
    key = s < 0 || s > NGRAM_MAX_ID ? 0 : key << 16 | (uint64_t)(s + 1);
  }
  out[i] = ngram_query(t, key, sym[i]);
}

}  // namespace

extern "C" int asr_ngram_logp(const uint64_t* keys, const float* vals, int64_t capacity, int max_probe, int order, const int32_t* ctx,
                              const int32_t* sym, int64_t n, float* out, hipStream_t s) {
  const int rc = ngram_check_table(keys, vals, capacity, max_probe, order);
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 38));
  if (n == 0) return ASR_OK;
  ASR_CHECK_ARG(sym && out && (order == 1 || ctx));
  const NgramTable t{keys, reinterpret_cast<const float2*>(vals), (uint32_t)(capacity - 1), max_probe, order};
  hipLaunchKernelGGL(ngram_logp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, ctx, sym, n, out);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
