// Sequence log-probabilities of a rescoring batch (attention rescoring of the CTC n-best): what
// F.log_softmax(logits, -1).gather(-1, tgt) and a masked sum per hypothesis compute, without the (M, V) log-probability tensor.
//   tok_lp[m] = logits[m, tgt[m]] - logsumexp(logits[m, :V])          score[r] = sum of tok_lp over rows seg_off[r] .. seg_off[r + 1] - 1
// Two launches.  seq_row_kernel: one wave per row, SEQ_ROWS rows per workgroup (ce_fwd_kernel's shape), the row read ONCE.
// seq_sum_kernel: one lane per segment adds its rows in row order.  A segment's rows lie in several workgroups of the first launch, so
// adding them in its tail would need an order between workgroups (a counter and atomics); R lanes of a second launch need neither, and
// the bits are a function of the input alone.  HBM-bound: M * V * 4 bytes in, M + R floats out.
// Requirement: every row has at least one finite logit among its V and none is +inf.
#include "common.h"
#include "lse.h"        // Lse, lse_row: shared with the backward (csrc/mwer.hip); no multiply-add contraction from here on

namespace {

constexpr int SEQ_ROWS = 8;                    // == CE_ROWS of csrc/ce.hip

__global__ __launch_bounds__(64 * SEQ_ROWS) void seq_row_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt,
                                                                int M, int V, float* __restrict__ tok_lp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * SEQ_ROWS + wave;
  if (row >= M) return;
  const float* l = logits + (int64_t)row * ld;
  const Lse st = lse_row(l, V, lane);           // the row read ONCE; both load arms give the same bits (csrc/lse.h)
  if (lane == 0) {
    const int64_t t = tgt[row];
    float lp = -INFINITY;                      // a target outside [0, V): -inf, nothing read
    if (t >= 0 && t < V) {
      const float xt = l[t];
      if (xt > -INFINITY) lp = (xt - st.m) - log1pf(st.s1);      // lse_logprob of csrc/lse.h written out: the logarithm only where the target has mass
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
  ASR_TRY(asr_launch<seq_row_kernel>(dim3((M + SEQ_ROWS - 1) / SEQ_ROWS), dim3(64 * SEQ_ROWS), 0, s, logits, ld, tgt, M, V, tok_lp));
  return asr_launch<seq_sum_kernel>(dim3((R + 63) / 64), dim3(64), 0, s, tok_lp, seg_off, R, M, score);
}
