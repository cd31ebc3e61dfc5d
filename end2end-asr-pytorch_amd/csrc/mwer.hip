// Minimum word error rate (MWER) training over the CTC n-best: the two kernels the n-best pipeline lacked.
//
// asr_seq_logprob_bwd: the backward of asr_seq_logprob (csrc/seq_logprob.hip).  Row m of segment r, c = grad_out * coef[r]:
//   dlogits[m, v] = c * ([v == tgt[m]] - softmax(logits[m, :V])[v])
// One wave per row, SEQ_BWD_ROWS rows per workgroup (seq_row_kernel's shape).  The log-sum-exp is recomputed with the forward's code
// (lse_row of csrc/lse.h: the same bits through the 16-byte and the scalar arm), then the row is read a second time (from cache) and
// every lane writes the four columns it read: one owner per element, no atomics.  The output has the form asr_ce_bwd writes for the
// vocabulary projection's data-gradient GEMM: fp32 or bf16, row width ldd >= V, columns V .. ldd-1 zero.
// HBM-bound: M * V * 4 bytes in, M * ldd * {2,4} out.
//
// asr_mwer_loss: softmax over an utterance's hypothesis scores, the expected error above the list's mean, and the coefficients the
// backward above multiplies into the rows.  One lane per utterance walks its hypotheses in index order; one lane adds the B risks and gold
// scores in utterance order after the others have finished: the bits are a function of the input alone.
#include "common.h"
#include "lse.h"        // Lse, lse_row (no multiply-add contraction from here on: a row gives the same bits through either arm)

namespace {

constexpr int SEQ_BWD_ROWS = 8;                // == SEQ_ROWS of csrc/seq_logprob.hip

template <typename T> struct Vec4;             // four output elements of one lane: a 16-byte (fp32) or 8-byte (bf16) store
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<bf16_t> { typedef ushort4 type; };
__device__ __forceinline__ float4 pack4(const float (&o)[4], float*) { return make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ ushort4 pack4(const float (&o)[4], bf16_t*) {
  return make_ushort4(f32_to_bf16(o[0]), f32_to_bf16(o[1]), f32_to_bf16(o[2]), f32_to_bf16(o[3]));
}

// the segment that owns row m: the LAST r with seg_off[r] <= m (empty segments in front of it share the offset and own nothing), or -1
__device__ __forceinline__ int segment_of(const int32_t* __restrict__ seg_off, int R, int m) {
  if (R <= 0 || m < seg_off[0] || m >= seg_off[R]) return -1;
  int lo = 0, hi = R;                          // seg_off[lo] <= m < seg_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= m) lo = mid; else hi = mid;
  }
  return lo;
}

// (GradRow of csrc/loss_rows.h writes the same row shape for rnnt_bwd_kernel.  This kernel stays written out: through the shared writer its
// fp32 arm measured 1.3 % above the parent's range at M 3360 and the bf16 arm gained nothing; profiles/loss_rows_refactor.txt.)
template <typename T>
__global__ __launch_bounds__(64 * SEQ_BWD_ROWS) void seq_bwd_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ tgt,
                                                                    const int32_t* __restrict__ seg_off, const float* __restrict__ coef,
                                                                    const float* __restrict__ grad_out, int R, int M, int V,
                                                                    T* __restrict__ dl, int64_t ldd) {
  typedef typename Vec4<T>::type V4T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * SEQ_BWD_ROWS + wave;
  if (row >= M) return;
  T* d = dl + (int64_t)row * ldd;
  const int ldd4 = (int)(ldd & ~(int64_t)3);
  const bool vst = (((uintptr_t)d) & (sizeof(V4T) - 1)) == 0;           // this row's stores may be four elements wide
  // everything up to here and the three values below are the same in all lanes of the wave (a row per wave)
  const int r = segment_of(seg_off, R, row);
  const int64_t t = tgt[row];
  float c = 0.f;
  if (r >= 0 && t >= 0 && t < V) c = (grad_out ? grad_out[0] : 1.f) * coef[r];
  if (c == 0.f) {                              // a row that carries no gradient (or a target outside [0, V)): zeros, its logits are not read
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = lane * 4; v < ldd4; v += 256) {
      if (vst) *reinterpret_cast<V4T*>(d + v) = pack4(z, d);
      else { DT<T>::st(d + v, 0.f); DT<T>::st(d + v + 1, 0.f); DT<T>::st(d + v + 2, 0.f); DT<T>::st(d + v + 3, 0.f); }
    }
    if (ldd4 + lane < ldd) DT<T>::st(d + ldd4 + lane, 0.f);
    return;
  }
  const float* l = logits + (int64_t)row * ld;
  const Lse st = lse_row(l, V, lane);
  const float lz = log1pf(st.s1);              // logsumexp = st.m + lz; the forward's tok_lp is (x - st.m) - lz, and so is the exponent here
  const bool vld = (((uintptr_t)l) & 15) == 0;
  const int tcol = (int)t;
  // second pass: lane `lane` owns columns 4 lane + 256 k .. + 3 up to ldd4 (the columns it read, from cache), then column ldd4 + lane
  for (int v = lane * 4; v < ldd4; v += 256) {
    float x[4];
    if (vld && v + 3 < V) {
      const float4 q = *reinterpret_cast<const float4*>(l + v);
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = v + j < V ? l[v + j] : -INFINITY;            // columns >= V are never read
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = expf((x[j] - st.m) - lz);                                       // exp(-inf) = 0: a -inf logit, a pad column
      o[j] = v + j < V ? c * ((v + j == tcol ? 1.f : 0.f) - p) : 0.f;
    }
    if (vst) *reinterpret_cast<V4T*>(d + v) = pack4(o, d);
    else { DT<T>::st(d + v, o[0]); DT<T>::st(d + v + 1, o[1]); DT<T>::st(d + v + 2, o[2]); DT<T>::st(d + v + 3, o[3]); }
  }
  const int v = ldd4 + lane;
  if (v < ldd) {
    float o = 0.f;
    if (v < V) o = c * ((v == tcol ? 1.f : 0.f) - expf((l[v] - st.m) - lz));
    DT<T>::st(d + v, o);
  }
}

// One workgroup.  Thread u takes utterances u, u + 256, ...: segments utt_off[b] (gold) and utt_off[b] + 1 .. utt_off[b + 1] - 1 (the
// hypotheses), walked in index order in fp32.  Then thread 0 adds the risks and the gold scores in utterance order.
__global__ __launch_bounds__(256) void mwer_loss_kernel(const float* __restrict__ score, const float* __restrict__ err,
                                                        const int32_t* __restrict__ utt_off, int B, int R, float risk_scale, float gold_scale,
                                                        float* __restrict__ prob, float* __restrict__ coef, float* __restrict__ risk,
                                                        float* __restrict__ sums) {
  for (int b = threadIdx.x; b < B; b += 256) {
    const int g = min(max(utt_off[b], 0), R), end = min(max(utt_off[b + 1], g), R);     // offsets clamped to [0, R]: no access outside
    float rk = 0.f;
    if (g < end) {
      prob[g] = 0.f;
      coef[g] = -gold_scale;
      const int h0 = g + 1, n = end - h0;
      float mx = -INFINITY;
      for (int i = h0; i < end; ++i) mx = fmaxf(mx, score[i]);
      if (n <= 1 || mx == -INFINITY) {           // nothing to rank (or no hypothesis with any mass): risk 0, no gradient
        for (int i = h0; i < end; ++i) { prob[i] = (n == 1 && mx > -INFINITY) ? 1.f : 0.f; coef[i] = 0.f; }
      } else {
        float z = 0.f, esum = 0.f;
        for (int i = h0; i < end; ++i) { z += expf(score[i] - mx); esum += err[i]; }     // exp(-inf) = 0
        const float emean = esum / (float)n;
        float ebar = 0.f;
        for (int i = h0; i < end; ++i) {
          const float p = expf(score[i] - mx) / z;
          prob[i] = p;
          ebar += p * err[i];
          rk += p * (err[i] - emean);
        }
        for (int i = h0; i < end; ++i) coef[i] = risk_scale * (prob[i] * (err[i] - ebar));
      }
    }
    risk[b] = rk;
  }
  __syncthreads();                               // the risks above are visible to thread 0 (one workgroup)
  if (threadIdx.x == 0) {
    float a = 0.f, s = 0.f;
    for (int b = 0; b < B; ++b) {
      const int g = min(max(utt_off[b], 0), R), end = min(max(utt_off[b + 1], g), R);
      a += risk[b];
      if (g < end) s += score[g];
    }
    sums[0] = a;
    sums[1] = s;
  }
}

}  // namespace

extern "C" int asr_seq_logprob_bwd(const float* logits, int64_t ld, const int64_t* tgt, const int32_t* seg_off, const float* coef,
                                   const float* grad_out, int R, int M, int V, void* dlogits, int64_t ldd, int out_dtype, hipStream_t s) {
  ASR_CHECK_ARG(R >= 0 && M >= 0 && V >= 1 && ld >= V && ldd >= V);
  ASR_CHECK_ARG(out_dtype == ASR_F32 || out_dtype == ASR_BF16);
  ASR_CHECK_ARG(M == 0 || (logits && tgt && dlogits && (R == 0 || (seg_off && coef))));
  if (M == 0) return ASR_OK;
  const dim3 grid((M + SEQ_BWD_ROWS - 1) / SEQ_BWD_ROWS), block(64 * SEQ_BWD_ROWS);
  return asr_with_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    return asr_launch<seq_bwd_kernel<T>>(grid, block, 0, s, logits, ld, tgt, seg_off, coef, grad_out, R, M, V, (T*)dlogits, ldd);
  });
}

extern "C" int asr_mwer_loss(const float* score, const float* err, const int32_t* utt_off, int B, int R, float risk_scale, float gold_scale,
                             float* prob, float* coef, float* risk, float* sums, hipStream_t s) {
  ASR_CHECK_ARG(B >= 0 && R >= 0 && sums && utt_off && (B == 0 || risk) && (R == 0 || (score && err && prob && coef)));
  return asr_launch<mwer_loss_kernel>(dim3(1), dim3(256), 0, s, score, err, utt_off, B, R, risk_scale, gold_scale, prob, coef, risk, sums);
}
