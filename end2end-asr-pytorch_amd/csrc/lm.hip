// LSTM language model for beam-search rescoring (reference: utils/lstm_utils.py LM.evaluate / RNNModel.forward), fp32 in /
// fp32 accumulate on v_mfma_f32_16x16x4_f32 whatever the ASR model's precision.
//
// Four kernels, all one 16x16 MFMA fragment per (wave, tile) with the operand pack of common.h (lane l: row l & 15, 4
// consecutive k at 4 (l >> 4) of every 16-wide k step):
//   * lm_proj         out = X W^T + bias over all tokens of a layer (layer 0 gathers embedding rows through `ids`);
//   * lstm_step       one time step of one layer: gates = xproj[t] + h[t-1] W_hh^T, then the cell update.  W_hh's rows are
//                     packed unit-major (row 4 j + q = gate q of unit j), so the four gates of a unit land in ONE lane's four
//                     accumulator registers (D row = A row) and the epilogue needs no lane exchange;
//   * nll_partials    logits of a 64-token x 256-word chunk, reduced in registers to per-token (max, sum exp) and the target
//                     logit: the (tokens x V) logits never reach memory;
//   * nll_finish      per-token NLL = logsumexp over the chunks (fixed order) - target logit; per-sequence sums.
// Every output element is computed by one lane with an instruction sequence that does not depend on the tile it sits in or on
// how many rows are launched: a sentence's score is bitwise the same alone or inside any batch.
//
// The contraction operands have rows padded with zeros to a multiple of 16 floats (K16 16-wide steps) and 16-byte aligned
// rows; row indices past the end of an operand are clamped (their results are discarded), so no load leaves the tensors.
#include "lm_common.h"

namespace {

constexpr int LM_NLL_CHUNK = 256;     // vocabulary words per partial (one wave)

// 256 threads = 4 waves side by side along N; a wave owns 32 output columns x 64 tokens.
__global__ __launch_bounds__(256) void lm_proj_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ ids,
                                                      const float* __restrict__ w, int64_t ldw, const float* __restrict__ bias,
                                                      float* __restrict__ out, int64_t ldo, int M, int N, int K16) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int n0 = (blockIdx.x * 4 + wave) * 32;
  if (n0 >= N) return;
  const int m0 = blockIdx.y * 64;
  f32x4_t acc[2][4] = {};
  lm_tile<2, 4>(w, ldw, N, n0, x, ldx, ids, M, m0, K16, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = n0 + 16 * i + 4 * g;
    if (n >= N) continue;
    const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(bias + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + 16 * j + r;
      if (m < M) *reinterpret_cast<f32x4_t*>(out + (int64_t)m * ldo + n) = acc[i][j] + bb;
    }
  }
}

// 4 waves along the hidden units (4 units = 16 packed gate rows each) x 16 * TN sequences.
template <int TN>
__global__ __launch_bounds__(256) void lstm_step_kernel(const float* __restrict__ xproj, int64_t ldx, const float* __restrict__ hp,
                                                        int64_t ldhp, const float* __restrict__ whh, int64_t ldw, float* __restrict__ c,
                                                        int64_t ldc, float* __restrict__ h, int64_t ldh, int n, int H, int K16) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int u0 = (blockIdx.x * 4 + wave) * 4;
  if (u0 >= H) return;
  const int m0 = blockIdx.y * 16 * TN;
  f32x4_t acc[1][TN] = {};
  if (hp) lm_tile<1, TN>(whh, ldw, 4 * H, 4 * u0, hp, ldhp, nullptr, n, m0, K16, acc);
  const int u = u0 + g;
  if (u >= H) return;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int m = m0 + 16 * j + r;
    if (m >= n) continue;
    const f32x4_t gx = acc[0][j] + *reinterpret_cast<const f32x4_t*>(xproj + (int64_t)m * ldx + 4 * u);   // i, f, g, o
    float* cp = c + (int64_t)m * ldc + u;
    const float cn = sigmoidf_(gx[1]) * (hp ? *cp : 0.f) + sigmoidf_(gx[0]) * tanhf(gx[2]);
    *cp = cn;
    h[(int64_t)m * ldh + u] = sigmoidf_(gx[3]) * tanhf(cn);
  }
}

// (m, s) <- the log-sum-exp pair of (m, s) and (om, os); symmetric in its two arguments (both lanes of a butterfly agree).
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  s = (m == -INFINITY ? 0.f : s * expf(m - nm)) + (om == -INFINITY ? 0.f : os * expf(om - nm));
  m = nm;
}

// 4 waves side by side along the vocabulary; wave = one 256-word chunk x 64 tokens, 4 sub-tiles of 64 words.
__global__ __launch_bounds__(256) void lm_nll_partials_kernel(const float* __restrict__ hid, int64_t ldh, const float* __restrict__ w,
                                                              int64_t ldw, const float* __restrict__ bias, const int32_t* __restrict__ tgt,
                                                              int M, int V, int K16, int nchunk, float2* __restrict__ part,
                                                              float* __restrict__ tgt_logit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int chunk = blockIdx.x * 4 + wave;
  if (chunk >= nchunk) return;
  const int m0 = blockIdx.y * 64;
  float mx[4], sm[4];
  int tg[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mx[j] = -INFINITY;
    sm[j] = 0.f;
    tg[j] = tgt[min(m0 + 16 * j + r, M - 1)];
  }
  for (int sub = 0; sub < LM_NLL_CHUNK / 64; ++sub) {
    const int v0 = chunk * LM_NLL_CHUNK + sub * 64;
    if (v0 >= V) break;
    f32x4_t acc[4][4] = {};
    lm_tile<4, 4>(w, ldw, V, v0, hid, ldh, nullptr, M, m0, K16, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + 16 * j + r;
      float lmax = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int v = v0 + 16 * i + 4 * g + q;
          if (v < V) {
            const float xv = acc[i][j][q] + bias[v];
            acc[i][j][q] = xv;
            lmax = fmaxf(lmax, xv);
            if (v == tg[j] && m < M) tgt_logit[m] = xv;
          }
        }
      float add = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (v0 + 16 * i + 4 * g + q < V) add += expf(acc[i][j][q] - fmaxf(mx[j], lmax));
      const float nm = fmaxf(mx[j], lmax);
      sm[j] = (mx[j] == -INFINITY ? 0.f : sm[j] * expf(mx[j] - nm)) + add;
      mx[j] = nm;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) lse_merge(mx[j], sm[j], __shfl_xor(mx[j], o, 64), __shfl_xor(sm[j], o, 64));
    const int m = m0 + 16 * j + r;
    if (g == 0 && m < M) part[(int64_t)m * nchunk + chunk] = make_float2(mx[j], sm[j]);
  }
}

// One wave per sequence: lane t (+ 64 k) takes token t; the per-sequence sum is a fixed butterfly over the lanes.
__global__ __launch_bounds__(256) void lm_nll_finish_kernel(const float2* __restrict__ part, int nchunk, const float* __restrict__ tgt_logit,
                                                            const int32_t* __restrict__ step_off, const int32_t* __restrict__ lens, int S,
                                                            float* __restrict__ nll_tok, float* __restrict__ nll_sum) {
  const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= S) return;
  const int L = lens[s];
  float acc = 0.f;
  for (int t = lane; t < L; t += 64) {
    const int64_t m = (int64_t)step_off[t] + s;
    const float2* p = part + m * nchunk;
    float mx = p[0].x, sm = p[0].y;
    for (int k = 1; k < nchunk; ++k) lse_merge(mx, sm, p[k].x, p[k].y);
    const float nll = mx + logf(sm) - tgt_logit[m];
    if (nll_tok) nll_tok[m] = nll;
    acc += nll;
  }
  acc = wave_sum(acc);
  if (lane == 0) nll_sum[s] = acc;
}

}  // namespace

extern "C" int asr_lm_proj(const float* x, int64_t ldx, const int32_t* ids, const float* w, int64_t ldw, const float* bias, float* out,
                           int64_t ldo, int M, int N, int K, hipStream_t s) {
  const int K16 = (K + 15) / 16;
  ASR_CHECK_ARG(x && w && bias && out && M >= 0 && N > 0 && N % 4 == 0 && K > 0);
  ASR_CHECK_ARG(ok_rows(x, ldx) && ok_rows(w, ldw) && ok_rows(out, ldo) && aligned16(bias) && ldx >= 16 * K16 && ldw >= 16 * K16 && ldo >= N);
  if (M == 0) return ASR_OK;
  hipLaunchKernelGGL(lm_proj_kernel, dim3(ceil_div64(N, 128), ceil_div64(M, 64)), dim3(256), 0, s, x, ldx, ids, w, ldw, bias, out, ldo,
                     M, N, K16);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lstm_step(const float* xproj, int64_t ldx, const float* h_prev, int64_t ldhp, const float* whh, int64_t ldw, float* c,
                             int64_t ldc, float* h, int64_t ldh, int n, int H, hipStream_t s) {
  const int K16 = (H + 15) / 16;
  ASR_CHECK_ARG(xproj && whh && c && h && n >= 0 && H > 0 && ok_rows(xproj, ldx) && ldx >= 4 * H && ok_rows(whh, ldw) && ldw >= 16 * K16);
  ASR_CHECK_ARG(ldc >= H && ldh >= H && (!h_prev || (ok_rows(h_prev, ldhp) && ldhp >= 16 * K16)));
  if (n == 0) return ASR_OK;
  const dim3 grid(ceil_div64(H, 16), 1);
  if (n > 16) {
    hipLaunchKernelGGL(lstm_step_kernel<4>, dim3(grid.x, ceil_div64(n, 64)), dim3(256), 0, s, xproj, ldx, h_prev, ldhp, whh, ldw, c, ldc,
                       h, ldh, n, H, K16);
  } else {
    hipLaunchKernelGGL(lstm_step_kernel<1>, dim3(grid.x, 1), dim3(256), 0, s, xproj, ldx, h_prev, ldhp, whh, ldw, c, ldc, h, ldh, n, H,
                       K16);
  }
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_nll_chunks(int V) { return V > 0 ? (int)ceil_div64(V, LM_NLL_CHUNK) : 0; }

extern "C" int asr_lm_nll_partials(const float* h, int64_t ldh, const float* w, int64_t ldw, const float* bias, const int32_t* tgt, int M,
                                   int V, int K, float* part, float* tgt_logit, hipStream_t s) {
  const int K16 = (K + 15) / 16;
  ASR_CHECK_ARG(h && w && bias && tgt && part && tgt_logit && M >= 0 && V > 0 && K > 0);
  ASR_CHECK_ARG(ok_rows(h, ldh) && ok_rows(w, ldw) && ldh >= 16 * K16 && ldw >= 16 * K16 && aligned16(part));
  if (M == 0) return ASR_OK;
  const int nchunk = asr_lm_nll_chunks(V);
  hipLaunchKernelGGL(lm_nll_partials_kernel, dim3(ceil_div64(nchunk, 4), ceil_div64(M, 64)), dim3(256), 0, s, h, ldh, w, ldw, bias, tgt,
                     M, V, K16, nchunk, reinterpret_cast<float2*>(part), tgt_logit);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_nll_finish(const float* part, int nchunk, const float* tgt_logit, const int32_t* step_off, const int32_t* lens, int S,
                                 float* nll_tok, float* nll_sum, hipStream_t s) {
  ASR_CHECK_ARG(part && tgt_logit && step_off && lens && nll_sum && nchunk > 0 && S >= 0 && aligned16(part));
  if (S == 0) return ASR_OK;
  hipLaunchKernelGGL(lm_nll_finish_kernel, dim3(ceil_div64(S, 4)), dim3(256), 0, s, reinterpret_cast<const float2*>(part), nchunk,
                     tgt_logit, step_off, lens, S, nll_tok, nll_sum);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
