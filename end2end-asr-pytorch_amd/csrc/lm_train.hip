// Training of the LSTM language model (asr_hip/lm_train.py): what csrc/lm.hip lacks for a backward pass.  fp32 storage, f32-input
// MFMA (v_mfma_f32_16x16x4_f32), fp32 accumulation, and lm.hip's conventions: time-major packed tokens (row step_off[t] + s, longest
// sentence first), unit-major gate rows (4 j + q = gate q of unit j), operand rows zero-padded to 16 floats, clamped row indices.
//
//   * lm_dropout          out = dropout(x[ids]) -- the embedding site -- and, in place on a gradient, the backward of any site;
//   * lstm_step_train     lstm_step that also keeps, per token, the activated gates i f g o and the cell state, writes the dropped
//                         copy of h (the next layer's / the decoder's input) and h again at the row of the SAME sentence's next step
//                         (the gathered h_prev of dW_hh = dG^T h_prev, made where h is produced);
//   * lstm_bptt_step      one (layer, step) of back-propagation through time: dh = dh_above + dG[t+1] W_hh (an MFMA contraction over
//                         4H against a transposed W_hh), cell and gate derivatives in the epilogue, dG[t] written over the gates;
//   * lm_train_loss       per-token log-sum-exp (kept for the backward) and the mean NLL, added in a fixed order;
//   * lm_dlogits          softmax / N of a chunk of tokens, logits recomputed with the forward's own tile.  The "- onehot" half of the
//                         output layer's gradient never enters a GEMM: it is one row operation per token (lm_sub_rows on dh, lm_emb_grad
//                         over the sorted targets on the decoder weight and bias).  The contraction over V that gives dh then adds
//                         V terms of one magnitude; with the target's term in it (V times larger than the others) every later add
//                         rounds at that term's magnitude, which cost a factor 8 in the error of dh at V = 32768;
//   * lm_colsum, lm_emb_grad, lm_sumsq   bias gradients, the sum of the rows of every word over sorted token ids (embedding gradient,
//                         onehot half of the decoder's), the gradient's squared norm.
// No reduction here uses atomics: every output element has one owner and a fixed summation order, so a step is reproducible to the
// bit.  Every time step is its own launch; nothing waits on another workgroup.
//
// Dropout: element (row m, column c) of a site with C columns is kept iff asr_keep(seed, m * C + c, thr), m the packed row; the seed
// is distinct per site and per step, the mask is never stored.
#include "lm_common.h"

namespace {

__global__ __launch_bounds__(256) void lm_dropout_kernel(const float* x, int64_t ldx, const int32_t* __restrict__ ids, float* out, int64_t ldo, int M, int C, uint64_t seed, uint32_t thr,
                                                         float scale) {
  const int m = blockIdx.x;
  const float* src = x + (int64_t)(ids ? ids[m] : m) * ldx;
  float* dst = out + (int64_t)m * ldo;
  for (int c = threadIdx.x; c < C; c += 256) dst[c] = asr_keep(seed, (uint64_t)m * C + c, thr) ? src[c] * scale : 0.f;
}

struct StepTrainArgs {
  const float* xproj; int64_t ldx;
  const float* hp; int64_t ldhp;          // h of the previous step (null at t = 0)
  const float* whh; int64_t ldw;
  const float* cp;                        // c of the previous step (null at t = 0)
  float* c; int64_t ldc;
  float* h; int64_t ldh;
  float* gates; int64_t ldg;              // activated i f g o, unit-major
  float* hd;                              // dropout(h) (ldh), or null
  float* hnext;                           // h at the rows of step t + 1 of the h_prev buffer (ldh), rows < n_next; or null
  int n, n_next, H, K16;
  int64_t row0;                           // packed row of this step's first row (dropout index)
  uint64_t seed; uint32_t thr; float scale;
};

template <int TN>
__global__ __launch_bounds__(256) void lstm_step_train_kernel(const StepTrainArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int u0 = (blockIdx.x * 4 + wave) * 4;
  if (u0 >= p.H) return;
  const int m0 = blockIdx.y * 16 * TN;
  f32x4_t acc[1][TN] = {};
  if (p.hp) lm_tile<1, TN>(p.whh, p.ldw, 4 * p.H, 4 * u0, p.hp, p.ldhp, nullptr, p.n, m0, p.K16, acc);
  const int u = u0 + g;
  if (u >= p.H) return;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int m = m0 + 16 * j + r;
    if (m >= p.n) continue;
    const f32x4_t gx = acc[0][j] + *reinterpret_cast<const f32x4_t*>(p.xproj + (int64_t)m * p.ldx + 4 * u);   // i, f, g, o
    const f32x4_t a = {sigmoidf_(gx[0]), sigmoidf_(gx[1]), tanhf(gx[2]), sigmoidf_(gx[3])};
    const float cn = a[1] * (p.cp ? p.cp[(int64_t)m * p.ldc + u] : 0.f) + a[0] * a[2];
    const float hn = a[3] * tanhf(cn);
    *reinterpret_cast<f32x4_t*>(p.gates + (int64_t)m * p.ldg + 4 * u) = a;
    p.c[(int64_t)m * p.ldc + u] = cn;
    p.h[(int64_t)m * p.ldh + u] = hn;
    if (p.hnext && m < p.n_next) p.hnext[(int64_t)m * p.ldh + u] = hn;
    if (p.hd) p.hd[(int64_t)m * p.ldh + u] = asr_keep(p.seed, (uint64_t)(p.row0 + m) * p.H + u, p.thr) ? hn * p.scale : 0.f;
  }
}

struct BpttArgs {
  const float* dh; int64_t lddh;          // gradient from above at this step's rows
  const float* dgn; int64_t ldg;          // dG of step t + 1 (n_next rows; null at the last step)
  const float* whht; int64_t ldwt;        // W_hh transposed: (H, 16 * ceil(4H / 16)), column 4 j + q = gate q of unit j
  float* g;                               // this step's gates (ldg): read activated, overwritten with the pre-activation gradients
  const float* c; const float* cp; int64_t ldc;   // c of this step, of the previous one (null at t = 0)
  float* dc; int64_t lddc;                // carried dL/dc (n_0, H): read for rows < n_next, written for all n rows
  int n, n_next, H, K16;
};

// 4 waves along the hidden units, 16 units each (A rows = rows of W_hh^T = units) x 16 * TN sequences; D: unit = 4 (l >> 4) + reg,
// sequence = l & 15.
template <int TN>
__global__ __launch_bounds__(256) void lstm_bptt_step_kernel(const BpttArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int u0 = (blockIdx.x * 4 + wave) * 16;
  if (u0 >= p.H) return;
  const int m0 = blockIdx.y * 16 * TN;
  f32x4_t acc[1][TN] = {};
  if (p.dgn) lm_tile<1, TN>(p.whht, p.ldwt, p.H, u0, p.dgn, p.ldg, nullptr, p.n_next, m0, p.K16, acc);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int m = m0 + 16 * j + r;
    if (m >= p.n) continue;
    const bool run = m < p.n_next;          // the sentence goes on after this step: it has a recurrent term and a carried dc
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = u0 + 4 * g + q;
      if (u >= p.H) continue;
      float* gp = p.g + (int64_t)m * p.ldg + 4 * u;
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(gp);          // i, f, g, o
      const float dh = p.dh[(int64_t)m * p.lddh + u] + (run ? acc[0][j][q] : 0.f);
      const float tc = tanhf(p.c[(int64_t)m * p.ldc + u]);
      float* dcp = p.dc + (int64_t)m * p.lddc + u;
      const float dc = dh * a[3] * (1.f - tc * tc) + (run ? *dcp : 0.f);
      const float cprev = p.cp ? p.cp[(int64_t)m * p.ldc + u] : 0.f;
      const f32x4_t d = {dc * a[2] * a[0] * (1.f - a[0]), dc * cprev * a[1] * (1.f - a[1]), dc * a[0] * (1.f - a[2] * a[2]),
                         dh * tc * a[3] * (1.f - a[3])};
      *reinterpret_cast<f32x4_t*>(gp) = d;
      *dcp = dc * a[1];
    }
  }
}

__device__ __forceinline__ void lse_merge2(float& m, float& s, float om, float os) {      // lm.hip's lse_merge
  const float nm = fmaxf(m, om);
  s = (m == -INFINITY ? 0.f : s * expf(m - nm)) + (om == -INFINITY ? 0.f : os * expf(om - nm));
  m = nm;
}

// One workgroup: thread i takes tokens i, i + 256, ...; the 256 sums meet in a fixed tree.
__global__ __launch_bounds__(256) void lm_train_loss_kernel(const float2* __restrict__ part, int nchunk, const float* __restrict__ tgt_logit,
                                                            int M, float inv_n, float* __restrict__ lse, float* __restrict__ loss) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int m = threadIdx.x; m < M; m += 256) {
    const float2* q = part + (int64_t)m * nchunk;
    float mx = q[0].x, sm = q[0].y;
    for (int k = 1; k < nchunk; ++k) lse_merge2(mx, sm, q[k].x, q[k].y);
    const float l = mx + logf(sm);
    lse[m] = l;
    acc += l - tgt_logit[m];
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] * inv_n;
}

// 4 waves side by side along the vocabulary; wave = 64 tokens x 64 words, the tile of lm_nll_partials (the same logits, bit for bit).
__global__ __launch_bounds__(256) void lm_dlogits_kernel(const float* __restrict__ hid, int64_t ldh, const float* __restrict__ w, int64_t ldw,
                                                         const float* __restrict__ bias, const float* __restrict__ lse, int M, int V, int Vp, int K16, float inv_n,
                                                         float* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int v0 = (blockIdx.x * 4 + wave) * 64;
  if (v0 >= Vp) return;
  const int m0 = blockIdx.y * 64;
  f32x4_t acc[4][4] = {};
  if (v0 < V) lm_tile<4, 4>(w, ldw, V, v0, hid, ldh, nullptr, M, m0, K16, acc);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + 16 * j + r;
    if (m >= M) continue;
    const float l = lse[m];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4_t d;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int v = v0 + 16 * i + 4 * g + q;
        d[q] = v < V ? expf(acc[i][j][q] + bias[v] - l) * inv_n : 0.f;
      }
      *reinterpret_cast<f32x4_t*>(out + (int64_t)m * ldo + v0 + 16 * i + 4 * g) = d;
    }
  }
}

// dh[m] -= w[tgt[m]] * inv_n: the onehot half of the output layer's data gradient.
__global__ __launch_bounds__(256) void lm_sub_rows_kernel(float* __restrict__ dh, int64_t ldd, const float* __restrict__ w, int64_t ldw,
                                                          const int32_t* __restrict__ tgt, int C, float inv_n) {
  const int m = blockIdx.x;
  const float* src = w + (int64_t)tgt[m] * ldw;
  float* dst = dh + (int64_t)m * ldd;
  for (int c = threadIdx.x; c < C; c += 256) dst[c] -= src[c] * inv_n;
}

// 64 columns x 4 row groups per workgroup; group k adds rows k, k + 4, ... in order, the four groups meet in order.
__global__ __launch_bounds__(256) void lm_colsum_kernel(const float* __restrict__ x, int64_t ld, int M, int N, float* __restrict__ out,
                                                        float* __restrict__ out2, int accumulate) {
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), k = threadIdx.x >> 6;
  float s = 0.f;
  if (col < N)
    for (int m = k; m < M; m += 4) s += x[(int64_t)m * ld + col];
  red[k][threadIdx.x & 63] = s;
  __syncthreads();
  if (k == 0 && col < N) {
    const float t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    const float v = accumulate ? out[col] + t : t;
    out[col] = v;
    if (out2) out2[col] = v;
  }
}

// One wave per distinct word: the rows of its tokens (ascending packed row) are added in that order.
__global__ __launch_bounds__(256) void lm_emb_grad_kernel(const float* __restrict__ dx, int64_t ldx, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_word,
                                                          int nseg, int E, float scale, float* __restrict__ demb, int64_t ldd) {
  const int lane = threadIdx.x & 63, sg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (sg >= nseg) return;
  const int a = seg_off[sg], b = seg_off[sg + 1];
  float* dst = demb + (int64_t)seg_word[sg] * ldd;
  for (int c = lane; c < E; c += 64) {
    float s = 0.f;
    for (int k = a; k < b; ++k) s += dx[(int64_t)rows[k] * ldx + c];
    dst[c] += scale * s;
  }
}

constexpr int LM_SUMSQ_BLOCKS = 256;

__global__ __launch_bounds__(256) void lm_sumsq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)LM_SUMSQ_BLOCKS * 256) s += g[i] * g[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void lm_sumsq_finish_kernel(const float* __restrict__ part, float* __restrict__ out) {
  __shared__ float red[256];
  red[threadIdx.x] = part[threadIdx.x];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

}  // namespace

extern "C" int asr_lm_dropout(const float* x, int64_t ldx, const int32_t* ids, float* out, int64_t ldo, int M, int C, float p,
                              uint64_t seed, hipStream_t s) {
  ASR_CHECK_ARG(x && out && M >= 0 && C > 0 && ldx >= C && ldo >= C && p >= 0.f && p < 1.f);
  if (M == 0) return ASR_OK;
  hipLaunchKernelGGL(lm_dropout_kernel, dim3(M), dim3(256), 0, s, x, ldx, ids, out, ldo, M, C, seed, asr_drop_threshold(p), 1.f / (1.f - p));
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lstm_step_train(const float* xproj, int64_t ldx, const float* h_prev, int64_t ldhp, const float* whh, int64_t ldw,
                                   const float* c_prev, float* c, int64_t ldc, float* h, int64_t ldh, float* gates, int64_t ldg,
                                   float* h_drop, float* h_next, int n, int n_next, int H, int64_t row0, float p, uint64_t seed,
                                   hipStream_t s) {
  const int K16 = (H + 15) / 16;
  ASR_CHECK_ARG(xproj && whh && c && h && gates && n >= 0 && n_next >= 0 && n_next <= n && H > 0 && ok_rows(xproj, ldx) && ldx >= 4 * H);
  ASR_CHECK_ARG(ok_rows(whh, ldw) && ldw >= 16 * K16 && ldc >= H && ldh >= H && ok_rows(gates, ldg) && ldg >= 4 * H);
  ASR_CHECK_ARG((!h_prev) == (!c_prev) && (!h_prev || (ok_rows(h_prev, ldhp) && ldhp >= 16 * K16)) && p >= 0.f && p < 1.f && row0 >= 0);
  if (n == 0) return ASR_OK;
  StepTrainArgs a{xproj, ldx, h_prev, ldhp, whh, ldw, c_prev, c, ldc, h, ldh, gates, ldg, h_drop, h_next, n, n_next, H, K16, row0, seed,
                  asr_drop_threshold(p), 1.f / (1.f - p)};
  const unsigned gx = (unsigned)ceil_div64(H, 16);
  if (n > 16) hipLaunchKernelGGL(lstm_step_train_kernel<4>, dim3(gx, ceil_div64(n, 64)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(lstm_step_train_kernel<1>, dim3(gx, 1), dim3(256), 0, s, a);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lstm_bptt_step(const float* dh, int64_t lddh, const float* dg_next, float* g, int64_t ldg, const float* whh_t,
                                  int64_t ldwt, const float* c, const float* c_prev, int64_t ldc, float* dc, int64_t lddc, int n,
                                  int n_next, int H, hipStream_t s) {
  const int K16 = (4 * H + 15) / 16;
  ASR_CHECK_ARG(dh && g && whh_t && c && dc && n >= 0 && n_next >= 0 && n_next <= n && H > 0 && lddh >= H && ldc >= H && lddc >= H);
  ASR_CHECK_ARG(ok_rows(g, ldg) && ldg >= 16 * K16 && ok_rows(whh_t, ldwt) && ldwt >= 16 * K16 && (n_next == 0 || dg_next));
  ASR_CHECK_ARG(!dg_next || aligned16(dg_next));
  if (n == 0) return ASR_OK;
  BpttArgs a{dh, lddh, n_next > 0 ? dg_next : nullptr, ldg, whh_t, ldwt, g, c, c_prev, ldc, dc, lddc, n, n_next, H, K16};
  const unsigned gx = (unsigned)ceil_div64(H, 64);
  if (n > 16) hipLaunchKernelGGL(lstm_bptt_step_kernel<4>, dim3(gx, ceil_div64(n, 64)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(lstm_bptt_step_kernel<1>, dim3(gx, 1), dim3(256), 0, s, a);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_train_loss(const float* part, int nchunk, const float* tgt_logit, int M, float* lse, float* loss, hipStream_t s) {
  ASR_CHECK_ARG(part && tgt_logit && lse && loss && nchunk > 0 && M > 0 && aligned16(part));
  hipLaunchKernelGGL(lm_train_loss_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const float2*>(part), nchunk, tgt_logit, M,
                     1.f / (float)M, lse, loss);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_dlogits(const float* h, int64_t ldh, const float* w, int64_t ldw, const float* bias, const float* lse, int M, int V, int K, float inv_n, float* out, int64_t ldo, hipStream_t s) {
  const int K16 = (K + 15) / 16;
  const int Vp = (int)(ceil_div64(V, 64) * 64);
  ASR_CHECK_ARG(h && w && bias && lse && out && M >= 0 && V > 0 && K > 0);
  ASR_CHECK_ARG(ok_rows(h, ldh) && ok_rows(w, ldw) && ldh >= 16 * K16 && ldw >= 16 * K16 && ok_rows(out, ldo) && ldo >= Vp);
  if (M == 0) return ASR_OK;
  hipLaunchKernelGGL(lm_dlogits_kernel, dim3(ceil_div64(Vp, 256), ceil_div64(M, 64)), dim3(256), 0, s, h, ldh, w, ldw, bias, lse, M,
                     V, Vp, K16, inv_n, out, ldo);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_sub_rows(float* dh, int64_t ldd, const float* w, int64_t ldw, const int32_t* tgt, int M, int C, float inv_n,
                               hipStream_t s) {
  ASR_CHECK_ARG(dh && w && tgt && M >= 0 && C > 0 && ldd >= C && ldw >= C);
  if (M == 0) return ASR_OK;
  hipLaunchKernelGGL(lm_sub_rows_kernel, dim3(M), dim3(256), 0, s, dh, ldd, w, ldw, tgt, C, inv_n);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_colsum(const float* x, int64_t ld, int M, int N, float* out, float* out2, int accumulate, hipStream_t s) {
  ASR_CHECK_ARG(x && out && M >= 0 && N > 0 && ld >= N);
  hipLaunchKernelGGL(lm_colsum_kernel, dim3(ceil_div64(N, 64)), dim3(256), 0, s, x, ld, M, N, out, out2, accumulate);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_emb_grad(const float* dx, int64_t ldx, const int32_t* rows, const int32_t* seg_off, const int32_t* seg_word, int nseg,
                               int E, float scale, float* demb, int64_t ldd, hipStream_t s) {
  ASR_CHECK_ARG(dx && rows && seg_off && seg_word && demb && nseg >= 0 && E > 0 && ldx >= E && ldd >= E);
  if (nseg == 0) return ASR_OK;
  hipLaunchKernelGGL(lm_emb_grad_kernel, dim3(ceil_div64(nseg, 4)), dim3(256), 0, s, dx, ldx, rows, seg_off, seg_word, nseg, E, scale, demb, ldd);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_lm_sumsq_floats(void) { return LM_SUMSQ_BLOCKS; }

extern "C" int asr_lm_sumsq(const float* g, int64_t n, float* partials, float* out, hipStream_t s) {
  ASR_CHECK_ARG(g && partials && out && n >= 0);
  hipLaunchKernelGGL(lm_sumsq_partial_kernel, dim3(LM_SUMSQ_BLOCKS), dim3(256), 0, s, g, n, partials);
  hipLaunchKernelGGL(lm_sumsq_finish_kernel, dim3(1), dim3(256), 0, s, partials, out);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
