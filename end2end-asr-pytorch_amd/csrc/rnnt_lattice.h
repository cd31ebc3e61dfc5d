// The transducer loss kernels that csrc/rnnt.hip (the full T x (U + 1) lattice) and csrc/rnnt_pruned.hip (a band of W label positions per
// frame) share: the row pass, the fp64 lattice, the finish and the gradient.  One source, so the arithmetic of a row
// is the same in both.  BAND = false: row (b,t,u) of the logits is cell (t,u).  BAND = true: the logits are (B,T,W,ld), row (b,t,w) is cell
// (t, s_begin[b,t] + w); lse is kept by row, lpb / lpl / alpha / beta by cell, and the caller has filled lpb / lpl with -inf, so a node
// outside the band has no outgoing arc.  With W = U + 1 and s_begin = 0 the two are the same bits.
#pragma once
#include "common.h"
#include "lse.h"        // Lse, lse_row, lse_logprob (no multiply-add contraction from here on: a row gives the same bits through either load arm)
#include "loss_rows.h"  // GradRow: the gradient rows (shared with csrc/mwer.hip)
#include "rnnt_common.h"      // rnnt_lae, clampi

namespace {

constexpr int RNNT_ROWS = 8;                   // rows (waves) per workgroup of the row pass and the backward: == SEQ_ROWS of csrc/seq_logprob.hip

// row -> (b t, u, cell); s_begin is clamped to [0, U1 - W], so a cell is inside the lattice whatever the caller hands in
template <bool BAND>
__device__ __forceinline__ void rnnt_row_map(int64_t row, int U1, int W, const int32_t* __restrict__ s_begin, int64_t& bt, int& u, int64_t& cell) {
  if constexpr (BAND) {
    const int w = (int)(row % W);
    bt = row / W;
    u = clampi(s_begin[bt], 0, U1 - W) + w;
    cell = bt * U1 + u;
  } else {
    u = (int)(row % U1);
    bt = row / U1;
    cell = row;
  }
}

// ------------------------------------------------------------------------------------------------ loss: row pass
// one wave per row (b,t,u); a live row leaves its log-sum-exp and the two log-probabilities the lattice needs, a dead row is not read.
// A label that is the blank or outside [0,V) reads nothing and leaves -inf (the lattice kernel refuses the utterance as a whole).
template <bool BAND>
__global__ __launch_bounds__(64 * RNNT_ROWS) void rnnt_row_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets,
                                                                  const int32_t* __restrict__ frames, const int32_t* __restrict__ tg_len,
                                                                  int Tn, int Umax, int V, int blank, int64_t rows,
                                                                  float* __restrict__ lse, float* __restrict__ lpb, float* __restrict__ lpl,
                                                                  const int32_t* __restrict__ s_begin, int W) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * RNNT_ROWS + wave;
  if (row >= rows) return;
  const int U1 = Umax + 1;
  int u;
  int64_t bt, cell;
  rnnt_row_map<BAND>(row, U1, W, s_begin, bt, u, cell);
  const int t = (int)(bt % Tn);
  const int b = (int)(bt / Tn);
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  if (t >= Tb || u > Ub) return;
  const float* l = logits + row * ld;
  const Lse st = lse_row(l, V, lane);
  if (lane == 0) {
    const float lz = log1pf(st.s1);
    lse[row] = st.m + lz;
    lpb[cell] = lse_logprob(l[blank], st.m, lz);
    float ll = -INFINITY;
    if (u < Ub) {
      const int64_t y = targets[(int64_t)b * Umax + u];
      if (y >= 0 && y < V && y != blank) ll = lse_logprob(l[y], st.m, lz);
    }
    lpl[cell] = ll;
  }
}

// ------------------------------------------------------------------------------------------------ loss: lattice
// grid (B, 2): y = 0 alpha, y = 1 beta.  LDS: [2][U1] doubles, the previous / current diagonal by u.
__global__ __launch_bounds__(256) void rnnt_lattice_kernel(const int64_t* __restrict__ targets, const int32_t* __restrict__ frames,
                                                           const int32_t* __restrict__ tg_len, int Tn, int Umax, int V, int blank,
                                                           const float* __restrict__ lpb, const float* __restrict__ lpl,
                                                           double* __restrict__ alpha, double* __restrict__ beta, double* __restrict__ nll_d,
                                                           float* __restrict__ nll) {
  extern __shared__ double sh[];
  const int U1 = Umax + 1;
  double* prev = sh;
  double* cur = sh + U1;
  const int b = blockIdx.x;
  const bool backward = blockIdx.y == 1;
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  bool bad = false;
  for (int i = threadIdx.x; i < Ub; i += 256) {
    const int64_t y = targets[(int64_t)b * Umax + i];
    bad |= y < 0 || y >= V || y == blank;
  }
  bad = __syncthreads_or(bad) != 0 || Tb == 0;
  if (bad) {                                   // no alignment exists: +inf, and the backward writes zero rows (block-uniform)
    if (!backward && threadIdx.x == 0) { nll_d[b] = (double)INFINITY; nll[b] = INFINITY; }
    return;
  }
  const int64_t cell0 = (int64_t)b * Tn * U1;
  const float* pb = lpb + cell0;
  const float* pl = lpl + cell0;
  double* lat = (backward ? beta : alpha) + cell0;
  const int D = Tb + Ub - 1;                    // the last diagonal
  for (int step = 0; step <= D; ++step) {
    const int d = backward ? D - step : step;
    const int ulo = d - (Tb - 1) > 0 ? d - (Tb - 1) : 0, uhi = d < Ub ? d : Ub;
    for (int u = ulo + threadIdx.x; u <= uhi; u += 256) {        // a diagonal longer than the workgroup: strided
      const int t = d - u;
      const int64_t c = (int64_t)t * U1 + u;
      const double ninf = -(double)INFINITY;
      double v;
      if (!backward) {
        const double a0 = t > 0 ? prev[u] + (double)pb[c - U1] : ninf;            // from (t-1, u) by a blank
        const double a1 = u > 0 ? prev[u - 1] + (double)pl[c - 1] : ninf;         // from (t, u-1) by label u
        v = d == 0 ? 0.0 : rnnt_lae(a0, a1);
      } else {
        const double b0 = t + 1 < Tb ? prev[u] + (double)pb[c] : (u == Ub ? (double)pb[c] : ninf);      // beta(T_b, U_b) = 0, every other beta(T_b, u) = -inf
        const double b1 = u < Ub ? prev[u + 1] + (double)pl[c] : ninf;
        v = rnnt_lae(b0, b1);
      }
      cur[u] = v;
      lat[c] = v;
    }
    __syncthreads();
    double* tmp = prev; prev = cur; cur = tmp;
  }
  if (!backward && threadIdx.x == 0) {
    const double v = -(prev[Ub] + (double)pb[(int64_t)(Tb - 1) * U1 + Ub]);
    nll_d[b] = v;
    nll[b] = (float)v;
  }
}

// loss = mean_b nll_b / max(U_b, 1), added in utterance order by one lane and rounded once
__global__ __launch_bounds__(64) void rnnt_finish_kernel(const double* __restrict__ nll_d, const int32_t* __restrict__ tg_len, int B, int Umax,
                                                         float* __restrict__ loss) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const int Ub = clampi(tg_len[b], 0, Umax);
    s += nll_d[b] / (double)(Ub > 1 ? Ub : 1);
  }
  *loss = (float)(s / (double)B);
}

// ------------------------------------------------------------------------------------------------ loss: gradient
// one wave per row, written through GradRow of csrc/loss_rows.h (seq_bwd_kernel's shape, csrc/mwer.hip)
template <typename T, bool BAND>
__global__ __launch_bounds__(64 * RNNT_ROWS) void rnnt_bwd_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ targets,
                                                                  const int32_t* __restrict__ frames, const int32_t* __restrict__ tg_len,
                                                                  int B, int Tn, int Umax, int V, int blank, int64_t rows,
                                                                  const float* __restrict__ lse, const float* __restrict__ lpb,
                                                                  const float* __restrict__ lpl, const double* __restrict__ alpha,
                                                                  const double* __restrict__ beta, const double* __restrict__ nll_d,
                                                                  const float* __restrict__ grad_out, T* __restrict__ dl, int64_t ldd,
                                                                  const int32_t* __restrict__ s_begin, int W) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * RNNT_ROWS + wave;
  if (row >= rows) return;
  const int U1 = Umax + 1;
  int u;
  int64_t bt, cell;
  rnnt_row_map<BAND>(row, U1, W, s_begin, bt, u, cell);
  const int t = (int)(bt % Tn);
  const int b = (int)(bt / Tn);
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  const GradRow<T> out(dl + row * ldd, ldd);
  // everything up to here and the values below are the same in all lanes of the wave (a row per wave)
  float gb = 0.f, gl = 0.f, c = 0.f;
  int ycol = -1;
  bool live = t < Tb && u <= Ub;
  if (live) {
    const double nl = nll_d[b];
    live = nl < (double)INFINITY;
    if (live) {
      const double a = alpha[cell];
      const double bnext = t + 1 < Tb ? beta[cell + U1] : (u == Ub ? 0.0 : -(double)INFINITY);
      gb = (float)exp(a + (double)lpb[cell] + bnext + nl);
      if (u < Ub) {
        ycol = (int)targets[(int64_t)b * Umax + u];
        gl = (float)exp(a + (double)lpl[cell] + beta[cell + 1] + nl);
      }
      c = (grad_out ? grad_out[0] : 1.f) / ((float)(Ub > 1 ? Ub : 1) * (float)B);
    }
  }
  if (!live) {                                 // a dead row, or an utterance without an alignment: zeros, its logits are not read
    out.zero(lane);
    return;
  }
  const float* l = logits + row * ld;
  const float ls = lse[row];
  const float g = gb + gl;
  out.write(l, V, lane, [&](int v, float x) {
    const float sm = expf(x - ls);
    return c * ((g * sm - (v == blank ? gb : 0.f)) - (v == ycol ? gl : 0.f));
  });
}

bool rnnt_rows_ok(int B, int T, int Umax, int64_t* rows) {
  *rows = (int64_t)B * T * (Umax + 1);
  return ceil_div64(*rows, RNNT_ROWS) < ((int64_t)1 << 31);
}

}  // namespace
