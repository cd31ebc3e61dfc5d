// Pruned transducer training (Kuang et al. 2022, arXiv:2206.13236): a cheap "simple" joiner am[b,t,:] + lm[b,u,:] whose
// lattice gives node posteriors, a band of W label positions per frame chosen from them, and the real joiner and loss on that band only.
// Notation of csrc/rnnt.hip: blank = PAD, utterance b has T_b frames and labels y_1 .. y_{U_b}, U1 = Umax + 1.
//
// 1. simple loss   N(t,u)     = log sum_v exp(am[t,v] + lm[u,v]) = (ma[t] + ml[u]) + log(max(dot(t,u), FLT_MIN)),
//                  dot(t,u)   = sum_v Ea[t,v] El[u,v],  Ea = expf(am - ma),  El = expf(lm - ml),  ma / ml the row maxima          (fp32)
//                  blank(t,u) = (am[t,0] + lm[u,0]) - N,   label(t,u) = (am[t,y_{u+1}] + lm[u,y_{u+1}]) - N
//                  nll_b: the lattice of csrc/rnnt_lattice.h on these two arrays (fp64), the edge rules of asr_rnnt_fwd
//                  gb, gl: the arc posteriors of csrc/rnnt.hip;  G(t,u) = (gb + gl)(t,u) / max(dot(t,u), FLT_MIN)
//                  d nll / d am[t,v] = Ea[t,v] sum_u G(t,u) El[u,v] - [v = 0] sum_u gb(t,u) - sum_{u: y_{u+1} = v} gl(t,u)
//                  d nll / d lm[u,v] = El[u,v] sum_t G(t,u) Ea[t,v] - [v = 0] sum_t gb(t,u) - [v = y_{u+1}] sum_t gl(t,u)
//    The floor FLT_MIN is a stated limit, not a feature: the formula is exact while (ma - min am) + (ml - min lm) stays below about 87.
// 2. band          occ(t,u) = gb + gl in fp32; W = min(S, U1).  U_b + 1 <= W: s(t) = 0.  Otherwise fin = U_b + 1 - W and
//                  raw(t) = the lowest a in 0..fin that maximises sum_{u=a}^{a+W-1} occ(t,u) (fp64, ascending u, from +0.0);
//                  s(0) = 0, s(t) = min(max(raw(t), s(t-1)), s(t-1) + W - 1); s(T_b-1) = fin; then for t = T_b-2 .. 0:
//                  s(t) = max(s(t), s(t+1) - (W-1)).  Frames t >= T_b get 0.
// 3. pruned loss   z[b,t,w,:] = tanh(e[b,t] + p[b, s(t) + w]), logits (B,T,W,V) = rnnt_out(z), and the lattice of csrc/rnnt.hip with
//                  blank(t,u) = label(t,u) = -inf for every node outside s(t) <= u < s(t) + W: a node outside the band has no outgoing
//                  arc, so an arc that leads out of the band carries no mass.  No complete path inside the band: nll_b = +inf, zero rows.
//
// The three T x U1 x V contractions (dot = Ea El^T, K = V; G El, K = U1; G^T Ea, K = T) run on v_mfma_f32_32x32x2_f32 from LDS tiles: ONE
// templated tile core (rnnt_contract_kernel) with a k-major / k-minor switch per operand and an epilogue switch.  The f32 MFMA is an
// fmaf chain in k order, so a result is a function of the inputs alone.  No atomics anywhere; repeated labels (y = 3,3,3) are added to
// their column by ONE thread in u order.  All offsets into am / lm / logits / z are 64 bit.
#include <cfloat>

#include "rnnt_lattice.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int CT_MN = 64;                      // output tile of a workgroup: 64 x 64, a 32 x 32 MFMA tile per wave
constexpr int CT_K = 16;                       // K per LDS stage: 8 MFMAs per wave and stage
constexpr int CT_LD = CT_MN + 4;               // LDS row stride in floats

// ------------------------------------------------------------------------------------------------ simple loss: rows
// one wave per row of am (rows 0 .. B T - 1) or lm (the rest): the row maximum and E = expf(x - max); a dead row (t >= T_b, u > U_b) is
// not read and leaves zeros, so it adds nothing to any contraction
__global__ __launch_bounds__(64 * RNNT_ROWS) void simple_rows_kernel(const float* __restrict__ am, int64_t lda, const float* __restrict__ lm,
                                                                     int64_t ldl, const int32_t* __restrict__ frames,
                                                                     const int32_t* __restrict__ tg_len, int B, int Tn, int Umax, int V,
                                                                     float* __restrict__ ma, float* __restrict__ ml, float* __restrict__ Ea,
                                                                     float* __restrict__ El) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int U1 = Umax + 1;
  const int64_t nA = (int64_t)B * Tn, rows = nA + (int64_t)B * U1;
  const int64_t row = (int64_t)blockIdx.x * RNNT_ROWS + wave;
  if (row >= rows) return;
  const bool isA = row < nA;
  const int64_t r = isA ? row : row - nA;
  const int b = (int)(r / (isA ? Tn : U1)), i = (int)(r % (isA ? Tn : U1));
  const bool live = isA ? i < clampi(frames[b], 0, Tn) : i <= clampi(tg_len[b], 0, Umax);
  const float* x = isA ? am + r * lda : lm + r * ldl;
  float* E = (isA ? Ea : El) + r * V;
  float* mx = (isA ? ma : ml) + r;
  if (!live) {
    for (int v = lane; v < V; v += 64) E[v] = 0.f;
    if (lane == 0) *mx = 0.f;
    return;
  }
  float m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  for (int v = lane; v < V; v += 64) E[v] = expf(x[v] - m);
  if (lane == 0) *mx = m;
}

// ------------------------------------------------------------------------------------------------ the contraction core
// KMAJOR: the operand is stored (K x X) row-major (x contiguous), else (X x K) row-major (k contiguous).  Out of range: zero.
template <bool KMAJOR>
__device__ __forceinline__ void ct_load(float (*S)[CT_LD], const float* __restrict__ g, int64_t ldg, int x0, int X, int k0, int K, int tid) {
#pragma unroll
  for (int r = 0; r < (CT_MN * CT_K) / 256; ++r) {
    const int idx = tid + 256 * r;
    int x, k;
    if constexpr (KMAJOR) { x = idx % CT_MN; k = idx / CT_MN; }
    else { k = idx % CT_K; x = idx / CT_K; }
    const int gx = x0 + x, gk = k0 + k;
    float v = 0.f;
    if (gx < X && gk < K) v = KMAJOR ? g[(int64_t)gk * ldg + gx] : g[(int64_t)gx * ldg + gk];
    S[k][x] = v;
  }
}

// C[b] (M x N) = A[b] (M x K) B[b] (K x N), grid (ceil(N / 64), ceil(M / 64), batch), 256 threads.  Lane l of a wave hands the MFMA
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; accumulator r is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
// EPI 0: C = acc.  EPI 1: C = c_b (E * acc) with E laid out as C and c_b = grad_out / (B max(U_b, 1)): the gradient of the simple loss
// before its one-hot terms.
template <bool AK, bool BK, int EPI>
__global__ __launch_bounds__(256) void rnnt_contract_kernel(const float* __restrict__ A, int64_t lda, int64_t strideA,
                                                            const float* __restrict__ Bm, int64_t ldb, int64_t strideB, float* __restrict__ C,
                                                            int64_t ldc, int64_t strideC, int M, int N, int K, const float* __restrict__ E,
                                                            const int32_t* __restrict__ tg_len, int Umax, int Bn,
                                                            const float* __restrict__ grad_out) {
  __shared__ float As[CT_K][CT_LD];
  __shared__ float Bs[CT_K][CT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.z;
  const int m0 = blockIdx.y * CT_MN, n0 = blockIdx.x * CT_MN;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const float* Ab = A + b * strideA;
  const float* Bb = Bm + b * strideB;
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += CT_K) {
    ct_load<AK>(As, Ab, lda, m0, M, k0, K, tid);
    ct_load<BK>(Bs, Bb, ldb, n0, N, k0, K, tid);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < CT_K; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + (lane >> 5)][wm + (lane & 31)], Bs[kk + (lane >> 5)][wn + (lane & 31)], acc, 0, 0, 0);
    __syncthreads();
  }
  float c = 0.f;
  if constexpr (EPI == 1) {
    const int Ub = clampi(tg_len[b], 0, Umax);
    c = (grad_out ? grad_out[0] : 1.f) / ((float)(Ub > 1 ? Ub : 1) * (float)Bn);
  }
  const int j = n0 + wn + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (i < M && j < N) {
      const int64_t o = b * strideC + (int64_t)i * ldc + j;
      if constexpr (EPI == 0) C[o] = acc[r];
      else C[o] = c * (E[o] * fminf(acc[r], FLT_MAX));          // past the stated limit a sum of G may overflow: 0 * inf is not a number
    }
  }
}

// ------------------------------------------------------------------------------------------------ simple loss: cells
// one thread per cell: the log-normaliser from the contraction and the two log-probabilities the lattice needs; a dead cell writes nothing
__global__ __launch_bounds__(256) void simple_cell_kernel(const float* __restrict__ am, int64_t lda, const float* __restrict__ lm, int64_t ldl,
                                                          const int64_t* __restrict__ targets, const int32_t* __restrict__ frames,
                                                          const int32_t* __restrict__ tg_len, int Tn, int Umax, int V, int blank, int64_t cells,
                                                          const float* __restrict__ ma, const float* __restrict__ ml,
                                                          const float* __restrict__ dot, float* __restrict__ lpb, float* __restrict__ lpl) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const int U1 = Umax + 1;
  const int u = (int)(cell % U1);
  const int64_t bt = cell / U1;
  const int t = (int)(bt % Tn);
  const int64_t b = bt / Tn;
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  if (t >= Tb || u > Ub) return;
  const float* a = am + bt * lda;
  const float* l = lm + (b * U1 + u) * ldl;
  const float n = (ma[bt] + ml[b * U1 + u]) + logf(fmaxf(dot[cell], FLT_MIN));
  lpb[cell] = (a[blank] + l[blank]) - n;
  float ll = -INFINITY;
  if (u < Ub) {
    const int64_t y = targets[b * Umax + u];
    if (y >= 0 && y < V && y != blank) ll = (a[y] + l[y]) - n;
  }
  lpl[cell] = ll;
}

// one thread per cell: the arc posteriors gb, gl of csrc/rnnt.hip (the same fp64 exponents) and G = (gb + gl) / max(dot, FLT_MIN); zeros in
// every dead cell and in an utterance without an alignment
__global__ __launch_bounds__(256) void simple_occ_kernel(const int32_t* __restrict__ frames, const int32_t* __restrict__ tg_len, int Tn, int Umax,
                                                         int64_t cells, const float* __restrict__ lpb, const float* __restrict__ lpl,
                                                         const double* __restrict__ alpha, const double* __restrict__ beta,
                                                         const double* __restrict__ nll_d, const float* __restrict__ dot,
                                                         float* __restrict__ gbo, float* __restrict__ glo, float* __restrict__ G) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= cells) return;
  const int U1 = Umax + 1;
  const int u = (int)(cell % U1);
  const int64_t bt = cell / U1;
  const int t = (int)(bt % Tn);
  const int64_t b = bt / Tn;
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  float gb = 0.f, gl = 0.f, g = 0.f;
  if (t < Tb && u <= Ub) {
    const double nl = nll_d[b];
    if (nl < (double)INFINITY) {
      const double a = alpha[cell];
      const double bnext = t + 1 < Tb ? beta[cell + U1] : (u == Ub ? 0.0 : -(double)INFINITY);
      gb = (float)exp(a + (double)lpb[cell] + bnext + nl);
      if (u < Ub) gl = (float)exp(a + (double)lpl[cell] + beta[cell + 1] + nl);
      g = (gb + gl) / fmaxf(dot[cell], FLT_MIN);
    }
  }
  gbo[cell] = gb;
  glo[cell] = gl;
  G[cell] = g;
}

// the one-hot terms of the simple gradient, one thread per row of d am (rows 0 .. B T - 1) or d lm: ONE owner per row, who subtracts in u
// order (d am: labels may repeat) or adds the column sums in t order (d lm)
__global__ __launch_bounds__(256) void simple_onehot_kernel(const int64_t* __restrict__ targets, const int32_t* __restrict__ frames,
                                                            const int32_t* __restrict__ tg_len, int B, int Tn, int Umax, int V, int blank,
                                                            const float* __restrict__ gb, const float* __restrict__ gl,
                                                            const double* __restrict__ nll_d, const float* __restrict__ grad_out,
                                                            float* __restrict__ dam, float* __restrict__ dlm) {
  const int U1 = Umax + 1;
  const int64_t nA = (int64_t)B * Tn, rows = nA + (int64_t)B * U1;
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const bool isA = row < nA;
  const int64_t r = isA ? row : row - nA;
  const int64_t b = r / (isA ? Tn : U1);
  const int i = (int)(r % (isA ? Tn : U1));
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  if (!(nll_d[b] < (double)INFINITY)) return;                  // no alignment (a label may be out of range): the rows are zero already
  const float c = (grad_out ? grad_out[0] : 1.f) / ((float)(Ub > 1 ? Ub : 1) * (float)B);
  const int64_t* y = targets + b * Umax;
  if (isA) {
    if (i >= Tb) return;
    const float* pb = gb + r * U1;
    const float* pl = gl + r * U1;
    float* d = dam + r * V;
    float sb = 0.f;
    for (int u = 0; u <= Ub; ++u) sb += pb[u];
    d[blank] -= c * sb;
    for (int u = 0; u < Ub; ++u) d[y[u]] -= c * pl[u];
  } else {
    if (i > Ub) return;
    const float* pb = gb + b * Tn * U1 + i;
    const float* pl = gl + b * Tn * U1 + i;
    float* d = dlm + r * V;
    float sb = 0.f, sl = 0.f;
    for (int t = 0; t < Tb; ++t) { sb += pb[(int64_t)t * U1]; sl += pl[(int64_t)t * U1]; }
    d[blank] -= c * sb;
    if (i < Ub) d[y[i]] -= c * sl;
  }
}

// ------------------------------------------------------------------------------------------------ the band
// grid (B), 256 threads: the window sums and the arg max of every frame in parallel, then the two scans by one lane
__global__ __launch_bounds__(256) void prune_ranges_kernel(const float* __restrict__ gb, const float* __restrict__ gl,
                                                           const int32_t* __restrict__ frames, const int32_t* __restrict__ tg_len, int Tn,
                                                           int Umax, int W, int32_t* __restrict__ s_begin) {
  const int64_t b = blockIdx.x;
  const int U1 = Umax + 1;
  const int Tb = clampi(frames[b], 0, Tn), Ub = clampi(tg_len[b], 0, Umax);
  int32_t* s = s_begin + b * Tn;
  const int fin = Ub + 1 - W;
  for (int t = threadIdx.x; t < Tn; t += 256) {
    int best = 0;
    if (t < Tb && fin > 0) {
      const float* pb = gb + (b * Tn + t) * U1;
      const float* pl = gl + (b * Tn + t) * U1;
      double top = -1.0;
      for (int a = 0; a <= fin; ++a) {
        double sum = 0.0;
        for (int u = a; u < a + W; ++u) sum += (double)(pb[u] + pl[u]);          // occ = gb + gl rounded to fp32, then added in fp64
        if (sum > top) { top = sum; best = a; }                                  // the lowest start among equal sums
      }
    }
    s[t] = best;
  }
  __syncthreads();
  if (threadIdx.x != 0 || fin <= 0 || Tb == 0) return;
  int prev = 0;
  s[0] = 0;
  for (int t = 1; t < Tb; ++t) {
    int v = s[t];
    v = v > prev ? v : prev;
    v = v < prev + W - 1 ? v : prev + W - 1;
    s[t] = prev = v;
  }
  s[Tb - 1] = fin;
  int next = fin;
  for (int t = Tb - 2; t >= 0; --t) {
    int v = s[t];
    v = v > next - (W - 1) ? v : next - (W - 1);
    s[t] = next = v;
  }
}

// ------------------------------------------------------------------------------------------------ the banded joint
// one thread per 16-byte chunk of z (B,T,W,J): rnnt_joint_fwd_kernel of csrc/rnnt.hip with the predictor row s_begin[b,t] + w
template <typename T>
__global__ __launch_bounds__(256) void joint_pruned_fwd_kernel(const T* __restrict__ e, const T* __restrict__ p,
                                                               const int32_t* __restrict__ s_begin, T* __restrict__ z, int Tn, int U1, int W,
                                                               int J, int64_t chunks) {
  constexpr int EPC = DT<T>::EPC;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const int JC = J / EPC;
  const int jc = (int)(c % JC);
  const int64_t row = c / JC;                  // (b t) W + w
  const int w = (int)(row % W);
  const int64_t bt = row / W;
  const int64_t b = bt / Tn;
  const int u = clampi(s_begin[bt], 0, U1 - W) + w;
  Chunk<T> ce, cp, cz;
  ce.v = *reinterpret_cast<const uint4*>(e + bt * J + (int64_t)jc * EPC);
  cp.v = *reinterpret_cast<const uint4*>(p + (b * U1 + u) * J + (int64_t)jc * EPC);
#pragma unroll
  for (int i = 0; i < EPC; ++i) cz.e[i] = DT<T>::to(tanhf(DT<T>::from(ce.e[i]) + DT<T>::from(cp.e[i])));
  *reinterpret_cast<uint4*>(z + row * J + (int64_t)jc * EPC) = cz.v;
}

// one thread per element of de (rows 0 .. B T - 1: the sum over w, in w order) or of dp (rows B T ..: the sum over the frames whose window
// holds u, in t order; with a monotone s they form one interval).  fp32 sums, one owner per element.
template <typename T>
__global__ __launch_bounds__(256) void joint_pruned_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                               const int32_t* __restrict__ s_begin, T* __restrict__ de, T* __restrict__ dp, int B,
                                                               int Tn, int U1, int W, int J) {
  const int64_t nE = (int64_t)B * Tn * J, total = nE + (int64_t)B * U1 * J;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  if (idx < nE) {
    const int64_t bt = idx / J;
    const int col = (int)(idx % J);
    const int64_t base = bt * W * J + col;
    float acc = 0.f;
    for (int w = 0; w < W; ++w) {
      const float zz = DT<T>::ld(z + base + (int64_t)w * J);
      acc += DT<T>::ld(dz + base + (int64_t)w * J) * (1.f - zz * zz);
    }
    DT<T>::st(de + idx, acc);
  } else {
    const int64_t r = idx - nE;
    const int col = (int)(r % J);
    const int64_t bu = r / J;
    const int u = (int)(bu % U1);
    const int64_t b = bu / U1;
    const int32_t* s = s_begin + b * Tn;
    float acc = 0.f;
    for (int t = 0; t < Tn; ++t) {
      const int w = u - clampi(s[t], 0, U1 - W);
      if (w < 0 || w >= W) continue;
      const int64_t o = ((b * Tn + t) * W + w) * J + col;
      const float zz = DT<T>::ld(z + o);
      acc += DT<T>::ld(dz + o) * (1.f - zz * zz);
    }
    DT<T>::st(dp + r, acc);
  }
}

// ------------------------------------------------------------------------------------------------ pruned loss
__global__ __launch_bounds__(256) void fill_ninf_kernel(float* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = -INFINITY;
}

bool grid_ok(int64_t blocks) { return blocks < ((int64_t)1 << 31); }

struct SimpleWs {                              // the simple loss' workspace, in floats from an 8-byte aligned base
  double *alpha, *beta, *nll_d;
  float *lpb, *lpl, *gb, *gl, *dot, *G, *ma, *ml, *Ea, *El, *nll;
  SimpleWs(float* ws, int B, int T, int Umax, int V) {
    const int64_t cells = (int64_t)B * T * (Umax + 1);
    alpha = reinterpret_cast<double*>(ws);
    beta = alpha + cells;
    nll_d = beta + cells;
    lpb = reinterpret_cast<float*>(nll_d + B);
    lpl = lpb + cells;
    gb = lpl + cells;
    gl = gb + cells;
    dot = gl + cells;
    G = dot + cells;
    ma = G + cells;
    ml = ma + (int64_t)B * T;
    Ea = ml + (int64_t)B * (Umax + 1);
    El = Ea + (int64_t)B * T * V;
    nll = El + (int64_t)B * (Umax + 1) * V;
  }
};

}  // namespace

extern "C" int64_t asr_rnnt_simple_workspace(int B, int T, int Umax, int V) {
  if (B <= 0 || T <= 0 || Umax < 0 || V <= 0) return 0;
  // alpha | beta | nll (fp64, two floats each), then fp32: blank | label log-prob | gb | gl | dot | G (B T U1 each) | ma (B T) | ml (B U1) |
  // Ea (B T V) | El (B U1 V) | nll (B)
  const int64_t U1 = Umax + 1;
  return 10 * (int64_t)B * T * U1 + 3 * (int64_t)B + (int64_t)B * (T + U1) * (1 + (int64_t)V);
}

extern "C" int asr_rnnt_simple_fwd(const float* am, int64_t lda, const float* lm, int64_t ldl, const int64_t* targets,
                                   const int32_t* frame_lengths, const int32_t* target_lengths, int B, int T, int Umax, int V, int blank,
                                   float* workspace, int64_t workspace_floats, float* loss, hipStream_t s) {
  ASR_CHECK_ARG(am && lm && frame_lengths && target_lengths && workspace && loss && (Umax == 0 || targets));
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Umax >= 0 && lda >= V && ldl >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG(workspace_floats >= asr_rnnt_simple_workspace(B, T, Umax, V) && aligned8(workspace));
  const int U1 = Umax + 1;
  const int64_t cells = (int64_t)B * T * U1, rows = (int64_t)B * (T + U1);
  const size_t lds = (size_t)2 * U1 * sizeof(double);
  if (lds > 64 * 1024 || B > 65535 || ceil_div64(T, CT_MN) > 65535 || !grid_ok(ceil_div64(cells, 256))) return ASR_EUNSUPPORTED;
  const SimpleWs w(workspace, B, T, Umax, V);
  AsrProfScope prof(ASR_OP_CE, s);
  ASR_TRY(asr_launch<simple_rows_kernel>(dim3((unsigned)ceil_div64(rows, RNNT_ROWS)), dim3(64 * RNNT_ROWS), 0, s, am, lda, lm, ldl, frame_lengths,
                                         target_lengths, B, T, Umax, V, w.ma, w.ml, w.Ea, w.El));
  ASR_TRY(asr_launch<rnnt_contract_kernel<false, false, 0>>(dim3((U1 + CT_MN - 1) / CT_MN, (T + CT_MN - 1) / CT_MN, B), dim3(256), 0, s, w.Ea,
                                                            (int64_t)V, (int64_t)T * V, w.El, (int64_t)V, (int64_t)U1 * V, w.dot, (int64_t)U1,
                                                            (int64_t)T * U1, T, U1, V, (const float*)nullptr, (const int32_t*)nullptr, 0, B, (const float*)nullptr));
  ASR_TRY(asr_launch<simple_cell_kernel>(dim3((unsigned)ceil_div64(cells, 256)), dim3(256), 0, s, am, lda, lm, ldl, targets, frame_lengths,
                                         target_lengths, T, Umax, V, blank, cells, w.ma, w.ml, w.dot, w.lpb, w.lpl));
  // (64 KB at once, as asr_rnnt_fwd)
  if (lds > 48 * 1024) (void)asr_grant_lds<rnnt_lattice_kernel>(64 * 1024);
  ASR_TRY(asr_launch<rnnt_lattice_kernel>(dim3(B, 2), dim3(256), lds, s, targets, frame_lengths, target_lengths, T, Umax, V, blank, w.lpb, w.lpl,
                                          w.alpha, w.beta, w.nll_d, w.nll));
  ASR_TRY(asr_launch<rnnt_finish_kernel>(dim3(1), dim3(64), 0, s, w.nll_d, target_lengths, B, Umax, loss));
  return asr_launch<simple_occ_kernel>(dim3((unsigned)ceil_div64(cells, 256)), dim3(256), 0, s, frame_lengths, target_lengths, T, Umax, cells,
                                       w.lpb, w.lpl, w.alpha, w.beta, w.nll_d, w.dot, w.gb, w.gl, w.G);
}

extern "C" int asr_rnnt_simple_bwd(const int64_t* targets, const int32_t* frame_lengths, const int32_t* target_lengths, int B, int T, int Umax,
                                   int V, int blank, const float* workspace, const float* grad_out, float* dam, float* dlm, hipStream_t s) {
  ASR_CHECK_ARG(frame_lengths && target_lengths && workspace && dam && dlm && (Umax == 0 || targets));
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Umax >= 0 && blank >= 0 && blank < V && aligned8(workspace));
  const int U1 = Umax + 1;
  const int64_t rows = (int64_t)B * (T + U1);
  if (B > 65535 || ceil_div64(T, CT_MN) > 65535 || ceil_div64(U1, CT_MN) > 65535) return ASR_EUNSUPPORTED;
  const SimpleWs w(const_cast<float*>(workspace), B, T, Umax, V);
  AsrProfScope prof(ASR_OP_CE, s);
  const unsigned nt = (V + CT_MN - 1) / CT_MN;
  // d am (B,T,V) = c Ea (G El): A = G (T x U1, k minor), B = El (U1 x V, k major)
  ASR_TRY(asr_launch<rnnt_contract_kernel<false, true, 1>>(dim3(nt, (T + CT_MN - 1) / CT_MN, B), dim3(256), 0, s, w.G, (int64_t)U1, (int64_t)T * U1,
                                                           w.El, (int64_t)V, (int64_t)U1 * V, dam, (int64_t)V, (int64_t)T * V, T, V, U1, w.Ea,
                                                           target_lengths, Umax, B, grad_out));
  // d lm (B,U1,V) = c El (G^T Ea): A = G (stored T x U1: k major), B = Ea (T x V, k major)
  ASR_TRY(asr_launch<rnnt_contract_kernel<true, true, 1>>(dim3(nt, (U1 + CT_MN - 1) / CT_MN, B), dim3(256), 0, s, w.G, (int64_t)U1, (int64_t)T * U1,
                                                          w.Ea, (int64_t)V, (int64_t)T * V, dlm, (int64_t)V, (int64_t)U1 * V, U1, V, T, w.El,
                                                          target_lengths, Umax, B, grad_out));
  return asr_launch<simple_onehot_kernel>(dim3((unsigned)ceil_div64(rows, 256)), dim3(256), 0, s, targets, frame_lengths, target_lengths, B, T,
                                          Umax, V, blank, w.gb, w.gl, w.nll_d, grad_out, dam, dlm);
}

extern "C" int asr_rnnt_prune_ranges(const float* gb, const float* gl, const int32_t* frame_lengths, const int32_t* target_lengths, int B,
                                     int T, int Umax, int S, int32_t* s_begin, hipStream_t s) {
  ASR_CHECK_ARG(gb && gl && frame_lengths && target_lengths && s_begin && B > 0 && T > 0 && Umax >= 0 && S >= 1);
  const int W = S < Umax + 1 ? S : Umax + 1;
  return asr_launch<prune_ranges_kernel>(dim3(B), dim3(256), 0, s, gb, gl, frame_lengths, target_lengths, T, Umax, W, s_begin);
}

extern "C" int asr_rnnt_joint_pruned_fwd(const void* e, const void* p, const int32_t* s_begin, void* z, int B, int T, int U1, int W, int J,
                                         int dtype, hipStream_t s) {
  ASR_CHECK_ARG(e && p && s_begin && z && B > 0 && T > 0 && U1 > 0 && W > 0 && W <= U1 && J > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (J % 8 != 0 || !aligned16(e) || !aligned16(p) || !aligned16(z)) return ASR_EUNSUPPORTED;      // whole 16-byte chunks in both dtypes
  return asr_with_dtype(dtype, [&](auto tag) {
    using E = decltype(tag);
    const int64_t chunks = (int64_t)B * T * W * (J / DT<E>::EPC);
    if (!grid_ok(ceil_div64(chunks, 256))) return (int)ASR_EUNSUPPORTED;
    return asr_launch<joint_pruned_fwd_kernel<E>>(dim3((unsigned)ceil_div64(chunks, 256)), dim3(256), 0, s, (const E*)e, (const E*)p, s_begin,
                                                  (E*)z, T, U1, W, J, chunks);
  });
}

extern "C" int asr_rnnt_joint_pruned_bwd(const void* dz, const void* z, const int32_t* s_begin, void* de, void* dp, int B, int T, int U1, int W,
                                         int J, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(dz && z && s_begin && de && dp && B > 0 && T > 0 && U1 > 0 && W > 0 && W <= U1 && J > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  const int64_t total = (int64_t)B * (T + U1) * J;
  if (!grid_ok(ceil_div64(total, 256))) return ASR_EUNSUPPORTED;
  return asr_with_dtype(dtype, [&](auto tag) {
    using E = decltype(tag);
    return asr_launch<joint_pruned_bwd_kernel<E>>(dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, s, (const E*)dz, (const E*)z, s_begin,
                                                  (E*)de, (E*)dp, B, T, U1, W, J);
  });
}

extern "C" int64_t asr_rnnt_pruned_workspace(int B, int T, int Umax, int W) {
  if (B <= 0 || T <= 0 || Umax < 0 || W <= 0 || W > Umax + 1) return 0;
  // alpha | beta | nll, all fp64 (two floats each), then fp32: row lse (B T W) | blank log-prob | label log-prob (B T U1 each) | nll:
  // asr_rnnt_workspace's layout when W = Umax + 1
  return 6 * (int64_t)B * T * (Umax + 1) + (int64_t)B * T * W + 3 * (int64_t)B;
}

extern "C" int asr_rnnt_pruned_fwd(const float* logits, int64_t ld, const int64_t* targets, const int32_t* frame_lengths,
                                   const int32_t* target_lengths, const int32_t* s_begin, int B, int T, int Umax, int W, int V, int blank,
                                   float* workspace, int64_t workspace_floats, float* loss, hipStream_t s) {
  ASR_CHECK_ARG(logits && frame_lengths && target_lengths && s_begin && workspace && loss && (Umax == 0 || targets));
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Umax >= 0 && W > 0 && W <= Umax + 1 && ld >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG(workspace_floats >= asr_rnnt_pruned_workspace(B, T, Umax, W) && aligned8(workspace));
  int64_t cells;
  if (!rnnt_rows_ok(B, T, Umax, &cells)) return ASR_EUNSUPPORTED;
  const int64_t rows = (int64_t)B * T * W;
  const size_t lds = (size_t)2 * (Umax + 1) * sizeof(double);
  if (lds > 64 * 1024 || !grid_ok(ceil_div64(2 * cells, 256))) return ASR_EUNSUPPORTED;
  double* alpha = reinterpret_cast<double*>(workspace);
  double* beta = alpha + cells;
  double* nll_d = beta + cells;
  float* lse = reinterpret_cast<float*>(nll_d + B);
  float* lpb = lse + rows;
  float* lpl = lpb + cells;
  float* nll = lpl + cells;
  AsrProfScope prof(ASR_OP_CE, s);
  ASR_TRY(asr_launch<fill_ninf_kernel>(dim3((unsigned)ceil_div64(2 * cells, 256)), dim3(256), 0, s, lpb, 2 * cells));
  ASR_TRY(asr_launch<rnnt_row_kernel<true>>(dim3((unsigned)ceil_div64(rows, RNNT_ROWS)), dim3(64 * RNNT_ROWS), 0, s, logits, ld, targets,
                                            frame_lengths, target_lengths, T, Umax, V, blank, rows, lse, lpb, lpl, s_begin, W));
  // (64 KB at once, as asr_rnnt_fwd)
  if (lds > 48 * 1024) (void)asr_grant_lds<rnnt_lattice_kernel>(64 * 1024);
  ASR_TRY(asr_launch<rnnt_lattice_kernel>(dim3(B, 2), dim3(256), lds, s, targets, frame_lengths, target_lengths, T, Umax, V, blank, lpb, lpl,
                                          alpha, beta, nll_d, nll));
  return asr_launch<rnnt_finish_kernel>(dim3(1), dim3(64), 0, s, nll_d, target_lengths, B, Umax, loss);
}

extern "C" int asr_rnnt_pruned_bwd(const float* logits, int64_t ld, const int64_t* targets, const int32_t* frame_lengths,
                                   const int32_t* target_lengths, const int32_t* s_begin, int B, int T, int Umax, int W, int V, int blank,
                                   const float* workspace, const float* grad_out, void* dlogits, int64_t ldd, int out_dtype, hipStream_t s) {
  ASR_CHECK_ARG(logits && frame_lengths && target_lengths && s_begin && workspace && dlogits && (Umax == 0 || targets));
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Umax >= 0 && W > 0 && W <= Umax + 1 && ld >= V && ldd >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG((out_dtype == ASR_F32 || out_dtype == ASR_BF16) && aligned8(workspace));
  int64_t cells;
  if (!rnnt_rows_ok(B, T, Umax, &cells)) return ASR_EUNSUPPORTED;
  const int64_t rows = (int64_t)B * T * W;
  const double* alpha = reinterpret_cast<const double*>(workspace);
  const double* beta = alpha + cells;
  const double* nll_d = beta + cells;
  const float* lse = reinterpret_cast<const float*>(nll_d + B);
  const float* lpb = lse + rows;
  const float* lpl = lpb + cells;
  const dim3 grid((unsigned)ceil_div64(rows, RNNT_ROWS)), block(64 * RNNT_ROWS);
  AsrProfScope prof(ASR_OP_CE, s);
  return asr_with_dtype(out_dtype, [&](auto tag) {
    using E = decltype(tag);
    return asr_launch<rnnt_bwd_kernel<E, true>>(grid, block, 0, s, logits, ld, targets, frame_lengths, target_lengths, B, T, Umax, V, blank, rows,
                                                lse, lpb, lpl, alpha, beta, nll_d, grad_out, (E*)dlogits, ldd, s_begin, W);
  });
}
