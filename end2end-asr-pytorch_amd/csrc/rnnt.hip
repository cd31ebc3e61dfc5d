// Transducer (RNN-T, Graves 2012) head: the joint's elementwise part, the loss over the T x (U + 1) lattice and its gradient with respect to
// the LOGITS, log-softmax included.  Blank = PAD.  Utterance b has T_b live frames and U_b labels y_1 .. y_U:
//
//   z[b,t,u,:]   = tanh(e[b,t,:] + p[b,u,:])                                            asr_rnnt_joint_fwd
//   de[b,t,:]    = sum_u dz (1 - z^2),   dp[b,u,:] = sum_t dz (1 - z^2)                 asr_rnnt_joint_bwd
//   blank(t,u)   = logits[b,t,u,blank] - lse(t,u),   label(t,u) = logits[b,t,u,y_{u+1}] - lse(t,u)
//   alpha(t,u)   = logaddexp(alpha(t-1,u) + blank(t-1,u), alpha(t,u-1) + label(t,u-1)),   alpha(0,0) = 0
//   beta(t,u)    = logaddexp(beta(t+1,u) + blank(t,u), beta(t,u+1) + label(t,u)),         beta(T_b,U_b) = 0, every other beta(T_b,u) = -inf
//   nll_b        = -(alpha(T_b-1,U_b) + blank(T_b-1,U_b)),   loss = mean_b nll_b / max(U_b, 1)   (the reduction of the CTC term, csrc/ctc.hip)
//   gb = exp(alpha(t,u) + blank(t,u) + beta(t+1,u) + nll_b),   gl = exp(alpha(t,u) + label(t,u) + beta(t,u+1) + nll_b)
//   d nll_b / d logits[b,t,u,v] = (gb + gl) softmax_v - gb [v == blank] - gl [v == y_{u+1}]
//
// Cells with t >= T_b or u > U_b are dead: their logits are never read, their gradient rows are zero.  T_b = 0, or a label among y_1 .. y_U
// that is the blank or lies outside [0,V): nll_b = +inf and the utterance's gradient rows are zero, the other utterances are untouched.
//
// asr_rnnt_fwd is three launches, as asr_ctc_fwd: a row pass (one wave per live row, the row read ONCE: lse_row of csrc/lse.h), the lattice
// (one workgroup per (utterance, direction) walking anti-diagonals d = t + u, whose cells are independent: one barrier per diagonal, the
// previous diagonal in LDS, the whole lattice in the caller's workspace for the backward) and a finish that adds the B terms in utterance
// order.  asr_rnnt_bwd is ONE launch, one wave per row, every lane writing the columns it read: one owner per element.  No atomics
// anywhere: every output is a function of the inputs alone.  All indices into logits / dlogits / z are 64 bit.
// Precision: rows (log-sum-exp, log-probabilities, softmax) are fp32 like every other loss kernel here.  The lattice, log Z and the two
// exponents of gb / gl are fp64: alpha + beta is a sum of terms as large as |log Z| (40 for a dozen frames, hundreds at the workload)
// whose result is near 0, and in fp32 each such term carries half an ulp of ITS size -- 1e-5 of relative error in every gradient row,
// ten times what autograd through an fp32 logaddexp lattice leaves (tests/test_gpu_rnnt_model.py holds the step to 4x the latter).
// The lattice is latency bound (one dependent step per diagonal), so the wider arithmetic costs no time that shows.
#include "rnnt_lattice.h"    // the row pass, the lattice, the finish and the gradient (shared with csrc/rnnt_pruned.hip)

namespace {

constexpr int RNNT_JB_COLS = 64;               // columns of J per workgroup of the joint backward (one per lane)
constexpr int RNNT_JB_UC = 32;                 // label positions whose dp partials a workgroup holds in LDS at once: 4 x 32 x 64 floats = 32 KB

// ------------------------------------------------------------------------------------------------ joint
// one thread per 16-byte chunk of z: the sum and the tanh in fp32, rounded once to the storage type
template <typename T>
__global__ __launch_bounds__(256) void rnnt_joint_fwd_kernel(const T* __restrict__ e, const T* __restrict__ p, T* __restrict__ z, int Tn,
                                                             int U1, int J, int64_t chunks) {
  constexpr int EPC = DT<T>::EPC;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const int JC = J / EPC;
  const int jc = (int)(c % JC);
  const int64_t row = c / JC;                  // (b t) U1 + u
  const int u = (int)(row % U1);
  const int64_t bt = row / U1;
  const int64_t b = bt / Tn;
  Chunk<T> ce, cp, cz;
  ce.v = *reinterpret_cast<const uint4*>(e + bt * J + (int64_t)jc * EPC);
  cp.v = *reinterpret_cast<const uint4*>(p + (b * U1 + u) * J + (int64_t)jc * EPC);
#pragma unroll
  for (int i = 0; i < EPC; ++i) cz.e[i] = DT<T>::to(tanhf(DT<T>::from(ce.e[i]) + DT<T>::from(cp.e[i])));
  *reinterpret_cast<uint4*>(z + row * J + (int64_t)jc * EPC) = cz.v;
}

// grid (ceil(J / 64), B), 256 threads = 4 waves x 64 columns.  Wave w walks frames t = w, w + 4, ...; a lane owns one column.  de[b,t,c] is
// that lane's running sum over u (one owner, u order).  dp[b,u,c]: every wave keeps a partial over ITS frames in LDS (one owner per slot,
// t order), and after the walk the four partials are added in wave order.  U + 1 is taken in pieces of RNNT_JB_UC positions so the LDS
// need does not grow with U; from the second piece on the owner of de adds to what it wrote itself.  dz and z are read once.
template <typename T>
__global__ __launch_bounds__(256) void rnnt_joint_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ z, T* __restrict__ de,
                                                             T* __restrict__ dp, float* __restrict__ de_acc, int Tn, int U1, int J) {
  __shared__ float part[4][RNNT_JB_UC][RNNT_JB_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * RNNT_JB_COLS + lane;
  const int64_t b = blockIdx.y;
  const bool live = col < J;
  for (int u0 = 0; u0 < U1; u0 += RNNT_JB_UC) {
    const int un = min(RNNT_JB_UC, U1 - u0);
    for (int i = 0; i < un; ++i) part[wave][i][lane] = 0.f;
    for (int t = wave; t < Tn; t += 4) {
      const int64_t base = ((b * Tn + t) * U1 + u0) * J + col;
      float acc = 0.f;
      if (live) {
        if (u0 > 0) acc = de_acc[(b * Tn + t) * J + col];
        int i = 0;
        for (; i + 8 <= un; i += 8) {          // eight positions' loads in flight; the additions stay in u order
          float zz[8], dd[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            zz[k] = DT<T>::ld(z + base + (int64_t)(i + k) * J);
            dd[k] = DT<T>::ld(dz + base + (int64_t)(i + k) * J);
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float g = dd[k] * (1.f - zz[k] * zz[k]);
            acc += g;
            part[wave][i + k][lane] += g;
          }
        }
        for (; i < un; ++i) {
          const float zz = DT<T>::ld(z + base + (int64_t)i * J);
          const float g = DT<T>::ld(dz + base + (int64_t)i * J) * (1.f - zz * zz);
          acc += g;
          part[wave][i][lane] += g;
        }
        if (u0 + un < U1) de_acc[(b * Tn + t) * J + col] = acc;        // more pieces follow: the fp32 running sum waits in the workspace
        else DT<T>::st(de + (b * Tn + t) * J + col, acc);
      }
    }
    __syncthreads();
    for (int i = wave; i < un; i += 4)
      if (live) DT<T>::st(dp + (b * U1 + u0 + i) * J + col, ((part[0][i][lane] + part[1][i][lane]) + part[2][i][lane]) + part[3][i][lane]);
    __syncthreads();
  }
}

}  // namespace

extern "C" int asr_rnnt_joint_fwd(const void* e, const void* p, void* z, int B, int T, int U1, int J, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(e && p && z && B > 0 && T > 0 && U1 > 0 && J > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (J % 8 != 0 || !aligned16(e) || !aligned16(p) || !aligned16(z)) return ASR_EUNSUPPORTED;      // whole 16-byte chunks in both dtypes
  return asr_with_dtype(dtype, [&](auto tag) {
    using E = decltype(tag);
    const int64_t chunks = (int64_t)B * T * U1 * (J / DT<E>::EPC);
    if (ceil_div64(chunks, 256) >= ((int64_t)1 << 31)) return (int)ASR_EUNSUPPORTED;
    return asr_launch<rnnt_joint_fwd_kernel<E>>(dim3((unsigned)ceil_div64(chunks, 256)), dim3(256), 0, s, (const E*)e, (const E*)p, (E*)z, T, U1,
                                                J, chunks);
  });
}

extern "C" int64_t asr_rnnt_joint_bwd_workspace(int B, int T, int U1, int J) {
  if (B <= 0 || T <= 0 || U1 <= RNNT_JB_UC || J <= 0) return 0;
  return (int64_t)B * T * J;
}

extern "C" int asr_rnnt_joint_bwd(const void* dz, const void* z, void* de, void* dp, float* workspace, int64_t workspace_floats, int B, int T,
                                  int U1, int J, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(dz && z && de && dp && B > 0 && T > 0 && U1 > 0 && J > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  const int64_t need = asr_rnnt_joint_bwd_workspace(B, T, U1, J);
  ASR_CHECK_ARG(need == 0 || (workspace && workspace_floats >= need));
  if (B > 65535) return ASR_EUNSUPPORTED;
  return asr_with_dtype(dtype, [&](auto tag) {
    using E = decltype(tag);
    return asr_launch<rnnt_joint_bwd_kernel<E>>(dim3((J + RNNT_JB_COLS - 1) / RNNT_JB_COLS, B), dim3(256), 0, s, (const E*)dz, (const E*)z,
                                                (E*)de, (E*)dp, workspace, T, U1, J);
  });
}

extern "C" int64_t asr_rnnt_workspace(int B, int T, int Umax) {
  if (B <= 0 || T <= 0 || Umax < 0) return 0;
  // alpha | beta | nll, all fp64 (two floats each), then fp32: row lse | blank log-prob | label log-prob | nll
  return 7 * (int64_t)B * T * (Umax + 1) + 3 * (int64_t)B;
}

extern "C" int asr_rnnt_fwd(const float* logits, int64_t ld, const int64_t* targets, const int32_t* frame_lengths,
                            const int32_t* target_lengths, int B, int T, int Umax, int V, int blank, float* workspace,
                            int64_t workspace_floats, float* loss, hipStream_t s) {
  ASR_CHECK_ARG(logits && frame_lengths && target_lengths && workspace && loss && (Umax == 0 || targets));
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Umax >= 0 && ld >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG(workspace_floats >= asr_rnnt_workspace(B, T, Umax) && aligned8(workspace));
  int64_t rows;
  if (!rnnt_rows_ok(B, T, Umax, &rows)) return ASR_EUNSUPPORTED;
  const size_t lds = (size_t)2 * (Umax + 1) * sizeof(double);
  if (lds > 64 * 1024) return ASR_EUNSUPPORTED;
  double* alpha = reinterpret_cast<double*>(workspace);
  double* beta = alpha + rows;
  double* nll_d = beta + rows;
  float* lse = reinterpret_cast<float*>(nll_d + B);
  float* lpb = lse + rows;
  float* lpl = lpb + rows;
  float* nll = lpl + rows;
  AsrProfScope prof(ASR_OP_CE, s);
  ASR_TRY(asr_launch<rnnt_row_kernel<false>>(dim3((unsigned)ceil_div64(rows, RNNT_ROWS)), dim3(64 * RNNT_ROWS), 0, s, logits, ld, targets, frame_lengths,
                                             target_lengths, T, Umax, V, blank, rows, lse, lpb, lpl, (const int32_t*)nullptr, Umax + 1));
  // the whole 64 KB at the first need (asr_launch would grant `lds`): a later batch with a longer U then asks for no second grant, which
  // must not run inside a stream capture
  if (lds > 48 * 1024) (void)asr_grant_lds<rnnt_lattice_kernel>(64 * 1024);
  ASR_TRY(asr_launch<rnnt_lattice_kernel>(dim3(B, 2), dim3(256), lds, s, targets, frame_lengths, target_lengths, T, Umax, V, blank, lpb, lpl,
                                          alpha, beta, nll_d, nll));
  return asr_launch<rnnt_finish_kernel>(dim3(1), dim3(64), 0, s, nll_d, target_lengths, B, Umax, loss);
}

extern "C" int asr_rnnt_bwd(const float* logits, int64_t ld, const int64_t* targets, const int32_t* frame_lengths,
                            const int32_t* target_lengths, int B, int T, int Umax, int V, int blank, const float* workspace,
                            const float* grad_out, void* dlogits, int64_t ldd, int out_dtype, hipStream_t s) {
  ASR_CHECK_ARG(logits && frame_lengths && target_lengths && workspace && dlogits && (Umax == 0 || targets));
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Umax >= 0 && ld >= V && ldd >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG((out_dtype == ASR_F32 || out_dtype == ASR_BF16) && aligned8(workspace));
  int64_t rows;
  if (!rnnt_rows_ok(B, T, Umax, &rows)) return ASR_EUNSUPPORTED;
  const double* alpha = reinterpret_cast<const double*>(workspace);
  const double* beta = alpha + rows;
  const double* nll_d = beta + rows;
  const float* lse = reinterpret_cast<const float*>(nll_d + B);
  const float* lpb = lse + rows;
  const float* lpl = lpb + rows;
  const dim3 grid((unsigned)ceil_div64(rows, RNNT_ROWS)), block(64 * RNNT_ROWS);
  AsrProfScope prof(ASR_OP_CE, s);
  return asr_with_dtype(out_dtype, [&](auto tag) {
    using E = decltype(tag);
    return asr_launch<rnnt_bwd_kernel<E, false>>(grid, block, 0, s, logits, ld, targets, frame_lengths, target_lengths, B, T, Umax, V, blank, rows,
                                                 lse, lpb, lpl, alpha, beta, nll_d, grad_out, (E*)dlogits, ldd, (const int32_t*)nullptr,
                                                 Umax + 1);
  });
}

