// Knowledge distillation from a teacher's logits (train.py --distill-from): the temperature-softened
// KL(teacher || student) of every live row, optionally with ce.hip's label-smoothed cross entropy of the same student row, and ONE
// backward that writes the combined CE + KD logit gradient in the form asr_ce_bwd writes (the vocabulary projection's hand-over slot
// takes one gradient per logits tensor).  One wave per row, DS_ROWS rows per block, no atomics: the results are a function of the
// inputs alone.  Forward reads 2*M*V*4 bytes (its second pass is L2-resident), backward the same and writes M*ldd elements.
#include "common.h"
#include "topk.h"            // MaxIdx, wave_best: the arg-max order of csrc/ce.hip

// The two load arms of a row pass (16-byte loads / one by one) feed the same values in the same order through the same arithmetic; without
// multiply-add contraction the compiler cannot round the two differently.
#pragma clang fp contract(off)

#include "loss_rows.h"       // Smoothing, smoothed_row_loss, finish_sums: behind the pragma, so they round as this file does

namespace {

constexpr int DS_ROWS = 8;

__device__ __forceinline__ float4 ld4(const float* __restrict__ p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

// f(v, student[v], teacher[v]) for the columns of a row that `lane` owns, in ascending v: columns 4 lane + 256 k .. + 3, then column
// V4 + lane of the tail -- in BOTH load arms, so a row gives the same bits through an aligned and a misaligned base.  Columns >= V are
// never read.
template <typename F>
__device__ __forceinline__ void row_pairs(const float* __restrict__ s, const float* __restrict__ t, int V, int lane, F&& f) {
  const bool vs = (((uintptr_t)s) & 15) == 0, vt = (((uintptr_t)t) & 15) == 0;
  const int V4 = V & ~3;
#pragma unroll 2
  for (int v = lane * 4; v < V4; v += 256) {
    const float4 a = ld4(s + v, vs), b = ld4(t + v, vt);
    f(v, a.x, b.x); f(v + 1, a.y, b.y); f(v + 2, a.z, b.z); f(v + 3, a.w, b.w);
  }
  if (V4 + lane < V) f(V4 + lane, s[V4 + lane], t[V4 + lane]);
}

// softmax(x / tau)[v] from the row's log-sum-exp of x / tau: the ONE instruction sequence that gives both pS and pT in the backward
// (equal student and teacher bits give equal probabilities, and the KD gradient is then exactly 0)
__device__ __forceinline__ float soft_prob(float x, float tau, float lse) { return expf(x / tau - lse); }

// max + log(sum) rounded ONCE: the backward forms every probability as exp(x - lse) from this fp32 value, so whatever the stored
// log-sum-exp is off by moves all probabilities of the row by that much, relatively -- half an ulp of |lse| is what the format costs, and
// the logarithm and the addition in double (three per row) keep it at that
__device__ __forceinline__ float row_lse(float mx, float sum_exp) { return (float)((double)mx + log((double)sum_exp)); }

template <bool CE>
__global__ __launch_bounds__(64 * DS_ROWS) void distill_fwd_kernel(const float* __restrict__ student, int64_t ld_s,
                                                                   const float* __restrict__ teacher, int64_t ld_t,
                                                                   const int64_t* __restrict__ gold, int M, int V, float eps, int pad_id,
                                                                   float tau, float* __restrict__ row_stats, int64_t* __restrict__ argmax,
                                                                   float* __restrict__ partials) {
  __shared__ float s_part[DS_ROWS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * DS_ROWS + wave;
  float part[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < M) {
    const int64_t g = gold[row];
    float st[4] = {0.f, 0.f, 0.f, 0.f};
    int am = 0;
    if (g != pad_id) {                                     // a dead row's logits are never read, in either tensor
      const float* ls = student + (int64_t)row * ld_s;
      const float* lt = teacher + (int64_t)row * ld_t;
      MaxIdx mi{-INFINITY, 0x7fffffff};
      float mt = -INFINITY, sum = 0.f;
      row_pairs(ls, lt, V, lane, [&](int v, float a, float b) {
        if (CE) sum += a;
        if (a > mi.v) { mi.v = a; mi.i = v; }              // strictly greater, ascending v: the lowest index per lane
        mt = fmaxf(mt, b);
      });
      mi = wave_best(mi);
      mt = wave_max(mt);
      if (CE) sum = wave_sum(sum);
      // x -> x / tau is monotone (tau > 0, correctly rounded), so the maxima of the softened rows are the softened maxima
      const float ms = mi.v, mzs = ms / tau, mzt = mt / tau;
      float es = 0.f, est = 0.f, ett = 0.f, acc = 0.f;
      row_pairs(ls, lt, V, lane, [&](int v, float a, float b) {
        if (CE) es += expf(a - ms);
        const float as = a / tau - mzs, at = b / tau - mzt;       // both <= 0: no overflow, and the large terms have small arguments
        const float w = expf(at);
        est += expf(as);
        ett += w;
        acc += w * (at - as);
      });
      if (CE) es = wave_sum(es);
      est = wave_sum(est);
      ett = wave_sum(ett);
      acc = wave_sum(acc);
      // sum_v pT (log pT - log pS) = sum_v pT ((at - as) - (log ett - log est)): the maxima cancel in exact arithmetic and are never
      // added back, so a KD far below the log-sum-exps keeps its precision; equal rows give acc = 0, ett = est and exactly 0
      const float kd = tau * tau * (acc / ett - logf(ett / est));
      st[1] = row_lse(mzs, est);
      st[2] = row_lse(mzt, ett);
      st[3] = kd;
      part[1] = 1.f;
      part[3] = kd;
      if (CE) {
        const float lse = row_lse(ms, es);
        st[0] = lse;
        am = mi.i == 0x7fffffff ? 0 : mi.i;
        const float lpg = (g >= 0 && g < V) ? ls[g] - lse : 0.f;
        part[0] = smoothed_row_loss(lpg, sum, V, lse, eps);
        part[2] = mi.i == g ? 1.f : 0.f;
      }
    }
    if (lane < 4) row_stats[(int64_t)row * 4 + lane] = st[lane];
    if (CE && lane == 0) argmax[row] = am;
  }
  if (lane < 4) s_part[wave][lane] = part[lane];
  __syncthreads();
  if (threadIdx.x < 4) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < DS_ROWS; ++w) t += s_part[w][threadIdx.x];
    partials[(int64_t)blockIdx.x * 4 + threadIdx.x] = t;           // every slot written: nobody zeroes a destination first
  }
}

// sums[k] = the blocks' partial sums added in a fixed order (finish_sums of csrc/loss_rows.h);
// loss = (ce_scale sums[0] + kd_scale sums[3]) / (den ? den[0] : sums[1])
__global__ __launch_bounds__(256) void distill_finish_kernel(const float* __restrict__ partials, int nblocks, const float* __restrict__ den,
                                                             float ce_scale, float kd_scale, float* __restrict__ sums,
                                                             float* __restrict__ loss) {
  __shared__ float red[4][256];
  const int tid = threadIdx.x;
  finish_sums<4>(partials, nblocks, red);
  if (tid < 4) sums[tid] = red[tid][0];
  if (tid == 0) loss[0] = (ce_scale * red[0][0] + kd_scale * red[3][0]) / (den ? den[0] : red[1][0]);
}

// (its own four-wide store and one-by-one dead-row loop, not store4 / GradRow::zero of csrc/loss_rows.h: with those both arms gained a VGPR
// and the bf16 arm 36 instructions, and it measured at the upper edge of the parent's range; profiles/loss_rows_refactor.txt)
struct alignas(8) bf16x4_t { bf16_t v[4]; };
__device__ __forceinline__ void st4(float* p, float a, float b, float c, float d) {
  if ((((uintptr_t)p) & 15) == 0) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); return; }
  p[0] = a; p[1] = b; p[2] = c; p[3] = d;
}
__device__ __forceinline__ void st4(bf16_t* p, float a, float b, float c, float d) {
  const bf16x4_t o{{f32_to_bf16(a), f32_to_bf16(b), f32_to_bf16(c), f32_to_bf16(d)}};
  if ((((uintptr_t)p) & 7) == 0) { *reinterpret_cast<bf16x4_t*>(p) = o; return; }
  p[0] = o.v[0]; p[1] = o.v[1]; p[2] = o.v[2]; p[3] = o.v[3];
}

template <typename T>
__global__ __launch_bounds__(64 * DS_ROWS) void distill_bwd_kernel(const float* __restrict__ student, int64_t ld_s,
                                                                   const float* __restrict__ teacher, int64_t ld_t,
                                                                   const int64_t* __restrict__ gold, const float* __restrict__ row_stats,
                                                                   int M, int V, float eps, int pad_id, float tau, float ce_scale,
                                                                   float kd_scale, const float* __restrict__ grad_out,
                                                                   const float* __restrict__ count, T* __restrict__ dl, int64_t ldd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * DS_ROWS + wave;
  if (row >= M) return;
  T* d = dl + (int64_t)row * ldd;
  const int64_t g = gold[row];
  if (g == pad_id) {
    for (int64_t v = lane; v < ldd; v += 64) DT<T>::st(d + v, 0.f);
    return;
  }
  const float coef = (*grad_out) / (*count);
  const float* ls = student + (int64_t)row * ld_s;
  const float* lt = teacher + (int64_t)row * ld_t;
  const float lse = row_stats[(int64_t)row * 4], lse_s = row_stats[(int64_t)row * 4 + 1], lse_t = row_stats[(int64_t)row * 4 + 2];
  const Smoothing q(eps, V);
  const float kt = kd_scale * tau;
  const bool ce = ce_scale != 0.f;
  // The fp32 arm (parity mode, and the CTC head's frame-level term) first sums each distribution as it will be formed, exp(x - lse), and
  // divides by that sum: what the stored fp32 log-sum-exp is off by -- up to half an ulp of |lse|, 5e-7 of every probability at |lse| ~ 9
  // -- is common to the row and cancels.  The bf16 arm (the hand-over to the vocabulary projection) rounds every element to 2**-9 and
  // keeps the single pass.
  float zc = 1.f, zs = 1.f, zt = 1.f;
  if (DT<T>::kDtype == ASR_F32) {
    zc = zs = zt = 0.f;
    row_pairs(ls, lt, V, lane, [&](int, float a, float b) {
      if (ce) zc += expf(a - lse);
      zs += soft_prob(a, tau, lse_s);
      zt += soft_prob(b, tau, lse_t);
    });
    zc = ce ? wave_sum(zc) : 1.f;
    zs = wave_sum(zs);
    zt = wave_sum(zt);
  }
  auto grad = [&](int v, float a, float b) {
    float o = kt * (soft_prob(a, tau, lse_s) / zs - soft_prob(b, tau, lse_t) / zt);
    if (ce) o = ce_scale * (expf(a - lse) / zc * q.sum_q - (v == g ? q.q_gold : q.q_other)) + o;
    return coef * o;
  };
  // this kernel stays off GradRow (csrc/loss_rows.h): it reads two tensors and owns its columns by V4 as row_pairs does, not by ldd4
  const bool vs = (((uintptr_t)ls) & 15) == 0, vt = (((uintptr_t)lt) & 15) == 0;
  const int V4 = V & ~3;
#pragma unroll 2
  for (int v = lane * 4; v < V4; v += 256) {
    const float4 a = ld4(ls + v, vs), b = ld4(lt + v, vt);
    st4(d + v, grad(v, a.x, b.x), grad(v + 1, a.y, b.y), grad(v + 2, a.z, b.z), grad(v + 3, a.w, b.w));
  }
  if (V4 + lane < V) DT<T>::st(d + V4 + lane, grad(V4 + lane, ls[V4 + lane], lt[V4 + lane]));
  for (int64_t v = V + lane; v < ldd; v += 64) DT<T>::st(d + v, 0.f);
}

}  // namespace

extern "C" int asr_distill_partial_blocks(int M) { return M > 0 ? (M + DS_ROWS - 1) / DS_ROWS : 0; }

extern "C" int asr_distill_fwd(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t, const int64_t* gold, int M, int V,
                               float smoothing, int pad_id, float temperature, int with_ce, float* row_stats, int64_t* argmax,
                               float* partials, hipStream_t s) {
  ASR_CHECK_ARG(student && teacher && gold && row_stats && partials && (argmax || !with_ce));
  ASR_CHECK_ARG(M >= 1 && V >= 1 && ld_s >= V && ld_t >= V && smoothing >= 0.f && smoothing < 1.f && temperature >= 0.5f &&
                temperature <= 16.f);
  AsrProfScope prof(ASR_OP_CE, s);
  const dim3 grid((M + DS_ROWS - 1) / DS_ROWS), block(64 * DS_ROWS);
  return with_ce ? asr_launch<distill_fwd_kernel<true>>(grid, block, 0, s, student, ld_s, teacher, ld_t, gold, M, V, smoothing, pad_id,
                                                        temperature, row_stats, argmax, partials)
                 : asr_launch<distill_fwd_kernel<false>>(grid, block, 0, s, student, ld_s, teacher, ld_t, gold, M, V, smoothing, pad_id,
                                                         temperature, row_stats, argmax, partials);
}

extern "C" int asr_distill_finish(const float* partials, int nblocks, const float* den, float ce_scale, float kd_scale, float* sums,
                                  float* loss, hipStream_t s) {
  ASR_CHECK_ARG(sums && loss && nblocks >= 0 && (partials || nblocks == 0));
  return asr_launch<distill_finish_kernel>(dim3(1), dim3(256), 0, s, partials, nblocks, den, ce_scale, kd_scale, sums, loss);
}

extern "C" int asr_distill_bwd(const float* student, int64_t ld_s, const float* teacher, int64_t ld_t, const int64_t* gold,
                               const float* row_stats, int M, int V, float smoothing, int pad_id, float temperature, float ce_scale,
                               float kd_scale, const float* grad_out, const float* count, void* dlogits, int64_t ldd, int out_dtype,
                               hipStream_t s) {
  ASR_CHECK_ARG(student && teacher && gold && row_stats && grad_out && count && dlogits);
  ASR_CHECK_ARG(M >= 1 && V >= 1 && ld_s >= V && ld_t >= V && ldd >= V && smoothing >= 0.f && smoothing < 1.f && temperature >= 0.5f &&
                temperature <= 16.f);
  if (out_dtype != ASR_F32 && out_dtype != ASR_BF16) return ASR_EINVAL;
  AsrProfScope prof(ASR_OP_CE, s);
  const dim3 grid((M + DS_ROWS - 1) / DS_ROWS), block(64 * DS_ROWS);
  return asr_with_dtype(out_dtype, [&](auto tag) {
    using T = decltype(tag);
    return asr_launch<distill_bwd_kernel<T>>(grid, block, 0, s, student, ld_s, teacher, ld_t, gold, row_stats, M, V, smoothing, pad_id,
                                             temperature, ce_scale, kd_scale, grad_out, count, (T*)dlogits, ldd);
  });
}
