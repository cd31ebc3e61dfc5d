// SpecAugment (Park et al. 2019: time warp, frequency masks, time masks) of the per-utterance normalised log-spectrogram on the GPU.
// The reference has no counterpart; the definition is DESIGN.md section 7:
//   warp   c -> w over the n kept frames of an utterance, applied when 0 < c < n and 0 <= w < n: output frame t reads the segment
//          (u, s, d, base) = (t, c, w, 0) for t < w, else (t - w, n - c, n - w, c), at the half-pixel position
//          num = (2u+1) s - d, den = 2d:  i0 = num / den, r = num % den (num < 0: i0 = r = 0), i1 = min(i0 + 1, s - 1),
//          y = fmaf(float(r) / float(den), x[base+i1] - x[base+i0], x[base+i0])   (r == 0: x[base+i0] itself, so c == w is the
//          identity on every bit pattern; fmaf would turn -0.0 into +0.0)
//   masks  rows f0 <= f < f0+fw and frames t0 <= t < t0+tw are +0.0 (the utterance mean), as are the frames t >= n.
// One out-of-place pass over (B, F, T_out): lanes along t (coalesced stores, monotone gather loads), a workgroup covers kRows rows of
// one utterance so the integer division of a frame is paid once per kRows elements, the parameter row is read once per workgroup
// into LDS, masked rows / frames are written without reading the input.  NORM: the input is the raw log-magnitude and every loaded
// value goes through spect_norm_apply first (the expressions of spect_normalize_kernel), so the fused launch of
// asr_spect_finish_aug is bitwise asr_spect_finish followed by asr_spec_augment.  Contraction into FMA is off in this file for
// that reason: (v - mean) * rstd must round before the difference x1 - x0 is taken.  The interpolation's own fmaf is explicit.
#pragma clang fp contract(off)

#include "spec_augment.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 8;

struct WarpSrc {
  int i0, i1;          // source frames (already offset by the segment's base)
  float frac;
};

template <typename I>
__device__ __forceinline__ WarpSrc warp_src_t(int t, int n, int c, int w) {
  I u, s, d;
  int base;
  if (t < w) { u = t; s = c; d = w; base = 0; }
  else { u = t - w; s = n - c; d = n - w; base = c; }
  const I num = (2 * u + 1) * s - d, den = 2 * d;
  I q = 0, r = 0;
  if (num >= 0) { q = num / den; r = num % den; }        // q <= s - 1: num < (2d - 1) s
  WarpSrc o;
  o.i0 = base + (int)q;
  o.i1 = base + (int)(q + 1 < s ? q + 1 : s - 1);
  o.frac = (float)r / (float)den;
  return o;
}

template <bool NORM, int VEC>
__global__ __launch_bounds__(kThreads) void spec_augment_kernel(const float* __restrict__ x, int64_t ldx_row, float* __restrict__ out,
                                                                int64_t ldo_row, const int32_t* __restrict__ params,
                                                                const int32_t* __restrict__ lengths, const float* __restrict__ sums,
                                                                const float* __restrict__ sq, int hop, int F, int T_out) {
  __shared__ int32_t prm[kSpecParams];
  const int b = blockIdx.z, f_lo = blockIdx.y * kRows;
  if (threadIdx.x < kSpecParams) prm[threadIdx.x] = params[(int64_t)b * kSpecParams + threadIdx.x];
  __syncthreads();
  const int t_lo = (blockIdx.x * kThreads + threadIdx.x) * VEC;
  if (t_lo >= T_out) return;

  int n = min(max(prm[0], 0), T_out);
  SpectNorm nm = {0.f, 1.f};
  if (NORM) {
    const int nfr = spect_frames(lengths[b], hop);
    n = min(n, nfr);
    nm = spect_norm_of(sums, sq, b, nfr, F);
  }
  const int c = prm[1], w = prm[2];
  const bool warp = c > 0 && c < n && w >= 0 && w < n;
  const int nF = min(max(prm[3], 0), kSpecMaxMasks), nT = min(max(prm[4], 0), kSpecMaxMasks);

  // per frame: live (inside [0, n) and outside every time mask) and where it reads
  bool live[VEC];
  WarpSrc src[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int t = t_lo + v;                               // VEC > 1 only with T_out % VEC == 0: t < T_out
    bool ok = t < n;
    for (int k = 0; k < nT; ++k) {
      const int64_t m0 = prm[8 + 2 * kSpecMaxMasks + 2 * k], mw = prm[9 + 2 * kSpecMaxMasks + 2 * k];
      if (t >= m0 && t < m0 + mw) ok = false;
    }
    live[v] = ok;
    src[v].i0 = src[v].i1 = t;
    src[v].frac = 0.f;
    if (ok && warp) src[v] = n <= kSpecWarp32 ? warp_src_t<int>(t, n, c, w) : warp_src_t<int64_t>(t, n, c, w);
  }

#pragma unroll 2
  for (int rr = 0; rr < kRows; ++rr) {
    const int f = f_lo + rr;
    if (f >= F) break;
    bool row = true;                                      // block-uniform
    for (int k = 0; k < nF; ++k) {
      const int64_t m0 = prm[8 + 2 * k], mw = prm[9 + 2 * k];
      if (f >= m0 && f < m0 + mw) row = false;
    }
    const float* xr = x + ((int64_t)b * F + f) * ldx_row;
    float y[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      y[v] = 0.f;
      if (row && live[v]) {
        float x0 = xr[src[v].i0];
        if (NORM) x0 = spect_norm_apply(x0, nm);
        y[v] = x0;
        if (src[v].frac != 0.f) {
          float x1 = xr[src[v].i1];
          if (NORM) x1 = spect_norm_apply(x1, nm);
          y[v] = fmaf(src[v].frac, x1 - x0, x0);
        }
      }
    }
    float* o = out + ((int64_t)b * F + f) * ldo_row + t_lo;
    if (VEC == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = y[v];
    }
  }
}

template <bool NORM>
int launch(const float* x, int64_t ldx_row, float* out, int64_t ldo_row, const int32_t* params, const int32_t* lengths,
           const float* sums, const float* sq, int hop, int B, int F, int T_out, hipStream_t stream) {
  // 16-byte stores need every row base aligned and whole groups of four frames; anything else takes the scalar kernel
  const bool vec = aligned16(out) && ldo_row % 4 == 0 && T_out % 4 == 0;
  const int per = kThreads * (vec ? 4 : 1);
  const dim3 grid((unsigned)((T_out + per - 1) / per), (unsigned)((F + kRows - 1) / kRows), (unsigned)B);
  if (vec) return asr_launch<spec_augment_kernel<NORM, 4>>(grid, dim3(kThreads), 0, stream, x, ldx_row, out, ldo_row, params, lengths, sums, sq, hop, F, T_out);
  return asr_launch<spec_augment_kernel<NORM, 1>>(grid, dim3(kThreads), 0, stream, x, ldx_row, out, ldo_row, params, lengths, sums, sq, hop, F, T_out);
}

}  // namespace

int spec_augment_launch(const float* x, int64_t ldx_row, float* out, int64_t ldo_row, const int32_t* params, const int32_t* lengths,
                        const float* sums, const float* sq, int hop, int B, int F, int T_out, hipStream_t stream) {
  ASR_CHECK_ARG(x && out && params && x != out && B >= 0 && B <= 65535 && F > 0 && F <= 65535 * kRows && T_out >= 0 && T_out <= (1 << 30));
  ASR_CHECK_ARG(ldx_row >= T_out && ldo_row >= T_out);
  if (B == 0 || T_out == 0) return ASR_OK;
  if (lengths) {
    ASR_CHECK_ARG(sums && sq && hop > 0);
    return launch<true>(x, ldx_row, out, ldo_row, params, lengths, sums, sq, hop, B, F, T_out, stream);
  }
  return launch<false>(x, ldx_row, out, ldo_row, params, nullptr, nullptr, nullptr, 1, B, F, T_out, stream);
}

extern "C" int asr_spec_augment(const float* x, int64_t ldx_row, float* out, int64_t ldo_row, const int32_t* params, int B, int F,
                                int T_out, hipStream_t stream) {
  AsrProfScope prof(ASR_OP_LAYOUT, stream);
  return spec_augment_launch(x, ldx_row, out, ldo_row, params, nullptr, nullptr, nullptr, 1, B, F, T_out, stream);
}
