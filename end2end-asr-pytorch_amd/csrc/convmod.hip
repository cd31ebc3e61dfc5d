// Conformer-style convolution module (arXiv:2005.08100 without its BatchNorm): the three memory-bound kernels between
// the module's two pointwise GEMMs.  Channel last throughout: u (B,T,2D) = [a | gate] from pointwise_1, everything else (B,T,D).
//
//   g[b,t,c] = a sigma(gate)                       for t < len_b, 0 for t >= len_b and outside [0,T)   (the zero fill in front of the conv)
//   s[b,t,c] = bd[c] + sum_k wd[c,k] g[b,t+k-P,c]  P = (K-1)/2, cross-correlation as torch's Conv1d(D, D, K, padding=P, groups=D)
//   v[b,t,c] = s sigma(s)                          for t < len_b, 0 for t >= len_b
//
//   ds = dv sigma(s) (1 + s (1 - sigma(s)))        for t < len_b, else 0
//   dg[t'] = sum_k wd[c,k] ds[t'+P-k]              for t' < len_b, else 0
//   du[..., :D] = dg sigma(gate)       du[..., D:] = dg a sigma(gate) (1 - sigma(gate))
//   dwd[c,k] += sum_{b,t} ds[b,t,c] g[b,t+k-P,c]   dbd[c] += sum_{b,t} ds[b,t,c]
//
// sigma(x) = 1 / (1 + expf(-x)): exactly 1 for x >= 32 (expf(-x) < 2^-24), exactly 0 for x <= -88 (expf overflows to inf).  All
// arithmetic is fp32; s and u are read back in the storage type as saved.
//
// One shape for the three kernels.  A workgroup of 256 threads owns a tile of 64 frames x 128 channels of one utterance: lane cl of
// the 32 channel lanes takes channels c0 + 4 cl .. + 3 (one 16-byte access in fp32, 8 bytes in bf16; 32 lanes = one contiguous
// 512 / 256-byte piece of a row), time group tg of 8 takes 8 consecutive frames.  The tile's windowed operand -- g for the forward and
// the weight gradient, ds for the data gradient -- is computed ONCE per element for the tile's 64 + KB - 1 frames (the tile and its
// halo) and staged in LDS as fp32; a thread then walks the 8 + KB - 1 rows of its window once, every row feeding the up to 8 outputs
// (or, in the weight gradient, the up to 8 taps) it belongs to.  The KB x 4 per-lane weights (read through LDS, where the chunk's
// taps arrive as one contiguous copy) or weight-gradient sums stay in registers: the kernels are instantiated for the tap buckets KB = 7, 15, 31 and a K below its bucket is centred in it between zero
// taps (0 * g adds an exact zero, and only the staged rows, zero-filled outside [0, len), are ever multiplied).
// Rows t >= len_b are never read: they are staged, and written, as zeros.
//
// The weight gradient uses no atomics: the grid is channel chunks x row slices, slice z sums the tiles z, z + NS, ... in registers,
// folds its 8 time groups in LDS in index order and stores one (K + 1, D) slab (taps, then the bias row) into the caller's workspace;
// a finish launch adds the slabs in index order and ACCUMULATES into the fp32 gradient buffers.  Same inputs, same bits.
#include <type_traits>

#include "common.h"

namespace {

constexpr int CM_LANES = 32;                    // channel lanes of a workgroup, 4 channels each
constexpr int CM_CC = 4 * CM_LANES;             // channels per workgroup
constexpr int CM_TG = 8;                        // time groups of a workgroup
constexpr int CM_R = 8;                         // consecutive frames per thread
constexpr int CM_TT = CM_TG * CM_R;             // frames per tile
constexpr int CM_MAX_SLICES = 128;              // row slices of the weight gradient (slabs the finish pass adds)

__device__ __forceinline__ float cm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float cm_swish_grad(float s) {
  const float sg = cm_sigmoid(s);
  return sg * (1.f + s * (1.f - sg));
}

template <typename T> __device__ __forceinline__ f32x4_t cm_ld4(const T* p);
template <> __device__ __forceinline__ f32x4_t cm_ld4<float>(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }
template <> __device__ __forceinline__ f32x4_t cm_ld4<bf16_t>(const bf16_t* p) {
  const uint2 r = *reinterpret_cast<const uint2*>(p);
  f32x4_t v;
  v[0] = __uint_as_float(r.x << 16);
  v[1] = __uint_as_float(r.x & 0xFFFF0000u);
  v[2] = __uint_as_float(r.y << 16);
  v[3] = __uint_as_float(r.y & 0xFFFF0000u);
  return v;
}
template <typename T> __device__ __forceinline__ void cm_st4(T* p, const f32x4_t& v);
template <> __device__ __forceinline__ void cm_st4<float>(float* p, const f32x4_t& v) { *reinterpret_cast<f32x4_t*>(p) = v; }
template <> __device__ __forceinline__ void cm_st4<bf16_t>(bf16_t* p, const f32x4_t& v) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
}

__device__ __forceinline__ int cm_len(const int32_t* len, int b, int T) {
  const int L = len[b];
  return L < 0 ? 0 : (L > T ? T : L);
}

// The chunk's taps, wd[c0 .. c0 + 128)[K], are one contiguous run of the (D,K) array: copied to LDS with consecutive lanes on
// consecutive floats (a lane reading its own channels' taps straight from memory touches 32 cache lines per load instruction, K x 4
// of them per thread: measured, that alone made K = 31 twice as slow as K = 15).
__device__ __forceinline__ void cm_stage_taps(float* wl, const float* __restrict__ wd, int c0, int D, int K, int tid) {
  const int n = (D - c0 < CM_CC ? D - c0 : CM_CC) * K;
  const float* src = wd + (int64_t)c0 * K;
  for (int i = tid; i < n; i += 256) wl[i] = src[i];
}
// The K taps of channels 4 cl .. + 3 of the chunk, from LDS, centred in the bucket's KB (zero taps around them); FLIP: reversed, the
// data gradient's order.
template <int KB, bool FLIP> __device__ __forceinline__ void cm_load_taps(f32x4_t (&w)[KB], const float* wl, int cl, int K, bool cok) {
  const int off = (KB - K) / 2;
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int kk = (FLIP ? KB - 1 - k : k) - off;
    const bool ok = cok && kk >= 0 && kk < K;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[k][i] = ok ? wl[(4 * cl + i) * K + kk] : 0.f;
  }
}

// sh[row][lane] <- g of frame t_lo + row, channels c0 + 4 lane .. + 3, for the 64 + KB - 1 rows of a tile: the GLU once per element.
template <typename T, int KB>
__device__ __forceinline__ void cm_stage_glu(f32x4_t* sh, const T* __restrict__ u_b, int t_lo, int L, int D, int c0, int tid) {
  constexpr int N = (CM_TT + KB - 1) * CM_LANES, STEPS = (N + 255) / 256;
  // (a fixed trip count, unrolled: the loads of all steps are in flight together instead of one latency per step)
  f32x4_t a[STEPS], gt[STEPS];
#pragma unroll
  for (int j = 0; j < STEPS; ++j) {
    const int i = tid + 256 * j;
    const int t = t_lo + i / CM_LANES, c = c0 + 4 * (i % CM_LANES);
    a[j] = gt[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (i < N && t >= 0 && t < L && c < D) {
      const T* p = u_b + (int64_t)t * 2 * D + c;
      a[j] = cm_ld4<T>(p);
      gt[j] = cm_ld4<T>(p + D);
    }
  }
#pragma unroll
  for (int j = 0; j < STEPS; ++j) {
    const int i = tid + 256 * j;
    const int t = t_lo + i / CM_LANES, c = c0 + 4 * (i % CM_LANES);
    f32x4_t g = {0.f, 0.f, 0.f, 0.f};
    if (i < N && t >= 0 && t < L && c < D) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = a[j][e] * cm_sigmoid(gt[j][e]);
    }
    if (i < N) sh[i] = g;
  }
}

// out[r] += sum_k w[k] * window row (r + k), r < 8: the thread's 8 + KB - 1 staged rows are read once each.
template <int KB> __device__ __forceinline__ void cm_window_dot(f32x4_t (&out)[CM_R], const f32x4_t (&w)[KB], const f32x4_t* sh_thread) {
#pragma unroll
  for (int j = 0; j < CM_R + KB - 1; ++j) {
    const f32x4_t x = sh_thread[j * CM_LANES];
#pragma unroll
    for (int r = 0; r < CM_R; ++r)
      if (j - r >= 0 && j - r < KB) out[r] += w[j - r] * x;
  }
}

template <typename T, int KB>
__global__ __launch_bounds__(256) void convmod_fwd_kernel(const T* __restrict__ u, const float* __restrict__ wd, const float* __restrict__ bd,
                                                          const int32_t* __restrict__ len, int ntiles, int Tn, int D, int K,
                                                          T* __restrict__ s_out, T* __restrict__ v_out) {
  __shared__ f32x4_t sh[(CM_TT + KB - 1) * CM_LANES];
  __shared__ float wl[CM_CC * KB];
  const int tid = threadIdx.x, cl = tid % CM_LANES, tg = tid / CM_LANES;
  const int b = blockIdx.x / ntiles, t0 = (blockIdx.x % ntiles) * CM_TT, c0 = blockIdx.y * CM_CC;
  const int L = cm_len(len, b, Tn);
  const int c = c0 + 4 * cl;
  const bool cok = c < D;
  cm_stage_taps(wl, wd, c0, D, K, tid);
  cm_stage_glu<T, KB>(sh, u + (int64_t)b * Tn * 2 * D, t0 - (KB - 1) / 2, L, D, c0, tid);
  f32x4_t acc[CM_R];
  f32x4_t bias = {0.f, 0.f, 0.f, 0.f};
  if (cok) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[e] = bd[c + e];      // (a parameter's slot in the flat buffer need not be 16-byte aligned)
  }
#pragma unroll
  for (int r = 0; r < CM_R; ++r) acc[r] = bias;
  __syncthreads();
  f32x4_t w[KB];
  cm_load_taps<KB, false>(w, wl, cl, K, cok);
  cm_window_dot<KB>(acc, w, sh + tg * CM_R * CM_LANES + cl);
  if (!cok) return;
#pragma unroll
  for (int r = 0; r < CM_R; ++r) {
    const int t = t0 + tg * CM_R + r;
    if (t >= Tn) break;
    f32x4_t v ={0.f, 0.f, 0.f, 0.f};
    if (t < L) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = acc[r][e] * cm_sigmoid(acc[r][e]);
    }
    const int64_t o = ((int64_t)b * Tn + t) * D + c;
    cm_st4<T>(s_out + o, acc[r]);
    cm_st4<T>(v_out + o, v);
  }
}

template <typename T, int KB>
__global__ __launch_bounds__(256) void convmod_bwd_data_kernel(const T* __restrict__ dv, const T* __restrict__ s, const T* __restrict__ u,
                                                               const float* __restrict__ wd, const int32_t* __restrict__ len, int ntiles,
                                                               int Tn, int D, int K, T* __restrict__ du) {
  constexpr int ROWS = CM_TT + KB - 1;
  __shared__ f32x4_t sh[ROWS * CM_LANES];
  __shared__ float wl[CM_CC * KB];
  const int tid = threadIdx.x, cl = tid % CM_LANES, tg = tid / CM_LANES;
  const int b = blockIdx.x / ntiles, t0 = (blockIdx.x % ntiles) * CM_TT, c0 = blockIdx.y * CM_CC;
  const int L = cm_len(len, b, Tn);
  const int c = c0 + 4 * cl;
  const bool cok = c < D;
  cm_stage_taps(wl, wd, c0, D, K, tid);
  // ds of the tile and its halo (loads first, all in flight together; then the arithmetic)
  {
    constexpr int N = ROWS * CM_LANES, STEPS = (N + 255) / 256;
    f32x4_t g[STEPS], sv[STEPS];
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
      const int i = tid + 256 * j;
      const int t = t0 - (KB - 1) / 2 + i / CM_LANES, ci = c0 + 4 * (i % CM_LANES);
      g[j] = sv[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (i < N && t >= 0 && t < L && ci < D) {
        const int64_t o = ((int64_t)b * Tn + t) * D + ci;
        g[j] = cm_ld4<T>(dv + o);
        sv[j] = cm_ld4<T>(s + o);
      }
    }
#pragma unroll
    for (int j = 0; j < STEPS; ++j) {
      const int i = tid + 256 * j;
      const int t = t0 - (KB - 1) / 2 + i / CM_LANES, ci = c0 + 4 * (i % CM_LANES);
      f32x4_t ds = {0.f, 0.f, 0.f, 0.f};
      if (i < N && t >= 0 && t < L && ci < D) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ds[e] = g[j][e] * cm_swish_grad(sv[j][e]);
      }
      if (i < N) sh[i] = ds;
    }
  }
  f32x4_t dg[CM_R];
#pragma unroll
  for (int r = 0; r < CM_R; ++r) dg[r] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  f32x4_t w[KB];
  cm_load_taps<KB, true>(w, wl, cl, K, cok);
  cm_window_dot<KB>(dg, w, sh + tg * CM_R * CM_LANES + cl);
  if (!cok) return;
#pragma unroll
  for (int r = 0; r < CM_R; ++r) {
    const int t = t0 + tg * CM_R + r;
    if (t >= Tn) break;
    f32x4_t da = {0.f, 0.f, 0.f, 0.f}, dgate = {0.f, 0.f, 0.f, 0.f};
    const int64_t o = ((int64_t)b * Tn + t) * 2 * D + c;
    if (t < L) {
      const f32x4_t a = cm_ld4<T>(u + o), gt = cm_ld4<T>(u + o + D);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sg = cm_sigmoid(gt[e]);
        da[e] = dg[r][e] * sg;
        dgate[e] = dg[r][e] * a[e] * (sg * (1.f - sg));
      }
    }
    cm_st4<T>(du + o, da);
    cm_st4<T>(du + o + D, dgate);
  }
}

template <typename T, int KB>
__global__ __launch_bounds__(256) void convmod_bwd_weight_kernel(const T* __restrict__ dv, const T* __restrict__ s, const T* __restrict__ u,
                                                                 const int32_t* __restrict__ len, int ntiles, int total_tiles, int Tn, int D,
                                                                 int K, float* __restrict__ ws) {
  __shared__ f32x4_t sh[(CM_TT + KB - 1) * CM_LANES];       // the g window; afterwards the (KB + 1, 32) fold of the time groups
  const int tid = threadIdx.x, cl = tid % CM_LANES, tg = tid / CM_LANES;
  const int z = blockIdx.x, NS = gridDim.x, c0 = blockIdx.y * CM_CC;
  const int c = c0 + 4 * cl;
  const bool cok = c < D;
  f32x4_t accw[KB], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < KB; ++k) accw[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int tile = z; tile < total_tiles; tile += NS) {      // (every condition below is the same for all threads of the workgroup)
    const int b = tile / ntiles, t0 = (tile % ntiles) * CM_TT;
    const int L = cm_len(len, b, Tn);
    if (t0 >= L) continue;                                   // ds = 0 on the whole tile
    __syncthreads();                                         // the previous tile's window has been read
    cm_stage_glu<T, KB>(sh, u + (int64_t)b * Tn * 2 * D, t0 - (KB - 1) / 2, L, D, c0, tid);
    f32x4_t ds[CM_R];
#pragma unroll
    for (int r = 0; r < CM_R; ++r) {
      const int t = t0 + tg * CM_R + r;
      ds[r] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      if (cok && t < L) {
        const int64_t o = ((int64_t)b * Tn + t) * D + c;
        const f32x4_t g = cm_ld4<T>(dv + o), sv = cm_ld4<T>(s + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) ds[r][e] = g[e] * cm_swish_grad(sv[e]);
      }
      accb += ds[r];
    }
    __syncthreads();
    const f32x4_t* win = sh + tg * CM_R * CM_LANES + cl;
#pragma unroll
    for (int j = 0; j < CM_R + KB - 1; ++j) {
      const f32x4_t x = win[j * CM_LANES];
#pragma unroll
      for (int r = 0; r < CM_R; ++r)
        if (j - r >= 0 && j - r < KB) accw[j - r] += ds[r] * x;
    }
  }
  __syncthreads();
  // the 8 time groups, in index order
  for (int i = 0; i < CM_TG; ++i) {
    if (tg == i) {
#pragma unroll
      for (int k = 0; k < KB; ++k) sh[k * CM_LANES + cl] = i == 0 ? accw[k] : sh[k * CM_LANES + cl] + accw[k];
      sh[KB * CM_LANES + cl] = i == 0 ? accb : sh[KB * CM_LANES + cl] + accb;
    }
    __syncthreads();
  }
  // slab z: rows k < K the taps, row K the bias
  const int off = (KB - K) / 2;
  for (int i = tid; i < (K + 1) * CM_LANES; i += 256) {
    const int k = i / CM_LANES, l = i % CM_LANES, cc = c0 + 4 * l;
    if (cc < D) cm_st4<float>(ws + ((int64_t)z * (K + 1) + k) * D + cc, sh[(k < K ? k + off : KB) * CM_LANES + l]);
  }
}

__global__ __launch_bounds__(256) void convmod_wgrad_finish_kernel(const float* __restrict__ ws, int NS, int D, int K, float* __restrict__ dwd,
                                                                   float* __restrict__ dbd) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= (K + 1) * D) return;
  const int k = e / D, c = e % D;
  float sum = 0.f;
#pragma unroll 16                                             // (16 loads in flight; the adds stay in index order)
  for (int z = 0; z < NS; ++z) sum += ws[(int64_t)z * (K + 1) * D + e];
  if (k < K) dwd[(int64_t)c * K + k] += sum;
  else dbd[c] += sum;
}

inline bool cm_supported(int B, int T, int D, int K, int dtype) {
  return B >= 1 && T >= 1 && D >= 8 && D % 8 == 0 && K >= 3 && K <= 31 && (K & 1) && (dtype == ASR_F32 || dtype == ASR_BF16) &&
         (int64_t)B * ((T + CM_TT - 1) / CM_TT) < (1ll << 31);
}
inline int cm_tiles(int T) { return (T + CM_TT - 1) / CM_TT; }
inline int cm_slices(int B, int T) {
  const int64_t total = (int64_t)B * cm_tiles(T);
  return (int)(total < CM_MAX_SLICES ? total : CM_MAX_SLICES);
}

// f(bucket tag) with the smallest tap bucket that holds K
template <class F> int cm_with_bucket(int K, F&& f) {
  if (K <= 7) return f(std::integral_constant<int, 7>{});
  if (K <= 15) return f(std::integral_constant<int, 15>{});
  return f(std::integral_constant<int, 31>{});
}

}  // namespace

extern "C" int64_t asr_convmod_workspace(int B, int T, int D, int K) {
  if (!cm_supported(B, T, D, K, ASR_F32)) return 0;
  return (int64_t)cm_slices(B, T) * (K + 1) * D;
}

extern "C" int asr_convmod_fwd(const void* u, const float* wd, const float* bd, const int32_t* len, int B, int T, int D, int K, int dtype,
                               void* s_out, void* v_out, hipStream_t stream) {
  if (!cm_supported(B, T, D, K, dtype)) return ASR_EUNSUPPORTED;
  ASR_CHECK_ARG(u && wd && bd && len && s_out && v_out);
  const dim3 grid((unsigned)(B * cm_tiles(T)), (unsigned)((D + CM_CC - 1) / CM_CC));
  return asr_with_dtype(dtype, [&](auto tag) {
    using T_ = decltype(tag);
    return cm_with_bucket(K, [&](auto kb) {
      return asr_launch<convmod_fwd_kernel<T_, decltype(kb)::value>>(grid, dim3(256), 0, stream, (const T_*)u, wd, bd, len, cm_tiles(T), T, D, K,
                                                                      (T_*)s_out, (T_*)v_out);
    });
  });
}

extern "C" int asr_convmod_bwd_data(const void* dv, const void* s, const void* u, const float* wd, const int32_t* len, int B, int T, int D,
                                    int K, int dtype, void* du_out, hipStream_t stream) {
  if (!cm_supported(B, T, D, K, dtype)) return ASR_EUNSUPPORTED;
  ASR_CHECK_ARG(dv && s && u && wd && len && du_out);
  const dim3 grid((unsigned)(B * cm_tiles(T)), (unsigned)((D + CM_CC - 1) / CM_CC));
  return asr_with_dtype(dtype, [&](auto tag) {
    using T_ = decltype(tag);
    return cm_with_bucket(K, [&](auto kb) {
      return asr_launch<convmod_bwd_data_kernel<T_, decltype(kb)::value>>(grid, dim3(256), 0, stream, (const T_*)dv, (const T_*)s, (const T_*)u,
                                                                           wd, len, cm_tiles(T), T, D, K, (T_*)du_out);
    });
  });
}

extern "C" int asr_convmod_bwd_weight(const void* dv, const void* s, const void* u, const int32_t* len, int B, int T, int D, int K, int dtype,
                                      float* workspace, int64_t workspace_floats, float* dwd, float* dbd, hipStream_t stream) {
  if (!cm_supported(B, T, D, K, dtype)) return ASR_EUNSUPPORTED;
  ASR_CHECK_ARG(dv && s && u && len && workspace && dwd && dbd);
  ASR_CHECK_ARG(workspace_floats >= asr_convmod_workspace(B, T, D, K));
  const int NS = cm_slices(B, T);
  const dim3 grid((unsigned)NS, (unsigned)((D + CM_CC - 1) / CM_CC));
  const int rc = asr_with_dtype(dtype, [&](auto tag) {
    using T_ = decltype(tag);
    return cm_with_bucket(K, [&](auto kb) {
      return asr_launch<convmod_bwd_weight_kernel<T_, decltype(kb)::value>>(grid, dim3(256), 0, stream, (const T_*)dv, (const T_*)s,
                                                                             (const T_*)u, len, cm_tiles(T), B * cm_tiles(T), T, D, K, workspace);
    });
  });
  if (rc != ASR_OK) return rc;
  return asr_launch<convmod_wgrad_finish_kernel>(dim3((unsigned)(((K + 1) * D + 255) / 256)), dim3(256), 0, stream, (const float*)workspace, NS, D,
                                                 K, dwd, dbd);
}
