// conv.0 of the vgg_cnn front end (reference: models/asr/transformer.py:43-44): one input channel, so no implicit GEMM -- HBM-bound
// streaming kernels on the vector ALU (forward + ReLU, weight / bias gradient; bf16 with 64 channels: conv1_wgrad_mfma.hip).
#include "common.h"
#include "conv1_wgrad_mfma.h"

namespace {

// Direct convolution on the vector ALU, HBM bound (528 MB of bf16 activations written / read at B = 32).  A thread owns EPC
// output channels (taps + bias in registers) and walks QUADS of 4 horizontally adjacent pixels: the 3 x 6 input window of a
// quad is loaded once (4.5 instead of 9 input loads per pixel, bounds handled by clamped addresses + selects), channel
// pairs are packed fp32 (v_pk_fma_f32).  The C0/EPC threads of a quad are adjacent lanes, so a pixel's NHWC row is one
// contiguous C0*sizeof(T) run.
constexpr int C1_PW = 4;

__device__ __forceinline__ void conv1_window(const float* __restrict__ x, int64_t b, int yh, int x0, int H, int W,
                                             float (*in)[C1_PW + 2]) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = yh + ky - 1;
    const bool rowok = yy >= 0 && yy < H;
    const float* xr = x + (b * H + (rowok ? yy : yh)) * (int64_t)W;
#pragma unroll
    for (int k = 0; k < C1_PW + 2; ++k) {
      const int xx = x0 + k - 1;
      const bool ok = rowok && xx >= 0 && xx < W;
      const float v = xr[xx < 0 ? 0 : (xx < W ? xx : W - 1)];
      in[ky][k] = ok ? v : 0.f;
    }
  }
}

// The two halves of conv1_window: the clamped loads alone (issued early), and the zeroing of out-of-image taps (applied when the
// values are consumed) -- a select right behind the load would make the compiler wait for the load where it is issued.
__device__ __forceinline__ void conv1_window_load(const float* __restrict__ x, int64_t b, int yh, int x0, int H, int W,
                                                  float (*raw)[C1_PW + 2]) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = yh + ky - 1;
    const float* xr = x + (b * H + ((yy >= 0 && yy < H) ? yy : yh)) * (int64_t)W;
#pragma unroll
    for (int k = 0; k < C1_PW + 2; ++k) {
      const int xx = x0 + k - 1;
      raw[ky][k] = xr[xx < 0 ? 0 : (xx < W ? xx : W - 1)];
    }
  }
}
__device__ __forceinline__ void conv1_window_mask(int yh, int x0, int H, int W, const float (*raw)[C1_PW + 2], float (*in)[C1_PW + 2]) {
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = yh + ky - 1;
    const bool rowok = yy >= 0 && yy < H;
#pragma unroll
    for (int k = 0; k < C1_PW + 2; ++k) {
      const int xx = x0 + k - 1;
      in[ky][k] = (rowok && xx >= 0 && xx < W) ? raw[ky][k] : 0.f;
    }
  }
}

// FULL: W is a multiple of the quad width, every quad stores exactly C1_PW chunks -- the compiler then KNOWS how many stores follow
// the prefetch loads and can wait for the loads alone (s_waitcnt vmcnt(C1_PW)); behind a conditional store it has to assume none.
template <typename T, bool FULL>
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, T* __restrict__ y, int B, int H,
                                                        int W, int C0) {
  constexpr int EPC = DT<T>::EPC, NP = EPC / 2;
  const int groups = C0 / EPC;                // 256 % groups == 0
  const int cg = threadIdx.x % groups;
  asr_f32x2_t wr[NP][9], br[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    br[j] = asr_f32x2_t{bias[cg * EPC + 2 * j], bias[cg * EPC + 2 * j + 1]};
#pragma unroll
    for (int t = 0; t < 9; ++t) wr[j][t] = asr_f32x2_t{w[(cg * EPC + 2 * j) * 9 + t], w[(cg * EPC + 2 * j + 1) * 9 + t]};
  }
  // a block walks whole image rows (b, yh); its threads cover the row's quads: no 64-bit division per work item (an emulated
  // int64 div/mod costs more instructions than the 288 FMAs of a quad)
  const int wq = (W + C1_PW - 1) / C1_PW;
  const int qpb = 256 / groups;
  // the weights have landed before the loops start: left pending, their first use INSIDE the quad loop carries an
  // s_waitcnt vmcnt(<prefetch loads>) that every iteration then pays by waiting for the previous iteration's stores
#pragma unroll
  for (int j = 0; j < NP; ++j) {             // (an empty asm that "reads" every weight register: the waits happen here)
    asm volatile("" ::"v"(br[j][0]), "v"(br[j][1]));
#pragma unroll
    for (int t = 0; t < 9; ++t) asm volatile("" ::"v"(wr[j][t][0]), "v"(wr[j][t][1]));
  }
  for (int row = blockIdx.x; row < B * H; row += gridDim.x) {
   const int yh = row % H;
   const int64_t b = row / H;
   // The NEXT quad's window is loaded before this quad's stores are issued: loads and stores retire through one in-order counter
   // (vmcnt), so a window loaded AFTER the stores could only be waited for together with them -- every iteration then exposed a
   // full store round trip to HBM and the 60 us of arithmetic never overlapped the 114 us of stores.
   float in[3][C1_PW + 2], nxt[3][C1_PW + 2];
   int qx = threadIdx.x / groups;
   if (qx < wq) conv1_window(x, b, yh, qx * C1_PW, H, W, in);
   for (; qx < wq; qx += qpb) {
    const int x0 = qx * C1_PW;
    const int qn = min(qx + qpb, wq - 1);            // always issued (clamped): no branch between the prefetch and the stores
    conv1_window_load(x, b, yh, qn * C1_PW, H, W, nxt);
    __builtin_amdgcn_sched_barrier(0);               // (the scheduler otherwise sinks the loads below the first stores)
#pragma unroll
    for (int px = 0; px < C1_PW; ++px) {
      if (!FULL && x0 + px >= W) break;
      Chunk<T> o;
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        asr_f32x2_t a = br[j];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float v = in[ky][px + kx];
            a += wr[j][ky * 3 + kx] * asr_f32x2_t{v, v};
          }
        o.e[2 * j] = DT<T>::to(fmaxf(a[0], 0.f));
        o.e[2 * j + 1] = DT<T>::to(fmaxf(a[1], 0.f));
      }
      *reinterpret_cast<uint4*>(y + (((b * H + yh) * (int64_t)W) + x0 + px) * C0 + cg * EPC) = o.v;
    }
    __builtin_amdgcn_sched_barrier(0);               // consume the prefetch only here: C1_PW stores are younger, s_waitcnt vmcnt(C1_PW) suffices
    conv1_window_mask(yh, qn * C1_PW, H, W, nxt, in);
   }
  }
}

// dw[c][tap] += sum_px dy[px][c] * x[px + tap], db[c] += sum_px dy[px][c]: same quad walk, per-thread accumulators for
// its EPC channels, then LDS atomics per block and one global atomic per (block, element).
template <typename T>
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ dy,
                                                          float* dw, float* db, int B, int H, int W, int C0) {
  constexpr int EPC = DT<T>::EPC, NP = EPC / 2;
  extern __shared__ float sacc[];     // [C0*10]
  for (int i = threadIdx.x; i < C0 * 10; i += 256) sacc[i] = 0.f;
  __syncthreads();
  const int groups = C0 / EPC;        // 256 % groups == 0 -> a thread keeps its channel group across the loop
  const int cg = threadIdx.x % groups;
  asr_f32x2_t aw[NP][9], ab[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    ab[j] = asr_f32x2_t{0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) aw[j][t] = asr_f32x2_t{0.f, 0.f};
  }
  const int wq = (W + C1_PW - 1) / C1_PW;
  const int qpb = 256 / groups;
  for (int row = blockIdx.x; row < B * H; row += gridDim.x) {
   const int yh = row % H;
   const int64_t b = row / H;
   for (int qx = threadIdx.x / groups; qx < wq; qx += qpb) {
    const int x0 = qx * C1_PW;
    Chunk<T> d[C1_PW];
#pragma unroll
    for (int px = 0; px < C1_PW; ++px) {          // unconditional loads (clamped address + select): one round trip for all
      const int xx = x0 + px < W ? x0 + px : W - 1;
      const uint4 v = *reinterpret_cast<const uint4*>(dy + (((b * H + yh) * (int64_t)W) + xx) * C0 + cg * EPC);
      d[px].v = x0 + px < W ? v : make_uint4(0u, 0u, 0u, 0u);
    }
    float in[3][C1_PW + 2];
    conv1_window(x, b, yh, x0, H, W, in);
#pragma unroll
    for (int px = 0; px < C1_PW; ++px)
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const asr_f32x2_t g = asr_f32x2_t{DT<T>::from(d[px].e[2 * j]), DT<T>::from(d[px].e[2 * j + 1])};
        ab[j] += g;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float v = in[ky][px + kx];
            aw[j][ky * 3 + kx] += g * asr_f32x2_t{v, v};
          }
      }
   }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = cg * EPC + 2 * j + h;
      atomicAdd(&sacc[C0 * 9 + c], ab[j][h]);
#pragma unroll
      for (int t = 0; t < 9; ++t) atomicAdd(&sacc[c * 9 + t], aw[j][t][h]);
    }
  __syncthreads();
  for (int i = threadIdx.x; i < C0 * 10; i += 256) {
    if (i < C0 * 9) atomicAdd(dw + i, sacc[i]);
    else atomicAdd(db + (i - C0 * 9), sacc[i]);
  }
}

}  // namespace

extern "C" int asr_conv1_fwd(const float* x, const float* w, const float* bias, void* y, int B, int H, int W, int C0, int dtype,
                             hipStream_t s) {
  ASR_CHECK_ARG(x && w && bias && y && B >= 0 && H > 0 && W > 0 && C0 > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  const int epc = dtype == ASR_F32 ? 4 : 8;
  if (C0 % epc != 0 || !aligned16(y)) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  if (256 % (C0 / epc) != 0) return ASR_EUNSUPPORTED;
  int64_t rows = (int64_t)B * H;                                          // blocks walk image rows
  ASR_CHECK_ARG(rows < ((int64_t)1 << 31));
  unsigned grid1 = (unsigned)(rows < 8192 ? rows : 8192);
  AsrProfScope prof(ASR_OP_CONV1, s);
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (W % C1_PW == 0) return asr_launch<conv1_fwd_kernel<T, true>>(dim3(grid1), dim3(256), 0, s, x, w, bias, (T*)y, B, H, W, C0);
    return asr_launch<conv1_fwd_kernel<T, false>>(dim3(grid1), dim3(256), 0, s, x, w, bias, (T*)y, B, H, W, C0);
  });
}

extern "C" int asr_conv1_wgrad(const float* x, const void* dy, float* dw, float* db, int B, int H, int W, int C0, int dtype,
                               hipStream_t s) {
  ASR_CHECK_ARG(x && dy && dw && db && B >= 0 && H > 0 && W > 0 && C0 > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  const int epc = dtype == ASR_F32 ? 4 : 8;
  if (C0 % epc != 0 || 256 % (C0 / epc) != 0 || !aligned16(dy)) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  int64_t blocks = (int64_t)B * H;        // blocks walk image rows
  ASR_CHECK_ARG(blocks < ((int64_t)1 << 31));
  if (blocks > 1024) blocks = 1024;       // every block ends with C0*10 same-address global atomics
  if (blocks < 1) blocks = 1;
  const size_t lds = (size_t)C0 * 10 * sizeof(float);
  AsrProfScope prof(ASR_OP_CONV1, s);
  // bf16 storage, 64 channels: matrix-core kernel with the pixel as contraction index (conv1_wgrad_mfma.hip)
  if (dtype == ASR_BF16 && C0 == 64) return asr_conv1_wgrad_mfma_launch(x, (const bf16_t*)dy, dw, db, B, H, W, s);
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return asr_launch<conv1_wgrad_kernel<T>>(dim3((unsigned)blocks), dim3(256), lds, s, x, (const T*)dy, dw, db, B, H, W, C0);
  });
}
