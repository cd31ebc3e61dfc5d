// Weight and bias gradients of the 3x3 convolutions of the vgg_cnn front end, straight from the NHWC tensors:
//   asr_conv3x3_wgrad_nhwc : dW = dY^T . shift(X) over the B*H*W pixels (transposing LDS reads build the pixel-major MFMA operands);
//                       per-workgroup partial dW blocks meet in a workspace and are folded in a fixed order (no atomics).
// Also the grid and workspace contract of that launch, which conv_wgrad_dma.hip (bf16, LDS-DMA pipelined) and conv_level0.hip share.
#include "conv_common.h"
#include "conv_wgrad_dma.h"

namespace {

// ================================================================================================ wgrad, NHWC native
// dW[co][ci][tap] += sum_px dY[px][co] * X[px + tap][ci]   straight from the NHWC tensors (no planar copies):
// a workgroup owns a 64(co) x 64(ci) x 9(tap) block of dW and walks 8x16-pixel patches; per patch it stages the halo
// patch of X (180 px x 64 ci) and the dY tile (128 px x 64 co) in LDS in their natural pixel-major layout and builds the
// MFMA operands (which need 8 CONSECUTIVE PIXELS per lane) with the transposing LDS read ds_read_b64_tr_b16:
//   in each 16-lane group, lane i slot j receives element (i&3) of the 8-byte row supplied by lane 4j+(i>>2)
//   (measured: tools/probes/tr_read_probe.hip), so lane i supplying &T[p0 + (i>>2)][c0 + 4*(i&3)] gets T[p0..p0+3][c0+i].
// A tap is a row offset into the halo patch, so all 9 taps reuse one staged patch: 2*64*576*128 flop per 41 KB staged.
// fp32 mode uses one 4-byte read per MFMA operand element instead (k <-> lane group, conflict free).
struct WgradNArgs {
  const void* x; const void* dy; float* dw; float* db;
  float* ws;    // optional: per-workgroup partial dW blocks [gridDim.y][gridDim.x][9][64 co][64 ci] (two-stage reduction)
  int B, H, W, Cin, Cout, tiles_h, tiles_w, npatch, patches_per_wg, nci;
  int ablate;   // tuning only (ASR_WGRAD_ABLATE): 1 = no global loads, 2 = no MFMA loop, 4 = no final atomics
};

template <typename T> struct WgPack;
template <> struct WgPack<bf16_t> {
  // pack = 8 consecutive pixels (k = 8g .. 8g+7 of a 32-pixel macro step) of channel c0 + lr
  // pixel (macro step ms, k) -> patch row 2*ms + (k >> 4), col k & 15
  template <int PITCH>
  static __device__ __forceinline__ uint4 load(const unsigned char* tile, int ms, int lr, int g, int c0, int row_pitch_px,
                                               int dy, int dx) {
    const int y = 2 * ms + (g >> 1), x = 8 * (g & 1) + (lr >> 2);
    const unsigned char* p = tile + ((y + dy) * row_pitch_px + x + dx) * PITCH + (c0 + 4 * (lr & 3)) * 2;
    const uint2 lo = asr_lds_read_tr16(p), hi = asr_lds_read_tr16(p + 4 * PITCH);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
  static constexpr int NMS = 4;      // 128 pixels / 32
};
template <> struct WgPack<float> {
  // pack element s (the s-th 16x16x4 MFMA of the macro step) <-> pixel 4*s + g of patch row ms
  template <int PITCH>
  static __device__ __forceinline__ uint4 load(const unsigned char* tile, int ms, int lr, int g, int c0, int row_pitch_px,
                                               int dy, int dx) {
    const unsigned char* p = tile + ((ms + dy) * row_pitch_px + g + dx) * PITCH + (c0 + lr) * 4;
    uint4 r;
    r.x = *reinterpret_cast<const uint32_t*>(p);
    r.y = *reinterpret_cast<const uint32_t*>(p + 4 * PITCH);
    r.z = *reinterpret_cast<const uint32_t*>(p + 8 * PITCH);
    r.w = *reinterpret_cast<const uint32_t*>(p + 12 * PITCH);
    return r;
  }
  static constexpr int NMS = 8;      // 128 pixels / 16
};

template <typename T>
__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_nhwc_kernel(WgradNArgs p) {
  constexpr int EPC = DT<T>::EPC, ESZ = (int)sizeof(T);
  constexpr int CPP = 64 / EPC;
  constexpr int PP = 64 * ESZ + 16;          // LDS pitch of one pixel's 64-channel slice
  constexpr int NX = 180 * CPP, NDY = 128 * CPP;
  constexpr int RX = (NX + 255) / 256, RDY = NDY / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sX = smem;                  // halo patch 10 x 18 pixels
  unsigned char* sD = smem + 180 * PP;       // dY tile 8 x 16 pixels
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int co0 = (blockIdx.y / p.nci) * 64, ci0 = (blockIdx.y % p.nci) * 64;
  const T* X = static_cast<const T*>(p.x);
  const T* DY = static_cast<const T*>(p.dy);
  const int p_beg = blockIdx.x * p.patches_per_wg, p_end = min(p.npatch, p_beg + p.patches_per_wg);

  f32x4_t acc[9][4];                         // [tap][co fragment]; this wave's ci fragment is `wave`
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_bias = p.db != nullptr && ci0 == 0 && wave == 0;

  u32x4_t rx[RX], rd[RDY];
  auto gload = [&](int patch) __attribute__((always_inline)) {
    int t = patch;
    const int tw = t % p.tiles_w; t /= p.tiles_w;
    const int th = t % p.tiles_h;
    const int b = t / p.tiles_h;
    const int h0 = th * 8, w0 = tw * 16;
#pragma unroll
    for (int i = 0; i < RX; ++i) {
      const int c = tid + i * 256;
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (c < NX) {
        const int hp = c / CPP, ch = c % CPP;
        const int gy = h0 + hp / 18 - 1, gx = w0 + hp % 18 - 1;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W)
          v = *reinterpret_cast<const u32x4_t*>(X + (((int64_t)b * p.H + gy) * p.W + gx) * p.Cin + ci0 + ch * EPC);
      }
      rx[i] = v;
    }
#pragma unroll
    for (int i = 0; i < RDY; ++i) {
      const int c = tid + i * 256, px = c / CPP, ch = c % CPP;
      const int gy = h0 + (px >> 4), gx = w0 + (px & 15);
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (gy < p.H && gx < p.W)
        v = *reinterpret_cast<const u32x4_t*>(DY + (((int64_t)b * p.H + gy) * p.W + gx) * p.Cout + co0 + ch * EPC);
      rd[i] = v;
    }
  };
  auto swrite = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < RX; ++i) {
      const int c = tid + i * 256;
      if (c < NX) *reinterpret_cast<u32x4_t*>(sX + (c / CPP) * PP + (c % CPP) * 16) = rx[i];
    }
#pragma unroll
    for (int i = 0; i < RDY; ++i) {
      const int c = tid + i * 256;
      *reinterpret_cast<u32x4_t*>(sD + (c / CPP) * PP + (c % CPP) * 16) = rd[i];
    }
  };

  if (p_beg < p_end) gload(p_beg);
  for (int patch = p_beg; patch < p_end; ++patch) {
    swrite();
    __syncthreads();
    if (patch + 1 < p_end && !ASR_ABL(p, 1)) gload(patch + 1);          // next patch's HBM latency hides under this patch's MFMAs
#pragma unroll 1
    for (int ms = 0; ms < (ASR_ABL(p, 2) ? 0 : WgPack<T>::NMS); ++ms) {
      uint4 a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = WgPack<T>::template load<PP>(sD, ms, lr, g, i * 16, 16, 0, 0);
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Chunk<T> c; c.v = a[i];
#pragma unroll
          for (int e = 0; e < EPC; ++e) bsum[i] += DT<T>::from(c.e[e]);
        }
      }
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const uint4 bfr = WgPack<T>::template load<PP>(sX, ms, lr, g, wave * 16, 18, t / 3, t % 3);
#pragma unroll
        for (int i = 0; i < 4; ++i) mma16<T>(acc[t][i], a[i], bfr);
      }
    }
    __syncthreads();
  }

  if (p.ws) {
    // two-stage reduction: 36,864 plain stores per workgroup instead of as many fp32 atomics on the same 147 KB of dW
    // (measured: the atomics were > 50 % of this kernel's time); wgrad_reduce_kernel folds the partial blocks into dW
    float* part = p.ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (9 * 64 * 64);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(t * 64 + i * 16 + g * 4 + r) * 64 + wave * 16 + lr] = acc[t][i][r];
  } else {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co0 + i * 16 + g * 4 + r, ci = ci0 + wave * 16 + lr;
          if (!ASR_ABL(p, 4) || acc[t][i][r] == 12345.f) atomicAdd(p.dw + ((int64_t)co * p.Cin + ci) * 9 + t, acc[t][i][r]);
        }
  }
  if (do_bias) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      // with a workspace: the slot after the partial dW blocks, folded in workgroup order (no atomics, the same bits every run)
      if (g == 0) {
        if (p.ws) p.ws[(int64_t)gridDim.x * gridDim.y * (9 * 64 * 64) + ((int64_t)(co0 / 64) * gridDim.x + blockIdx.x) * 64 + i * 16 + lr] = v;
        else atomicAdd(p.db + co0 + i * 16 + lr, v);
      }
    }
  }
}

// db[64 cob + t] += the bias partials of co block cob, in workgroup order (slots [Cout / 64][wgx][64] after the partial dW blocks)
// (256 threads: each wave adds a quarter of the workgroups with eight loads in flight, the quarters meet in LDS in wave order)
__device__ inline void wgrad_bias_fold(const float* slots, float* db, int wgx, int cob) {
  __shared__ float red[4][64];
  const int t = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int per = (wgx + 3) / 4, w0 = grp * per, w1 = min(wgx, w0 + per);
  const float* s = slots + (int64_t)cob * wgx * 64 + t;
  float acc = 0.f;
#pragma unroll 8
  for (int w = w0; w < w1; ++w) acc += s[(int64_t)w * 64];
  red[grp][t] = acc;
  __syncthreads();
  if (grp == 0) db[cob * 64 + t] += (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}
__global__ __launch_bounds__(256) void wgrad_bias_reduce_kernel(const float* __restrict__ ws, float* db, int wgx, int blocks_y) {
  wgrad_bias_fold(ws + (int64_t)wgx * blocks_y * (9 * 64 * 64), db, wgx, blockIdx.x);
}

// dW[co0+co][ci0+ci][t] += sum over this slice of the workgroup partials ws[by][wg][t][co][ci]; db (optional) += the bias partials
// No atomics (1.2 M same-line fp32 atomics were most of this kernel's time: 8 slices x 147 K elements x 4 blocks at the ~40 / ns the
// chip sustains) and a fixed summation order: a workgroup owns 256 consecutive elements, its four waves each add a quarter of the
// partial blocks with 16-byte loads (eight in flight), the quarters meet in LDS and wave 0 does the plain dw += .
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* dw, float* db, int wgx, int nci, int Cin) {
  __shared__ float4 red[4][64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  if (blockIdx.x == 9 * 64 * 64 / 256) {         // with db: one extra column of workgroups folds the bias partials
    if (blockIdx.y % nci == 0) wgrad_bias_fold(ws + (int64_t)wgx * gridDim.y * (9 * 64 * 64), db, wgx, blockIdx.y / nci);
    return;
  }
  const int e = (blockIdx.x * 64 + col) * 4;             // 4 elements of the 9 x 64 x 64 block: (t, co, ci .. ci+3), ci fastest
  const int by = blockIdx.y;
  const int per = (wgx + 3) / 4;
  const int w0 = grp * per, w1 = min(wgx, w0 + per);
  const float* src = ws + ((int64_t)by * wgx) * (9 * 64 * 64) + e;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int w = w0; w < w1; ++w) {
    const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)w * (9 * 64 * 64));
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  red[grp][col] = acc;
  __syncthreads();
  if (grp != 0) return;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const float4 v = red[k][col];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  const int ci = e & 63, co = (e >> 6) & 63, t = e >> 12;
  const int co0 = (by / nci) * 64, ci0 = (by % nci) * 64;
  float* dst = dw + ((int64_t)(co0 + co) * Cin + ci0 + ci) * 9 + t;
  dst[0] += acc.x; dst[9] += acc.y; dst[18] += acc.z; dst[27] += acc.w;
}

}  // namespace

// workgroups along the pixel axis (x) and dW blocks (y) of the NHWC weight-gradient launch.  ONE definition (declared in
// conv_wgrad_dma.h): conv_level0.hip writes partial blocks on this grid and asr_conv3x3_wgrad_reduce folds them on it.
void asr_conv3x3_wgrad_grid(int B, int H, int W, int Cin, int Cout, int* wgx, int* blocks_y, int* patches_per_wg) {
  const int npatch = B * ((H + 7) / 8) * ((W + 15) / 16);
  *blocks_y = (Cout / 64) * (Cin / 64);
  int gx = 512 / *blocks_y;                         // ~2 workgroups per CU in flight
  if (gx < 1) gx = 1;
  int ppw = (npatch + gx - 1) / gx;
  if (ppw < 4) ppw = 4;
  *patches_per_wg = ppw;
  *wgx = (npatch + ppw - 1) / ppw;
}

extern "C" int64_t asr_conv3x3_wgrad_workspace(int B, int H, int W, int Cin, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin % 64 != 0 || Cout % 64 != 0) return 0;
  int wgx, by, ppw;
  asr_conv3x3_wgrad_grid(B, H, W, Cin, Cout, &wgx, &by, &ppw);
  return (int64_t)wgx * by * 9 * 64 * 64 + (int64_t)wgx * Cout;      // partial dW blocks + bias partials
}

namespace {
// the fold alone, on the grid above; the caller holds the profiling scope
int wgrad_reduce_launch(const float* ws, float* dw, float* db, int wgx, int blocks_y, int Cin, hipStream_t s) {
  return asr_launch<wgrad_reduce_kernel>(dim3(9 * 64 * 64 / 256 + (db ? 1 : 0), (unsigned)blocks_y), dim3(256), 0, s, ws, dw, db, wgx, Cin / 64,
                                         Cin);
}

int conv3x3_wgrad_impl(const void* x, const void* dy, float* dw, float* db, float* workspace, int64_t workspace_floats, int B, int H,
                       int W, int Cin, int Cout, int dtype, bool reduce, hipStream_t s) {
  ASR_CHECK_ARG(x && dy && dw && B >= 0 && H > 0 && W > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (Cin % 64 != 0 || Cout % 64 != 0 || !aligned16(x) || !aligned16(dy)) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  WgradNArgs p{};
  p.x = x; p.dy = dy; p.dw = dw; p.db = db;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.tiles_h = (H + 7) / 8; p.tiles_w = (W + 15) / 16;
  p.npatch = B * p.tiles_h * p.tiles_w;
  p.nci = Cin / 64;
#ifdef ASR_TUNE_ABLATE
  p.ablate = (int)asr_tuning("WGRAD_ABLATE", 0);
#endif
  int wgx, blocks_y;
  asr_conv3x3_wgrad_grid(B, H, W, Cin, Cout, &wgx, &blocks_y, &p.patches_per_wg);
  p.ws = (workspace && workspace_floats >= (int64_t)wgx * blocks_y * 9 * 64 * 64 + (int64_t)wgx * Cout) ? workspace : nullptr;
  const int esz = dtype == ASR_F32 ? 4 : 2;
  const size_t lds = (size_t)(180 + 128) * (64 * esz + 16);
  AsrProfScope prof(ASR_OP_CONV_WGRAD, s);
  // bf16 with a workspace: the LDS-DMA pipelined kernel (conv_wgrad_dma.hip); same grid, same partial-block layout
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  int rc;
  if (dtype == ASR_BF16 && p.ws && (int64_t)B * H * W * cmax * 2 < ((int64_t)1 << 32)) {
    WgdArgs q{};
    q.x = static_cast<const bf16_t*>(x); q.dy = static_cast<const bf16_t*>(dy); q.db = db; q.ws = p.ws;
    q.B = B; q.H = H; q.W = W; q.Cin = Cin; q.Cout = Cout; q.tiles_h = p.tiles_h; q.tiles_w = p.tiles_w;
    q.npatch = p.npatch; q.patches_per_wg = p.patches_per_wg; q.nci = p.nci;
    rc = asr_conv3x3_wgrad_dma_launch(q, (unsigned)wgx, (unsigned)blocks_y, s);
  } else {
    rc = asr_with_dtype(dtype, [&](auto t) {
      return asr_launch<conv3x3_wgrad_nhwc_kernel<decltype(t)>>(dim3((unsigned)wgx, (unsigned)blocks_y), dim3(256), lds, s, p);
    });
  }
  if (rc != ASR_OK) return rc;
  if (p.ws && reduce) return wgrad_reduce_launch(p.ws, dw, db, wgx, blocks_y, Cin, s);
  // partials only: the bias partials are folded now, dW waits for asr_conv3x3_wgrad_reduce
  if (p.ws && db) return asr_launch<wgrad_bias_reduce_kernel>(dim3((unsigned)(Cout / 64)), dim3(256), 0, s, (const float*)p.ws, db, wgx, blocks_y);
  return ASR_OK;
}
}  // namespace

// dw += the partial blocks and, with db, db += the bias partials (conv_level0.hip's weight gradient: one launch for both)
int asr_conv3x3_wgrad_fold(const float* workspace, float* dw, float* db, int B, int H, int W, int Cin, int Cout, hipStream_t s) {
  ASR_CHECK_ARG(workspace && dw && B >= 0 && H > 0 && W > 0);
  if (Cin % 64 != 0 || Cout % 64 != 0) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  int wgx, blocks_y, ppw;
  asr_conv3x3_wgrad_grid(B, H, W, Cin, Cout, &wgx, &blocks_y, &ppw);
  AsrProfScope prof(ASR_OP_CONV_WGRAD, s);
  return wgrad_reduce_launch(workspace, dw, db, wgx, blocks_y, Cin, s);
}

extern "C" int asr_conv3x3_wgrad_nhwc(const void* x, const void* dy, float* dw, float* db, float* workspace,
                                      int64_t workspace_floats, int B, int H, int W, int Cin, int Cout, int dtype, hipStream_t s) {
  return conv3x3_wgrad_impl(x, dy, dw, db, workspace, workspace_floats, B, H, W, Cin, Cout, dtype, true, s);
}
// first stage only: the per-workgroup partial dW blocks stay in `workspace` (required) until asr_conv3x3_wgrad_reduce
extern "C" int asr_conv3x3_wgrad_partials(const void* x, const void* dy, float* db, float* workspace, int64_t workspace_floats, int B,
                                          int H, int W, int Cin, int Cout, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(workspace && workspace_floats >= asr_conv3x3_wgrad_workspace(B, H, W, Cin, Cout));
  if (asr_conv3x3_wgrad_workspace(B, H, W, Cin, Cout) == 0) return ASR_EUNSUPPORTED;
  return conv3x3_wgrad_impl(x, dy, workspace /* dw is not touched without the reduction */, db, workspace, workspace_floats, B, H, W,
                            Cin, Cout, dtype, false, s);
}
// second stage: dw += the partial blocks of asr_conv3x3_wgrad_partials (same geometry arguments)
extern "C" int asr_conv3x3_wgrad_reduce(const float* workspace, float* dw, int B, int H, int W, int Cin, int Cout, hipStream_t s) {
  return asr_conv3x3_wgrad_fold(workspace, dw, nullptr, B, H, W, Cin, Cout, s);
}
