// vgg_cnn front end (reference: models/asr/transformer.py:42-53 applied at :70-71, reshape :74-76).
// Activations are NHWC (B, H=F, W=T, C): the contraction axis of every 3x3 convolution (taps x channels) is then
// made of 9 shifted, channel-contiguous rows, i.e. an implicit GEMM whose A operand is read from ONE halo patch
// staged in LDS per workgroup.
//
//   asr_conv3x3_igemm : forward (+bias+ReLU) and dgrad (tap-flipped weights, ReLU mask of the consumer's input).
//                       MFMA-bound: 2*9*Cin*Cout flop per output pixel; HBM bytes per pixel = (Cin + Cout)*sizeof(T)
//                       (+ halo overlap 1.4x on the read side, served by L2).  This file holds the weight packers, the generic
//                       kernel and the dispatch to the shape-specific ones (conv_c64.hip, conv_ws.hip).
//   asr_conv3x3_wgrad_nhwc : conv_wgrad.hip.  conv.0 (one input channel): conv1.hip.  Max pooling: pool.hip.
#include "conv_common.h"
#include "conv_c64.h"
#include "conv_ws.h"

namespace {

// ================================================================================================ weight packing
template <typename T>
__global__ void pack_weight_kernel(const float* __restrict__ w, T* __restrict__ wk, T* __restrict__ wd, int Cout, int Cin) {
  const int64_t total = (int64_t)Cout * Cin * 9;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int tap = (int)(i % 9);
    const int ci = (int)((i / 9) % Cin);
    const int co = (int)(i / (9 * (int64_t)Cin));
    const float v = w[i];
    if (wk) DT<T>::st(wk + ((int64_t)co * 9 + tap) * Cin + ci, v);
    if (wd) DT<T>::st(wd + ((int64_t)ci * 9 + (8 - tap)) * Cout + co, v);   // tap flip: (2-ky)*3+(2-kx) = 8 - tap
  }
}

// up to 8 weight tensors in one launch (the conv stack's three packs were three 5 us launches per step)
struct PackMulti {
  const float* w[8]; void* wk[8]; void* wd[8];
  int cout[8], cin[8];
  int64_t start[9];        // element ranges of the tensors in the launch's flat index
  int n;
};
template <typename T>
__global__ void pack_weight_multi_kernel(PackMulti a) {
  const int64_t total = a.start[a.n];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) k += (j < a.n && i >= a.start[j]) ? 1 : 0;
    const int64_t e = i - a.start[k];
    const int Cin = a.cin[k], Cout = a.cout[k];
    const int tap = (int)(e % 9);
    const int ci = (int)((e / 9) % Cin);
    const int co = (int)(e / (9 * (int64_t)Cin));
    const float v = a.w[k][e];
    T* wk = static_cast<T*>(a.wk[k]);
    T* wd = static_cast<T*>(a.wd[k]);
    if (wk) DT<T>::st(wk + ((int64_t)co * 9 + tap) * Cin + ci, v);
    if (wd) DT<T>::st(wd + ((int64_t)ci * 9 + (8 - tap)) * Cout + co, v);
  }
}

// ================================================================================================ implicit GEMM 3x3
__device__ const uint4 conv_zero_page = {0u, 0u, 0u, 0u};      // source of halo pixels outside the image

struct ConvArgs {
  const void* x; const void* wk; const float* bias; const void* mask_src; void* y;
  void* pool; uint8_t* code;    // PT kernels: (B, W/2, Cout, H/2) pooled output + its selection bytes instead of y
  int xcd_order;                // consecutive tiles on one XCD (always 1: the other order lost its A/B)
  int B, H, W, Cin, Cout, relu, tiles_h, tiles_w;
  int ablate;   // tuning only (ASR_IGEMM_ABLATE in -DASR_TUNE_ABLATE builds): 1 = no patch loads, 2 = no weight loads, 4 = no stores, 8 = no MFMAs
};

// Workgroup tile = TH x 16 pixels x NCO output channels, K step = (tap, 64-channel slice).  The TH+2 x 18 halo patch of a
// channel slice is staged once and read at 9 shifted positions; the tap's weight rows are double buffered (register
// prefetch).  Waves: (TH/4) along pixel rows x WN along Cout, each wave 4 pixel-row fragments x FN = NCO/(16 WN) Cout
// fragments.  TH = 16 gives 4 x 4 (NCO 64) / 4 x 8 (NCO 128) fragments per wave: 2 / 2.7 MFMAs per LDS operand read
// instead of 1.3 / 2 with TH = 8.  What bounds the loop is instruction issue around the MFMAs (an MFMA leaves room for about two
// other vector instructions, tools/probes/mfma_valu_probe.hip; this loop carries 1.8 - 3.4) and the two barriers per tap.
template <typename T, int NCO, int TH, int TPS, int WBUF, bool PT = false>
__global__ __launch_bounds__(256) void conv3x3_igemm_kernel(ConvArgs p) {
  constexpr int EPC = DT<T>::EPC, ESZ = (int)sizeof(T);
  constexpr int CPP = 64 / EPC;            // 16-B chunks per 64-channel pixel slice
  // LDS rows (pixel slices / weight rows): unpadded rows of 64 channels, 16-B chunk c of row r in slot c ^ (r & 7) (conflict-free
  // operand reads; the image is lane-linear, so the halo patch can be filled by the LDS-DMA with the swizzle applied on the
  // source address).  fp32 rows are 256 B = 16 chunks: the XOR only permutes the low 3 bits of the chunk index.
  constexpr bool SWZ = true;
  constexpr int PP = 64 * ESZ;
#define ASR_SLOT(ROW, CH) ((SWZ ? ((CH) ^ ((ROW) & 7)) : (CH)) << 4)
  constexpr int NMS = 64 / (4 * EPC);      // macro steps per 64 channels
  constexpr int WM = TH / 4, WN = 4 / WM;  // wave grid
  constexpr int FN = NCO / (16 * WN);      // cout fragments per wave
  constexpr int WROWS = TPS * NCO;         // weight rows per step (TPS taps)
  constexpr int WCH = WROWS * CPP / 256;   // weight chunks per thread
  constexpr int SPS = (9 + TPS - 1) / TPS; // steps per 64-channel slice
  constexpr int NHALO = (TH + 2) * 18;     // halo pixels
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sP = smem;
  unsigned char* sW0 = smem + NHALO * PP;         // weight tile, buffer 0
  unsigned char* sW1 = WBUF == 2 ? sW0 + WROWS * PP : sW0;   // buffer 1 (WBUF == 1: one weight buffer, an extra barrier per step)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;
  int t = blockIdx.x, tw, th, b;
  if (PT || p.xcd_order) {
    // consecutive tile ids on ONE XCD (blockIdx is dealt round-robin over the 8 XCDs, each with its own L2): neighbouring tiles share
    // their halo rows / columns in that L2 (PMC, conv.7 forward: 167.5 -> 131.1 MB fetched)
    t = asr_xcd_linear(t, (int)gridDim.x);
  }
  if constexpr (PT) {
    // pooled epilogue: the five row tiles of a column strip each write 16 bytes of every 80-byte (column, channel) run of the encoder
    // layout.  Row tile fastest: the pieces of a cache line then meet in one L2 before it is written back, instead of five partial
    // write-backs from five L2s (PMC WRITE_SIZE 256 000 -> 100 414 KB).
    th = t % p.tiles_h; t /= p.tiles_h;
    tw = t % p.tiles_w;
    b = t / p.tiles_w;
  } else {
    tw = t % p.tiles_w; t /= p.tiles_w;
    th = t % p.tiles_h;
    b = t / p.tiles_h;
  }
  const int h0 = th * TH, w0 = tw * 16;
  const T* X = static_cast<const T*>(p.x);
  const T* Wk = static_cast<const T*>(p.wk);
  const int nchunk = p.Cin / 64;
  const int nsteps = nchunk * SPS;

  f32x4_t acc[4][FN];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // weight tile (TPS taps, 64-channel slice): global -> registers -> LDS; the register copy lives for one iteration only.
  // Row tt * NCO + co of the tile holds tap (first tap of the step + tt); a step past tap 8 loads nothing for that row.
#define ASR_WLOAD(RW, STEP)                                                                                   \
  {                                                                                                           \
    const int cc_ = (STEP) / SPS, tap0_ = ((STEP) % SPS) * TPS;                                               \
    _Pragma("unroll") for (int i = 0; i < WCH; ++i) {                                                         \
      const int c = tid + i * 256, row = c / CPP, ch = c % CPP, tt = row / NCO, co = row % NCO;               \
      if (TPS == 1 || tap0_ + tt < 9)                                                                         \
        RW[i] = *reinterpret_cast<const u32x4_t*>(Wk + ((int64_t)co * 9 + tap0_ + tt) * p.Cin + cc_ * 64 + ch * EPC); \
    }                                                                                                         \
  }
#define ASR_WWRITE(RW, DST)                                                                                   \
  {                                                                                                           \
    _Pragma("unroll") for (int i = 0; i < WCH; ++i) {                                                         \
      const int c = tid + i * 256, row = c / CPP, ch = c % CPP;                                               \
      *reinterpret_cast<u32x4_t*>((DST) + row * PP + ASR_SLOT(row, ch)) = RW[i];                                        \
    }                                                                                                         \
  }
  // halo patch of one 64-channel slice, HBM -> LDS by the LDS-DMA (no registers, one round trip): chunk c = (pixel hp, slot) of the
  // lane-linear image takes source chunk slot ^ (hp & 7); pixels outside the image are read from a 16-byte zero page.
  constexpr int PIT = (NHALO * CPP + 255) / 256;
  auto pstage = [&](int cc) __attribute__((always_inline)) {
#pragma unroll 1                         // rolled on purpose: a DMA is fire-and-forget, unrolling only pins 2 address registers per pass
    for (int it = 0; it < PIT; ++it) {
      const int c = tid + it * 256;
      if (c < NHALO * CPP) {
        const int hp = c / CPP, slot = c % CPP, ch = SWZ ? (slot ^ (hp & 7)) : slot;
        const int gy = h0 + hp / 18 - 1, gx = w0 + hp % 18 - 1;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        const T* src = in ? X + (((int64_t)b * p.H + gy) * p.W + gx) * p.Cin + cc * 64 + ch * EPC
                          : reinterpret_cast<const T*>(&conv_zero_page);       // the DMA cannot zero-fill: outside pixels read zeros
        unsigned char* dst = sP + (it * 256 + (tid & ~63)) * 16;      // wave-uniform; the DMA adds lane * 16
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
    }
  };
  {
    u32x4_t rw0[WCH];
#pragma unroll
    for (int i = 0; i < WCH; ++i) rw0[i] = u32x4_t{0u, 0u, 0u, 0u};
    ASR_WLOAD(rw0, 0)
    ASR_WWRITE(rw0, sW0)
  }
#pragma unroll 1
  for (int step = 0; step < nsteps; ++step) {
    const int sstep = step % SPS;
    if (sstep == 0) {
      if (step > 0) __syncthreads();      // everybody is done with the previous channel slice of the patch
      if (!ASR_ABL(p, 1)) pstage(step / SPS);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                     // patch + weight buffer (step&1) visible
    }
    const bool has_next = step + 1 < nsteps;
    u32x4_t rw[WCH];
#pragma unroll
    for (int i = 0; i < WCH; ++i) rw[i] = u32x4_t{0u, 0u, 0u, 0u};
    if (has_next && !ASR_ABL(p, 2)) ASR_WLOAD(rw, step + 1)
    const unsigned char* sW = (step & 1) ? sW1 : sW0;
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) {
      const int tap = sstep * TPS + tt;
      if (TPS > 1 && tap >= 9) break;
      const int dy = tap / 3, dx = tap % 3;
#pragma unroll
      for (int ms = 0; ms < NMS; ++ms) {
        uint4 a[4], bfr[FN];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int hp = (wm * 4 + i + dy) * 18 + lr + dx;
          a[i] = *reinterpret_cast<const uint4*>(sP + hp * PP + ASR_SLOT(hp, ms * 4 + g));
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int row = tt * NCO + wn * (NCO / WN) + j * 16 + lr;
          bfr[j] = *reinterpret_cast<const uint4*>(sW + row * PP + ASR_SLOT(row, ms * 4 + g));
        }
        if (!ASR_ABL(p, 8)) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) mma16<T>(acc[i][j], bfr[j], a[i]);   // D = (co rows) x (pixel columns)
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) asm volatile("" :: "v"(a[i].x));
#pragma unroll
          for (int j = 0; j < FN; ++j) asm volatile("" :: "v"(bfr[j].x));
        }
      }
    }
    if (has_next) {
      unsigned char* dst = (step & 1) ? sW0 : sW1;
      if (WBUF == 1) __syncthreads();       // single buffer: everybody must be done reading this step's weights first
      ASR_WWRITE(rw, dst)
      // the next step either re-stages the patch (last step of a slice -> barrier pair above) or needs this barrier
      if (sstep != SPS - 1) __syncthreads();
    }
  }

#undef ASR_WLOAD
#undef ASR_WWRITE
#undef ASR_SLOT

  if constexpr (PT) {
    // ---- pooled epilogue (conv.7 + ReLU + MaxPool2d + the view / transpose of transformer.py:50-52,74-76): bias + ReLU on the
    // accumulators, 2 x 2 maximum over the wave's row pairs (registers) and the lane pairs (lr, lr ^ 1: DPP), one selection byte per
    // pooled element (packed 16-bit arithmetic on the bf16 bit patterns, as in conv_c64.hip), the 8 x 8 x 128 pooled tile and its
    // bytes staged in LDS as [pooled column][channel][pooled row] so that the (B, W/2, C, H/2) output gets 16-byte runs along H/2.
    // The un-pooled output is never stored.  Launcher: bf16, 128 outputs, H and W multiples of 16.
    static_assert(!PT || (sizeof(T) == 2 && NCO == 128 && TH == 16 && WM == 4), "pooled epilogue: bf16, 128 channels, 16-row tile");
    __syncthreads();                       // every wave is done with the operand tiles
    bf16_t* sPool = reinterpret_cast<bf16_t*>(smem);
    uint8_t* sCode = smem + 8 * 128 * 8 * 2;
    const bool odd = (lr & 1) != 0;
    const uint32_t one = 0x00010001u;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const f32x4_t bvj = p.bias ? *reinterpret_cast<const f32x4_t*>(p.bias + j * 16 + 4 * g) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        uint32_t mx[2], cd[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const f32x4_t x0 = acc[2 * pr][j] + bvj, x1 = acc[2 * pr + 1][j] + bvj;
          const uint32_t mine0 = (uint32_t)f32_to_bf16(fmaxf(x0[2 * d], 0.f)) | ((uint32_t)f32_to_bf16(fmaxf(x0[2 * d + 1], 0.f)) << 16);
          const uint32_t mine1 = (uint32_t)f32_to_bf16(fmaxf(x1[2 * d], 0.f)) | ((uint32_t)f32_to_bf16(fmaxf(x1[2 * d + 1], 0.f)) << 16);
          const uint32_t oth0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine0, 0xB1, 0xf, 0xf, true);      // lane ^ 1
          const uint32_t oth1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine1, 0xB1, 0xf, 0xf, true);
          const uint32_t v0 = odd ? oth0 : mine0, v1 = odd ? mine0 : oth0, v2 = odd ? oth1 : mine1, v3 = odd ? mine1 : oth1;
          uint32_t m = v0;
          asm("v_pk_max_u16 %0, %0, %1" : "+v"(m) : "v"(v1));
          asm("v_pk_max_u16 %0, %0, %1" : "+v"(m) : "v"(v2));
          asm("v_pk_max_u16 %0, %0, %1" : "+v"(m) : "v"(v3));
          uint32_t n0 = v0 ^ m, n1 = v1 ^ m, n2 = v2 ^ m, nz = m;
          asm("v_pk_min_u16 %0, %0, %1" : "+v"(n0) : "v"(one));
          asm("v_pk_min_u16 %0, %0, %1" : "+v"(n1) : "v"(one));
          asm("v_pk_min_u16 %0, %0, %1" : "+v"(n2) : "v"(one));
          asm("v_pk_min_u16 %0, %0, %1" : "+v"(nz) : "v"(one));
          const uint32_t n01 = n0 & n1, n012 = n01 & n2;
          uint32_t c = one + n0 + n01 + n012;
          asm("v_pk_mul_lo_u16 %0, %0, %1" : "+v"(c) : "v"(nz));
          mx[d] = m; cd[d] = c;
        }
        if (!odd) {
          const int base = (((lr >> 1) * 128 + j * 16 + 4 * g) * 8) + wave * 2 + pr;       // [pooled column][channel][pooled row]
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            sPool[base + (2 * d) * 8] = (bf16_t)(mx[d] & 0xffffu);
            sPool[base + (2 * d + 1) * 8] = (bf16_t)(mx[d] >> 16);
            sCode[base + (2 * d) * 8] = (uint8_t)(cd[d] & 0xffu);
            sCode[base + (2 * d + 1) * 8] = (uint8_t)((cd[d] >> 16) & 0xffu);
          }
        }
      }
    __syncthreads();
    const int H2 = p.H >> 1, W2 = p.W >> 1;
    bf16_t* out = static_cast<bf16_t*>(p.pool);
    for (int c = tid; c < 8 * 128; c += 256) {
      const int owl = c >> 7, ch = c & 127;
      const int64_t gi = (((int64_t)b * W2 + (w0 >> 1) + owl) * 128 + ch) * H2 + (h0 >> 1);
      *reinterpret_cast<uint4*>(out + gi) = *reinterpret_cast<const uint4*>(sPool + c * 8);
      *reinterpret_cast<uint2*>(p.code + gi) = *reinterpret_cast<const uint2*>(sCode + c * 8);
    }
    return;
  }
  // ---- epilogue straight from the accumulators (operands were swapped: a fragment is (16 co rows) x (16 pixel columns), so a
  // lane holds 4 consecutive output channels of ONE pixel).  bias / ReLU in fp32, then the storage dtype; bf16 lanes exchange
  // halves with the neighbouring lane group (v_permlane16_swap) so that every lane owns one aligned 16-byte chunk of a pixel's
  // NHWC row: no LDS staging, no barrier, 64 contiguous bytes per pixel per store instruction.
  T* Y = static_cast<T*>(p.y);
  const T* Msk = static_cast<const T*>(p.mask_src);
  const int gx = w0 + lr;
  constexpr int NJ = ESZ == 2 ? FN / 2 : FN;        // chunks per pixel fragment and lane
  // channel of the lane's chunk q: bf16 pairs fragments (2q, 2q+1) -- even lane groups end up with 8 channels of 2q, odd ones of 2q+1
  int cho[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q)
    cho[q] = wn * (NCO / WN) + (ESZ == 2 ? (2 * q + (g & 1)) * 16 + 4 * (g & 2) : q * 16 + 4 * g);
  u32x4_t mk[4][NJ];
  if (Msk) {                                        // all mask chunks first (clamped addresses): one memory round trip
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gy = min(h0 + wm * 4 + i, p.H - 1);
      const T* mrow = Msk + (((int64_t)b * p.H + gy) * p.W + min(gx, p.W - 1)) * p.Cout;
#pragma unroll
      for (int q = 0; q < NJ; ++q) mk[i][q] = *reinterpret_cast<const u32x4_t*>(mrow + cho[q]);
    }
  }
  f32x4_t bv[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j)
    bv[j] = p.bias ? *reinterpret_cast<const f32x4_t*>(p.bias + wn * (NCO / WN) + j * 16 + 4 * g) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gy = h0 + wm * 4 + i;
    const bool ok = gy < p.H && gx < p.W;
    T* yrow = Y + (((int64_t)b * p.H + (ok ? gy : 0)) * p.W + (ok ? gx : 0)) * p.Cout;
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      Chunk<T> o;
      if constexpr (ESZ == 2) {
        uint32_t lo[2], hi[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          f32x4_t xa = acc[i][2 * q] + bv[2 * q], xb = acc[i][2 * q + 1] + bv[2 * q + 1];
          if (p.relu) {
            xa[2 * d] = fmaxf(xa[2 * d], 0.f); xa[2 * d + 1] = fmaxf(xa[2 * d + 1], 0.f);
            xb[2 * d] = fmaxf(xb[2 * d], 0.f); xb[2 * d + 1] = fmaxf(xb[2 * d + 1], 0.f);
          }
          const uint32_t pa = (uint32_t)DT<T>::to(xa[2 * d]) | ((uint32_t)DT<T>::to(xa[2 * d + 1]) << 16);
          const uint32_t pb = (uint32_t)DT<T>::to(xb[2 * d]) | ((uint32_t)DT<T>::to(xb[2 * d + 1]) << 16);
          // (a, b) -> a' = {a.row0, b.row0, a.row2, b.row2}, b' = {a.row1, b.row1, a.row3, b.row3}
          auto sw = __builtin_amdgcn_permlane16_swap(pa, pb, false, false);
          lo[d] = sw[0]; hi[d] = sw[1];
        }
        o.v = make_uint4(lo[0], lo[1], hi[0], hi[1]);
      } else {
        f32x4_t x = acc[i][q] + bv[q];
        if (p.relu) { x[0] = fmaxf(x[0], 0.f); x[1] = fmaxf(x[1], 0.f); x[2] = fmaxf(x[2], 0.f); x[3] = fmaxf(x[3], 0.f); }
        o.v = __builtin_bit_cast(uint4, x);
      }
      if (Msk) {
        Chunk<T> m;
        m.v = __builtin_bit_cast(uint4, mk[i][q]);
#pragma unroll
        for (int e = 0; e < EPC; ++e)
          if (!(DT<T>::from(m.e[e]) > 0.f)) o.e[e] = DT<T>::to(0.f);
      }
      if (ok && !ASR_ABL(p, 4)) *reinterpret_cast<uint4*>(yrow + cho[q]) = o.v;
    }
  }
}
template <typename T, int NCO, int TH, int TPS, int WBUF, bool PT = false>
int launch_igemm_t(const ConvArgs& a, hipStream_t s) {
  ConvArgs p = a;
  p.tiles_h = (p.H + TH - 1) / TH;
  p.tiles_w = (p.W + 15) / 16;
  p.xcd_order = 1;
  const size_t lds = (size_t)((TH + 2) * 18 + WBUF * TPS * NCO) * (64 * sizeof(T));      // (>= the 24 KB the pooled epilogue stages)
  return asr_launch<conv3x3_igemm_kernel<T, NCO, TH, TPS, WBUF, PT>>(dim3((unsigned)(p.B * p.tiles_h * p.tiles_w)), dim3(256), lds, s, p);
}
// Tile height: 16 rows in bf16 (wave tile 4 x 4 / 4 x 8 fragments: 2 / 2.7 MFMAs per LDS operand read), 8 rows in fp32 (LDS).
// History of this choice: with register-staged patches and double-buffered weights the 16-row tile LOST to the 8-row one (a
// workgroup per CU less); once the patch came in by LDS-DMA, the weights were single buffered and the mask loads of the epilogue
// hoisted, it wins on every layer (profiles/r01_microbench_v7.txt).  Two taps per step at Cout 64 with the 8-row tile measured slower.
// Weights are SINGLE buffered in LDS (prefetched in registers): one more barrier per step, but one more workgroup per CU --
// +9 % (Cout 64) to +23 % (Cout 128) measured.  At the 16-row tile two weight buffers or two taps per step still leave two workgroups
// per CU (74 KB each) -- and change nothing: 307 - 313 us on the 128 -> 128 layer whichever way (profiles/r03_igemm_variants_ab.txt).
template <typename T, int NCO>
int launch_igemm(const ConvArgs& a, hipStream_t s) {
  return launch_igemm_t<T, NCO, sizeof(T) == 2 ? 16 : 8, 1, 1>(a, s);
}

// The launcher arguments of conv_c64.hip / conv_ws.hip from an entry point's: what every arm fills; pool, code and bits are the caller's.
C64Args c64_args(const void* x, const void* wk, const float* bias, const void* mask, void* y, int B, int H, int W, int relu) {
  C64Args a{};
  a.x = static_cast<const bf16_t*>(x); a.wk = static_cast<const bf16_t*>(wk); a.bias = bias;
  a.mask = static_cast<const bf16_t*>(mask); a.y = static_cast<bf16_t*>(y);
  a.B = B; a.H = H; a.W = W; a.relu = relu;
  return a;
}
WsArgs ws_args(const void* x, const void* wk, const float* bias, const void* mask, void* y, int B, int H, int W, int Cin, int Cout, int relu) {
  WsArgs a{};
  a.x = static_cast<const bf16_t*>(x); a.wk = static_cast<const bf16_t*>(wk); a.bias = bias;
  a.mask = static_cast<const bf16_t*>(mask); a.y = static_cast<bf16_t*>(y);
  a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.relu = relu;
  return a;
}

/* conv.2 + ReLU with its 2x2/2 max-pool from the same epilogue: pool (B, H/2, W/2, Cout); with `code`, one selection byte per pooled element
 * (layout of pool; asr_maxpool_bwd_code consumes it) and y may be null (not stored) -- what the training step needs of conv.2: its un-pooled
 * output is only ever read to find the arg max again. */
int conv3x3_relu_pool_impl(const void* x, const void* wk, const float* bias, void* y, void* pool, uint8_t* code, int B, int H, int W,
                           int Cin, int Cout, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  // only the layer that has it in the model: bf16, 64 -> 64 channels (conv_c64.hip); callers fall back to conv + asr_maxpool_fwd{,_code}
  if (dtype != ASR_BF16 || Cin != 64 || Cout != 64 || !aligned16(x) || !aligned16(wk) || (y && !aligned16(y)) || !aligned16(pool) ||
      (((uintptr_t)code) & 7) != 0 || (int64_t)B * H * W * 128 >= ((int64_t)1 << 32))
    return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_CONV_IGEMM, s);
  C64Args a = c64_args(x, wk, bias, nullptr, y, B, H, W, 1);
  a.pool = static_cast<bf16_t*>(pool); a.code = code;
  return asr_conv3x3_c64_launch(a, s);
}
}  // namespace

extern "C" int asr_conv_pack_weight(const float* w, void* wk, void* wd, int Cout, int Cin, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(w && (wk || wd) && Cout > 0 && Cin > 0);
  const int64_t total = (int64_t)Cout * Cin * 9;
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return asr_launch<pack_weight_kernel<T>>(dim3(stream_grid(total)), dim3(256), 0, s, w, (T*)wk, (T*)wd, Cout, Cin);
  });
}

extern "C" int asr_conv_pack_weight_multi(int n, const float* const* w, void* const* wk, void* const* wd, const int* Cout, const int* Cin,
                                          int dtype, hipStream_t s) {
  ASR_CHECK_ARG(n >= 0 && n <= 8 && (n == 0 || (w && wk && wd && Cout && Cin)));
  if (n == 0) return ASR_OK;
  PackMulti a{};
  a.n = n;
  int64_t total = 0;
  for (int k = 0; k < n; ++k) {
    ASR_CHECK_ARG(w[k] && (wk[k] || wd[k]) && Cout[k] > 0 && Cin[k] > 0);
    a.w[k] = w[k]; a.wk[k] = wk[k]; a.wd[k] = wd[k]; a.cout[k] = Cout[k]; a.cin[k] = Cin[k];
    a.start[k] = total;
    total += (int64_t)Cout[k] * Cin[k] * 9;
  }
  for (int k = n; k <= 8; ++k) a.start[k] = total;
  return asr_with_dtype(dtype, [&](auto t) {
    return asr_launch<pack_weight_multi_kernel<decltype(t)>>(dim3(stream_grid(total)), dim3(256), 0, s, a);
  });
}

extern "C" int asr_conv3x3_igemm(const void* x, const void* wk, const float* bias, const void* mask_src, void* y, int B, int H,
                                 int W, int Cin, int Cout, int relu, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && wk && y && B >= 0 && H > 0 && W > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (Cin % 64 != 0 || (Cout != 64 && Cout != 128) || !aligned16(x) || !aligned16(wk) || !aligned16(y) ||
      (mask_src && !aligned16(mask_src))) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  ConvArgs p{};
  p.x = x; p.wk = wk; p.bias = bias; p.mask_src = mask_src; p.y = y;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
#ifdef ASR_TUNE_ABLATE
  p.ablate = (int)asr_tuning("IGEMM_ABLATE", 0);      // timing builds: the generic kernel with parts of its work left out
  const bool ablate = p.ablate != 0;
#else
  constexpr bool ablate = false;
#endif
  AsrProfScope prof(ASR_OP_CONV_IGEMM, s);
  // the 64 -> 64 channel bf16 layer (full-resolution conv2 and its dgrad) has a persistent kernel with register-resident weights
  if (dtype == ASR_BF16 && Cin == 64 && Cout == 64 && (int64_t)B * H * W * 128 < ((int64_t)1 << 32) && !ablate)
    return asr_conv3x3_c64_launch(c64_args(x, wk, bias, mask_src, y, B, H, W, relu), s);
  // 64 -> 128 channels without a mask (conv.5 forward) in ONE pass: the weight-stationary kernel of conv_ws.hip with 64 input channels
  // (a wave keeps 32 of the 128 output channels x 9 x 64 in 144 registers, two workgroups per CU, 4-row tiles; round 5).  WS64 = 0
  // (tuning): the two-pass form below
  if (dtype == ASR_BF16 && Cin == 64 && Cout == 128 && !mask_src && !ablate && asr_tuning("WS64", 1) != 0) {
    const int rc = asr_conv3x3_ws128_launch(ws_args(x, wk, bias, nullptr, y, B, H, W, 64, Cout, relu), s);
    if (rc != ASR_EUNSUPPORTED) return rc;
  }
  // 64 -> 128 channels without a mask (conv.5 forward): the same kernel once per half of the output channels -- each half's 72 KB of
  // weights sits in registers, the 64-channel input is read twice (the second time from L2 / MALL)
  if (dtype == ASR_BF16 && Cin == 64 && Cout == 128 && !mask_src && (int64_t)B * H * W * 256 < ((int64_t)1 << 32) && !ablate) {
    for (int half = 0; half < 2; ++half) {
      C64Args a = c64_args(x, wk, bias ? bias + half * 64 : nullptr, nullptr, y, B, H, W, relu);
      a.wk += (size_t)half * 64 * 9 * 64;
      a.y += half * 64; a.ypix = 256;
      const int rc = asr_conv3x3_c64_launch(a, s);
      if (rc != ASR_OK) return rc;
    }
    return ASR_OK;
  }
  // 128 input channels in bf16 (conv.7's data gradient with conv.5's ReLU mask, conv.5's data gradient): the persistent
  // weight-stationary kernel of conv_ws.hip; WS128 = 0 (tuning) or a shape outside its domain -> the generic implicit GEMM
  if (dtype == ASR_BF16 && Cin == 128 && !ablate && asr_tuning("WS128", 1) != 0) {
    const int rc = asr_conv3x3_ws128_launch(ws_args(x, wk, bias, mask_src, y, B, H, W, 128, Cout, relu), s);
    if (rc != ASR_EUNSUPPORTED) return rc;
  }
  return asr_with_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return Cout == 64 ? launch_igemm<T, 64>(p, s) : launch_igemm<T, 128>(p, s);
  });
}

extern "C" int64_t asr_relu_bits_bytes(int B, int H, int W, int C) {
  if (B < 0 || H <= 0 || W <= 0 || C != 128) return -1;
  return (int64_t)B * (2 * ((H + 7) / 8)) * ((W + 15) / 16) * (C / 32) * 256;       // one dword per (4 x 16-pixel tile, 32 channels, lane)
}

// The convolution with a ReLU mask of ONE BIT per element on either side (conv_ws.hip): bits_out -- written for this launch's ReLU output
// (conv.5 forward, bf16 64 -> 128); bits_in -- the output is zeroed where the bit is 0 (conv.7's data gradient, bf16 128 -> 128).
extern "C" int asr_conv3x3_igemm_bits(const void* x, const void* wk, const float* bias, const uint8_t* bits_in, void* y, uint8_t* bits_out,
                                      int B, int H, int W, int Cin, int Cout, int relu, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && wk && y && B >= 0 && H > 0 && W > 0);
  ASR_CHECK_ARG((bits_in != nullptr) != (bits_out != nullptr));
  if (dtype != ASR_BF16 || !aligned16(x) || !aligned16(wk) || !aligned16(y) || ((uintptr_t)bits_in & 3) || ((uintptr_t)bits_out & 3))
    return ASR_EUNSUPPORTED;
  if (bits_in ? (Cin != 128 || Cout != 128) : (Cin != 64 || Cout != 128 || !relu)) return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_CONV_IGEMM, s);
  WsArgs a = ws_args(x, wk, bias, nullptr, y, B, H, W, Cin, Cout, relu);
  a.bits_in = bits_in; a.bits_out = bits_out;
  return asr_conv3x3_ws128_launch(a, s);
}

extern "C" int asr_conv3x3_relu_pool(const void* x, const void* wk, const float* bias, void* y, void* pool, int B, int H, int W,
                                     int Cin, int Cout, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && wk && y && pool && B >= 0 && H > 0 && W > 0);
  return conv3x3_relu_pool_impl(x, wk, bias, y, pool, nullptr, B, H, W, Cin, Cout, dtype, s);
}
extern "C" int asr_conv3x3_relu_pool_code(const void* x, const void* wk, const float* bias, void* y_or_null, void* pool, uint8_t* code,
                                          int B, int H, int W, int Cin, int Cout, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && wk && pool && code && B >= 0 && H > 0 && W > 0);
  return conv3x3_relu_pool_impl(x, wk, bias, y_or_null, pool, code, B, H, W, Cin, Cout, dtype, s);
}

/* y never stored: pool (B, W/2, Cout, H/2) = the encoder layout (B, T', C F') of the 2x2/2 max-pool of ReLU(conv3x3_pad1(x; wk) + bias), and
 * one selection byte per pooled element in the same layout (conv.7 + ReLU + MaxPool2d + view / transpose, transformer.py:50-52,74-76).
 * ASR_EUNSUPPORTED unless bf16, Cout = 128, Cin a multiple of 64, H and W multiples of 16 (callers use asr_conv3x3_igemm +
 * asr_maxpool_fwd_code). */
namespace {
int conv3x3_relu_pool_tcf_code_impl(const void* x, const void* wk, const float* bias, void* pool, uint8_t* code, int code_cl, int B, int H,
                                    int W, int Cin, int Cout, int dtype, hipStream_t s) {
  ASR_CHECK_ARG(x && wk && pool && code && B >= 0 && H > 0 && W > 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (dtype != ASR_BF16 || Cout != 128 || Cin % 64 != 0 || H % 8 != 0 || W % 16 != 0 || !aligned16(x) || !aligned16(wk) || !aligned16(pool) ||
      (((uintptr_t)code) & 7) != 0)
    return ASR_EUNSUPPORTED;
  if (B == 0) return ASR_OK;
  if (Cin == 128 && H % 8 == 0 && asr_tuning("WS128", 1) != 0) {        // conv.7 forward: persistent weight-stationary kernel (conv_ws.hip)
    WsArgs a = ws_args(x, wk, bias, nullptr, nullptr, B, H, W, 128, Cout, 1);
    a.pool = static_cast<bf16_t*>(pool); a.code = code; a.code_cl = code_cl;
    AsrProfScope prof(ASR_OP_CONV_IGEMM, s);
    const int rc = asr_conv3x3_ws128_launch(a, s);
    if (rc != ASR_EUNSUPPORTED) return rc;
  }
  if (code_cl) return ASR_EUNSUPPORTED;        // channel-last selection bytes: the weight-stationary kernel only
  if (H % 16 != 0) return ASR_EUNSUPPORTED;        // the pooled epilogue of the generic kernel: 16-row tiles
  ConvArgs p{};
  p.x = x; p.wk = wk; p.bias = bias; p.pool = pool; p.code = code;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = 1;
  AsrProfScope prof(ASR_OP_CONV_IGEMM, s);
  return launch_igemm_t<bf16_t, 128, 16, 1, 1, true>(p, s);
}
}  // namespace
extern "C" int asr_conv3x3_relu_pool_tcf_code(const void* x, const void* wk, const float* bias, void* pool, uint8_t* code, int B, int H,
                                              int W, int Cin, int Cout, int dtype, hipStream_t s) {
  return conv3x3_relu_pool_tcf_code_impl(x, wk, bias, pool, code, 0, B, H, W, Cin, Cout, dtype, s);
}
extern "C" int asr_conv3x3_relu_pool_tcf_codecl(const void* x, const void* wk, const float* bias, void* pool, uint8_t* code_cl, int B, int H,
                                                int W, int Cin, int Cout, int dtype, hipStream_t s) {
  return conv3x3_relu_pool_tcf_code_impl(x, wk, bias, pool, code_cl, 1, B, H, W, Cin, Cout, dtype, s);
}
