// ================================================================================================ TN (weight gradient)
// C[N,K] += sum_m A[m,n] * B[m,k]  (+ colsum[n] += sum_m A[m,n])  with A = dY (M,N) and B = X (M,K) in their NATURAL
// row-major layouts: the contraction index m is the slow axis of both, so the MFMA operands (8 consecutive m per lane)
// are built with the transposing LDS read ds_read_b64_tr_b16 (bf16) / one 4-byte read per element (fp32) -- no
// transposed copies of the activations are ever written (reference: autograd of every nn.Linear / Conv1d(k=1) weight).
// Workgroup: 64x64 tile of C; a stage holds RM = 4 macro steps of m; wave w contracts macro step w of every stage against
// the full 64x64 tile (16 operand reads feed 16 MFMAs), the four partial tiles are summed through LDS at the end.
#include <algorithm>
#include <mutex>
#include <queue>
#include <utility>
#include <vector>
#include "common.h"
#include "gemm.h"

namespace {

template <typename T, int NBUF>
__global__ __launch_bounds__(256) void gemm_tn_kernel(TnArgs p) {
  using P = TnPack<T>;
  constexpr int ESZ = (int)sizeof(T);
  constexpr int STAGE = 2 * P::RM * P::ROWB;            // A tile + B tile
  constexpr int MS_ROWS = P::RM / 4;                    // rows of one macro step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wid = asr_xcd_linear(bid, nwg);
  const int split = wid / p.ntiles, tile = wid % p.ntiles;
  const int n0 = (tile / p.tiles_k) * 64, k0 = (tile % p.tiles_k) * 64;
  const int m_beg = split * p.m_per_split, m_end = min(p.M, m_beg + p.m_per_split);
  const int nstage = (m_end - m_beg + P::RM - 1) / P::RM;   // the last stage of the last split may be partial
  const unsigned char* A = static_cast<const unsigned char*>(p.A);
  const unsigned char* B = static_cast<const unsigned char*>(p.B);
  // column chunk (16 B) this tile may read: clamp to the operand's last whole chunk (columns past N / K are never stored)
  // (ldb < K: the rows of B are overlapping windows over one longer buffer -- the clamp is then the window's own width)
  const int a_chunks = (int)(p.lda * ESZ / 16), b_chunks = (int)((p.ldb >= p.K ? p.ldb : (int64_t)((p.K + 7) / 8 * 8)) * ESZ / 16);

  // per-thread byte offsets of its DMA chunks relative to the first row of a stage (the stage base is workgroup-uniform: the
  // loads of a whole stage then cost one scalar base update instead of ~12 vector ops of address arithmetic per chunk)
  constexpr int NIT = P::RM * P::CPR / 256;
  unsigned offA[NIT], offB[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    const int c = i * 256 + tid, row = c / P::CPR, slot = (c % P::CPR) ^ (row & 7);
    int ca = n0 * ESZ / 16 + slot; ca = ca < a_chunks ? ca : a_chunks - 1;
    int cb = k0 * ESZ / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
    offA[i] = (unsigned)(row * (int)p.lda * ESZ + ca * 16);
    offB[i] = (unsigned)(row * (int)p.ldb * ESZ + cb * 16);
  }
  auto stage = [&](int st, int buf) __attribute__((always_inline)) {
    unsigned char* s = smem + buf * STAGE;
    const int64_t mrow = m_beg + (int64_t)st * P::RM;
    if (mrow + P::RM <= p.M) {            // every row of the stage exists
      const unsigned char* ba = A + mrow * p.lda * ESZ;
      const unsigned char* bb = B + mrow * p.ldb * ESZ;
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        unsigned char* d = s + (i * 256 + wave * 64) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ba + offA[i]),
                                         (__attribute__((address_space(3))) void*)d, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bb + offB[i]),
                                         (__attribute__((address_space(3))) void*)(d + P::RM * P::ROWB), 16, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < P::RM * P::CPR / 256; ++i) {
      const int c = i * 256 + tid, row = c / P::CPR, slot = (c % P::CPR) ^ (row & 7);
      int ca = n0 * ESZ / 16 + slot; ca = ca < a_chunks ? ca : a_chunks - 1;
      int cb = k0 * ESZ / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
      // rows past M: re-read the last valid row (finite data); the A side of those rows is zeroed in LDS before use
      const int64_t gr = mrow + row < p.M ? mrow + row : (int64_t)p.M - 1;
      const unsigned char* sa = A + gr * p.lda * ESZ + (int64_t)ca * 16;
      const unsigned char* sb = B + gr * p.ldb * ESZ + (int64_t)cb * 16;
      unsigned char* d = s + (i * 256 + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sa,
                                       (__attribute__((address_space(3))) void*)d, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)sb,
                                       (__attribute__((address_space(3))) void*)(d + P::RM * P::ROWB), 16, 0, 0);
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_colsum = p.colsum != nullptr && k0 == 0;

  // NBUF == 2: the next stage's LDS-DMA overlaps this stage's MFMAs.  NBUF == 1: load, wait, compute -- half the LDS, twice the
  // workgroups per CU, and the overlap comes from the other workgroups (measured faster, like every occupancy trade here).
  if (NBUF == 2) {
    if (nstage > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  for (int st = 0; st < nstage; ++st) {
    if (NBUF == 2) {
      if (st + 1 < nstage) stage(st + 1, (st + 1) & 1);
    } else {
      stage(st, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    const int cur = NBUF == 2 ? (st & 1) : 0;
    const unsigned char* sA = smem + cur * STAGE;
    const unsigned char* sB = sA + P::RM * P::ROWB;
    const int valid = m_end - (m_beg + st * P::RM);          // rows of this stage that exist (uniform over the workgroup)
    if (valid < P::RM) {
      unsigned char* zA = smem + cur * STAGE;
      for (int c = valid * (P::ROWB / 16) + tid; c < P::RM * (P::ROWB / 16); c += 256)
        *reinterpret_cast<uint4*>(zA + c * 16) = make_uint4(0u, 0u, 0u, 0u);
      __syncthreads();
    }
    uint4 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = P::load(sA, wave * MS_ROWS, lr, g, i * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = P::load(sB, wave * MS_ROWS, lr, g, j * 16);
    if (do_colsum) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Chunk<T> c; c.v = a[i];
#pragma unroll
        for (int e = 0; e < DT<T>::EPC; ++e) bsum[i] += DT<T>::from(c.e[e]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma16<T>(acc[i][j], a[i], b[j]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- sum the four waves' partial tiles (tree, in fragment layout: lane-private slots, no index math), then wave 0 lays the
  // total out row-major for 16-byte row-contiguous accumulation into C.  32 KB of LDS instead of four 17 KB tiles.
  constexpr int CP = 64 * 4 + 16;
  float* slot = reinterpret_cast<float*>(smem);                 // [2][64 values][64 lanes]
  float (*s_col)[64] = reinterpret_cast<float (*)[64]>(smem + 2 * 64 * 64 * 4);
  if (do_colsum) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (g == 0) s_col[wave][i * 16 + lr] = v;
    }
  }
  auto put = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) slot[(sl * 64 + (i * 4 + j) * 4 + r) * 64 + lane] = acc[i][j][r];
  };
  auto add = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += slot[(sl * 64 + (i * 4 + j) * 4 + r) * 64 + lane];
  };
  if (wave & 1) put(wave >> 1);
  __syncthreads();
  if (!(wave & 1)) add(wave >> 1);
  __syncthreads();
  if (wave == 2) put(0);
  __syncthreads();
  if (wave == 0) add(0);
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<float*>(smem + (i * 16 + g * 4 + r) * CP + (j * 16 + lr) * 4) = acc[i][j][r];
  }
  __syncthreads();
  const bool single = gridDim.x == (unsigned)p.ntiles;       // no split over m: plain read-modify-write
  if (!single && p.ws) {
    // two-stage reduction: the partial tile goes to the workspace with plain coalesced stores (fp32 atomics on C cost more
    // than the MFMAs of a split), tn_reduce_kernel adds the slices into C
    float* part = p.ws + ((int64_t)split * p.ntiles + tile) * 4096;
    for (int c = tid; c < 64 * 16; c += 256) {
      const int row = c >> 4, col = (c & 15) * 4;
      *reinterpret_cast<float4*>(part + row * 64 + col) = *reinterpret_cast<const float4*>(smem + row * CP + col * 4);
    }
  } else
  for (int c = tid; c < 64 * 16; c += 256) {
    const int row = c >> 4, col = (c & 15) * 4;
    const int gn = n0 + row, gk = k0 + col;
    if (gn >= p.N || gk >= p.K) continue;
    const float4 v = *reinterpret_cast<const float4*>(smem + row * CP + col * 4);
    float* dst = p.C + (int64_t)gn * p.ldc + gk;
    const int nv = min(4, p.K - gk);
    const float vv[4] = {v.x, v.y, v.z, v.w};
    if (single && nv == 4 && ((((uintptr_t)dst) & 15) == 0)) {
      float4 o = *reinterpret_cast<float4*>(dst);
      o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
      *reinterpret_cast<float4*>(dst) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nv) { if (single) dst[e] += vv[e]; else atomicAdd(dst + e, vv[e]); }
    }
  }
  if (do_colsum && tid < 64 && n0 + tid < p.N)
    atomicAdd(p.colsum + n0 + tid, s_col[0][tid] + s_col[1][tid] + s_col[2][tid] + s_col[3][tid]);
}


// C tile += sum over the m-slices of the partial tiles written by gemm_tn_kernel
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ ws, float* C, int64_t ldc, int N, int K,
                                                        int ntiles, int tiles_k, int splits) {
  const int tile = blockIdx.x >> 2;
  const int e = ((blockIdx.x & 3) * 256 + threadIdx.x) * 4;        // 4 consecutive columns of one row of the tile
  const int row = e >> 6, col = e & 63;
  const int gn = (tile / tiles_k) * 64 + row, gk = (tile % tiles_k) * 64 + col;
  if (gn >= N || gk >= K) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sp = 0; sp < splits; ++sp) {
    const float4 t = *reinterpret_cast<const float4*>(ws + ((int64_t)sp * ntiles + tile) * 4096 + e);
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  float* dst = C + (int64_t)gn * ldc + gk;
  const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (gk + i < K) dst[i] += vv[i];
}

// ------------------------------------------------------------------------------------------------ TN, 128 x 128 tiles (bf16)
// Same contraction for the larger weight gradients.  The 64x64-tile kernel above moves 32 flop per byte through L2 (12 TB/s
// on the 2048x512 FFN gradient): this one owns a 128 x 128 block of dW per workgroup (64 flop per byte), waves in a 2 x 2 grid
// of 64 x 64 quadrants (each wave contracts EVERY row of a stage: no cross-wave reduction, the partial block goes from the
// accumulators straight to the workspace / C).  (Its single-stage form, 64 rows of m per stage with compiler-issued loads, lost
// to the pipelined one below at every shape the dispatch sends here and is gone: profiles/r02_microbench_tn.txt.)
struct Tn128Args {
  const void* A; const void* B; float* C; float* colsum; float* ws;
  int64_t lda, ldb, ldc;
  int M, N, K, m_per_split, tiles_k, ntiles;
};

// ---- pipelined: the 128 x 128 block and wave layout above, RM = 32 rows of m per stage in an NST-deep LDS ring filled
// by HAND-ISSUED LDS-DMA (inline asm: the compiler must not know a DMA is in flight, or it drains the VMEM counter in front of
// every transposing read it can see -- the reason the removed single-stage 128 x 128 kernel could not overlap its loads), counted
// s_waitcnt vmcnt, raw s_barrier.  One barrier per stage; the DMA of stage st + NST - 1 is issued right behind the barrier of
// stage st (the ring slot it overwrites was read at stage st - 1, which every wave has left).  A partial last stage reads the
// missing rows of A from a 16-byte zero page (the DMA cannot zero fill).  64 KB of LDS at NST = 4: two workgroups per CU.
__device__ __forceinline__ uint4 tn32_pack(const unsigned char* tile, int lr, int g, int c0) {
  // 8 consecutive rows 8g .. 8g+7 of column c0 + lr of a [32][128] bf16 tile (256-byte rows, chunk c of row r in slot c ^ (r & 7))
  const int row = 8 * g + (lr >> 2), col = c0 + 4 * (lr & 3);
  const int chunk = col >> 3, half = (col >> 2) & 1;
  const uint2 lo = asr_lds_read_tr16(tile + row * 256 + ((chunk ^ (row & 7)) << 4) + half * 8);
  const uint2 hi = asr_lds_read_tr16(tile + (row + 4) * 256 + ((chunk ^ ((row + 4) & 7)) << 4) + half * 8);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}

template <int NST>
__device__ __forceinline__ void tn128p_body(const Tn128Args& p, unsigned char* smem, int wid, bool single) {
  constexpr int RM = 32, ROWB = 256, TILEB = RM * ROWB, STAGEB = 2 * TILEB;       // 8 KB per operand, 16 KB per stage
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int split = wid / p.ntiles, tile = wid % p.ntiles;
  const int n0 = (tile / p.tiles_k) * 128, k0 = (tile % p.tiles_k) * 128;
  const int m_beg = split * p.m_per_split, m_end = min(p.M, m_beg + p.m_per_split);
  const int nstage = (m_end - m_beg + RM - 1) / RM;
  const unsigned char* A = static_cast<const unsigned char*>(p.A);
  const unsigned char* B = static_cast<const unsigned char*>(p.B);
  const int a_chunks = (int)(p.lda * 2 / 16), b_chunks = (int)((p.ldb >= p.K ? p.ldb : (int64_t)((p.K + 7) / 8 * 8)) * 2 / 16);

  // per-thread DMA pieces: 512 chunks per operand tile = 2 per thread; chunk c = (row, slot), source chunk slot ^ (row & 7)
  int64_t offA[2], offB[2];
  int rowi[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i * 256 + tid, row = c >> 4, slot = (c & 15) ^ (row & 7);
    int ca = n0 * 2 / 16 + slot; ca = ca < a_chunks ? ca : a_chunks - 1;       // columns past N / K are never stored
    int cb = k0 * 2 / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
    offA[i] = (int64_t)row * p.lda * 2 + (int64_t)ca * 16;
    offB[i] = (int64_t)row * p.ldb * 2 + (int64_t)cb * 16;
    rowi[i] = row;
  }
  const unsigned smem_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned wave_lds = smem_base + (unsigned)wave * 1024u;
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(&tn_zero_page);
  auto stage = [&](int st) __attribute__((always_inline)) {
    const unsigned sl = wave_lds + (unsigned)((st % NST) * STAGEB);
    const int64_t mrow = m_beg + (int64_t)st * RM;
    const unsigned char* ba = A + mrow * p.lda * 2;
    const unsigned char* bb = B + mrow * p.ldb * 2;
    const int valid = m_end - (int)mrow;                  // rows of this stage that exist (uniform)
    if (valid >= RM) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        asr_lds_dma16(sl + i * 4096, ba + offA[i]);
        asr_lds_dma16(sl + TILEB + i * 4096, bb + offB[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool in = rowi[i] < valid;
        asr_lds_dma16(sl + i * 4096, in ? ba + offA[i] : zero);
        asr_lds_dma16(sl + TILEB + i * 4096, in ? bb + offB[i] : zero);
      }
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_colsum = p.colsum != nullptr && k0 == 0 && wk == 0;

#pragma unroll
  for (int st = 0; st < NST - 1; ++st)
    if (st < nstage) stage(st);
  for (int st = 0; st < nstage; ++st) {
    // stage st has landed once at most the DMA pieces of the later stages are outstanding (4 pieces per stage and thread, in order)
    const int ahead = min(NST - 2, nstage - 1 - st);
    if (ahead >= 2) asr_wait_vmcnt<8>();
    else if (ahead == 1) asr_wait_vmcnt<4>();
    else asr_wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();              // stage st visible to every wave; every wave is done reading stage st - 1
    asm volatile("" ::: "memory");
    if (st + NST - 1 < nstage) stage(st + NST - 1);
    const unsigned char* sA = smem + (st % NST) * STAGEB;
    const unsigned char* sB = sA + TILEB;
    uint4 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = tn32_pack(sA, lr, g, wn * 64 + i * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = tn32_pack(sB, lr, g, wk * 64 + j * 16);
    if (do_colsum) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Chunk<bf16_t> c; c.v = a[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum[i] += bf16_to_f32(c.e[e]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma16<bf16_t>(acc[i][j], a[i], b[j]);
  }

  // ---- the wave's 64 x 64 quadrant: lane (lr, g) holds rows 4g..4g+3 of column lr of every fragment
  float* part = p.ws ? p.ws + ((int64_t)split * p.ntiles + tile) * 16384 : nullptr;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wn * 64 + i * 16 + g * 4 + r, gn = n0 + row;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = wk * 64 + j * 16 + lr, gk = k0 + col;
        const float v = acc[i][j][r];
        if (!single && part) part[row * 128 + col] = v;
        else if (gn < p.N && gk < p.K) {
          float* dst = p.C + (int64_t)gn * p.ldc + gk;
          if (single) *dst += v; else atomicAdd(dst, v);
        }
      }
    }
  if (do_colsum) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int gn = n0 + wn * 64 + i * 16 + lr;
      if (g == 0 && gn < p.N) atomicAdd(p.colsum + gn, v);
    }
  }
}

template <int NST>
__global__ __launch_bounds__(256, 2) void gemm_tn128p_kernel(Tn128Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wid = asr_xcd_linear(bid, nwg);
  tn128p_body<NST>(p, smem, wid, gridDim.x == (unsigned)p.ntiles);
}

__global__ __launch_bounds__(256) void tn128_reduce_kernel(const float* __restrict__ ws, float* C, int64_t ldc, int N, int K,
                                                           int ntiles, int tiles_k, int splits) {
  const int tile = blockIdx.x >> 4;
  const int e = ((blockIdx.x & 15) * 256 + threadIdx.x) * 4;       // 4 consecutive columns of one row of the 128 x 128 block
  const int row = e >> 7, col = e & 127;
  const int gn = (tile / tiles_k) * 128 + row, gk = (tile % tiles_k) * 128 + col;
  if (gn >= N || gk >= K) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sp = 0; sp < splits; ++sp) {
    const float4 t = *reinterpret_cast<const float4*>(ws + ((int64_t)sp * ntiles + tile) * 16384 + e);
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  float* dst = C + (int64_t)gn * ldc + gk;
  const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (gk + i < K) dst[i] += vv[i];
}

// slices over m: explicit, or automatic.  With a workspace the split costs one extra pass over splits*N*K floats, so the grid is
// filled to ~2 workgroups per CU; without one the slices meet in fp32 atomics and are kept to the measured optimum (<= 4).
int tn_splits(int M, int N, int K, int splits, int dtype, bool have_ws) {
  constexpr int ASR_TN_TARGET_WGS = 512;
  const int rm = dtype == ASR_F32 ? 64 : 128;
  const int ntiles = ((N + 63) / 64) * ((K + 63) / 64);
  const int stages = (M + rm - 1) / rm;
  if (splits <= 0) {
    if (have_ws) {
      splits = (ASR_TN_TARGET_WGS + ntiles / 2) / ntiles;
      if (splits > 8) splits = 8;
      while (splits > 1 && stages / splits < 4) --splits;      // at least 4 stages per slice
    } else {
      splits = (160 + ntiles - 1) / ntiles;
      if (splits > 4) splits = 4;
    }
  }
  if (splits > stages) splits = stages;
  if (splits < 1) splits = 1;
  const int sps = (stages + splits - 1) / splits;
  return (stages + sps - 1) / sps;
}

// 128 x 128-tile kernel: bf16, automatic split, a workspace, and enough 128-blocks that ~512 workgroups of >= 4 stages exist.
// Returns the number of m-slices (0 = use the 64 x 64-tile kernel).
// LDS stages of the pipelined 128 x 128 kernel, and the number of blocks from which it replaces the single-stage 64 x 64 kernel.  Measured
// (profiles/r02_microbench_tn.txt): from 64 blocks on (2048 x 512 and larger) the pipelined kernel wins
// (512 x 2048 over 6400 rows: 38.9 -> 33.8 us; 2048 x 512 over 12720 rows: 58.8 -> 47.6 us), below that its m-slices are too
// short to fill the ring and the 64 x 64 kernel's 8 workgroups per CU win (512 x 512: 19 vs 30 us).  3 stages (48 KB, 3
// workgroups per CU) tie or beat 4.
constexpr int kTnPipe = 3, kTnPipeMin = 64;

int tn128_splits(int M, int N, int K, int splits, int dtype) {
  if (dtype != ASR_BF16 || splits > 0 || N < 128 || K < 128) return 0;
  const int nt = ((N + 127) / 128) * ((K + 127) / 128);
  if (nt < kTnPipeMin) return 0;      // (the single-stage 128 x 128 kernel's own threshold was 128 blocks: above kTnPipeMin, so it never ran)
  const int stages = (M + 31) / 32;
  int sp = (512 + nt / 2) / nt;
  if (sp > 32) sp = 32;
  while (sp > 1 && stages / sp < 4) --sp;
  if (sp < 1) sp = 1;
  const int sps = (stages + sp - 1) / sp;
  return (stages + sps - 1) / sps;
}

}  // namespace

extern "C" int64_t asr_gemm_tn_workspace(int M, int N, int K, int splits, int dtype) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const int s128 = tn128_splits(M, N, K, splits, dtype);
  if (s128 > 1) return (int64_t)s128 * ((N + 127) / 128) * ((K + 127) / 128) * 16384;
  const int sp = tn_splits(M, N, K, splits, dtype, true);
  return sp > 1 ? (int64_t)sp * ((N + 63) / 64) * ((K + 63) / 64) * 4096 : 0;
}

extern "C" int asr_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, float* colsum_acc,
                           float* workspace, int64_t workspace_floats, int M, int N, int K, int splits, int dtype,
                           hipStream_t stream) {
  ASR_CHECK_ARG(A && B && C && M >= 0 && N >= 0 && K >= 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (N == 0 || K == 0 || M == 0) return ASR_OK;
  const int esz = dtype == ASR_F32 ? 4 : 2, epc = 16 / esz;
  const int rm = dtype == ASR_F32 ? 64 : 128;
  // 16-byte aligned rows; a partial last stage of m is zero-filled in LDS by the kernel
  if (lda % epc != 0 || ldb % epc != 0 || !aligned16(A) || !aligned16(B) || lda < N ||
      lda >= ((int64_t)1 << 22) || ldb >= ((int64_t)1 << 22))      // (32-bit byte offsets inside one stage of rows)
    return ASR_EUNSUPPORTED;
  {
    const int s128 = tn128_splits(M, N, K, splits, dtype);
    const int64_t need = (int64_t)s128 * ((N + 127) / 128) * ((K + 127) / 128) * 16384;
    if (s128 >= 1 && (s128 == 1 || (workspace && workspace_floats >= need))) {
      Tn128Args q{};
      q.A = A; q.B = B; q.C = C; q.colsum = colsum_acc; q.ws = s128 > 1 ? workspace : nullptr;
      q.lda = lda; q.ldb = ldb; q.ldc = ldc; q.M = M; q.N = N; q.K = K;
      q.tiles_k = (K + 127) / 128;
      q.ntiles = ((N + 127) / 128) * q.tiles_k;
      const int stages = (M + 31) / 32;
      q.m_per_split = ((stages + s128 - 1) / s128) * 32;
      AsrProfScope prof(ASR_OP_GEMM, stream);
      (void)asr_grant_lds<gemm_tn128p_kernel<kTnPipe>>(kTnPipe * 16384);
      hipLaunchKernelGGL(gemm_tn128p_kernel<kTnPipe>, dim3((unsigned)(q.ntiles * s128)), dim3(256), kTnPipe * 16384, stream, q);
      ASR_LAUNCH_CHECK();
      if (q.ws) {
        hipLaunchKernelGGL(tn128_reduce_kernel, dim3((unsigned)(q.ntiles * 16)), dim3(256), 0, stream, q.ws, C, ldc, N, K, q.ntiles,
                           q.tiles_k, s128);
        ASR_LAUNCH_CHECK();
      }
      return ASR_OK;
    }
  }
  TnArgs p{};
  p.A = A; p.B = B; p.C = C; p.colsum = colsum_acc;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  const int tiles_n = (N + 63) / 64;
  p.tiles_k = (K + 63) / 64;
  p.ntiles = tiles_n * p.tiles_k;
  const int stages = (M + rm - 1) / rm;
  const int64_t tile_floats = (int64_t)p.ntiles * 4096;
  bool have_ws = workspace != nullptr && workspace_floats >= 2 * tile_floats;
  const int want = tn_splits(M, N, K, splits, dtype, have_ws);
  if (have_ws && workspace_floats < (int64_t)want * tile_floats) have_ws = false;
  splits = have_ws ? want : tn_splits(M, N, K, splits, dtype, false);
  const int sps = (stages + splits - 1) / splits;
  p.m_per_split = sps * rm;
  p.ws = (have_ws && splits > 1) ? workspace : nullptr;
  const size_t lds_stage = (size_t)2 * rm * (64 * esz);        // one LDS stage
  const size_t lds_epi = (size_t)2 * 64 * 64 * 4 + 4 * 64 * sizeof(float);
  const size_t lds = lds_stage > lds_epi ? lds_stage : lds_epi;
  AsrProfScope prof(ASR_OP_GEMM, stream);
  const dim3 grid((unsigned)(p.ntiles * splits));
  if (dtype == ASR_F32) {
    (void)asr_grant_lds<gemm_tn_kernel<float, 1>>(80 * 1024);
    hipLaunchKernelGGL((gemm_tn_kernel<float, 1>), grid, dim3(256), lds, stream, p);
  } else {
    (void)asr_grant_lds<gemm_tn_kernel<bf16_t, 1>>(80 * 1024);
    hipLaunchKernelGGL((gemm_tn_kernel<bf16_t, 1>), grid, dim3(256), lds, stream, p);
  }
  ASR_LAUNCH_CHECK();
  if (p.ws) {
    hipLaunchKernelGGL(tn_reduce_kernel, dim3((unsigned)(p.ntiles * 4)), dim3(256), 0, stream, p.ws, C, ldc, N, K, p.ntiles, p.tiles_k,
                       splits);
    ASR_LAUNCH_CHECK();
  }
  return ASR_OK;
}

// ================================================================================================ grouped: many layers, one launch
namespace {

// ---- 256 x 256 blocks of dW, eight waves (4 x 2 grid of 64 x 128 quadrants), 32 rows of m per stage in an NST-deep ring.
// Twice the flop per staged byte of the 128 x 128 block (128 instead of 64): the grouped launch below has ~500 of them in flight
// with a contraction 1600 - 6400 rows long, so the block lives in its steady state, and what bounds the 128 x 128 form there is the
// operand traffic per MFMA (4 LDS-DMA pieces and 16 transposing reads per 16 MFMAs; here 4 pieces and 24 reads per 32).
// LDS image of an operand tile: [32 rows][32 chunks of 16 B]; chunk c of row r sits in slot c ^ key(r), key(r) = ((r & 3) | ((r >> 3)
// & 1) << 2) << 1: the 8 rows one transposing read touches (r0 .. r0+3 and r0+8 .. r0+11, 32 bytes each) land on 8 different
// 32-byte bank groups.
__device__ __forceinline__ int tn256_key(int r) { return ((r & 3) | (((r >> 3) & 1) << 2)) << 1; }
// (Round 3's loop over the same LDS image, tn256_body, was removed in round 6 with its switches TN_ROT / TN_GROUP_STAGES / TN_ROT_NST:
// this loop gives the same bits -- same DMA, same MFMA order per accumulator -- and won every measurement, profiles/r05_tn_grouped.txt.)
typedef __attribute__((ext_vector_type(2))) unsigned int tn_u32x2_t;
__device__ __forceinline__ tn_u32x2_t tn_tr_read(unsigned addr, const int off2048) {
  tn_u32x2_t v;
  if (off2048) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"(v) : "v"(addr));
  else asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
#define TN_FRAG_READ(F, ADDR) { const tn_u32x2_t lo_ = tn_tr_read(ADDR, 0), hi_ = tn_tr_read(ADDR, 1); F = u32x4_t{lo_.x, lo_.y, hi_.x, hi_.y}; }
template <int N> __device__ __forceinline__ void tn_wait_lgkm(u32x4_t& x, u32x4_t& y) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(x), "+v"(y) : "n"(N));
}
// SWAP: the fragment comes out transposed (k rows, n columns) -- a lane then holds four CONSECUTIVE k of one row of dW
template <bool SWAP> __device__ __forceinline__ void tn_mma2(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b) {
  if constexpr (SWAP) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, b), __builtin_bit_cast(bf16x8_t, a), acc, 0, 0, 0);
  else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}

#ifdef TN_TIMING        // tuning builds only (ASR_HIPCC_EXTRA=-DTN_TIMING): s_memtime stamps at the section boundaries of a stage, workgroup 0
__device__ long long tn_dbg[64];
#define TN_STAMP(K) { const long long now_ = clock64(); tsec[K] += now_ - tlast; tlast = now_; }
#else
#define TN_STAMP(K)
#endif
template <int NST, bool SWAP>
__device__ __forceinline__ void tn256r_body(const Tn128Args& p, unsigned char* smem, int tile, int m_beg, int m_end, bool single) {
  static_assert(NST == 3 || NST == 4, "ring of three or four stages");
  constexpr int RM = 32, TILEB = RM * 512, STAGEB = 2 * TILEB;
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  // every argument the loop touches, in registers before it
  const int64_t lda2 = p.lda * 2, ldb2 = p.ldb * 2;
  const int pM = p.M, pN = p.N, pK = p.K;
  const unsigned char* A = static_cast<const unsigned char*>(p.A);
  const unsigned char* B = static_cast<const unsigned char*>(p.B);
  float* const C = p.C;
  float* const colsum = p.colsum;
  const int64_t ldc = p.ldc;
  const int n0 = (tile / p.tiles_k) * 256, k0 = (tile % p.tiles_k) * 256;
  const int nstage = (m_end - m_beg + RM - 1) / RM;
  const int a_chunks = (int)(lda2 / 16), b_chunks = (int)((p.ldb >= pK ? p.ldb : (int64_t)((pK + 7) / 8 * 8)) * 2 / 16);
  asm volatile("" ::"s"(lda2), "s"(ldb2), "s"(pM), "s"(pN), "s"(pK), "s"(A), "s"(B), "s"(C), "s"(colsum), "s"(ldc), "s"(n0), "s"(k0), "s"(nstage));

  int64_t offA[2], offB[2];
  int rowi[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i * 512 + tid, row = c >> 5, slot = (c & 31) ^ tn256_key(row);
    int ca = n0 * 2 / 16 + slot; ca = ca < a_chunks ? ca : a_chunks - 1;
    int cb = k0 * 2 / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
    offA[i] = (int64_t)row * lda2 + (int64_t)ca * 16;
    offB[i] = (int64_t)row * ldb2 + (int64_t)cb * 16;
    rowi[i] = row;
  }
  const unsigned smem_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned wave_lds = smem_base + (unsigned)wave * 1024u;
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(&tn_zero_page);
  const unsigned char* ba = A + (int64_t)m_beg * lda2;        // rows of the stage being staged next: advanced by 32 rows per call
  const unsigned char* bb = B + (int64_t)m_beg * ldb2;
  int staged = 0;                                              // stages handed to the DMA so far
  unsigned ring_w = 0;                                         // ring position (bytes) of the next stage to stage
  auto stage = [&]() __attribute__((always_inline)) {
    const unsigned sl = wave_lds + ring_w;
    const int valid = m_end - m_beg - staged * RM;
    if (valid >= RM) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        asr_lds_dma16(sl + i * 8192, ba + offA[i]);
        asr_lds_dma16(sl + TILEB + i * 8192, bb + offB[i]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bool in = rowi[i] < valid;
        asr_lds_dma16(sl + i * 8192, in ? ba + offA[i] : zero);
        asr_lds_dma16(sl + TILEB + i * 8192, in ? bb + offB[i] : zero);
      }
    }
    ba += RM * lda2; bb += RM * ldb2;
    ++staged;
    ring_w = ring_w == (unsigned)(NST - 1) * STAGEB ? 0u : ring_w + STAGEB;
  };

  // fragment read offsets inside a stage: row 8 g + (lr >> 2) (+ 4: offset 2048), column c0 + 4 (lr & 3)
  const int frow = 8 * g + (lr >> 2), fkey = tn256_key(frow);
  unsigned fa[4], fb[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int col = wn * 64 + i * 16 + 4 * (lr & 3);
    fa[i] = smem_base + (unsigned)(frow * 512 + (((col >> 3) ^ fkey) << 4) + ((col >> 2) & 1) * 8);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = wk * 128 + j * 16 + 4 * (lr & 3);
    fb[j] = smem_base + (unsigned)(TILEB + frow * 512 + (((col >> 3) ^ fkey) << 4) + ((col >> 2) & 1) * 8);
  }

  f32x4_t acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // column sums of dY (the bias gradient) from the A fragments of the k0 = 0 blocks.  Round 6: four v_dot2c per fragment (asr_sum8_bf16)
  // instead of a chain of 16 dependent shift / mask / add, and the four fragments of a row band split between the two waves that read them
  // (wk = 0: fragments 0, 1; wk = 1: 2, 3).  In-kernel section timing (-DTN_TIMING) had the summing wave as the straggler of every stage of
  // such a block: 1 745 cycles between the barriers against 1 050 for a wave that only multiplies.
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_colsum = colsum != nullptr && k0 == 0;
  auto addsum = [&](int i, const u32x4_t& v) __attribute__((always_inline)) {
    if ((i >> 1) == wk) asr_sum8_bf16(bsum[i], __builtin_bit_cast(bf16x8_t, v));
  };

  // prologue: stages 0 .. 2 on their way, stage 0 landed and published, its fragments requested
  for (int st = 0; st < NST && st < nstage; ++st) stage();
  if (NST == 4 && nstage >= 4) asr_wait_vmcnt<12>(); else if (nstage >= 3) asr_wait_vmcnt<8>(); else if (nstage == 2) asr_wait_vmcnt<4>(); else asr_wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  u32x4_t a[4], b[8];
  unsigned ring_r = 0;                                         // ring position of the stage whose fragments are requested next
#pragma unroll
  for (int i = 0; i < 3; ++i) TN_FRAG_READ(a[i], fa[i] + ring_r)
#pragma unroll
  for (int j = 0; j < 8; ++j) TN_FRAG_READ(b[j], fb[j] + ring_r)
  TN_FRAG_READ(a[3], fa[3] + ring_r)
  ring_r = STAGEB;

#ifdef TN_TIMING
  long long tsec[6] = {0, 0, 0, 0, 0, 0}, tlast = clock64();
#endif
  for (int st = 0; st < nstage; ++st) {
    TN_STAMP(5)
    // ---- row 0: the only waits of the stage.  Requests in flight, oldest first: a0 a1 a2 b0 .. b7 a3 (two reads each)
    tn_wait_lgkm<15>(a[0], b[0]);
    if (do_colsum) addsum(0, a[0]);
    tn_mma2<SWAP>(acc[0][0], a[0], b[0]);
    tn_wait_lgkm<14>(a[0], b[1]); tn_mma2<SWAP>(acc[0][1], a[0], b[1]);
    tn_wait_lgkm<12>(a[0], b[2]); tn_mma2<SWAP>(acc[0][2], a[0], b[2]);
    tn_wait_lgkm<10>(a[0], b[3]); tn_mma2<SWAP>(acc[0][3], a[0], b[3]);
    tn_wait_lgkm<8>(a[0], b[4]);  tn_mma2<SWAP>(acc[0][4], a[0], b[4]);
    tn_wait_lgkm<6>(a[0], b[5]);  tn_mma2<SWAP>(acc[0][5], a[0], b[5]);
    tn_wait_lgkm<4>(a[0], b[6]);  tn_mma2<SWAP>(acc[0][6], a[0], b[6]);
    tn_wait_lgkm<2>(a[0], b[7]);  tn_mma2<SWAP>(acc[0][7], a[0], b[7]);
    // ---- stage st + 1 published (every wave's pieces landed), stage st's buffer free (every wave's reads of it returned)
    TN_STAMP(0)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));
    TN_STAMP(1)
    if (NST == 4 && st + 3 < nstage) asr_wait_vmcnt<8>(); else if (st + 2 < nstage) asr_wait_vmcnt<4>(); else asr_wait_vmcnt<0>();
    TN_STAMP(2)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    TN_STAMP(3)
    if (staged < nstage) stage();                              // stage st + NST into the buffer of stage st
    // (past the last stage the requests below fetch stale bytes of the ring that nobody uses)
    TN_FRAG_READ(a[0], fa[0] + ring_r)
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      if (do_colsum) addsum(i, a[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        tn_mma2<SWAP>(acc[i][j], a[i], b[j]);
        if (i == 3) TN_FRAG_READ(b[j], fb[j] + ring_r)
      }
      TN_FRAG_READ(a[i], fa[i] + ring_r)
    }
    ring_r = ring_r == (unsigned)(NST - 1) * STAGEB ? 0u : ring_r + STAGEB;
    TN_STAMP(4)
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the stale requests of the last stage: the next piece rewrites the ring
#ifdef TN_TIMING
  if (blockIdx.x == 0 && lane == 0) {
    for (int k = 0; k < 6; ++k) tn_dbg[wave * 8 + k] = tsec[k];
    tn_dbg[wave * 8 + 7] = nstage;
  }
#endif

  if constexpr (!SWAP) {
    // ---- epilogue of the shared-block forms (equal pieces, slices): lane (lr, g) holds rows 4g .. 4g+3 of column lr of a fragment --
    // an instruction's 64 lanes touch 4 runs of 64 contiguous bytes, which is what the fp32 atomics want
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gn = n0 + wn * 64 + i * 16 + g * 4 + r;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int gk = k0 + wk * 128 + j * 16 + lr;
          if (gn < pN && gk < pK) {
            float* dst = C + (int64_t)gn * ldc + gk;
            if (single) *dst += acc[i][j][r]; else atomicAdd(dst, acc[i][j][r]);
          }
        }
      }
  } else {
  // ---- epilogue.  The MFMAs ran with the operands swapped (k rows, n columns): lane (lr, g) holds, of fragment (i, j), the FOUR
  // consecutive k = k0 + wk 128 + 16 j + 4 g .. + 3 of row n = n0 + wn 64 + 16 i + lr -- 16 contiguous bytes of dW
  // A block with one owner: plain read-modify-write, the 8 loads of a fragment row issued TOGETHER (the compiler cannot prove that
  // dst(i, j) and dst(i', j') differ -- ldc is a run-time value -- and would otherwise wait for every load behind the previous store:
  // 32 dependent round trips to L2 / HBM per block).  A sliced block: fp32 atomics without a return value (nothing to wait for).
  const bool vec = (ldc & 3) == 0 && ((uintptr_t)C & 15) == 0 && (pK & 3) == 0;
  const bool full = n0 + 256 <= pN && k0 + 256 <= pK;          // no edge inside the block: no per-element tests (wave-uniform)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gn = n0 + wn * 64 + i * 16 + lr;
    const int gk0 = k0 + wk * 128 + g * 4;
    float* const row = C + (int64_t)gn * ldc + gk0;
    if (full && vec && single) {
      f32x4_t old[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) old[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(row + j * 16));
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4_t*>(row + j * 16) = old[j] + acc[i][j];
    } else if (full && !single) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(row + j * 16 + r, acc[i][j][r]);
    } else if (gn < pN) {
      if (single && vec) {
        f32x4_t old[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (gk0 + j * 16 < pK) old[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(row + j * 16));
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (gk0 + j * 16 < pK) *reinterpret_cast<f32x4_t*>(row + j * 16) = old[j] + acc[i][j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (gk0 + j * 16 + r < pK) {
              if (single) row[j * 16 + r] += acc[i][j][r];
              else atomicAdd(row + j * 16 + r, acc[i][j][r]);
            }
      }
    }
  }
  }
  if (do_colsum) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if ((i >> 1) != wk) continue;
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int gn = n0 + wn * 64 + i * 16 + lr;
      if (g == 0 && gn < pN) atomicAdd(colsum + gn, v);
    }
  }
}
#undef TN_FRAG_READ

// ---- grouped form: the weight gradients of up to TN_GROUP_MAX linear layers in ONE launch.  A weight gradient is off the
// critical path of backward (only the data gradient feeds the next layer), and alone it is latency bound: 16 - 64 blocks of dW, each
// a serial chain over all M rows.  Queued and launched together at the end of backward, the layers' blocks fill the chip
// (~1900 blocks of 128 x 128 for the 4-layer model), every block contracts ALL rows of its layer (no m-split: no partial-sum
// workspace, no fold pass, plain += into the fp32 gradient), longest layers first.
constexpr int TN_GROUP_MAX = 48;
struct TnGroupProb {                  // Tn128Args in 72 bytes: 48 problems + their prefix sums stay inside the 4 KB of kernel arguments
  const void* A; const void* B; float* C; float* colsum;
  int lda, ldb, ldc, M, N, K, m_per_split, tiles_k, ntiles, pad;
};
struct TnGroupArgs {
  TnGroupProb p[TN_GROUP_MAX];
  int first[TN_GROUP_MAX + 1];       // first[i] = number of blocks of the problems before i
  int n;
};
static_assert(sizeof(TnGroupArgs) + 16 <= 4096, "kernel argument segment");
__device__ __forceinline__ Tn128Args tn_group_prob(const TnGroupArgs& ga, int i) {
  const TnGroupProb& q = ga.p[i];
  Tn128Args p;
  p.A = q.A; p.B = q.B; p.C = q.C; p.colsum = q.colsum; p.ws = nullptr;
  p.lda = q.lda; p.ldb = q.ldb; p.ldc = q.ldc;
  p.M = q.M; p.N = q.N; p.K = q.K; p.m_per_split = q.m_per_split; p.tiles_k = q.tiles_k; p.ntiles = q.ntiles;
  return p;
}
template <int NST, bool ROT, bool SWAP = false>        // ROT: the launch is a list of whole-contraction blocks, longest first (walk order below)
__global__ __launch_bounds__(512, 2) void gemm_tn256g_kernel(TnGroupArgs ga) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nwg = gridDim.x, bid = blockIdx.x;
  // ROT (whole-contraction blocks, longest first): workgroups are dispatched in blockIdx order as CUs free up, so the list must be
  // walked in that order -- in rounds of 256 (one per CU), and inside a round the 32 blocks of an XCD are consecutive list entries
  // (blocks of one problem share operand columns in that XCD's L2)
  int wid;
  if constexpr (ROT) {
    const int base = bid & ~255, left = min(256, nwg - base), q = left >> 3, r = left & 7, b = bid - base;
    wid = base + ((b & 7) < r ? (b & 7) * (q + 1) : r * (q + 1) + ((b & 7) - r) * q) + (b >> 3);
  } else {
    wid = asr_xcd_linear(bid, nwg);
  }
  int i = 0;
  while (i + 1 < ga.n && wid >= ga.first[i + 1]) ++i;
  const Tn128Args p = tn_group_prob(ga, i);
  const int w = wid - ga.first[i], split = w / p.ntiles, m_beg = split * p.m_per_split;
  tn256r_body<NST, SWAP>(p, smem, w % p.ntiles, m_beg, min(p.M, m_beg + p.m_per_split), p.m_per_split >= p.M);
}

// ---- the same blocks, scheduled by the host: the launch is ONE workgroup per CU and every workgroup gets the same number of 32-row
// stages.  All (problem, block of dW, stage) triples of the launch form one line -- problems in launch order, blocks within a
// problem, stages within a block -- which is cut into gridDim.x equal pieces; a workgroup walks its piece: the tail of one block's
// rows, whole blocks, the head of the next (a block of dW whose rows are shared between workgroups is summed with fp32 atomics).
// Measured before (profiles/r03_bench_timeline.txt, launch-by-launch listing): 184 / 300 / 304 equal-length blocks on 256 CUs
// took 185 / 340 / 266 us -- the second round of 44 blocks costs as much as the first of 256.
// first[] holds the prefix sums of STAGES per problem here; m_per_split the stages of one block of that problem.
template <int NST>
__global__ __launch_bounds__(512, 2) void gemm_tn256s_kernel(TnGroupArgs ga, int per_wg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wid = asr_xcd_linear(bid, nwg);
  const int total = ga.first[ga.n];
  int x = wid * per_wg;
  const int x1 = min(total, x + per_wg);
  int i = 0;
  bool again = false;
  while (x < x1) {
    while (i + 1 < ga.n && x >= ga.first[i + 1]) ++i;
    const Tn128Args p = tn_group_prob(ga, i);
    const int spb = p.m_per_split;                         // stages of one block of this problem
    const int w = x - ga.first[i], tile = w / spb, st0 = w % spb;
    const int st1 = min(spb, st0 + (x1 - x));
    if (again) __syncthreads();                            // every wave is done reading the previous piece's last stages
    tn256r_body<NST, false>(p, smem, tile, st0 * 32, min(p.M, st1 * 32), st0 == 0 && st1 == spb);
    x += st1 - st0;
    again = true;
  }
}
template <int NST>
__global__ __launch_bounds__(256, 2) void gemm_tn128g_kernel(TnGroupArgs ga) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wid = asr_xcd_linear(bid, nwg);
  int i = 0;
  while (i + 1 < ga.n && wid >= ga.first[i + 1]) ++i;
  tn128p_body<NST>(tn_group_prob(ga, i), smem, wid - ga.first[i], true);
}

}  // namespace

// Slices per problem for the whole-block form of asr_gemm_tn_grouped: the launch's workgroups (one per block of dW and slice of its
// rows, longest first) are played through on 256 CUs -- each goes to the CU that is free first, as the dispatcher does -- for a few
// upper bounds on the slice length; a workgroup costs its stages + a fixed part (pipeline fill, epilogue; more with atomics).
// The plan of the last few distinct problem lists is kept (a training step asks for the same lists again and again).
static bool tn_rot_plan(int cnt, const int* order, const int* M, const int* N, const int* K, int* splits_out) {
  struct Memo { uint64_t key; int cnt; bool whole_wins; int splits[TN_GROUP_MAX]; };
  static Memo memo[8];
  static int memo_next = 0;
  static std::mutex memo_lock;                  // (the library is called from one thread per process; a second caller must not tear an entry)
  std::lock_guard<std::mutex> hold(memo_lock);
  uint64_t key = 1469598103934665603ull;
  for (int j = 0; j < cnt; ++j) {
    const int i = order[j];
    for (const int v : {M[i], N[i], K[i]}) key = (key ^ (uint64_t)(uint32_t)v) * 1099511628211ull;
  }
  for (const Memo& m : memo)
    if (m.key == key && m.cnt == cnt) {
      for (int j = 0; j < cnt; ++j) splits_out[order[j]] = m.splits[j];
      return m.whole_wins;
    }
  // a visit that ends in 65 536 fp32 atomics costs about as much as 100 stages (profiles/r05_tn_grouped.txt: 123 us of a 480 us
  // pass for ~2.3 visits per workgroup)
  constexpr int CUS = 256, FIXED = 10, FIXED_ATOMIC = 100;
  int64_t whole = 0;
  int longest = 0;
  for (int j = 0; j < cnt; ++j) {
    const int i = order[j];
    const int st = (M[i] + 31) / 32;
    whole += (int64_t)((N[i] + 255) / 256) * ((K[i] + 255) / 256) * st;
    longest = st > longest ? st : longest;
  }
  const int64_t share = whole / CUS > 32 ? whole / CUS : 32;
  const double cuts[] = {1e30, 1.0, 1.0 / 1.5, 0.5, 1.0 / 3, 0.25};
  int best_splits[TN_GROUP_MAX];
  int64_t best = -1;
  std::vector<std::pair<int, int>> items;          // (cost, count) runs, longest first
  for (const double cut : cuts) {
    const double lim = cut > 1e20 ? 1e30 : (double)share * cut;
    if (cut < 1e20 && lim >= longest) continue;      // the same plan as "whole"
    int sp[TN_GROUP_MAX];
    items.clear();
    for (int j = 0; j < cnt; ++j) {
      const int i = order[j];
      const int st = (M[i] + 31) / 32;
      int s = st > lim ? (int)((st + lim - 1) / lim) : 1;
      if (s > st) s = st;
      sp[j] = s;
      const int len = (st + s - 1) / s;
      items.push_back({len + (s > 1 ? FIXED_ATOMIC : FIXED), ((N[i] + 255) / 256) * ((K[i] + 255) / 256) * s});
    }
    std::sort(items.begin(), items.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first > b.first; });
    std::priority_queue<int64_t, std::vector<int64_t>, std::greater<int64_t>> free_at;
    for (int c = 0; c < CUS; ++c) free_at.push(0);
    int64_t end = 0;
    for (const auto& it : items)
      for (int c = 0; c < it.second; ++c) {
        const int64_t t = free_at.top() + it.first;
        free_at.pop();
        free_at.push(t);
        end = t > end ? t : end;
      }
    if (best < 0 || end < best) {
      best = end;
      for (int j = 0; j < cnt; ++j) best_splits[j] = sp[j];
    }
  }
  // the alternative: equal pieces of the launch's stages on one workgroup per CU -- perfectly balanced, but nearly every block is
  // shared between two workgroups (two atomic visits each)
  const int64_t pieces = share + 2 * FIXED_ATOMIC + FIXED;
  Memo& m = memo[memo_next];
  memo_next = (memo_next + 1) % 8;
  m.key = key; m.cnt = cnt; m.whole_wins = best <= pieces;
  for (int j = 0; j < cnt; ++j) { m.splits[j] = best_splits[j]; splits_out[order[j]] = best_splits[j]; }
  return m.whole_wins;
}

// The decision asr_gemm_tn_grouped takes for a list of problems, without launching anything (host only; tests, tuning): 1 = one
// workgroup per whole block of dW (splits[i] > 1: the slices of an over-long block), 0 = round 3's shared forms.
extern "C" int asr_gemm_tn_grouped_plan(int n, const int* M, const int* N, const int* K, int* splits) {
  ASR_CHECK_ARG(n >= 0 && n <= TN_GROUP_MAX && (n == 0 || (M && N && K && splits)));
  int order[TN_GROUP_MAX];
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    ASR_CHECK_ARG(M[i] >= 0 && N[i] >= 0 && K[i] >= 0);
    splits[i] = 1;
    if (M[i] > 0 && N[i] > 0 && K[i] > 0) order[cnt++] = i;
  }
  if (cnt == 0) return 1;
  for (int a = 1; a < cnt; ++a)
    for (int b = a; b > 0 && M[order[b]] > M[order[b - 1]]; --b) { const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t; }
  return tn_rot_plan(cnt, order, M, N, K, splits) ? 1 : 0;
}

extern "C" int asr_gemm_tn_grouped(int n, const void* const* dy, const int64_t* ld_dy, const void* const* x, const int64_t* ld_x,
                                   float* const* dw, const int64_t* ld_dw, float* const* db, const int* M, const int* N, const int* K,
                                   int dtype, hipStream_t stream) {
  ASR_CHECK_ARG(n >= 0 && n <= TN_GROUP_MAX && dtype == ASR_BF16);
  if (n == 0) return ASR_OK;
  ASR_CHECK_ARG(dy && ld_dy && x && ld_x && dw && ld_dw && db && M && N && K);
  int order[TN_GROUP_MAX];
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    ASR_CHECK_ARG(M[i] >= 0 && N[i] >= 0 && K[i] >= 0);
    if (M[i] == 0 || N[i] == 0 || K[i] == 0) continue;   // an empty problem adds nothing (its pointers may be null)
    ASR_CHECK_ARG(dy[i] && x[i] && dw[i]);
    if (ld_dy[i] % 8 != 0 || ld_x[i] % 8 != 0 || !aligned16(dy[i]) || !aligned16(x[i]) || ld_dy[i] < N[i] ||
        ld_dy[i] >= ((int64_t)1 << 22) || ld_x[i] >= ((int64_t)1 << 22) || ld_dw[i] >= ((int64_t)1 << 31))
      return ASR_EUNSUPPORTED;
    order[cnt++] = i;
  }
  if (cnt == 0) return ASR_OK;
  // longest row count first: a block's run time is proportional to M, and the late blocks decide when the launch ends
  for (int a = 1; a < cnt; ++a)
    for (int b = a; b > 0 && M[order[b]] > M[order[b - 1]]; --b) { const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t; }
  TnGroupArgs ga{};
  int total = 0;
  // Forms: 256 x 256 blocks (eight waves), one workgroup per CU, the launch's stages dealt out in equal pieces (gemm_tn256s_kernel);
  // one workgroup per (block of dW, slice of <= mrows rows), fp32 atomics where a block has more than one slice (A/B of the
  // slice length: profiles/r03_grouped_wgrad_ab.txt); the 128 x 128 / four-wave form, one workgroup per whole contraction.  TN_GROUP_TILE:
  // 0 (default): by the longest contraction of the group -- equal pieces up to slice_min rows, per-slice blocks from there on: with
  // >= 3 slices per block of dW the launch is several rounds of workgroups whatever the form, and the slices of one block run side by
  // side on one L2 (47 % hits against 7 %, profiles/r03_tn_group_l2.txt): configs[3] (12 720 rows) 13.16 -> 12.92 ms/step, while the
  // headline's 6 400 rows (2 slices: 1.2 rounds) keep the equal pieces.  1: equal pieces always; 256: per-slice always; 128.
  const int tmode = (int)asr_tuning("TN_GROUP_TILE", 0);
  constexpr int mrows = 3200, slice_min = 9600;
  int max_m = 0;
  for (int j = 0; j < cnt; ++j) max_m = M[order[j]] > max_m ? M[order[j]] : max_m;
  // Round 5: tn256r_body, and ONE workgroup per block of dW over the WHOLE contraction, dispatched longest
  // first -- no block is shared between workgroups, so no fp32 atomics and a vector epilogue: round 3's equal pieces shared almost
  // every block (pieces of 130 - 160 stages against blocks of 100 / 200), and the 65 536 atomics per visit were a quarter of the
  // launch (profiles/r05_tn_grouped.txt).
  // (every 256 x 256 form runs tn256r_body since round 6; tmode != 0 forces a form for the tests)
  const bool rot = tmode == 0;
  const bool big = tmode != 128;
  // ... cut into slices of its rows (summed with fp32 atomics, as before) where that shortens the launch: one block longer than a CU's
  // share (emb_cnn's window contractions: one or two blocks over several hundred thousand rows), or equal blocks whose count is an
  // awkward multiple of the CUs (configs[3]: 576 blocks of 398 stages = 2.25 rounds).  tn_rot_plan() decides by playing the dispatch
  // through for a few slice lengths; the list is then ordered by SLICE length.
  int rot_splits[TN_GROUP_MAX];
  // where the whole blocks would leave CUs idle (tn_rot_plan), round 3's shared forms (equal pieces / slices) with the new loop
  const bool whole = rot && tn_rot_plan(cnt, order, M, N, K, rot_splits);
  const bool sched = !whole && (tmode == 1 || (tmode == 0 && max_m < slice_min));
  if (whole) {
    int slice[TN_GROUP_MAX];
    for (int j = 0; j < cnt; ++j) {
      const int i = order[j];
      slice[i] = ((M[i] + 31) / 32 + rot_splits[i] - 1) / rot_splits[i];
    }
    for (int a = 1; a < cnt; ++a)
      for (int b = a; b > 0 && slice[order[b]] > slice[order[b - 1]]; --b) { const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t; }
  }
  for (int j = 0; j < cnt; ++j) {
    const int i = order[j];
    TnGroupProb& q = ga.p[j];
    q.A = dy[i]; q.B = x[i]; q.C = dw[i]; q.colsum = db[i];
    q.lda = (int)ld_dy[i]; q.ldb = (int)ld_x[i]; q.ldc = (int)ld_dw[i]; q.M = M[i]; q.N = N[i]; q.K = K[i];
    const int T = big ? 256 : 128;
    q.tiles_k = (K[i] + T - 1) / T;
    q.ntiles = ((N[i] + T - 1) / T) * q.tiles_k;
    ga.first[j] = total;
    if (sched) {
      q.m_per_split = (M[i] + 31) / 32;                      // stages per block
      total += q.ntiles * q.m_per_split;
      continue;
    }
    int splits = whole ? rot_splits[i] : 1;
    if (big && !whole) splits = (M[i] + mrows - 1) / mrows;
    if (splits < 1) splits = 1;
    q.m_per_split = ((M[i] + splits - 1) / splits + 31) / 32 * 32;
    splits = (M[i] + q.m_per_split - 1) / q.m_per_split;
    total += q.ntiles * splits;
  }
  ga.first[cnt] = total;
  ga.n = cnt;
  (void)asr_grant_lds<gemm_tn128g_kernel<3>>(3 * 16384);
  (void)asr_grant_lds<gemm_tn256g_kernel<3, true, false>>(3 * 32768);
  (void)asr_grant_lds<gemm_tn256g_kernel<3, true, true>>(3 * 32768);
  (void)asr_grant_lds<gemm_tn256s_kernel<3>>(3 * 32768);
  AsrProfScope prof(ASR_OP_GEMM, stream);
  if (sched) {
    // one workgroup per CU, at least 16 stages each; pieces of equal length
    int nwg = 256;
    if (nwg > total / 16) nwg = total / 16;
    if (nwg < 1) nwg = 1;
    const int per_wg = (total + nwg - 1) / nwg;
    nwg = (total + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(gemm_tn256s_kernel<3>, dim3((unsigned)nwg), dim3(512), 3 * 32768, stream, ga, per_wg);
  } else if (big) {
    if (whole) hipLaunchKernelGGL((gemm_tn256g_kernel<3, true, true>), dim3((unsigned)total), dim3(512), 3 * 32768, stream, ga);
    else hipLaunchKernelGGL((gemm_tn256g_kernel<3, true, false>), dim3((unsigned)total), dim3(512), 3 * 32768, stream, ga);
  } else hipLaunchKernelGGL(gemm_tn128g_kernel<3>, dim3((unsigned)total), dim3(256), 3 * 16384, stream, ga);
  ASR_LAUNCH_CHECK();
#ifdef TN_TIMING
  if (big && !sched) {
    long long h[64];
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(tn_dbg), sizeof(h));
    static int shown = 0;
    if (shown++ % 8 == 3)
      for (int w = 0; w < 8; w += 3)
        fprintf(stderr, "tn256g timing wave %d stages %lld: row0 %lld lgkm %lld vmcnt %lld barrier %lld rest %lld looptop %lld (s_memtime ticks)\n", w, h[w * 8 + 7],
                h[w * 8 + 0], h[w * 8 + 1], h[w * 8 + 2], h[w * 8 + 3], h[w * 8 + 4], h[w * 8 + 5]);
  }
#endif
  return ASR_OK;
}
