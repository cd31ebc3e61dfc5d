// What the GEMM translation units share: gemm_nt.hip (both operands K-contiguous: forward, explicit transposes), gemm_nn.hip (data
// gradient) and gemm_tn.hip (weight gradient).  Argument structs and __forceinline__ device helpers only: every __global__ kernel is
// defined in exactly one of those files, above the extern "C" entry that launches it.
#pragma once
#include "common.h"

namespace {

struct GemmArgs {
  const void* A; const void* B; void* C; const float* bias; const void* mask;
  int64_t lda, ldb, ldc;
  int M, N, K;
  int k_per_split;     // multiple of BK
  float alpha;
  int relu, accumulate, atomic, vecA, vecB, vecC;
  int tiles_n, ntiles;
  int ablate;          // -DASR_TUNE_ABLATE builds only (tuning "GEMM_ABLATE"): 1 = stage A once, 2 = stage B once (stale operands: timing only)
  // NN, bf16 out (asr_gemm_nn_rowdot; gemm_big.h has the definition): the attention backward's delta from the block that is dO
  const void* dot_o; const float* dot_o32; float* dot_out; int dot_T, dot_H;
};

constexpr int kPitch = 144;   // bytes per LDS tile row: 128 data + 16 pad (keeps 16-B alignment, breaks the 128-B stride)

template <typename T>
__device__ __forceinline__ uint4 load_chunk(const T* row, int64_t k, int64_t kend, bool row_ok, bool vec) {
  Chunk<T> c;
  c.v = make_uint4(0u, 0u, 0u, 0u);
  if (row_ok) {
    if (vec) {
      if (k < kend) c.v = *reinterpret_cast<const uint4*>(row + k);
    } else {
#pragma unroll
      for (int j = 0; j < DT<T>::EPC; ++j)
        if (k + j < kend) c.e[j] = row[k + j];
    }
  }
  return c.v;
}

template <typename TO> __device__ __forceinline__ void store_out(TO* p, float v, int accumulate, int atomic);
template <> __device__ __forceinline__ void store_out<float>(float* p, float v, int accumulate, int atomic) {
  if (atomic) atomicAdd(p, v);
  else if (accumulate) *p += v;
  else *p = v;
}
template <> __device__ __forceinline__ void store_out<bf16_t>(bf16_t* p, float v, int accumulate, int) {
  if (accumulate) v += bf16_to_f32(*p);
  *p = f32_to_bf16(v);
}

// Direct-to-LDS staging of ROWS tile rows (gemm_nt.hip gemm_glds_kernel describes the LDS image; gemm_nn.hip stages its A operand the same way)
template <int ROWS>
__device__ __forceinline__ void stage_glds(unsigned char* lds_stage, const unsigned char* gbase, int64_t ld_bytes,
                                           int row0, int row_limit, int64_t kbyte0, int tid,
                                           int wave) {
#pragma unroll
  for (int i = 0; i < ROWS * 8 / 256; ++i) {
    const int c = i * 256 + tid, row = c >> 3, slot = (c & 7) ^ (row & 7);
    int gr = row0 + row;
    gr = gr < row_limit ? gr : row_limit - 1;                       // clamp: rows past the edge are never stored
    const unsigned char* src = gbase + (int64_t)gr * ld_bytes + kbyte0 + slot * 16;
    unsigned char* dst = lds_stage + (i * 256 + wave * 64) * 16;    // wave-uniform; the DMA adds lane * 16
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  }
}

// ---- TN (weight gradient; gemm_tn.hip describes the contraction): the 64 x 64 kernel there and the quadrant form in gemm_nn.hip
struct TnArgs {
  const void* A; const void* B; float* C; float* colsum;
  float* ws;     // split over m with a workspace: partial 64x64 tiles [split][tile][64][64], folded by tn_reduce_kernel
  int64_t lda, ldb, ldc;
  int M, N, K, m_per_split, tiles_k, ntiles;
};

template <typename T> struct TnPack;
template <> struct TnPack<bf16_t> {
  static constexpr int RM = 128, ROWB = 128, CPR = 8;
  // 8 consecutive rows m = m0 + 8g .. +7 of column c0 + lr  (m0 = first row of this wave's macro step)
  template <bool GMAJOR = false>
  static __device__ __forceinline__ uint4 load(const unsigned char* tile, int m0, int lr, int g, int c0) {
    const int row = m0 + 8 * g + (lr >> 2), col = c0 + 4 * (lr & 3);          // this lane SUPPLIES 4 columns of one row
    const int chunk = col >> 3, half = (col >> 2) & 1;
    const uint2 lo = asr_lds_read_tr16(tile + row * ROWB + ((chunk ^ (row & 7)) << 4) + half * 8);
    const uint2 hi = asr_lds_read_tr16(tile + (row + 4) * ROWB + ((chunk ^ ((row + 4) & 7)) << 4) + half * 8);
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
};
template <> struct TnPack<float> {
  static constexpr int RM = 64, ROWB = 256, CPR = 16;
  // pack element s feeds the s-th 16x16x4 MFMA, lane group g is its k index.  GMAJOR = false: row = m0 + 4s + g (both
  // operands come from this loader); GMAJOR = true: row = m0 + 4g + s, the k order of an operand read as one aligned 16-byte
  // chunk of 4 consecutive k (the A side of the NN kernel) -- the two operands of an MFMA must agree on k.
  template <bool GMAJOR = false>
  static __device__ __forceinline__ uint4 load(const unsigned char* tile, int m0, int lr, int g, int c0) {
    const int col = c0 + lr, chunk = col >> 2, sub = (col & 3) * 4;
    uint4 r;
    uint32_t* rr = &r.x;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = m0 + (GMAJOR ? 4 * g + s : 4 * s + g);
      rr[s] = *reinterpret_cast<const uint32_t*>(tile + row * ROWB + ((chunk ^ (row & 7)) << 4) + sub);
    }
    return r;
  }
};

// a partial last stage of a hand-issued LDS-DMA pipeline reads its missing rows from here (the DMA cannot zero fill)
__device__ const uint4 tn_zero_page = {0u, 0u, 0u, 0u};

}  // namespace
