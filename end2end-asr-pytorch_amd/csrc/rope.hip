// Rotary position embedding (RoPE, Su et al. 2021, arXiv:2104.09864) of the encoder's self-attention: one
// memory-bound kernel between the Q|K|V projection and asr_attn_fwd, its transpose between asr_attn_bwd and the projection backward.
//
//   x  (B, T, nheads d) with element strides (x_sb, x_st, 1), rotated IN PLACE; cs (T, d/2, 2) fp32 = [cos, sin], contiguous.
//   pair i of head h of frame t is (x0, x1) = (x[t, h d + 2 i], x[t, h d + 2 i + 1])  (interleaved, the RoFormer paper's layout) and
//   (c, s) = cs[t, i]: the same row for every batch entry and head.
//     forward    y0 = x0 c - x1 s      y1 = x0 s + x1 c
//     inverse    y0 = x0 c + x1 s      y1 = x1 c - x0 s          (the transpose = the inverse: the backward of the forward)
//   fp32 arithmetic from the loaded elements and the fp32 table; each result is (a b) -/+ (e f) with the two products and the sum
//   rounded separately (no contraction into an fma, so the forward and the inverse round alike), then rounded once to the storage type.
//
// Two arms, chosen in the entry point as AttnArgs::vec is chosen:
//   chunk arm   x 16-byte aligned, both strides multiples of a chunk's elements (8 bf16 / 4 fp32): a lane owns one 16-byte chunk =
//               4 / 2 whole pairs (d is a multiple of 16, so a chunk never straddles a head), reads its 4 / 2 table entries with
//               16-byte loads and stores 16 bytes.
//   pair arm    anything else with even strides: one pair per lane, 4- / 8-byte accesses.
// 256 threads per block, at most 2048 blocks, a grid stride over the chunks (pairs).  No LDS, no atomics, no cross-lane traffic; the
// table (T d/2 entries of 8 bytes, a few tens of KB) is read B nheads times and stays in L2.  Sines are never computed here.
#include "common.h"

namespace {

constexpr int ROPE_THREADS = 256;
constexpr int ROPE_MAX_BLOCKS = 2048;

template <bool INV> __device__ __forceinline__ void rope_pair(float& x0, float& x1, float c, float s) {
  // (the products as separate roundings: an fma would round x0 c - x1 s differently from its transpose's x1 c - x0 s)
  const float a = __fmul_rn(x0, c), b = __fmul_rn(x1, s), e = __fmul_rn(x0, s), f = __fmul_rn(x1, c);
  x0 = INV ? __fadd_rn(a, b) : __fsub_rn(a, b);
  x1 = INV ? __fsub_rn(f, e) : __fadd_rn(e, f);
}

// one pair as one 8- / 4-byte access
__device__ __forceinline__ void rope_ld2(const float* p, float& x0, float& x1) {
  const float2 v = *reinterpret_cast<const float2*>(p);
  x0 = v.x;
  x1 = v.y;
}
__device__ __forceinline__ void rope_ld2(const bf16_t* p, float& x0, float& x1) {
  const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
  x0 = __uint_as_float(v << 16);
  x1 = __uint_as_float(v & 0xFFFF0000u);
}
__device__ __forceinline__ void rope_st2(float* p, float x0, float x1) { *reinterpret_cast<float2*>(p) = make_float2(x0, x1); }
__device__ __forceinline__ void rope_st2(bf16_t* p, float x0, float x1) { *reinterpret_cast<uint32_t*>(p) = pack_bf16(x0, x1); }

// n = B T (nheads d / EPC) chunks; chunk q = (b, t, j) with j the fastest.  A chunk's first pair in its head: (j EPC % d) / 2.
template <typename T, bool INV>
__global__ __launch_bounds__(ROPE_THREADS) void rope_chunk_kernel(T* __restrict__ x, int64_t x_sb, int64_t x_st, int T_, int row_chunks, int d,
                                                                  const float* __restrict__ cs, int64_t n) {
  constexpr int EPC = DT<T>::EPC, PAIRS = EPC / 2;
  const int64_t step = (int64_t)gridDim.x * ROPE_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * ROPE_THREADS + threadIdx.x; q < n; q += step) {
    const int j = (int)(q % row_chunks);
    const int64_t bt = q / row_chunks;
    const int t = (int)(bt % T_);
    const int64_t b = bt / T_;
    T* p = x + b * x_sb + (int64_t)t * x_st + (int64_t)j * EPC;
    const float* tab = cs + ((int64_t)t * (d / 2) + ((j * EPC) % d) / 2) * 2;      // PAIRS entries of [cos, sin]
    Chunk<T> v;
    v.v = *reinterpret_cast<const uint4*>(p);
    f32x4_t w[PAIRS / 2];
#pragma unroll
    for (int k = 0; k < PAIRS / 2; ++k) w[k] = *reinterpret_cast<const f32x4_t*>(tab + 4 * k);
#pragma unroll
    for (int i = 0; i < PAIRS; ++i) {
      float x0 = DT<T>::from(v.e[2 * i]), x1 = DT<T>::from(v.e[2 * i + 1]);
      rope_pair<INV>(x0, x1, w[i / 2][2 * (i % 2)], w[i / 2][2 * (i % 2) + 1]);
      v.e[2 * i] = DT<T>::to(x0);
      v.e[2 * i + 1] = DT<T>::to(x1);
    }
    *reinterpret_cast<uint4*>(p) = v.v;
  }
}

// n = B T (nheads d / 2) pairs; pair q = (b, t, j) with j the fastest, its table entry (t, j % (d/2)).
template <typename T, bool INV>
__global__ __launch_bounds__(ROPE_THREADS) void rope_pair_kernel(T* __restrict__ x, int64_t x_sb, int64_t x_st, int T_, int row_pairs, int d,
                                                                 const float* __restrict__ cs, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * ROPE_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * ROPE_THREADS + threadIdx.x; q < n; q += step) {
    const int j = (int)(q % row_pairs);
    const int64_t bt = q / row_pairs;
    const int t = (int)(bt % T_);
    const int64_t b = bt / T_;
    T* p = x + b * x_sb + (int64_t)t * x_st + 2 * (int64_t)j;
    const float2 e = *reinterpret_cast<const float2*>(cs + ((int64_t)t * (d / 2) + j % (d / 2)) * 2);
    float x0, x1;
    rope_ld2(p, x0, x1);
    rope_pair<INV>(x0, x1, e.x, e.y);
    rope_st2(p, x0, x1);
  }
}

inline unsigned rope_blocks(int64_t n) {
  const int64_t blocks = ceil_div64(n, ROPE_THREADS);
  return (unsigned)(blocks < ROPE_MAX_BLOCKS ? blocks : ROPE_MAX_BLOCKS);
}

}  // namespace

extern "C" int asr_rope(void* x, int64_t x_sb, int64_t x_st, int B, int T, int nheads, int d, const float* cs, int inverse, int dtype,
                        hipStream_t stream) {
  ASR_CHECK_ARG(B >= 0 && T >= 0 && nheads >= 0 && x_sb >= 0 && x_st >= 0);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  if (d != 16 && d != 32 && d != 64) return ASR_EUNSUPPORTED;
  if ((x_sb & 1) || (x_st & 1)) return ASR_EUNSUPPORTED;          // a pair is one aligned 4- / 8-byte access in either arm
  if (B == 0 || T == 0 || nheads == 0) return ASR_OK;
  ASR_CHECK_ARG(x && cs);
  ASR_CHECK_ARG((int64_t)nheads * d < (1ll << 30) && (T == 1 || (int64_t)nheads * d <= x_st));
  const int epc = dtype == ASR_F32 ? 4 : 8;
  ASR_CHECK_ARG(((uintptr_t)x) % (dtype == ASR_F32 ? 8 : 4) == 0 && aligned8(cs));
  const bool vec = aligned16(x) && aligned16(cs) && x_sb % epc == 0 && x_st % epc == 0;
  const int row = nheads * d / (vec ? epc : 2);
  const int64_t n = (int64_t)B * T * row;
  const dim3 grid(rope_blocks(n)), block(ROPE_THREADS);
  return asr_with_dtype(dtype, [&](auto tag) {
    using T_ = decltype(tag);
    if (vec)
      return inverse ? asr_launch<rope_chunk_kernel<T_, true>>(grid, block, 0, stream, (T_*)x, x_sb, x_st, T, row, d, cs, n)
                     : asr_launch<rope_chunk_kernel<T_, false>>(grid, block, 0, stream, (T_*)x, x_sb, x_st, T, row, d, cs, n);
    return inverse ? asr_launch<rope_pair_kernel<T_, true>>(grid, block, 0, stream, (T_*)x, x_sb, x_st, T, row, d, cs, n)
                   : asr_launch<rope_pair_kernel<T_, false>>(grid, block, 0, stream, (T_*)x, x_sb, x_st, T, row, d, cs, n);
  });
}
