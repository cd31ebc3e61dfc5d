// What the bf16 / head dim 64 attention kernels share (attention_d64_fwd.hip, attention_d64_bwd.hip, attention_d64_bwd_fused.hip,
// attention_pp.hip): the 64-row LDS tile image and its LDS-DMA staging, the fragment reads, the MFMA wrappers, the mask helpers, the
// XCD-aware workgroup id, and fast_ok(), the domain of these kernels that the dispatch of attention.hip tests.  Two-lane vectors are
// asr_f32x2_t / asr_bf16x2_t and the transposing LDS read is asr_lds_read_tr16 (common.h).  What only one kernel uses stays with it.
#pragma once
#include "attention.h"

namespace asr_attn {

constexpr int HD = 64;
constexpr int ROWB = 128;                 // bytes per LDS row (64 bf16)
constexpr int TILE = 64 * ROWB;           // one 64-row operand tile
constexpr float LOG2E = 1.4426950408889634f;

// all-reduce over the 4 lane groups that share lane & 15, on the VALU (gfx950 lane-swap instructions) instead of two
// ds_bpermute round trips: v_permlane16_swap(v, v) -> {rows 0,0,2,2} / {rows 1,1,3,3}; v_permlane32_swap(v, v) -> {lo,lo} / {hi,hi}
__device__ __forceinline__ float group_max4(float v) {
  uint32_t u = __float_as_uint(v);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  u = __float_as_uint(fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])));
  auto c = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(c[0]), __uint_as_float(c[1]));
}
__device__ __forceinline__ float group_sum4(float v) {
  uint32_t u = __float_as_uint(v);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  u = __float_as_uint(__uint_as_float(a[0]) + __uint_as_float(a[1]));
  auto c = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(c[0]) + __uint_as_float(c[1]);
}

__device__ __forceinline__ int xcd_linear_id() { return asr_xcd_linear((int)blockIdx.x, (int)gridDim.x); }

// The attention tiles come in by asr_lds_dma16 (common.h), the LDS-DMA issued BY HAND.  Through the builtin the compiler counts these
// loads itself, and its waitcnt pass cannot tell a DMA's LDS write from the tile a later ds_read wants: it put s_waitcnt vmcnt(0) in
// front of the first LDS read that followed the prefetch of the next tile (the P.V operand reads) -- the "double buffering" only ever
// overlapped the softmax, and every tile exposed most of a global-memory round trip.  Hand-issued, nothing waits until the explicit
// s_waitcnt vmcnt(0) in front of the barrier at the end of the tile (every tile loop of attention_d64_fwd.hip, attention_d64_bwd.hip and
// attention_d64_bwd_fused.hip has one); ordinary global loads issued while a DMA is in flight still wait for it (vmcnt retires in
// order), so those loops issue them BEFORE the prefetch.
// The same piece with 4 bytes per lane (a row of 64 floats per wave):
__device__ __forceinline__ void lds_dma4(unsigned lds_wave_base, const void* src) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "s"(lds_wave_base), "v"(src)
               : "memory");
}

// 64 rows x 128 B of a (rows, 64) bf16 slice -> LDS, chunk c of row r stored at slot c ^ (r & 7).  Rows past `nrows`
// re-read the last valid row (the LDS-DMA cannot zero-fill; such rows are masked / never stored by the callers).
// Full tiles go by a wave-uniform base address + per-thread byte offsets that do not change from tile to tile: the loops of the forward
// kernel hoist the offsets (tile_voff) and pay no vector instruction per prefetch (the per-tile 64-bit row * stride arithmetic was 24 of
// the 245 vector instructions of a forward tile).
// byte offset of this thread's i-th chunk of a tile relative to the tile's first row (row stride st elements; fast_ok(): < 2^22)
__device__ __forceinline__ unsigned tile_voff(int64_t st, int tid, int i) {
  const int c = i * 256 + tid, row = c >> 3, slot = c & 7;
  return (unsigned)(row * (int)st * 2 + ((slot ^ (row & 7)) << 4));
}
__device__ __forceinline__ void stage_tile(unsigned char* lds, const bf16_t* g, int64_t st, int r0, int nrows, int tid, int wave);
// full tiles (r0 + 64 <= nrows) go by base + hoisted offsets, the ragged last tile by the clamped per-row addresses
__device__ __forceinline__ void stage_tile_h(unsigned char* lds, const bf16_t* g, int64_t st, int r0, int nrows, const unsigned (&voff)[2],
                                             int tid, int wave) {
  if (r0 + 64 <= nrows) {
    const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const bf16_t* gb = g + (int64_t)r0 * st;
#pragma unroll
    for (int i = 0; i < 2; ++i) asr_lds_dma16(base + (unsigned)((i * 256 + wave * 64) * 16), gb, voff[i]);
  } else {
    stage_tile(lds, g, st, r0, nrows, tid, wave);
  }
}
__device__ __forceinline__ void stage_tile(unsigned char* lds, const bf16_t* g, int64_t st, int r0, int nrows, int tid, int wave) {
  const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i * 256 + tid, row = c >> 3, slot = c & 7;
    int gr = r0 + row;
    gr = gr < nrows ? gr : nrows - 1;
    const bf16_t* src = g + (int64_t)gr * st + ((slot ^ (row & 7)) << 3);
    asr_lds_dma16(base + (unsigned)((i * 256 + wave * 64) * 16), src);
  }
}
// A-operand pack (one row, 8 consecutive d) from a natural tile: row, macro step ds over d, lane group g
__device__ __forceinline__ uint4 frag_rows(const unsigned char* tile, int row, int ds, int g) {
  return *reinterpret_cast<const uint4*>(tile + row * ROWB + (((ds * 4 + g) ^ (row & 7)) << 4));
}
// A-operand pack of the TRANSPOSED tile: for column (= output row) c0 + lr, the 8 tile rows 32 ms + 4 g + {0..3} and
// 32 ms + 16 + 4 g + {0..3} -- the k order of pack_p() below.  ds_read_b64_tr_b16: lane i of a 16-lane group supplies the
// 8-byte address of row p0 + (i >> 2), columns c0 + 4 (i & 3).., and receives rows p0..p0+3 of column c0 + i.
__device__ __forceinline__ uint4 frag_cols(const unsigned char* tile, int c0, int ms, int lr, int g) {
  const int row = 32 * ms + 4 * g + (lr >> 2), col = c0 + 4 * (lr & 3);
  const int chunk = col >> 3, half = (col >> 2) & 1;
  // the builtin (not inline asm) so that the compiler tracks lgkmcnt for the result registers itself
  const uint2 lo = asr_lds_read_tr16(tile + row * ROWB + ((chunk ^ (row & 7)) << 4) + half * 8);
  const uint2 hi = asr_lds_read_tr16(tile + (row + 16) * ROWB + ((chunk ^ ((row + 16) & 7)) << 4) + half * 8);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
// The same two reads with the LANE part of the address (row within its 16-row fragment, swizzled chunk) computed once per kernel:
// the row of a fragment read is 16 X + lr (rows) or 32 ms + 4 g + (lr >> 2) (+ 16) (columns), so row & 7 -- the swizzle -- does not
// depend on X / ms, and what is left per read is tile base + lane offset + a compile-time constant that fits the DS offset field.
// (Computed per read, the address arithmetic was ~20 of the ~100 vector instructions of a backward half tile.)
struct FragOff {
  unsigned rows[2];          // [ds]
  unsigned cols[4];          // [df]
  __device__ __forceinline__ void init(int lr, int g) {
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) rows[ds] = (unsigned)(lr * ROWB + (((ds * 4 + g) ^ (lr & 7)) << 4));
    const int row = 4 * g + (lr >> 2);
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const int chunk = 2 * df + ((lr & 3) >> 1), half = lr & 1;       // column 16 df + 4 (lr & 3): 16-byte chunk, 8-byte half
      cols[df] = (unsigned)(row * ROWB + ((chunk ^ (row & 7)) << 4) + half * 8);
    }
  }
};
__device__ __forceinline__ uint4 frag_rows_at(const unsigned char* tile, unsigned off, int X) {
  return *reinterpret_cast<const uint4*>(tile + off + X * 16 * ROWB);
}
__device__ __forceinline__ uint4 frag_cols_at(const unsigned char* tile, unsigned off, int ms) {
  const uint2 lo = asr_lds_read_tr16(tile + off + 32 * ms * ROWB);
  const uint2 hi = asr_lds_read_tr16(tile + off + (32 * ms + 16) * ROWB);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
// B-operand pack from C fragments v[f][r] = X[16 f + 4 g + r][col]: k = 32 ms + 4 g + r (f = 2 ms), 32 ms + 16 + 4 g + r (f = 2 ms + 1)
__device__ __forceinline__ uint4 pack_p(const f32x4_t* v, int ms) {
  const f32x4_t a = v[2 * ms], b = v[2 * ms + 1];
  return make_uint4(pack_bf16(a[0], a[1]), pack_bf16(a[2], a[3]), pack_bf16(b[0], b[1]), pack_bf16(b[2], b[3]));
}
__device__ __forceinline__ void mma(f32x4_t& acc, const uint4& a, const uint4& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4_t mma_z(const uint4& a, const uint4& b) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
}
__device__ __forceinline__ uint4 load_row16(const bf16_t* base, int64_t st, int row, int nrows, int col0) {
  const int r = row < nrows ? row : nrows - 1;
  return *reinterpret_cast<const uint4*>(base + (int64_t)r * st + col0);
}

// Buffer resource over the whole key-padding mask ((B, Tk) or (B, Tq, Tk) bytes; fast_ok() guarantees < 2^31): raw buffer, stride 0,
// out-of-range reads return 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mask_rsrc(const AttnArgs& p) {
  const int64_t n = (int64_t)(p.B - 1) * p.m_sb + (int64_t)(p.Tq - 1) * p.m_sq + p.Tk;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.key_pad), 0, (int)n, 0x00020000);
}

// Mask NKF key fragments of raw scores s[qi][kf][r] (key = kbase + 16 kf + 4 g + r, query = q_lane + 16 qi): straight-line
// selects, mask bytes read with clamped (always valid) addresses.
template <int NKF, int NQ = 2>
__device__ __forceinline__ void mask_scores(const AttnArgs& p, f32x4_t (*s)[NKF], int b, int kbase, int g, int q_lane, int kend) {
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int q = q_lane + qi * 16;
    // every mask byte of this lane is loaded up front, unconditionally (a short-circuit `dead || byte` compiled to one branch, one
    // load and one s_waitcnt vmcnt(0) PER ELEMENT: 16 NQ serialised global round trips per tile) -- as BUFFER loads: one 32-bit
    // offset register + immediates instead of a 64-bit address per byte, and the hardware's range check (bytes past the end of
    // the mask read as 0) instead of per-element clamps; keys >= Tk are dead by kend anyway.
    uint32_t mbits = 0u;
    if (p.key_pad) {
      const int off = (int)((int64_t)b * p.m_sb + (int64_t)(q < p.Tq ? q : p.Tq - 1) * p.m_sq) + kbase + g * 4;
#pragma unroll
      for (int i = 0; i < NKF * 4; ++i)
        mbits |= (uint32_t)(__builtin_amdgcn_raw_buffer_load_b8(mask_rsrc(p), off + (i >> 2) * 16 + (i & 3), 0, 0) != 0) << i;
    }
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kg = kbase + kf * 16 + g * 4 + r;
        const bool dead = (kg >= kend) | (p.causal != 0 & kg > q) | (((mbits >> (kf * 4 + r)) & 1u) != 0u);
        s[qi][kf][r] = dead ? -INFINITY : s[qi][kf][r];
      }
  }
}

// the domain of the bf16 / d = 64 kernels; each arm's further conditions are written next to it in attention.hip
inline bool fast_ok(const AttnArgs& p, int d, int dtype) {
  if (p.q_st >= (1 << 22) || p.k_st >= (1 << 22) || p.v_st >= (1 << 22) || p.o_st >= (1 << 22)) return false;   // 32-bit in-tile byte offsets
  if (p.key_pad && (int64_t)(p.B - 1) * p.m_sb + (int64_t)(p.Tq - 1) * p.m_sq + p.Tk >= ((int64_t)1 << 31)) return false;   // 32-bit mask offsets
  return dtype == ASR_BF16 && d == HD && p.vec && p.Tq > 0 && p.Tk > 0;
}

}  // namespace asr_attn
