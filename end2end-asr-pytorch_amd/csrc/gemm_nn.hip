// ================================================================================================ NN (data gradient)
// C[M,N] (op)= alpha * sum_k A[m,k] * B[k,n]  with B = W (K_red, N_out) in its NATURAL master layout: dX = dY . W needs the
// contraction index as W's slow axis, so the B operand is built with the transposing LDS read (bf16) / 4-byte reads (fp32)
// exactly like gemm_tn -- no transposed weight shadows.  A staging, pipeline and epilogue are those of gemm_glds (BN = 64).
// NST = 1: one LDS stage, "load, wait, compute" -- the form for launches of several workgroups per CU, which hide each other's load
// latency.  NST = 3 (bf16): a private ring of hand-issued LDS-DMA stages with counted waits and ONE barrier per K step, for launches
// that leave a CU with a single workgroup (the decoder's data gradients: 1600 rows x 512 columns = 200 blocks over K = 1536 - 4416):
// there nothing else covers the ~0.9 us a K step spends waiting for its operands.
#include "common.h"
#include "gemm.h"
#include "gemm_big.h"

namespace {

template <typename T, typename TO, int BM, int NST = 1>
__device__ __forceinline__ void gemm_nn_body(const GemmArgs& p, const int bid, const int nwg, unsigned char* smem) {
  using P = TnPack<T>;
  constexpr int ESZ = (int)sizeof(T);
  constexpr int BN = 64, BKB = 128;
  constexpr int BKR = BKB / ESZ;                 // reduction rows per stage: 64 (bf16) / 32 (fp32)
  constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
  constexpr int STAGE = BM * BKB + BKR * P::ROWB;
  constexpr int CPITCH = BN * 4 + 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, g = lane >> 4;
  const int tile = asr_xcd_linear(bid, nwg);
  const int m0 = (tile / p.tiles_n) * BM, n0 = (tile % p.tiles_n) * BN;
  const unsigned char* A = static_cast<const unsigned char*>(p.A);
  const unsigned char* B = static_cast<const unsigned char*>(p.B);
  const int nk = (p.K + BKR - 1) / BKR;          // a partial last stage: A's columns past K are zero (caller), B's rows are clamped
  const int b_chunks = (int)(p.ldb * ESZ / 16);

  // ---- the storage-dtype epilogue's global operands (ReLU mask, `+=` base, O of the row-dot), requested all together BEFORE the
  // store loop (`request()`): none depends on the accumulators, and loaded inside the store loop every trip was a round trip of its own
  // at the tail of the block.  Piece i of a thread = chunk c = tid + 256 i of the tile (the epilogue's own mapping); a piece past M or N
  // takes a clamped, valid address (row M - 1, last whole chunk) and is never stored.  eop[0]: mask, or O (bf16) / the first half of
  // O32; eop[1]: the `+=` base, or the second half of O32 (the launchers make mask / `+=` and the row-dot exclusive).
  // The ring form (one or two workgroups per CU by its launch condition) requests them in its LAST K step, behind that step's barrier:
  // one round trip under the step's MFMAs and the staging of the tile.  Not earlier: vmcnt retires in order, so a request in front of
  // the ring makes the first counted wait wait for these cold lines (measured: the latency moves from the tail to the head,
  // profiles/nn_epilogue_operands_ab.txt); behind the last step's vmcnt(0) no LDS-DMA is in flight or follows.  The single-stage form
  // lives on workgroups per CU (64 rows: 7 at 68 registers, 5 at the 82 that 16 registers held across a K step cost; fp32 has twice
  // the pieces), so it requests them once the accumulators are staged, in front of the barrier that publishes the tile, in registers
  // the K loop and the accumulators no longer need.
  constexpr int EPCO = 16 / (int)sizeof(TO), CPRO = BN / EPCO, EP = BM * CPRO / 256;
  const bool chunked = sizeof(TO) == sizeof(T) && p.vecC && p.N % EPCO == 0 && p.ldc % EPCO == 0;
  const bool rowdot = sizeof(TO) == 2 && !p.accumulate && p.dot_out != nullptr;
  const T* Msk = rowdot ? nullptr : static_cast<const T*>(p.mask);
  uint4 eop[2][EP];
  auto request = [&]() __attribute__((always_inline)) {
    if constexpr (sizeof(TO) == sizeof(T)) {
      // one address computation and two wave-uniform tests on kernel arguments for every form: base 0 / base 1 = mask / C, O / none,
      // O32 / O32 + 16 bytes; rows of ld elements of esz bytes
      const bool o32 = rowdot && p.dot_o32 != nullptr;
      const unsigned char* b0 = static_cast<const unsigned char*>(rowdot ? (o32 ? (const void*)p.dot_o32 : p.dot_o) : (const void*)Msk);
      const unsigned char* b1 = rowdot ? (o32 ? reinterpret_cast<const unsigned char*>(p.dot_o32) + 16 : nullptr)
                                       : (p.accumulate ? static_cast<const unsigned char*>(p.C) : nullptr);
      if (!chunked) b0 = b1 = nullptr;
      const int64_t ld = rowdot ? (int64_t)p.N : p.ldc;
      const int esz = o32 ? 4 : (int)sizeof(TO);
      const int nch = p.N / EPCO;
#pragma unroll
      for (int i = 0; i < EP; ++i) {
        const int c = tid + 256 * i, row = c / CPRO, pc = c % CPRO;
        int gr = m0 + row, gch = n0 / EPCO + pc;
        gr = gr < p.M ? gr : p.M - 1;
        gch = gch < nch ? gch : nch - 1;
        const int64_t eoff = ((int64_t)gr * ld + gch * EPCO) * esz;
        if (b0) eop[0][i] = *reinterpret_cast<const uint4*>(b0 + eoff);
        if (b1) eop[1][i] = *reinterpret_cast<const uint4*>(b1 + eoff);
      }
    }
    asm volatile("" ::: "memory");                 // the loads stay where they are issued (tests/test_isa_epilogue_operands.py)
  };

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int kt, int buf) __attribute__((always_inline)) {
    unsigned char* s = smem + buf * STAGE;
    stage_glds<BM>(s, A, p.lda * ESZ, m0, p.M, (int64_t)kt * BKB, tid, wave);
    unsigned char* sb = s + BM * BKB;
#pragma unroll
    for (int i = 0; i < BKR * P::CPR / 256; ++i) {
      const int c = i * 256 + tid, row = c / P::CPR, slot = (c % P::CPR) ^ (row & 7);
      int cb = n0 * ESZ / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
      const int br = min(kt * BKR + row, p.K - 1);
      const unsigned char* src = B + (int64_t)br * p.ldb * ESZ + (int64_t)cb * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(sb + (i * 256 + wave * 64) * 16), 16, 0, 0);
    }
  };

  auto compute = [&](const unsigned char* sA) __attribute__((always_inline)) {
    const unsigned char* sB = sA + BM * BKB;
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      uint4 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int r = wm * WM + i * 16 + lr;
        a[i] = *reinterpret_cast<const uint4*>(sA + r * BKB + (((ms * 4 + g) ^ (r & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = P::template load<true>(sB, ms * (BKR / 2), lr, g, wn * WN + j * 16);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) mma16<T>(acc[i][j], a[i], b[j]);
    }
  };
  if constexpr (NST == 1) {
    // one LDS stage: load, wait, compute (see gemm_glds_kernel: workgroups per CU beat a private prefetch queue here)
    for (int kt = 0; kt < nk; ++kt) {
      if (kt > 0) __syncthreads();                 // everybody is done reading step kt-1
      stage(kt, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      compute(smem);
    }
  } else {
    static_assert(ESZ == 2, "the ring form is bf16 only");
    constexpr int PA = BM * 8 / 256, PB = BKR * P::CPR / 256;      // DMA pieces per thread and stage: A rows, B rows
    const unsigned smem_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = smem_base + (unsigned)wave * 1024u;
    // the DMA is hand issued (the compiler does not count it): its waits are the counted ones below, and the operand reads of
    // compute() carry no s_waitcnt vmcnt(0) of the compiler's own
    auto stage_ring = [&](int kt) __attribute__((always_inline)) {
      const unsigned sl = wave_lds + (unsigned)((kt % NST) * STAGE);
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const int c = i * 256 + tid, row = c >> 3, slot = (c & 7) ^ (row & 7);
        int gr = m0 + row;
        gr = gr < p.M ? gr : p.M - 1;
        asr_lds_dma16(sl + (unsigned)(i * 4096), A + (int64_t)gr * p.lda * ESZ + (int64_t)kt * BKB + slot * 16);
      }
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int c = i * 256 + tid, row = c / P::CPR, slot = (c % P::CPR) ^ (row & 7);
        int cb = n0 * ESZ / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
        const int br = min(kt * BKR + row, p.K - 1);
        asr_lds_dma16(sl + (unsigned)(BM * BKB + i * 4096), B + (int64_t)br * p.ldb * ESZ + (int64_t)cb * 16);
      }
    };
#pragma unroll
    for (int kt = 0; kt < NST - 1; ++kt)
      if (kt < nk) stage_ring(kt);
    for (int kt = 0; kt < nk; ++kt) {
      // step kt has landed once at most the pieces of the later steps are outstanding (PA + PB per step and thread, retired in order)
      const int ahead = min(NST - 2, nk - 1 - kt);
      if (ahead >= 1) asr_wait_vmcnt<PA + PB>();
      else asr_wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();                // step kt visible to every wave; every wave is done reading step kt - 1
      asm volatile("" ::: "memory");
      if (kt + NST - 1 < nk) stage_ring(kt + NST - 1);
      if (kt == nk - 1) request();
      compute(smem + (kt % NST) * STAGE);
    }
  }
  __syncthreads();                               // operand stage free for the epilogue

  // ---- storage-dtype output in whole 16-byte chunks (every data-gradient GEMM of the model).  Plain store: the tile is staged
  // in the output dtype.  Accumulate (dX added into the residual gradient): staged in fp32 so that C + acc is rounded ONCE.
  if constexpr (sizeof(TO) == sizeof(T)) {
    if (chunked) {                                 // (no global load below: the operands are the registers request() filled)
      TO* C = static_cast<TO*>(p.C);
      if (!p.accumulate) {
        constexpr int OP = BN * (int)sizeof(TO) + 16;
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *reinterpret_cast<TO*>(smem + (wm * WM + i * 16 + g * 4 + r) * OP + (wn * WN + j * 16 + lr) * sizeof(TO)) =
                  DT<TO>::to(acc[i][j][r] * p.alpha);
        if constexpr (NST == 1) request();
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EP; ++i) {
          const int c = tid + 256 * i;
          const int row = c / CPRO, col = (c % CPRO) * EPCO;
          const int gr = m0 + row, gc = n0 + col;
          if (gr >= p.M || gc >= p.N) continue;
          Chunk<TO> o;
          o.v = *reinterpret_cast<const uint4*>(smem + row * OP + col * sizeof(TO));
          if (Msk) {
            Chunk<T> m;
            m.v = eop[0][i];
#pragma unroll
            for (int e = 0; e < EPCO; ++e)
              if (!(DT<T>::from(m.e[e]) > 0.f)) o.e[e] = DT<TO>::to(0.f);
          }
          *reinterpret_cast<uint4*>(C + (int64_t)gr * p.ldc + gc) = o.v;
          if constexpr (sizeof(TO) == 2) {
            if (rowdot) {
              // the attention backward's delta = rowsum(dO * O) per head from the block that IS dO (asr_gemm_nn_rowdot; the lanes, the
              // order of additions and therefore the bits of csrc/attention_d64_bwd.hip attn_delta_bf16_d64_kernel): 8 lanes = one head
              float acc = 0.f;
              if (p.dot_o32) {
                const uint4 q0 = eop[0][i], q1 = eop[1][i];
                const float o0[4] = {__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z), __uint_as_float(q0.w)};
                const float o1[4] = {__uint_as_float(q1.x), __uint_as_float(q1.y), __uint_as_float(q1.z), __uint_as_float(q1.w)};
                // which of the two products is rounded before the add is WRITTEN OUT: left to -ffp-contract the compiler picks it by the shape of
                // the surrounding code, and delta changes in its last bit (exact-integer tests cannot see that; the dumped step can)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += __builtin_fmaf(o0[e], bf16_to_f32(o.e[e]), o1[e] * bf16_to_f32(o.e[4 + e]));
              } else {
                Chunk<bf16_t> f;
                f.v = eop[0][i];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += bf16_to_f32(f.e[e]) * bf16_to_f32(o.e[e]);
              }
              acc += __shfl_xor(acc, 4, 64);
              acc += __shfl_xor(acc, 2, 64);
              acc += __shfl_xor(acc, 1, 64);
              if ((c % CPRO) == 0) p.dot_out[((int64_t)(gr / p.dot_T) * p.dot_H + (gc >> 6)) * p.dot_T + gr % p.dot_T] = acc;
            }
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *reinterpret_cast<float*>(smem + (wm * WM + i * 16 + g * 4 + r) * CPITCH + (wn * WN + j * 16 + lr) * 4) = acc[i][j][r] * p.alpha;
        if constexpr (NST == 1) request();
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EP; ++i) {
          const int c = tid + 256 * i;
          const int row = c / CPRO, col = (c % CPRO) * EPCO;
          const int gr = m0 + row, gc = n0 + col;
          if (gr >= p.M || gc >= p.N) continue;
          TO* dst = C + (int64_t)gr * p.ldc + gc;
          Chunk<TO> o, old;
          old.v = eop[1][i];
          Chunk<T> m;
          if (Msk) m.v = eop[0][i];
#pragma unroll
          for (int e = 0; e < EPCO; ++e) {
            float v = *reinterpret_cast<const float*>(smem + row * CPITCH + (col + e) * 4);
            if (Msk && !(DT<T>::from(m.e[e]) > 0.f)) v = 0.f;
            o.e[e] = DT<TO>::to(v + DT<TO>::from(old.e[e]));
          }
          *reinterpret_cast<uint4*>(dst) = o.v;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float*>(smem + (wm * WM + i * 16 + g * 4 + r) * CPITCH + (wn * WN + j * 16 + lr) * 4) = acc[i][j][r] * p.alpha;
  __syncthreads();
  TO* C = static_cast<TO*>(p.C);
  constexpr int CPR = BN / 4;
  for (int c = tid; c < BM * CPR; c += 256) {
    const int row = c / CPR, col = (c % CPR) * 4;
    const int gr = m0 + row, gc = n0 + col;
    if (gr >= p.M || gc >= p.N) continue;
    const float4 v4 = *reinterpret_cast<const float4*>(smem + row * CPITCH + col * 4);
    float v[4] = {v4.x, v4.y, v4.z, v4.w};
    TO* dst = C + (int64_t)gr * p.ldc + gc;
    const int nvalid = min(4, p.N - gc);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < nvalid && Msk && !(DT<T>::ld(Msk + (int64_t)gr * p.ldc + gc + e) > 0.f)) v[e] = 0.f;
    if (p.vecC && nvalid == 4) {
      if constexpr (sizeof(TO) == 4) {
        float4 o = make_float4(v[0], v[1], v[2], v[3]);
        if (p.accumulate) { const float4 old = *reinterpret_cast<const float4*>(dst); o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w; }
        *reinterpret_cast<float4*>(dst) = o;
      } else {
        if (p.accumulate) {
          const uint2 old = *reinterpret_cast<const uint2*>(dst);
          v[0] += bf16_to_f32((bf16_t)(old.x & 0xffff)); v[1] += bf16_to_f32((bf16_t)(old.x >> 16));
          v[2] += bf16_to_f32((bf16_t)(old.y & 0xffff)); v[3] += bf16_to_f32((bf16_t)(old.y >> 16));
        }
        uint2 o;
        o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
        o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
        *reinterpret_cast<uint2*>(dst) = o;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < nvalid) store_out<TO>(dst + e, v[e], p.accumulate, 0);
    }
  }
}

template <typename T, typename TO, int BM, int NST = 1>
__global__ __launch_bounds__(256) void gemm_nn_kernel(GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  gemm_nn_body<T, TO, BM, NST>(p, (int)blockIdx.x, (int)gridDim.x, smem);
}

template <typename T, typename TO, int BM, int NST = 1>
int launch_nn(const GemmArgs& a, hipStream_t s) {
  GemmArgs p = a;
  const int tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + 63) / 64;
  p.ntiles = tiles_m * p.tiles_n;
  const int esz = (int)sizeof(T);
  size_t lds = (size_t)NST * (size_t)(BM * 128 + (128 / esz) * (64 * esz));      // NST operand stages
  const size_t cl = (size_t)BM * (64 * 4 + 16);
  if (cl > lds) lds = cl;
  if (lds > 48 * 1024) (void)asr_grant_lds<gemm_nn_kernel<T, TO, BM, NST>>(lds);
  hipLaunchKernelGGL((gemm_nn_kernel<T, TO, BM, NST>), dim3((unsigned)p.ntiles), dim3(256), lds, s, p);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

constexpr int64_t kNnBig = 1700;      // data gradient (asr_gemm_nn, asr_gemm_nn_tn): 128x64 tiles from this many 64x64 tiles on

}  // namespace

extern "C" int asr_gemm_nn(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const void* relu_mask,
                           int M, int N, int K, float alpha, int flags, int in_dtype, int out_dtype, hipStream_t stream) {
  ASR_CHECK_ARG(A && B && C && M >= 0 && N >= 0 && K >= 0);
  ASR_CHECK_ARG(in_dtype == ASR_F32 || in_dtype == ASR_BF16);
  ASR_CHECK_ARG(out_dtype == in_dtype || (in_dtype == ASR_BF16 && out_dtype == ASR_F32));
  if (M == 0 || N == 0) return ASR_OK;
  const int esz = in_dtype == ASR_F32 ? 4 : 2, epc = 16 / esz, bkr = 128 / esz;
  if (K <= 0 || lda % epc != 0 || ldb % epc != 0 || !aligned16(A) || !aligned16(B) || ldb < N || lda < (K + bkr - 1) / bkr * bkr)
    return ASR_EUNSUPPORTED;
  GemmArgs p{};
  p.A = A; p.B = B; p.C = C; p.mask = relu_mask;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.alpha = alpha;
  p.accumulate = (flags & ASR_GEMM_ACCUMULATE) != 0;
  p.vecC = ((((uintptr_t)C) & 15) == 0) && (ldc % 4 == 0);
  AsrProfScope prof(ASR_OP_GEMM, stream);
  if (in_dtype == ASR_BF16 && out_dtype == ASR_BF16) {    // eight-wave 128 x 128 blocks (csrc/gemm_big.hip) where the shape fills the chip with them
    BigGemmArgs q{};
    q.A = A; q.B = B; q.C = C; q.bias = nullptr; q.mask = relu_mask;
    q.lda = lda; q.ldb = ldb; q.ldc = ldc; q.M = M; q.N = N; q.K = K; q.alpha = alpha;
    q.relu = 0; q.accumulate = p.accumulate; q.out_f32 = 0;
    if (asr_gemm_big_nn(q, stream)) return ASR_OK;
  }
  const int64_t t64 = ceil_div64(M, 64) * ceil_div64(N, 64);
  const bool big = t64 >= kNnBig && M > 64;
  if (in_dtype == ASR_F32) return big ? launch_nn<float, float, 128>(p, stream) : launch_nn<float, float, 64>(p, stream);
  // a launch that leaves a CU with one workgroup or two and walks at least four K steps: the private three-stage ring (NN_RING: the
  // largest number of 64 x 64 blocks that takes it; 0 = never).  profiles/r03_gemm_nn_ring_ab.txt
  if (out_dtype == ASR_BF16 && !big && t64 <= asr_tuning("NN_RING", 512) && K >= 256)
    return launch_nn<bf16_t, bf16_t, 64, 3>(p, stream);
  if (out_dtype == ASR_BF16) return big ? launch_nn<bf16_t, bf16_t, 128>(p, stream) : launch_nn<bf16_t, bf16_t, 64>(p, stream);
  return big ? launch_nn<bf16_t, float, 128>(p, stream) : launch_nn<bf16_t, float, 64>(p, stream);
}

// asr_gemm_nn (bf16, alpha = 1, no mask, no +=) whose epilogue also writes the attention backward's delta (include/asr_hip.h)
extern "C" int asr_gemm_nn_rowdot(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, const void* O, const float* O32,
                                  float* rowdot, int M, int N, int K, int T, int dtype, hipStream_t stream) {
  ASR_CHECK_ARG(A && B && C && (O || O32) && rowdot && M >= 0 && N >= 0 && K >= 0 && T > 0);
  if (dtype != ASR_BF16 || N % 64 != 0 || M % T != 0) return ASR_EUNSUPPORTED;
  if (M == 0 || N == 0) return ASR_OK;
  if (K <= 0 || lda % 8 != 0 || ldb % 8 != 0 || !aligned16(A) || !aligned16(B) || !aligned16(C) || (O && !aligned16(O)) ||
      (O32 && !aligned16(O32)) || ldb < N || lda < (K + 63) / 64 * 64)
    return ASR_EUNSUPPORTED;
  AsrProfScope prof(ASR_OP_GEMM, stream);
  BigGemmArgs q{};
  q.A = A; q.B = B; q.C = C; q.lda = lda; q.ldb = ldb; q.ldc = N; q.M = M; q.N = N; q.K = K; q.alpha = 1.f;
  q.dot_o = O; q.dot_o32 = O32; q.dot_out = rowdot; q.dot_T = T; q.dot_H = N / 64;
  if (asr_gemm_big_nn(q, stream)) return ASR_OK;
  GemmArgs p{};
  p.A = A; p.B = B; p.C = C; p.lda = lda; p.ldb = ldb; p.ldc = N; p.M = M; p.N = N; p.K = K; p.alpha = 1.f;
  p.vecC = 1;
  p.dot_o = O; p.dot_o32 = O32; p.dot_out = rowdot; p.dot_T = T; p.dot_H = N / 64;
  const int64_t t64 = ceil_div64(M, 64) * ceil_div64(N, 64);
  if (t64 <= asr_tuning("NN_RING", 512) && K >= 256) return launch_nn<bf16_t, bf16_t, 64, 3>(p, stream);
  return launch_nn<bf16_t, bf16_t, 64>(p, stream);
}

// asr_gemm_nn whose epilogue is the second max-pool's backward (include/asr_hip.h): the encoder input projection's data gradient lands
// directly in the un-pooled NHWC gradient of conv.7's output.  Eight-wave 128 x 128 blocks only (csrc/gemm_big.hip).
extern "C" int asr_gemm_nn_poolbwd(const void* A, int64_t lda, const void* Bp, int64_t ldb, const uint8_t* code_cl, void* dy, int M, int K,
                                   int H2, int W2, int C, int dtype, hipStream_t stream) {
  ASR_CHECK_ARG(A && Bp && code_cl && dy && M >= 0 && K >= 0 && H2 > 0 && W2 > 0 && C > 0);
  const int64_t N = (int64_t)H2 * C;
  if (dtype != ASR_BF16 || C % 8 != 0 || M % W2 != 0 || N >= ((int64_t)1 << 30)) return ASR_EUNSUPPORTED;
  if (M == 0) return ASR_OK;
  if (K <= 0 || K % 64 != 0 || lda % 8 != 0 || ldb % 8 != 0 || !aligned16(A) || !aligned16(Bp) || !aligned16(dy) || (((uintptr_t)code_cl) & 7) != 0 ||
      ldb < N || lda < K)
    return ASR_EUNSUPPORTED;
  AsrProfScope prof(ASR_OP_GEMM, stream);
  BigGemmArgs q{};
  q.A = A; q.B = Bp; q.C = dy; q.lda = lda; q.ldb = ldb; q.ldc = N; q.M = M; q.N = (int)N; q.K = K; q.alpha = 1.f;
  q.pool_code = code_cl; q.pool_H2 = H2; q.pool_W2 = W2; q.pool_C = C;
  return asr_gemm_big_nn(q, stream) ? ASR_OK : ASR_EUNSUPPORTED;
}

namespace {

// ------------------------------------------------------------------------------------------------ TN on quadrant waves (bf16)
// The weight-gradient contraction again, with the FOOTPRINT of the data-gradient kernel (64 x 64 tile of dW, waves in a 2 x 2
// grid of 32 x 32 quadrants, every wave contracts every row of a 64-row stage: 16 accumulator registers, one 16 KB LDS stage,
// no cross-wave reduction) so that both can be workgroups of ONE launch (gemm_nn_tnq_kernel below): a layer's dX and dW used to
// be two launches on two streams, and every fork / join of a replayed graph is a 5-10 us hole on the main stream (88 of them
// per step).  Partial tiles go to the workspace [split][tile][64][64]; asr_tn_reduce_multi folds all layers at once.
__device__ __forceinline__ void gemm_tnq_body(const TnArgs& p, const int bid, const int nwg, unsigned char* smem) {
  using P = TnPack<bf16_t>;
  constexpr int RM = 64, TILEB = RM * P::ROWB;                    // 8 KB per operand
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int wid = asr_xcd_linear(bid, nwg);
  const int split = wid / p.ntiles, tile = wid % p.ntiles;
  const int n0 = (tile / p.tiles_k) * 64, k0 = (tile % p.tiles_k) * 64;
  const int m_beg = split * p.m_per_split, m_end = min(p.M, m_beg + p.m_per_split);
  const int nstage = (m_end - m_beg + RM - 1) / RM;
  const unsigned char* A = static_cast<const unsigned char*>(p.A);
  const unsigned char* B = static_cast<const unsigned char*>(p.B);
  const int a_chunks = (int)(p.lda * 2 / 16), b_chunks = (int)((p.ldb >= p.K ? p.ldb : (int64_t)((p.K + 7) / 8 * 8)) * 2 / 16);
  const unsigned char* zero = reinterpret_cast<const unsigned char*>(&tn_zero_page);

  unsigned offA[2], offB[2];
  int rowi[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = i * 256 + tid, row = c >> 3, slot = (c & 7) ^ (row & 7);
    int ca = n0 * 2 / 16 + slot; ca = ca < a_chunks ? ca : a_chunks - 1;       // columns past N / K are never stored
    int cb = k0 * 2 / 16 + slot; cb = cb < b_chunks ? cb : b_chunks - 1;
    offA[i] = (unsigned)(row * (int)p.lda * 2 + ca * 16);
    offB[i] = (unsigned)(row * (int)p.ldb * 2 + cb * 16);
    rowi[i] = row;
  }

  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum[2] = {0.f, 0.f};
  const bool do_colsum = p.colsum != nullptr && k0 == 0 && wk == 0;

  for (int st = 0; st < nstage; ++st) {
    if (st > 0) __syncthreads();                 // everybody is done reading stage st-1
    const int64_t mrow = m_beg + (int64_t)st * RM;
    const unsigned char* ba = A + mrow * p.lda * 2;
    const unsigned char* bb = B + mrow * p.ldb * 2;
    const int valid = m_end - (int)mrow;         // rows of this stage that exist (uniform); the others come from a page of zeros
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool in = rowi[i] < valid;
      unsigned char* d = smem + (i * 256 + wave * 64) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in ? ba + offA[i] : zero),
                                       (__attribute__((address_space(3))) void*)d, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in ? bb + offB[i] : zero),
                                       (__attribute__((address_space(3))) void*)(d + TILEB), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned char* sA = smem;
    const unsigned char* sB = smem + TILEB;
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      uint4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = P::load(sA, ms * 32, lr, g, wn * 32 + i * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = P::load(sB, ms * 32, lr, g, wk * 32 + j * 16);
      if (do_colsum) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          Chunk<bf16_t> c; c.v = a[i];
#pragma unroll
          for (int e = 0; e < 8; ++e) bsum[i] += bf16_to_f32(c.e[e]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mma16<bf16_t>(acc[i][j], a[i], b[j]);
    }
  }

  // ---- the wave's 32 x 32 quadrant: lane (lr, g) holds rows 4g..4g+3 of column lr of every fragment
  const bool single = nwg == p.ntiles;
  float* part = p.ws ? p.ws + ((int64_t)split * p.ntiles + tile) * 4096 : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wn * 32 + i * 16 + g * 4 + r, gn = n0 + row;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wk * 32 + j * 16 + lr, gk = k0 + col;
        const float v = acc[i][j][r];
        if (part) part[row * 64 + col] = v;
        else if (gn < p.N && gk < p.K) {
          float* dst = p.C + (int64_t)gn * p.ldc + gk;
          if (single) *dst += v; else atomicAdd(dst, v);
        }
      }
    }
  if (do_colsum) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int gn = n0 + wn * 32 + i * 16 + lr;
      if (g == 0 && gn < p.N) atomicAdd(p.colsum + gn, v);
    }
  }
}

// C tile += the m-slices of its partial tiles [split][tile][64][64]: one workgroup folds a quarter tile (fixed order).
__device__ __forceinline__ void tn_fold_block(const float* __restrict__ ws, float* C, const int64_t ldc, const int N, const int K,
                                              const int splits, const int bid) {
  const int tiles_k = (K + 63) / 64, ntiles = ((N + 63) / 64) * tiles_k;
  const int tile = bid >> 2;
  if (tile >= ntiles) return;
  const int e = ((bid & 3) * 256 + threadIdx.x) * 4;               // 4 consecutive columns of one row of the tile
  const int row = e >> 6, col = e & 63;
  const int gn = (tile / tiles_k) * 64 + row, gk = (tile % tiles_k) * 64 + col;
  if (gn >= N || gk >= K) return;
  const float* src = ws + (int64_t)tile * 4096 + e;
  const int64_t step = (int64_t)ntiles * 4096;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int sp = 0; sp < splits; ++sp) {
    const float4 t = *reinterpret_cast<const float4*>(src + sp * step);
    v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
  }
  float* dst = C + (int64_t)gn * ldc + gk;
  if (gk + 3 < K && ((((uintptr_t)dst) & 15) == 0)) {
    float4 o = *reinterpret_cast<float4*>(dst);
    o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
    *reinterpret_cast<float4*>(dst) = o;
  } else {
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (gk + i < K) dst[i] += vv[i];
  }
}

// dX workgroups and dW workgroups of one linear layer in ONE launch: the first n_tn workgroups are the (longer) weight-gradient
// tiles, then the n_nn data-gradient tiles, then -- software pipelining across launches -- the workgroups that fold the partial
// tiles the PREVIOUS layer's launch left behind (HBM-bound, they ride under the MFMA-bound tiles of this one).
struct TnFoldArgs {
  const float* ws; float* C; int64_t ldc; int N, K, splits;
};
template <int BM>
__global__ __launch_bounds__(256) void gemm_nn_tnq_kernel(GemmArgs pn, TnArgs pt, TnFoldArgs pf, int n_tn, int n_nn) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int bid = (int)blockIdx.x;
  if (bid < n_tn) gemm_tnq_body(pt, bid, n_tn, smem);
  else if (bid < n_tn + n_nn) gemm_nn_body<bf16_t, bf16_t, BM>(pn, bid - n_tn, n_nn, smem);
  else tn_fold_block(pf.ws, pf.C, pf.ldc, pf.N, pf.K, pf.splits, bid - n_tn - n_nn);
}

// Second stage for up to TN_MULTI layers in one launch (blockIdx.y = layer).
constexpr int TN_MULTI = 48;
struct TnMultiArgs {
  const float* ws[TN_MULTI];
  float* C[TN_MULTI];
  int ldc[TN_MULTI], N[TN_MULTI], K[TN_MULTI], splits[TN_MULTI];
};
__global__ __launch_bounds__(256) void tn_reduce_multi_kernel(TnMultiArgs q) {
  const int l = blockIdx.y;
  tn_fold_block(q.ws[l], q.C[l], q.ldc[l], q.N[l], q.K[l], q.splits[l], (int)blockIdx.x);
}

}  // namespace

// ---- one launch for a linear layer's backward: dx (M,K) (+)= dy (M,N) . w (N,K) [ReLU mask]  AND  the partial sums of
// dw (N,K) += dy^T . x (M,K), db (N) += column sums of dy.  bf16 operands.  splits = 0: chosen here.
static int nn_tn_splits(int M, int splits, int* m_per_split) {
  const int stages = (M + 63) / 64;
  if (splits <= 0) {
    constexpr int per = 16;           // 64-row stages of one weight-gradient workgroup
    splits = (stages + per - 1) / per;
  }
  splits = splits < 1 ? 1 : (splits > stages ? stages : splits);
  const int mps = ((stages + splits - 1) / splits) * 64;
  if (m_per_split) *m_per_split = mps;
  return (M + mps - 1) / mps;                                      // no empty slice
}

extern "C" int asr_gemm_nn_tn_splits(int M, int splits) { return M > 0 ? nn_tn_splits(M, splits, nullptr) : 0; }

extern "C" int64_t asr_gemm_nn_tn_workspace(int M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return (int64_t)nn_tn_splits(M, splits, nullptr) * ((N + 63) / 64) * ((K + 63) / 64) * 4096;
}

extern "C" int asr_gemm_nn_tn(const void* dy, int64_t ld_dy, const void* w, int64_t ldw, const void* x, int64_t ldx, void* dx,
                              int64_t ld_dx, const void* relu_mask, float* db, float* workspace, int64_t workspace_floats, int M,
                              int N, int K, int flags, int splits, int dtype, const float* fold_ws, float* fold_dw,
                              int64_t fold_ld, int fold_N, int fold_K, int fold_splits, hipStream_t stream) {
  ASR_CHECK_ARG(dy && w && x && dx && workspace && M > 0 && N > 0 && K > 0);
  if (dtype != ASR_BF16) return ASR_EUNSUPPORTED;
  if (ld_dy % 8 != 0 || ldw % 8 != 0 || ldx % 8 != 0 || !aligned16(dy) || !aligned16(w) || !aligned16(x) || ldw < K ||
      ld_dy < (N + 63) / 64 * 64 || ld_dy >= ((int64_t)1 << 22) || ldx >= ((int64_t)1 << 22))
    return ASR_EUNSUPPORTED;
  int m_per_split = 0;
  splits = nn_tn_splits(M, splits, &m_per_split);
  TnArgs t{};
  t.A = dy; t.B = x; t.C = nullptr; t.colsum = db; t.ws = workspace;
  t.lda = ld_dy; t.ldb = ldx; t.ldc = 0;
  t.M = M; t.N = N; t.K = K;
  t.tiles_k = (K + 63) / 64;
  t.ntiles = ((N + 63) / 64) * t.tiles_k;
  t.m_per_split = m_per_split;
  if (workspace_floats < (int64_t)splits * t.ntiles * 4096) return ASR_EINVAL;
  GemmArgs p{};
  p.A = dy; p.B = w; p.C = dx; p.mask = relu_mask;
  p.lda = ld_dy; p.ldb = ldw; p.ldc = ld_dx;
  p.M = M; p.N = K; p.K = N; p.alpha = 1.f;
  p.accumulate = (flags & ASR_GEMM_ACCUMULATE) != 0;
  p.vecC = ((((uintptr_t)dx) & 15) == 0) && (ld_dx % 4 == 0);
  p.tiles_n = (K + 63) / 64;
  const int64_t t64 = ceil_div64(M, 64) * p.tiles_n;
  const bool big = t64 >= kNnBig && M > 64;
  const int bm = big ? 128 : 64;
  p.ntiles = ((M + bm - 1) / bm) * p.tiles_n;
  const int n_tn = t.ntiles * splits;
  size_t lds = (size_t)(bm * 128 + 64 * 128);
  const size_t cl = (size_t)bm * (64 * 4 + 16);
  if (cl > lds) lds = cl;
  AsrProfScope prof(ASR_OP_GEMM, stream);
  TnFoldArgs f{};
  int n_fold = 0;
  if (fold_ws) {
    ASR_CHECK_ARG(fold_dw && fold_N > 0 && fold_K > 0 && fold_splits > 0);
    f.ws = fold_ws; f.C = fold_dw; f.ldc = fold_ld; f.N = fold_N; f.K = fold_K; f.splits = fold_splits;
    n_fold = ((fold_N + 63) / 64) * ((fold_K + 63) / 64) * 4;
  }
  const dim3 grid((unsigned)(n_tn + p.ntiles + n_fold));
  if (big) hipLaunchKernelGGL(gemm_nn_tnq_kernel<128>, grid, dim3(256), lds, stream, p, t, f, n_tn, p.ntiles);
  else hipLaunchKernelGGL(gemm_nn_tnq_kernel<64>, grid, dim3(256), lds, stream, p, t, f, n_tn, p.ntiles);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_tn_reduce_multi(const float* const* workspaces, float* const* dw, const int64_t* ld_dw, const int* N, const int* K,
                                   const int* splits, int count, hipStream_t stream) {
  ASR_CHECK_ARG(count >= 0 && (count == 0 || (workspaces && dw && ld_dw && N && K && splits)));
  for (int base = 0; base < count; base += TN_MULTI) {
    const int n = count - base < TN_MULTI ? count - base : TN_MULTI;
    TnMultiArgs q{};
    int max_tiles = 0;
    for (int i = 0; i < n; ++i) {
      ASR_CHECK_ARG(workspaces[base + i] && dw[base + i] && N[base + i] > 0 && K[base + i] > 0 && splits[base + i] > 0);
      q.ws[i] = workspaces[base + i]; q.C[i] = dw[base + i]; q.ldc[i] = (int)ld_dw[base + i];
      q.N[i] = N[base + i]; q.K[i] = K[base + i]; q.splits[i] = splits[base + i];
      const int nt = ((q.N[i] + 63) / 64) * ((q.K[i] + 63) / 64);
      if (nt > max_tiles) max_tiles = nt;
    }
    AsrProfScope prof(ASR_OP_GEMM, stream);
    hipLaunchKernelGGL(tn_reduce_multi_kernel, dim3((unsigned)(max_tiles * 4), (unsigned)n), dim3(256), 0, stream, q);
    ASR_LAUNCH_CHECK();
  }
  return ASR_OK;
}
