// NT GEMM on MFMA:  C[M,N] (op)= alpha * sum_k A[m,k] * B[n,k]  (+ bias[n]) (ReLU)
//
// Replaces every nn.Linear / Conv1d(k=1) call on the hot path (reference: models/common_layers.py:136-142,
// :181-187, :197; models/asr/transformer.py:172, :302) and, with explicitly transposed operands, their dgrad
// and wgrad.  Both operands are K-contiguous ("NT"), which is how nn.Linear stores its weight (N,K).
//
// Structure: 256 threads = 4 waves (2x2), tile BMxBN, LDS row = 128 data bytes (+16 pad) per tile row,
// register-staged global->LDS with the next tile's loads issued before the current tile's MFMAs.
#include "common.h"
#include "gemm.h"
#include "gemm_big.h"

namespace {

template <typename T, typename TO, int BM, int BN>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmArgs p) {
  constexpr int EPC = DT<T>::EPC;
  constexpr int BK = 128 / (int)sizeof(T);
  constexpr int CA = BM * 8 / 256, CB = BN * 8 / 256;
  constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sA = smem;
  unsigned char* sB = smem + BM * kPitch;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int m0 = (tile / p.tiles_n) * BM, n0 = (tile % p.tiles_n) * BN;
  const int64_t kbeg = (int64_t)blockIdx.z * p.k_per_split;
  const int64_t kend = min((int64_t)p.K, kbeg + p.k_per_split);
  const T* A = static_cast<const T*>(p.A);
  const T* B = static_cast<const T*>(p.B);

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  uint4 ra[CA], rb[CB];
  auto gload = [&](int64_t k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      int c = tid + i * 256, row = c >> 3, kc = c & 7;
      int gm = m0 + row;
      ra[i] = load_chunk<T>(A + (int64_t)gm * p.lda, k0 + kc * EPC, kend, gm < p.M, p.vecA);
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      int c = tid + i * 256, row = c >> 3, kc = c & 7;
      int gn = n0 + row;
      rb[i] = load_chunk<T>(B + (int64_t)gn * p.ldb, k0 + kc * EPC, kend, gn < p.N, p.vecB);
    }
  };
  auto swrite = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      int c = tid + i * 256, row = c >> 3, kc = c & 7;
      *reinterpret_cast<uint4*>(sA + row * kPitch + kc * 16) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      int c = tid + i * 256, row = c >> 3, kc = c & 7;
      *reinterpret_cast<uint4*>(sB + row * kPitch + kc * 16) = rb[i];
    }
  };

  if (kbeg < kend) gload(kbeg);
  for (int64_t k0 = kbeg; k0 < kend; k0 += BK) {
    swrite();
    __syncthreads();
    if (k0 + BK < kend) gload(k0 + BK);
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      uint4 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i)
        a[i] = *reinterpret_cast<const uint4*>(sA + (wm * WM + i * 16 + lr) * kPitch + (ms * 4 + g) * 16);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        b[j] = *reinterpret_cast<const uint4*>(sB + (wn * WN + j * 16 + lr) * kPitch + (ms * 4 + g) * 16);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) mma16<T>(acc[i][j], a[i], b[j]);
    }
    __syncthreads();
  }

  TO* C = static_cast<TO*>(p.C);
  const T* Msk = static_cast<const T*>(p.mask);
  const bool add_bias = p.bias != nullptr && blockIdx.z == 0;
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int col = n0 + wn * WN + j * 16 + lr;
    if (col >= p.N) continue;
    const float bv = add_bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * WM + i * 16 + g * 4 + r;
        if (row < p.M) {
          float v = acc[i][j][r] * p.alpha + bv;
          if (p.relu) v = fmaxf(v, 0.f);
          if (Msk && !(DT<T>::ld(Msk + (int64_t)row * p.ldc + col) > 0.f)) v = 0.f;
          store_out<TO>(C + (int64_t)row * p.ldc + col, v, p.accumulate, p.atomic);
        }
      }
    }
  }
}

template <typename T, typename TO, int BM, int BN>
int launch(const GemmArgs& a, int splits, hipStream_t s) {
  GemmArgs p = a;
  const int tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  dim3 grid((unsigned)(tiles_m * p.tiles_n), 1, (unsigned)splits);
  const size_t lds = (size_t)(BM + BN) * kPitch;
  hipLaunchKernelGGL((gemm_nt_kernel<T, TO, BM, BN>), grid, dim3(256), lds, s, p);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

template <typename T, typename TO>
int dispatch_tile(const GemmArgs& a, int splits, hipStream_t s) {
  const int64_t t128 = ceil_div64(a.M, 128) * ceil_div64(a.N, 128) * splits;
  const int64_t t12864 = ceil_div64(a.M, 128) * ceil_div64(a.N, 64) * splits;
  if (t128 >= 384 || (a.M > 64 && a.N > 64 && t12864 < 8)) return launch<T, TO, 128, 128>(a, splits, s);
  if (t12864 >= 384 && a.M > 64) return launch<T, TO, 128, 64>(a, splits, s);
  return launch<T, TO, 64, 64>(a, splits, s);
}


// ================================================================================================ fast path
// Direct-to-LDS staging (global_load_lds_dwordx4: no VGPR round trip, one wave instruction = 8 tile rows = 1 KiB),
// LDS image is lane-linear [row][8 x 16 B] with the 16-B slot XOR-swizzled by (row & 7) -- applied on the per-lane
// SOURCE address and again on the fragment read (the destination of an LDS-DMA cannot be permuted), two LDS stages,
// one barrier per K step, XCD-aware tile order, and an epilogue that goes through LDS so that bias / ReLU / mask /
// accumulate / atomics and the global stores are 16-byte row-contiguous.
// Requirements: 16-B aligned operands, lda/ldb multiples of a 16-B chunk, every K range a multiple of BK (128 bytes).
// NS LDS stages (ONE, or the three-stage ring of launch_fast on bf16 64 x 64 tiles), NS-1 K steps of LDS-DMA in flight.  A deeper pipeline needs counted
// s_waitcnt vmcnt(N), a RAW s_barrier (__syncthreads() carries a fence that drains every pending LDS-DMA write) and operand
// reads the compiler cannot see (see the asm block below).  Measured (profiles/r01_microbench_v4.txt, MI355X): with all of that
// in place, MORE stages are SLOWER on every shape of this model -- 6400x2048x512: 33.0 / 39.6 / 44 / 55 us for 1 / 2 / 3 / 4
// stages; 3200x4364x512: 37.9 / 47.9 / 53 / 66 us.  The 64x64 tile moves 32 flop per byte through L2, the kernel lives on
// workgroups per CU (8 at one stage), and the other workgroups hide the load latency better than a private prefetch queue.
template <typename T, typename TO, int BM, int BN, int NS>
__global__ __launch_bounds__(256) void gemm_glds_kernel(GemmArgs p) {
  constexpr int ESZ = (int)sizeof(T);
  constexpr int BKB = 128;                       // bytes of K per stage row
  constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
  constexpr int STAGE = (BM + BN) * BKB;
  constexpr int LPS = (BM + BN) * 8 / 256;       // LDS-DMA instructions per thread per stage
  constexpr int CPITCH = BN * 4 + 16;            // fp32 C tile staged in LDS for the epilogue
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, g = lane >> 4;
  // XCD-aware order: blocks b, b+8, b+16 ... run on the same XCD (private L2) -> give them consecutive tiles
  // The linear work id is (split, tile) with the tile index fastest, so all tiles of one K slice (which share their
  // A and B panels) sit next to each other on one XCD's L2.
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int wid = asr_xcd_linear(bid, nwg);
  const int split = wid / p.ntiles, tile = wid % p.ntiles;
  const int m0 = (tile / p.tiles_n) * BM, n0 = (tile % p.tiles_n) * BN;
  const int64_t kbeg = (int64_t)split * p.k_per_split;
  const int64_t kend = min((int64_t)p.K, kbeg + p.k_per_split);
  const unsigned char* A = static_cast<const unsigned char*>(p.A);
  const unsigned char* B = static_cast<const unsigned char*>(p.B);
  int nk = (int)((kend - kbeg) * ESZ / BKB);
#ifdef ASR_TUNE_ABLATE
  if (p.ablate & 16) nk = 0;
#endif

  // the chunked epilogue's bias values (one per fragment column of the lane), requested before the first operand piece: they do not
  // depend on the accumulators, and loaded behind the K loop they were a round trip in front of the tile's staging
  float bvj[FN];
  if constexpr (sizeof(TO) == sizeof(T)) {
    constexpr int EPCO = 16 / (int)sizeof(TO);
    const bool add_bias = p.bias != nullptr && split == 0 && p.vecC && !p.atomic && !p.accumulate && p.N % EPCO == 0 && p.ldc % EPCO == 0;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = n0 + wn * WN + j * 16 + lr;
      bvj[j] = (add_bias && col < p.N) ? p.bias[col] : 0.f;
    }
  }
  asm volatile("" ::: "memory");

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int kt, int buf) __attribute__((always_inline)) {
    unsigned char* s = smem + buf * STAGE;
    const int64_t kb = (kbeg * ESZ) + (int64_t)kt * BKB;
#ifdef ASR_TUNE_ABLATE
    if (!(p.ablate & 1) || kt == 0) stage_glds<BM>(s, A, p.lda * ESZ, m0, p.M, kb, tid, wave);
    if (!(p.ablate & 2) || kt == 0) stage_glds<BN>(s + BM * BKB, B, p.ldb * ESZ, n0, p.N, kb, tid, wave);
#else
    stage_glds<BM>(s, A, p.lda * ESZ, m0, p.M, kb, tid, wave);
    stage_glds<BN>(s + BM * BKB, B, p.ldb * ESZ, n0, p.N, kb, tid, wave);
#endif
  };

#pragma unroll
  for (int st = 0; st < NS - 1; ++st)
    if (st < nk) stage(st, st);
  int buf = 0;                                   // LDS stage of K step kt
  for (int kt = 0; kt < nk; ++kt) {
    if (NS == 1) {                               // one stage: load, wait, compute; the overlap comes from the other workgroups
      if (kt > 0) __builtin_amdgcn_s_barrier(); // everybody is done reading step kt-1
      stage(kt, 0);
    }
    // this thread's DMA of step kt has landed once at most the later steps' loads are outstanding
    const int ahead = min(NS - 2, nk - 1 - kt);
    if (NS >= 4 && ahead >= 2) asr_wait_vmcnt<2 * LPS>();
    else if (NS >= 3 && ahead >= 1) asr_wait_vmcnt<LPS>();
    else asr_wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                // step kt visible to all waves; everybody is done reading step kt-1
    if (NS > 1 && kt + NS - 1 < nk) stage(kt + NS - 1, buf == 0 ? NS - 1 : buf - 1);      // refill the stage step kt-1 used
    const unsigned char* sA = smem + buf * STAGE;
    const unsigned char* sB = sA + BM * BKB;
    if constexpr (FM == 2 && FN == 2 && NS > 2) {
      // Operand fragments by inline asm: for a compiler-visible LDS read the waitcnt pass cannot tell the read apart from the
      // LDS-DMA writes still in flight for later stages and inserts s_waitcnt vmcnt(0) -- which serialises the pipeline again.
      // One block = the 8 reads of this K step + the wait for them; rows i*16 apart share their swizzle slot (offset:2048).
      const int ra = wm * WM + lr, rb = wn * WN + lr;
      const uint32_t aa0 = (uint32_t)(uintptr_t)(sA + ra * BKB + ((g ^ (ra & 7)) << 4));
      const uint32_t aa1 = (uint32_t)(uintptr_t)(sA + ra * BKB + (((4 + g) ^ (ra & 7)) << 4));
      const uint32_t ab0 = (uint32_t)(uintptr_t)(sB + rb * BKB + ((g ^ (rb & 7)) << 4));
      const uint32_t ab1 = (uint32_t)(uintptr_t)(sB + rb * BKB + (((4 + g) ^ (rb & 7)) << 4));
      u32x4_t fa[2][2], fb[2][2];                  // [ms][fragment]
      asm volatile(
          "ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:2048\n\t"
          "ds_read_b128 %2, %10\n\tds_read_b128 %3, %10 offset:2048\n\t"
          "ds_read_b128 %4, %9\n\tds_read_b128 %5, %9 offset:2048\n\t"
          "ds_read_b128 %6, %11\n\tds_read_b128 %7, %11 offset:2048\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(fa[0][0]), "=&v"(fa[0][1]), "=&v"(fb[0][0]), "=&v"(fb[0][1]), "=&v"(fa[1][0]), "=&v"(fa[1][1]), "=&v"(fb[1][0]),
            "=&v"(fb[1][1])
          : "v"(aa0), "v"(aa1), "v"(ab0), "v"(ab1)
          : "memory");
#pragma unroll
      for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            mma16<T>(acc[i][j], __builtin_bit_cast(uint4, fa[ms][i]), __builtin_bit_cast(uint4, fb[ms][j]));
    } else {
#pragma unroll
      for (int ms = 0; ms < 2; ++ms) {
        uint4 a[FM], b[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const int r = wm * WM + i * 16 + lr;
          a[i] = *reinterpret_cast<const uint4*>(sA + r * BKB + (((ms * 4 + g) ^ (r & 7)) << 4));
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int r = wn * WN + j * 16 + lr;
          b[j] = *reinterpret_cast<const uint4*>(sB + r * BKB + (((ms * 4 + g) ^ (r & 7)) << 4));
        }
#ifdef ASR_TUNE_ABLATE
        if (p.ablate & 8) {
#pragma unroll
          for (int i = 0; i < FM; ++i) asm volatile("" :: "v"(a[i].x));
#pragma unroll
          for (int j = 0; j < FN; ++j) asm volatile("" :: "v"(b[j].x));
          continue;
        }
#endif
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) mma16<T>(acc[i][j], a[i], b[j]);
      }
    }
    buf = buf + 1 == NS ? 0 : buf + 1;
  }
  __syncthreads();                               // all waves are done with the operand stages before the epilogue reuses them

  // ---- epilogue, storage-dtype output with whole 16-byte chunks (every bf16 / fp32-parity activation GEMM of the model):
  // alpha / bias / ReLU on the accumulators, the tile staged in the OUTPUT dtype (half the LDS bytes of an fp32 tile in
  // bf16), then one 16-byte LDS read, mask read, optional read-modify-write and store per EPC columns
  if constexpr (sizeof(TO) == sizeof(T)) {
    constexpr int EPCO = 16 / (int)sizeof(TO);
    if (p.vecC && !p.atomic && !p.accumulate && p.N % EPCO == 0 && p.ldc % EPCO == 0) {     // (+= keeps the single rounding of the fp32 path)
      constexpr int OP = BN * (int)sizeof(TO) + 16;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = wn * WN + j * 16 + lr;
        const float bv = bvj[j];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = acc[i][j][r] * p.alpha + bv;
            if (p.relu) v = fmaxf(v, 0.f);
            *reinterpret_cast<TO*>(smem + (wm * WM + i * 16 + g * 4 + r) * OP + col * sizeof(TO)) = DT<TO>::to(v);
          }
      }
      __syncthreads();
      TO* C = static_cast<TO*>(p.C);
      const T* Msk = static_cast<const T*>(p.mask);
      constexpr int CPRO = BN / EPCO;
      for (int c = tid; c < BM * CPRO; c += 256) {
        const int row = c / CPRO, col = (c % CPRO) * EPCO;
        const int gr = m0 + row, gc = n0 + col;
        if (gr >= p.M || gc >= p.N) continue;
        Chunk<TO> o;
        o.v = *reinterpret_cast<const uint4*>(smem + row * OP + col * sizeof(TO));
        TO* dst = C + (int64_t)gr * p.ldc + gc;
        if (Msk) {
          Chunk<T> m;
          m.v = *reinterpret_cast<const uint4*>(Msk + (int64_t)gr * p.ldc + gc);
#pragma unroll
          for (int e = 0; e < EPCO; ++e)
            if (!(DT<T>::from(m.e[e]) > 0.f)) o.e[e] = DT<TO>::to(0.f);
        }
#ifdef ASR_TUNE_ABLATE
        if (p.ablate & 4) continue;
#endif
        *reinterpret_cast<uint4*>(dst) = o.v;
      }
      return;
    }
  }
  // ---- general epilogue: accumulators -> LDS (fp32, padded rows) -> row-contiguous 16-byte global accesses
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float*>(smem + (wm * WM + i * 16 + g * 4 + r) * CPITCH + (wn * WN + j * 16 + lr) * 4) = acc[i][j][r] * p.alpha;
  __syncthreads();
  TO* C = static_cast<TO*>(p.C);
  const T* Msk = static_cast<const T*>(p.mask);
  const bool add_bias = p.bias != nullptr && split == 0;
  constexpr int CPR = BN / 4;                    // 4-column chunks per tile row
  for (int c = tid; c < BM * CPR; c += 256) {
    const int row = c / CPR, col = (c % CPR) * 4;
    const int gr = m0 + row, gc = n0 + col;
    if (gr >= p.M || gc >= p.N) continue;
    const float4 v4 = *reinterpret_cast<const float4*>(smem + row * CPITCH + col * 4);
    float v[4] = {v4.x, v4.y, v4.z, v4.w};
    TO* dst = C + (int64_t)gr * p.ldc + gc;
    const int nvalid = min(4, p.N - gc);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < nvalid) {
        if (add_bias) v[e] += p.bias[gc + e];
        if (p.relu) v[e] = fmaxf(v[e], 0.f);
        if (Msk && !(DT<T>::ld(Msk + (int64_t)gr * p.ldc + gc + e) > 0.f)) v[e] = 0.f;
      }
    }
    if (p.vecC && nvalid == 4 && !p.atomic) {
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
        if (e < nvalid) store_out<TO>(dst + e, v[e], p.accumulate, p.atomic);
    }
  }
}

template <typename T, typename TO, int BM, int BN, int NS>
int launch_fast_ns(const GemmArgs& a, int splits, hipStream_t s) {
  GemmArgs p = a;
  const int tiles_m = (p.M + BM - 1) / BM;
  p.tiles_n = (p.N + BN - 1) / BN;
  p.ntiles = tiles_m * p.tiles_n;
  dim3 grid((unsigned)(p.ntiles * splits), 1, 1);
  size_t lds = (size_t)NS * (BM + BN) * 128;
  // epilogue staging: the tile in the OUTPUT dtype when the 16-byte-chunk epilogue applies (same test as in the kernel), else fp32.
  // (Sizing it as fp32 always cost the 128 x 128 tile two of its four workgroups per CU.)
  constexpr int EPCO = 16 / (int)sizeof(TO);
  const bool chunked = sizeof(TO) == sizeof(T) && p.vecC && !p.atomic && !p.accumulate && p.N % EPCO == 0 && p.ldc % EPCO == 0;
  const size_t cl = chunked ? (size_t)BM * (BN * sizeof(TO) + 16) : (size_t)BM * (BN * 4 + 16);
  if (cl > lds) lds = cl;
  if (lds > 48 * 1024) (void)asr_grant_lds<gemm_glds_kernel<T, TO, BM, BN, NS>>(lds);
  hipLaunchKernelGGL((gemm_glds_kernel<T, TO, BM, BN, NS>), grid, dim3(256), lds, s, p);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
template <typename T, typename TO, int BM, int BN>
int launch_fast(const GemmArgs& a, int splits, hipStream_t s) {
  // LDS stages: ONE wherever several workgroups share a CU (they cover each other's load latency: the measurement in front of
  // gemm_glds_kernel); a launch of at most NT_RING 64 x 64 blocks leaves a CU with one workgroup or two, and there the private
  // three-stage ring wins (the decoder's 3200 x 512 projections over K = 2048: 32 -> ~14 us; profiles/r03_gemm_nn_ring_ab.txt)
  if constexpr (BM == 64 && BN == 64 && sizeof(T) == 2) {
    const int64_t blocks = ceil_div64(a.M, BM) * ceil_div64(a.N, BN) * splits;
    if (a.K >= 256 && blocks <= asr_tuning("NT_RING", 512)) return launch_fast_ns<T, TO, BM, BN, 3>(a, splits, s);
  }
  return launch_fast_ns<T, TO, BM, BN, 1>(a, splits, s);
}

template <typename T, typename TO>
int dispatch_fast(const GemmArgs& a, int splits, hipStream_t s) {
  {                                                            // tuning hook (tools/microbench.py): -1 = automatic
    const int force = (int)asr_tuning("GEMM_TILE", -1);
    if (force == 0) return launch_fast<T, TO, 128, 128>(a, splits, s);
    if (force == 1) return launch_fast<T, TO, 128, 64>(a, splits, s);
    if (force == 2) return launch_fast<T, TO, 64, 64>(a, splits, s);
  }
  // Measured on MI355X (tools/microbench.py, profiles/r01_microbench_v5.txt): 64x64 tiles (8 workgroups per CU) win while the
  // grid is small; once 128x64 tiles still give >= ~1200 workgroups they tie or win (half the B-operand traffic through L2):
  // 6400x2048x512 26.4 vs 27.5 us, 6400x5120x512 57.8 vs 71.6 us.  The fp32-output epilogue (vocabulary logits) prefers 64x64.
  const int64_t t64 = ceil_div64(a.M, 64) * ceil_div64(a.N, 64) * splits;
  if (t64 >= 2400 && a.M > 64 && sizeof(TO) == sizeof(T)) return launch_fast<T, TO, 128, 64>(a, splits, s);
  return launch_fast<T, TO, 64, 64>(a, splits, s);
}

}  // namespace

extern "C" int asr_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                           const float* bias, const void* relu_mask, int M, int N, int K,
                           float alpha, int flags, int splits, int in_dtype, int out_dtype, hipStream_t stream) {
  ASR_CHECK_ARG(A && B && C && M >= 0 && N >= 0 && K >= 0);
  if (M == 0 || N == 0) return ASR_OK;
  ASR_CHECK_ARG(in_dtype == ASR_F32 || in_dtype == ASR_BF16);
  ASR_CHECK_ARG(out_dtype == ASR_F32 || out_dtype == ASR_BF16);
  ASR_CHECK_ARG(!(in_dtype == ASR_F32 && out_dtype == ASR_BF16));
  const int esz = in_dtype == ASR_F32 ? 4 : 2, epc = 16 / esz, bk = 128 / esz;
  GemmArgs p{};
  p.A = A; p.B = B; p.C = C; p.bias = bias; p.mask = relu_mask;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  p.alpha = alpha;
  p.relu = (flags & ASR_GEMM_RELU) != 0;
  p.accumulate = (flags & ASR_GEMM_ACCUMULATE) != 0;
  if (splits == 0) {
    // auto: fp32 atomics are expensive (~10 ns each), so split only while the 64x64 grid cannot fill the chip
    splits = 1;
    if (p.accumulate && out_dtype == ASR_F32 && !p.relu && !relu_mask) {
      const int64_t t64 = ceil_div64(M, 64) * ceil_div64(N, 64);
      int64_t sp = (256 + t64 / 2) / (t64 > 0 ? t64 : 1);
      if (sp > 4) sp = 4;
      if (sp > K / (4 * bk)) sp = K / (4 * bk);
      if (sp >= 2) splits = (int)sp;
    }
  }
  if (splits < 1) splits = 1;
  int kps = (int)(ceil_div64(ceil_div64(K > 0 ? K : 1, splits), bk) * bk);
  splits = (int)ceil_div64(K > 0 ? K : 1, kps);
  p.k_per_split = kps;
  p.atomic = 0;
  if (splits > 1) {
    // split-K partial sums are combined with fp32 atomics: the destination must already hold the value to add to
    ASR_CHECK_ARG(out_dtype == ASR_F32 && p.accumulate && !p.relu && !relu_mask);
    p.atomic = 1;
  }
  p.vecA = aligned16(A) && (lda % epc == 0) && (K % epc == 0);
  p.vecB = aligned16(B) && (ldb % epc == 0) && (K % epc == 0);
  const int oesz = out_dtype == ASR_F32 ? 4 : 2;
  p.vecC = ((((uintptr_t)C) & 15) == 0) && (ldc % 4 == 0) && (oesz == 4 || ldc % 4 == 0);
  AsrProfScope prof(ASR_OP_GEMM, stream);
#ifdef ASR_TUNE_ABLATE
  p.ablate = (int)asr_tuning("GEMM_ABLATE", 0);
#endif
  // eight-wave 256 x 256 / 128 x 128 blocks (csrc/gemm_big.hip) for the bf16 linear layers whose shape fills the chip with them
  if (in_dtype == ASR_BF16 && splits == 1 && !relu_mask) {
    BigGemmArgs q{};
    q.A = A; q.B = B; q.C = C; q.bias = bias; q.mask = nullptr;
    q.lda = lda; q.ldb = ldb; q.ldc = ldc; q.M = M; q.N = N; q.K = K; q.alpha = alpha;
    q.relu = p.relu; q.accumulate = p.accumulate; q.out_f32 = out_dtype == ASR_F32;
    if (asr_gemm_big_nt(q, stream)) return ASR_OK;
  }
  // fast path: LDS-DMA staging needs whole 16-B chunks everywhere and whole 128-byte K steps
  const bool fast = p.vecA && p.vecB && K > 0 && (K % bk == 0) && (kps % bk == 0);
  if (fast) {
    if (in_dtype == ASR_F32) return dispatch_fast<float, float>(p, splits, stream);
    if (out_dtype == ASR_BF16) return dispatch_fast<bf16_t, bf16_t>(p, splits, stream);
    return dispatch_fast<bf16_t, float>(p, splits, stream);
  }
  if (in_dtype == ASR_F32) return dispatch_tile<float, float>(p, splits, stream);
  if (out_dtype == ASR_BF16) return dispatch_tile<bf16_t, bf16_t>(p, splits, stream);
  return dispatch_tile<bf16_t, float>(p, splits, stream);
}
