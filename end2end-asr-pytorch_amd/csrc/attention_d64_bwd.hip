// Attention backward for bf16 / head dim 64 in two halves (the data path of attention_d64_fwd.hip): dQ workgroups walk the key tiles,
// dK / dV workgroups walk the query tiles, both recompute P from lse; one launch runs both kinds of workgroup (attn_bwd_both), a call
// that asks for one part gets that half alone.  delta = rowsum(dO * O) is a kernel of its own.  Short key sequences take the one-pass
// kernel of attention_d64_bwd_fused.hip instead (attention.hip decides).
#include "attention_d64.h"

namespace asr_attn {
namespace {

// ================================================================================================ backward: dQ
// Same work split as the forward (wave = 32 queries, 64-key K / V tiles double buffered in LDS):
//   S^T = K Q^T, dP^T = V dO^T (A operands: K / V rows from LDS; B: Q / dO rows in registers)
//   P = exp2(S c - lse c'), dS = P (keep/(1-p) dP - delta)
//   dQ^T[d][q] += K^T[d][key] dS^T[key][q]   (A: transposing reads of the natural K tile; B: dS from the accumulators)
// NQ as in the forward kernel: 16 NQ queries per wave.  In the two backward kernels 16-row waves win at every length (measured:
// (32, 8, 800, 800) p = 0.1 backward 324 -> 301 us, (16, 8, 795, 795) 185 -> 166 us; the forward loses 4 - 9 % there), so they are the default.
template <int NQ>
__device__ __forceinline__ void attn_bwd_dq_body(const AttnArgs& p, const int vid, unsigned char* smem) {
  constexpr int FQW = 64 * NQ;
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nqb = (p.Tq + FQW - 1) / FQW;
  const int bh = vid / nqb, qb = vid - bh * nqb;
  const int b = bh / p.H, h = bh - b * p.H;
  const int qw = qb * FQW + wave * 16 * NQ;
  const bf16_t* Qb = static_cast<const bf16_t*>(p.Q) + (int64_t)b * p.q_sb + (int64_t)h * HD;
  const bf16_t* Kb = static_cast<const bf16_t*>(p.K) + (int64_t)b * p.k_sb + (int64_t)h * HD;
  const bf16_t* Vb = static_cast<const bf16_t*>(p.V) + (int64_t)b * p.v_sb + (int64_t)h * HD;
  const bf16_t* dOb = static_cast<const bf16_t*>(p.dO) + (int64_t)b * p.o_sb + (int64_t)h * HD;
  const uint64_t seed = asr_mix_seed(p.seed, p.seed_dev);
  const float c2 = p.scale * LOG2E;
  const float keep_prob = p.thr ? 1.f / p.inv_keep : 1.f, out_scale = p.thr ? p.scale * p.inv_keep : p.scale;
  const uint32_t thr_hi = p.thr << 16;            // field >= thr  <=>  (field << 16) >= thr_hi (thr <= 0xffff)
  const unsigned voK[2] = {tile_voff(p.k_st, tid, 0), tile_voff(p.k_st, tid, 1)};
  const unsigned voV[2] = {tile_voff(p.v_st, tid, 0), tile_voff(p.v_st, tid, 1)};
  FragOff fo;
  fo.init(lr, g);

  uint4 qf[NQ][2], dof[NQ][2];
  uint32_t rkey[NQ];
  float lse2[NQ], dlt[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int q = qw + qi * 16 + lr;
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
      qf[qi][ds] = load_row16(Qb, p.q_st, q, p.Tq, ds * 32 + g * 8);
      dof[qi][ds] = load_row16(dOb, p.o_st, q, p.Tq, ds * 32 + g * 8);
    }
    // first hash stage of the dropout mask as a running sum: (row key + key pair) * DROP_C1 is linear modulo 2^32, the lane part
    // (row, 2 g) is multiplied once here, a tile adds 32 * DROP_C1, the (half, fragment, pair) part is a literal
    rkey[qi] = (drop_row_key(seed, drop_row(p, b, h, q)) + 2u * (uint32_t)g) * DROP_C1;
    const int64_t si = ((int64_t)b * p.H + h) * p.Tq + (q < p.Tq ? q : p.Tq - 1);
    lse2[qi] = p.lse[si] * LOG2E;                 // +inf for fully masked rows: exp2(-inf) = 0
    // dS = P (keep / (1 - p) dP - delta) = 1 / (1 - p) * P (keep dP - (1 - p) delta): the rescale leaves the loop (it joins p.scale
    // in the epilogue), the mask becomes a plain select of dP
    dlt[qi] = p.delta[si] * keep_prob;
  }
  f32x4_t dq[NQ][4];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi)
#pragma unroll
    for (int df = 0; df < 4; ++df) dq[qi][df] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int kend = key_end(p, b);
  int kstop = kend;
  if (p.causal) kstop = min(kend, qb * FQW + FQW);
  const int ntile = (kstop + 63) >> 6;

  if (ntile > 0) {
    stage_tile_h(smem, Kb, p.k_st, 0, p.Tk, voK, tid, wave);
    stage_tile_h(smem + TILE, Vb, p.v_st, 0, p.Tk, voV, tid, wave);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < ntile; ++t) {
    const int k0 = t << 6;
    const unsigned char* sK = smem + (t & 1) * 2 * TILE;
    const unsigned char* sV = sK + TILE;
    const bool need_mask = (k0 + 64 > kend) || p.key_pad != nullptr || (p.causal && k0 + 63 > qw);
    // the tile is consumed in two halves of 32 keys (one macro step of the dQ contraction each): half the live accumulators
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      f32x4_t s[NQ][2], dp[NQ][2];
#pragma unroll
      for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
          s[qi][k2] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          dp[qi][k2] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int ds = 0; ds < 2; ++ds) {
          const uint4 ak = frag_rows_at(sK, fo.rows[ds], 2 * ms + k2);
          const uint4 av = frag_rows_at(sV, fo.rows[ds], 2 * ms + k2);
#pragma unroll
          for (int qi = 0; qi < NQ; ++qi) {
            mma(s[qi][k2], ak, qf[qi][ds]);
            mma(dp[qi][k2], av, dof[qi][ds]);
          }
        }
      }
      if (need_mask) mask_scores<2, NQ>(p, s, b, k0 + 32 * ms, g, qw + lr, kend);
      if (ms == 0) {
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < ntile) {
          unsigned char* nb = smem + ((t + 1) & 1) * 2 * TILE;
          stage_tile_h(nb, Kb, p.k_st, k0 + 64, p.Tk, voK, tid, wave);
          stage_tile_h(nb + TILE, Vb, p.v_st, k0 + 64, p.Tk, voV, tid, wave);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      uint4 pb[NQ];
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) {
        if (p.thr) {
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
              const uint32_t y = drop_pair_mix(rkey[qi] + (uint32_t)((2 * ms + k2) * 8 + pr) * DROP_C1);
              dp[qi][k2][2 * pr] = (y << 16) < thr_hi ? 0.f : dp[qi][k2][2 * pr];
              dp[qi][k2][2 * pr + 1] = y < thr_hi ? 0.f : dp[qi][k2][2 * pr + 1];
            }
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
          for (int r = 0; r < 4; r += 2) {      // two scores per packed instruction (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32)
            const asr_f32x2_t e = asr_f32x2_t{s[qi][k2][r], s[qi][k2][r + 1]} * c2 - lse2[qi];       // masked: s = -inf -> exp2 = 0
            const asr_f32x2_t pv = {__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])};
            const asr_f32x2_t ds = pv * (asr_f32x2_t{dp[qi][k2][r], dp[qi][k2][r + 1]} - dlt[qi]);
            s[qi][k2][r] = ds[0];
            s[qi][k2][r + 1] = ds[1];
          }
        pb[qi] = pack_p(s[qi], 0);
      }
#pragma unroll
      for (int df = 0; df < 4; ++df) {
        const uint4 kt = frag_cols_at(sK, fo.cols[df], ms);
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) mma(dq[qi][df], kt, pb[qi]);
      }
    }
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) rkey[qi] += 32u * DROP_C1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int q = qw + qi * 16 + lr;
    if (q >= p.Tq) continue;
    bf16_t* o = static_cast<bf16_t*>(p.dQ) + (int64_t)b * p.q_sb + (int64_t)q * p.q_st + (int64_t)h * HD;
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const f32x4_t v = dq[qi][df] * out_scale;
      *reinterpret_cast<uint2*>(o + df * 16 + g * 4) = make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
    }
  }
}

// ================================================================================================ backward: dK, dV
// wave = 32 keys (two B fragments, K / V rows in registers); 64-query Q / dO tiles double buffered in LDS with their
// lse / delta rows.   S = Q K^T, dP = dO V^T (A: Q / dO rows from LDS), P, dS as above, then
//   dV^T[d][key] += dO^T[d][q] Pd[q][key],  dK^T[d][key] += Q^T[d][q] dS[q][key]   (A: transposing reads of dO / Q tiles)
// NK: 16 NK keys per wave (NK = 1 for Tk <= 256, as in the other two kernels).
template <int NK>
__device__ __forceinline__ void attn_bwd_dkv_body(const AttnArgs& p, const int vid, unsigned char* smem, float (*s_stat)[2][64]) {
  constexpr int FKW = 64 * NK;                               // keys per workgroup;  s_stat: [buffer][lse*log2e | delta][q]
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nkb = (p.Tk + FKW - 1) / FKW;
  const int bh = vid / nkb, kb = vid - bh * nkb;
  const int b = bh / p.H, h = bh - b * p.H;
  const int kw = kb * FKW + wave * 16 * NK;                 // first key of this wave
  const bf16_t* Qb = static_cast<const bf16_t*>(p.Q) + (int64_t)b * p.q_sb + (int64_t)h * HD;
  const bf16_t* Kb = static_cast<const bf16_t*>(p.K) + (int64_t)b * p.k_sb + (int64_t)h * HD;
  const bf16_t* Vb = static_cast<const bf16_t*>(p.V) + (int64_t)b * p.v_sb + (int64_t)h * HD;
  const bf16_t* dOb = static_cast<const bf16_t*>(p.dO) + (int64_t)b * p.o_sb + (int64_t)h * HD;
  const uint64_t seed = asr_mix_seed(p.seed, p.seed_dev);
  const float c2 = p.scale * LOG2E;
  const int kend = key_end(p, b);
  const int64_t stat0 = ((int64_t)b * p.H + h) * p.Tq;
  const uint32_t field_sh = (uint32_t)(lr & 1) << 4;        // this lane's keys are kw + 16 ki + lr with kw a multiple of 16: key & 1 = lr & 1
  // (no hoisted DMA offsets / column-fragment addresses here, unlike the dQ half: this half has to fit 128 registers for the fourth wave per
  //  SIMD, and its loop is bound by the dependent chain of a wave, not by the vector instruction count -- profiles/r04_attention_bwd_ablation.txt)
  FragOff fo;
  fo.init(lr, g);

  uint4 kfr[NK][2], vfr[NK][2];
#pragma unroll
  for (int ki = 0; ki < NK; ++ki)
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
      kfr[ki][ds] = load_row16(Kb, p.k_st, kw + ki * 16 + lr, p.Tk, ds * 32 + g * 8);
      vfr[ki][ds] = load_row16(Vb, p.v_st, kw + ki * 16 + lr, p.Tk, ds * 32 + g * 8);
    }
  f32x4_t dk[NK][4], dv[NK][4];
#pragma unroll
  for (int ki = 0; ki < NK; ++ki)
#pragma unroll
    for (int df = 0; df < 4; ++df) { dk[ki][df] = f32x4_t{0.f, 0.f, 0.f, 0.f}; dv[ki][df] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
  // causal: query tiles that end before the first key of this workgroup never see it
  const int t0 = p.causal ? (kb * FKW) >> 6 : 0;
  const int ntile = (p.Tq + 63) >> 6;
  // first hash stage of the dropout mask, (row key + key pair) * DROP_C1, as a running sum (linear modulo 2^32; the row key is linear
  // in the row, + DROP_ROW_C per row): the lane part (row 4 g + 2 (lr & 1) of tile t0, this lane's key pair) is multiplied once, a
  // tile adds 64 rows, the (half, fragment) part and the second row of the lane are literals
  constexpr uint32_t DROP_ROW_C = 0x9E3779B1u;
  uint32_t ybase[NK];
#pragma unroll
  for (int ki = 0; ki < NK; ++ki)
    ybase[ki] = (drop_row_key(seed, drop_row(p, b, h, (t0 << 6) + g * 4 + 2 * (lr & 1))) + ((uint32_t)(kw + ki * 16 + lr) >> 1)) * DROP_C1;

  // lse / delta of query tile t (64 floats each).  Full tiles: part of the tile's DMA request (wave 0 fetches the lse row, wave 1
  // the delta row, 4 bytes per lane) -- as ordinary loads stored to LDS by the threads, every tile exposed a global-memory round
  // trip: the value has to be CONSUMED before the hand-issued DMA of that tile goes out (vmcnt retires in order: waiting for it
  // later would wait for the DMA as well), i.e. half a tile after it was requested.  The ragged last tile (rows past Tq must read
  // lse = +inf: P = exp2(-inf) = 0) and the first tile keep the load / store path.
  auto load_stat = [&](int t) __attribute__((always_inline)) -> float {
    const int ql = tid & 63, qq = (t << 6) + ql;
    if (tid < 64) return qq < p.Tq ? p.lse[stat0 + qq] : INFINITY;
    return (tid < 128 && qq < p.Tq) ? p.delta[stat0 + qq] : 0.f;
  };
  auto dma_stats = [&](int t, int buf) __attribute__((always_inline)) {
    if (wave < 2) {
      const float* src = (wave == 0 ? p.lse : p.delta) + stat0 + (t << 6) + lane;
      lds_dma4((unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)&s_stat[buf][wave][0], src);
    }
  };
  auto stage_stats = [&](int t, int buf) __attribute__((always_inline)) {
    const float v = load_stat(t);
    if (tid < 128) s_stat[buf][tid >> 6][tid & 63] = v;
  };
  if (t0 < ntile) {
    stage_stats(t0, t0 & 1);
    stage_tile(smem, Qb, p.q_st, t0 << 6, p.Tq, tid, wave);
    stage_tile(smem + TILE, dOb, p.o_st, t0 << 6, p.Tq, tid, wave);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = t0; t < ntile; ++t) {
    const int q0 = t << 6;
    const unsigned char* sQ = smem + ((t - t0) & 1) * 2 * TILE;
    const unsigned char* sdO = sQ + TILE;
    const float* st_lse = s_stat[t & 1][0];
    const float* st_dlt = s_stat[t & 1][1];
    const bool need_mask = p.key_pad != nullptr || (p.causal && kw + 16 * NK - 1 > q0) || (kw + 16 * NK > kend);
    const bool next_ragged = q0 + 128 > p.Tq;
    const float next_stat = (t + 1 < ntile && next_ragged) ? load_stat(t + 1) : 0.f;
    // the query tile is consumed in two halves of 32 queries (one macro step of the dV / dK contractions each)
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      f32x4_t s[NK][2], dp[NK][2];
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2) {
#pragma unroll
        for (int ki = 0; ki < NK; ++ki) {
          s[ki][q2] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          dp[ki][q2] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int ds = 0; ds < 2; ++ds) {
          const uint4 aq = frag_rows_at(sQ, fo.rows[ds], 2 * ms + q2);
          const uint4 ao = frag_rows_at(sdO, fo.rows[ds], 2 * ms + q2);
#pragma unroll
          for (int ki = 0; ki < NK; ++ki) {
            mma(s[ki][q2], aq, kfr[ki][ds]);
            mma(dp[ki][q2], ao, vfr[ki][ds]);
          }
        }
      }
      // per-row statistics of the 8 queries this lane sees in this half: q = q0 + 32 ms + 16 q2 + 4 g + r
      f32x4_t lse2[2], dlt[2];
#pragma unroll
      for (int q2 = 0; q2 < 2; ++q2) {
        lse2[q2] = *reinterpret_cast<const f32x4_t*>(st_lse + (2 * ms + q2) * 16 + g * 4) * LOG2E;
        dlt[q2] = *reinterpret_cast<const f32x4_t*>(st_dlt + (2 * ms + q2) * 16 + g * 4);
      }
      if (ms == 0) {
        __builtin_amdgcn_sched_barrier(0);
        if (t + 1 < ntile) {
          unsigned char* nb = smem + ((t + 1 - t0) & 1) * 2 * TILE;
          if (!next_ragged) dma_stats(t + 1, (t + 1) & 1);
          else if (tid < 128) s_stat[(t + 1) & 1][tid >> 6][tid & 63] = next_stat;
          stage_tile(nb, Qb, p.q_st, q0 + 64, p.Tq, tid, wave);
          stage_tile(nb + TILE, dOb, p.o_st, q0 + 64, p.Tq, tid, wave);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      uint4 pa[NK], pd[NK];
#pragma unroll
      for (int ki = 0; ki < NK; ++ki) {
        const int key = kw + ki * 16 + lr;
        if (need_mask) {
          uint32_t mbits = 0u;                      // mask bytes loaded up front, unconditionally (see mask_scores)
          if (p.key_pad) {
            const int col = (int)((int64_t)b * p.m_sb) + (key < p.Tk ? key : p.Tk - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const int qq = q0 + (2 * ms + (i >> 2)) * 16 + g * 4 + (i & 3);
              mbits |= (uint32_t)(__builtin_amdgcn_raw_buffer_load_b8(mask_rsrc(p), col + (qq < p.Tq ? qq : p.Tq - 1) * (int)p.m_sq, 0, 0) != 0) << i;
            }
          }
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int qq = q0 + (2 * ms + q2) * 16 + g * 4 + r;
              const bool dead = (key >= kend) | (p.causal != 0 & key > qq) | (((mbits >> (q2 * 4 + r)) & 1u) != 0u);
              s[ki][q2][r] = dead ? -INFINITY : s[ki][q2][r];
            }
        }
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
          // Dropout mask of this lane's 4 consecutive query rows at ONE key.  The hash word of (row, key pair) holds the fields of keys
          // 2j and 2j + 1, i.e. of this lane and of lane ^ 1: the even lane of a pair hashes rows 0 and 1, the odd lane rows 2 and 3,
          // and both read all four words through quad permutes -- two hashes and four v_mov_dpp per lane instead of four hashes
          // (the row key is linear in the row: + 0x9E3779B1 per row, attention.h).
          uint32_t yw[4] = {0u, 0u, 0u, 0u};
          if (p.thr) {
            const uint32_t ya = drop_pair_mix(ybase[ki] + (uint32_t)((2 * ms + q2) * 16) * DROP_ROW_C * DROP_C1);
            const uint32_t yb = drop_pair_mix(ybase[ki] + (uint32_t)((2 * ms + q2) * 16 + 1) * DROP_ROW_C * DROP_C1);
            yw[0] = (uint32_t)__builtin_amdgcn_mov_dpp((int)ya, 0xA0, 0xf, 0xf, true);        // quad_perm [0,0,2,2]: the pair's even lane
            yw[1] = (uint32_t)__builtin_amdgcn_mov_dpp((int)yb, 0xA0, 0xf, 0xf, true);
            yw[2] = (uint32_t)__builtin_amdgcn_mov_dpp((int)ya, 0xF5, 0xf, 0xf, true);        // quad_perm [1,1,3,3]: the pair's odd lane
            yw[3] = (uint32_t)__builtin_amdgcn_mov_dpp((int)yb, 0xF5, 0xf, 0xf, true);
          }
#pragma unroll
          for (int r = 0; r < 4; r += 2) {      // two scores per packed instruction
            const asr_f32x2_t e = asr_f32x2_t{s[ki][q2][r], s[ki][q2][r + 1]} * c2 - asr_f32x2_t{lse2[q2][r], lse2[q2][r + 1]};
            const asr_f32x2_t pv = {__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])};
            // field of key & 1 (v_bfe_u32).  No test of p.thr here: with dropout off thr = 0 never exceeds a field and inv_keep = 1
            const asr_f32x2_t keepf = {((yw[r] >> field_sh) & 0xffffu) < p.thr ? 0.f : p.inv_keep,
                                       ((yw[r + 1] >> field_sh) & 0xffffu) < p.thr ? 0.f : p.inv_keep};
            const asr_f32x2_t pd = pv * keepf;                                                     // dropped / rescaled probabilities (for dV)
            const asr_f32x2_t ds = pv * (asr_f32x2_t{dp[ki][q2][r], dp[ki][q2][r + 1]} * keepf - asr_f32x2_t{dlt[q2][r], dlt[q2][r + 1]});   // dS (for dK)
            s[ki][q2][r] = pd[0];
            s[ki][q2][r + 1] = pd[1];
            dp[ki][q2][r] = ds[0];
            dp[ki][q2][r + 1] = ds[1];
          }
        }
        pa[ki] = pack_p(s[ki], 0);
        pd[ki] = pack_p(dp[ki], 0);
      }
#pragma unroll
      for (int df = 0; df < 4; ++df) {
        const uint4 aot = frag_cols(sdO, df * 16, ms, lr, g);        // (addresses computed per read: this half lives at 128 registers)
        const uint4 aqt = frag_cols(sQ, df * 16, ms, lr, g);
#pragma unroll
        for (int ki = 0; ki < NK; ++ki) {
          mma(dv[ki][df], aot, pa[ki]);
          mma(dk[ki][df], aqt, pd[ki]);
        }
      }
    }
#pragma unroll
    for (int ki = 0; ki < NK; ++ki) ybase[ki] += 64u * DROP_ROW_C * DROP_C1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#pragma unroll
  for (int ki = 0; ki < NK; ++ki) {
    const int key = kw + ki * 16 + lr;
    if (key >= p.Tk) continue;
    bf16_t* ok = static_cast<bf16_t*>(p.dK) + (int64_t)b * p.k_sb + (int64_t)key * p.k_st + (int64_t)h * HD;
    bf16_t* ov = static_cast<bf16_t*>(p.dV) + (int64_t)b * p.v_sb + (int64_t)key * p.v_st + (int64_t)h * HD;
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const f32x4_t a = dk[ki][df] * p.scale, c = dv[ki][df];
      *reinterpret_cast<uint2*>(ok + df * 16 + g * 4) = make_uint2(pack_bf16(a[0], a[1]), pack_bf16(a[2], a[3]));
      *reinterpret_cast<uint2*>(ov + df * 16 + g * 4) = make_uint2(pack_bf16(c[0], c[1]), pack_bf16(c[2], c[3]));
    }
  }
}

template <int NQ>
__global__ __launch_bounds__(256) void attn_bwd_dq_bf16_d64_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * TILE];
  attn_bwd_dq_body<NQ>(p, xcd_linear_id(), smem);
}
template <int NK>
__global__ __launch_bounds__(256, NK == 1 ? 4 : 2) void attn_bwd_dkv_bf16_d64_kernel(AttnArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * TILE];
  __shared__ float s_stat[2][2][64];
  attn_bwd_dkv_body<NK>(p, xcd_linear_id(), smem, s_stat);
}
// Both halves of the backward in ONE launch: the first n_dq workgroups are dQ workgroups, the others dK / dV workgroups (they are
// independent; both only need delta).  Two launches on two streams cost a fork and a join -- 0.16 ms of idle time per step over the
// 12 attention blocks of the benchmark model -- for the same overlap.
template <int N>
__global__ __launch_bounds__(256, N == 1 ? 4 : 2) void attn_bwd_both_bf16_d64_kernel(AttnArgs p, int n_dq) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * TILE];
  __shared__ float s_stat[2][2][64];
  const int bid = (int)blockIdx.x;
  if (bid < n_dq) attn_bwd_dq_body<N>(p, asr_xcd_linear(bid, n_dq), smem);
  else attn_bwd_dkv_body<N>(p, asr_xcd_linear(bid - n_dq, (int)gridDim.x - n_dq), smem, s_stat);
}

__global__ __launch_bounds__(256) void attn_delta_bf16_d64_kernel(AttnArgs p) {
  // delta[b,h,q] = sum_d dO * O : one 8-lane group per row (8 x 16 B = one 128-byte head row)
  const int64_t idx = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int64_t total = (int64_t)p.B * p.H * p.Tq;
  const int sub = threadIdx.x & 7;
  float acc = 0.f;
  if (idx < total) {
    const int q = (int)(idx % p.Tq);
    const int h = (int)((idx / p.Tq) % p.H);
    const int b = (int)(idx / ((int64_t)p.Tq * p.H));
    const int64_t off = (int64_t)b * p.o_sb + (int64_t)q * p.o_st + (int64_t)h * HD + sub * 8;
    Chunk<bf16_t> o, d;
    d.v = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(p.dO) + off);
    if (p.O32) {       // un-rounded forward output: the rounding error of a bf16 O does not cancel against dP (see asr_hip.h)
      const f32x4_t o0 = *reinterpret_cast<const f32x4_t*>(p.O32 + off), o1 = *reinterpret_cast<const f32x4_t*>(p.O32 + off + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += o0[j] * bf16_to_f32(d.e[j]) + o1[j] * bf16_to_f32(d.e[4 + j]);
    } else {
      o.v = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(p.O) + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += bf16_to_f32(o.e[j]) * bf16_to_f32(d.e[j]);
    }
  }
  acc += __shfl_xor(acc, 4, 64);
  acc += __shfl_xor(acc, 2, 64);
  acc += __shfl_xor(acc, 1, 64);
  if (idx < total && sub == 0) p.delta[idx] = acc;
}

}  // namespace

int attn_d64_delta(const AttnArgs& p, hipStream_t s) {
  const int64_t rows = (int64_t)p.B * p.H * p.Tq;
  return asr_launch<attn_delta_bf16_d64_kernel>(dim3((unsigned)ceil_div64(rows, 32)), dim3(256), 0, s, p);
}
// 64-row blocks at every length (the 128-row instantiations of these three kernels sat behind a length threshold whose setting was "never")
int attn_d64_bwd_both(const AttnArgs& p, hipStream_t s) {
  const int n_dq = ((p.Tq + 63) / 64) * p.B * p.H, n_dkv = ((p.Tk + 63) / 64) * p.B * p.H;
  return asr_launch<attn_bwd_both_bf16_d64_kernel<1>>(dim3((unsigned)(n_dq + n_dkv)), dim3(256), 0, s, p, n_dq);
}
int attn_d64_bwd_dq(const AttnArgs& p, hipStream_t s) {
  return asr_launch<attn_bwd_dq_bf16_d64_kernel<1>>(dim3((unsigned)(((p.Tq + 63) / 64) * p.B * p.H)), dim3(256), 0, s, p);
}
int attn_d64_bwd_dkv(const AttnArgs& p, hipStream_t s) {
  return asr_launch<attn_bwd_dkv_bf16_d64_kernel<1>>(dim3((unsigned)(((p.Tk + 63) / 64) * p.B * p.H)), dim3(256), 0, s, p);
}

}  // namespace asr_attn
