// Attention forward specialised for the reference configurations: bf16 storage, head dim 64, 16-byte aligned rows
// (models/common_layers.py:211-225 at dim_key = dim_value = 64).  Same algorithm and numerics as attention_generic.hip
// (flash style, swapped contractions S^T = K Q^T, O^T = V^T P^T, fp32 softmax statistics); what changes is the data path:
//   * K / V tiles (64 keys x 64 dims, natural [key][d] layout) go HBM -> LDS with the LDS-DMA (global_load_lds, 16 B per
//     lane, XOR-swizzled 16-byte chunks), double buffered: the next tile is in flight while this one is consumed;
//   * the V^T operand of O^T += V^T P^T is read from the NATURAL V tile with ds_read_b64_tr_b16 (no transposed copy);
//   * a wave owns 32 queries (two B fragments), so every LDS operand read feeds two MFMAs;
//   * softmax in base 2 (v_exp_f32 directly, scale*log2(e) folded into one FMA), hardware bf16 packing, pair-wise dropout
//     hash, masks evaluated only on tiles that touch a boundary;
//   * workgroups that share K/V (the query blocks of one (b,h)) are placed on the same XCD.
// The backward of the same data path: attention_d64_bwd.hip (two halves) and attention_d64_bwd_fused.hip (one pass, short keys); the
// long-sequence forward: attention_pp.hip.  Which call gets which: attention.hip.
#include "attention_d64.h"

namespace asr_attn {
namespace {

// ================================================================================================ forward
// workgroup = 4 waves x 16 NQ queries; grid = ceil(Tq / (64 NQ)) * B * H (1-D, XCD-aware).  NQ = 2 (32 queries per wave) for long
// sequences; NQ = 1 for short ones (Tq <= 256, every attention of the benchmark model at T' = 200): measured at (32, 8, 200, 200)
// the tile loop costs 2.1 us per 64-key tile with two waves per SIMD -- one wave's S -> softmax -> P V chain cannot overlap its own
// phases -- against 2.7 us for everything else in the launch; half the queries per wave doubles the waves per SIMD.

template <int NQ, bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_bf16_d64_kernel(AttnArgs p) {
  constexpr int FQW = 64 * NQ;                               // queries per workgroup
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * TILE];      // [buffer][K | V]
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nqb = (p.Tq + FQW - 1) / FQW;
  const int vid = xcd_linear_id();
  const int bh = vid / nqb, qb = vid - bh * nqb;
  const int b = bh / p.H, h = bh - b * p.H;
  const int qw = qb * FQW + wave * 16 * NQ;                 // first query of this wave
  const bf16_t* Qb = static_cast<const bf16_t*>(p.Q) + (int64_t)b * p.q_sb + (int64_t)h * HD;
  const bf16_t* Kb = static_cast<const bf16_t*>(p.K) + (int64_t)b * p.k_sb + (int64_t)h * HD;
  const bf16_t* Vb = static_cast<const bf16_t*>(p.V) + (int64_t)b * p.v_sb + (int64_t)h * HD;
  const uint64_t seed = asr_mix_seed(p.seed, p.seed_dev);
  const float c2 = p.scale * LOG2E;
  FragOff fo;
  fo.init(lr, g);

  uint4 qf[NQ][2];
  uint32_t rkey[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) qf[qi][ds] = load_row16(Qb, p.q_st, qw + qi * 16 + lr, p.Tq, ds * 32 + g * 8);
    rkey[qi] = drop_row_key(seed, drop_row(p, b, h, qw + qi * 16 + lr));
  }
  f32x4_t o[NQ][4];
  float m[NQ], l[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    m[qi] = -INFINITY;
    l[qi] = 0.f;
#pragma unroll
    for (int df = 0; df < 4; ++df) o[qi][df] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const int kend = key_end(p, b);
  int kstop = kend;
  if (p.causal) kstop = min(kend, qb * FQW + FQW);
  const int ntile = (kstop + 63) >> 6;

  const unsigned voK[2] = {tile_voff(p.k_st, tid, 0), tile_voff(p.k_st, tid, 1)};
  const unsigned voV[2] = {tile_voff(p.v_st, tid, 0), tile_voff(p.v_st, tid, 1)};
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
    // ---- S^T[key][q] = K . Q^T
    f32x4_t s[NQ][4];
#pragma unroll
    for (int kf = 0; kf < 4; ++kf) {
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) s[qi][kf] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < 2; ++ds) {
        const uint4 a = frag_rows_at(sK, fo.rows[ds], kf);
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) mma(s[qi][kf], a, qf[qi][ds]);
      }
    }
    // ---- masks only where a boundary crosses this tile (wave-uniform test)
    const bool need_mask = (k0 + 64 > kend) || p.key_pad != nullptr || (p.causal && k0 + 63 > qw);
    if (need_mask) mask_scores<4, NQ>(p, s, b, k0, g, qw + lr, kend);
    // next tile: HBM -> LDS in flight under the softmax and the second contraction.  Issued AFTER the mask bytes were
    // consumed: ordinary loads and LDS-DMA loads share vmcnt, and waiting for the former with the latter in flight
    // was observed to return stale mask bytes.
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < ntile) {
      unsigned char* nb = smem + ((t + 1) & 1) * 2 * TILE;
      stage_tile_h(nb, Kb, p.k_st, k0 + 64, p.Tk, voK, tid, wave);
      stage_tile_h(nb + TILE, Vb, p.v_st, k0 + 64, p.Tk, voV, tid, wave);
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- online softmax (base 2), dropout, pack P^T as the B operand
    uint4 pb[NQ][2];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      float mx = -INFINITY;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[qi][kf][r]);
      mx = group_max4(mx);
      const float m_new = fmaxf(m[qi], mx);
      const float m_safe = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f((m[qi] - m_safe) * c2);
      const float mc = m_safe * c2;
      float psum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __builtin_amdgcn_exp2f(s[qi][kf][r] * c2 - mc);
          psum += pv;
          s[qi][kf][r] = pv;
        }
      if (DROP) {                    // compile time: a run-time `if (p.thr)` here cost 8 register moves per query fragment even at p = 0
#pragma unroll
        for (int kf = 0; kf < 4; ++kf)
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            const uint32_t y = drop_pair_bits(rkey[qi], (uint32_t)(k0 + kf * 16 + g * 4 + pr * 2) >> 1);
            if ((y & 0xffffu) < p.thr) s[qi][kf][2 * pr] = 0.f;
            if ((y >> 16) < p.thr) s[qi][kf][2 * pr + 1] = 0.f;
          }
      }
      psum = group_sum4(psum);
      l[qi] = l[qi] * alpha + psum;
      m[qi] = m_new;
#pragma unroll
      for (int df = 0; df < 4; ++df) o[qi][df] *= alpha;
      pb[qi][0] = pack_p(s[qi], 0);
      pb[qi][1] = pack_p(s[qi], 1);
    }
    // ---- O^T[d][q] += V^T . P^T
#pragma unroll
    for (int ms = 0; ms < 2; ++ms)
#pragma unroll
      for (int df = 0; df < 4; ++df) {
        const uint4 vt = frag_cols_at(sV, fo.cols[df], ms);
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) mma(o[qi][df], vt, pb[qi][ms]);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const int q = qw + qi * 16 + lr;
    if (q >= p.Tq) continue;
    const float inv_l = l[qi] > 0.f ? p.inv_keep / l[qi] : 0.f;      // the dropout rescale is a constant: applied once here
    if (g == 0) p.lse[((int64_t)b * p.H + h) * p.Tq + q] = l[qi] > 0.f ? m[qi] * p.scale + logf(l[qi]) : INFINITY;
    bf16_t* Ob = static_cast<bf16_t*>(p.Out) + (int64_t)b * p.o_sb + (int64_t)q * p.o_st + (int64_t)h * HD;
#pragma unroll
    for (int df = 0; df < 4; ++df) {
      const f32x4_t v = o[qi][df] * inv_l;
      *reinterpret_cast<uint2*>(Ob + df * 16 + g * 4) = make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
      if (p.Out32) *reinterpret_cast<f32x4_t*>(p.Out32 + (int64_t)b * p.o_sb + (int64_t)q * p.o_st + (int64_t)h * HD + df * 16 + g * 4) = v;
    }
  }
}

// (A software-pipelined form of the forward -- S(t+1) issued before the softmax of S(t), interleaved instruction by instruction -- was
// measured slower at every shape in round 2, profiles/r02_ab_attn_pipe.txt, and removed in round 3.)

}  // namespace

// NQ = nq (1 or 2): 64 nq queries per workgroup
int attn_d64_fwd(const AttnArgs& p, int nq, hipStream_t s) {
  const dim3 grid((unsigned)(((p.Tq + 64 * nq - 1) / (64 * nq)) * p.B * p.H));
  if (nq == 1) {
    if (p.thr) return asr_launch<attn_fwd_bf16_d64_kernel<1, true>>(grid, dim3(256), 0, s, p);
    return asr_launch<attn_fwd_bf16_d64_kernel<1, false>>(grid, dim3(256), 0, s, p);
  }
  if (p.thr) return asr_launch<attn_fwd_bf16_d64_kernel<2, true>>(grid, dim3(256), 0, s, p);
  return asr_launch<attn_fwd_bf16_d64_kernel<2, false>>(grid, dim3(256), 0, s, p);
}

}  // namespace asr_attn
