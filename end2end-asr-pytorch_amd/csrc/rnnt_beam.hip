// Transducer (RNN-T) beam search: the n best label sequences of the transducer head, one fused search kernel per utterance (DESIGN.md
// section 7).  The predictor is stateless -- p = sum_k rnnt_embed.k[y_{-k}], C <= 2 table rows -- so a hypothesis carries no recurrent
// state, only its last labels, and a search step needs e[b,t], two table rows, tanh and the J x V output projection over at most 16
// hypothesis rows: the M of one v_mfma_f32_16x16x32_bf16.  tests/rnnt_beam_reference.py restates the definition in float64.
//
// Blank = `blank` (PAD).  A hypothesis is a label sequence y with score = the log-probability summed over all alignments found for it so
// far; its context is its last C labels, `sos` where it has fewer.  logp(t, h) = the fp32 log-softmax row of
// w_out tanh(e[b,t] + p(ctx(h))) + b_out.  W: beam, K: label candidates per row, S: max_symbols.  Per utterance b:
//
//   A = {(empty, 0)}; for each frame t < T_b:
//     C_0 = A, D = {}; for s = 0 .. S:
//       blank step   every h of C_s: (h.y, h.score + logp(t,h)[blank]) joins D; a sequence D already holds is merged by logaddexp
//       label step   (s < S) candidates (h.y + k, h.score + logp(t,h)[k]) for the K largest non-blank entries k of each row (greater logit
//                    first, lower label first among equals); C_{s+1} = the W best: score descending, then the parent's place in C_s, then
//                    the label id, both ascending.  Candidates of distinct parents are distinct sequences: nothing merges here
//     A = the W best of D: score descending, then order of first insertion
//   result: the nbest <= W best of A, best first; T_b = 0: the empty sequence with score 0; missing entries: length -1, score -inf
//
// No early exit and no expansion pruning: every frame runs its S + 1 steps.  With nothing pruned and S >= len(y), score(y) is the
// training likelihood of y, -nll of csrc/rnnt.hip.
//
// One workgroup of 8 waves per utterance, no atomics: the result is a function of the inputs alone.  A step is five phases between
// barriers in uniform control flow (every loop bound comes from the clamped frame length, S, W and K):
//   1  z rows -> LDS in the compute dtype: p = the table rows added in table order and rounded once, z = tanhf(e + p) rounded once (the
//      bits of asr_rnnt_joint_fwd); rows beyond the live count are zero.  Frames >= T_b of e are never read, nor a table row no
//      hypothesis has as context
//   2  the projection.  bf16 MFMA arm (bf16, J % 32 == 0, J <= 256): a wave holds the 16-row z fragment for all of J in registers (J/32 x 4
//      VGPRs) and the waves stride over the 16-column tiles of V; w_out (V,J) row-major IS the B operand with k contiguous, one 16-byte
//      global load per lane and k-step, no LDS and no barrier in the k loop; bias in the epilogue, the last tile of a V that is no
//      multiple of 16 masked.  Plain arm (everything else): one fp32 fmaf chain in k order per logit.  Both leave the fp32 logits rows in
//      the utterance's slice of the workspace (16 rows of V = 4364 are 279 KB: more than LDS, and L2 resident)
//   3  a wave per live row (rows wave, wave + 8): lse_row (csrc/lse.h), the blank's log-probability, and the K candidates in the order
//      of csrc/topk.h from one more pass over the row (rb_top_scan below; the last step of a frame needs no candidates)
//   4  the blank step (wave 0: a lane per row looks its key up in D) and the candidates' scores
//   5  every candidate counts the candidates that beat it; the W best become C_{s+1}
// Scores are fp64 (as the lattice of csrc/rnnt.hip, and for its reason); rows are fp32.  Sequences are trie nodes (parent, label) in the
// workspace -- the survivor of frame t, step s with rank r owns node 1 + (t S + s) W + r -- and are matched by the 64-bit key of
// csrc/beam_key.h.  Bookkeeping (C_s double buffered, D, the selection buffers) lives in LDS; D holds at most W (S + 1) <= 1024 entries.
// All indices into e, the tables, w_out and the workspace are 64 bit.
//
// The fused arms (asr_rnnt_beam_search_lm / _ctx, template <.., LM, CTX>): a label n-gram LM and a phrase list have their say while the
// beam is pruned.  q(h, c) is the query of csrc/ngram.h, step(s, c) -> (next, delta) and hold(s) the automaton of csrc/context.h, bonus
// the fp32 expression of csrc/beam_bonus.h; tests/rnnt_beam_fused_reference.py restates the arms in float64.  Added to the definition:
//   state        every entry of C_s, D and A also carries the BeamExt of csrc/beam_fuse.h (lm, len, nctx = its ctx, cst, cnt; root and
//                extension are defined there, once for both searches).  nctx holds order - 1 <= 3 labels, more than the predictor's l1 / l2
//   key          f(h) = score(h) + (double)bonus(h), bonus = alpha lm + beta (float)len, then + gamma (float)cnt; without an LM lm = 0.f
//   label step   the K candidates of a row stay the K best non-blank entries by logit (the acoustic model proposes); candidate (r, k)
//                gets score_r + logp and row r's state extended by its label; C_{s+1} = the W best by f descending, then the parent's
//                place, then the label id
//   blank step   the entry joins D with its whole state; a sequence D already holds merges score by rnnt_lae and keeps the rest, which
//                is equal by construction
//   frame end    A = the W best of D by f descending, then the order of first insertion
//   result       the entries of A ordered again by score + bonus(lm + q(nctx, eos), len, cnt - hold(cst)) (no end term for eos = -1),
//                the place in A first among equals; scores stays the acoustic log-probability, lm is written with the end term, credit
//                = cnt - hold(cst): an unfinished phrase earns nothing; missing entries: lm 0, credit 0.  T_b = 0: the empty sequence,
//                score 0, lm = q(ctx(bos), eos), credit 0
// With alpha = beta = gamma = 0 every key is the score: ids, lengths and scores are the plain arms' bits.  The lookups sit in phase 4, one
// candidate per thread (n K <= 256); the candidate's new state stays in that thread's registers until phase 5 places it.  The per-entry
// state (24 bytes) of D's 1024 entries, D's rank keys and C_s live in dynamic LDS behind the z rows (RB_FUSE_BYTES = 33 728), so the
// fused arms' J limit is lower (fp32 1384, bf16 2776) and the plain arms' static LDS and limit are what they were.  <.., false, false>
// instantiates none of this: its frame loop is the same instruction stream as before.
#include "common.h"
#include "lse.h"             // Lse, lse_row (no multiply-add contraction from here on)
#include "rnnt_common.h"     // rnnt_lae, clampi
#include "topk.h"            // MaxIdx, better, wave_best
#include "beam_key.h"        // beam_key, BEAM_ROOT_KEY_LO / _HI
#include "beam_fuse.h"       // BeamExt and its lookups, the table checks (shared with csrc/ctc_beam.hip; behind lse.h)
#include <type_traits>

namespace {

constexpr int RB_MAX = 16;                     // W and K; the rows of one MFMA tile
constexpr int RB_WAVES = 8;                    // 512 threads (at 1024 the MFMA arm's fragments spilled: 128 VGPRs a lane)
constexpr int RB_THREADS = 64 * RB_WAVES;
constexpr int RB_DMAX = 1024;                  // entries of D: W (S + 1) must fit (28 KB of LDS)
constexpr int RB_NK_MAX = 8;                   // MFMA arm: J <= 256, the z fragment is 32 VGPRs
constexpr size_t RB_LDS_DYN_MAX = 120 * 1024;  // the z rows beside ~34 KB of static LDS

struct RbArgs {
  const void *e, *t0, *t1, *w;
  const float* bias;
  const int32_t* frames;
  int T, J, V, W, K, S, nbest, blank, sos, ldv;
  float* ws;
  int64_t ws_stride;
  int32_t *ids, *lengths;
  float* scores;
};

// What the fused arms add to the plain search's arguments (the plain arms take the empty RbNoFuse).  Phrases without an LM: ng, bos, eos
// and alpha are not looked at, lm is 0 and beta still counts.  LM without phrases: cx, gamma and credit are not looked at.
struct RbFuse {
  NgramTable ng;
  CtxTable cx;
  int bos, eos;             // eos -1: no end term
  float alpha, beta, gamma;
  float* lm;                // (B,nbest)
  int32_t* credit;          // (B,nbest)
};
struct RbNoFuse {};

// The fused arms' per-entry state (lm, len, nctx, cst, cnt: 24 bytes) lives in dynamic LDS behind the z rows: D's 1024 entries and their
// rank keys, C_s double buffered, and the final order.  The plain arms ask for none of it.
constexpr size_t RB_FUSE_BYTES = (size_t)RB_DMAX * (8 + 8 + 4 * 4) + 2 * RB_MAX * (8 + 4 * 4) + RB_MAX * 3 * 4;

inline int rb_ldv(int V) { return (V + 3) & ~3; }                                       // rows of the logits slice start on 16 bytes
inline int64_t rb_nodes(int T, int S, int W) { return ((int64_t)T * S * W + 2) & ~(int64_t)1; }      // 1 + T S W, rounded up to even
inline int64_t rb_stride(int T, int V, int W, int S) { return (int64_t)RB_MAX * rb_ldv(V) + 2 * rb_nodes(T, S, W); }

// logits rows 0 .. n-1 of the 16 x V tile row [z (LDS, 16 rows of zld) x w^T] + bias; wave `wave` takes tiles wave, wave + 8, ...  One tile's
// NK fragment loads are in flight at a time.  Asking for four tiles' at once (32 loads per lane, 254 VGPRs) was measured and did not move
// the step (profiles/rnnt_beam_four_tiles.txt against profiles/rnnt_beam.txt), so the simple loop stays.
template <int NK>
__device__ __forceinline__ void rb_proj_mfma(const bf16_t* zl, int zld, const bf16_t* __restrict__ w, const float* __restrict__ bias, int J,
                                             int V, int n, float* lg, int ldv, int wave, int lane) {
  const int fr = lane & 15, g = lane >> 4;
  uint4 a[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) a[kk] = *reinterpret_cast<const uint4*>(zl + fr * zld + 32 * kk + 8 * g);
  const int ntiles = (V + 15) >> 4;
  for (int tile = wave; tile < ntiles; tile += RB_WAVES) {
    const int col = tile * 16 + fr;
    const int colc = col < V ? col : V - 1;                    // the masked columns of the last tile read the last row again
    const bf16_t* wr = w + (int64_t)colc * J + 8 * g;
    uint4 bq[NK];
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) bq[kk] = *reinterpret_cast<const uint4*>(wr + 32 * kk);
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) mma16<bf16_t>(acc, a[kk], bq[kk]);
    if (col < V) {
      const float bv = bias[col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 4 * g + i;
        if (row < n) lg[(int64_t)row * ldv + col] = acc[i] + bv;
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ void rb_proj_plain(const T* zl, int zld, const T* __restrict__ w, const float* __restrict__ bias, int J, int V, int n,
                                              float* lg, int ldv, int tid) {
  constexpr int EPC = DT<T>::EPC;
  const int JC = J / EPC;
  for (int idx = tid; idx < n * V; idx += RB_THREADS) {
    const int r = idx / V, v = idx - r * V;
    const T* wr = w + (int64_t)v * J;
    const T* zr = zl + r * zld;
    float acc = 0.f;
    for (int c = 0; c < JC; ++c) {
      Chunk<T> cw, cz;
      cw.v = *reinterpret_cast<const uint4*>(wr + c * EPC);
      cz.v = *reinterpret_cast<const uint4*>(zr + c * EPC);
#pragma unroll
      for (int i = 0; i < EPC; ++i) acc = fmaf(DT<T>::from(cz.e[i]), DT<T>::from(cw.e[i]), acc);
    }
    lg[(int64_t)r * ldv + v] = acc + bias[v];
  }
}

// The K best non-blank entries of a row, in the order of csrc/topk.h, from ONE pass over the row: every lane keeps the RB_TOP best of ITS
// columns, sorted, and the K rounds are a wave arg-max over the lanes' heads; the winner pops its head.  A lane whose list runs empty
// while it still owns entries behind it scans its columns again for the next RB_TOP (rare: five of the K best in one lane's 1/64 of
// the row), so the selection is exact.  (K arg-max passes over the row, each a chain of L2 latencies, were the first form and most of a step.)
constexpr int RB_TOP = 4;
constexpr int RB_NONE = 0x7fffffff;
struct RbTop {
  float v[RB_TOP];
  int i[RB_TOP];
  int more;                // entries of the lane that fell off the list
};

__device__ __forceinline__ void rb_top_push(RbTop& t, float x, int v) {      // (x, v) behind everything pushed before it among equals
  bool carry = false;
#pragma unroll
  for (int j = 0; j < RB_TOP; ++j) {
    const bool sw = carry || x > t.v[j] || t.i[j] == RB_NONE;
    const float ov = t.v[j];
    const int oi = t.i[j];
    t.v[j] = sw ? x : ov;
    t.i[j] = sw ? v : oi;
    x = sw ? ov : x;
    v = sw ? oi : v;
    carry = sw;
  }
  t.more += v != RB_NONE;
}

// the RB_TOP best of the lane's columns behind (pv, pi); lane `lane` owns the columns lse_row gives it, met in ascending order
__device__ __forceinline__ void rb_top_scan(RbTop& t, const float* l, int V, int lane, int blank, float pv, int pi) {
#pragma unroll
  for (int j = 0; j < RB_TOP; ++j) { t.v[j] = -INFINITY; t.i[j] = RB_NONE; }
  t.more = 0;
  auto take = [&](float x, int v) {
    if (v != blank && (x < pv || (x == pv && v > pi))) rb_top_push(t, x, v);
  };
  const int V4 = V & ~3;
#pragma unroll 4
  for (int v = lane * 4; v < V4; v += 256) {
    const float4 x = *reinterpret_cast<const float4*>(l + v);
    take(x.x, v); take(x.y, v + 1); take(x.z, v + 2); take(x.w, v + 3);
  }
  if (V4 + lane < V) take(l[V4 + lane], V4 + lane);
}

// LM: the n-gram arm, CTX: the phrase arm; <.., false, false> is the plain search and instantiates none of their code
template <typename T, bool MFMA, bool LM, bool CTX>
__global__ __launch_bounds__(RB_THREADS) void rnnt_beam_kernel(RbArgs a, std::conditional_t<LM || CTX, RbFuse, RbNoFuse> fz) {
  constexpr bool FUSED = LM || CTX;                            // entries are ranked by f = score + bonus and the result is ordered again
  constexpr int EPC = DT<T>::EPC;
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_dyn[];
  T* zl = reinterpret_cast<T*>(rb_dyn);                        // z rows [16][J + EPC]
  // C_s, double buffered: node -1 is no entry.  l1 / l2: the last label and the one before (sos where there is none)
  __shared__ double c_score[2][RB_MAX];
  __shared__ uint32_t c_klo[2][RB_MAX], c_khi[2][RB_MAX];
  __shared__ int c_node[2][RB_MAX], c_l1[2][RB_MAX], c_l2[2][RB_MAX];
  __shared__ double d_score[RB_DMAX];                          // D, in order of first insertion
  __shared__ uint32_t d_klo[RB_DMAX], d_khi[RB_DMAX];
  __shared__ int d_node[RB_DMAX], d_l1[RB_DMAX], d_l2[RB_DMAX];
  __shared__ int d_n;
  __shared__ int k_lab[RB_MAX][RB_MAX];                        // the rows' candidates and the blank's log-probability
  __shared__ float k_lp[RB_MAX][RB_MAX], r_lpb[RB_MAX];
  __shared__ double sc[RB_MAX * RB_MAX];                       // candidate x = r K + k: its score and its tie key (r << 32 | label)
  __shared__ uint64_t sc_tie[RB_MAX * RB_MAX];
  __shared__ int o_len[RB_MAX];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int T_ = a.T, J = a.J, V = a.V, W = a.W, K = a.K, S = a.S, blank = a.blank, ldv = a.ldv;
  const int Tb = clampi(a.frames[b], 0, T_);
  const int JC = J / EPC, zld = J + EPC;
  const T* e_b = reinterpret_cast<const T*>(a.e) + (int64_t)b * T_ * J;
  const T* tab0 = reinterpret_cast<const T*>(a.t0);
  const T* tab1 = reinterpret_cast<const T*>(a.t1);
  const T* w = reinterpret_cast<const T*>(a.w);
  float* lg = a.ws + (int64_t)b * a.ws_stride;
  int2* trie = reinterpret_cast<int2*>(lg + (int64_t)RB_MAX * ldv);
  // the fused arms' state (BeamExt, csrc/beam_fuse.h) of every entry of D (xd) and of C_s (xc: entry r of buffer c is cell c RB_MAX + r),
  // D's rank keys at the end of a frame and the final order, behind the z rows
  BeamExtSoa xd{}, xc{};
  double* x_df = nullptr;
  float* x_olm = nullptr; int *x_osrc = nullptr, *x_ocr = nullptr;
  if constexpr (FUSED) {
    unsigned char* q = rb_dyn + (size_t)RB_MAX * zld * sizeof(T);          // (a multiple of 16 bytes)
    xd.ctx = reinterpret_cast<uint64_t*>(q); q += RB_DMAX * 8;
    x_df = reinterpret_cast<double*>(q); q += RB_DMAX * 8;
    xc.ctx = reinterpret_cast<uint64_t*>(q); q += 2 * RB_MAX * 8;
    xd.lm = reinterpret_cast<float*>(q); q += RB_DMAX * 4;
    xd.len = reinterpret_cast<int*>(q); q += RB_DMAX * 4;
    xd.cst = reinterpret_cast<int*>(q); q += RB_DMAX * 4;
    xd.cnt = reinterpret_cast<int*>(q); q += RB_DMAX * 4;
    xc.lm = reinterpret_cast<float*>(q); q += 2 * RB_MAX * 4;
    xc.len = reinterpret_cast<int*>(q); q += 2 * RB_MAX * 4;
    xc.cst = reinterpret_cast<int*>(q); q += 2 * RB_MAX * 4;
    xc.cnt = reinterpret_cast<int*>(q); q += 2 * RB_MAX * 4;
    x_osrc = reinterpret_cast<int*>(q); q += RB_MAX * 4;
    x_olm = reinterpret_cast<float*>(q); q += RB_MAX * 4;
    x_ocr = reinterpret_cast<int*>(q);
  }

  if (tid < RB_MAX) {
    c_score[0][tid] = tid == 0 ? 0.0 : -(double)INFINITY;
    c_klo[0][tid] = tid == 0 ? BEAM_ROOT_KEY_LO : 0u;
    c_khi[0][tid] = tid == 0 ? BEAM_ROOT_KEY_HI : 0u;
    c_node[0][tid] = tid == 0 ? 0 : -1;                        // node 0 is the empty sequence
    c_l1[0][tid] = a.sos;
    c_l2[0][tid] = a.sos;
    // With phrases all five arrays are written: the moves below copy all five, and without an LM lm still enters the bonus as 0.f * lm.
    // The LM-only arms leave cst and cnt unwritten: they are moved along and never read (every use is under CTX), and the one more
    // store here measured 0.4 to 0.9 % of a batch in those arms (profiles/beam_fuse_refactor_isa.txt, 2a)
    if constexpr (CTX) xc.put<true, true>(tid, beam_ext_root<LM>(fz.ng, fz.bos));
    else if constexpr (LM) xc.put<true, false>(tid, beam_ext_root<LM>(fz.ng, fz.bos));
  }
  if (tid == 0) d_n = 0;
  __syncthreads();
  int cur = 0, n = 1;                                          // C_s = c_*[cur][0 .. n-1]; both are the same in every thread
  for (int t = 0; t < Tb; ++t) {
    for (int s = 0; s <= S; ++s) {
      // ---- 1: z rows
      for (int idx = tid; idx < RB_MAX * JC; idx += RB_THREADS) {
        const int row = idx / JC, c = idx - row * JC;
        Chunk<T> cz;
        cz.v = make_uint4(0u, 0u, 0u, 0u);
        if (row < n) {
          Chunk<T> ce, c0;
          ce.v = *reinterpret_cast<const uint4*>(e_b + (int64_t)t * J + c * EPC);
          c0.v = *reinterpret_cast<const uint4*>(tab0 + (int64_t)c_l1[cur][row] * J + c * EPC);
          if (tab1) {
            Chunk<T> c1;
            c1.v = *reinterpret_cast<const uint4*>(tab1 + (int64_t)c_l2[cur][row] * J + c * EPC);
#pragma unroll
            for (int i = 0; i < EPC; ++i) c0.e[i] = DT<T>::to(DT<T>::from(c0.e[i]) + DT<T>::from(c1.e[i]));
          }
#pragma unroll
          for (int i = 0; i < EPC; ++i) cz.e[i] = DT<T>::to(tanhf(DT<T>::from(ce.e[i]) + DT<T>::from(c0.e[i])));
        }
        *reinterpret_cast<uint4*>(zl + row * zld + c * EPC) = cz.v;
      }
      __syncthreads();
      // ---- 2: logits rows 0 .. n-1 -> workspace
      if constexpr (MFMA) {
        switch (J >> 5) {
          case 1: rb_proj_mfma<1>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          case 2: rb_proj_mfma<2>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          case 3: rb_proj_mfma<3>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          case 4: rb_proj_mfma<4>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          case 5: rb_proj_mfma<5>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          case 6: rb_proj_mfma<6>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          case 7: rb_proj_mfma<7>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
          default: rb_proj_mfma<8>(zl, zld, w, a.bias, J, V, n, lg, ldv, wave, lane); break;
        }
      } else {
        rb_proj_plain<T>(zl, zld, w, a.bias, J, V, n, lg, ldv, tid);
      }
      __syncthreads();
      // ---- 3: the rows' statistics and candidates, one wave per live row
      for (int row = wave; row < n; row += RB_WAVES) {
        const float* l = lg + (int64_t)row * ldv;
        const Lse st = lse_row(l, V, lane);
        const float lz = log1pf(st.s1);
        if (lane == 0) r_lpb[row] = (l[blank] - st.m) - lz;
        if (s < S) {
          RbTop tp;
          rb_top_scan(tp, l, V, lane, blank, INFINITY, -1);
          for (int j = 0; j < K; ++j) {
            const MaxIdx mi = wave_best(MaxIdx{tp.v[0], tp.i[0]});
            if (lane == 0) {                                   // (no entry left: only when logits are not numbers; any label in range, -inf)
              k_lab[row][j] = (unsigned)mi.i < (unsigned)V ? mi.i : (blank == 0 ? 1 : 0);
              k_lp[row][j] = (mi.v - st.m) - lz;
            }
            if (mi.i == tp.i[0] && mi.i != RB_NONE) {          // this lane's head was taken
#pragma unroll
              for (int q = 0; q + 1 < RB_TOP; ++q) { tp.v[q] = tp.v[q + 1]; tp.i[q] = tp.i[q + 1]; }
              tp.v[RB_TOP - 1] = -INFINITY;
              tp.i[RB_TOP - 1] = RB_NONE;
              if (tp.i[0] == RB_NONE && tp.more > 0) rb_top_scan(tp, l, V, lane, blank, mi.v, mi.i);
            }
          }
        }
      }
      __syncthreads();
      // ---- 4: blank step (the rows of C_s are distinct sequences: no two lanes meet in one entry) and the candidates' scores
      if (wave == 0) {
        const bool has = lane < n;
        const int dn = d_n;
        int found = -1;
        uint32_t klo = 0u, khi = 0u;
        if (has) {
          klo = c_klo[cur][lane];
          khi = c_khi[cur][lane];
          for (int i = 0; i < dn; ++i) found = d_klo[i] == klo && d_khi[i] == khi ? i : found;
        }
        const bool fresh = has && found < 0;
        const unsigned long long m = __ballot(fresh);
        if (has) {
          const double v = c_score[cur][lane] + (double)r_lpb[lane];
          if (found >= 0) {
            d_score[found] = rnnt_lae(d_score[found], v);
          } else {
            const int pos = dn + __popcll(m & ((1ull << lane) - 1ull));
            d_score[pos] = v;
            d_klo[pos] = klo;
            d_khi[pos] = khi;
            d_node[pos] = c_node[cur][lane];
            d_l1[pos] = c_l1[cur][lane];
            d_l2[pos] = c_l2[cur][lane];
            if constexpr (FUSED) {                             // the entry joins D with its whole state (field by field: beam_fuse.h)
              const int ce = cur * RB_MAX + lane;
              xd.ctx[pos] = xc.ctx[ce];
              xd.lm[pos] = xc.lm[ce];
              xd.len[pos] = xc.len[ce];
              xd.cst[pos] = xc.cst[ce];
              xd.cnt[pos] = xc.cnt[ce];
            }
          }
        }
        if (lane == 0) d_n = dn + __popcll(m);
      }
      const int nk = n * K;
      // fused arms: what candidate tid's entry would carry, kept in registers for phase 5 (the same thread places it)
      double e_ac = 0.0;
      BeamExt ex{0.f, 0, 0, 0, 0};
      if (s < S && tid < nk) {
        const int r = tid / K, k = tid - r * K;
        if constexpr (FUSED) {                                 // the step's lookups
          ex = beam_ext_extend<LM, CTX>(fz.ng, fz.cx, xc.get<LM, CTX>(cur * RB_MAX + r), k_lab[r][k]);
          e_ac = c_score[cur][r] + (double)k_lp[r][k];
          sc[tid] = e_ac + (double)beam_ext_bonus<LM, CTX>(fz.alpha, fz.beta, fz.gamma, ex);
        } else {
          sc[tid] = c_score[cur][r] + (double)k_lp[r][k];
        }
        sc_tie[tid] = (uint64_t)r << 32 | (uint32_t)k_lab[r][k];
      }
      __syncthreads();
      // ---- 5: C_{s+1} = the W best candidates
      if (s < S) {
        const int nxt = cur ^ 1;
        if (tid < nk) {
          const double my = sc[tid];
          const uint64_t tie = sc_tie[tid];
          int rank = 0;
          for (int y = 0; y < nk; ++y) {
            const double o = sc[y];
            rank += o > my || (o == my && sc_tie[y] < tie);
          }
          if (rank < W) {
            const int r = (int)(tie >> 32), label = (int)(uint32_t)tie;
            const int node = 1 + (t * S + s) * W + rank;
            const uint2 key = beam_key(make_uint2(c_klo[cur][r], c_khi[cur][r]), label);
            trie[node] = make_int2(c_node[cur][r], label);
            c_score[nxt][rank] = FUSED ? e_ac : my;            // (fused: my is the rank key f, the entry keeps the acoustic score)
            c_klo[nxt][rank] = key.x;
            c_khi[nxt][rank] = key.y;
            c_node[nxt][rank] = node;
            c_l1[nxt][rank] = label;
            c_l2[nxt][rank] = c_l1[cur][r];
            if constexpr (FUSED) {
              const int ne = nxt * RB_MAX + rank;
              xc.ctx[ne] = ex.ctx;
              xc.lm[ne] = ex.lm;
              xc.len[ne] = ex.len;
              xc.cst[ne] = ex.cst;
              xc.cnt[ne] = ex.cnt;
            }
          }
        }
        n = nk < W ? nk : W;
        cur = nxt;
        __syncthreads();
      }
    }
    // ---- A = the W best of D, the next frame's C_0
    const int dn = d_n, nxt = cur ^ 1;
    const double* d_rank = d_score;                            // what D is ranked by: the score, or f in the fused arms
    if constexpr (FUSED) {
      for (int i = tid; i < dn; i += RB_THREADS)
        x_df[i] = d_score[i] + (double)beam_bonus<LM, CTX>(fz.alpha, fz.beta, fz.gamma, xd.lm[i], xd.len[i], xd.cnt[i]);
      d_rank = x_df;
      __syncthreads();
    }
    for (int i = tid; i < dn; i += RB_THREADS) {
      const double my = d_rank[i];
      int rank = 0;
      for (int y = 0; y < dn; ++y) {
        const double o = d_rank[y];
        rank += o > my || (o == my && y < i);
      }
      if (rank < W) {
        c_score[nxt][rank] = d_score[i];
        c_klo[nxt][rank] = d_klo[i];
        c_khi[nxt][rank] = d_khi[i];
        c_node[nxt][rank] = d_node[i];
        c_l1[nxt][rank] = d_l1[i];
        c_l2[nxt][rank] = d_l2[i];
        if constexpr (FUSED) {
          const int ne = nxt * RB_MAX + rank;
          xc.ctx[ne] = xd.ctx[i];
          xc.lm[ne] = xd.lm[i];
          xc.len[ne] = xd.len[i];
          xc.cst[ne] = xd.cst[i];
          xc.cnt[ne] = xd.cnt[i];
        }
      }
    }
    n = dn < W ? dn : W;
    cur = nxt;
    __syncthreads();
    if (tid == 0) d_n = 0;                                     // (read next behind three barriers)
  }
  // ---- the n-best: one lane per hypothesis walks its parent chain (a parent is an older node: the chain ends at node 0)
  if constexpr (FUSED) {    // the final order: score + bonus(lm + q(nctx, eos), len, earned), the place in A first among equals; earned =
    const bool live = tid < n;                                 // cnt - hold(cst): an unfinished phrase earns nothing
    double fk = -(double)INFINITY;
    float lmv = 0.f;
    int cr = 0;
    if (live) {
      BeamExt e = xc.get<LM, CTX>(cur * RB_MAX + tid);
      if constexpr (LM) {
        if (fz.eos >= 0) e.lm = e.lm + ngram_query(fz.ng, e.ctx, fz.eos);
      }
      if constexpr (CTX) e.cnt = beam_ext_earned(fz.cx, e);
      lmv = e.lm;
      cr = e.cnt;
      fk = c_score[cur][tid] + (double)beam_ext_bonus<LM, CTX>(fz.alpha, fz.beta, fz.gamma, e);
    }
    if (tid < RB_MAX) { sc[tid] = fk; x_osrc[tid] = -1; }
    __syncthreads();
    if (live) {
      int rank = 0;
      for (int i = 0; i < n; ++i) {
        const double v = sc[i];
        rank += v > fk || (v == fk && i < tid);
      }
      x_osrc[rank] = tid;
      x_olm[rank] = lmv;
      x_ocr[rank] = cr;
    }
    __syncthreads();
  }
  const int L = T_ * S;
  int32_t* ids_b = a.ids + (int64_t)b * a.nbest * L;
  if (tid < a.nbest) {
    int len = -1, src = tid < n ? tid : -1;                    // the place in A of hypothesis tid (-1: none)
    if constexpr (FUSED) src = tid < n ? x_osrc[tid] : -1;
    if (src >= 0) {
      const int node = c_node[cur][src];
      len = 0;
      for (int nd = node; nd > 0 && len < L; nd = trie[nd].x) ++len;
      int p = len;
      for (int nd = node; nd > 0 && p > 0;) {
        const int2 en = trie[nd];
        ids_b[(int64_t)tid * L + --p] = en.y;
        nd = en.x;
      }
    }
    o_len[tid] = len < 0 ? 0 : len;
    a.lengths[(int64_t)b * a.nbest + tid] = len;
    a.scores[(int64_t)b * a.nbest + tid] = src >= 0 ? (float)c_score[cur][src] : -INFINITY;
    if constexpr (FUSED) fz.lm[(int64_t)b * a.nbest + tid] = src >= 0 ? x_olm[tid] : 0.f;
    if constexpr (CTX) fz.credit[(int64_t)b * a.nbest + tid] = src >= 0 ? x_ocr[tid] : 0;
  }
  __syncthreads();
  for (int y = tid; y < a.nbest * L; y += RB_THREADS) {
    const int r = y / L;
    if (y - r * L >= o_len[r]) ids_b[y] = blank;
  }
}

}  // namespace

extern "C" int64_t asr_rnnt_beam_workspace(int B, int T, int V, int W, int K, int S) {
  if (B <= 0 || T <= 0 || V <= 0 || W < 1 || K < 1 || S < 1) return 0;
  return (int64_t)B * rb_stride(T, V, W, S);
}

namespace {

// every entry: the plain search's checks, then the arm for the dtype and J
template <bool LM, bool CTX>
int rb_search(const void* e, const void* table0, const void* table1, const void* w_out, const float* b_out, const int32_t* frame_lengths,
              int B, int T, int J, int V, int W, int K, int S, int nbest, int blank, int sos, int dtype, float* workspace,
              int64_t workspace_floats, int32_t* ids, int32_t* lengths, float* scores,
              std::conditional_t<LM || CTX, RbFuse, RbNoFuse> fz, hipStream_t s) {
  ASR_CHECK_ARG(e && table0 && w_out && b_out && frame_lengths && workspace && ids && lengths && scores);
  ASR_CHECK_ARG(B > 0 && T > 0 && J > 0 && V > 0 && W >= 1 && K >= 1 && nbest >= 1);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  ASR_CHECK_ARG(blank >= 0 && blank < V && sos >= 0 && sos < V);
  if (W > RB_MAX || K > RB_MAX || nbest > W || S < 1) return ASR_EUNSUPPORTED;
  ASR_CHECK_ARG(K < V);                                        // K non-blank labels exist
  if ((int64_t)W * ((int64_t)S + 1) > RB_DMAX) return ASR_EUNSUPPORTED;      // D does not fit LDS
  if ((int64_t)T * S * W >= (1 << 30) || (int64_t)nbest * T * S >= ((int64_t)1 << 31)) return ASR_EUNSUPPORTED;
  if (J % 8 != 0 || !aligned16(e) || !aligned16(table0) || !aligned16(table1) || !aligned16(w_out) || !aligned16(workspace))
    return ASR_EUNSUPPORTED;                                   // whole 16-byte chunks in both dtypes
  ASR_CHECK_ARG(workspace_floats >= asr_rnnt_beam_workspace(B, T, V, W, K, S));
  // the fused arms' state sits behind the z rows: their J limit is lower by RB_FUSE_BYTES of rows (fp32 J <= 1384, bf16 J <= 2776)
  const size_t lds = (size_t)RB_MAX * (J + (dtype == ASR_BF16 ? 8 : 4)) * (dtype == ASR_BF16 ? 2 : 4) + (LM || CTX ? RB_FUSE_BYTES : 0);
  if (lds > RB_LDS_DYN_MAX) return ASR_EUNSUPPORTED;
  const RbArgs a{e, table0, table1, w_out, b_out, frame_lengths, T, J, V, W, K, S, nbest, blank, sos, rb_ldv(V), workspace,
                 rb_stride(T, V, W, S), ids, lengths, scores};
  AsrProfScope prof(ASR_OP_SEARCH, s);
  if (dtype == ASR_BF16 && J % 32 == 0 && J <= 32 * RB_NK_MAX)
    return asr_launch<rnnt_beam_kernel<bf16_t, true, LM, CTX>>(dim3(B), dim3(RB_THREADS), lds, s, a, fz);
  if (dtype == ASR_BF16) return asr_launch<rnnt_beam_kernel<bf16_t, false, LM, CTX>>(dim3(B), dim3(RB_THREADS), lds, s, a, fz);
  return asr_launch<rnnt_beam_kernel<float, false, LM, CTX>>(dim3(B), dim3(RB_THREADS), lds, s, a, fz);
}

}  // namespace

extern "C" int asr_rnnt_beam_search(const void* e, const void* table0, const void* table1, const void* w_out, const float* b_out,
                                    const int32_t* frame_lengths, int B, int T, int J, int V, int W, int K, int S, int nbest, int blank,
                                    int sos, int dtype, float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths,
                                    float* scores, hipStream_t s) {
  return rb_search<false, false>(e, table0, table1, w_out, b_out, frame_lengths, B, T, J, V, W, K, S, nbest, blank, sos, dtype, workspace,
                                 workspace_floats, ids, lengths, scores, RbNoFuse{}, s);
}

// The n-gram arm: the table must hold a unigram for every label 0..V-1 (utils/ngram.py's estimator does), so that every q is finite.
extern "C" int asr_rnnt_beam_search_lm(const void* e, const void* table0, const void* table1, const void* w_out, const float* b_out,
                                       const int32_t* frame_lengths, int B, int T, int J, int V, int W, int K, int S, int nbest, int blank,
                                       int sos, int dtype, float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths,
                                       float* scores, const uint64_t* keys, const float* vals, int64_t capacity, int max_probe, int order,
                                       int bos, int eos, float alpha, float beta, float* lm, hipStream_t s) {
  ASR_CHECK_ARG(lm);
  RbFuse fz{NgramTable{}, beam_no_ctx(), bos, eos, alpha, beta, 0.f, lm, nullptr};
  const int rc = beam_ngram_table(keys, vals, capacity, max_probe, order, bos, eos, V, &fz.ng);
  if (rc != ASR_OK) return rc;
  return rb_search<true, false>(e, table0, table1, w_out, b_out, frame_lengths, B, T, J, V, W, K, S, nbest, blank, sos, dtype, workspace,
                                workspace_floats, ids, lengths, scores, fz, s);
}

// The phrase arms: the table of utils/context.py (ContextGraph.device_table).  ng_keys == NULL: no LM -- alpha, bos and eos are not looked
// at, lm is 0 for every hypothesis and the length bonus beta still counts.
extern "C" int asr_rnnt_beam_search_ctx(const void* e, const void* table0, const void* table1, const void* w_out, const float* b_out,
                                        const int32_t* frame_lengths, int B, int T, int J, int V, int W, int K, int S, int nbest, int blank,
                                        int sos, int dtype, float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths,
                                        float* scores, const uint64_t* ng_keys, const float* ng_vals, int64_t ng_capacity,
                                        int ng_max_probe, int ng_order, int bos, int eos, float alpha, float beta,
                                        const uint64_t* cx_keys, const int32_t* cx_vals, int64_t cx_capacity, int cx_max_probe,
                                        const int32_t* cx_hold, int cx_states, float gamma, float* lm, int32_t* credit, hipStream_t s) {
  ASR_CHECK_ARG(lm && credit);
  CtxTable cx;
  int rc = beam_ctx_table(cx_keys, cx_vals, cx_capacity, cx_max_probe, cx_hold, cx_states, V, &cx);
  if (rc != ASR_OK) return rc;
  if (!ng_keys)
    return rb_search<false, true>(e, table0, table1, w_out, b_out, frame_lengths, B, T, J, V, W, K, S, nbest, blank, sos, dtype, workspace,
                                  workspace_floats, ids, lengths, scores, RbFuse{beam_no_ngram(), cx, 0, -1, 0.f, beta, gamma, lm, credit}, s);
  RbFuse fz{NgramTable{}, cx, bos, eos, alpha, beta, gamma, lm, credit};
  rc = beam_ngram_table(ng_keys, ng_vals, ng_capacity, ng_max_probe, ng_order, bos, eos, V, &fz.ng);
  if (rc != ASR_OK) return rc;
  return rb_search<true, true>(e, table0, table1, w_out, b_out, frame_lengths, B, T, J, V, W, K, S, nbest, blank, sos, dtype, workspace,
                               workspace_floats, ids, lengths, scores, fz, s);
}
