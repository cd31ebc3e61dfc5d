// CTC prefix beam search: the n best label sequences of the encoder CTC head's posteriors, from the head alone.  Where asr_ctc_align
// (ctc_align.hip) follows the one best path of a GIVEN sequence, this kernel searches the sequences and sums over the alignments of each.
//
// Per utterance b over its T_b true frames; lp(t, v) = logits[b, t, v] - lse[t] (one fp32 subtraction, the only source of
// log-probabilities); every log-add is the -inf safe lae2 of ctc_common.h.  tests/ctc_beam_reference.py restates this in NumPy.
//
//   candidates of frame t   the C labels with the largest raw logit, lowest index first among equals (idx of asr_logsoftmax_topk, k = C),
//                           the blank dropped, order kept
//   state                   an ordered list of at most W prefixes g with p_b(g), p_nb(g): the log-probability of the alignments of g over
//                           the frames so far that end in a blank / in a label.  Before frame 0: [() : p_b = 0, p_nb = -inf]
//   step t, slots in order  stay i        p_b' = tot(g) + lp(t, blank), p_nb' = p_nb(g) + lp(t, last(g)) (-inf for ());  tot = lae2(p_b, p_nb)
//                           W + j C + k   prefix h = list[j] extended by candidate c = k-th: p_b' = -inf,
//                                         p_nb' = (p_b(h) if c == last(h) else tot(h)) + lp(t, c)
//   merge                   when h.c is itself list[i], the extension's value is log-added into stay slot i,
//                           p_nb'(i) = lae2(repeat term, extension term), and the extension slot is dead
//   prune                   slots ranked by lae2(p_b', p_nb'), greater first, lower slot index first among equals; the best W slots with a
//                           finite score are the new list, in rank order
//   result                  the first nbest prefixes after frame T_b - 1, score = lae2(p_b, p_nb); missing entries: length -1, score -inf
//
// One workgroup per utterance walks the frames with the beam in LDS.  A thread owns one slot (256 threads, 320 for the 272 slots of
// W = C = 16) and keeps its p_b', p_nb' in registers between the step's two barriers: only the slot scores go through LDS, where every
// slot counts the slots that beat it (float4 reads of one score array, four in flight: no sort, no atomics, one fixed result).  The
// step is a chain of LDS latencies, so the 16-entry rows a slot searches (node ids, parents, last labels, candidates) are read as four
// 16-byte loads at once and compared in registers.
// A prefix is a node of a trie of (parent node, label) pairs in the caller's workspace: the survivor created at frame t with rank r owns node
// 1 + t W + r, so the trie needs no allocation counter.  A node id does not identify a label sequence, though: a prefix pruned and later
// re-created owns a new node while its children still in the list point at the old one.  Every list entry therefore carries a 64-bit
// key mixed from its parent's key and its last label (beam_key) and its parent's key; a stay slot finds its parent, and an extension the
// list entry it would duplicate, by comparing keys (<= 16 compares), so the merge is by label sequence, as the definition says.  The candidates' labels and log-probabilities and the blank's are staged
// 16 frames ahead in registers and handed to LDS at the chunk boundary, so the walk's global reads are off its critical path -- except
// lp(t, last(g)) of a prefix whose last label is NOT among the frame's candidates, the one dependent read (in a peaked posterior the
// label of a live prefix usually is a candidate and the staged value -- the same fp32 subtraction -- is used).
//
// The fused arm (asr_ctc_beam_search_lm, template <true>): a label n-gram LM has its say while the beam is pruned.  q(h, c) is the query
// of csrc/ngram.h; tests/ctc_beam_lm_reference.py restates the arm.  Added to the definition above:
//   state, step             every list entry also carries the BeamExt of csrc/beam_fuse.h (lm, len, ctx; root and extension are defined
//                           there, once for both searches); a stay slot keeps it
//   prune                   slots ranked by f = tot + (alpha lm + beta (float)len) in fp32, tot = lae2(p_b', p_nb'); greater first, lower
//                           slot index first among equals; a slot is live iff tot is finite
//   result                  the W entries ordered by f + alpha q(ctx, eos) (f alone for eos = -1), the list place first among equals; the
//                           first nbest are written: scores = tot (the CTC log-probability, as in the plain search), lm = the raw lm sum
//                           with the end term; missing entries: length -1, scores and lm -inf
// Only a live extension slot that is no merge runs a lookup, a dependent global read inside the step; the entries' extra state lives in
// LDS and the workspace is the plain search's.  The plain arm instantiates none of it.
//
// The phrase arms (asr_ctc_beam_search_ctx, template <LM, true>): hypotheses that spell a listed phrase get a bonus while the beam is
// pruned.  state(y), credit(y), hold(s) and earned(y) are those of utils/context.py, step(s, c) -> (next, delta) the lookup of
// csrc/context.h; tests/ctc_beam_ctx_reference.py restates the arms.  Added to the definitions above:
//   state, step             BeamExt's cst = state(prefix) and cnt = credit(prefix) are live; a stay slot keeps them
//   prune                   slots ranked by f = tot + ((alpha lm + beta (float)len) + gamma (float)cnt) in fp32, in this order; without an
//                           n-gram table lm = 0.f and len is still counted; liveness and the tie rules as above
//   result                  ordered by the fused arm's final key with gamma (float)earned in place of gamma (float)cnt, earned = cnt -
//                           hold(cst): a phrase left unfinished at the end of the utterance gets nothing.  Written: scores = tot, lm as in
//                           the fused arm (0 for found hypotheses without a table, -inf for missing ones), credit = earned (-1: missing)
// gamma times an integer: both arms and the host form the same bits from the same count.  The lookup sits where ngram_query sits, a live
// extension that is no merge.  The arms without phrases instantiate none of it.
#include <type_traits>

#include "ctc_common.h"      // NEG_INF, lae2, ctc_lse_kernel
#include "beam_key.h"        // beam_key, BEAM_ROOT_KEY_LO / _HI (shared with csrc/rnnt_beam.hip)
#include "beam_fuse.h"       // BeamExt and its lookups, the table checks (shared with csrc/rnnt_beam.hip; no lse.h before it)

namespace {

constexpr int BEAM_MAX = 16;                                  // W and C; C = TOPK_MAX of ce.hip
constexpr int BEAM_CHUNK = 16;                                // frames staged at a go: 16 frames x 16 candidates, one per staging thread
constexpr int BEAM_SLOTS = BEAM_MAX + BEAM_MAX * BEAM_MAX;    // 272

struct BeamStaged {       // a thread's piece of a chunk: candidate k = tid & 15 of frame t0 + (tid >> 4)
  int c;
  float lp, lpb, lse;
};

// 16 consecutive LDS words as four 16-byte reads in flight together (a scalar loop over them pays the LDS latency 16 times)
__device__ __forceinline__ void beam_row16(const int* p, int (&a)[BEAM_MAX]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int4 v = reinterpret_cast<const int4*>(p)[q];
    a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
  }
}

// What the fused arm adds to the plain search's arguments; the plain arm takes the empty BeamNoLm
struct BeamLm {
  NgramTable tab;
  int bos, eos;             // eos -1: no end term
  float alpha, beta;
  float* lm;                // (B,nbest)
};
struct BeamNoLm {};
// What the phrase arms add; with them and no LM, BeamLm still brings beta and lm (its table, bos, eos and alpha are not looked at)
struct BeamCtx {
  CtxTable tab;
  float gamma;
  int32_t* credit;          // (B,nbest)
};
struct BeamNoCtx {};

// blockDim.x = 256, or 320 when W + W C > 256: one slot per thread; the first 256 threads stage the chunks.  LM: the fused arm;
// CTX: the phrase arm, with or without it
template <bool LM, bool CTX>
__global__ __launch_bounds__(320) void ctc_beam_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ lse,
                                                       const int64_t* __restrict__ cand, const int32_t* __restrict__ in_len, int T, int W,
                                                       int C, int nbest, int blank, int2* trie, int32_t* __restrict__ ids,
                                                       int32_t* __restrict__ out_len, float* __restrict__ scores,
                                                       std::conditional_t<LM || CTX, BeamLm, BeamNoLm> fuse,
                                                       std::conditional_t<CTX, BeamCtx, BeamNoCtx> bias) {
  constexpr bool FUSED = LM || CTX;                  // the slots are ranked by a fused key and the final list is ordered again
  float gamma = 0.f;
  if constexpr (CTX) gamma = bias.gamma;
  // the list, double buffered; node -1: no entry (then keys 0, last -1, all three values -inf).  (klo, khi): the prefix' key, (plo, phi):
  // its parent's (0 for the empty prefix).  tot = lae2(p_b, p_nb), kept from the prune step that computed it as the slot's score
  __shared__ __attribute__((aligned(16))) int l_node[2][BEAM_MAX], l_last[2][BEAM_MAX];
  __shared__ __attribute__((aligned(16))) int l_klo[2][BEAM_MAX], l_khi[2][BEAM_MAX], l_plo[2][BEAM_MAX], l_phi[2][BEAM_MAX];
  __shared__ float l_pb[2][BEAM_MAX], l_pnb[2][BEAM_MAX], l_tot[2][BEAM_MAX];
  __shared__ __attribute__((aligned(16))) int c_id[BEAM_CHUNK][BEAM_MAX];          // candidates of the chunk's frames (-1: none)
  __shared__ float c_lp[BEAM_CHUNK][BEAM_MAX];
  __shared__ float f_lpb[BEAM_CHUNK], f_lse[BEAM_CHUNK];
  __shared__ __attribute__((aligned(16))) float sc[BEAM_SLOTS];
  __shared__ int o_len[BEAM_MAX];
  // the fused arms: the entries' BeamExt (csrc/beam_fuse.h: a stay slot keeps it, a merge needs no rule) as five parallel arrays, cst and
  // cnt for the phrase arms alone; `ext` views them: entry i of list buffer c is cell c * BEAM_MAX + i.  o_src: the list place of final rank r
  __shared__ float l_lm[2][BEAM_MAX], o_lm[BEAM_MAX];
  __shared__ uint64_t l_ctx[2][BEAM_MAX];
  __shared__ int l_len[2][BEAM_MAX], o_src[BEAM_MAX];
  __shared__ int l_cst[2][BEAM_MAX], l_cnt[2][BEAM_MAX], o_cr[BEAM_MAX];
  BeamExtSoa ext{}; CtxTable cx{};
  if constexpr (FUSED) ext = BeamExtSoa{&l_lm[0][0], &l_len[0][0], &l_ctx[0][0], &l_cst[0][0], &l_cnt[0][0]};
  if constexpr (CTX) cx = bias.tab;
  const int tid = threadIdx.x, b = blockIdx.x, nthr = blockDim.x;
  int Tb = in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float* lg = logits + (int64_t)b * T * ld;
  const float* lse_b = lse + (int64_t)b * T;
  const int64_t* cand_b = cand + (int64_t)b * T * C;
  int2* trie_b = trie + (int64_t)b * (1 + (int64_t)T * W);
  const int NS = W + W * C, NS16 = (NS + 15) & ~15;
  // this thread's slot x = tid: stay slot x < W, or the extension of list[sj] by candidate sk
  const int x = tid;
  const int sj = x >= W && x < NS ? (x - W) / C : 0;
  const int sk = x >= W && x < NS ? (x - W) % C : 0;
  if (tid < BEAM_MAX) {
    l_node[0][tid] = tid == 0 ? 0 : -1;                // node 0 is the empty prefix
    l_klo[0][tid] = tid == 0 ? (int)BEAM_ROOT_KEY_LO : 0;
    l_khi[0][tid] = tid == 0 ? (int)BEAM_ROOT_KEY_HI : 0;
    l_plo[0][tid] = 0;
    l_phi[0][tid] = 0;
    l_last[0][tid] = -1;
    l_pb[0][tid] = tid == 0 ? 0.f : NEG_INF;
    l_pnb[0][tid] = NEG_INF;
    l_tot[0][tid] = tid == 0 ? 0.f : NEG_INF;          // lae2(0, -inf) = 0
    if constexpr (FUSED) ext.put<LM, CTX>(tid, beam_ext_root<LM>(fuse.tab, fuse.bos));
  }
  for (int y = tid; y < BEAM_SLOTS; y += nthr) sc[y] = NEG_INF;         // (slots >= NS are never written: they never count)

  auto load = [&](int t0) {
    BeamStaged s;
    const int t = t0 + (tid >> 4), k = tid & 15;
    const bool frame = tid < 256 && t < Tb, valid = frame && k < C;
    s.c = valid ? (int)cand_b[(int64_t)t * C + k] : -1;
    s.lse = frame ? lse_b[t] : 0.f;
    s.lp = valid ? lg[(int64_t)t * ld + s.c] - s.lse : NEG_INF;
    s.lpb = frame && k == 0 ? lg[(int64_t)t * ld + blank] - s.lse : 0.f;
    return s;
  };
  BeamStaged st = load(0);
  int cur = 0;
  for (int t0 = 0; t0 < Tb; t0 += BEAM_CHUNK) {
    if (tid < 256) {   // the staged chunk goes to LDS, the blank squeezed out of every frame's candidates (a top-C of finite logits holds it at most once)
      const int f = tid >> 4, k = tid & 15;
      const bool is_blank = st.c == blank;
      const unsigned long long m = __ballot(is_blank);
      const unsigned bits = (unsigned)(m >> (((tid & 63) >> 4) * 16)) & 0xffffu;
      const int before = __popc(bits & ((1u << k) - 1u)), nblank = __popc(bits);
      if (st.c >= 0 && !is_blank) { c_id[f][k - before] = st.c; c_lp[f][k - before] = st.lp; }
      if (k >= C - nblank) { c_id[f][k] = -1; c_lp[f][k] = NEG_INF; }
      if (k == 0) { f_lpb[f] = st.lpb; f_lse[f] = st.lse; }
    }
    __syncthreads();
    if (t0 + BEAM_CHUNK < Tb) st = load(t0 + BEAM_CHUNK);
    const int n = Tb - t0 < BEAM_CHUNK ? Tb - t0 : BEAM_CHUNK;
    for (int f = 0; f < n; ++f) {
      const int t = t0 + f, nxt = cur ^ 1;
      float npb = NEG_INF, npnb = NEG_INF, sx = NEG_INF;
      int ext_c = -1;
      // fused arm: the slot's rank key f = tot + (alpha lm + beta len) (the plain arm ranks by sx = tot itself) and what its entry carries
      float fx = NEG_INF;
      BeamExt ex{0.f, 0, 0, 0, 0};
      if (x < W) {
        int cid[BEAM_MAX], klo[BEAM_MAX], khi[BEAM_MAX];
        beam_row16(c_id[f], cid);
        beam_row16(l_klo[cur], klo);
        beam_row16(l_khi[cur], khi);
        const int last = l_last[cur][x], plo = l_plo[cur][x], phi = l_phi[cur][x];
        const float pnb = l_pnb[cur][x];
        npb = l_tot[cur][x] + f_lpb[f];
        if (last >= 0) {
          int kk = -1, jj = -1;
#pragma unroll
          for (int k = 0; k < BEAM_MAX; ++k) {
            kk = cid[k] == last ? k : kk;
            jj = klo[k] == plo && khi[k] == phi ? k : jj;          // (a parent key has bit 0 set here; an empty place holds 0)
          }
          const float lpl = kk >= 0 ? c_lp[f][kk] : lg[(int64_t)t * ld + last] - f_lse[f];
          npnb = pnb + lpl;
          if (kk >= 0 && jj >= 0) {                      // the label is a candidate and the parent is in the list: its extension lands here
            const float base = l_last[cur][jj] == last ? l_pb[cur][jj] : l_tot[cur][jj];
            npnb = lae2(npnb, base + lpl);
          }
        }
        sx = lae2(npb, npnb);
        if constexpr (FUSED) {                               // a stay slot keeps its state
          ex = ext.get<LM, CTX>(cur * BEAM_MAX + x);
          if (sx > NEG_INF) fx = sx + beam_ext_bonus<LM, CTX>(fuse.alpha, fuse.beta, gamma, ex);
        }
        sc[x] = FUSED ? fx : sx;
      } else if (x < NS) {
        int plos[BEAM_MAX], phis[BEAM_MAX], lasts[BEAM_MAX];
        beam_row16(l_plo[cur], plos);
        beam_row16(l_phi[cur], phis);
        beam_row16(l_last[cur], lasts);
        const int c = c_id[f][sk], hn = l_node[cur][sj], hl = l_last[cur][sj], hklo = l_klo[cur][sj], hkhi = l_khi[cur][sj];
        const float hb = l_pb[cur][sj], ht = l_tot[cur][sj], lpc = c_lp[f][sk];
        if (c >= 0 && hn >= 0) {
          bool merged = false;
#pragma unroll
          for (int i = 0; i < BEAM_MAX; ++i) merged |= plos[i] == hklo && phis[i] == hkhi && lasts[i] == c;
          if (!merged) {
            npnb = (hl == c ? hb : ht) + lpc;
            sx = npnb;
            ext_c = c;
            if constexpr (FUSED) {
              if (sx > NEG_INF) {                          // a live extension that is no merge: the one lookup of the step
                ex = beam_ext_extend<LM, CTX>(fuse.tab, cx, ext.get<LM, CTX>(cur * BEAM_MAX + sj), c);
                fx = sx + beam_ext_bonus<LM, CTX>(fuse.alpha, fuse.beta, gamma, ex);
              }
            }
          }
        }
        sc[x] = FUSED ? fx : sx;
      }
      if (tid < BEAM_MAX) {                                   // places no survivor takes stay empty
        l_node[nxt][tid] = -1;
        l_klo[nxt][tid] = 0;
        l_khi[nxt][tid] = 0;
        l_plo[nxt][tid] = 0;
        l_phi[nxt][tid] = 0;
        l_last[nxt][tid] = -1;
        l_pb[nxt][tid] = NEG_INF;
        l_pnb[nxt][tid] = NEG_INF;
        l_tot[nxt][tid] = NEG_INF;
      }
      __syncthreads();
      if (x < NS && sx > NEG_INF) {
        const float rx = FUSED ? fx : sx;
        int rank = 0;
        for (int y = 0; y < NS16; y += 16) {
#pragma unroll
          for (int q = 0; q < 16; q += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&sc[y + q]);
            rank += (v.x > rx || (v.x == rx && y + q < x)) + (v.y > rx || (v.y == rx && y + q + 1 < x)) +
                    (v.z > rx || (v.z == rx && y + q + 2 < x)) + (v.w > rx || (v.w == rx && y + q + 3 < x));
          }
        }
        if (rank < W) {
          int node, last;
          uint2 key, pkey;
          if (x < W) {
            node = l_node[cur][x];
            last = l_last[cur][x];
            key = make_uint2((uint32_t)l_klo[cur][x], (uint32_t)l_khi[cur][x]);
            pkey = make_uint2((uint32_t)l_plo[cur][x], (uint32_t)l_phi[cur][x]);
          } else {
            node = 1 + t * W + rank;
            last = ext_c;
            pkey = make_uint2((uint32_t)l_klo[cur][sj], (uint32_t)l_khi[cur][sj]);
            key = beam_key(pkey, last);
            trie_b[node] = make_int2(l_node[cur][sj], last);
          }
          l_node[nxt][rank] = node;
          l_klo[nxt][rank] = (int)key.x;
          l_khi[nxt][rank] = (int)key.y;
          l_plo[nxt][rank] = (int)pkey.x;
          l_phi[nxt][rank] = (int)pkey.y;
          l_last[nxt][rank] = last;
          l_pb[nxt][rank] = npb;
          l_pnb[nxt][rank] = npnb;
          l_tot[nxt][rank] = sx;
          if constexpr (FUSED) ext.put<LM, CTX>(nxt * BEAM_MAX + rank, ex);
        }
      }
      __syncthreads();
      cur = nxt;
    }
  }
  __syncthreads();
  if constexpr (FUSED) {    // the final order: f + alpha q(ctx, eos) (f alone without an end term), the list place first among equals;
    const bool live = tid < W && l_node[cur][tid] >= 0;       // the phrase arms count what is earned: an unfinished phrase gets nothing
    float fk = NEG_INF, lmv = NEG_INF;
    int cr = -1;
    if (live) {
      BeamExt e = ext.get<LM, CTX>(cur * BEAM_MAX + tid);
      lmv = e.lm;
      if constexpr (CTX) e.cnt = cr = beam_ext_earned(cx, e);
      fk = l_tot[cur][tid] + beam_ext_bonus<LM, CTX>(fuse.alpha, fuse.beta, gamma, e);
      if constexpr (LM) {
        if (fuse.eos >= 0) {
          const float qe = ngram_query(fuse.tab, e.ctx, fuse.eos);
          fk = fk + fuse.alpha * qe;
          lmv = lmv + qe;
        }
      }
    }
    if (tid < BEAM_MAX) { sc[tid] = fk; o_src[tid] = -1; }
    __syncthreads();
    if (live) {
      int rank = 0;
      for (int i = 0; i < W; ++i) {
        const float v = sc[i];
        rank += v > fk || (v == fk && i < tid);
      }
      o_src[rank] = tid;
      o_lm[rank] = lmv;
      if constexpr (CTX) o_cr[rank] = cr;
    }
    __syncthreads();
  }
  // the n-best: one lane per hypothesis walks its parent chain (a parent is an older node: the chain ends at node 0)
  int32_t* ids_b = ids + (int64_t)b * nbest * T;
  if (tid < nbest) {
    const int src = FUSED ? o_src[tid] : tid;               // the list place of hypothesis tid (fused arm: -1 where there is none)
    const int node = src >= 0 ? l_node[cur][src] : -1;
    int len = -1;
    if (node >= 0) {
      len = 0;
      for (int nd = node; nd > 0 && len < T; nd = trie_b[nd].x) ++len;
      int p = len;
      for (int nd = node; nd > 0 && p > 0;) {
        const int2 e = trie_b[nd];
        ids_b[(int64_t)tid * T + --p] = e.y;
        nd = e.x;
      }
    }
    o_len[tid] = len < 0 ? 0 : len;
    out_len[(int64_t)b * nbest + tid] = len;
    scores[(int64_t)b * nbest + tid] = src >= 0 ? l_tot[cur][src] : NEG_INF;
    if constexpr (FUSED) fuse.lm[(int64_t)b * nbest + tid] = src >= 0 ? o_lm[tid] : NEG_INF;
    if constexpr (CTX) bias.credit[(int64_t)b * nbest + tid] = src >= 0 ? o_cr[tid] : -1;
  }
  __syncthreads();
  for (int y = tid; y < nbest * T; y += nthr) {
    const int r = y / T;
    if (y - r * T >= o_len[r]) ids_b[y] = blank;
  }
}

// workspace, in floats: row lse (B T) | the top-C values, unused (B T C) | [pad to 8 bytes] the top-C indices, int64 (B T C) | the trie
inline int64_t beam_idx_offset(int64_t B, int64_t T, int64_t C) { return (B * T + B * T * C + 1) & ~(int64_t)1; }

}  // namespace

extern "C" int64_t asr_ctc_beam_workspace(int B, int T, int W, int C) {
  if (B <= 0 || T <= 0 || W < 1 || C < 1) return 0;
  return beam_idx_offset(B, T, C) + 2 * (int64_t)B * T * C + 2 * (int64_t)B * (1 + (int64_t)T * W);
}

namespace {

// every entry: the row log-sum-exp, the candidates, then the search with or without the fused LM and the phrase automaton
template <bool LM, bool CTX>
int beam_search(const float* logits, int64_t ld, const int32_t* input_lengths, int B, int T, int V, int W, int C, int nbest, int blank,
                float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths, float* scores,
                std::conditional_t<LM || CTX, BeamLm, BeamNoLm> fuse, std::conditional_t<CTX, BeamCtx, BeamNoCtx> bias, hipStream_t s) {
  ASR_CHECK_ARG(logits && input_lengths && workspace && ids && lengths && scores);
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && ld >= V && W >= 1 && C >= 1 && nbest >= 1 && blank >= 0 && blank < V);
  if (W > BEAM_MAX || C > BEAM_MAX || nbest > W) return ASR_EUNSUPPORTED;
  ASR_CHECK_ARG(C <= V && (int64_t)T * W < (1 << 30) && (((uintptr_t)workspace) & 7) == 0);
  ASR_CHECK_ARG(workspace_floats >= asr_ctc_beam_workspace(B, T, W, C));
  const int64_t rows = (int64_t)B * T;
  ASR_CHECK_ARG(rows < (1 << 30));
  float* lse = workspace;
  float* vals = workspace + rows;
  int64_t* idx = reinterpret_cast<int64_t*>(workspace + beam_idx_offset(B, T, C));
  int2* trie = reinterpret_cast<int2*>(idx + rows * C);
  AsrProfScope prof(ASR_OP_CE, s);
  hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, ld, rows, V, lse);
  ASR_LAUNCH_CHECK();
  const int rc = asr_logsoftmax_topk(logits, ld, (int)rows, V, C, vals, idx, s);
  if (rc != ASR_OK) return rc;
  const int threads = W + W * C > 256 ? 320 : 256;                 // one per slot
  hipLaunchKernelGGL((ctc_beam_kernel<LM, CTX>), dim3(B), dim3(threads), 0, s, logits, ld, lse, idx, input_lengths, T, W, C, nbest, blank,
                     trie, ids, lengths, scores, fuse, bias);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

}  // namespace

extern "C" int asr_ctc_beam_search(const float* logits, int64_t ld, const int32_t* input_lengths, int B, int T, int V, int W, int C,
                                   int nbest, int blank, float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths,
                                   float* scores, hipStream_t s) {
  return beam_search<false, false>(logits, ld, input_lengths, B, T, V, W, C, nbest, blank, workspace, workspace_floats, ids, lengths,
                                   scores, BeamNoLm{}, BeamNoCtx{}, s);
}

// The fused arm: the table must hold a unigram for every label 0..V-1 (utils/ngram.py's estimator does), so that every q is finite.
extern "C" int asr_ctc_beam_search_lm(const float* logits, int64_t ld, const int32_t* input_lengths, int B, int T, int V, int W, int C,
                                      int nbest, int blank, float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths,
                                      float* scores, const uint64_t* keys, const float* vals, int64_t capacity, int max_probe, int order,
                                      int bos, int eos, float alpha, float beta, float* lm, hipStream_t s) {
  ASR_CHECK_ARG(lm);
  NgramTable tab;
  const int rc = beam_ngram_table(keys, vals, capacity, max_probe, order, bos, eos, V, &tab);
  if (rc != ASR_OK) return rc;
  return beam_search<true, false>(logits, ld, input_lengths, B, T, V, W, C, nbest, blank, workspace, workspace_floats, ids, lengths,
                                  scores, BeamLm{tab, bos, eos, alpha, beta, lm}, BeamNoCtx{}, s);
}

// The phrase arms: the table of utils/context.py (ContextGraph.device_table).  ng_keys == NULL: no LM -- alpha, bos and eos are not looked
// at, lm is 0 for every found hypothesis and the length bonus beta still counts.
extern "C" int asr_ctc_beam_search_ctx(const float* logits, int64_t ld, const int32_t* input_lengths, int B, int T, int V, int W, int C,
                                       int nbest, int blank, float* workspace, int64_t workspace_floats, int32_t* ids, int32_t* lengths,
                                       float* scores, const uint64_t* ng_keys, const float* ng_vals, int64_t ng_capacity,
                                       int ng_max_probe, int ng_order, int bos, int eos, float alpha, float beta, float* lm,
                                       const uint64_t* cx_keys, const int32_t* cx_vals, int64_t cx_capacity, int cx_max_probe,
                                       const int32_t* cx_hold, int cx_states, float gamma, int32_t* credit, hipStream_t s) {
  ASR_CHECK_ARG(lm && credit);
  BeamCtx bias{CtxTable{}, gamma, credit};
  int rc = beam_ctx_table(cx_keys, cx_vals, cx_capacity, cx_max_probe, cx_hold, cx_states, V, &bias.tab);
  if (rc != ASR_OK) return rc;
  if (!ng_keys)
    return beam_search<false, true>(logits, ld, input_lengths, B, T, V, W, C, nbest, blank, workspace, workspace_floats, ids, lengths,
                                    scores, BeamLm{beam_no_ngram(), 0, -1, 0.f, beta, lm}, bias, s);
  NgramTable tab;
  rc = beam_ngram_table(ng_keys, ng_vals, ng_capacity, ng_max_probe, ng_order, bos, eos, V, &tab);
  if (rc != ASR_OK) return rc;
  return beam_search<true, true>(logits, ld, input_lengths, B, T, V, W, C, nbest, blank, workspace, workspace_floats, ids, lengths,
                                 scores, BeamLm{tab, bos, eos, alpha, beta, lm}, bias, s);
}
