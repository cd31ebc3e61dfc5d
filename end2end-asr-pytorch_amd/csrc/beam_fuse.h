// What the fused arms of the beam searches (csrc/ctc_beam.hip, csrc/rnnt_beam.hip) have in common, stated once: the state a hypothesis
// carries for the n-gram LM and the phrase list, the one lookup of a step, and the entries' table checks.
// BeamExt is a function of the hypothesis' label sequence alone -- lm = the fp32 sum of q (csrc/ngram.h) over its labels, added in label
// order; len = their number; ctx = the key of the last order - 1 symbols of [bos] + labels; cst, cnt = state and credit of the phrase
// automaton (csrc/context.h) -- so a sequence pruned and created again gets the same bits, and whichever entry survives a merge holds
// the right ones.  LM / CTX say which tables there are: without an LM lm stays 0.f and ctx 0, without phrases cst and cnt stay 0; len is
// always counted.  The searches keep the state as five parallel arrays in LDS (their rank loops read single fields across entries);
// BeamExtSoa is the view of them, and get / put touch only the arrays the arm instantiates.  The transducer search moves entries between
// its lists (C_s, D, A) field by field through the view's pointers instead: get / put measured slower there
// (profiles/beam_fuse_refactor_isa.txt).
// What differs between the searches by definition stays in their files: what the bonus is added to (fp32 tot in CTC, the fp64 score in
// the transducer), where q(ctx, eos) enters the final key, a missing entry's lm and credit, and which entry keeps its state in a merge.
// Include order: csrc/lse.h turns multiply-add contraction off for the rest of the file that includes it.  csrc/rnnt_beam.hip includes
// it BEFORE this header and csrc/ctc_beam.hip not at all, so alpha * lm + beta * len (csrc/beam_bonus.h) may contract in the CTC kernel
// and does not in the transducer's; the tests pin both.  Neither file's include order relative to lse.h may change.
#pragma once
#include "beam_bonus.h"      // beam_bonus
#include "context.h"         // CtxTable, ctx_probe, ctx_finish
#include "ngram.h"           // NgramTable, ngram_query, ngram_shift

namespace {

struct BeamExt { float lm; int len; uint64_t ctx; int cst, cnt; };

// the empty sequence: lm 0, len 0, context [bos], state eps, credit 0
template <bool LM>
__device__ __forceinline__ BeamExt beam_ext_root(const NgramTable& ng, int bos) {
  BeamExt e{0.f, 0, 0, 0, 0};
  if constexpr (LM) e.ctx = ngram_shift(0, bos, ng.order);
  return e;
}

// h extended by `label`: the step's one lookup.  Both structures' first probes are in flight before either is consumed
template <bool LM, bool CTX>
__device__ __forceinline__ BeamExt beam_ext_extend(const NgramTable& ng, const CtxTable& cx, const BeamExt& h, int label) {
  BeamExt e{0.f, 0, 0, 0, 0};
  CtxProbe probe;
  if constexpr (CTX) probe = ctx_probe(cx, h.cst, label);
  if constexpr (LM) {
    e.lm = h.lm + ngram_query(ng, h.ctx, label);
    e.ctx = ngram_shift(h.ctx, label, ng.order);
  }
  e.len = h.len + 1;
  if constexpr (CTX) {
    const int2 tr = ctx_finish(cx, probe);
    e.cst = tr.x;
    e.cnt = h.cnt + tr.y;
  }
  return e;
}

// what the credit is worth at the end of the utterance: the labels of an unfinished phrase are taken back
__device__ __forceinline__ int beam_ext_earned(const CtxTable& cx, const BeamExt& e) {
  return e.cnt - cx.hold[e.cst >= 0 && e.cst < cx.states ? e.cst : 0];
}

template <bool LM, bool CTX>
__device__ __forceinline__ float beam_ext_bonus(float alpha, float beta, float gamma, const BeamExt& e) {
  return beam_bonus<LM, CTX>(alpha, beta, gamma, e.lm, e.len, e.cnt);
}

struct BeamExtSoa {
  float* lm; int* len; uint64_t* ctx; int *cst, *cnt;
  template <bool LM, bool CTX>
  __device__ __forceinline__ BeamExt get(int i) const {
    BeamExt e{0.f, 0, 0, 0, 0};
    if constexpr (LM) { e.lm = lm[i]; e.ctx = ctx[i]; }
    e.len = len[i];
    if constexpr (CTX) { e.cst = cst[i]; e.cnt = cnt[i]; }
    return e;
  }
  template <bool LM, bool CTX>
  __device__ __forceinline__ void put(int i, const BeamExt& e) const {
    if constexpr (LM) { lm[i] = e.lm; ctx[i] = e.ctx; }
    len[i] = e.len;
    if constexpr (CTX) { cst[i] = e.cst; cnt[i] = e.cnt; }
  }
};

// (The n-best tail stays written out in each kernel: as a shared function it rescheduled the PLAIN arms, whose text is held fixed.)

// ---- the host side of the entries: the checks of a table's arguments and the table.  The entries test their output pointers first;
// every check up to the label-range refusal returns ASR_EINVAL and CTX_MAX_ID == NGRAM_MAX_ID, so the order decides no return code
inline int beam_ngram_table(const uint64_t* keys, const float* vals, int64_t capacity, int max_probe, int order, int bos, int eos, int V,
                            NgramTable* t) {
  const int rc = ngram_check_table(keys, vals, capacity, max_probe, order);
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG(bos >= 0 && bos < V && eos >= -1 && eos < V);
  if (V > NGRAM_MAX_ID + 1) return ASR_EUNSUPPORTED;          // ids + 1 in 16-bit key fields
  *t = NgramTable{keys, reinterpret_cast<const float2*>(vals), (uint32_t)(capacity - 1), max_probe, order};
  return ASR_OK;
}

inline int beam_ctx_table(const uint64_t* keys, const int32_t* vals, int64_t capacity, int max_probe, const int32_t* hold, int states, int V,
                          CtxTable* t) {
  const int rc = ctx_check_table(keys, vals, capacity, max_probe, hold, states);
  if (rc != ASR_OK) return rc;
  if (V > CTX_MAX_ID + 1) return ASR_EUNSUPPORTED;            // labels + 1 in a 16-bit key field
  *t = CtxTable{keys, reinterpret_cast<const int2*>(vals), hold, (uint32_t)(capacity - 1), max_probe, states};
  return ASR_OK;
}

inline NgramTable beam_no_ngram() { return NgramTable{nullptr, nullptr, 0, 1, 1}; }
inline CtxTable beam_no_ctx() { return CtxTable{nullptr, nullptr, nullptr, 0, 1, 1}; }      // (an arm without the table never reads it)

}  // namespace
