// Fused multi-head attention core (models/common_layers.py:211-225): the two C entry points, the argument marshalling, and THE DISPATCH.
// No kernel lives here.  attn_choose_fwd / attn_choose_bwd list the arms in order, each with its whole eligibility condition; the
// launchers they call (attention.h) only launch.
//   attention_generic.hip         fp32 / bf16, d in {16, 32, 64}, any strides: forward, delta (two forms), dQ, dK / dV, probability dump
//   attention_pp.hip              bf16, d = 64: long-sequence forward (32x32 MFMA, 3-deep LDS ring)
//   attention_d64_fwd.hip         bf16, d = 64: forward, 64 or 128 queries per workgroup
//   attention_d64_bwd.hip         bf16, d = 64: delta, dQ half, dK / dV half, both halves in one launch
//   attention_d64_bwd_fused.hip   bf16, d = 64: the whole backward of a (batch, head) in one workgroup, short key sequences
#include "attention_d64.h"

using namespace asr_attn;

namespace {

// ---- the thresholds of the dispatch, all of them
// Long-sequence forward (attention_pp.hip) from this many keys: round 3's ATTN_PP_MIN switch at its setting (the table of
// switches folded into constants); the kernel against the first generation: tools/ab/ab_attn_pp.py, profiles/r03_attention_pp_ab.txt.
constexpr int kPpMinKeys = 384;
// 64-query workgroups (NQ = 1) up to this many queries, 128-query ones (NQ = 2) above: measured at (32, 8, 200, 200), where the tile loop
// costs 2.1 us per 64-key tile with two waves per SIMD against 2.7 us for everything else in the launch; half the queries per wave
// doubles the waves per SIMD (attention_d64_fwd.hip has the whole note).
constexpr int kShortQueries = 256;
// One-pass backward (attention_d64_bwd_fused.hip) up to this many keys: 8 waves x 32 keys hold a whole head -- every attention of the
// benchmark model, T' = 200 / 100 (round 5; the two-half form recomputes S, the softmax and dP in both halves).
constexpr int kFusedMaxKeys = 256;
// ... with 16 keys per wave up to this many keys (the decoder's self-attention: every wave has live keys), 32 keys per wave above.
constexpr int kFusedNarrowKeys = 128;

// Which forward kernel a call gets.  Arms in order of preference; the first whose condition holds runs.
int attn_choose_fwd(const AttnArgs& p, int d, int dtype, hipStream_t s) {
  int rc;
  // bf16, d = 64, 16-byte rows, strides below 2^22, mask extent below 2^31 (fast_ok), and O rows that take the 8-byte stores of the d = 64
  // epilogues; everything else is the generic kernels'
  const bool d64 = fast_ok(p, d, dtype) && aligned8(p.Out) && p.o_st % 4 == 0 && p.o_sb % 4 == 0;
  if (!d64)
    rc = attn_generic_fwd(p, d, dtype, s);
  // long sequences: the kernel knows key lengths only (no causal mask, no key-padding bytes) and stores 16-byte pieces of O and O32
  else if (!p.causal && !p.key_pad && p.Tk >= kPpMinKeys && aligned16(p.Out) && p.o_st % 8 == 0 && p.o_sb % 8 == 0 &&
           (!p.Out32 || aligned16(p.Out32)))
    rc = attn_pp_fwd(p, s);
  else
    rc = attn_d64_fwd(p, p.Tq <= kShortQueries ? 1 : 2, s);
  // the probability dump the reference returns, for whoever asked: one place, after any of the arms
  if (rc == ASR_OK && p.attn_out) rc = attn_probs(p, d, dtype, s);
  return rc;
}

// Which backward kernels a call gets: delta, dQ and dK / dV as p.parts asks (ops.attn_bwd asks for all three or, with delta handed in, for
// the last two; one half alone is a direct call of the entry point).
int attn_choose_bwd(const AttnArgs& p, int d, int dtype, hipStream_t s) {
  const bool delta = (p.parts & ASR_ATTN_DELTA) != 0, dq = (p.parts & ASR_ATTN_DQ) != 0, dkv = (p.parts & ASR_ATTN_DKV) != 0;
  int rc = ASR_OK;
  // bf16, d = 64 (fast_ok) with gradients and O that take 16-byte accesses
  if (fast_ok(p, d, dtype) && aligned16(p.dQ) && aligned16(p.dK) && aligned16(p.dV) && aligned16(p.O)) {
    if (delta) rc = attn_d64_delta(p, s);
    if (rc != ASR_OK) return rc;
    // both halves asked for and every key of a head fits one workgroup: one pass over the scores (ATTN_BWD_FUSED = 0 is the test hook
    // that takes the two-half launch instead)
    if (dq && dkv && p.Tk <= kFusedMaxKeys && asr_tuning("ATTN_BWD_FUSED", 1) != 0)
      return attn_d64_bwd_fused(p, p.Tk <= kFusedNarrowKeys ? 1 : 2, s);
    // both halves in one launch
    if (dq && dkv) return attn_d64_bwd_both(p, s);
    // one half alone
    if (dq) return attn_d64_bwd_dq(p, s);
    if (dkv) return attn_d64_bwd_dkv(p, s);
    return ASR_OK;
  }
  // generic.  fp32 is the parity mode: delta in the consistent form (one more pass over the keys; the kernel's note says why)
  if (delta) rc = dtype == ASR_F32 ? attn_generic_delta_consistent_f32(p, d, s) : attn_generic_delta_bf16(p, d, s);
  if (rc == ASR_OK && dq) rc = attn_generic_dq(p, d, dtype, s);
  if (rc == ASR_OK && dkv) rc = attn_generic_dkv(p, d, dtype, s);
  return rc;
}

int fill_common(AttnArgs& p, int B, int H, int Tq, int Tk, int d, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st,
                int64_t v_sb, int64_t v_st, int64_t o_sb, int64_t o_st, const int32_t* key_len, const uint8_t* key_pad,
                int64_t m_sb, int64_t m_sq, int causal, float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                int dtype) {
  ASR_CHECK_ARG(B >= 0 && H > 0 && Tq >= 0 && Tk >= 0 && d > 0 && dropout_p >= 0.f && dropout_p < 1.f);
  ASR_CHECK_ARG(dtype == ASR_F32 || dtype == ASR_BF16);
  p.B = B; p.H = H; p.Tq = Tq; p.Tk = Tk;
  p.q_sb = q_sb; p.q_st = q_st; p.k_sb = k_sb; p.k_st = k_st; p.v_sb = v_sb; p.v_st = v_st; p.o_sb = o_sb; p.o_st = o_st;
  p.key_len = key_len; p.key_pad = key_pad; p.m_sb = m_sb; p.m_sq = m_sq; p.causal = causal; p.scale = scale;
  // 16-bit dropout threshold; the rescale uses the QUANTISED probability so that E[dropout(x)] = x exactly
  p.thr = (uint32_t)(dropout_p * 65536.f + 0.5f);
  if (p.thr > 65535u) p.thr = 65535u;
  p.inv_keep = 1.f / (1.f - (float)p.thr / 65536.f); p.seed = seed; p.seed_dev = seed_dev;
  ASR_CHECK_ARG((int64_t)B * H * (Tq > 0 ? Tq : 1) < (int64_t)1 << 32);
  const int epc = dtype == ASR_F32 ? 4 : 8;
  p.vec = (q_sb % epc == 0) && (q_st % epc == 0) && (k_sb % epc == 0) && (k_st % epc == 0) && (v_sb % epc == 0) &&
          (v_st % epc == 0) && (o_sb % epc == 0) && (o_st % epc == 0);
  return ASR_OK;
}

}  // namespace

extern "C" int asr_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* o32, float* lse, float* attn_out, int B, int H,
                            int Tq, int Tk, int d, int64_t q_sb, int64_t q_st, int64_t k_sb, int64_t k_st, int64_t v_sb,
                            int64_t v_st, int64_t o_sb, int64_t o_st, const int32_t* key_len, const uint8_t* key_pad,
                            int64_t mask_sb, int64_t mask_sq, int causal, float scale, float dropout_p, uint64_t seed,
                            const uint64_t* seed_dev, int dtype, hipStream_t stream) {
  ASR_CHECK_ARG(Q && K && V && O && lse);
  AttnArgs p{};
  int rc = fill_common(p, B, H, Tq, Tk, d, q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st, key_len, key_pad, mask_sb, mask_sq, causal,
                       scale, dropout_p, seed, seed_dev, dtype);
  if (rc != ASR_OK) return rc;
  if (B == 0 || Tq == 0) return ASR_OK;
  p.Q = Q; p.K = K; p.V = V; p.Out = O; p.Out32 = o32; p.lse = lse; p.attn_out = attn_out;
  ASR_CHECK_ARG(!o32 || aligned16(o32));
  p.vec = p.vec && aligned16(Q) && aligned16(K) && aligned16(V);
  AsrProfScope prof(ASR_OP_ATTN_FWD, stream);
  return attn_choose_fwd(p, d, dtype, stream);
}

extern "C" int asr_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const float* o32, const void* dO, const float* lse,
                            float* delta, void* dQ, void* dK, void* dV, int B, int H, int Tq, int Tk, int d, int64_t q_sb,
                            int64_t q_st, int64_t k_sb, int64_t k_st, int64_t v_sb, int64_t v_st, int64_t o_sb, int64_t o_st,
                            const int32_t* key_len, const uint8_t* key_pad, int64_t mask_sb, int64_t mask_sq, int causal,
                            float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, int parts, int dtype,
                            hipStream_t stream) {
  ASR_CHECK_ARG(Q && K && V && O && dO && lse && delta && dQ && dK && dV);
  ASR_CHECK_ARG(parts > 0 && parts <= (ASR_ATTN_DELTA | ASR_ATTN_DQ | ASR_ATTN_DKV));
  AttnArgs p{};
  int rc = fill_common(p, B, H, Tq, Tk, d, q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st, key_len, key_pad, mask_sb, mask_sq, causal,
                       scale, dropout_p, seed, seed_dev, dtype);
  if (rc != ASR_OK) return rc;
  if (B == 0 || Tq == 0 || Tk == 0) return ASR_OK;
  p.Q = Q; p.K = K; p.V = V; p.O = O; p.O32 = o32; p.dO = dO; p.lse = const_cast<float*>(lse); p.delta = delta;
  p.dQ = dQ; p.dK = dK; p.dV = dV; p.parts = parts;
  p.vec = p.vec && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(dO);
  AsrProfScope prof(ASR_OP_ATTN_BWD, stream);
  return attn_choose_bwd(p, d, dtype, stream);
}
