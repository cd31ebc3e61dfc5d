// CTC prefix scorer for joint CTC / attention beam search (Watanabe et al. 2017, "Hybrid CTC/attention architecture for end-to-end
// speech recognition", algorithm 2).  lp[b,t,v] = log-softmax of the encoder's CTC logits, blank = 0, T_b = frames of utterance b.
//
// A hypothesis row with prefix g carries, for every frame t < T_b,
//   r_n[t] = log p(all alignments of g over frames 0..t that end in a non-blank),   r_b[t] = the same, ending in a blank
// (state (R,T,2): the pair of a frame is one 8-byte element).  g = <sos>: r_n = -inf, r_b[t] = sum_{tau <= t} lp[tau, blank].
//
// Extension of g by a label c (neither blank, SOS nor EOS), psi' = log p(g.c as a PREFIX):
//   phi[t]    = r_b[t] if c == last(g) else logaddexp(r_n[t], r_b[t])
//   r_n'[0]   = lp[0,c] if g is empty else -inf;   r_b'[0] = -inf;   psi' = r_n'[0]
//   r_n'[t]   = logaddexp(r_n'[t-1], phi[t-1]) + lp[t,c]
//   r_b'[t]   = logaddexp(r_n'[t-1], r_b'[t-1]) + lp[t,blank]
//   psi'      = logaddexp(psi', phi[t-1] + lp[t,c])                                   t = 1 .. T_b - 1
// c == EOS: psi' = logaddexp(r_n[T_b-1], r_b[T_b-1]) (the complete sequence g); c blank / SOS / out of range: psi' = -inf; both leave
// an all -inf state.  A prefix that does not fit into T_b frames comes out as -inf, never NaN (every log-add is -inf safe).
//
// The recursion is serial in t and independent per (row, candidate): R * K is a few hundred to a few thousand chains of T_b dependent
// log-adds, so the launch is latency bound.  One lane per (row, candidate), the K lanes of a row adjacent: the parent's (r_n, r_b)[t-1]
// and lp[t, blank] are one address per row (broadcast reads), lp[t, c] is one gather per lane; the three reads of frame t + 1 are issued
// before the log-add chain of frame t.  New states are written t-innermost per (row, candidate), (R,K,T,2); frames >= T_b are neither
// read nor written.  Selection of the survivors is an index_select on the device (asr_hip/decode.py).
#include "ctc_common.h"

namespace {

constexpr int PREFIX_K_MAX = 16;      // = TOPK_MAX of ce.hip: the candidates are asr_logsoftmax_topk's

__device__ __forceinline__ int prefix_frames(const int32_t* frames, int u, int B, int T) {
  if (u < 0 || u >= B) return 0;
  const int n = frames[u];
  return n < 0 ? 0 : (n > T ? T : n);
}

// one wave per row: lp[row, v] = logits[row, v] - lse[row]
__global__ __launch_bounds__(256) void ctc_prefix_lp_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ lse,
                                                            int64_t rows, int V, float* __restrict__ lp) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* x = logits + row * ld;
  float* y = lp + row * V;
  const float l = lse[row];
  for (int v = lane; v < V; v += 64) y[v] = x[v] - l;
}

// one lane per hypothesis row: the state of the empty prefix (a running sum in frame order, like the recursion itself)
__global__ __launch_bounds__(64) void ctc_prefix_init_kernel(const float* __restrict__ lp, const int32_t* __restrict__ frames,
                                                             const int32_t* __restrict__ row_utt, int B, int T, int V, int R, int blank,
                                                             float2* __restrict__ state) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int u = row_utt[r];
  const int Tb = prefix_frames(frames, u, B, T);
  float2* st = state + (int64_t)r * T;
  const float* lb = lp + (int64_t)(Tb > 0 ? u : 0) * T * V + blank;
  float s = 0.f;
  for (int t = 0; t < Tb; ++t) {
    s += lb[(int64_t)t * V];
    st[t] = make_float2(NEG_INF, s);
  }
  for (int t = Tb; t < T; ++t) st[t] = make_float2(NEG_INF, NEG_INF);
}

// one lane per (row, candidate)
__global__ __launch_bounds__(64) void ctc_prefix_step_kernel(const float* __restrict__ lp, const int32_t* __restrict__ frames,
                                                             const float2* __restrict__ state, const int32_t* __restrict__ row_utt,
                                                             const int64_t* __restrict__ last, const int32_t* __restrict__ first,
                                                             const int64_t* __restrict__ cand, int B, int T, int V, int R, int K, int blank,
                                                             int sos, int eos, float* __restrict__ psi, float2* __restrict__ out) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= R * K) return;
  const int r = g / K;
  const int u = row_utt[r];
  const int Tb = prefix_frames(frames, u, B, T);
  const int64_t c = cand[g];
  const bool empty = first[r] != 0;
  if (Tb == 0) {                            // no frames: only the empty sequence has any probability
    psi[g] = (c == eos && empty) ? 0.f : NEG_INF;
    return;
  }
  const float2* st = state + (int64_t)r * T;
  float2* o = out + (int64_t)g * T;
  if (c == eos || c < 0 || c >= V || c == blank || c == sos) {
    float p = NEG_INF;
    if (c == eos) {
      const float2 e = st[Tb - 1];
      p = lae2(e.x, e.y);
    }
    psi[g] = p;
    for (int t = 0; t < Tb; ++t) o[t] = make_float2(NEG_INF, NEG_INF);
    return;
  }
  const float* lc = lp + (int64_t)u * T * V + c;
  const float* lb = lp + (int64_t)u * T * V + blank;
  const bool same = c == last[r];
  float rn = empty ? lc[0] : NEG_INF, rb = NEG_INF, ps = rn;
  o[0] = make_float2(rn, rb);
  float2 s = st[0];                         // the parent's frame t - 1
  float pc = 0.f, pb = 0.f;                 // lp[t, c], lp[t, blank]
  if (Tb > 1) {
    pc = lc[V];
    pb = lb[V];
  }
  for (int t = 1; t < Tb; ++t) {
    float2 s_n = s;
    float pc_n = 0.f, pb_n = 0.f;
    if (t + 1 < Tb) {                       // frame t + 1's reads, in flight under the log-adds of frame t
      s_n = st[t];
      pc_n = lc[(int64_t)(t + 1) * V];
      pb_n = lb[(int64_t)(t + 1) * V];
    }
    const float phi = same ? s.y : lae2(s.x, s.y);
    const float nrn = lae2(rn, phi) + pc;
    const float nrb = lae2(rn, rb) + pb;
    ps = lae2(ps, phi + pc);
    rn = nrn;
    rb = nrb;
    o[t] = make_float2(rn, rb);
    s = s_n;
    pc = pc_n;
    pb = pb_n;
  }
  psi[g] = ps;
}

}  // namespace

extern "C" int asr_ctc_prefix_init(const float* logits, int64_t ld, const int32_t* frames, const int32_t* row_utt, int B, int T, int V,
                                   int R, int blank, float* lse, float* lp, float* state, hipStream_t s) {
  ASR_CHECK_ARG(logits && frames && row_utt && lse && lp && state);
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && R > 0 && ld >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG((((uintptr_t)state) & 7) == 0);
  const int64_t rows = (int64_t)B * T;
  AsrProfScope prof(ASR_OP_CE, s);
  hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, ld, rows, V, lse);
  ASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_prefix_lp_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, ld, lse, rows, V, lp);
  ASR_LAUNCH_CHECK();
  hipLaunchKernelGGL(ctc_prefix_init_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, s, lp, frames, row_utt, B, T, V, R, blank,
                     reinterpret_cast<float2*>(state));
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

extern "C" int asr_ctc_prefix_step(const float* lp, const int32_t* frames, const float* state, const int32_t* row_utt, const int64_t* last,
                                   const int32_t* first, const int64_t* cand, int B, int T, int V, int R, int K, int blank, int sos, int eos,
                                   float* psi, float* new_state, hipStream_t s) {
  ASR_CHECK_ARG(lp && frames && state && row_utt && last && first && cand && psi && new_state);
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && R > 0 && K > 0 && blank >= 0 && blank < V);
  ASR_CHECK_ARG((((uintptr_t)state) & 7) == 0 && (((uintptr_t)new_state) & 7) == 0);
  if (K > PREFIX_K_MAX) return ASR_EUNSUPPORTED;
  ASR_CHECK_ARG((int64_t)R * K < (1ll << 31));
  AsrProfScope prof(ASR_OP_CE, s);
  hipLaunchKernelGGL(ctc_prefix_step_kernel, dim3((unsigned)(((int64_t)R * K + 63) / 64)), dim3(64), 0, s, lp, frames,
                     reinterpret_cast<const float2*>(state), row_utt, last, first, cand, B, T, V, R, K, blank, sos, eos, psi,
                     reinterpret_cast<float2*>(new_state));
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}
