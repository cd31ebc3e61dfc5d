// CTC forced alignment: the best (Viterbi) path of a label sequence through the posteriors of the encoder's CTC head, with the frames,
// the log-probability of every label and the log-probability of the whole path.  asr_ctc_fwd (ctc.hip) SUMS over the alignments of the
// same lattice and keeps no back-pointers; this kernel keeps the maximum and walks back.
//
//   l' = blank-interleaved target, S_b = 2 L_b + 1, x_t(s) = logits[b, t, l'_s]                                 (the RAW logit)
//   v(0, s) = x_0(s) for s in {0, 1}, else -inf
//   v(t, s) = best + x_t(s),   best among v(t-1, s), v(t-1, s-1), [v(t-1, s-2) if l'_s != blank and l'_s != l'_{s-2}]
//   final state = S_b - 1 unless v(T_b-1, S_b-2) is strictly greater;   score_b = v(T_b-1, final) - sum_{t < T_b} lse[t]
//
// Three rules make the path a function of fp32 adds and comparisons only (tests/ctc_align_reference.py restates them in NumPy float32 and
// is compared bit for bit):
//   * the recursion runs on the raw logits: every path takes exactly one emission per frame, so subtracting lse[t] from a whole frame
//     cannot change an arg-max.  lse (ctc_lse_kernel) enters score and lab_score only;
//   * compare first, then ONE fp32 add: the predecessor is selected among the previous values and the logit is added to the winner;
//   * ties: a predecessor replaces the current best only if strictly greater, tried in the order offset 0, 1, 2 (stay, advance, skip).
//
// One workgroup per utterance walks time, 16 frames at a go: the emissions x_t(s) of the 16 frames are gathered into LDS with independent
// loads (the gather is the only global read of the walk, so its latency is paid once per 16 frames, not once per frame), then the 16
// dependent steps run out of LDS.  A step leaves one 2-bit back-pointer per state; the 16 of a state and a chunk are one 32-bit word that
// only the thread owning the state touches.  When the words of the whole utterance fit into LDS beside the rest (they do at the
// project's sizes: T' 625, S 601 is 141 KB) the back-walk never leaves LDS; otherwise each chunk's words go to a caller-owned workspace
// and come back chunk by chunk.  The back-walk is one lane following T_b dependent LDS reads; the label spans and scores are then written
// in parallel over frames and labels.
#include "ctc_common.h"      // NEG_INF, ctc_lse_kernel

namespace {

constexpr int ALIGN_CHUNK = 16;                  // frames per emission gather = 2-bit back-pointers per 32-bit word
constexpr size_t ALIGN_LDS_MAX = 160 * 1024 - 64;     // LDS of a gfx950 CU (one workgroup may hold all of it) less the static words below

// LDS words of a launch: v rows [2][S] | labels [S] | path [T] | emissions [16][S] | back-pointer words ([S] per chunk kept)
inline int64_t align_lds_words(int T, int S, int chunks_kept) { return (int64_t)(3 + ALIGN_CHUNK + chunks_kept) * S + T; }
__host__ __device__ inline int align_chunks(int T) { return (T + ALIGN_CHUNK - 1) / ALIGN_CHUNK; }
inline bool align_fits_lds(int T, int S) { return align_lds_words(T, S, align_chunks(T)) * 4 <= (int64_t)ALIGN_LDS_MAX; }

// WS: the back-pointer words live in `ws` (B, chunks, S) and pass through one [S] LDS buffer; else all of them stay in LDS.
template <bool WS>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ lse,
                                                        const int64_t* __restrict__ targets, int Lmax,
                                                        const int32_t* __restrict__ in_len, const int32_t* __restrict__ tg_len, int T,
                                                        int V, int S, int blank, uint32_t* __restrict__ ws, int32_t* __restrict__ path,
                                                        int32_t* __restrict__ start, int32_t* __restrict__ end,
                                                        float* __restrict__ lab_score, float* __restrict__ score) {
  extern __shared__ float sh[];
  __shared__ int flag[2];            // [0] a label that is blank or outside [0, V);  [1] the final state (-1: infeasible)
  __shared__ float red[4];
  float* prev = sh;
  float* cur = sh + S;
  int* lab = reinterpret_cast<int*>(sh + 2 * S);
  int* pth = lab + S;                                              // [T] the path, then read by every thread
  float* em = reinterpret_cast<float*>(pth + T);                   // [16][S]; after the walk: label starts [Lmax] | ends [Lmax]
  uint32_t* bp = reinterpret_cast<uint32_t*>(em + ALIGN_CHUNK * S);
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  int Tb = in_len[b];
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  int Lb = tg_len[b];
  Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
  const int Sb = 2 * Lb + 1;
  const int nch = (Tb + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
  int32_t* path_b = path + (int64_t)b * T;
  int32_t* start_b = start + (int64_t)b * Lmax;
  int32_t* end_b = end + (int64_t)b * Lmax;
  float* ls_b = lab_score + (int64_t)b * Lmax;
  if (tid < 2) flag[tid] = tid == 0 ? 0 : -1;
  __syncthreads();
  for (int s = tid; s < Sb; s += 256) {
    int v = blank;
    if (s & 1) {
      const int64_t id = targets[(int64_t)b * Lmax + (s >> 1)];
      if (id < 0 || id >= V || id == blank) flag[0] = 1;           // (every writer writes the same value)
      else v = (int)id;
    }
    lab[s] = v;
  }
  __syncthreads();
  const bool walk = flag[0] == 0 && Tb > 0;
  float vend = Tb == 0 && Lb == 0 && flag[0] == 0 ? 0.f : NEG_INF;          // no frames: only the empty target, with probability 1
  if (walk) {
    const float* lg = logits + (int64_t)b * T * ld;
    uint32_t* ws_b = WS ? ws + (int64_t)b * align_chunks(T) * S : nullptr;
    for (int c = 0; c < nch; ++c) {
      const int t0 = c * ALIGN_CHUNK;
      const int n = Tb - t0 < ALIGN_CHUNK ? Tb - t0 : ALIGN_CHUNK;
      for (int s = tid; s < Sb; s += 256) {
        const float* col = lg + (int64_t)t0 * ld + lab[s];
#pragma unroll
        for (int i = 0; i < ALIGN_CHUNK; ++i)
          if (i < n) em[i * S + s] = col[(int64_t)i * ld];
      }
      __syncthreads();
      uint32_t* bw = WS ? bp : bp + (int64_t)c * S;
      for (int i = 0; i < n; ++i) {
        for (int s = tid; s < Sb; s += 256) {
          const float x = em[i * S + s];
          float v;
          uint32_t w = 0;
          if (t0 + i == 0) {
            v = s < 2 ? x : NEG_INF;
          } else {
            float best = prev[s];
            uint32_t code = 0;
            if (s >= 1) {
              const float a1 = prev[s - 1];
              if (a1 > best) { best = a1; code = 1; }
            }
            if (s >= 2 && (s & 1) && lab[s] != lab[s - 2]) {        // (an odd state holds a label, never the blank)
              const float a2 = prev[s - 2];
              if (a2 > best) { best = a2; code = 2; }
            }
            v = best + x;
            w = (i == 0 ? 0u : bw[s]) | (code << (2 * i));
          }
          cur[s] = v;
          bw[s] = w;
        }
        __syncthreads();
        float* tmp = prev; prev = cur; cur = tmp;
      }
      if (WS)
        for (int s = tid; s < Sb; s += 256) ws_b[(int64_t)c * S + s] = bw[s];      // (its own word: no barrier needed)
    }
    if (tid == 0) {
      int sf = Sb - 1;
      float a = prev[sf];
      if (Sb >= 2 && prev[Sb - 2] > a) { a = prev[Sb - 2]; sf = Sb - 2; }
      red[0] = a;
      flag[1] = a > NEG_INF ? sf : -1;
    }
    __syncthreads();
    vend = red[0];
  }
  const int sf = walk ? flag[1] : -1;
  const bool feasible = vend > NEG_INF;
  __syncthreads();                                   // red[0] is reused below
  if (walk && sf >= 0) {
    // the back-walk: one lane, T_b dependent LDS reads
    int s = sf;
    for (int c = nch - 1; c >= 0; --c) {
      const int t0 = c * ALIGN_CHUNK;
      const int n = Tb - t0 < ALIGN_CHUNK ? Tb - t0 : ALIGN_CHUNK;
      const uint32_t* bw = WS ? bp : bp + (int64_t)c * S;
      if (WS) {
        const uint32_t* ws_b = ws + (int64_t)b * align_chunks(T) * S;
        for (int k = tid; k < Sb; k += 256) bp[k] = ws_b[(int64_t)c * S + k];
        __syncthreads();
      }
      if (tid == 0) {
        for (int i = n - 1; i >= 0; --i) {
          pth[t0 + i] = s;
          s -= (int)((bw[s] >> (2 * i)) & 3u);
        }
      }
      if (WS) __syncthreads();
    }
    __syncthreads();
  }
  // outputs.  path and the label spans, parallel over frames
  int* lstart = reinterpret_cast<int*>(em);
  int* lend = lstart + Lmax;
  for (int t = tid; t < T; t += 256) {
    int s = -1;
    if (feasible && t < Tb) {
      s = pth[t];
      if (s & 1) {
        if (t == 0 || pth[t - 1] != s) lstart[s >> 1] = t;
        if (t == Tb - 1 || pth[t + 1] != s) lend[s >> 1] = t + 1;
      }
    }
    path_b[t] = s;
  }
  __syncthreads();
  // label scores, parallel over labels (a label's frames summed in frame order), and sum_t lse[t]
  for (int l = tid; l < Lmax; l += 256) {
    int a = -1, e = -1;
    float acc = 0.f;
    if (feasible && l < Lb) {
      a = lstart[l];
      e = lend[l];
      const float* col = logits + (int64_t)b * T * ld + lab[2 * l + 1];
      for (int t = a; t < e; ++t) acc += col[(int64_t)t * ld] - lse[(int64_t)b * T + t];
    }
    start_b[l] = a;
    end_b[l] = e;
    ls_b[l] = acc;
  }
  float sum = 0.f;
  if (feasible)
    for (int t = tid; t < Tb; t += 256) sum += lse[(int64_t)b * T + t];
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) score[b] = feasible ? vend - (red[0] + red[1] + red[2] + red[3]) : NEG_INF;
}

template <bool WS>
int align_launch(size_t lds, int B, hipStream_t s, const float* logits, int64_t ld, const float* lse, const int64_t* targets, int Lmax,
                 const int32_t* in_len, const int32_t* tg_len, int T, int V, int S, int blank, uint32_t* ws, int32_t* path, int32_t* start,
                 int32_t* end, float* lab_score, float* score) {
  // above the 48 KB every kernel has, the dynamic LDS size is asked for explicitly (up to 141 KB at the project's sizes); a refused grant
  // is an unsupported shape, not a failed launch
  if (lds > 48 * 1024 && asr_grant_lds<ctc_align_kernel<WS>>(lds) != hipSuccess) return ASR_EUNSUPPORTED;
  hipLaunchKernelGGL(ctc_align_kernel<WS>, dim3(B), dim3(256), lds, s, logits, ld, lse, targets, Lmax, in_len, tg_len, T, V, S, blank, ws,
                     path, start, end, lab_score, score);
  ASR_LAUNCH_CHECK();
  return ASR_OK;
}

}  // namespace

extern "C" int64_t asr_ctc_align_workspace(int B, int T, int Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 1) return 0;
  const int S = 2 * Lmax + 1;
  const int64_t bp = align_fits_lds(T, S) ? 0 : (int64_t)B * align_chunks(T) * S;
  return (int64_t)B * T + bp;                                      // row lse | back-pointer words (only when LDS cannot hold them)
}

extern "C" int asr_ctc_align(const float* logits, int64_t ld, const int64_t* targets, const int32_t* input_lengths,
                             const int32_t* target_lengths, int B, int T, int V, int Lmax, int blank, float* workspace,
                             int64_t workspace_floats, int32_t* path, int32_t* start, int32_t* end, float* lab_score, float* score,
                             hipStream_t s) {
  ASR_CHECK_ARG(logits && targets && input_lengths && target_lengths && workspace && path && start && end && lab_score && score);
  ASR_CHECK_ARG(B > 0 && T > 0 && V > 0 && Lmax >= 1 && Lmax < (1 << 29) && ld >= V && blank >= 0 && blank < V);
  ASR_CHECK_ARG(workspace_floats >= asr_ctc_align_workspace(B, T, Lmax));
  const int S = 2 * Lmax + 1;
  const bool in_lds = align_fits_lds(T, S);
  const int64_t words = align_lds_words(T, S, in_lds ? align_chunks(T) : 1);
  if (words * 4 > (int64_t)ALIGN_LDS_MAX) return ASR_EUNSUPPORTED;
  const size_t lds = (size_t)words * 4;
  float* lse = workspace;
  uint32_t* ws = reinterpret_cast<uint32_t*>(workspace + (int64_t)B * T);
  const int64_t rows = (int64_t)B * T;
  AsrProfScope prof(ASR_OP_CE, s);
  hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, ld, rows, V, lse);
  ASR_LAUNCH_CHECK();
  if (in_lds)
    return align_launch<false>(lds, B, s, logits, ld, lse, targets, Lmax, input_lengths, target_lengths, T, V, S, blank, nullptr, path, start,
                               end, lab_score, score);
  return align_launch<true>(lds, B, s, logits, ld, lse, targets, Lmax, input_lengths, target_lengths, T, V, S, blank, ws, path, start, end,
                            lab_score, score);
}
