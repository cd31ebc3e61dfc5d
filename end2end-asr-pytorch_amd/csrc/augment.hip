// Tempo / gain perturbation and noise injection of padded waveforms on the GPU (reference: utils/audio.py:35-61 and
// NoiseInjection, utils/data_loader.py:60-70,145-179, which shell out to sox).  The definition is DESIGN.md section 7:
//   tempo  WSOLA at sox's `tempo` defaults: segments of S samples, overlap O, search window `search`; segment k >= 1 starts at
//          w_k = floor(tempo * k * (S - O) + .5) of the stream fifo[j] = x[j - search/2]; its offset off_k is the first minimum
//          over i < search of sum_{j<O} (fifo[w_k + i + j] - tail[j])^2, then O crossfaded samples, then the S - 2O middle ones;
//          tail = the O samples after them.  Segment 0 outputs fifo[search/2 : search/2 + S - O].
//   gain   y = clamp(rint(w * m * 32768), -32768, 32767) / 32768 with m = float32(10^(gain/20)) (sox's 16-bit output, no dither)
//   noise  y += ((level * n) * E_y) / E_n over an n_out-sample crop of a clip of the int16 bank, read cyclically; E = RMS in fp64
//          rounded to fp32; skipped when E_n == 0.
// One 256-thread workgroup per utterance; the WSOLA chain is sequential across segments (off_k needs segment k-1's tail), but the
// window starts are known in advance, so the next segment's window is loaded into registers while the current one is searched.
// Every f32 operation of the search, crossfade, gain and mix is separately rounded: contraction into FMA is off in this file (the
// library is built with hipcc's default -ffp-contract=fast); tests/test_augment_host.py checks the emitted code: the only f32 FMAs
// left are those of the correctly rounded division sequences (v_div_scale .. v_div_fixup).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPrefetch = 8;        // registers per lane for the next window: windows up to 2048 samples (S + search at <= 21 kHz)

// params row (double[8]): tempo (<= 0: no tempo / gain, the waveform passes through), m, noise clip index (< 0: none), crop start
// sample, noise level, n_out, unused x2
struct AugParams {
  double tempo;
  float m, level;
  int64_t clip, start;
  int n_out;
};

__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// first index of the minimum over the workgroup: (value, index) pairs, ties to the smaller index
__device__ __forceinline__ int block_argmin(float v, int i, float* redv, int* redi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { redv[wave] = v; redi[wave] = i; }
  __syncthreads();
  float bv = redv[0];
  int bi = redi[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) {
    if (redv[w] < bv || (redv[w] == bv && redi[w] < bi)) { bv = redv[w]; bi = redi[w]; }
  }
  return bi;
}

__device__ __forceinline__ float quantize16(float v, float m) {
  float q = rintf((v * m) * 32768.f);
  q = fminf(fmaxf(q, -32768.f), 32767.f);
  return q * (1.f / 32768.f);
}

__global__ __launch_bounds__(kThreads) void augment_wave_kernel(
    const float* __restrict__ wav, int64_t wav_stride, const int32_t* __restrict__ lens, const double* __restrict__ params,
    const int16_t* __restrict__ bank, const int64_t* __restrict__ bank_off, const int64_t* __restrict__ bank_len, int nclips,
    float* __restrict__ out, int64_t out_stride, int32_t* __restrict__ offsets, int64_t off_stride, int S, int search, int O) {
  extern __shared__ float smem[];
  __shared__ double red_d[kThreads / 64];
  __shared__ float red_v[kThreads / 64];
  __shared__ int red_i[kThreads / 64];

  const int b = blockIdx.x, tid = threadIdx.x;
  const double* pr = params + (int64_t)b * 8;
  AugParams p;
  p.tempo = pr[0];
  p.m = (float)pr[1];
  p.clip = (int64_t)pr[2];
  p.start = (int64_t)pr[3];
  p.level = (float)pr[4];
  p.n_out = (int)pr[5];
  const int L = min((int64_t)lens[b], wav_stride);
  const int n_out = (int)min((int64_t)max(p.n_out, 0), out_stride);
  const float* x = wav + (int64_t)b * wav_stride;
  float* y = out + (int64_t)b * out_stride;
  double acc = 0.0;

  if (p.tempo > 0.0) {
    const int half = search / 2, SO = S - O;
    const int Wn = (search + S + 3) & ~3;
    // windows at smem[0, Wn) / [Wn, 2 Wn), tails at [2 Wn, 2 Wn + O) / [2 Wn + O, 2 Wn + 2 O): plain offsets from the __shared__
    // symbol (an array of pointers indexed by the segment's parity turns them into generic pointers: flat loads)
    float* const tails = smem + 2 * Wn;
    const float inv_o = 1.f / (float)O;
    // fifo[j] = x[j - half] inside [0, L), else 0
    auto fetch = [&](int64_t j) -> float {
      const int64_t s = j - half;
      return (s >= 0 && s < L) ? x[s] : 0.f;
    };
    auto start_of = [&](int k) -> int64_t { return (int64_t)floor(p.tempo * (double)k * (double)SO + 0.5); };
    const int nseg = (n_out + SO - 1) / SO;
    for (int t = tid; t < Wn; t += kThreads) smem[t] = fetch(t);
    __syncthreads();
    for (int k = 0; k < nseg; ++k) {
      const int cur = k & 1;
      const bool more = k + 1 < nseg;
      const int64_t wn = more ? start_of(k + 1) : 0;
      float pf[kPrefetch];
#pragma unroll
      for (int r = 0; r < kPrefetch; ++r) {
        const int t = tid + r * kThreads;
        pf[r] = (more && t < Wn) ? fetch(wn + t) : 0.f;
      }
      const float* w = smem + cur * Wn;
      const float* tl = tails + cur * O;
      int off = half;
      if (k > 0) {
        float best = INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < search; i += kThreads) {
          // sequential in j (the definition's order), the LDS reads of the next 8 j issued before the arithmetic of these 8
          // (O is a multiple of 8)
          float s = 0.f;
          const float* c = w + i;
          float cv[8], tv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) { cv[u] = c[u]; tv[u] = tl[u]; }
          for (int j = 0; j < O; j += 8) {
            float cn[8], tn[8];
            const int jn = j + 8 < O ? j + 8 : j;
#pragma unroll
            for (int u = 0; u < 8; ++u) { cn[u] = c[jn + u]; tn[u] = tl[jn + u]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const float d = cv[u] - tv[u];
              s = s + d * d;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { cv[u] = cn[u]; tv[u] = tn[u]; }
          }
          if (s < best) { best = s; bi = i; }
        }
        off = block_argmin(best, bi, red_v, red_i);
      }
      const int64_t base = (int64_t)k * SO;
      for (int t = tid; t < SO && base + t < n_out; t += kThreads) {
        float v = w[off + t];
        if (k > 0 && t < O) {
          const float f = inv_o * (float)t;
          v = tl[t] * (1.f - f) + v * f;
        }
        const float q = quantize16(v, p.m);
        y[base + t] = q;
        acc += (double)q * (double)q;
      }
      float* nt = tails + (cur ^ 1) * O;
      for (int t = tid; t < O; t += kThreads) nt[t] = w[off + SO + t];
      if (offsets != nullptr && tid == 0) offsets[(int64_t)b * off_stride + k] = off;
      if (more) {
        float* nw = smem + (cur ^ 1) * Wn;
#pragma unroll
        for (int r = 0; r < kPrefetch; ++r) {
          const int t = tid + r * kThreads;
          if (t < Wn) nw[t] = pf[r];
        }
        for (int t = tid + kPrefetch * kThreads; t < Wn; t += kThreads) nw[t] = fetch(wn + t);
      }
      __syncthreads();
    }
  } else {
    for (int t = tid; t < n_out; t += kThreads) {
      const float v = t < L ? x[t] : 0.f;
      y[t] = v;
      acc += (double)v * (double)v;
    }
  }

  if (p.clip < 0 || p.clip >= nclips || n_out == 0) return;
  const int64_t clen64 = bank_len[p.clip];
  if (clen64 <= 0 || clen64 > 0x7fffffff) return;
  // the crop, read cyclically: sample t is clip[(start + t) mod clen]; lane positions advance by kThreads mod clen per step
  // (32-bit remainders: a 64-bit one expands into f32 reciprocal code)
  const unsigned clen = (unsigned)clen64;
  const int16_t* nz = bank + bank_off[p.clip];
  const unsigned st = (p.start < 0 || p.start > 0x7fffffff) ? 0u : (unsigned)p.start % clen;
  const unsigned r0 = (unsigned)(((uint64_t)st + (unsigned)tid) % clen), step = (unsigned)kThreads % clen;
  auto next = [&](unsigned r) { r += step; return r >= clen ? r - clen : r; };
  const float ey = (float)sqrt(block_sum_f64(acc, red_d) / (double)n_out);
  double an = 0.0;
  unsigned r = r0;
  for (int t = tid; t < n_out; t += kThreads, r = next(r)) {
    const float n = (float)nz[r] * (1.f / 32768.f);
    an += (double)n * (double)n;
  }
  const float en = (float)sqrt(block_sum_f64(an, red_d) / (double)n_out);
  if (en == 0.f) return;
  r = r0;
  for (int t = tid; t < n_out; t += kThreads, r = next(r)) {
    const float n = (float)nz[r] * (1.f / 32768.f);
    y[t] = y[t] + ((p.level * n) * ey) / en;
  }
}

}  // namespace

extern "C" int asr_augment_wave(const float* wav, int64_t wav_stride, const int32_t* lens, const double* params, const int16_t* bank,
                                const int64_t* bank_off, const int64_t* bank_len, int nclips, float* out, int64_t out_stride,
                                int32_t* offsets, int64_t off_stride, int B, int S, int search, int O, hipStream_t stream) {
  ASR_CHECK_ARG(wav && lens && params && out && B >= 0 && wav_stride >= 0 && out_stride >= 0 && nclips >= 0);
  ASR_CHECK_ARG(S > 0 && search > 0 && O > 0 && 2 * O <= S);
  ASR_CHECK_ARG(nclips == 0 || (bank && bank_off && bank_len));
  if (B == 0) return ASR_OK;
  const int Wn = (search + S + 3) & ~3;
  const size_t lds = (size_t)(2 * Wn + 2 * O) * sizeof(float);
  if (lds > 64 * 1024) return ASR_EINVAL;
  AsrProfScope prof(ASR_OP_LAYOUT, stream);
  return asr_launch<augment_wave_kernel>(dim3(B), dim3(kThreads), lds, stream, wav, wav_stride, lens, params, bank, bank_off, bank_len, nclips,
                                         out, out_stride, offsets, off_stride, S, search, O);
}
