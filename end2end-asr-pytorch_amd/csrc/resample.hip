// Speed perturbation of padded waveforms on the GPU: band-limited resampling by a rational factor num / den (no counterpart in the
// reference, which only has sox's `tempo`; Ko et al., Interspeech 2015).  The definition is DESIGN.md section 7:
//   output m of an utterance sits at input position m num / den = i_m + phi_m / den (64-bit integers, no floating-point positions);
//   y[m] = sum_{q < 2R} H[phi_m][q] x[i_m + q - R + 1], x = 0 outside [0, n): ONE fmaf chain in ascending q from +0.0, fp32;
//   H (den, 2R): the Hann-windowed sinc of the factor, computed in float64 on the host (utils/audio.py resample_table).
// Grid: (tiles of kTile consecutive outputs) x utterances, 256 threads.  A tile's input span -- kTile num / den + 2R samples -- is
// loaded once into LDS with 16-byte loads, zero filled outside [0, n); lane l then owns outputs l, l + 256, l + 512, l + 768 of the
// tile, so that one wave's LDS reads of a tap are ~num / den apart (neighbouring banks; four consecutive outputs per lane would put the
// lanes 4 num / den apart: a 4-way conflict on every tap) and its stores are one contiguous 256-byte run.  The taps come from the table
// through the cache: den x 2R floats, ~0.5 KB for the factors 0.9 / 1.1, at most 104 KB (den = 1000, R = 13).  Rows that are copied
// (num == den) and tiles behind n_out move 16 bytes per lane.  No atomics: the same inputs give the same bits.
#include "wave_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                          // outputs per lane
constexpr int kTile = ASR_RESAMPLE_TILE;         // outputs per workgroup
constexpr int kLds = 2304;                       // staged input samples: kTile * 2 + 2 * 13 + alignment (factors 0.5 .. 2); tests/test_gpu_frontend_golden.py repeats it
constexpr int kMaxDen = 1000;
static_assert(kTile == kThreads * kPer, "one tile is kPer outputs per lane");

struct ResamplePlan {                            // one row of `plan`, clamped: a bad row resamples nothing and is written as zeros
  int num, den, R, n_out;
  int64_t off;
  bool copy;
};

__device__ __forceinline__ ResamplePlan load_plan(const int32_t* __restrict__ pl, int64_t table_floats, int out_cols) {
  ResamplePlan p;
  p.num = pl[0];
  p.den = pl[1];
  p.R = pl[2];
  p.off = pl[3];
  p.n_out = min(max(pl[4], 0), out_cols);
  p.copy = p.num == p.den && p.num >= 1;
  const bool ok = p.copy || (p.num >= 1 && p.den >= 1 && p.den <= kMaxDen && p.R >= 1 && p.off >= 0 &&
                             p.off + (int64_t)p.den * 2 * (int64_t)p.R <= table_floats);
  if (!ok) p.n_out = 0;
  return p;
}

__global__ __launch_bounds__(kThreads) void resample_kernel(const float* __restrict__ wav, int64_t wav_stride,
                                                            const int32_t* __restrict__ lens, const int32_t* __restrict__ plan,
                                                            const float* __restrict__ table, int64_t table_floats,
                                                            float* __restrict__ out, int64_t out_stride, int out_cols, int vec_in,
                                                            int vec_out) {
  __shared__ __attribute__((aligned(16))) float xs[kLds];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * kTile;
  const ResamplePlan p = load_plan(plan + (int64_t)b * 8, table_floats, out_cols);
  const int n = (int)min((int64_t)max(lens[b], 0), wav_stride);
  const float* x = wav + (int64_t)b * wav_stride;
  float* y = out + (int64_t)b * out_stride;

  if (p.copy || m0 >= p.n_out) {
    copy_or_zero4(x, y, m0 + kPer * tid, p.copy ? min(n, p.n_out) : 0, out_cols, vec_in != 0, vec_out != 0);
    return;
  }

  // the tile's first output: i0 + phi0 / den, the only 64-bit division; the others follow in 32 bits from num = qs den + rs
  const int64_t pos0 = (int64_t)m0 * p.num;
  const int64_t i0 = pos0 / p.den;
  const unsigned den = (unsigned)p.den, phi0 = (unsigned)(pos0 % p.den);
  const unsigned qs = (unsigned)p.num / den, rs = (unsigned)p.num % den;
  const int live = min(kTile, p.n_out - m0);                                     // >= 1
  const int64_t i_last = i0 + (int64_t)(live - 1) * qs + (phi0 + (unsigned)(live - 1) * rs) / den;
  const int64_t a0 = (i0 - p.R + 1) & ~(int64_t)3;                               // floor to a multiple of 4: 16-byte loads
  const int64_t span = i_last + p.R - a0 + 1;                                    // input samples [a0, a0 + span) feed the tile
  const bool staged = span <= kLds;
  if (staged) {
    for (int c = kPer * tid; c < (int)span; c += kTile) {          // written out here and in reverb.hip: see wave_rows.h
      const int64_t j = a0 + c;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vec_in && j >= 0 && j + 3 < n) {
        v = *reinterpret_cast<const float4*>(x + j);
      } else {
        if (j >= 0 && j < n) v.x = x[j];
        if (j + 1 >= 0 && j + 1 < n) v.y = x[j + 1];
        if (j + 2 >= 0 && j + 2 < n) v.z = x[j + 2];
        if (j + 3 >= 0 && j + 3 < n) v.w = x[j + 3];
      }
      *reinterpret_cast<float4*>(xs + c) = v;
    }
    __syncthreads();
  }

  // outputs tid, tid + 256, ...: position of the first by one 32-bit division, the next by adding 256 num / den
  const unsigned e0 = phi0 + (unsigned)tid * rs;                                 // < 1000 + 255 * 999
  int64_t i = i0 + (int64_t)tid * qs + e0 / den;
  unsigned phi = e0 % den;
  const unsigned step_phi = ((unsigned)kThreads * rs) % den;
  const int64_t step_i = (int64_t)kThreads * qs + ((unsigned)kThreads * rs) / den;
  const int taps = 2 * p.R;
  const float* h[kPer];
  int64_t first[kPer];                                                           // input index of tap 0
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const bool on = tid + k * kThreads < live;                                   // an output behind n_out: computed at the tile's
    h[k] = table + p.off + (int64_t)(on ? phi : phi0) * taps;                    // first position (in range), written as zero
    first[k] = (on ? i : i0) - p.R + 1;
    phi += step_phi;
    i += step_i;
    if (phi >= den) {
      phi -= den;
      ++i;
    }
  }
  float acc[kPer] = {0.f, 0.f, 0.f, 0.f};
  if (staged) {
    int s[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) s[k] = (int)(first[k] - a0);
    // one tap per load: 8-byte loads of two taps measured 3 % faster on the 10-phase tables and 28 % SLOWER on a 1000-phase one, where
    // every lane reads a row of its own (profiles/resample.txt)
    for (int q = 0; q < taps; ++q) {
#pragma unroll
      for (int k = 0; k < kPer; ++k) acc[k] = fmaf(h[k][q], xs[s[k] + q], acc[k]);
    }
  } else {
    // a span beyond the LDS image (a factor above 2, or a longer filter): the same sums with the samples read from memory
    for (int q = 0; q < taps; ++q) {
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const int64_t j = first[k] + q;
        acc[k] = fmaf(h[k][q], (j >= 0 && j < n) ? x[j] : 0.f, acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int t = tid + k * kThreads;
    if (m0 + t < out_cols) y[m0 + t] = t < live ? acc[k] : 0.f;
  }
}

}  // namespace

extern "C" int asr_resample(const float* wav, int64_t wav_stride, const int32_t* lens, const int32_t* plan, const float* table,
                            int64_t table_floats, float* out, int64_t out_stride, int out_cols, int B, hipStream_t stream) {
  WaveRowsLaunch l;
  ASR_CHECK_ARG(wave_rows_launch(wav, wav_stride, out, out_stride, out_cols, B, kTile, &l));
  ASR_CHECK_ARG(lens && plan && table_floats >= 0 && (table || table_floats == 0));
  if (B == 0 || out_cols == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_LAYOUT, stream);
  return asr_launch<resample_kernel>(l.grid, dim3(kThreads), 0, stream, wav, wav_stride, lens, plan, table, table_floats, out, out_stride,
                                     out_cols, l.vec_in, l.vec_out);
}
