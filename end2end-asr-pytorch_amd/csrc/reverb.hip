// Reverberation of padded waveforms on the GPU with recorded room impulse responses (no counterpart in the reference; Ko et al.,
// ICASSP 2017).  The definition is DESIGN.md section 7: for a row with RIR index r >= 0, L taps h (prepared on the host: direct path
// at lag 0, unit energy; utils/audio.py prepare_rir) and n samples,
//   y[m] = sum_{k = 0}^{min(L - 1, m)} h[k] x[m - k],  0 <= m < n: ONE fmaf chain in ascending k from +0.0, fp32; the tail behind n is cut.
// A row with r = -1 is copied; columns [n, out_cols) are +0.0.  This is the front end's one FMA-bound kernel: n L multiply-adds per row.
// Grid: (tiles of kTile consecutive outputs) x utterances, 256 threads.  A tile of a reverberated row costs kTile L multiply-adds, a
// tile of a copied row or behind n moves 8 KB; launched as they lie, the cheap ones end at once and the expensive ones that follow
// pile up on the compute units that were freed first (measured at every second row copied: 86 % of the time for half the work).  So
// every workgroup works out which tile is its own: the expensive tiles come first in launch order, row by row in the batch's own order
// (longest first), the cheap ones after them -- a prefix sum over the rows' tile counts, for batches of up to 256 rows (larger ones
// are walked as they lie).  The taps are walked in chunks of kChunk; for each chunk the tile's input span, kTile + kChunk samples, goes
// into LDS with 16-byte loads, zero filled in front of sample 0 -- so the terms with k > m multiply +0.0 and leave the chain's bits
// alone (taps are finite).  Chunks whose taps all have k > m for the whole tile are not walked.
// Ownership: lane l owns the kPer = kTile / 256 CONSECUTIVE outputs kPer l .. kPer l + kPer - 1 of the tile -- the opposite of
// resample.hip's lane-strided choice, and on purpose: there every output has its own input position and phase, here kPer outputs and four
// consecutive taps touch only kPer + 3 consecutive samples, so a lane keeps a sliding window of kPer / 4 + 1 aligned float4 in registers
// and one ds_read_b128 feeds 4 kPer fmaf (lane-strided ownership would need one ds_read_b32 per fmaf: LDS bound at a quarter of the FMA
// rate).  Lanes kPer floats apart make that read a kPer / 4-way bank conflict; at one read per 2 kPer v_pk_fma_f32 the LDS stays far
// from its limit, and the longer run needs fewer register moves: v_pk_fma_f32 takes its two samples from an even-aligned register
// pair, the odd taps' pairs straddle two and are built with v_pk_mov_b32, and a run shares them between neighbouring outputs (two runs of
// four per lane, conflict free, measured 10 % slower than one run of eight).  A tap is the same for the whole workgroup: it is read at
// a uniform address, which the compiler turns into scalar loads (nothing is ever stored through the scalar path).
// Copied rows, rows the kernel refuses (written as zeros) and tiles behind n move 16 bytes per lane.  No atomics, no workspace: the
// bits of a row depend on its samples, its taps and n alone -- not on the batch, the row's position in it, alignment, or the run.
#include "wave_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = ASR_REVERB_TILE;           // outputs per workgroup
constexpr int kPer = kTile / kThreads;           // consecutive outputs per lane
constexpr int kQ = kPer / 4;                     // ... in float4
constexpr int kChunk = ASR_REVERB_CHUNK;         // taps per staged span
constexpr int kSpan = kTile + kChunk;            // staged samples
static_assert(kTile == kPer * kThreads && kPer % 4 == 0 && kChunk % 4 == 0, "whole float4 per lane and per chunk");

// outputs [m, m + 4), m < n somewhere in the run: the sums below n, +0.0 from there on
__device__ __forceinline__ void store4(float* __restrict__ y, int m, int n, int out_cols, const float (&a)[4], bool vec_out) {
  if (m >= out_cols) return;
  if (vec_out && m + 3 < n) {                    // n <= out_cols
    *reinterpret_cast<float4*>(y + m) = make_float4(a[0], a[1], a[2], a[3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (m + i < out_cols) y[m + i] = m + i < n ? a[i] : 0.f;
}

// NT consecutive taps h[0 .. NT) on a lane's kPer outputs.  The window: w[1 ..] = the samples under the outputs at the first tap,
// w[0] = the four samples before them; output i at tap t reads sample 4 + i - t of the window.
template <int NT>
__device__ __forceinline__ void taps(const float* __restrict__ h, const float4 (&w)[kQ + 1], float (&acc)[kPer]) {
  float f[4 * (kQ + 1)];
#pragma unroll
  for (int q = 0; q <= kQ; ++q) {
    f[4 * q] = w[q].x;
    f[4 * q + 1] = w[q].y;
    f[4 * q + 2] = w[q].z;
    f[4 * q + 3] = w[q].w;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float ht = h[t];
#pragma unroll
    for (int i = 0; i < kPer; ++i) acc[i] = fmaf(ht, f[4 + i - t], acc[i]);
  }
}

// one row's work, clamped: n samples to reverberate, copy or zero; a row whose index is outside [-1, nrir) or whose taps leave the bank
// reverberates nothing and is written as zeros (n = 0)
struct ReverbRow {
  int n, taps;
  int64_t off;
  bool copy;
};

__device__ __forceinline__ ReverbRow load_row(int b, const int32_t* __restrict__ lens, const int32_t* __restrict__ rir, int64_t bank_floats,
                                              const int64_t* __restrict__ rir_off, const int64_t* __restrict__ rir_len, int nrir,
                                              int64_t wav_stride, int out_cols) {
  ReverbRow w;
  w.n = (int)min((int64_t)max(lens[b], 0), min(wav_stride, (int64_t)out_cols));
  const int r = rir[b];
  w.copy = r == -1;
  w.off = 0;
  int64_t L = 0;
  if (r >= 0 && r < nrir) {
    w.off = rir_off[r];
    L = rir_len[r];
  }
  if (!w.copy && !(L >= 1 && w.off >= 0 && L <= bank_floats && w.off <= bank_floats - L)) w.n = 0;
  w.taps = (int)min(L, (int64_t)0x7fffffff);                                 // a tap beyond 2^31 never meets a sample
  return w;
}

// inclusive prefix sum of v over the workgroup's 256 threads; *total = the sum
__device__ __forceinline__ int block_scan(int v, int* wave_sums, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_scan_incl(v);
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  const int s0 = wave_sums[0], s1 = wave_sums[1], s2 = wave_sums[2], s3 = wave_sums[3];
  *total = s0 + s1 + s2 + s3;
  return incl + (wave > 0 ? s0 : 0) + (wave > 1 ? s1 : 0) + (wave > 2 ? s2 : 0);
}

__global__ __launch_bounds__(kThreads) void reverb_kernel(const float* __restrict__ wav, int64_t wav_stride,
                                                          const int32_t* __restrict__ lens, const int32_t* __restrict__ rir,
                                                          const float* __restrict__ bank, int64_t bank_floats,
                                                          const int64_t* __restrict__ rir_off, const int64_t* __restrict__ rir_len,
                                                          int nrir, float* __restrict__ out, int64_t out_stride, int out_cols,
                                                          int vec_in, int vec_out) {
  __shared__ __attribute__((aligned(16))) float xs[kSpan];
  __shared__ int wave_sums[4], mine[2];
  const int tid = threadIdx.x, B = gridDim.y, tiles = gridDim.x;
  int b = blockIdx.y, tile = blockIdx.x;
  if (B <= kThreads) {
    // thread t counts row t's expensive tiles, the first ceil(n / kTile) of a reverberated row; the g-th workgroup in launch order
    // takes the g-th expensive tile, or behind them the (g - all expensive)-th cheap one -- the tiles of a row from its count on
    int heavy = 0;
    if (tid < B) {
      const ReverbRow w = load_row(tid, lens, rir, bank_floats, rir_off, rir_len, nrir, wav_stride, out_cols);
      heavy = w.copy ? 0 : (w.n + kTile - 1) / kTile;                        // <= tiles: n <= out_cols
    }
    int all_heavy;
    const int incl = block_scan(heavy, wave_sums, &all_heavy);
    const int g = blockIdx.y * tiles + blockIdx.x;                           // < 256 * 2^20
    if (tid < B) {
      const int first = g < all_heavy ? incl - heavy : all_heavy + tid * tiles - (incl - heavy);
      const int count = g < all_heavy ? heavy : tiles - heavy;
      if (g >= first && g - first < count) {
        mine[0] = tid;
        mine[1] = g - first + (g < all_heavy ? 0 : heavy);
      }
    }
    __syncthreads();
    b = __builtin_amdgcn_readfirstlane(mine[0]);
    tile = __builtin_amdgcn_readfirstlane(mine[1]);
  }
  const int m0 = tile * kTile;
  const float* x = wav + (int64_t)b * wav_stride;
  float* y = out + (int64_t)b * out_stride;
  const ReverbRow row = load_row(b, lens, rir, bank_floats, rir_off, rir_len, nrir, wav_stride, out_cols);
  const int n = row.n;
  const bool copy = row.copy;

  if (copy || m0 >= n) {
#pragma unroll
    for (int q = 0; q < kQ; ++q) copy_or_zero4(x, y, m0 + kPer * tid + 4 * q, n, out_cols, vec_in != 0, vec_out != 0);
    return;
  }

  const float* h = bank + row.off;
  const int taps_live = min(row.taps, min(n, m0 + kTile));          // a tap k > m meets only the zeros in front of sample 0
  float acc[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) acc[i] = 0.f;
  const int ia = kChunk + kPer * tid;                                        // xs index of the lane's first sample at the chunk's first tap
  for (int c0 = 0; c0 < taps_live; c0 += kChunk) {
    // xs[i] = x[j0 + i]: the samples under the tile for the taps [c0, c0 + kChunk); j0 is a multiple of 4
    const int j0 = m0 - c0 - kChunk;
    if (c0) __syncthreads();
    for (int c = 4 * tid; c < kSpan; c += 4 * kThreads) {               // written out here and in resample.hip: see wave_rows.h
      const int j = j0 + c;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vec_in && j >= 0 && j + 3 < n) {
        v = *reinterpret_cast<const float4*>(x + j);
      } else if (j + 3 >= 0 && j < n) {
        if (j >= 0) v.x = x[j];
        if (j + 1 >= 0 && j + 1 < n) v.y = x[j + 1];
        if (j + 2 >= 0 && j + 2 < n) v.z = x[j + 2];
        if (j + 3 < n) v.w = x[j + 3];
      }
      *reinterpret_cast<float4*>(xs + c) = v;
    }
    __syncthreads();
    const int nt = min(kChunk, taps_live - c0);
    const float* hc = h + c0;
    float4 w[kQ + 1];
#pragma unroll
    for (int q = 1; q <= kQ; ++q) w[q] = *reinterpret_cast<const float4*>(xs + ia + 4 * (q - 1));
    int kk = 0;
#pragma unroll 4
    for (; kk + 4 <= nt; kk += 4) {
      w[0] = *reinterpret_cast<const float4*>(xs + ia - kk - 4);
      taps<4>(hc + kk, w, acc);
#pragma unroll
      for (int q = kQ; q >= 1; --q) w[q] = w[q - 1];
    }
    if (kk < nt) {                                                           // the last one to three taps of the response
      w[0] = *reinterpret_cast<const float4*>(xs + ia - kk - 4);
      if (nt - kk == 1) taps<1>(hc + kk, w, acc);
      else if (nt - kk == 2) taps<2>(hc + kk, w, acc);
      else taps<3>(hc + kk, w, acc);
    }
  }
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const float a[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    store4(y, m0 + kPer * tid + 4 * q, n, out_cols, a, vec_out != 0);
  }
}

}  // namespace

extern "C" int asr_reverb(const float* wav, int64_t wav_stride, const int32_t* lens, const int32_t* rir, const float* bank,
                          int64_t bank_floats, const int64_t* rir_off, const int64_t* rir_len, int nrir, float* out,
                          int64_t out_stride, int out_cols, int B, hipStream_t stream) {
  WaveRowsLaunch l;
  ASR_CHECK_ARG(wave_rows_launch(wav, wav_stride, out, out_stride, out_cols, B, kTile, &l));
  ASR_CHECK_ARG(lens && rir && bank_floats >= 0 && nrir >= 0 && ((bank && rir_off && rir_len) || nrir == 0));
  if (B == 0 || out_cols == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_LAYOUT, stream);
  return asr_launch<reverb_kernel>(l.grid, dim3(kThreads), 0, stream, wav, wav_stride, lens, rir, bank, bank_floats, rir_off, rir_len, nrir, out,
                                   out_stride, out_cols, l.vec_in, l.vec_out);
}
