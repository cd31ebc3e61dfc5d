// SpecAugment on the normalised log-spectrogram (csrc/spec_augment.hip; definition in DESIGN.md section 7) and the per-utterance
// normalisation it shares with spect_normalize_kernel (csrc/spectrogram.hip): both go through spect_norm_of / spect_norm_apply, so the
// fused normalise + warp + mask pass produces the bits of the separate passes.
#pragma once
#include "common.h"

constexpr int kSpecParams = ASR_SPEC_AUGMENT_PARAMS;      // int32 per utterance: {n, c, w, nF, nT, 0, 0, 0, 8 x (f0, fw), 8 x (t0, tw)}
constexpr int kSpecMaxMasks = 8;
// (2u+1) s - d of the time warp stays below 2^31 for n <= 16384 frames; longer utterances take the same expressions in 64-bit integers
constexpr int kSpecWarp32 = 16384;

// frames of an utterance of `len` samples: 1 + (len + n_fft - n_fft) / hop of the centred STFT; the host path pads utterances shorter
// than 2 samples (utils/audio.py spec_frames)
__host__ __device__ __forceinline__ int spect_frames(int len, int hop) { return 1 + (len > 2 ? len : 2) / hop; }

// what a thread of a (B * F * ceil(Tmax / 256)) x 256 grid works on: frame t (Tmax and beyond in the last block of a row) of row (b, f)
struct SpectPos {
  int b, f, t;
};
__device__ __forceinline__ SpectPos spect_pos(int F, int Tmax) {
  const int tb = (Tmax + 255) / 256;
  const int tblk = blockIdx.x % tb, f = (blockIdx.x / tb) % F, b = blockIdx.x / (tb * F);
  return {b, f, (int)(tblk * 256 + threadIdx.x)};
}

struct SpectNorm {
  float mean, rstd;
};

// mean and 1 / unbiased std of an utterance of nfr frames x F bins from the two reductions of asr_spect_finish
__device__ __forceinline__ SpectNorm spect_norm_of(const float* __restrict__ sums, const float* __restrict__ sq, int b, int nfr, int F) {
  const float n = (float)nfr * (float)F;
  SpectNorm s;
  s.mean = sums[b] / n;
  s.rstd = rsqrtf(sq[b] / (n - 1.f));                     // unbiased, as torch.Tensor.std() (data_loader.py:87-88)
  return s;
}
__device__ __forceinline__ float spect_norm_apply(float v, const SpectNorm& s) { return (v - s.mean) * s.rstd; }

// out (B, F, T_out) <- warp + masks of x (B, F, >= T_out), rows ldx_row / ldo_row floats apart.  lengths != nullptr: x is the raw
// log-magnitude and is normalised on load with (sums, sq) over the spect_frames(lengths[b], hop) frames of the utterance.
__attribute__((visibility("hidden"))) int spec_augment_launch(const float* x, int64_t ldx_row, float* out, int64_t ldo_row,
                                                              const int32_t* params, const int32_t* lengths, const float* sums,
                                                              const float* sq, int hop, int B, int F, int T_out, hipStream_t stream);
