// Spectrogram front end on the GPU (reference: SpectrogramParser.parse_audio, utils/data_loader.py:72-89):
//   D = |STFT(y)| with n_fft = win_length = 320, hop 160, symmetric Hamming window, centred frames with reflect padding,
//   spect = log1p(D), then (spect - mean) / std over the whole utterance with the unbiased std.
// The DFT is a dense contraction: windowed frames (B*T, 320) x [cos | -sin] basis (322, 320)^T on asr_gemm_nt in fp32
// (MFMA 16x16x4 f32, fp32 accumulate); this file holds the kernels either side of it:
//   asr_stft_frames   : padded waveforms -> windowed frames, reflect padding resolved per sample, rows of frames past an
//                       utterance's end written as zeros
//   asr_spect_logmag  : (re, im) rows -> log1p(sqrt(re^2 + im^2)) stored as (B, F, T) (T contiguous, the loader's layout,
//                       data_loader.py:196-209: zero padded along T) + per-utterance sum
//   asr_spect_sqdev   : per-utterance sum of squared deviations from the mean (two-pass variance)
//   asr_spect_normalize: in place (x - mean) * rstd on the valid frames
// asr_spect_finish_aug ends with the SpecAugment pass of csrc/spec_augment.hip instead, which normalises on load with the same
// expressions (spec_augment.h) and writes the features already cut to T_out frames.
// asr_fbank_finish / asr_fbank_finish_aug (--features fbank) replace only the first pass: fbank_logmel_kernel
// turns the same (re, im) rows into log-mel filterbank features (B, M, T) + per-utterance sum; the passes after it are the ones above
// with F := M.
#include "spec_augment.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void stft_frames_kernel(const float* __restrict__ wav, int64_t wav_stride,
                                                          const int32_t* __restrict__ lengths, const float* __restrict__ window,
                                                          float* __restrict__ frames, int B, int Tmax, int n_fft, int hop) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)B * Tmax * n_fft;
  if (i >= total) return;
  const int n = (int)(i % n_fft);
  const int64_t ft = i / n_fft;
  const int t = (int)(ft % Tmax), b = (int)(ft / Tmax);
  const int len = max(lengths[b], 2);                 // the host path pads utterances shorter than 2 samples (audio.py)
  const int nfr = spect_frames(lengths[b], hop);
  float v = 0.f;
  if (t < nfr) {
    const int pad = n_fft / 2;
    int j = t * hop + n - pad;                        // index into the unpadded signal
    bool ok = true;
    if (len > pad) {                                  // numpy 'reflect' (no edge repeat)
      if (j < 0) j = -j;
      if (j >= len) j = 2 * (len - 1) - j;
      ok = j >= 0 && j < len;
    } else {
      ok = j >= 0 && j < len;                         // very short signals: zero padding (audio.py)
    }
    if (ok) {
      const float s = j < lengths[b] ? wav[b * wav_stride + j] : 0.f;
      v = s * window[n];
    }
  }
  frames[i] = v;
}

// block = 256 threads over consecutive t of one (b, f) row segment: coalesced writes along T; reads re/im with stride ld
__global__ __launch_bounds__(256) void spect_logmag_kernel(const float* __restrict__ reim, int64_t ld, const int32_t* __restrict__ lengths,
                                                           float* __restrict__ spect, float* __restrict__ sums, int B, int F,
                                                           int Tmax, int hop) {
  __shared__ float red[4];
  const auto [b, f, t] = spect_pos(F, Tmax);
  const int nfr = spect_frames(lengths[b], hop);
  float v = 0.f;
  if (t < Tmax) {
    if (t < nfr) {
      const float* r = reim + ((int64_t)b * Tmax + t) * ld;
      const float re = r[f], im = r[F + f];
      v = log1pf(sqrtf(re * re + im * im));
    }
    spect[((int64_t)b * F + f) * Tmax + t] = v;
  }
  const float s = block_sum(v, red);
  if (threadIdx.x == 0) atomicAdd(sums + b, s);
}

__global__ __launch_bounds__(256) void spect_sqdev_kernel(const float* __restrict__ spect, const int32_t* __restrict__ lengths,
                                                          const float* __restrict__ sums, float* __restrict__ sq, int B, int F, int Tmax,
                                                          int hop) {
  __shared__ float red[4];
  const auto [b, f, t] = spect_pos(F, Tmax);
  const int nfr = spect_frames(lengths[b], hop);
  const float mean = sums[b] / ((float)nfr * (float)F);
  float v = 0.f;
  if (t < nfr && t < Tmax) {
    const float d = spect[((int64_t)b * F + f) * Tmax + t] - mean;
    v = d * d;
  }
  const float s = block_sum(v, red);
  if (threadIdx.x == 0) atomicAdd(sq + b, s);
}

__global__ __launch_bounds__(256) void spect_normalize_kernel(float* __restrict__ spect, const int32_t* __restrict__ lengths,
                                                              const float* __restrict__ sums, const float* __restrict__ sq, int B, int F,
                                                              int Tmax, int hop) {
  const auto [b, f, t] = spect_pos(F, Tmax);
  const int nfr = spect_frames(lengths[b], hop);
  if (t >= nfr || t >= Tmax) return;
  const SpectNorm nm = spect_norm_of(sums, sq, b, nfr, F);
  float* p = spect + ((int64_t)b * F + f) * Tmax + t;
  *p = spect_norm_apply(*p, nm);
}

// Log-mel first pass.  One workgroup per (utterance, tile of 64 frames): the tile's (re, im) rows are read ALONG the row (a wave per
// row, 256 contiguous bytes per load) and their power spectrum is staged in LDS as 64 x K fp32 with an odd row stride S = K | 1, so
// that in the second half, where each lane owns a frame and reads its own row, the 32 lanes of an LDS access fall on 32 banks.  Each
// wave then walks every fourth filter: first / count / weights are wave-uniform (scalar loads), the store is 256 contiguous bytes
// along T.  Filters are clamped to the K bins and the nw weights: nothing outside the staged tile or the arrays is read.
constexpr int kFbankTile = 64;                   // tests/test_gpu_frontend_golden.py repeats it (FBANK_TILE)

__global__ __launch_bounds__(256) void fbank_logmel_kernel(const float* __restrict__ reim, int64_t ld, const int32_t* __restrict__ lengths,
                                                           const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                           const float* __restrict__ wts, int nw, float floor_v, float* __restrict__ feat,
                                                           float* __restrict__ sums, int B, int K, int M, int Tmax, int hop) {
  extern __shared__ __attribute__((aligned(16))) float fbank_lds[];
  __shared__ float red[4];
  const int S = K | 1;
  float* pw = fbank_lds;                                                  // kFbankTile x S power spectrum
  int* offs = reinterpret_cast<int*>(fbank_lds + kFbankTile * S);         // M: start of each filter's weights
  const int tiles = (Tmax + kFbankTile - 1) / kFbankTile;
  const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * kFbankTile;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nfr = spect_frames(lengths[b], hop);
  const int nv = min(min(nfr, Tmax) - t0, kFbankTile);                    // frames of this tile that belong to the utterance
  const int t = t0 + lane;
  float* out = feat + (int64_t)b * M * Tmax + t;
  if (nv <= 0) {                                                          // whole tile past the utterance's end: zeros, nothing to add
    if (t < Tmax)
      for (int m = wave; m < M; m += 4) out[(int64_t)m * Tmax] = 0.f;
    return;
  }
  if (wave == 0) {                                                        // exclusive prefix sum of the counts
    int carry = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {
      const int m = m0 + lane;
      const int c = m < M ? min(max(count[m], 0), K) : 0;
      const int incl = wave_scan_incl(c);
      if (m < M) offs[m] = carry + incl - c;
      carry += __shfl(incl, 63, 64);
    }
  }
  for (int r = wave; r < nv; r += 4) {
    const float* row = reim + ((int64_t)b * Tmax + t0 + r) * ld;
    for (int k = lane; k < K; k += 64) {
      const float re = row[k], im = row[K + k];
      pw[r * S + k] = re * re + im * im;
    }
  }
  __syncthreads();
  const bool valid = lane < nv;
  const float* p = pw + lane * S;
  float part = 0.f;
  for (int m = wave; m < M; m += 4) {
    const int o = __builtin_amdgcn_readfirstlane(offs[m]);
    const int f0 = min(max(__builtin_amdgcn_readfirstlane(first[m]), 0), K);
    const int c = max(min(min(__builtin_amdgcn_readfirstlane(count[m]), K - f0), nw - o), 0);
    float acc = 0.f;
    for (int j = 0; j < c; ++j) acc = fmaf(wts[o + j], p[f0 + j], acc);
    const float v = valid ? logf(fmaxf(acc, floor_v)) : 0.f;
    if (t < Tmax) out[(int64_t)m * Tmax] = v;
    part += v;
  }
  const float s = block_sum(part, red);
  if (threadIdx.x == 0) atomicAdd(sums + b, s);
}

struct MelBank {                                 // the sparse filter bank of the log-mel first pass
  const int32_t *first, *count;
  const float* weights;
  int nw;
  float floor;
};
struct SpecAug {                                 // SpecAugment rows and where the augmented features, cut to T_out frames, go
  const int32_t* params;
  float* out;
  int T_out;
};

// The finish of all four entries: first pass (log-mel through `bank`, log-magnitude of the K = F bins without one) -> feat (B, F, Tmax)
// and sums; with `normalize` the squared deviations, then either the in-place normalisation or, with `aug`, the SpecAugment pass that
// normalises on load.
int features_finish(const float* reim, int64_t ld, const int32_t* lengths, float* feat, float* sums, float* sqdev, int B, int K, int F,
                    int Tmax, int hop, const MelBank* bank, bool normalize, const SpecAug* aug, hipStream_t stream) {
  ASR_CHECK_ARG(reim && lengths && feat && sums && sqdev && B >= 0 && K > 0 && F > 0 && Tmax >= 0 && hop > 0 && ld >= 2 * (int64_t)K);
  if (bank) ASR_CHECK_ARG(bank->first && bank->count && bank->weights && bank->nw >= 0 && bank->floor > 0.f);
  if (aug) ASR_CHECK_ARG(aug->out && aug->params && aug->T_out >= 0 && aug->T_out <= Tmax && feat != aug->out);
  if (B == 0 || Tmax == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_LAYOUT, stream);
  const dim3 grid((unsigned)((int64_t)B * F * ((Tmax + 255) / 256))), block(256);
  if (bank) {
    const size_t lds = ((size_t)kFbankTile * (K | 1) + F) * sizeof(float);
    if (lds > 160 * 1024) return ASR_EUNSUPPORTED;
    const dim3 tiles((unsigned)((int64_t)B * ((Tmax + kFbankTile - 1) / kFbankTile)));
    ASR_TRY(asr_launch<fbank_logmel_kernel>(tiles, block, lds, stream, reim, ld, lengths, bank->first, bank->count, bank->weights, bank->nw,
                                            bank->floor, feat, sums, B, K, F, Tmax, hop));
  } else {
    ASR_TRY(asr_launch<spect_logmag_kernel>(grid, block, 0, stream, reim, ld, lengths, feat, sums, B, F, Tmax, hop));
  }
  if (!normalize) return ASR_OK;
  ASR_TRY(asr_launch<spect_sqdev_kernel>(grid, block, 0, stream, feat, lengths, sums, sqdev, B, F, Tmax, hop));
  if (aug) return spec_augment_launch(feat, Tmax, aug->out, aug->T_out, aug->params, lengths, sums, sqdev, hop, B, F, aug->T_out, stream);
  return asr_launch<spect_normalize_kernel>(grid, block, 0, stream, feat, lengths, sums, sqdev, B, F, Tmax, hop);
}

}  // namespace

extern "C" int asr_stft_frames(const float* wav, int64_t wav_stride, const int32_t* lengths, const float* window, float* frames, int B,
                               int Tmax, int n_fft, int hop, hipStream_t stream) {
  ASR_CHECK_ARG(wav && lengths && window && frames && B >= 0 && Tmax >= 0 && n_fft > 0 && hop > 0);
  const int64_t total = (int64_t)B * Tmax * n_fft;
  if (total == 0) return ASR_OK;
  AsrProfScope prof(ASR_OP_LAYOUT, stream);
  return asr_launch<stft_frames_kernel>(dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, stream, wav, wav_stride, lengths, window, frames,
                                        B, Tmax, n_fft, hop);
}

extern "C" int asr_spect_finish(const float* reim, int64_t ld, const int32_t* lengths, float* spect, float* sums, float* sqdev, int B,
                                int F, int Tmax, int hop, int normalize, hipStream_t stream) {
  return features_finish(reim, ld, lengths, spect, sums, sqdev, B, F, F, Tmax, hop, nullptr, normalize != 0, nullptr, stream);
}

extern "C" int asr_spect_finish_aug(const float* reim, int64_t ld, const int32_t* lengths, float* raw, float* sums, float* sqdev, float* out,
                                    const int32_t* params, int B, int F, int Tmax, int T_out, int hop, hipStream_t stream) {
  const SpecAug aug = {params, out, T_out};
  return features_finish(reim, ld, lengths, raw, sums, sqdev, B, F, F, Tmax, hop, nullptr, true, &aug, stream);
}

extern "C" int asr_fbank_finish(const float* reim, int64_t ld, const int32_t* lengths, float* feat, float* sums, float* sqdev, int B, int K,
                                int M, int Tmax, int hop, int normalize, const int32_t* first, const int32_t* count, const float* weights,
                                int nw, float floor, hipStream_t stream) {
  const MelBank bank = {first, count, weights, nw, floor};
  return features_finish(reim, ld, lengths, feat, sums, sqdev, B, K, M, Tmax, hop, &bank, normalize != 0, nullptr, stream);
}

extern "C" int asr_fbank_finish_aug(const float* reim, int64_t ld, const int32_t* lengths, float* raw, float* sums, float* sqdev, float* out,
                                    const int32_t* params, int B, int K, int M, int Tmax, int T_out, int hop, const int32_t* first,
                                    const int32_t* count, const float* weights, int nw, float floor, hipStream_t stream) {
  const MelBank bank = {first, count, weights, nw, floor};
  const SpecAug aug = {params, out, T_out};
  return features_finish(reim, ld, lengths, raw, sums, sqdev, B, K, M, Tmax, hop, &bank, true, &aug, stream);
}
