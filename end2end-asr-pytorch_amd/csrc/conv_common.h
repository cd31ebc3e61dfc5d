// What the translation units of the vgg_cnn front end share besides common.h (conv_igemm.hip, conv_wgrad.hip, pool.hip).
#pragma once
#include "common.h"

// Ablation hooks (ASR_IGEMM_ABLATE / ASR_WGRAD_ABLATE) exist only in -DASR_TUNE_ABLATE builds: a run-time test inside the MFMA
// loops costs scalar branches per step and blocks unrolling.
#ifdef ASR_TUNE_ABLATE
#define ASR_ABL(P, BIT) (((P).ablate & (BIT)) != 0)
#else
#define ASR_ABL(P, BIT) false
#endif

// workgroups of 256 threads for a grid-stride streaming kernel over `total_threads` items
static inline unsigned stream_grid(int64_t total_threads) {
  int64_t blocks = ceil_div64(total_threads, 256);
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
