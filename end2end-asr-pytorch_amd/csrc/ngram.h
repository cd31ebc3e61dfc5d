// The label n-gram LM's query on the device (utils/ngram.py has the estimator and the same query on the host; include/asr_hip.h states
// the table).  keys: 64-bit n-gram keys (ids + 1 in 16-bit fields, last symbol lowest; 0 = empty slot) in an open-addressing table with
// linear probing, vals: (logp, bo) per slot.  A stored key is found within max_probe slots; an empty slot ends a search.
//   q(h, c):  acc = 0.f;  for m = len(h) .. 1:  g = last m of h, then c;  g stored: return acc + logp[g];  (last m of h) stored: acc += bo
//             return acc + logp[(c)]                                                       (fp32 adds in this order, as on the host)
// The keys of all 2 len(h) + 1 searches are known up front, so their first probes are issued together: a query costs the round trip of
// those, one more for the values, and further ones only where a first probe met another key.
#pragma once
#include "common.h"

struct NgramTable {
  const uint64_t* keys;
  const float2* vals;
  uint32_t mask;            // capacity - 1
  int max_probe, order;
};

constexpr int NGRAM_MAX_ORDER = 4;
constexpr int NGRAM_MAX_ID = 65534;

__device__ __forceinline__ uint32_t ngram_home(uint64_t key, uint32_t mask) {
  return (uint32_t)(((key ^ (key >> 31)) * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// the search from its first probe `k` (the key read at `home`): the slot that holds `key`, or -1
__device__ __forceinline__ int ngram_find(const NgramTable& t, uint64_t key, uint32_t home, uint64_t k) {
  for (int i = 0;;) {
    if (k == key) return (int)((home + (uint32_t)i) & t.mask);
    if (k == 0 || ++i >= t.max_probe) return -1;
    k = t.keys[(home + (uint32_t)i) & t.mask];
  }
}

// ctx: the key of the symbols before c, at most order - 1 of them (fields above its length are 0); c outside 0..65534: -inf
__device__ __forceinline__ float ngram_query(const NgramTable& t, uint64_t ctx, int c) {
  if (c < 0 || c > NGRAM_MAX_ID) return -INFINITY;
  const uint64_t cf = (uint64_t)(c + 1);
  uint64_t gk[NGRAM_MAX_ORDER], g1[NGRAM_MAX_ORDER], h1[NGRAM_MAX_ORDER];
  uint32_t gh[NGRAM_MAX_ORDER], hh[NGRAM_MAX_ORDER];
  bool use[NGRAM_MAX_ORDER];
#pragma unroll
  for (int m = 0; m < NGRAM_MAX_ORDER; ++m) {                 // m symbols of context: all first probes in flight together
    use[m] = m == 0 || (m < t.order && ((ctx >> (16 * (m - 1))) & 0xffffu) != 0);
    const uint64_t h = m == 0 ? 0 : ctx & ((1ull << (16 * m)) - 1ull);
    gk[m] = h << 16 | cf;
    gh[m] = ngram_home(gk[m], t.mask);
    hh[m] = ngram_home(h, t.mask);
    g1[m] = use[m] ? t.keys[gh[m]] : 0;
    h1[m] = use[m] && m > 0 ? t.keys[hh[m]] : 0;
  }
  float acc = 0.f;
#pragma unroll
  for (int m = NGRAM_MAX_ORDER - 1; m >= 1; --m) {
    if (!use[m]) continue;
    int s = ngram_find(t, gk[m], gh[m], g1[m]);
    if (s >= 0) return acc + t.vals[s].x;
    s = ngram_find(t, gk[m] >> 16, hh[m], h1[m]);
    if (s >= 0) acc += t.vals[s].y;
  }
  const int s = ngram_find(t, gk[0], gh[0], g1[0]);
  return s >= 0 ? acc + t.vals[s].x : -INFINITY;
}

// the context after `c`: the last order - 1 symbols
__device__ __forceinline__ uint64_t ngram_shift(uint64_t ctx, int c, int order) {
  return order > 1 ? (ctx << 16 | (uint64_t)(c + 1)) & ((1ull << (16 * (order - 1))) - 1ull) : 0;
}

inline int ngram_check_table(const void* keys, const void* vals, int64_t capacity, int max_probe, int order) {
  ASR_CHECK_ARG(keys && vals && max_probe >= 1);
  ASR_CHECK_ARG(capacity >= 1 && capacity <= ((int64_t)1 << 31) && (capacity & (capacity - 1)) == 0);
  ASR_CHECK_ARG(order >= 1 && order <= NGRAM_MAX_ORDER);
  return ASR_OK;
}
