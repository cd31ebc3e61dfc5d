// The phrase automaton's transition on the device (utils/context.py has the automaton, the credit and the same rule on the host;
// include/asr_hip.h states the table).  keys: (state + 1) << 16 | (label + 1) in an open-addressing table of the n-gram table's form
// (0 = empty slot, linear probing, the home function of ngram.h), vals: (next state, delta of the credit) per slot, hold: per state the
// labels of its partial match that are not yet earned.  Stored are the transitions out of eps (state 0) and those that lead neither to
// eps nor where eps itself would go:
//   step(s, c):  (s, c) stored: its value;  else (eps, c) stored: (next, delta_eps - hold[s]);  else (eps, -hold[s])
// A label outside 0..65534 steps to eps; a state outside 0..states-1 is taken for eps.  Both first probes, the values beside them and
// hold[s] are issued together: a step costs the one round trip of those, and further ones only where a first probe met another key (the
// table is at most half full).
#pragma once
#include "ngram.h"           // ngram_home: the one hash

struct CtxTable {
  const uint64_t* keys;
  const int2* vals;
  const int32_t* hold;
  uint32_t mask;            // capacity - 1
  int max_probe, states;
};

constexpr int CTX_MAX_ID = NGRAM_MAX_ID;

// the first probes of a step, in flight before anything waits for them
struct CtxProbe {
  uint64_t ks, ke, s1, e1;  // the keys of (s, c) and (eps, c) and what their home slots hold
  int2 sv, ev;              // the values at the two home slots
  uint32_t hs, he;
  int hold;
  bool ok;                  // the label fits a key field
};

__device__ __forceinline__ CtxProbe ctx_probe(const CtxTable& t, int s, int c) {
  CtxProbe p;
  p.ok = c >= 0 && c <= CTX_MAX_ID;
  s = s >= 0 && s < t.states ? s : 0;
  const uint64_t cf = p.ok ? (uint64_t)(c + 1) : 0;
  p.ks = (uint64_t)(s + 1) << 16 | cf;
  p.ke = (uint64_t)1 << 16 | cf;
  p.hs = ngram_home(p.ks, t.mask);
  p.he = ngram_home(p.ke, t.mask);
  p.s1 = p.ok ? t.keys[p.hs] : 0;
  p.e1 = p.ok ? t.keys[p.he] : 0;
  p.sv = p.ok ? t.vals[p.hs] : make_int2(0, 0);
  p.ev = p.ok ? t.vals[p.he] : make_int2(0, 0);
  p.hold = t.hold[s];
  return p;
}

// the search from its first probe `k` (the key read at `home`): the slot that holds `key`, or -1
__device__ __forceinline__ int ctx_find(const CtxTable& t, uint64_t key, uint32_t home, uint64_t k) {
  for (int i = 0;;) {
    if (k == key) return (int)((home + (uint32_t)i) & t.mask);
    if (k == 0 || ++i >= t.max_probe) return -1;
    k = t.keys[(home + (uint32_t)i) & t.mask];
  }
}

// -> (next state, delta of the credit)
__device__ __forceinline__ int2 ctx_finish(const CtxTable& t, const CtxProbe& p) {
  if (!p.ok) return make_int2(0, -p.hold);
  int i = ctx_find(t, p.ks, p.hs, p.s1);
  if (i >= 0) return (uint32_t)i == p.hs ? p.sv : t.vals[i];
  i = ctx_find(t, p.ke, p.he, p.e1);
  if (i < 0) return make_int2(0, -p.hold);
  const int2 v = (uint32_t)i == p.he ? p.ev : t.vals[i];
  return make_int2(v.x, v.y - p.hold);
}

__device__ __forceinline__ int2 ctx_step(const CtxTable& t, int s, int c) { return ctx_finish(t, ctx_probe(t, s, c)); }

inline int ctx_check_table(const void* keys, const void* vals, int64_t capacity, int max_probe, const void* hold, int states) {
  ASR_CHECK_ARG(keys && vals && hold && max_probe >= 1 && states >= 1);
  ASR_CHECK_ARG(capacity >= 1 && capacity <= ((int64_t)1 << 31) && (capacity & (capacity - 1)) == 0);
  return ASR_OK;
}
