// The key of a label sequence in the beam searches (csrc/ctc_beam.hip, csrc/rnnt_beam.hip): 64 bits mixed from the parent's key and the last
// label, so equal label sequences have equal keys however and whenever they were created (a trie node id does not: a prefix pruned and
// re-created gets a new node).  Bit 0 is set: 0 is "no key".  Two different sequences meet in a key with probability 2^-63 per comparison.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint2 beam_key(uint2 parent, int label) {
  uint64_t k = ((uint64_t)parent.y << 32 | parent.x) ^ (uint64_t)(uint32_t)(label + 1);
  k *= 0x9E3779B97F4A7C15ull; k ^= k >> 29;
  k *= 0xBF58476D1CE4E5B9ull; k ^= k >> 32;
  return make_uint2((uint32_t)k | 1u, (uint32_t)(k >> 32));
}
constexpr uint32_t BEAM_ROOT_KEY_LO = 0x2545F491u | 1u, BEAM_ROOT_KEY_HI = 0x4F6CDD1Du;      // the empty prefix

}  // namespace
