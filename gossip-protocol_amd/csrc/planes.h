// planes.h — the mongering counters: C[n][r] in 0..15 as four bit planes in
// the layout of S and H, so that one instruction updates 64 rumors.  Shared by monger.hip (push) and
// monger_pull.hip (pull).  Internal to csrc/, device-inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gossip {

// c += 1 at the bits of x, saturating at 15: a ripple-carry add over the planes; a carry out of
// plane 3 sets all four planes of those bits.
__device__ __forceinline__ void planes_add(uint64_t (&c)[4], uint64_t x) {
  uint64_t carry = x;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint64_t t = c[b] & carry;
    c[b] ^= carry;
    carry = t;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) c[b] |= carry;
}

// The bits whose count is at least limit (uniform, 1..15), most significant plane first.
__device__ __forceinline__ uint64_t planes_ge(const uint64_t (&c)[4], uint32_t limit) {
  uint64_t gt = 0, eq = ~0ull;
#pragma unroll
  for (int b = 3; b >= 0; --b) {
    if ((limit >> b) & 1u) {
      eq &= c[b];
    } else {
      gt |= eq & c[b];
      eq &= ~c[b];
    }
  }
  return gt | eq;
}

}  // namespace gossip
