// monger_close.h — the cooling step the close passes of pull and push-pull mongering share
// (monger_pull.hip, monger_pushpull.hip).
// Internal to csrc/, device-inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "monger_pull.h"
#include "planes.h"

namespace gossip {

// One word of node s (at = its offset in the [W][N] arrays, plane = W * N) with feedback nd / ls, at
// least one of them set.  One coin per node and round, drawn on first use (coin < 0: not drawn yet).
// A needed rumor's count goes back to 0 and nothing else happens to it; a rumor that was only
// needless, under a coin that holds, is counted once and cools at the limit.  Returns the bits that
// cool.  While a rumor is hot its count is below the limit, so planes_add never saturates here.
template <bool COUNT>
__device__ __forceinline__ uint64_t monger_cool_word(const MongerPullArgs& m, uint64_t s, uint64_t at, uint64_t plane,
                                                     uint64_t nd, uint64_t ls, int& coin) {
  const RoundArgs& a = m.a;
  if (coin < 0) coin = m.cool && cool_draws((uint32_t)s, a.t, 0u, a.key0, a.key1).x < m.cool;
  const uint64_t inc = coin ? ls & ~nd : 0ull;
  uint64_t clear = inc;
  if (COUNT) {
    uint64_t c[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) c[b] = m.C[(uint64_t)b * plane + at];
    const uint64_t reset = nd & (c[0] | c[1] | c[2] | c[3]);
#pragma unroll
    for (int b = 0; b < 4; ++b) c[b] &= ~nd;
    if (inc) {
      planes_add(c, inc);
      clear = planes_ge(c, m.limit) & inc;
    }
    if (reset | inc) {
#pragma unroll
      for (int b = 0; b < 4; ++b) m.C[(uint64_t)b * plane + at] = c[b];
    }
  }
  return clear;
}

}  // namespace gossip
