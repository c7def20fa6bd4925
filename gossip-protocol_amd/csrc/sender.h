// sender.h — what the sender-per-lane rounds share (topo_peers.hip, monger.hip; DESIGN.md §3.9,
// §3.11): one lane per sender, at most 8192 blocks of 256 and a stride loop, the edges in batches
// of four (one Philox block).  Internal to csrc/, device-inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "philox.h"
#include "wave.h"

namespace gossip {

constexpr int kSenderBlock = 256;

// at most 8192 blocks, as the FLOOD launches: larger ranges take further trips of the stride loop
inline uint32_t sender_grid(uint64_t work) {
  const uint64_t b = (work + kSenderBlock - 1) / kSenderBlock;
  return (uint32_t)(b == 0 ? 1 : (b < 8192 ? b : 8192));
}

// index of word 0 of global node n in the gathered [G][W][Nl] image (word w: + w * Nl)
__device__ __forceinline__ uint64_t image_base(uint32_t n, uint64_t Nl, uint32_t W) {
  const uint32_t r = n / (uint32_t)Nl;
  return (uint64_t)r * W * Nl + (n - r * (uint32_t)Nl);
}

// Edges 4q .. 4q + cnt - 1 of sender n: the peers and whether each edge is live (drawn and not
// lost).  TOPO: the row of d > 0 entries at a.ocol + b; else uniform over the other N - 1 nodes
// (b and d are not read).  Every draw is made and every row load issued before one is consumed.
// fa is the caller's fault block, which need not be a.fa (topo_peers.hip clears its stall array).
template <bool TOPO, bool FAULTS>
__device__ __forceinline__ void resolve_batch(const RoundArgs& a, const Faults& fa, const Reach& rc, uint32_t n,
                                              uint32_t b, uint32_t d, uint32_t q, uint32_t cnt, uint32_t (&p)[4],
                                              bool (&live)[4]) {
  const u32x4 x = philox4x32_10(u32x4{n, a.t, 0u, q}, a.key0, a.key1);
  u32x4 lw{0, 0, 0, 0};
  if (FAULTS && fa.loss) lw = loss_draws(n, a.t, q, a.key0, a.key1);
  if (TOPO) {
    uint32_t idx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) idx[i] = topo_index_from_word(lane_of(x, i), d);
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = (uint32_t)i < cnt ? a.ocol[b + idx[i]] : n;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = peer_from_word(lane_of(x, i), a.N - 1, n);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    live[i] = (uint32_t)i < cnt && !(FAULTS && edge_lost(fa, rc, p[i], lane_of(lw, i)));
}

}  // namespace gossip
