// topo_peers.h — random gossip over the topology: PUSH / PULL /
// PUSHPULL whose k peers per node and round are drawn from the node's own row of the
// topology (GOSSIP_FLAG_TOPO_PEERS) instead of from all N nodes.
//
// Reference: (*NodeState).Gossip ranges over Topology[node.ID()] (main.go:72) and sends to
// every neighbour; here a node sends to k of them, drawn with replacement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "philox.h"

namespace gossip {

// Index into a row of d entries from one Philox word: floor(x * d / 2^32), one high-half
// product (the scaling of peer_from_word, over the row instead of over [0, N) \ {n}).
__host__ __device__ __forceinline__ uint32_t topo_index_from_word(uint32_t x, uint32_t d) {
  return (uint32_t)(((uint64_t)x * d) >> 32);
}

// One round over a.orow / a.ocol (rows as sorted sets); the sender ranges of launch_round_random.
// Adds the exchanges initiated by the owned senders to a.partial[2].
hipError_t launch_round_topo(const RoundArgs& a, hipStream_t st);
// Stall streaks after round t, the peers resolved through the rows (all N nodes).
hipError_t launch_stall_update_topo(uint8_t* stall, uint64_t N, uint32_t k, uint32_t t, uint32_t key0, uint32_t key1,
                                    const Faults& fa, const uint32_t* orow, const uint32_t* ocol, hipStream_t st);

}  // namespace gossip
