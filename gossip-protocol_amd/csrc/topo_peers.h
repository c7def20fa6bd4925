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

// One round over a.orow / a.ocol (rows as sorted sets); the sender ranges of launch_round_random.
// Adds the exchanges initiated by the owned senders to a.partial[2].  (The row index of a draw is
// philox.h's topo_index_from_word; the stall streaks over the rows are kernels.h's launch_stall_update.)
hipError_t launch_round_topo(const RoundArgs& a, hipStream_t st);

}  // namespace gossip
