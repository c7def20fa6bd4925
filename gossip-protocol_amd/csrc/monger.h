// monger.h — rumor mongering: PUSH gossip whose nodes lose interest.
// An engine created with GOSSIP_FLAG_MONGER keeps, beside S (the rumors a node knows), a second
// bitset H ⊆ S per node in the same layout (the rumors it is still spreading, "hot").  A push
// carries only the hot rumors; a counted contact cools them with probability cool / 2^32.
// From the first gossip_set_monger_limit above 1 on the engine also keeps a count in 0..15 per node
// and rumor: a contact whose coin holds is counted, and a rumor cools
// once its count reaches the limit.
//
// Reference: (*NodeState).Gossip forwards every value once (main.go:65-89) and the broadcast
// handler drops a value it holds (main.go:113); rumor mongering (Demers et al., "Epidemic
// algorithms for replicated database maintenance", feedback / blind, coin) is the strategy
// between that direct mail and anti-entropy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "monger_conn.h"
#include "philox.h"

namespace gossip {

// One shard (G == 1): the image a.G is S_t itself, word w of node n at a.G[w * N + n].
struct MongerArgs {
  RoundArgs a;         // S_t (a.G), S_{t+1} (a.Snext, a copy of S_t), rows, faults, partial
  const uint64_t* H;   // H_t      [W][N]
  uint64_t* Hnext;     // H_{t+1}  [W][N], a copy of H_t
  uint32_t cool;       // an edge's coin (stream tag 5) holds when its word is below this
  uint32_t blind;      // 0: feedback (a delivered push counts what the peer held), 1: every attempt counts
  bool topo;           // peers drawn from the rows (GOSSIP_FLAG_TOPO_PEERS) or from all N nodes
  // Counters, after the fields every engine has so that their offsets stay: bit r of
  // plane b of C[n][r] at C[(b * W + w) * N + n], r = 64 w + bit.  Only lane n reads or writes C[*][n].
  uint64_t* C;         // [4][W][N], updated in place; null: the engine holds no counters (the coin round)
  uint32_t limit;      // 1..15: a rumor cools at a counted contact that leaves its count at or above this
  // Connection limit, after everything above for the same reason: conn.c == 0 is the
  // unlimited round; else the slots hold the round's verdicts (launch_conn_arbitrate ran before)
  ConnArgs conn;
};

// The cooling coins of edges 4q .. 4q + 3 of node n in round t: Philox stream tag 5.
__host__ __device__ __forceinline__ u32x4 cool_draws(uint32_t n, uint32_t t, uint32_t q, uint32_t k0, uint32_t k1) {
  return philox4x32_10(u32x4{n, t, 5u, q}, k0, k1);
}

// One round: ORs the pushes into a.Snext and Hnext, clears the cooled bits of Hnext, and adds k per
// initiating node to a.partial[2] (with m.conn.c set nothing: the arbitration counted the attempts).  With m.C set, a coin that holds adds one to the count of every
// rumor of its counted set (saturating at 15), and a rumor cools when that leaves it at m.limit or more.
hipError_t launch_round_monger(const MongerArgs& m, hipStream_t st);
// Client broadcast: node >= 0 sets one bit, node < 0 every rumor at its tag-2 origin; the bit is
// set in H only where it is new in S (a cooled rumor is not re-heated).
hipError_t launch_monger_inject(uint64_t* S, uint64_t* H, uint64_t N, uint32_t R, uint32_t key0, uint32_t key1,
                                int64_t node, uint32_t rumor, hipStream_t st);

}  // namespace gossip
