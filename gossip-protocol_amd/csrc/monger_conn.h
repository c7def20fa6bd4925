// monger_conn.h — connection limits and hunting for the three mongering rounds (DESIGN.md §2.17,
// §3.15): a node accepts at most c incoming connections per round, and an initiator whose edge was
// refused tries up to h further peers.  Which edges count as delivered, and with which peer, is
// decided before the request pass by an arbitration that does not depend on the schedule; the
// request kernels (monger.hip, monger_pull.hip, monger_pushpull.hip) then read the verdicts through
// conn_resolve and run §2.13-§2.16 on the accepted edges.
//
// Reference: (*NodeState).Gossip sends to every neighbour and each send is served (main.go:65-89);
// Demers et al. ("Epidemic algorithms for replicated database maintenance", §1.4) name connection
// limits and hunting as the last pair of variations of rumor mongering.
//
// Arbitration keeps c slots per node, [c][N] 64-bit keys, all ones = empty.  An attempt of stage s
// carries the key s << 60 | prio << 38 | n << 6 | j; inserting it is a chain of atomic minima down
// the slots of its target (conn_insert), after which slot i holds the (i+1)-th smallest key in any
// schedule.  The stage is in the top bits, so a key of a later stage never displaces an earlier
// one and the final slots answer for every stage: accepted iff key <= slot[c - 1][target].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "philox.h"

namespace gossip {

constexpr uint64_t kConnEmpty = ~0ull;
constexpr uint32_t kConnMaxLimit = 8, kConnMaxHunt = 15;
// the counters of one round: attempts, accepted, finally refused, hunt attempts, then the delivered
// attempts of each stage (what a later stage reads to know that nothing is open)
constexpr uint32_t kConnCounters = 4 + kConnMaxHunt + 1;

struct ConnArgs {
  uint64_t* slots;  // [c][N]; null: no limit (c == 0)
  uint64_t* cnt;    // [kConnCounters], zero at the start of a round; the request kernels do not read it
  uint32_t c, h;    // 1..8 and 0..15; c == 0: the unlimited round
};

// Stream tag 6, the stage in the tag word's upper half.  Priority words use counter word 3 = j >> 2,
// hunt words 16 + (j >> 2): k <= 64 keeps the two apart.
__host__ __device__ __forceinline__ u32x4 conn_prio_draws(uint32_t n, uint32_t t, uint32_t s, uint32_t q, uint32_t k0,
                                                          uint32_t k1) {
  return philox4x32_10(u32x4{n, t, 6u | (s << 16), q}, k0, k1);
}
__host__ __device__ __forceinline__ u32x4 conn_hunt_draws(uint32_t n, uint32_t t, uint32_t s, uint32_t q, uint32_t k0,
                                                          uint32_t k1) {
  return philox4x32_10(u32x4{n, t, 6u | (s << 16), 16u + q}, k0, k1);
}
// n < N < 2^32: no key is all ones
__host__ __device__ __forceinline__ uint64_t conn_key(uint32_t s, uint32_t prio_word, uint32_t n, uint32_t j) {
  return ((uint64_t)s << 60) | ((uint64_t)(prio_word >> 10) << 38) | ((uint64_t)n << 6) | j;
}

// The verdicts of stage s for the batch q of initiator n.  open[i]: edge 4q + i made a delivered
// attempt at p[i] in stage s, and every attempt of that stage has been inserted.  acc[i] = it was
// accepted; open[i] stays set where it was refused.  Keys of later stages that other lanes insert
// meanwhile do not change the answer: they are larger, and the last slot only falls.
__device__ __forceinline__ void conn_verdicts(const ConnArgs& ca, const RoundArgs& a, uint32_t n, uint32_t q,
                                              uint32_t s, const uint32_t (&p)[4], bool (&open)[4], bool (&acc)[4]) {
  const u32x4 pw = conn_prio_draws(n, a.t, s, q, a.key0, a.key1);
  const uint64_t* last = ca.slots + (uint64_t)(ca.c - 1u) * a.N;
  uint64_t lv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) lv[i] = open[i] ? last[p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc[i] = open[i] && conn_key(s, lane_of(pw, i), n, 4u * q + i) <= lv[i];
    open[i] = open[i] && !acc[i];
  }
}

// The hunt of stage s >= 1: open[i] = edge 4q + i was refused in stage s - 1.  Draws its next target
// into p[i] as the stage-0 word is mapped (with replacement); open[i] stays set where the attempt
// is delivered, that is, where the target lies in n's partition block.
template <bool TOPO, bool FAULTS>
__device__ __forceinline__ void conn_hunt(const RoundArgs& a, const Reach& rc, uint32_t n, uint32_t b, uint32_t d,
                                          uint32_t q, uint32_t s, uint32_t (&p)[4], bool (&open)[4]) {
  const u32x4 hw = conn_hunt_draws(n, a.t, s, q, a.key0, a.key1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!open[i]) continue;
    p[i] = TOPO ? a.ocol[b + topo_index_from_word(lane_of(hw, i), d)] : peer_from_word(lane_of(hw, i), a.N - 1, n);
    if (FAULTS) open[i] = p[i] >= rc.lo && p[i] < rc.hi;
  }
}

// The resolve front end of the request kernels: p[4] and live[4] of resolve_batch (stage 0) become
// the accepted target of each edge, or live[i] = false where the edge was lost or finally refused.
template <bool TOPO, bool FAULTS>
__device__ __forceinline__ void conn_resolve(const ConnArgs& ca, const RoundArgs& a, const Reach& rc, uint32_t n,
                                             uint32_t b, uint32_t d, uint32_t q, uint32_t (&p)[4], bool (&live)[4]) {
  bool open[4], acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    open[i] = live[i];
    live[i] = false;
  }
  for (uint32_t s = 0;; ++s) {
    if (!(open[0] || open[1] || open[2] || open[3])) break;
    conn_verdicts(ca, a, n, q, s, p, open, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) live[i] = live[i] || acc[i];
    if (s == ca.h) break;
    conn_hunt<TOPO, FAULTS>(a, rc, n, b, d, q, s + 1u, p, open);
  }
}

// What the arbitration of one round reads: the round's arguments, the slots (all ones) and the
// counters (zero), and H_t where only hot nodes initiate (GOSSIP_FLAG_MONGER; else null).
struct ConnStageArgs {
  RoundArgs a;
  ConnArgs ca;
  const uint64_t* H;  // push: [W][N], a node initiates iff it has something hot; null: every node does
  bool topo;          // peers from the rows (an empty row initiates nothing) or from all N nodes
};

// Stages 0 .. h on the stream, one launch each, and one more that only counts the verdicts of stage
// h.  Fills ca.slots and ca.cnt; push (x.H set): adds the attempts to a.partial[2], the round's messages.
hipError_t launch_conn_arbitrate(const ConnStageArgs& x, hipStream_t st);

}  // namespace gossip
