// monger_pull.h — pull rumor mongering: every node asks k peers per round and
// is answered with the rumors the peer is still hot on; the node that loses interest is the server.
// An engine created with GOSSIP_FLAG_MONGER_PULL keeps S (known) and H ⊆ S (hot) in the layout of a
// GOSSIP_FLAG_MONGER engine (monger.h), the counters of §2.14 from the first limit above 1 on, and
// two feedback buffers in the same layout that are all zero between rounds.
//
// Reference: (*NodeState).Gossip forwards every value once (main.go:65-89); pull mongering with
// feedback and a counter is the strategy of Demers et al.'s third table ("Epidemic algorithms for
// replicated database maintenance"), whose footnote gives the rule of one counter step per cycle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "monger.h"

namespace gossip {

// One shard (G == 1): a.S is S_t, word w of node n at a.S[w * N + n]; a.Snext is written whole.
struct MongerPullArgs {
  RoundArgs a;         // S_t (a.S), S_{t+1} (a.Snext, no seed copy: the request pass writes every word), rows, faults, partial
  const uint64_t* H;   // H_t      [W][N]
  uint64_t* Hnext;     // H_{t+1}  [W][N], written whole by the request pass, cooled by the close pass
  uint64_t* need;      // [W][N] per server: the hot rumors some delivered request lacked; zero between rounds
  uint64_t* less;      // [W][N] per server: the hot rumors some delivered request held; zero between rounds
  uint64_t* hotmap;    // W > 1: bit n of word n / 64 = node n has something hot in H_t; the close pass
                       // rewrites it for H_{t+1}; bits past N are 0.  Null for W == 1
  uint64_t* hot_nodes; // the close pass adds the nodes with something hot in H_{t+1} (zeroed per round)
  uint32_t cool;       // the server's coin (stream tag 5, q = 0, word 0) holds when it is below this
  uint32_t blind;      // 0: feedback; 1: every delivered request counts every hot rumor as needless
  bool topo;           // peers drawn from the rows (GOSSIP_FLAG_TOPO_PEERS) or from all N nodes
  uint64_t* C;         // [4][W][N] counter planes (monger.h), or null: the engine holds no counters
  uint32_t limit;      // 1..15
  ConnArgs conn;       // connection limit: conn.c == 0 is the unlimited round (monger.h)
};

// The request pass: S_{t+1} and H_{t+1} with the replies in, the feedback in need / less, and the
// replies that carried a rumor added to a.partial[2].
hipError_t launch_round_monger_pull(const MongerPullArgs& m, hipStream_t st);
// The close pass (after the request pass on the same stream): the servers' coins, counters and cooling
// (§2.15 item 5), need / less back to zero, hotmap of H_{t+1}, and the hot nodes of H_{t+1}.
hipError_t launch_monger_pull_close(const MongerPullArgs& m, hipStream_t st);
// From H (either mongering flag): hotmap (ceil(N / 64) words, or null) rewritten, and the nodes with
// something hot added to *hot_nodes (zeroed by the caller; or null).  After an inject, and for
// gossip_monger_hot_nodes.
hipError_t launch_monger_hot_scan(const uint64_t* H, uint64_t N, uint32_t W, uint64_t* hotmap, uint64_t* hot_nodes,
                                  hipStream_t st);

}  // namespace gossip
