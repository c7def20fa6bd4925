// monger_pushpull.h — push-pull rumor mongering: every node starts k
// exchanges per round, both ends of a delivered exchange send what they are hot on, and both ends
// lose interest by what the other end told them.  An engine created with
// GOSSIP_FLAG_MONGER_PUSHPULL keeps S, H, the counters, the feedback buffers and the hot bitmap of a
// GOSSIP_FLAG_MONGER_PULL engine (monger_pull.h), and one buffer more: the gains of the round.
//
// Reference: (*NodeState).Gossip forwards every value once (main.go:65-89); push-pull mongering
// with feedback and a counter is the symmetric strategy of Demers et al. ("Epidemic algorithms for
// replicated database maintenance", §1.4), and the round Karp et al.'s "Randomized rumor
// spreading" analyses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "monger_pull.h"

namespace gossip {

// One shard (G == 1).  m is read as in monger_pull.h, except that the request pass writes neither
// next image: m.a.Snext and m.Hnext are written whole by the close pass.
struct MongerPushPullArgs {
  MongerPullArgs m;
  uint64_t* gain;  // [W][N] per node: the rumors some delivered exchange brought that it lacked; zero between rounds
};

// The request pass: gains and feedback of both ends of every delivered exchange ORed into gain /
// need / less, and the delivered exchanges with a hot end added to m.a.partial[2].
hipError_t launch_round_monger_pushpull(const MongerPushPullArgs& x, hipStream_t st);
// The close pass (after the request pass on the same stream): S_{t+1} = S_t | gain, the coins,
// counters and cooling (§2.16 item 5), H_{t+1}, gain / need / less back to zero, hotmap of H_{t+1},
// and the hot nodes of H_{t+1}.
hipError_t launch_monger_pushpull_close(const MongerPushPullArgs& x, hipStream_t st);

}  // namespace gossip
