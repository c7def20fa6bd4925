// topo_peers.hip — random gossip over the topology, written for gfx950 (CDNA4, wave64).
//
// Reference hot path: (*NodeState).Gossip, main.go:65-89, which ranges over
// Topology[node.ID()] (:72) and sends to every neighbour.  Here each node draws k of its
// neighbours per round: i_j = floor(x_j * deg / 2^32) from the Philox word
// of §2.2, p_j = row[i_j], and PUSH / PULL / PUSHPULL read §2.4 with these peers.  All reads
// are of S_t (the gathered image), all writes atomic ORs into S_{t+1}, so the result does not
// depend on the schedule.
//
// One lane per sender, the edges in batches of four (one Philox block).  Inside a batch the
// draws come first, then every row load is issued before one is consumed, then every S_t
// gather, then the deltas in registers, and only then the atomics: on gfx950 vmcnt retires in
// order, so a load consumed after an atomic was issued also waits for that atomic
// (DESIGN.md §3.3).  The draws and row loads of a batch are resolve_batch<true, FAULTS> of
// sender.h, which the mongering round (monger.hip) shares; its fault block here has a null
// stall array, since a stalled sender never gets that far.
#include "topo_peers.h"

#include "sender.h"

namespace gossip {

namespace {

// One batch of a one-word sender: pulls into acc, pushes into S_{t+1}.
template <bool PULL, bool PUSH, bool FAULTS>
__device__ __forceinline__ void batch_one_word(const RoundArgs& a, const Faults& fa, const Reach& rc, uint32_t n,
                                               bool own, uint64_t vs, uint32_t b, uint32_t d, uint32_t q,
                                               uint32_t cnt, uint64_t& acc) {
  uint32_t p[4];
  bool live[4], pown[4], need[4];
  resolve_batch<true, FAULTS>(a, fa, rc, n, b, d, q, cnt, p, live);
  uint64_t pv[4], nb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pown[i] = ((uint64_t)p[i] - a.lo) < a.nown;
    need[i] = live[i] && ((PULL && own) || (PUSH && pown[i] && vs != 0));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) pv[i] = need[i] ? a.G[p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (PULL && own) acc |= pv[i];
    // a push whose bits the peer holds in S_t cannot change S_{t+1}: dropped, exactly
    nb[i] = (PUSH && need[i] && pown[i]) ? (vs & ~pv[i]) : 0ull;
  }
  if (PUSH) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (nb[i]) atomicOr((unsigned long long*)&a.Snext[p[i] - a.lo], (unsigned long long)nb[i]);
  }
}

// One batch of a sender with W > 1 words: the peers resolved once, then every word.
template <bool PULL, bool PUSH, bool FAULTS>
__device__ __forceinline__ void batch_words(const RoundArgs& a, const Faults& fa, const Reach& rc, uint32_t n, bool own,
                                            uint64_t sbase, uint32_t b, uint32_t d, uint32_t q, uint32_t cnt) {
  uint32_t p[4];
  bool live[4], pown[4];
  resolve_batch<true, FAULTS>(a, fa, rc, n, b, d, q, cnt, p, live);
  uint64_t pbase[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pown[i] = ((uint64_t)p[i] - a.lo) < a.nown;
    pbase[i] = image_base(p[i], a.Nl, a.W);
  }
  for (uint32_t w = 0; w < a.W; ++w) {
    const uint64_t vs = a.G[sbase + (uint64_t)w * a.Nl];
    bool need[4];
    uint64_t pv[4], nb[4], acc = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) need[i] = live[i] && ((PULL && own) || (PUSH && pown[i] && vs != 0));
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i] = need[i] ? a.G[pbase[i] + (uint64_t)w * a.Nl] : 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (PULL && own) acc |= pv[i];
      nb[i] = (PUSH && need[i] && pown[i]) ? (vs & ~pv[i]) : 0ull;
    }
    if (PUSH) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (nb[i])
          atomicOr((unsigned long long*)&a.Snext[(uint64_t)w * a.Nl + (p[i] - a.lo)], (unsigned long long)nb[i]);
    }
    if (PULL && own) {
      const uint64_t nw = acc & ~vs;
      if (nw) atomicOr((unsigned long long*)&a.Snext[(uint64_t)w * a.Nl + (n - a.lo)], (unsigned long long)nw);
    }
  }
}

// ---------------------------------------------------------------------------
// The round.  Senders [s_begin, s_end): all N when the mode pushes (a sender of another
// shard may push into an owned node), the owned ones for PULL.  Messages:
// k per owned sender that initiates — a row that is not empty, not stalled and, for PUSH,
// something to send — whether or not an attempt is lost.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool PULL, bool PUSH, bool FAULTS>
__global__ __launch_bounds__(kSenderBlock) void round_topo_kernel(RoundArgs a, uint64_t s_begin, uint64_t s_end) {
  uint64_t msgs = 0;
  Faults fa = a.fa;
  fa.stall = nullptr;  // the partition block of a sender that is not stalled
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * kSenderBlock;
  for (uint64_t s = s_begin + (uint64_t)blockIdx.x * kSenderBlock + threadIdx.x; s < s_end; s += stride) {
    const uint32_t n = (uint32_t)s;
    const bool own = (s - a.lo) < a.nown;
    uint64_t vs = 0, sbase = s;
    bool nz, full;
    if (ONE_WORD) {
      vs = a.G[s];
      nz = vs != 0;
      const uint64_t fm = full_mask(a.R, 0);
      full = (vs & fm) == fm;
    } else {
      sbase = image_base(n, a.Nl, a.W);
      nz = false;
      full = true;
      for (uint32_t w = 0; w < a.W; ++w) {
        const uint64_t v = a.G[sbase + (uint64_t)w * a.Nl], fm = full_mask(a.R, w);
        nz = nz || v != 0;
        full = full && (v & fm) == fm;
      }
    }
    // nothing to push and nobody to pull for: neither an exchange nor a message
    if (!nz && (!PULL || !own)) continue;
    const uint32_t b = a.orow[n], d = a.orow[n + 1] - b;
    if (d == 0) continue;
    if (FAULTS && a.fa.stall && a.fa.stall[n] >= a.fa.D) continue;  // stalled: initiates nothing
    if (own) msgs += a.k;
    if (!PUSH && full) continue;  // a full row pulls nothing new
    const Reach rc = FAULTS ? reach_of(n, fa) : Reach{0u, 0xFFFFFFFFu};
    if (ONE_WORD) {
      uint64_t acc = 0;
      if (a.k <= 4u) {
        batch_one_word<PULL, PUSH, FAULTS>(a, fa, rc, n, own, vs, b, d, 0u, a.k, acc);
      } else {
        for (uint32_t q = 0; q < nblk; ++q)
          batch_one_word<PULL, PUSH, FAULTS>(a, fa, rc, n, own, vs, b, d, q, min(4u, a.k - 4u * q), acc);
      }
      if (PULL && own) {
        const uint64_t nw = acc & ~vs;
        if (nw) atomicOr((unsigned long long*)&a.Snext[s - a.lo], (unsigned long long)nw);
      }
    } else {
      for (uint32_t q = 0; q < nblk; ++q)
        batch_words<PULL, PUSH, FAULTS>(a, fa, rc, n, own, sbase, b, d, q, min(4u, a.k - 4u * q));
    }
  }
  msgs = wave_sum64(msgs);
  if ((threadIdx.x & 63) == 0 && msgs) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)msgs);
}

template <bool ONE_WORD, bool FAULTS>
void launch_mode(const RoundArgs& a, bool pull, bool push, uint32_t grid, uint64_t sb, uint64_t se, hipStream_t st) {
  if (pull && push) round_topo_kernel<ONE_WORD, true, true, FAULTS><<<grid, kSenderBlock, 0, st>>>(a, sb, se);
  else if (pull) round_topo_kernel<ONE_WORD, true, false, FAULTS><<<grid, kSenderBlock, 0, st>>>(a, sb, se);
  else round_topo_kernel<ONE_WORD, false, true, FAULTS><<<grid, kSenderBlock, 0, st>>>(a, sb, se);
}

}  // namespace

hipError_t launch_round_topo(const RoundArgs& a, hipStream_t st) {
  const bool pull = a.mode == 2 || a.mode == 3, push = a.mode == 1 || a.mode == 3;
  // pull-only rounds need only the owned senders; any push needs every sender
  const uint64_t sb = push ? 0 : a.lo, se = push ? a.N : a.lo + a.nown;
  const uint32_t grid = sender_grid(se - sb);
  const bool faults = a.fa.any();
  if (a.W == 1) {
    if (faults) launch_mode<true, true>(a, pull, push, grid, sb, se, st);
    else launch_mode<true, false>(a, pull, push, grid, sb, se, st);
  } else {
    if (faults) launch_mode<false, true>(a, pull, push, grid, sb, se, st);
    else launch_mode<false, false>(a, pull, push, grid, sb, se, st);
  }
  return hipGetLastError();
}

}  // namespace gossip
