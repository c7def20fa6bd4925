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
// (DESIGN.md §3.3).
#include "topo_peers.h"

namespace gossip {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ uint64_t full_mask(uint32_t R, uint32_t w) {
  const uint32_t bits = R - 64u * w;
  return bits >= 64u ? ~0ull : ((1ull << bits) - 1ull);
}

// index of word 0 of global node n in the gathered [G][W][Nl] image (word w: + w * Nl)
__device__ __forceinline__ uint64_t image_base(uint32_t n, uint64_t Nl, uint32_t W) {
  const uint32_t r = n / (uint32_t)Nl;
  return (uint64_t)r * W * Nl + (n - r * (uint32_t)Nl);
}

// Edges 4q .. 4q + cnt - 1 of sender n (row of d > 0 entries at ocol + b): the peers and
// whether each edge is live (drawn and not lost).  fa.stall is null here: a stalled sender
// never gets this far.
template <bool FAULTS>
__device__ __forceinline__ void resolve_batch(const RoundArgs& a, const Faults& fa, const Reach& rc, uint32_t n,
                                              uint32_t b, uint32_t d, uint32_t q, uint32_t cnt, uint32_t (&p)[4],
                                              bool (&live)[4]) {
  const u32x4 x = philox4x32_10(u32x4{n, a.t, 0u, q}, a.key0, a.key1);
  u32x4 lw{0, 0, 0, 0};
  if (FAULTS && fa.loss) lw = loss_draws(n, a.t, q, a.key0, a.key1);
  uint32_t idx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) idx[i] = topo_index_from_word(lane_of(x, i), d);
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = (uint32_t)i < cnt ? a.ocol[b + idx[i]] : n;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    live[i] = (uint32_t)i < cnt && !(FAULTS && edge_lost(fa, rc, p[i], lane_of(lw, i)));
}

// One batch of a one-word sender: pulls into acc, pushes into S_{t+1}.
template <bool PULL, bool PUSH, bool FAULTS>
__device__ __forceinline__ void batch_one_word(const RoundArgs& a, const Faults& fa, const Reach& rc, uint32_t n,
                                               bool own, uint64_t vs, uint32_t b, uint32_t d, uint32_t q,
                                               uint32_t cnt, uint64_t& acc) {
  uint32_t p[4];
  bool live[4], pown[4], need[4];
  resolve_batch<FAULTS>(a, fa, rc, n, b, d, q, cnt, p, live);
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
  resolve_batch<FAULTS>(a, fa, rc, n, b, d, q, cnt, p, live);
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
__global__ __launch_bounds__(kBlock) void round_topo_kernel(RoundArgs a, uint64_t s_begin, uint64_t s_end) {
  uint64_t msgs = 0;
  Faults fa = a.fa;
  fa.stall = nullptr;  // the partition block of a sender that is not stalled
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t s = s_begin + (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < s_end; s += stride) {
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
  msgs = wave_sum_u64(msgs);
  if ((threadIdx.x & 63) == 0 && msgs) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)msgs);
}

// Stall streaks after round t (DESIGN.md §2.9 over §2.10's peers): a node not yet stalled
// counts the round when any of its k exchanges was lost, else starts over; an empty row has
// no exchange to lose.  Draws and rows only: the streaks never depend on S.
__global__ __launch_bounds__(kBlock) void stall_update_topo_kernel(uint8_t* __restrict__ st, uint64_t N, uint32_t k,
                                                                   uint32_t t, uint32_t key0, uint32_t key1, Faults fa,
                                                                   const uint32_t* __restrict__ orow,
                                                                   const uint32_t* __restrict__ ocol) {
  fa.stall = nullptr;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t n = (uint32_t)i;
    const uint32_t c = st[i];
    if (c >= fa.D) continue;
    const uint32_t b = orow[n], d = orow[n + 1] - b;
    bool any = false;
    if (d) {
      const Reach rc = reach_of(n, fa);
      u32x4 x{0, 0, 0, 0}, lw{0, 0, 0, 0};
      for (uint32_t j = 0; j < k && !any; ++j) {
        if ((j & 3u) == 0) {
          x = philox4x32_10(u32x4{n, t, 0u, j >> 2}, key0, key1);
          if (fa.loss) lw = loss_draws(n, t, j >> 2, key0, key1);
        }
        const uint32_t p = ocol[b + topo_index_from_word(lane_of(x, j & 3u), d)];
        any = edge_lost(fa, rc, p, lane_of(lw, j & 3u));
      }
    }
    st[i] = (uint8_t)(any ? c + 1 : 0);
  }
}

// at most 8192 blocks, as the FLOOD launches: larger ranges take further trips of the stride loop
uint32_t grid_for(uint64_t work) {
  const uint64_t b = (work + kBlock - 1) / kBlock;
  return (uint32_t)(b == 0 ? 1 : (b < 8192 ? b : 8192));
}

template <bool ONE_WORD, bool FAULTS>
void launch_mode(const RoundArgs& a, bool pull, bool push, uint32_t grid, uint64_t sb, uint64_t se, hipStream_t st) {
  if (pull && push) round_topo_kernel<ONE_WORD, true, true, FAULTS><<<grid, kBlock, 0, st>>>(a, sb, se);
  else if (pull) round_topo_kernel<ONE_WORD, true, false, FAULTS><<<grid, kBlock, 0, st>>>(a, sb, se);
  else round_topo_kernel<ONE_WORD, false, true, FAULTS><<<grid, kBlock, 0, st>>>(a, sb, se);
}

}  // namespace

hipError_t launch_round_topo(const RoundArgs& a, hipStream_t st) {
  const bool pull = a.mode == 2 || a.mode == 3, push = a.mode == 1 || a.mode == 3;
  // pull-only rounds need only the owned senders; any push needs every sender
  const uint64_t sb = push ? 0 : a.lo, se = push ? a.N : a.lo + a.nown;
  const uint32_t grid = grid_for(se - sb);
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

hipError_t launch_stall_update_topo(uint8_t* stall, uint64_t N, uint32_t k, uint32_t t, uint32_t key0, uint32_t key1,
                                    const Faults& fa, const uint32_t* orow, const uint32_t* ocol, hipStream_t st) {
  stall_update_topo_kernel<<<grid_for(N), kBlock, 0, st>>>(stall, N, k, t, key0, key1, fa, orow, ocol);
  return hipGetLastError();
}

}  // namespace gossip
