// monger.hip — the rumor-mongering round, written for gfx950 (CDNA4, wave64).
//
// Reference hot path: (*NodeState).Gossip, main.go:65-89, forwards a value once and is done with
// it; here a node keeps pushing the rumors it is still hot on to k peers per round and drops one
// when a counted contact's coin says so.  All reads are of S_t and H_t, S_{t+1} and H_{t+1} start
// as copies; a node gains only bits outside S_t[n] (atomic ORs) and loses only bits inside
// H_t[n] ⊆ S_t[n] (one atomic AND), so the result does not depend on the schedule.
//
// One lane per sender over all N nodes.  H_t[n] == 0 is the early exit: late in a run that is
// almost every lane, and it costs one coalesced 8-byte load per word.  A hot sender follows the
// batch shape of topo_peers.hip: the edges in batches of four (one Philox block each for the
// peers, the loss draws and the coins), all draws first, then all row loads, then all S_t[p]
// gathers, then the deltas in registers, and only then the atomics — on gfx950 vmcnt retires in
// order, so a load consumed after an atomic was issued also waits for that atomic.
//
// blind is a run-time value, not a template parameter: the gather of S_t[p] decides which bits
// are new at p (and so hot there) in both variants, so a blind kernel would save no load.
//
// An engine that holds counters (gossip_set_monger_limit above 1) runs the sibling
// round_monger_count_kernel; every other engine launches round_monger_kernel as before.
#include "monger.h"

#include "topo_peers.h"

namespace gossip {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Edges 4q .. 4q + cnt - 1 of sender n: the peers, whether each push is delivered (drawn and not
// lost) and whether each edge's coin holds.  TOPO: the row of d > 0 entries at ocol + b.
template <bool TOPO, bool FAULTS>
__device__ __forceinline__ void resolve_batch(const MongerArgs& m, const Reach& rc, uint32_t n, uint32_t b, uint32_t d,
                                              uint32_t q, uint32_t cnt, uint32_t (&p)[4], bool (&live)[4],
                                              bool (&coin)[4]) {
  const RoundArgs& a = m.a;
  const u32x4 x = philox4x32_10(u32x4{n, a.t, 0u, q}, a.key0, a.key1);
  u32x4 lw{0, 0, 0, 0}, cw{0, 0, 0, 0};
  if (FAULTS && a.fa.loss) lw = loss_draws(n, a.t, q, a.key0, a.key1);
  if (m.cool) cw = cool_draws(n, a.t, q, a.key0, a.key1);  // (cool == 0: no word is below it)
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
  for (int i = 0; i < 4; ++i) {
    live[i] = (uint32_t)i < cnt && !(FAULTS && edge_lost(a.fa, rc, p[i], lane_of(lw, i)));
    coin[i] = (uint32_t)i < cnt && lane_of(cw, i) < m.cool;
  }
}

// What one batch does to one word: h = that word of H_t[n] (not zero), woff = its offset in S and H.
// Returns the bits the batch cools at n.
__device__ __forceinline__ uint64_t push_word(const MongerArgs& m, uint64_t h, uint64_t woff, const uint32_t (&p)[4],
                                              const bool (&live)[4], const bool (&coin)[4]) {
  const RoundArgs& a = m.a;
  uint64_t pv[4], nb[4], clear = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) pv[i] = live[i] ? a.G[woff + p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // a rumor the peer holds in S_t changes nothing there: the push is dropped, exactly
    nb[i] = live[i] ? (h & ~pv[i]) : 0ull;
    // feedback: the peer says what it held (nothing without a delivery); blind: every attempt counts
    const uint64_t counted = m.blind ? h : (live[i] ? (h & pv[i]) : 0ull);
    if (coin[i]) clear |= counted;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (nb[i]) {  // new at p: known there and hot there
      atomicOr((unsigned long long*)&a.Snext[woff + p[i]], (unsigned long long)nb[i]);
      atomicOr((unsigned long long*)&m.Hnext[woff + p[i]], (unsigned long long)nb[i]);
    }
  return clear;
}

// ---------------------------------------------------------------------------
// The round.  Messages: k per node that initiates — something hot and,
// over the topology, a row that is not empty — whether or not an attempt is lost.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool TOPO, bool FAULTS>
__global__ __launch_bounds__(kBlock) void round_monger_kernel(MongerArgs m) {
  const RoundArgs& a = m.a;
  uint64_t msgs = 0;
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < a.N; s += stride) {
    const uint32_t n = (uint32_t)s;
    uint64_t h = 0;
    if (ONE_WORD) {
      h = m.H[s];
    } else {
      for (uint32_t w = 0; w < a.W; ++w) h |= m.H[(uint64_t)w * a.N + s];
    }
    if (h == 0) continue;  // nothing hot: neither a push nor a message
    uint32_t b = 0, d = 0;
    if (TOPO) {
      b = a.orow[n];
      d = a.orow[n + 1] - b;
      if (d == 0) continue;
    }
    msgs += a.k;
    const Reach rc = FAULTS ? reach_of(n, a.fa) : Reach{0u, 0xFFFFFFFFu};
    uint32_t p[4];
    bool live[4], coin[4];
    if (ONE_WORD) {
      uint64_t clear = 0;
      if (a.k <= 4u) {
        resolve_batch<TOPO, FAULTS>(m, rc, n, b, d, 0u, a.k, p, live, coin);
        clear = push_word(m, h, 0, p, live, coin);
      } else {
        for (uint32_t q = 0; q < nblk; ++q) {
          resolve_batch<TOPO, FAULTS>(m, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live, coin);
          clear |= push_word(m, h, 0, p, live, coin);
        }
      }
      // an atomic, not a store: other lanes OR new hot bits into the same word
      if (clear) atomicAnd((unsigned long long*)&m.Hnext[s], (unsigned long long)~clear);
    } else {
      // the peers of a batch resolved once, then every word; a word's cooled bits go out per batch
      // (one AND per word up to k = 4): AND commutes, and keeping W unions in registers does not scale
      for (uint32_t q = 0; q < nblk; ++q) {
        resolve_batch<TOPO, FAULTS>(m, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live, coin);
        for (uint32_t w = 0; w < a.W; ++w) {
          const uint64_t woff = (uint64_t)w * a.N;
          const uint64_t hw = m.H[woff + s];
          if (hw == 0) continue;
          const uint64_t clear = push_word(m, hw, woff, p, live, coin);
          if (clear) atomicAnd((unsigned long long*)&m.Hnext[woff + s], (unsigned long long)~clear);
        }
      }
    }
  }
  msgs = wave_sum_u64(msgs);
  if ((threadIdx.x & 63) == 0 && msgs) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)msgs);
}

// ---------------------------------------------------------------------------
// The round with counters: C[n][r] in 0..15 as four bit planes in the
// layout of S and H, so that one instruction updates 64 rumors.  Only lane n touches C[*][n]: plain
// loads and stores.  The planes of a word are loaded before the batch's atomics are issued and are
// consumed before them, as every other load of the batch.
// ---------------------------------------------------------------------------

// c += 1 at the bits of x, saturating at 15: a ripple-carry add over the planes; a carry out of
// plane 3 sets all four planes of those bits.
__device__ __forceinline__ void planes_add(uint64_t (&c)[4], uint64_t x) {
  uint64_t carry = x;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint64_t t = c[b] & carry;
    c[b] ^= carry;
    carry = t;
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) c[b] |= carry;
}

// The bits whose count is at least limit (uniform, 1..15), most significant plane first.
__device__ __forceinline__ uint64_t planes_ge(const uint64_t (&c)[4], uint32_t limit) {
  uint64_t gt = 0, eq = ~0ull;
#pragma unroll
  for (int b = 3; b >= 0; --b) {
    if ((limit >> b) & 1u) {
      eq &= c[b];
    } else {
      gt |= eq & c[b];
      eq &= ~c[b];
    }
  }
  return gt | eq;
}

// What one batch does to one word of a counting engine: push_word, but an edge whose coin holds adds
// its counted set to the planes c (in registers).  Returns the bits that were incremented.
__device__ __forceinline__ uint64_t count_word(const MongerArgs& m, uint64_t h, uint64_t woff, const uint32_t (&p)[4],
                                               const bool (&live)[4], const bool (&coin)[4], uint64_t (&c)[4]) {
  const RoundArgs& a = m.a;
  uint64_t pv[4], nb[4], x[4], inc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) pv[i] = live[i] ? a.G[woff + p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    nb[i] = live[i] ? (h & ~pv[i]) : 0ull;
    const uint64_t counted = m.blind ? h : (live[i] ? (h & pv[i]) : 0ull);
    x[i] = coin[i] ? counted : 0ull;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (x[i]) {
      planes_add(c, x[i]);
      inc |= x[i];
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (nb[i]) {
      atomicOr((unsigned long long*)&a.Snext[woff + p[i]], (unsigned long long)nb[i]);
      atomicOr((unsigned long long*)&m.Hnext[woff + p[i]], (unsigned long long)nb[i]);
    }
  return inc;
}

// Ends a word (one word: after every batch; several: after each): the incremented rumors whose count
// has reached the limit cool, and the planes go back only when something was counted.  Cooling per
// batch equals cooling per round: counts only grow within a round, and
// the last batch that increments a rumor sees its final count.
__device__ __forceinline__ void count_close(const MongerCountArgs& ca, uint64_t at, uint64_t plane, uint64_t inc,
                                            const uint64_t (&c)[4]) {
  if (inc == 0) return;
  const uint64_t clear = planes_ge(c, ca.limit) & inc;
  if (clear) atomicAnd((unsigned long long*)&ca.m.Hnext[at], (unsigned long long)~clear);
#pragma unroll
  for (int b = 0; b < 4; ++b) ca.C[(uint64_t)b * plane + at] = c[b];
}

template <bool ONE_WORD, bool TOPO, bool FAULTS>
__global__ __launch_bounds__(kBlock) void round_monger_count_kernel(MongerCountArgs ca) {
  const MongerArgs& m = ca.m;
  const RoundArgs& a = m.a;
  uint64_t msgs = 0;
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t plane = (uint64_t)a.W * a.N;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < a.N; s += stride) {
    const uint32_t n = (uint32_t)s;
    uint64_t h = 0;
    if (ONE_WORD) {
      h = m.H[s];
    } else {
      for (uint32_t w = 0; w < a.W; ++w) h |= m.H[(uint64_t)w * a.N + s];
    }
    if (h == 0) continue;  // nothing hot: no push, no message, and no plane is read
    uint32_t b = 0, d = 0;
    if (TOPO) {
      b = a.orow[n];
      d = a.orow[n + 1] - b;
      if (d == 0) continue;
    }
    msgs += a.k;
    const Reach rc = FAULTS ? reach_of(n, a.fa) : Reach{0u, 0xFFFFFFFFu};
    uint32_t p[4];
    bool live[4], coin[4];
    uint64_t c[4];
    if (ONE_WORD) {  // the planes stay in registers across the batches
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = ca.C[(uint64_t)i * plane + s];
      uint64_t inc = 0;
      for (uint32_t q = 0; q < nblk; ++q) {
        resolve_batch<TOPO, FAULTS>(m, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live, coin);
        inc |= count_word(m, h, 0, p, live, coin, c);
      }
      count_close(ca, s, plane, inc, c);
    } else {  // per word and batch, as the AND of round_monger_kernel
      for (uint32_t q = 0; q < nblk; ++q) {
        resolve_batch<TOPO, FAULTS>(m, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live, coin);
        for (uint32_t w = 0; w < a.W; ++w) {
          const uint64_t woff = (uint64_t)w * a.N;
          const uint64_t hw = m.H[woff + s];
          if (hw == 0) continue;
#pragma unroll
          for (int i = 0; i < 4; ++i) c[i] = ca.C[(uint64_t)i * plane + woff + s];
          const uint64_t inc = count_word(m, hw, woff, p, live, coin, c);
          count_close(ca, woff + s, plane, inc, c);
        }
      }
    }
  }
  msgs = wave_sum_u64(msgs);
  if ((threadIdx.x & 63) == 0 && msgs) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)msgs);
}

__global__ void monger_inject_kernel(uint64_t* S, uint64_t* H, uint64_t N, uint32_t R, uint32_t key0, uint32_t key1,
                                     int64_t node, uint32_t rumor) {
  const uint32_t r = node >= 0 ? rumor : blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= 0 && (blockIdx.x | threadIdx.x)) return;
  if (r >= R) return;
  const uint64_t n = node >= 0 ? (uint64_t)node : origin_of(r, N, key0, key1);
  if (n >= N) return;
  const uint64_t bit = 1ull << (r & 63), at = (uint64_t)(r >> 6) * N + n;
  const uint64_t old = atomicOr((unsigned long long*)&S[at], (unsigned long long)bit);
  if (!(old & bit)) atomicOr((unsigned long long*)&H[at], (unsigned long long)bit);  // held: not re-heated
}

// at most 8192 blocks, as the other direct launches: larger ranges take further trips of the stride loop
uint32_t grid_for(uint64_t work) {
  const uint64_t b = (work + kBlock - 1) / kBlock;
  return (uint32_t)(b == 0 ? 1 : (b < 8192 ? b : 8192));
}

template <bool ONE_WORD, bool TOPO>
void launch_faults(const MongerArgs& m, uint32_t grid, hipStream_t st) {
  if (m.a.fa.any()) round_monger_kernel<ONE_WORD, TOPO, true><<<grid, kBlock, 0, st>>>(m);
  else round_monger_kernel<ONE_WORD, TOPO, false><<<grid, kBlock, 0, st>>>(m);
}

template <bool ONE_WORD, bool TOPO>
void launch_count_faults(const MongerCountArgs& c, uint32_t grid, hipStream_t st) {
  if (c.m.a.fa.any()) round_monger_count_kernel<ONE_WORD, TOPO, true><<<grid, kBlock, 0, st>>>(c);
  else round_monger_count_kernel<ONE_WORD, TOPO, false><<<grid, kBlock, 0, st>>>(c);
}

}  // namespace

hipError_t launch_round_monger_count(const MongerCountArgs& c, hipStream_t st) {
  const uint32_t grid = grid_for(c.m.a.N);
  if (c.m.a.W == 1) {
    if (c.m.topo) launch_count_faults<true, true>(c, grid, st);
    else launch_count_faults<true, false>(c, grid, st);
  } else {
    if (c.m.topo) launch_count_faults<false, true>(c, grid, st);
    else launch_count_faults<false, false>(c, grid, st);
  }
  return hipGetLastError();
}

hipError_t launch_round_monger(const MongerArgs& m, hipStream_t st) {
  const uint32_t grid = grid_for(m.a.N);
  if (m.a.W == 1) {
    if (m.topo) launch_faults<true, true>(m, grid, st);
    else launch_faults<true, false>(m, grid, st);
  } else {
    if (m.topo) launch_faults<false, true>(m, grid, st);
    else launch_faults<false, false>(m, grid, st);
  }
  return hipGetLastError();
}

hipError_t launch_monger_inject(uint64_t* S, uint64_t* H, uint64_t N, uint32_t R, uint32_t key0, uint32_t key1,
                                int64_t node, uint32_t rumor, hipStream_t st) {
  const uint32_t grid = node >= 0 ? 1 : (R + kBlock - 1) / kBlock;
  monger_inject_kernel<<<grid, kBlock, 0, st>>>(S, H, N, R, key0, key1, node, rumor);
  return hipGetLastError();
}

}  // namespace gossip
