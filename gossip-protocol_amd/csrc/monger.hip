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
// coins, the peers and the loss draws; the last two are resolve_batch of sender.h, shared with that
// file), all draws first, then all row loads, then all S_t[p] gathers, then the deltas in registers,
// and only then the atomics — on gfx950 vmcnt retires in order, so a load consumed after an atomic
// was issued also waits for that atomic.
//
// blind is a run-time value, not a template parameter: the gather of S_t[p] decides which bits
// are new at p (and so hot there) in both variants, so a blind kernel would save no load.
//
// One kernel template serves both ways of cooling.  COUNT = false: a counted contact whose coin
// holds cools its rumors (§2.13).  COUNT = true: it adds one to their
// counts, and a rumor cools once its count reaches the limit.  Only an engine that holds counters
// (gossip_set_monger_limit above 1) launches a COUNT form; no other engine pays for the planes by
// a register, a load or a launch (§2.14 item 9).
//
// CONN: the engine holds a connection limit.  The arbitration of
// monger_conn.hip has run; conn_resolve turns the stage-0 peers of a batch into the accepted targets,
// and an edge that was refused for good is a lost one.  The unlimited forms keep their code.
#include "monger.h"

#include "planes.h"
#include "sender.h"

namespace gossip {

namespace {

// The coins of edges 4q .. 4q + cnt - 1 of sender n: whether each edge's coin holds.
__device__ __forceinline__ void draw_coins(const MongerArgs& m, uint32_t n, uint32_t q, uint32_t cnt,
                                           bool (&coin)[4]) {
  u32x4 cw{0, 0, 0, 0};
  if (m.cool) cw = cool_draws(n, m.a.t, q, m.a.key0, m.a.key1);  // (cool == 0: no word is below it)
#pragma unroll
  for (int i = 0; i < 4; ++i) coin[i] = (uint32_t)i < cnt && lane_of(cw, i) < m.cool;
}

// ---------------------------------------------------------------------------
// The counters: C[n][r] in 0..15 as four bit planes in the layout of S
// and H, so that one instruction updates 64 rumors.  Only lane n touches C[*][n]: plain loads and
// stores.  The planes of a word are loaded before the batch's atomics are issued and are consumed
// before them, as every other load of the batch.  planes_add and planes_ge are in planes.h.
// ---------------------------------------------------------------------------

// What one batch does to one word: h = that word of H_t[n] (not zero), woff = its offset in S and H.
// Returns the counted bits of the edges whose coin holds; COUNT: and adds each such edge's set to
// the planes c (in registers; not touched otherwise).
template <bool COUNT>
__device__ __forceinline__ uint64_t push_word(const MongerArgs& m, uint64_t h, uint64_t woff, const uint32_t (&p)[4],
                                              const bool (&live)[4], const bool (&coin)[4], uint64_t (&c)[4]) {
  const RoundArgs& a = m.a;
  uint64_t pv[4], nb[4], x[4], hit = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) pv[i] = live[i] ? a.G[woff + p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // a rumor the peer holds in S_t changes nothing there: the push is dropped, exactly
    nb[i] = live[i] ? (h & ~pv[i]) : 0ull;
    // feedback: the peer says what it held (nothing without a delivery); blind: every attempt counts
    const uint64_t counted = m.blind ? h : (live[i] ? (h & pv[i]) : 0ull);
    x[i] = coin[i] ? counted : 0ull;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (x[i]) {  // (the union inside the test: outside it the counter forms take 5 to 7 more VGPRs)
      if (COUNT) planes_add(c, x[i]);
      hit |= x[i];
    }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (nb[i]) {  // new at p: known there and hot there
      atomicOr((unsigned long long*)&a.Snext[woff + p[i]], (unsigned long long)nb[i]);
      atomicOr((unsigned long long*)&m.Hnext[woff + p[i]], (unsigned long long)nb[i]);
    }
  return hit;
}

// Ends a word (one word: after every batch; several: after each batch): at = its index in H, hit
// the union of what push_word returned.  The coin form cools all of hit.  COUNT: the incremented
// rumors whose count has reached the limit cool, and the planes go back only when something was
// counted; cooling per batch equals cooling per round: counts only grow
// within a round, and the last batch that increments a rumor sees its final count.
template <bool COUNT>
__device__ __forceinline__ void close_word(const MongerArgs& m, uint64_t at, uint64_t plane, uint64_t hit,
                                           const uint64_t (&c)[4]) {
  if (hit == 0) return;
  const uint64_t clear = COUNT ? planes_ge(c, m.limit) & hit : hit;
  // an atomic, not a store: other lanes OR new hot bits into the same word
  if (clear) atomicAnd((unsigned long long*)&m.Hnext[at], (unsigned long long)~clear);
  if (COUNT) {
#pragma unroll
    for (int b = 0; b < 4; ++b) m.C[(uint64_t)b * plane + at] = c[b];
  }
}

// ---------------------------------------------------------------------------
// The round.  Messages: k per node that initiates — something hot and,
// over the topology, a row that is not empty — whether or not an attempt is lost.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool TOPO, bool FAULTS, bool COUNT, bool CONN>
__global__ __launch_bounds__(kSenderBlock) void round_monger_kernel(MongerArgs m) {
  const RoundArgs& a = m.a;
  uint64_t msgs = 0;
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t plane = (uint64_t)a.W * a.N;
  const uint64_t stride = (uint64_t)gridDim.x * kSenderBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kSenderBlock + threadIdx.x; s < a.N; s += stride) {
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
    if (!CONN) msgs += a.k;  // (CONN: messages are the attempts, hunts included; the arbitration added them)
    const Reach rc = FAULTS ? reach_of(n, a.fa) : Reach{0u, 0xFFFFFFFFu};
    uint32_t p[4];
    bool live[4], coin[4];
    uint64_t c[4];
    if (ONE_WORD) {  // the cooled set, and the planes, stay in registers across the batches
      if (COUNT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = m.C[(uint64_t)i * plane + s];
      }
      uint64_t hit = 0;
      if (!COUNT && a.k <= 4u) {  // one unrolled batch; with the planes live it costs the counter forms a wave
        draw_coins(m, n, 0u, a.k, coin);
        resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, 0u, a.k, p, live);
        if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, 0u, p, live);
        hit = push_word<COUNT>(m, h, 0, p, live, coin, c);
      } else {
        for (uint32_t q = 0; q < nblk; ++q) {
          draw_coins(m, n, q, min(4u, a.k - 4u * q), coin);
          resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live);
          if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, q, p, live);
          hit |= push_word<COUNT>(m, h, 0, p, live, coin, c);
        }
      }
      close_word<COUNT>(m, s, plane, hit, c);
    } else {
      // the peers of a batch resolved once, then every word; a word is closed per batch (one AND per
      // word up to k = 4): AND commutes, and keeping W unions in registers does not scale
      for (uint32_t q = 0; q < nblk; ++q) {
        draw_coins(m, n, q, min(4u, a.k - 4u * q), coin);
        resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live);
        if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, q, p, live);
        for (uint32_t w = 0; w < a.W; ++w) {
          const uint64_t woff = (uint64_t)w * a.N;
          const uint64_t hw = m.H[woff + s];
          if (hw == 0) continue;
          if (COUNT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = m.C[(uint64_t)i * plane + woff + s];
          }
          const uint64_t hit = push_word<COUNT>(m, hw, woff, p, live, coin, c);
          close_word<COUNT>(m, woff + s, plane, hit, c);
        }
      }
    }
  }
  msgs = wave_sum64(msgs);
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

template <bool ONE_WORD, bool TOPO, bool FAULTS, bool CONN>
void launch_count(const MongerArgs& m, uint32_t grid, hipStream_t st) {
  if (m.C) round_monger_kernel<ONE_WORD, TOPO, FAULTS, true, CONN><<<grid, kSenderBlock, 0, st>>>(m);
  else round_monger_kernel<ONE_WORD, TOPO, FAULTS, false, CONN><<<grid, kSenderBlock, 0, st>>>(m);
}

template <bool ONE_WORD, bool TOPO, bool FAULTS>
void launch_conn(const MongerArgs& m, uint32_t grid, hipStream_t st) {
  if (m.conn.c) launch_count<ONE_WORD, TOPO, FAULTS, true>(m, grid, st);
  else launch_count<ONE_WORD, TOPO, FAULTS, false>(m, grid, st);
}

template <bool ONE_WORD, bool TOPO>
void launch_faults(const MongerArgs& m, uint32_t grid, hipStream_t st) {
  if (m.a.fa.any()) launch_conn<ONE_WORD, TOPO, true>(m, grid, st);
  else launch_conn<ONE_WORD, TOPO, false>(m, grid, st);
}

}  // namespace

hipError_t launch_round_monger(const MongerArgs& m, hipStream_t st) {
  const uint32_t grid = sender_grid(m.a.N);
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
  const uint32_t grid = node >= 0 ? 1 : (R + kSenderBlock - 1) / kSenderBlock;
  monger_inject_kernel<<<grid, kSenderBlock, 0, st>>>(S, H, N, R, key0, key1, node, rumor);
  return hipGetLastError();
}

}  // namespace gossip
