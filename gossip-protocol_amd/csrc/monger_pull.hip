// monger_pull.hip — the pull rumor-mongering round, written for gfx950
// (CDNA4, wave64).
//
// Reference hot path: (*NodeState).Gossip, main.go:65-89, forwards a value once and is done with it;
// here every node asks k peers per round, a peer answers with the rumors it is still hot on, and
// it is the peer — the server — that loses interest, by what all the requests that reached it in the
// round told it.  All reads are of S_t, H_t and C_t.
//
// Two passes.  The request pass has one lane per requester.  The requester owns its gains: they go
// to its own words of S_{t+1} and H_{t+1} with plain stores (the pass writes both images whole, so
// there is no seed copy).  Only the feedback scatters: two ORs per served word into need / less at
// the server, and only where they are not zero — a peer with nothing hot costs no atomic.  The
// edges go in batches of four as in monger.hip (resolve_batch of sender.h): all draws first, then the
// row loads, then the gathers of H_t[p], then the deltas in registers, and only then the atomics —
// on gfx950 vmcnt retires in order, so a load consumed after an atomic was issued also waits for
// that atomic.  The close pass has one lane per node: where a feedback word is set
// it draws the server's coin, applies the rule of one counter step per round and clears the word.
// Gains lie outside S_t[n] ⊇ H_t[n], losses inside H_t[p], need and less are ORs: the result does not
// depend on the schedule.
//
// blind is a run-time value, as in monger.hip: both variants gather H_t[p].
//
// CONN: as in monger.hip, conn_resolve replaces the stage-0 peers of a batch
// by the accepted targets; "delivered" then reads "accepted".  The unlimited forms keep their code.
#include "monger_pull.h"

#include "monger_close.h"
#include "sender.h"

namespace gossip {

namespace {

// What one batch does to one word: sv = that word of S_t[n], woff = its offset in the [W][N] arrays,
// ask[i] = the request was delivered (several words: and the server has something hot).  Returns the
// union of the replies; replies != null: counts the edges whose reply carried a rumor.
__device__ __forceinline__ uint64_t pull_word(const MongerPullArgs& m, uint64_t sv, uint64_t woff,
                                              const uint32_t (&p)[4], const bool (&ask)[4], uint64_t* replies) {
  uint64_t hp[4], nd[4], ls[4], gain = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) hp[i] = ask[i] ? m.H[woff + p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // feedback: the requester says which of the reply it lacked and which it held; blind: it says
    // nothing, and the server counts the request against everything it sent
    nd[i] = m.blind ? 0ull : hp[i] & ~sv;
    ls[i] = m.blind ? hp[i] : hp[i] & sv;
    gain |= hp[i];
    if (replies) *replies += hp[i] != 0;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (nd[i]) atomicOr((unsigned long long*)&m.need[woff + p[i]], (unsigned long long)nd[i]);
    if (ls[i]) atomicOr((unsigned long long*)&m.less[woff + p[i]], (unsigned long long)ls[i]);
  }
  return gain;
}

// ---------------------------------------------------------------------------
// The request pass.  Messages: the delivered requests whose server had
// something hot.  A full node asks too: it cannot know that it lacks nothing, and its answer is
// the feedback that cools the server.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool TOPO, bool FAULTS, bool CONN>
__global__ __launch_bounds__(kSenderBlock) void round_monger_pull_kernel(MongerPullArgs m) {
  const RoundArgs& a = m.a;
  uint64_t msgs = 0;
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * kSenderBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kSenderBlock + threadIdx.x; s < a.N; s += stride) {
    const uint32_t n = (uint32_t)s;
    uint32_t b = 0, d = 0;
    if (TOPO) {
      b = a.orow[n];
      d = a.orow[n + 1] - b;
    }
    const bool asks = !TOPO || d != 0;  // an empty row asks nobody; its words are carried over below
    const Reach rc = FAULTS ? reach_of(n, a.fa) : Reach{0u, 0xFFFFFFFFu};
    uint32_t p[4];
    bool live[4];
    if (ONE_WORD) {  // the gains stay in a register across the batches: one store per image
      const uint64_t sv = a.S[s], hv = m.H[s];
      uint64_t gain = 0;
      if (asks) {
        for (uint32_t q = 0; q < nblk; ++q) {
          resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live);
          if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, q, p, live);
          gain |= pull_word(m, sv, 0, p, live, &msgs);
        }
      }
      a.Snext[s] = sv | gain;
      m.Hnext[s] = hv | (gain & ~sv);  // new here: known here and hot here
    } else {
      for (uint32_t w = 0; w < a.W; ++w) {
        const uint64_t at = (uint64_t)w * a.N + s;
        a.Snext[at] = a.S[at];
        m.Hnext[at] = m.H[at];
      }
      if (!asks) continue;
      // the peers of a batch resolved once and probed in the bitmap of H_t: late in a run every probe
      // says no, and k probes replace k * W gathers.  Own words are read back: only this lane writes them
      for (uint32_t q = 0; q < nblk; ++q) {
        resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live);
        if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, q, p, live);
        uint64_t bits[4];
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) bits[i] = live[i] ? m.hotmap[p[i] >> 6] : 0ull;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          live[i] = (bits[i] >> (p[i] & 63u)) & 1ull;
          any = any || live[i];
          msgs += live[i];
        }
        if (!any) continue;
        for (uint32_t w = 0; w < a.W; ++w) {
          const uint64_t woff = (uint64_t)w * a.N;
          const uint64_t sv = a.S[woff + s];
          const uint64_t gain = pull_word(m, sv, woff, p, live, nullptr);
          if (gain & ~sv) {
            a.Snext[woff + s] |= gain;
            m.Hnext[woff + s] |= gain & ~sv;
          }
        }
      }
    }
  }
  msgs = wave_sum64(msgs);
  if ((threadIdx.x & 63) == 0 && msgs) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)msgs);
}

// ---------------------------------------------------------------------------
// The close pass, after the request pass has finished: plain loads
// and stores, lane n alone touches the words of node n.  One coin per node and round, drawn where a
// feedback word is set.  A needed rumor's count goes back to 0 and nothing else happens to it; a
// rumor that was only needless, under a coin that holds, is counted once and cools at the limit.
// While a rumor is hot its count is below the limit, so planes_add never saturates here.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool COUNT>
__global__ __launch_bounds__(kSenderBlock) void monger_pull_close_kernel(MongerPullArgs m) {
  const RoundArgs& a = m.a;
  const uint32_t W = ONE_WORD ? 1u : a.W;
  const uint64_t plane = (uint64_t)a.W * a.N;
  uint64_t hot_nodes = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kSenderBlock;
  // whole waves walk the range (the ballot below), 64 consecutive nodes from a multiple of 64 each
  for (uint64_t base = (uint64_t)blockIdx.x * kSenderBlock; base < a.N; base += stride) {
    const uint64_t s = base + threadIdx.x;
    bool hot = false;
    if (s < a.N) {
      int coin = -1;  // not drawn yet
      for (uint32_t w = 0; w < W; ++w) {
        const uint64_t at = (uint64_t)w * a.N + s;
        const uint64_t nd = m.need[at], ls = m.less[at];
        uint64_t hn = m.Hnext[at];
        if (nd | ls) {
          if (nd) m.need[at] = 0;
          if (ls) m.less[at] = 0;
          const uint64_t clear = monger_cool_word<COUNT>(m, s, at, plane, nd, ls, coin);  // (monger_close.h)
          if (clear) {
            hn &= ~clear;
            m.Hnext[at] = hn;
          }
        }
        hot = hot || hn != 0;
      }
    }
    const uint64_t bal = __ballot(hot);  // lanes past N vote no: the bits past N are 0
    if ((threadIdx.x & 63) == 0 && s < a.N) {
      hot_nodes += (uint64_t)__popcll(bal);
      if (!ONE_WORD) m.hotmap[s >> 6] = bal;
    }
  }
  if (hot_nodes) atomicAdd((unsigned long long*)m.hot_nodes, (unsigned long long)hot_nodes);
}

__global__ __launch_bounds__(kSenderBlock) void monger_hot_scan_kernel(const uint64_t* H, uint64_t N, uint32_t W,
                                                                       uint64_t* hotmap, uint64_t* hot_nodes) {
  uint64_t cnt = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kSenderBlock;
  for (uint64_t base = (uint64_t)blockIdx.x * kSenderBlock; base < N; base += stride) {
    const uint64_t s = base + threadIdx.x;
    bool hot = false;
    if (s < N)
      for (uint32_t w = 0; w < W; ++w) hot = hot || H[(uint64_t)w * N + s] != 0;
    const uint64_t bal = __ballot(hot);
    if ((threadIdx.x & 63) == 0 && s < N) {
      cnt += (uint64_t)__popcll(bal);
      if (hotmap) hotmap[s >> 6] = bal;
    }
  }
  if (hot_nodes && cnt) atomicAdd((unsigned long long*)hot_nodes, (unsigned long long)cnt);
}

template <bool ONE_WORD, bool TOPO, bool FAULTS>
void launch_conn(const MongerPullArgs& m, uint32_t grid, hipStream_t st) {
  if (m.conn.c) round_monger_pull_kernel<ONE_WORD, TOPO, FAULTS, true><<<grid, kSenderBlock, 0, st>>>(m);
  else round_monger_pull_kernel<ONE_WORD, TOPO, FAULTS, false><<<grid, kSenderBlock, 0, st>>>(m);
}

template <bool ONE_WORD, bool TOPO>
void launch_faults(const MongerPullArgs& m, uint32_t grid, hipStream_t st) {
  if (m.a.fa.any()) launch_conn<ONE_WORD, TOPO, true>(m, grid, st);
  else launch_conn<ONE_WORD, TOPO, false>(m, grid, st);
}

template <bool ONE_WORD>
void launch_close(const MongerPullArgs& m, uint32_t grid, hipStream_t st) {
  if (m.C) monger_pull_close_kernel<ONE_WORD, true><<<grid, kSenderBlock, 0, st>>>(m);
  else monger_pull_close_kernel<ONE_WORD, false><<<grid, kSenderBlock, 0, st>>>(m);
}

}  // namespace

hipError_t launch_round_monger_pull(const MongerPullArgs& m, hipStream_t st) {
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

hipError_t launch_monger_pull_close(const MongerPullArgs& m, hipStream_t st) {
  const uint32_t grid = sender_grid(m.a.N);
  if (m.a.W == 1) launch_close<true>(m, grid, st);
  else launch_close<false>(m, grid, st);
  return hipGetLastError();
}

hipError_t launch_monger_hot_scan(const uint64_t* H, uint64_t N, uint32_t W, uint64_t* hotmap, uint64_t* hot_nodes,
                                  hipStream_t st) {
  monger_hot_scan_kernel<<<sender_grid(N), kSenderBlock, 0, st>>>(H, N, W, hotmap, hot_nodes);
  return hipGetLastError();
}

}  // namespace gossip
