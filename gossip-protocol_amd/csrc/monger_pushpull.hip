// monger_pushpull.hip — the push-pull rumor-mongering round, written for
// gfx950 (CDNA4, wave64).
//
// Reference hot path: (*NodeState).Gossip, main.go:65-89, forwards a value once and is done with it;
// here every node starts k exchanges per round, both ends of an exchange send the rumors they are
// still hot on, and both ends lose interest by what the other end told them.  All reads are of
// S_t, H_t and C_t.
//
// Two passes.  The request pass has one lane per initiator.  A node's next words are no longer its
// own: the initiators that drew it push into them.  So the pass writes neither next image; what an
// exchange moves goes into three [W][N] buffers that are zero between rounds, with ORs and only
// where the value is not zero: gain (what the end lacked), need and less (the feedback of
// monger_pull.hip, now for both ends).  Per edge and word that is at most three scattered atomics
// at the target; the initiator's own three values stay in registers across the batches (one word)
// and are ORed into its own words once.  The edges go in batches of four (resolve_batch of
// sender.h): all draws first, then the row loads, then the gathers of H_t[p] and S_t[p], then the
// deltas in registers, and only then the atomics — on gfx950 vmcnt retires in order, so a load
// consumed after an atomic was issued also waits for that atomic.  The close pass
// has one lane per node: it writes S_{t+1} = S_t | gain and H_{t+1} whole, draws the node's coin where
// a feedback word is set, applies the rule of one counter step per round (monger_close.h) and
// clears what it read.  Gains lie outside S_t[x] ⊇ H_t[x], losses inside H_t[x], gain, need and less
// are ORs: the result does not depend on the schedule.
//
// blind is a run-time value, as in monger_pull.hip: both variants gather H_t[p] and S_t[p].
//
// CONN: as in monger.hip, conn_resolve replaces the stage-0 peers of a batch
// by the accepted targets; "delivered" then reads "accepted".  The unlimited forms keep their code.
#include "monger_pushpull.h"

#include "monger_close.h"
#include "sender.h"

namespace gossip {

namespace {

// what the exchanges of one initiator bring to its own word
struct Own {
  uint64_t gain, need, less;
};

__device__ __forceinline__ void or_nonzero(uint64_t* at, uint64_t v) {
  if (v) atomicOr((unsigned long long*)at, (unsigned long long)v);
}

// What one batch does to one word: sv / hv = that word of S_t[n] / H_t[n], woff = its offset in the
// [W][N] arrays, ex[i] = the exchange was delivered (several words: and one end has something hot).
// The targets' shares go out as atomics, the initiator's are ORed into o.  msgs != null: counts the
// exchanges in which an end had something hot in this word.
__device__ __forceinline__ void exchange_word(const MongerPushPullArgs& x, uint64_t sv, uint64_t hv, uint64_t woff,
                                              const uint32_t (&p)[4], const bool (&ex)[4], Own& o, uint64_t* msgs) {
  const MongerPullArgs& m = x.m;
  uint64_t hp[4], sp[4], pg[4], pn[4], pl[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) hp[i] = ex[i] ? m.H[woff + p[i]] : 0ull;
  // S_t[p] decides only what becomes of the initiator's hot rumors: a cold initiator does not gather it
#pragma unroll
  for (int i = 0; i < 4; ++i) sp[i] = ex[i] && hv ? m.a.S[woff + p[i]] : 0ull;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t hx = ex[i] ? hv : 0ull;  // what the initiator sends over this edge
    pg[i] = hx & ~sp[i];
    o.gain |= hp[i] & ~sv;
    // feedback: each end learns which of what it sent the other lacked and which it held; blind: it
    // learns only that the exchange took place, and counts it against everything it sent
    pn[i] = m.blind ? 0ull : hp[i] & ~sv;
    pl[i] = m.blind ? hp[i] : hp[i] & sv;
    o.need |= m.blind ? 0ull : pg[i];
    o.less |= m.blind ? hx : hx & sp[i];
    if (msgs) *msgs += (hx | hp[i]) != 0;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    or_nonzero(&x.gain[woff + p[i]], pg[i]);
    or_nonzero(&m.need[woff + p[i]], pn[i]);
    or_nonzero(&m.less[woff + p[i]], pl[i]);
  }
}

// ---------------------------------------------------------------------------
// The request pass.  Messages: the delivered exchanges in which at least
// one end had something hot, once per exchange.  A full or cold node initiates too: it cannot know
// that its peer has nothing for it, and what it holds is the feedback that cools the peer.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool TOPO, bool FAULTS, bool CONN>
__global__ __launch_bounds__(kSenderBlock) void round_monger_pushpull_kernel(MongerPushPullArgs x) {
  const MongerPullArgs& m = x.m;
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
      if (d == 0) continue;  // an empty row starts no exchange; the node is still a target
    }
    const Reach rc = FAULTS ? reach_of(n, a.fa) : Reach{0u, 0xFFFFFFFFu};
    uint32_t p[4];
    bool live[4];
    if (ONE_WORD) {  // the own shares stay in registers across the batches: at most three ORs at the end
      const uint64_t sv = a.S[s], hv = m.H[s];
      Own o{0, 0, 0};
      for (uint32_t q = 0; q < nblk; ++q) {
        resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live);
        if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, q, p, live);
        exchange_word(x, sv, hv, 0, p, live, o, &msgs);
      }
      or_nonzero(&x.gain[s], o.gain);
      or_nonzero(&m.need[s], o.need);
      or_nonzero(&m.less[s], o.less);
    } else {
      // the initiator's own bit of the bitmap of H_t: with something hot every delivered exchange is a
      // message and S_t[p] is gathered whatever p holds; with nothing hot the peers of a batch are
      // probed in the bitmap and a cold one costs no gather — late in a run every probe says no
      const bool own_hot = (m.hotmap[s >> 6] >> (s & 63u)) & 1ull;
      for (uint32_t q = 0; q < nblk; ++q) {
        resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, min(4u, a.k - 4u * q), p, live);
        if (CONN) conn_resolve<TOPO, FAULTS>(m.conn, a, rc, n, b, d, q, p, live);
        if (!own_hot) {
          uint64_t bits[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) bits[i] = live[i] ? m.hotmap[p[i] >> 6] : 0ull;
#pragma unroll
          for (int i = 0; i < 4; ++i) live[i] = (bits[i] >> (p[i] & 63u)) & 1ull;
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          any = any || live[i];
          msgs += live[i];
        }
        if (!any) continue;
        // W is a run-time value: the own shares of a word go out per batch
        for (uint32_t w = 0; w < a.W; ++w) {
          const uint64_t woff = (uint64_t)w * a.N;
          const uint64_t sv = a.S[woff + s], hv = own_hot ? m.H[woff + s] : 0ull;
          Own o{0, 0, 0};
          exchange_word(x, sv, hv, woff, p, live, o, nullptr);
          or_nonzero(&x.gain[woff + s], o.gain);
          or_nonzero(&m.need[woff + s], o.need);
          or_nonzero(&m.less[woff + s], o.less);
        }
      }
    }
  }
  msgs = wave_sum64(msgs);
  if ((threadIdx.x & 63) == 0 && msgs) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)msgs);
}

// ---------------------------------------------------------------------------
// The close pass, after the request pass has finished: plain loads
// and stores, lane n alone touches the words of node n.  Both next images are written whole here.
// ---------------------------------------------------------------------------
template <bool ONE_WORD, bool COUNT>
__global__ __launch_bounds__(kSenderBlock) void monger_pushpull_close_kernel(MongerPushPullArgs x) {
  const MongerPullArgs& m = x.m;
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
        const uint64_t sv = a.S[at], hv = m.H[at];
        const uint64_t g = x.gain[at], nd = m.need[at], ls = m.less[at];
        uint64_t hn = hv | (g & ~sv);  // new here: known here and hot here
        if (g) x.gain[at] = 0;
        if (nd | ls) {
          if (nd) m.need[at] = 0;
          if (ls) m.less[at] = 0;
          hn &= ~monger_cool_word<COUNT>(m, s, at, plane, nd, ls, coin);
        }
        a.Snext[at] = sv | g;
        m.Hnext[at] = hn;
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

template <bool ONE_WORD, bool TOPO, bool FAULTS>
void launch_conn(const MongerPushPullArgs& x, uint32_t grid, hipStream_t st) {
  if (x.m.conn.c) round_monger_pushpull_kernel<ONE_WORD, TOPO, FAULTS, true><<<grid, kSenderBlock, 0, st>>>(x);
  else round_monger_pushpull_kernel<ONE_WORD, TOPO, FAULTS, false><<<grid, kSenderBlock, 0, st>>>(x);
}

template <bool ONE_WORD, bool TOPO>
void launch_faults(const MongerPushPullArgs& x, uint32_t grid, hipStream_t st) {
  if (x.m.a.fa.any()) launch_conn<ONE_WORD, TOPO, true>(x, grid, st);
  else launch_conn<ONE_WORD, TOPO, false>(x, grid, st);
}

template <bool ONE_WORD>
void launch_close(const MongerPushPullArgs& x, uint32_t grid, hipStream_t st) {
  if (x.m.C) monger_pushpull_close_kernel<ONE_WORD, true><<<grid, kSenderBlock, 0, st>>>(x);
  else monger_pushpull_close_kernel<ONE_WORD, false><<<grid, kSenderBlock, 0, st>>>(x);
}

}  // namespace

hipError_t launch_round_monger_pushpull(const MongerPushPullArgs& x, hipStream_t st) {
  const uint32_t grid = sender_grid(x.m.a.N);
  if (x.m.a.W == 1) {
    if (x.m.topo) launch_faults<true, true>(x, grid, st);
    else launch_faults<true, false>(x, grid, st);
  } else {
    if (x.m.topo) launch_faults<false, true>(x, grid, st);
    else launch_faults<false, false>(x, grid, st);
  }
  return hipGetLastError();
}

hipError_t launch_monger_pushpull_close(const MongerPushPullArgs& x, hipStream_t st) {
  const uint32_t grid = sender_grid(x.m.a.N);
  if (x.m.a.W == 1) launch_close<true>(x, grid, st);
  else launch_close<false>(x, grid, st);
  return hipGetLastError();
}

}  // namespace gossip
