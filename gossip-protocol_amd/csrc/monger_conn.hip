// monger_conn.hip — the arbitration of a round with a connection limit,
// written for gfx950 (CDNA4, wave64).
//
// Reference hot path: (*NodeState).Gossip, main.go:65-89, sends to every neighbour and every send
// is served; here a node serves at most c connections per round, and the initiators contend for
// them before the request pass runs.
//
// One launch per stage s = 0 .. h, one lane per initiator, the edges in batches of four as in the
// request kernels (resolve_batch of sender.h).  A lane finds its open edges by walking the verdicts
// of the stages before s again (conn_verdicts / conn_hunt of monger_conn.h: the stages before s are
// final once their launch has ended, whatever this launch inserts), so no per-edge state is kept:
// k <= 64 edges per node would cost more memory than the whole engine.  The open edges of stage s
// then insert their keys, per batch: all draws and the loads of the last slot first, and only then
// the chains of atomic minima — on gfx950 vmcnt retires in order, so a load consumed after an atomic
// was issued also waits for that atomic.  Within a batch only: with k > 4 the next
// batch's draws and loads come after this batch's returning minima and wait for them.  A key above
// the last slot's present value is refused already (that slot only falls) and issues no atomic.
// The launch after stage h only counts the verdicts of stage h.  A stage in whose predecessor
// nothing contended has nothing open: it returns on one load.
//
// The chain: old = atomicMin(&slot[i][p], v); v = max(old, v).  Every key passes slot 0, which keeps
// the minimum and hands everything else on to slot 1, and so on: slot i ends as the (i+1)-th smallest
// key in any schedule, with no lock and no sort.
#include "monger_conn.h"

#include "sender.h"

namespace gossip {

namespace {

__device__ __forceinline__ void conn_insert(const ConnArgs& ca, uint64_t N, uint32_t p, uint64_t v) {
  for (uint32_t i = 0; i < ca.c && v != kConnEmpty; ++i) {
    const uint64_t old = atomicMin((unsigned long long*)&ca.slots[(uint64_t)i * N + p], (unsigned long long)v);
    v = old > v ? old : v;
  }
}

__device__ __forceinline__ uint32_t count4(const bool (&f)[4]) {
  return (uint32_t)f[0] + (uint32_t)f[1] + (uint32_t)f[2] + (uint32_t)f[3];
}

// Stage s of the round; s == h + 1: the verdicts of stage h only.
template <bool TOPO, bool FAULTS>
__global__ __launch_bounds__(kSenderBlock) void conn_stage_kernel(ConnStageArgs x, uint32_t s) {
  const RoundArgs& a = x.a;
  const ConnArgs& ca = x.ca;
  if (s != 0 && ca.cnt[4 + s - 1] == 0) return;  // (uniform: the launch before this one wrote it)
  uint64_t att = 0, accepted = 0, refused = 0, deliv = 0;
  const uint32_t nblk = (a.k + 3u) >> 2;
  const uint64_t stride = (uint64_t)gridDim.x * kSenderBlock;
  for (uint64_t sn = (uint64_t)blockIdx.x * kSenderBlock + threadIdx.x; sn < a.N; sn += stride) {
    const uint32_t n = (uint32_t)sn;
    if (x.H) {  // push: a node with nothing hot starts nothing
      uint64_t h = 0;
      for (uint32_t w = 0; w < a.W; ++w) h |= x.H[(uint64_t)w * a.N + sn];
      if (h == 0) continue;
    }
    uint32_t b = 0, d = 0;
    if (TOPO) {
      b = a.orow[n];
      d = a.orow[n + 1] - b;
      if (d == 0) continue;
    }
    const Reach rc = FAULTS ? reach_of(n, a.fa) : Reach{0u, 0xFFFFFFFFu};
    for (uint32_t q = 0; q < nblk; ++q) {
      const uint32_t cnt = min(4u, a.k - 4u * q);
      uint32_t p[4];
      bool open[4], acc[4];
      resolve_batch<TOPO, FAULTS>(a, a.fa, rc, n, b, d, q, cnt, p, open);
      if (s == 0) att += cnt;  // lost attempts included
      for (uint32_t st = 0; st < s; ++st) {
        if (!(open[0] || open[1] || open[2] || open[3])) break;
        conn_verdicts(ca, a, n, q, st, p, open, acc);
        const bool newest = st + 1u == s;
        if (newest) accepted += count4(acc);
        if (st == ca.h) {  // (s == h + 1) refused for good
          refused += count4(open);
          break;
        }
        if (newest) att += count4(open);  // every refused edge hunts, whether or not the attempt is delivered
        conn_hunt<TOPO, FAULTS>(a, rc, n, b, d, q, st + 1u, p, open);
      }
      if (s > ca.h) continue;
      // the delivered attempts of stage s contend
      const u32x4 pw = conn_prio_draws(n, a.t, s, q, a.key0, a.key1);
      const uint64_t* last = ca.slots + (uint64_t)(ca.c - 1u) * a.N;
      uint64_t key[4], lv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) lv[i] = open[i] ? last[p[i]] : 0ull;
#pragma unroll
      for (int i = 0; i < 4; ++i) key[i] = conn_key(s, lane_of(pw, i), n, 4u * q + i);
      deliv += count4(open);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (open[i] && key[i] <= lv[i]) conn_insert(ca, a.N, p[i], key[i]);
    }
  }
  att = wave_sum64(att);
  accepted = wave_sum64(accepted);
  refused = wave_sum64(refused);
  deliv = wave_sum64(deliv);
  if ((threadIdx.x & 63) == 0) {
    if (att) {
      atomicAdd((unsigned long long*)&ca.cnt[0], (unsigned long long)att);
      if (s != 0) atomicAdd((unsigned long long*)&ca.cnt[3], (unsigned long long)att);
      if (x.H) atomicAdd((unsigned long long*)&a.partial[2], (unsigned long long)att);
    }
    if (accepted) atomicAdd((unsigned long long*)&ca.cnt[1], (unsigned long long)accepted);
    if (refused) atomicAdd((unsigned long long*)&ca.cnt[2], (unsigned long long)refused);
    if (deliv) atomicAdd((unsigned long long*)&ca.cnt[4 + s], (unsigned long long)deliv);
  }
}

template <bool TOPO>
void launch_faults(const ConnStageArgs& x, uint32_t s, uint32_t grid, hipStream_t st) {
  if (x.a.fa.any()) conn_stage_kernel<TOPO, true><<<grid, kSenderBlock, 0, st>>>(x, s);
  else conn_stage_kernel<TOPO, false><<<grid, kSenderBlock, 0, st>>>(x, s);
}

}  // namespace

hipError_t launch_conn_arbitrate(const ConnStageArgs& x, hipStream_t st) {
  const uint32_t grid = sender_grid(x.a.N);
  for (uint32_t s = 0; s <= x.ca.h + 1u; ++s) {
    if (x.topo) launch_faults<true>(x, s, grid, st);
    else launch_faults<false>(x, s, grid, st);
  }
  return hipGetLastError();
}

}  // namespace gossip
