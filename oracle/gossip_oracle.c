/*
 * gossip_oracle.c — TEST INFRASTRUCTURE ONLY (see gossip_oracle.h).
 *
 * Plain-C restatement of the round model in DESIGN.md §2.  Every function
 * names the reference code it restates.  Reference = 0xSherlokMo/gossip-protocol
 * main.go (Go; not buildable here: no Go toolchain).  Parity is pinned by
 * Philox KATs, FLOOD BFS properties and the independent numpy restatement
 * (oracle/numpy_ref.py → tests/golden/); see DESIGN.md §4.
 *
 * threads == 1: scalar reference loops.  threads > 1: the same loops under
 * OpenMP with atomic ORs for pushes (used only as bench.py's cpu_baseline).
 */
#include "gossip_oracle.h"
#include "../gossip-protocol_amd/csrc/plan.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define GOLD64 0x9E3779B97F4A7C15ull
#define WALK_NONE 0xFFFFFFFFu /* FLOOD walks: no first sender (a client value) */

struct oracle_sim {
  gossip_config_t cfg;
  int threads;
  uint64_t N, Nl, lo, hi, nown;
  uint32_t R, W, k, mode, G, rank;
  uint64_t* S;     /* own shard S_t, [W][Nl]                  */
  uint64_t* Snext; /* own shard S_{t+1}, [W][Nl]              */
  uint64_t* Sprev; /* FLOOD: own shard S_{t-1}                */
  uint64_t* skip;  /* FLOOD: first-sender-in-Adj mask per bit */
  uint64_t* send;  /* exchange send buffer [W][Nl]            */
  uint64_t* recv;  /* gathered [G][W][Nl]                     */
  uint64_t* fullm; /* W valid-bit masks                        */
  uint32_t *orow, *ocol, *irow, *icol;
  uint64_t E;
  int has_topo;
  uint32_t t;
  /* ANTIENTROPY: V[n*K + c], alive bytes, global max vector */
  uint32_t *V, *Vn, *target;
  uint8_t *alive, *alive_n;
  /* sparse sharded rounds (include/gossip.h; the engine's csrc/sharded.hip):
   * items are {node, value} pairs of uint64 */
  uint64_t* gtot;           /* global totals of S_t [5 + R] */
  int gtot_valid, planned, last_sparse;
  uint32_t maj;
  plan_cfg pl; /* the round planner's shape, knobs (oracle_set_param, oracle_set_faults) and state: csrc/plan.h */
  uint64_t *rare_send, *rare_recv, stride; /* [Nl] items; [G * stride] items */
  uint64_t *msg_send, *msg_recv, msg_cap;  /* [k * nown] items grouped by owner; received items */
  uint64_t* D;                             /* pending push deltas of the owned nodes */
  uint64_t* counts;                        /* rare list lengths of the current round [G] */
  /* stall mode: random modes, lost-exchange streak per node (all N) */
  uint8_t* streak;
  /* FLOOD with faults: one walk per (value x, node u), index x * N + u: next
   * position in u's row (rows keep the topology message's order), lost attempts there, first
   * sender (WALK_NONE: a client) */
  int flood_edges;
  uint32_t *wcur, *wsnd;
  uint8_t* watt;
  /* sharded ANTIENTROPY (G > 1): V/Vn = own rows [Nl][K], alive bytes of all N,
   * aex_img = every shard's {alive, stale} word pairs per 64 nodes (the all-gather image: the
   * owner churns its nodes at exchange_buffers, aex_churned = that round), request / reply items */
  int aex, aex_target_ok;
  uint32_t aex_churned;
  uint32_t rw, pw;
  uint64_t* aex_img;
  uint32_t *req, *loc, *in, *resp_out, *resp_in;
  uint64_t nreq, nloc, nin, in_cap, aex_msgs;
  /* exchange dense rounds (kind 3): items {p at owner | flags, S_t[n]} by owner;
   * xnode = the own sender of each send item; replies in send / received order */
  int xd_planned;
  uint32_t *xid, *xrid;
  uint64_t *xval, *xrval, *xrep_out, *xrep_in, *xnode;
  uint64_t xn_out, xn_in;
  /* the exchange round's edge filter: filt bit 0 drops pull-only edges into empty peers, bit 1
   * push-only edges into full peers (decided from the global totals, threshold xd_filter_frac);
   * xcls = every shard's [nz][full] occupancy bitmaps of S_t (nwl words each) */
  uint32_t xd_filt;
  int xcls_ok;
  uint64_t* xcls;
  /* class-coded state all-gather (kind 4): every shard's slot ([nz][full]
   * bitmaps, nwl words each, then nwl uint32 prefixes: the mixed nodes before each bitmap
   * word), the own mixed words, every shard's at q * cc_stride */
  int cc_planned;
  /* replicated dense rounds (plan kinds 5 / 6 / 7): every shard computes the whole
   * image's round, so the next dense round needs no all-gather (pl.rep_img_ok) */
  int rep_planned;
  uint64_t *cc_bits, *cc_send, *cc_vals, cc_stride;
};

static inline int churned(int alive, uint32_t n, uint32_t t, uint32_t k, const uint32_t key[2], uint32_t fail,
                          uint32_t rec);
static inline int alive_bit(const oracle_sim_t* s, uint64_t n);
static void aex_own_fill_alive(oracle_sim_t* s);

/* ---------------- Philox4x32-10 (Random123; rocRAND philox4x32_10.h:270-302) ---- */
void oracle_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
  uint32_t k0 = key[0], k1 = key[1];
  for (int i = 0; i < 10; ++i) {
    uint64_t m0 = (uint64_t)0xD2511F53u * c0;
    uint64_t m1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0;
    uint32_t n1 = (uint32_t)m1;
    uint32_t n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
    uint32_t n3 = (uint32_t)m0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* Peer draw p_j(n,t) — replaces Topology[node.ID()] (main.go:72). */
static inline uint32_t peer_from_word(uint32_t x, uint64_t N, uint32_t n) {
  uint32_t p = (uint32_t)(((uint64_t)x * (N - 1)) >> 32);
  return p + (p >= n);
}

uint32_t oracle_peer(uint64_t seed, uint64_t N, uint32_t n, uint32_t t, uint32_t j) {
  uint32_t ctr[4] = {n, t, 0u, j >> 2};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t x[4];
  oracle_philox4x32_10(ctr, key, x);
  return peer_from_word(x[j & 3], N, n);
}

/* Rumor origin, Philox stream tag 2. */
/* Fault model (the reference's lossy SyncRPC, main.go:77-87):
 * the edge n -> p_j(n) of round t is lost, both directions, when a partition
 * (nodes split into P contiguous blocks, block(n) = n*P/N) separates n and p,
 * or when Philox({n, t, 4, j>>2}, key)[j&3] < edge_loss. */
static int edge_lost(const gossip_config_t* cfg, uint64_t N, uint32_t n, uint32_t p, uint32_t t, uint32_t j,
                     const uint32_t key[2]) {
  if (cfg->partitions > 1 &&
      (uint64_t)n * cfg->partitions / N != (uint64_t)p * cfg->partitions / N) return 1;
  if (cfg->edge_loss) {
    uint32_t ctr[4] = {n, t, 4u, j >> 2}, x[4];
    oracle_philox4x32_10(ctr, key, x);
    if (x[j & 3] < cfg->edge_loss) return 1;
  }
  return 0;
}

/* Stall mode (main.go:77-87: a neighbour's 2 s context expires and the
 * goroutine retries forever): a node whose initiated exchanges were lost in stall_rounds
 * rounds in a row initiates none until reset.  It still answers pulls and takes pushes. */
static inline int stalled(const oracle_sim_t* s, uint32_t n) {
  return s->streak && s->streak[n] >= s->cfg.stall_rounds;
}

/* edge n -> p (slot j of initiator n, round t) carries nothing this round */
static inline int lost_edge(const oracle_sim_t* s, uint32_t n, uint32_t p, uint32_t j, const uint32_t key[2]) {
  return stalled(s, n) || edge_lost(&s->cfg, s->N, n, p, s->t, j, key);
}

uint32_t oracle_origin(uint64_t seed, uint64_t N, uint32_t r) {
  uint32_t ctr[4] = {r, 0u, 2u, 0u};
  uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t x[4];
  oracle_philox4x32_10(ctr, key, x);
  return (uint32_t)(((uint64_t)x[0] * N) >> 32);
}

uint64_t oracle_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

static inline int popc64(uint64_t x) { return __builtin_popcountll(x); }

/* ---------------- construction (NewState/NewMessageKeeper, main.go:28-33,91-97) -- */
int oracle_create(const gossip_config_t* cfg, int threads, oracle_sim_t** out) {
  if (!cfg || !out) return GOSSIP_EINVAL;
  *out = NULL;
  if (cfg->n_nodes < 2 || cfg->n_nodes >= (1ull << 32)) return GOSSIP_EINVAL;
  if (cfg->n_rumors == 0 || cfg->n_rumors > 4096) return GOSSIP_EINVAL;
  if (cfg->mode > GOSSIP_MODE_ANTIENTROPY) return GOSSIP_ENOTSUP;
  if (cfg->mode != GOSSIP_MODE_FLOOD && (cfg->fanout == 0 || cfg->fanout > 64)) return GOSSIP_EINVAL;
  uint32_t G = cfg->shard_count ? cfg->shard_count : 1;
  if (cfg->shard_rank >= G) return GOSSIP_EINVAL;
  if (cfg->mode == GOSSIP_MODE_ANTIENTROPY && (cfg->n_rumors > 64 || G > 1024)) return GOSSIP_ENOTSUP;
  if (cfg->stall_rounds > 16) return GOSSIP_EINVAL;
  const int faulty = cfg->edge_loss || cfg->partitions > 1 || cfg->stall_rounds;
  if (faulty && (cfg->mode == GOSSIP_MODE_ANTIENTROPY || (cfg->mode == GOSSIP_MODE_FLOOD && G != 1)))
    return GOSSIP_ENOTSUP;
  oracle_sim_t* s = (oracle_sim_t*)calloc(1, sizeof(*s));
  if (!s) return GOSSIP_ENOMEM;
  s->cfg = *cfg;
  s->threads = threads < 1 ? 1 : threads;
  s->N = cfg->n_nodes;
  s->R = cfg->n_rumors;
  s->W = (s->R + 63) / 64;
  s->k = cfg->fanout;
  s->mode = cfg->mode;
  s->G = G;
  s->rank = cfg->shard_rank;
  s->Nl = (s->N + G - 1) / G;
  s->aex = s->mode == GOSSIP_MODE_ANTIENTROPY && G > 1;
  if (s->aex) s->Nl = (s->Nl + 63) / 64 * 64; /* 64-aligned row blocks, as the engine */
  s->lo = (uint64_t)s->rank * s->Nl;
  s->hi = s->lo + s->Nl < s->N ? s->lo + s->Nl : s->N;
  if (s->lo > s->hi) s->lo = s->hi;
  s->nown = s->hi - s->lo;
  size_t shard = (size_t)s->W * s->Nl;
  s->S = (uint64_t*)calloc(shard, 8);
  s->Snext = (uint64_t*)calloc(shard, 8);
  s->send = (uint64_t*)calloc(shard, 8);
  s->recv = G > 1 ? (uint64_t*)calloc(shard * G, 8) : NULL;
  s->fullm = (uint64_t*)calloc(s->W, 8);
  if (s->mode == GOSSIP_MODE_FLOOD) {
    s->Sprev = (uint64_t*)calloc(shard, 8);
    s->skip = (uint64_t*)calloc(shard, 8);
  }
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) {
    const size_t rows = s->aex ? s->Nl : s->N;
    s->V = (uint32_t*)calloc(rows * s->R + 1, 4);
    s->Vn = (uint32_t*)calloc(rows * s->R + 1, 4);
    if (s->aex) {
      s->rw = (s->R + 3) / 2 * 2;
      s->pw = (s->R + 1) / 2 * 2;
      s->aex_img = (uint64_t*)calloc(2 * ((size_t)G * s->Nl / 64 + 1), 8);
      const size_t cap = (size_t)s->nown * s->k + 1;
      s->req = (uint32_t*)calloc(cap * s->rw, 4);
      s->loc = (uint32_t*)calloc(cap * 2, 4);
      s->resp_in = (uint32_t*)calloc(cap * s->pw, 4);
    }
    s->target = (uint32_t*)calloc(s->R, 4);
    s->alive = (uint8_t*)malloc(s->N);
    s->alive_n = (uint8_t*)malloc(s->N);
    if (!s->V || !s->Vn || !s->target || !s->alive || !s->alive_n) {
      oracle_destroy(s);
      return GOSSIP_ENOMEM;
    }
    memset(s->alive, 1, s->N);
    if (s->aex) aex_own_fill_alive(s);
  }
  if (!s->S || !s->Snext || !s->send || (G > 1 && !s->recv) || !s->fullm ||
      (s->mode == GOSSIP_MODE_FLOOD && (!s->Sprev || !s->skip))) {
    oracle_destroy(s);
    return GOSSIP_ENOMEM;
  }
  for (uint32_t w = 0; w < s->W; ++w) {
    uint32_t bits = s->R - 64 * w;
    s->fullm[w] = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
  }
  s->gtot = (uint64_t*)calloc(5 + s->R, 8);
  s->counts = (uint64_t*)calloc(G, 8);
  plan_defaults(&s->pl);
  s->pl.N = s->N, s->pl.Nl = s->Nl, s->pl.G = G, s->pl.k = s->k, s->pl.R = s->R, s->pl.mode = s->mode;
  s->pl.edge_loss = cfg->edge_loss, s->pl.partitions = cfg->partitions;
  /* host shards can run every kind of round (oracle_sharded_plan plans only where sparse_ok) */
  s->pl.sharded = s->pl.can_sparse = s->pl.can_xd = s->pl.can_rep = 1;
  s->flood_edges = s->mode == GOSSIP_MODE_FLOOD && faulty;
  if (s->flood_edges) {
    const size_t nw = (size_t)s->R * s->N;
    s->wcur = (uint32_t*)malloc(nw * 4);
    s->wsnd = (uint32_t*)malloc(nw * 4);
    s->watt = (uint8_t*)calloc(nw, 1);
    if (!s->wcur || !s->wsnd || !s->watt) { oracle_destroy(s); return GOSSIP_ENOMEM; }
    memset(s->wcur, 0xFF, nw * 4); /* WALK_DONE */
    memset(s->wsnd, 0xFF, nw * 4); /* WALK_NONE */
  }
  if (cfg->stall_rounds && s->mode >= GOSSIP_MODE_PUSH && s->mode <= GOSSIP_MODE_PUSHPULL &&
      !(s->streak = (uint8_t*)calloc(s->N, 1))) {
    oracle_destroy(s);
    return GOSSIP_ENOMEM;
  }
  if (!s->gtot || !s->counts) {
    oracle_destroy(s);
    return GOSSIP_ENOMEM;
  }
  *out = s;
  return GOSSIP_OK;
}

void oracle_destroy(oracle_sim_t* s) {
  if (!s) return;
  free(s->S); free(s->Snext); free(s->Sprev); free(s->skip); free(s->send); free(s->recv);
  free(s->fullm); free(s->orow); free(s->ocol); free(s->irow); free(s->icol);
  free(s->V); free(s->Vn); free(s->target); free(s->alive); free(s->alive_n);
  free(s->gtot); free(s->counts); free(s->rare_send); free(s->rare_recv); free(s->msg_send); free(s->msg_recv);
  free(s->D);
  free(s->streak); free(s->wcur); free(s->wsnd); free(s->watt);
  free(s->aex_img); free(s->req); free(s->loc); free(s->in); free(s->resp_out); free(s->resp_in);
  free(s->xid); free(s->xrid); free(s->xval); free(s->xrval); free(s->xrep_out); free(s->xrep_in); free(s->xnode);
  free(s->cc_bits); free(s->cc_send); free(s->cc_vals); free(s->xcls);
  free(s);
}

/* "topology" handler, main.go:132-149: State.Topology = body.Topology (:142).
 * Rows are treated as sets (sorted, duplicates dropped); the in-adjacency
 * (transpose) is built for the pull form of the flood. */
static int cmp_u32(const void* a, const void* b) {
  uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
  return x < y ? -1 : x > y;
}

int oracle_set_topology_csr(oracle_sim_t* s, const uint32_t* row_ptr, const uint32_t* col,
                            uint64_t n, uint64_t n_edges) {
  if (!s || !row_ptr || (n_edges && !col) || n != s->N) return GOSSIP_EINVAL;
  if (row_ptr[0] != 0 || row_ptr[n] != n_edges) return GOSSIP_EINVAL;
  for (uint64_t u = 0; u < n; ++u)
    if (row_ptr[u + 1] < row_ptr[u]) return GOSSIP_EINVAL;
  for (uint64_t e = 0; e < n_edges; ++e)
    if (col[e] >= n) return GOSSIP_EINVAL;
  uint32_t* orow = (uint32_t*)calloc(n + 1, 4);
  uint32_t* ocol = (uint32_t*)malloc((n_edges ? n_edges : 1) * 4);
  uint32_t* irow = (uint32_t*)calloc(n + 1, 4);
  uint32_t* icol = (uint32_t*)malloc((n_edges ? n_edges : 1) * 4);
  if (!orow || !ocol || !irow || !icol) {
    free(orow); free(ocol); free(irow); free(icol);
    return GOSSIP_ENOMEM;
  }
  uint64_t E = 0;
  for (uint64_t u = 0; u < n; ++u) {
    uint64_t b = row_ptr[u], e = row_ptr[u + 1];
    uint64_t start = E;
    memcpy(ocol + E, col + b, (e - b) * 4);
    uint64_t m = e - b;
    if (!s->flood_edges) { /* rows as sets; the walks of FLOOD with faults keep the message's order */
      qsort(ocol + E, e - b, 4, cmp_u32);
      m = 0;
      for (uint64_t i = 0; i < e - b; ++i)
        if (m == 0 || ocol[start + m - 1] != ocol[start + i]) ocol[start + m++] = ocol[start + i];
    }
    E += m;
    orow[u + 1] = (uint32_t)E;
  }
  for (uint64_t e = 0; e < E; ++e) irow[ocol[e] + 1]++;
  for (uint64_t v = 0; v < n; ++v) irow[v + 1] += irow[v];
  uint32_t* fill = (uint32_t*)malloc((n + 1) * 4);
  if (!fill) {
    free(orow); free(ocol); free(irow); free(icol);
    return GOSSIP_ENOMEM;
  }
  memcpy(fill, irow, (n + 1) * 4);
  for (uint64_t u = 0; u < n; ++u) /* ascending u => each in-row sorted */
    for (uint32_t e = orow[u]; e < orow[u + 1]; ++e) icol[fill[ocol[e]]++] = (uint32_t)u;
  free(fill);
  free(s->orow); free(s->ocol); free(s->irow); free(s->icol);
  s->orow = orow; s->ocol = ocol; s->irow = irow; s->icol = icol;
  s->E = E;
  if (s->flood_edges) { /* a new topology ends every walk: held values are not sent again */
    memset(s->wcur, 0xFF, (size_t)s->R * s->N * 4);
    memset(s->wsnd, 0xFF, (size_t)s->R * s->N * 4);
    memset(s->watt, 0, (size_t)s->R * s->N);
  }
  s->has_topo = 1;
  return GOSSIP_OK;
}

int oracle_reset(oracle_sim_t* s) {
  if (!s) return GOSSIP_EINVAL;
  size_t shard = (size_t)s->W * s->Nl * 8;
  memset(s->S, 0, shard);
  memset(s->Snext, 0, shard);
  if (s->Sprev) memset(s->Sprev, 0, shard);
  if (s->skip) memset(s->skip, 0, shard);
  s->aex_target_ok = 0;
  if (s->V) {
    memset(s->V, 0, (size_t)(s->aex ? s->Nl : s->N) * s->R * 4);
    memset(s->target, 0, (size_t)s->R * 4);
    memset(s->alive, 1, s->N);
    if (s->aex) aex_own_fill_alive(s);
  }
  if (s->streak) memset(s->streak, 0, s->N);
  if (s->flood_edges) {
    memset(s->wcur, 0xFF, (size_t)s->R * s->N * 4);
    memset(s->wsnd, 0xFF, (size_t)s->R * s->N * 4);
    memset(s->watt, 0, (size_t)s->R * s->N);
  }
  s->t = 0;
  s->gtot_valid = s->planned = s->last_sparse = 0;
  s->rep_planned = s->pl.rep_img_ok = 0;
  return GOSSIP_OK;
}

/* Client "broadcast" (main.go:102-117): dedupe (:113) is the bit test, Append (:117)
 * the bit set.  Injected bits carry no sender in Adj, so skip stays 0 for them. */
int oracle_inject(oracle_sim_t* s, uint64_t node, uint32_t rumor) {
  if (!s || node >= s->N || rumor >= s->R) return GOSSIP_EINVAL;
  if (s->aex) { /* a local write on the owner; the global max vector is re-derived before a round */
    if (node >= s->lo && node < s->hi) s->V[(node - s->lo) * s->R + rumor] += 1;
    s->aex_target_ok = 0;
    return GOSSIP_OK;
  }
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) { /* a local write of key `rumor` */
    uint32_t* x = &s->V[node * s->R + rumor];
    *x += 1;
    if (*x > s->target[rumor]) s->target[rumor] = *x;
    return GOSSIP_OK;
  }
  s->gtot_valid = 0;
  s->pl.rep_img_ok = 0;
  if (node < s->lo || node >= s->hi) return GOSSIP_OK;
  uint64_t* w = &s->S[(size_t)(rumor >> 6) * s->Nl + (node - s->lo)];
  if (s->flood_edges && !(*w & (1ull << (rumor & 63)))) { /* a client's value: its walk starts next round */
    const size_t i = (size_t)rumor * s->N + node;
    s->wcur[i] = 0;
    s->watt[i] = 0;
    s->wsnd[i] = WALK_NONE;
  }
  *w |= 1ull << (rumor & 63);
  return GOSSIP_OK;
}

int oracle_inject_random(oracle_sim_t* s) {
  if (!s) return GOSSIP_EINVAL;
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) { /* V[n][c] = Philox({n, c/4, 3, 0})[c%4] & 0xFFFF */
    const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
    memset(s->target, 0, (size_t)s->R * 4);
    s->aex_target_ok = 0;
    for (uint64_t n = s->aex ? s->lo : 0; n < (s->aex ? s->hi : s->N); ++n)
      for (uint32_t c = 0; c < s->R; c += 4) {
        uint32_t ctr[4] = {(uint32_t)n, c >> 2, 3u, 0u}, x[4];
        oracle_philox4x32_10(ctr, key, x);
        for (uint32_t q = 0; q < 4 && c + q < s->R; ++q) {
          uint32_t v = x[q] & 0xFFFFu;
          s->V[(n - (s->aex ? s->lo : 0)) * s->R + c + q] = v;
          if (v > s->target[c + q]) s->target[c + q] = v;
        }
      }
    return GOSSIP_OK;
  }
  for (uint32_t r = 0; r < s->R; ++r) oracle_inject(s, oracle_origin(s->cfg.seed, s->N, r), r);
  return GOSSIP_OK;
}

/* [0] full [1] alive [2] messages [3] hash [4, 4+R) infected [4+R] nonzero nodes */
uint64_t oracle_partial_len(const oracle_sim_t* s) { return 5 + (s ? s->R : 0); }

/* Exchange payload: S_t for random modes, the frontier F_t = S_t & ~S_{t-1} for FLOOD. */
int oracle_exchange_buffers(oracle_sim_t* s, void** send, void** recv, uint64_t* send_bytes) {
  if (!s) return GOSSIP_EINVAL;
  if (s->aex) { /* the own {alive, stale} word pairs into every shard's image, after the own churn */
    if (s->aex_churned != s->t) {
      const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
      uint64_t* own = s->aex_img + (size_t)s->rank * s->Nl / 32;
      for (uint64_t i = 0; i < s->nown; ++i) {
        const uint64_t bit = 1ull << (i & 63), n = s->lo + i;
        const int al = churned((own[2 * (i >> 6)] & bit) != 0, (uint32_t)n, s->t, s->k, key, s->cfg.churn_fail,
                               s->cfg.churn_recover);
        own[2 * (i >> 6)] = al ? own[2 * (i >> 6)] | bit : own[2 * (i >> 6)] & ~bit;
      }
      s->aex_churned = s->t;
    }
    if (send) *send = s->aex_img + (size_t)s->rank * s->Nl / 32;
    if (recv) *recv = s->aex_img;
    if (send_bytes) *send_bytes = s->Nl / 4;
    return GOSSIP_OK;
  }
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) return GOSSIP_OK; /* single shard: nothing to exchange */
  size_t shard = (size_t)s->W * s->Nl;
  if (s->mode == GOSSIP_MODE_FLOOD)
    for (size_t i = 0; i < shard; ++i) s->send[i] = s->S[i] & ~s->Sprev[i];
  else
    memcpy(s->send, s->S, shard * 8);
  if (send) *send = s->send;
  if (recv) *recv = s->G > 1 ? s->recv : s->send;
  if (send_bytes) *send_bytes = shard * 8;
  return GOSSIP_OK;
}

/* word w of global node n inside the gathered [G][W][Nl] image */
static inline uint64_t gword(const oracle_sim_t* s, const uint64_t* g, uint64_t n, uint32_t w) {
  uint64_t r = n / s->Nl, i = n - r * s->Nl;
  return g[(r * s->W + w) * s->Nl + i];
}

static int in_sorted(const uint32_t* a, uint32_t len, uint32_t x) {
  uint32_t lo = 0, hi = len;
  while (lo < hi) {
    uint32_t mid = (lo + hi) / 2;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo < len && a[lo] == x;
}

/* One round S_t -> S_{t+1} for the owned nodes (Gossip, main.go:65-89, as a
 * synchronous round).  g = gathered exchange image (S_t or F_t). */
/* Churn: the alive flag of node n after round t's churn.  The draw is the last
 * word of the node's first peer draw Philox({n, t, 0, 0}) for fanout k <= 3 (its words 0 .. k-1
 * are the peers), else Philox({n, t, 1, 0})[0]. */
static inline int churned(int alive, uint32_t n, uint32_t t, uint32_t k, const uint32_t key[2], uint32_t fail,
                          uint32_t rec) {
  uint32_t ctr[4] = {n, t, k <= 3 ? 0u : 1u, 0u}, x[4];
  oracle_philox4x32_10(ctr, key, x);
  const uint32_t w = k <= 3 ? x[3] : x[0];
  return alive ? !(w < fail) : (w < rec);
}

/* max-merge into a row word another thread may also be merging into (OpenMP rounds); max is
 * commutative and idempotent, so the result does not depend on the order of the merges */
static inline void max_merge_u32(uint32_t* p, uint32_t v, int shared) {
  if (!shared) {
    if (v > *p) *p = v;
    return;
  }
  uint32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > cur && !__atomic_compare_exchange_n(p, &cur, v, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
  }
}

/* Anti-entropy round: push-pull max-merge over alive-alive edges (each
 * exchange restates one request/reply of main.go:77-81).  threads > 1: the same round on
 * OpenMP threads (reads are of V = S_t, merges into Vn are atomic maxima). */
static int ae_round(oracle_sim_t* s, uint64_t* partial) {
  const uint64_t N = s->N;
  const uint32_t K = s->R, k = s->k, t = s->t;
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  const uint32_t fail = s->cfg.churn_fail, rec = s->cfg.churn_recover;
  const int nt = s->threads, shared = nt > 1;
#pragma omp parallel for num_threads(nt) if (nt > 1) schedule(static)
  for (uint64_t n = 0; n < N; ++n) s->alive_n[n] = (uint8_t)churned(s->alive[n], (uint32_t)n, t, k, key, fail, rec);
#pragma omp parallel for num_threads(nt) if (nt > 1) schedule(static)
  for (uint64_t n = 0; n < N; ++n) memcpy(s->Vn + n * K, s->V + n * K, (size_t)K * 4);
  uint64_t msgs = 0;
#pragma omp parallel for num_threads(nt) if (nt > 1) schedule(static) reduction(+ : msgs)
  for (uint64_t n = 0; n < N; ++n) {
    if (!s->alive_n[n]) continue;
    uint32_t x[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < k; ++j) {
      if ((j & 3) == 0) {
        uint32_t ctr[4] = {(uint32_t)n, t, 0u, j >> 2};
        oracle_philox4x32_10(ctr, key, x);
      }
      uint32_t p = peer_from_word(x[j & 3], N, (uint32_t)n);
      if (!s->alive_n[p]) continue;
      ++msgs;
      for (uint32_t c = 0; c < K; ++c) {
        uint32_t a = s->V[n * K + c], b = s->V[(uint64_t)p * K + c];
        max_merge_u32(&s->Vn[n * K + c], b, shared);                /* pull */
        max_merge_u32(&s->Vn[(uint64_t)p * K + c], a, shared);      /* push */
      }
    }
  }
  uint64_t full = 0, alive = 0, hash = 0;
  uint64_t* inf = partial + 4;
  memset(inf, 0, (size_t)K * 8);
#pragma omp parallel num_threads(nt) if (nt > 1)
  {
    uint64_t f = 0, a = 0, h = 0, cnt[64] = {0};
#pragma omp for schedule(static)
    for (uint64_t n = 0; n < N; ++n) {
      int isfull = 1;
      for (uint32_t c = 0; c < K; ++c) {
        uint32_t v = s->Vn[n * K + c];
        if (v && (s->cfg.flags & GOSSIP_FLAG_HASH)) h += oracle_mix64((uint64_t)v + ((uint64_t)c * N + n) * GOLD64);
        if (v != s->target[c]) isfull = 0;
        else if (s->alive_n[n]) cnt[c]++;
      }
      if (s->alive_n[n]) {
        a++;
        f += isfull;
      }
    }
#pragma omp critical
    {
      full += f;
      alive += a;
      hash += h;
      for (uint32_t c = 0; c < K; ++c) inf[c] += cnt[c];
    }
  }
  partial[0] = full;
  partial[1] = alive;
  partial[2] = msgs;
  partial[3] = hash;
  partial[4 + s->R] = 0; /* nonzero count: random modes only */
  return GOSSIP_OK;
}

/* FLOOD with faults (main.go:72-87): the reference forwards a value from one
 * goroutine that walks Topology[node] in order (:72), skipping the value's sender (:73), and
 * blocks in SyncRPC on each neighbour until it is acked (:80-87); a neighbour's 2 s context
 * (:77) expires after stall_rounds = D lost attempts (D = 0: never).  Round t, every walk of a
 * value x held by u goes on from its position c: the sender is skipped (no message); any other
 * neighbour w costs one message, which is lost like a random-mode edge (partition, or its own
 * loss draw: each value is one SyncRPC, so the draw is per (u, c, t, value), flood_lost below).  A lost
 * attempt ends the walk's round (head-of-line: the later neighbours wait); a delivered one gives
 * w the value and moves on to c + 1 — unless the context has expired, when the walk stays on w
 * for good (it keeps retrying, and w can still learn x from it).  w's first sender of x is the
 * lowest u that delivered it in the round w learned it; w's walk of x starts the next round. */
/* One SyncRPC per value (main.go:81): the message of value x from u at row position j is lost on a
 * partition or when Philox({u, t, 4 | x << 16, j >> 2})[j & 3] < edge_loss (x = 0: the random
 * modes' edge draw). */
static int flood_lost(const oracle_sim_t* s, uint32_t u, uint32_t w, uint32_t j, uint32_t x, const uint32_t key[2]) {
  const gossip_config_t* cfg = &s->cfg;
  if (cfg->partitions > 1 &&
      (uint64_t)u * cfg->partitions / s->N != (uint64_t)w * cfg->partitions / s->N) return 1;
  if (cfg->edge_loss) {
    uint32_t ctr[4] = {u, s->t, 4u | (x << 16), j >> 2}, d[4];
    oracle_philox4x32_10(ctr, key, d);
    if (d[j & 3] < cfg->edge_loss) return 1;
  }
  return 0;
}

static int holds(const oracle_sim_t* s, const uint64_t* S, uint64_t n, uint32_t x) {
  return (int)((S[(size_t)(x >> 6) * s->Nl + n] >> (x & 63)) & 1);
}

static uint64_t flood_faults_round(oracle_sim_t* s, uint64_t* Sn) {
  const uint64_t N = s->N;
  const uint32_t R = s->R, D = s->cfg.stall_rounds;
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  uint64_t msgs = 0;
  for (uint64_t u = 0; u < N; ++u) {
    const uint32_t b = s->orow[u], deg = s->orow[u + 1] - b;
    for (uint32_t x = 0; x < R; ++x) {
      if (!holds(s, s->S, u, x)) continue;
      const size_t i = (size_t)x * N + u;
      uint32_t c = s->wcur[i], a = s->watt[i];
      const uint32_t snd = s->wsnd[i];
      while (c < deg) {
        const uint32_t w = s->ocol[b + c];
        if (w == snd) { /* main.go:73 */
          ++c;
          continue;
        }
        ++msgs;
        if (flood_lost(s, (uint32_t)u, w, c, x, key)) {
          if (a < 255) ++a;
          break;
        }
        if (!holds(s, s->S, w, x)) {
          Sn[(size_t)(x >> 6) * s->Nl + w] |= 1ull << (x & 63);
          uint32_t* fs = &s->wsnd[(size_t)x * N + w]; /* WALK_NONE while w does not hold x */
          if ((uint32_t)u < *fs) *fs = (uint32_t)u;
        }
        if (D && a >= D) break; /* expired context: the walk never moves on */
        ++c;
        a = 0;
      }
      s->wcur[i] = c;
      s->watt[i] = (uint8_t)a;
    }
  }
  for (uint32_t x = 0; x < R; ++x) /* the values learned this round: their walks start next round */
    for (uint64_t w = 0; w < N; ++w)
      if (holds(s, Sn, w, x) && !holds(s, s->S, w, x)) {
        s->wcur[(size_t)x * N + w] = 0;
        s->watt[(size_t)x * N + w] = 0;
      }
  return msgs;
}

/* Stall streaks after round t (random modes): every node that is not
 * stalled counts a round in which any of its k exchanges was lost, and resets on a round
 * with none lost.  Depends only on the draws and the fault model, never on S. */
static void stall_update(oracle_sim_t* s) {
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  for (uint64_t n = 0; n < s->N; ++n) {
    if (s->streak[n] >= s->cfg.stall_rounds) continue;
    int any = 0;
    uint32_t x[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < s->k && !any; ++j) {
      if ((j & 3) == 0) {
        uint32_t ctr[4] = {(uint32_t)n, s->t, 0u, j >> 2};
        oracle_philox4x32_10(ctr, key, x);
      }
      any = edge_lost(&s->cfg, s->N, (uint32_t)n, peer_from_word(x[j & 3], s->N, (uint32_t)n), s->t, j, key);
    }
    s->streak[n] = any ? (uint8_t)(s->streak[n] + 1) : 0;
  }
}

static void totals_of(const oracle_sim_t* s, const uint64_t* X, uint64_t* partial);

/* Replicated dense round (plan kinds 5 / 6): S_{t+1} of every node from the whole image of S_t
 * (s->recv: gathered for kind 5, left by the previous replicated round for kind 6), written back
 * into the image; the own slice becomes Snext and the partial holds its totals, as in a sharded
 * dense round.  Same draws, edges and faults as oracle_round_compute. */
static int rep_round(oracle_sim_t* s, uint64_t* partial) {
  const uint64_t N = s->N;
  const uint32_t k = s->k, t = s->t;
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  uint64_t* g = s->recv;
  uint64_t* ni = (uint64_t*)malloc(N * 8);
  if (!ni) return GOSSIP_ENOMEM;
  memcpy(ni, g, N * 8);
  const int do_pull = s->mode == GOSSIP_MODE_PULL || s->mode == GOSSIP_MODE_PUSHPULL;
  const int do_push = s->mode == GOSSIP_MODE_PUSH || s->mode == GOSSIP_MODE_PUSHPULL;
  for (uint64_t sn = 0; sn < N; ++sn) {
    uint32_t n = (uint32_t)sn, x[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < k; ++j) {
      if ((j & 3) == 0) {
        uint32_t ctr[4] = {n, t, 0u, j >> 2};
        oracle_philox4x32_10(ctr, key, x);
      }
      uint32_t p = peer_from_word(x[j & 3], N, n);
      if (lost_edge(s, n, p, j, key)) continue;
      if (do_pull) ni[n] |= g[p];
      if (do_push) ni[p] |= g[n];
    }
  }
  memcpy(g, ni, N * 8);
  memset(s->Snext, 0, (size_t)s->Nl * 8);
  memcpy(s->Snext, ni + s->lo, s->nown * 8);
  free(ni);
  totals_of(s, s->Snext, partial);
  return GOSSIP_OK;
}

int oracle_round_compute(oracle_sim_t* s, uint64_t* partial) {
  if (!s || !partial) return GOSSIP_EINVAL;
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) return ae_round(s, partial);
  if (s->rep_planned) return rep_round(s, partial);
  const uint64_t* g = s->G > 1 ? s->recv : s->send;
  const uint64_t N = s->N, Nl = s->Nl, lo = s->lo, nown = s->nown;
  const uint32_t W = s->W, k = s->k, t = s->t;
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  const int nt = s->threads;
  uint64_t* Sn = s->Snext;
  memcpy(Sn, s->S, (size_t)W * Nl * 8); /* S_{t+1} starts as S_t (OR is monotone) */
  uint64_t msgs = 0;

  if (s->mode == GOSSIP_MODE_FLOOD && s->flood_edges) {
    if (!s->has_topo) return GOSSIP_ESTATE;
    msgs = flood_faults_round(s, Sn);
  } else if (s->mode == GOSSIP_MODE_FLOOD) {
    if (!s->has_topo) return GOSSIP_ESTATE;
    /* main.go:72-75: every node that learned a value last round (frontier F)
     * sends it to each topology neighbour except the one it came from. */
#pragma omp parallel for num_threads(nt) if (nt > 1) schedule(static) reduction(+ : msgs)
    for (uint64_t i = 0; i < nown; ++i) {
      uint64_t v = lo + i;
      uint32_t ob = s->orow[v], oe = s->orow[v + 1], deg = oe - ob;
      for (uint32_t w = 0; w < W; ++w) {
        uint64_t Fv = s->S[(size_t)w * Nl + i] & ~s->Sprev[(size_t)w * Nl + i];
        msgs += (uint64_t)popc64(Fv) * deg - popc64(Fv & s->skip[(size_t)w * Nl + i]);
        uint64_t acc = s->S[(size_t)w * Nl + i];
        for (uint32_t e = s->irow[v]; e < s->irow[v + 1]; ++e) acc |= gword(s, g, s->icol[e], w);
        uint64_t nw = acc & ~s->S[(size_t)w * Nl + i];
        uint64_t seen = 0, sk = 0;
        for (uint32_t e = s->irow[v]; e < s->irow[v + 1] && seen != nw; ++e) {
          uint32_t u = s->icol[e];
          uint64_t c = gword(s, g, u, w) & nw & ~seen;
          if (c && in_sorted(s->ocol + ob, deg, u)) sk |= c; /* sender skip, main.go:73 */
          seen |= c;
        }
        Sn[(size_t)w * Nl + i] = acc;
        s->skip[(size_t)w * Nl + i] = sk;
      }
    }
  } else {
    const int do_pull = s->mode == GOSSIP_MODE_PULL || s->mode == GOSSIP_MODE_PUSHPULL;
    const int do_push = s->mode == GOSSIP_MODE_PUSH || s->mode == GOSSIP_MODE_PUSHPULL;
    if (do_pull) {
#pragma omp parallel for num_threads(nt) if (nt > 1) schedule(static)
      for (uint64_t i = 0; i < nown; ++i) {
        uint32_t n = (uint32_t)(lo + i), x[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < k; ++j) {
          if ((j & 3) == 0) {
            uint32_t ctr[4] = {n, t, 0u, j >> 2};
            oracle_philox4x32_10(ctr, key, x);
          }
          uint32_t p = peer_from_word(x[j & 3], N, n);
          if (lost_edge(s, n, p, j, key)) continue;
          for (uint32_t w = 0; w < W; ++w) Sn[(size_t)w * Nl + i] |= gword(s, g, p, w);
        }
      }
    }
    if (do_push) {
      /* every sender s in [0,N): contributions that land in the owned range */
#pragma omp parallel for num_threads(nt) if (nt > 1) schedule(static)
      for (uint64_t sn = 0; sn < N; ++sn) {
        uint32_t n = (uint32_t)sn, x[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < k; ++j) {
          if ((j & 3) == 0) {
            uint32_t ctr[4] = {n, t, 0u, j >> 2};
            oracle_philox4x32_10(ctr, key, x);
          }
          uint32_t p = peer_from_word(x[j & 3], N, n);
          if (p < lo || p >= lo + nown) continue;
          if (lost_edge(s, n, p, j, key)) continue;
          for (uint32_t w = 0; w < W; ++w) {
            uint64_t v = gword(s, g, n, w);
            if (!v) continue;
            uint64_t* dst = &Sn[(size_t)w * Nl + (p - lo)];
            if (nt > 1) __atomic_fetch_or(dst, v, __ATOMIC_RELAXED);
            else *dst |= v;
          }
        }
      }
    }
  }

  /* stats partials over S_{t+1} */
  uint64_t full = 0, hash = 0, nonzero = 0;
  uint64_t* inf = partial + 4;
  memset(inf, 0, (size_t)s->R * 8);
  const int do_hash = (s->cfg.flags & GOSSIP_FLAG_HASH) != 0;
#pragma omp parallel num_threads(nt) if (nt > 1)
  {
    uint64_t* li = (uint64_t*)calloc(s->R, 8);
    uint64_t lf = 0, lh = 0, lz = 0;
#pragma omp for schedule(static)
    for (uint64_t i = 0; i < nown; ++i) {
      int isfull = 1, nz = 0;
      for (uint32_t w = 0; w < W; ++w) {
        uint64_t x = Sn[(size_t)w * Nl + i];
        nz |= x != 0;
        if ((x & s->fullm[w]) != s->fullm[w]) isfull = 0;
        if (x && do_hash) lh += oracle_mix64(x + ((uint64_t)w * N + lo + i) * GOLD64);
        while (x) {
          int b = __builtin_ctzll(x);
          li[w * 64 + b]++;
          x &= x - 1;
        }
      }
      lf += isfull;
      lz += nz;
    }
#pragma omp critical
    {
      full += lf;
      hash += lh;
      nonzero += lz;
      for (uint32_t r = 0; r < s->R; ++r) inf[r] += li[r];
    }
    free(li);
  }
  partial[0] = full;
  partial[1] = nown;
  partial[2] = msgs;
  partial[3] = hash;
  partial[4 + s->R] = nonzero;
  return GOSSIP_OK;
}

int oracle_round_commit(oracle_sim_t* s, const uint64_t* total, gossip_round_stats_t* st) {
  if (!s || !total) return GOSSIP_EINVAL;
  uint64_t* tmp;
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) {
    uint32_t* tv = s->V; s->V = s->Vn; s->Vn = tv;
    uint8_t* ta = s->alive; s->alive = s->alive_n; s->alive_n = ta;
  } else if (s->mode == GOSSIP_MODE_FLOOD) { /* S_{t-1} <- S_t <- S_{t+1} */
    tmp = s->Sprev; s->Sprev = s->S; s->S = s->Snext; s->Snext = tmp;
  } else if (!s->last_sparse) { /* sparse sharded rounds update S in place */
    tmp = s->S; s->S = s->Snext; s->Snext = tmp;
  }
  s->last_sparse = 0;
  s->pl.rep_img_ok = s->rep_planned; /* the image holds S_{t+1} of every node after a replicated round */
  s->rep_planned = 0;
  if (s->streak) stall_update(s); /* (uses s->t: the round just computed) */
  memcpy(s->gtot, total, oracle_partial_len(s) * 8);
  s->gtot_valid = 1;
  if (st) {
    st->round = s->t;
    st->full_nodes = total[0];
    st->alive_nodes = total[1];
    st->converged = total[0] == total[1];
    st->messages = total[2];
    st->state_hash = (s->cfg.flags & GOSSIP_FLAG_HASH) ? total[3] : 0;
  }
  s->t++;
  return GOSSIP_OK;
}

/* ---------------- sparse sharded rounds (include/gossip.h) --------
 * Plain restatement of the engine's protocol for the driver tests: the same
 * items and phases, planned by the same csrc/plan.h (the plan changes no result);
 * lookups by binary search in the sorted lists. */

static int sparse_ok(const oracle_sim_t* s) {
  return s->G > 1 && s->W == 1 && s->mode >= GOSSIP_MODE_PUSH && s->mode <= GOSSIP_MODE_PUSHPULL;
}

/* rare under maj: 0 -> nonzero, 1 -> not full (one word: W == 1) */
static inline int is_rare(const oracle_sim_t* s, uint64_t x) { return s->maj ? x != s->fullm[0] : x != 0; }

/* totals of the owned nodes' state X (same layout as round_compute) */
static void totals_of(const oracle_sim_t* s, const uint64_t* X, uint64_t* partial) {
  memset(partial, 0, oracle_partial_len(s) * 8);
  const int do_hash = (s->cfg.flags & GOSSIP_FLAG_HASH) != 0;
  for (uint64_t i = 0; i < s->nown; ++i) {
    uint64_t x = X[i];
    partial[0] += (x & s->fullm[0]) == s->fullm[0];
    partial[4 + s->R] += x != 0;
    if (x && do_hash) partial[3] += oracle_mix64(x + (s->lo + i) * GOLD64);
    while (x) {
      partial[4 + __builtin_ctzll(x)]++;
      x &= x - 1;
    }
  }
  partial[1] = s->nown;
}

static void own_totals(const oracle_sim_t* s, uint64_t* partial) { totals_of(s, s->S, partial); }

int oracle_local_totals(oracle_sim_t* s, uint64_t* partial) {
  if (!s || !partial || !sparse_ok(s)) return GOSSIP_EINVAL;
  own_totals(s, partial);
  return GOSSIP_OK;
}

int oracle_sharded_plan(oracle_sim_t* s, const uint64_t* total, int32_t* kind) {
  if (!s || !kind) return GOSSIP_EINVAL;
  s->planned = s->xd_planned = s->cc_planned = s->rep_planned = 0;
  if (s->aex) {
    *kind = s->aex_target_ok ? 2 : -2;
    return GOSSIP_OK;
  }
  if (!sparse_ok(s)) {
    *kind = 0;
    return GOSSIP_OK;
  }
  if (total) {
    memcpy(s->gtot, total, oracle_partial_len(s) * 8);
    s->gtot_valid = 1;
  }
  if (!s->gtot_valid) {
    *kind = -1;
    return GOSSIP_OK;
  }
  const plan_round p = plan_sharded_round(&s->pl, s->gtot);
  s->planned = p.sparse, s->rep_planned = p.rep, s->xd_planned = p.xd, s->cc_planned = p.cc;
  s->maj = p.maj;
  s->xd_filt = p.xd_filt;
  s->xcls_ok = 0;
  *kind = p.kind;
  return GOSSIP_OK;
}

int oracle_sparse_rare(oracle_sim_t* s, void** send, uint64_t* count) {
  if (!s || !send || !count || !s->planned) return GOSSIP_ESTATE;
  if (!s->rare_send && !(s->rare_send = (uint64_t*)calloc(2 * s->Nl, 8))) return GOSSIP_ENOMEM;
  uint64_t c = 0;
  for (uint64_t i = 0; i < s->nown; ++i)
    if (is_rare(s, s->S[i])) {
      s->rare_send[2 * c] = s->lo + i;
      s->rare_send[2 * c + 1] = s->S[i];
      ++c;
    }
  *send = s->rare_send;
  *count = c;
  return GOSSIP_OK;
}

int oracle_sparse_rare_recv(oracle_sim_t* s, uint64_t stride, void** recv) {
  if (!s || !recv || !s->planned || stride > s->Nl) return GOSSIP_EINVAL;
  free(s->rare_recv);
  s->rare_recv = (uint64_t*)calloc(2 * (stride * s->G + 1), 8);
  if (!s->rare_recv) return GOSSIP_ENOMEM;
  s->stride = stride;
  *recv = s->rare_recv;
  return GOSSIP_OK;
}

/* S_t of node p if it is rare (in its owner's list), else -1 */
static int rare_lookup(const oracle_sim_t* s, uint64_t p, uint64_t* v) {
  uint64_t q = p / s->Nl, lo = 0, hi = s->counts[q];
  const uint64_t* list = s->rare_recv + 2 * q * s->stride;
  while (lo < hi) {
    uint64_t mid = (lo + hi) / 2;
    if (list[2 * mid] < p) lo = mid + 1; else hi = mid;
  }
  if (lo < s->counts[q] && list[2 * lo] == p) {
    *v = list[2 * lo + 1];
    return 1;
  }
  return 0;
}

int oracle_sparse_scan(oracle_sim_t* s, const uint64_t* counts, void** send, uint64_t* send_counts) {
  if (!s || !counts || !send || !send_counts || !s->planned || !s->rare_recv) return GOSSIP_EINVAL;
  for (uint32_t q = 0; q < s->G; ++q) {
    if (counts[q] > s->stride) return GOSSIP_EINVAL;
    s->counts[q] = counts[q];
  }
  const uint64_t cap = (uint64_t)s->k * s->nown + 1;
  if (!s->msg_send && !(s->msg_send = (uint64_t*)calloc(2 * cap, 8))) return GOSSIP_ENOMEM;
  if (!s->D && !(s->D = (uint64_t*)calloc(s->Nl, 8))) return GOSSIP_ENOMEM;
  /* pending pushes per owner, then grouped */
  uint64_t* tmp = (uint64_t*)malloc(3 * cap * 8);
  if (!tmp) return GOSSIP_ENOMEM;
  uint64_t nt = 0;
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  const int do_pull = s->mode != GOSSIP_MODE_PUSH, do_push = s->mode != GOSSIP_MODE_PULL;
  const uint64_t majv = s->maj ? s->fullm[0] : 0;
  memcpy(s->Snext, s->S, s->Nl * 8); /* pulls land in Snext; S stays S_t during the scan */
  for (uint64_t i = 0; i < s->nown; ++i) {
    const uint32_t n = (uint32_t)(s->lo + i);
    const uint64_t x = s->S[i];
    const int rn = is_rare(s, x);
    uint32_t r[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < s->k; ++j) {
      if ((j & 3) == 0) {
        uint32_t ctr[4] = {n, s->t, 0u, j >> 2};
        oracle_philox4x32_10(ctr, key, r);
      }
      const uint32_t p = peer_from_word(r[j & 3], s->N, n);
      if (lost_edge(s, n, p, j, key)) continue;
      uint64_t v = majv;
      int rp;
      if (p >= s->lo && p < s->hi) {
        v = s->S[p - s->lo];
        rp = is_rare(s, v);
        if (!rp) v = majv;
      } else {
        rp = rare_lookup(s, p, &v);
      }
      if (!rn && !rp) continue; /* both ends majority: nothing moves */
      if (do_pull) s->Snext[i] |= v;
      if (do_push && (x & ~v)) {
        if (p >= s->lo && p < s->hi) {
          s->D[p - s->lo] |= x & ~v;
        } else {
          const uint64_t q = p / s->Nl;
          tmp[3 * nt] = q;
          tmp[3 * nt + 1] = p - q * s->Nl;
          tmp[3 * nt + 2] = x & ~v;
          ++nt;
        }
      }
    }
  }
  uint64_t c = 0;
  for (uint32_t q = 0; q < s->G; ++q) {
    send_counts[q] = 0;
    for (uint64_t m = 0; m < nt; ++m)
      if (tmp[3 * m] == q) {
        s->msg_send[2 * c] = tmp[3 * m + 1];
        s->msg_send[2 * c + 1] = tmp[3 * m + 2];
        ++c;
        ++send_counts[q];
      }
  }
  free(tmp);
  *send = s->msg_send;
  return GOSSIP_OK;
}

int oracle_sparse_msg_recv(oracle_sim_t* s, uint64_t items, void** recv) {
  if (!s || !recv || !s->planned) return GOSSIP_EINVAL;
  free(s->msg_recv);
  s->msg_recv = (uint64_t*)calloc(2 * (items + 1), 8);
  if (!s->msg_recv) return GOSSIP_ENOMEM;
  s->msg_cap = items;
  *recv = s->msg_recv;
  return GOSSIP_OK;
}

int oracle_sparse_commit(oracle_sim_t* s, uint64_t items, uint64_t* partial) {
  if (!s || !partial || !s->planned || items > s->msg_cap || !s->D) return GOSSIP_EINVAL;
  for (uint64_t m = 0; m < items; ++m) s->D[s->msg_recv[2 * m]] |= s->msg_recv[2 * m + 1];
  for (uint64_t i = 0; i < s->nown; ++i) {
    s->S[i] = s->Snext[i] | s->D[i];
    s->D[i] = 0;
  }
  own_totals(s, partial);
  s->planned = 0;
  s->last_sparse = 1;
  return GOSSIP_OK;
}

/* ---------------- exchange dense rounds (include/gossip.h gossip_xd_*) ----
 * Each live edge n -> p of an own sender is one item for p's owner: id = (p - owner*Nl) |
 * NO_PUSH / NO_PULL, value = S_t[n] (0 without a push) — the directions as the engine's
 * sender_dirs (a push needs S_t[n] != 0, a pull S_t[n] != full).  The owner ORs pushes into
 * S_{t+1}[p] and replies S_t[p] to pulls in the received order; the replies are ORed into
 * S_{t+1}[n].  (main.go:65-89: each exchange is one request and its reply.) */
#define XD_NO_PUSH (1u << 30)
#define XD_NO_PULL (1u << 31)

/* The own slot of the class image ([nz][full], nwl words each) when this round filters. */
int oracle_xd_classes(oracle_sim_t* s, void** send, void** image, uint64_t* bytes) {
  if (!s || !send || !image || !bytes) return GOSSIP_EINVAL;
  if (!s->xd_planned) return GOSSIP_ESTATE;
  *send = *image = NULL;
  *bytes = 0;
  if (!s->xd_filt) return GOSSIP_OK;
  const uint64_t nwl = (s->Nl + 63) / 64, fm = s->fullm[0];
  if (!s->xcls && !(s->xcls = (uint64_t*)calloc(2 * nwl * s->G, 8))) return GOSSIP_ENOMEM;
  uint64_t* own = s->xcls + (size_t)s->rank * 2 * nwl;
  memset(own, 0, 2 * nwl * 8);
  for (uint64_t i = 0; i < s->nown; ++i) {
    if (s->S[i]) own[i / 64] |= 1ull << (i & 63);
    if (s->S[i] == fm) own[nwl + i / 64] |= 1ull << (i & 63);
  }
  s->xcls_ok = 1;
  *send = own;
  *image = s->xcls;
  *bytes = 2 * nwl * 8;
  return GOSSIP_OK;
}

/* directions kept of edge n -> p (bit 0 push, bit 1 pull) under the round's filter: a one-way
 * edge into a peer that cannot gain (push into full) or give (pull from empty) moves nothing */
static int xd_keep(const oracle_sim_t* s, int push, int pull, uint64_t p) {
  if (!s->xcls_ok || !s->xd_filt) return push | (pull << 1);
  const uint64_t nwl = (s->Nl + 63) / 64, q = p / s->Nl, pl = p - q * s->Nl;
  const uint64_t* slot = s->xcls + (size_t)q * 2 * nwl;
  const int nz = (int)((slot[pl / 64] >> (pl & 63)) & 1), full = (int)((slot[nwl + pl / 64] >> (pl & 63)) & 1);
  if ((s->xd_filt & 1u) && !push && pull && !nz) return 0;
  if ((s->xd_filt & 2u) && push && !pull && full) return 0;
  return push | (pull << 1);
}

int oracle_xd_requests(oracle_sim_t* s, void** ids, void** vals, uint64_t* send_counts) {
  if (!s || !ids || !vals || !send_counts || !s->xd_planned) return GOSSIP_ESTATE;
  const uint64_t cap = (uint64_t)s->k * s->nown + 1;
  if (!s->xid && !(s->xid = (uint32_t*)calloc(cap, 4))) return GOSSIP_ENOMEM;
  if (!s->xval && !(s->xval = (uint64_t*)calloc(cap, 8))) return GOSSIP_ENOMEM;
  if (!s->xnode && !(s->xnode = (uint64_t*)calloc(cap, 8))) return GOSSIP_ENOMEM;
  if (!s->xrep_in && !(s->xrep_in = (uint64_t*)calloc(cap, 8))) return GOSSIP_ENOMEM;
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  const int can_push = s->mode != GOSSIP_MODE_PULL, can_pull = s->mode != GOSSIP_MODE_PUSH;
  memcpy(s->Snext, s->S, s->Nl * 8); /* S_{t+1} starts as S_t */
  uint64_t* pos = (uint64_t*)calloc(s->G + 1, 8);
  if (!pos) return GOSSIP_ENOMEM;
  for (int pass = 0; pass < 2; ++pass) { /* count per owner, then place (owner-major, sender order) */
    if (pass == 1)
      for (uint32_t q = 0, a = 0; q <= s->G; ++q) {
        const uint64_t c = q < s->G ? pos[q] : 0;
        if (q < s->G) send_counts[q] = c;
        pos[q] = a;
        a += (uint32_t)c;
      }
    for (uint64_t i = 0; i < s->nown; ++i) {
      const uint32_t n = (uint32_t)(s->lo + i);
      const uint64_t x = s->S[i];
      const int push = can_push && x != 0, pull = can_pull && x != s->fullm[0];
      if (!push && !pull) continue;
      uint32_t r[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; j < s->k; ++j) {
        if ((j & 3) == 0) {
          uint32_t ctr[4] = {n, s->t, 0u, j >> 2};
          oracle_philox4x32_10(ctr, key, r);
        }
        const uint32_t p = peer_from_word(r[j & 3], s->N, n);
        if (lost_edge(s, n, p, j, key)) continue;
        const int d = xd_keep(s, push, pull, p);
        if (!d) continue;
        const uint64_t q = p / s->Nl;
        if (pass == 0) {
          pos[q]++;
          continue;
        }
        const uint64_t at = pos[q]++;
        s->xid[at] = (uint32_t)(p - q * s->Nl) | ((d & 1) ? 0u : XD_NO_PUSH) | ((d & 2) ? 0u : XD_NO_PULL);
        s->xval[at] = (d & 1) ? x : 0;
        s->xnode[at] = i;
      }
    }
  }
  s->xn_out = 0;
  for (uint32_t q = 0; q < s->G; ++q) s->xn_out += send_counts[q];
  free(pos);
  *ids = s->xid;
  *vals = s->xval;
  return GOSSIP_OK;
}

int oracle_xd_request_recv(oracle_sim_t* s, uint64_t items, void** ids, void** vals) {
  if (!s || !ids || !vals || !s->xd_planned) return GOSSIP_ESTATE;
  free(s->xrid); free(s->xrval); free(s->xrep_out);
  s->xrid = (uint32_t*)calloc(items + 1, 4);
  s->xrval = (uint64_t*)calloc(items + 1, 8);
  s->xrep_out = (uint64_t*)calloc(items + 1, 8);
  if (!s->xrid || !s->xrval || !s->xrep_out) return GOSSIP_ENOMEM;
  s->xn_in = items;
  *ids = s->xrid;
  *vals = s->xrval;
  return GOSSIP_OK;
}

int oracle_xd_serve(oracle_sim_t* s, void** replies) {
  if (!s || !replies || !s->xd_planned || !s->xrid) return GOSSIP_ESTATE;
  for (uint64_t i = 0; i < s->xn_in; ++i) {
    const uint32_t id = s->xrid[i];
    const uint64_t p = id & (XD_NO_PUSH - 1u);
    if (p >= s->nown) return GOSSIP_EINVAL;
    if (!(id & XD_NO_PUSH)) s->Snext[p] |= s->xrval[i];
    s->xrep_out[i] = (id & XD_NO_PULL) ? 0 : s->S[p];
  }
  *replies = s->xrep_out;
  return GOSSIP_OK;
}

int oracle_xd_response_recv(oracle_sim_t* s, void** replies) {
  if (!s || !replies || !s->xd_planned || !s->xrep_in) return GOSSIP_ESTATE;
  *replies = s->xrep_in;
  return GOSSIP_OK;
}

int oracle_xd_finish(oracle_sim_t* s, uint64_t* partial) {
  if (!s || !partial || !s->xd_planned || !s->xrep_in) return GOSSIP_ESTATE;
  for (uint64_t j = 0; j < s->xn_out; ++j) s->Snext[s->xnode[j]] |= s->xrep_in[j];
  totals_of(s, s->Snext, partial);
  s->xd_planned = s->xcls_ok = 0;
  s->last_sparse = 0;
  return GOSSIP_OK;
}

/* ---- class-coded state all-gather (include/gossip.h gossip_cc_*; the engine's
 * csrc/sharded.hip cc_compact / cc_expand).  The image the dense round reads is the
 * all-gathered S_t of oracle_exchange_buffers, rebuilt from each shard's classes:
 * empty -> 0, full -> the R-bit mask, mixed -> its word (in id order). ---- */
static uint64_t cc_full(const oracle_sim_t* s) { return s->R >= 64 ? ~0ull : ((1ull << s->R) - 1ull); }
static uint64_t cc_slot(uint64_t nwl) { return 2 * nwl + (nwl + 1) / 2; } /* sharded.h cc_slot_words */

int oracle_cc_send(oracle_sim_t* s, void** bits, uint64_t* bits_bytes, void** vals, uint64_t* count) {
  if (!s || !bits || !bits_bytes || !vals || !count) return GOSSIP_EINVAL;
  if (!s->cc_planned) return GOSSIP_ESTATE;
  const uint64_t nwl = (s->Nl + 63) / 64, fm = cc_full(s);
  if (!s->cc_bits && !(s->cc_bits = (uint64_t*)calloc(cc_slot(nwl) * s->G, 8))) return GOSSIP_ENOMEM;
  if (!s->cc_send && !(s->cc_send = (uint64_t*)calloc(s->Nl + 1, 8))) return GOSSIP_ENOMEM;
  uint64_t* own = s->cc_bits + (size_t)s->rank * cc_slot(nwl);
  uint32_t* pre = (uint32_t*)(own + 2 * nwl);
  memset(own, 0, cc_slot(nwl) * 8);
  uint64_t c = 0;
  for (uint64_t i = 0; i < s->nown; ++i) {
    const uint64_t v = s->S[i], bit = 1ull << (i & 63);
    if ((i & 63) == 0) pre[i / 64] = (uint32_t)c;
    if (!v) continue;
    own[i / 64] |= bit;
    if (v == fm) own[nwl + i / 64] |= bit;
    else s->cc_send[c++] = v;
  }
  *bits = own;
  *bits_bytes = cc_slot(nwl) * 8;
  *vals = s->cc_send;
  *count = c;
  return GOSSIP_OK;
}

int oracle_cc_recv(oracle_sim_t* s, uint64_t stride, void** bits_image, void** vals_image) {
  if (!s || !bits_image || !vals_image) return GOSSIP_EINVAL;
  if (!s->cc_planned || !s->cc_bits) return GOSSIP_ESTATE;
  if (stride > s->Nl) return GOSSIP_EINVAL;
  free(s->cc_vals);
  if (!(s->cc_vals = (uint64_t*)calloc(stride * s->G + 1, 8))) return GOSSIP_ENOMEM;
  s->cc_stride = stride;
  *bits_image = s->cc_bits;
  *vals_image = s->cc_vals;
  return GOSSIP_OK;
}

int oracle_cc_expand(oracle_sim_t* s, const uint64_t* counts) {
  if (!s || !counts) return GOSSIP_EINVAL;
  if (!s->cc_planned || !s->cc_vals) return GOSSIP_ESTATE;
  const uint64_t nwl = (s->Nl + 63) / 64, fm = cc_full(s);
  for (uint32_t q = 0; q < s->G; ++q) {
    if (counts[q] > s->cc_stride) return GOSSIP_EINVAL;
    uint64_t* img = s->recv + (size_t)q * s->Nl;
    if (q == s->rank) {
      memcpy(img, s->S, s->Nl * 8);
      continue;
    }
    const uint64_t *nz = s->cc_bits + (size_t)q * cc_slot(nwl), *full = nz + nwl;
    const uint32_t* pre = (const uint32_t*)(full + nwl);
    const uint64_t nq = (uint64_t)q * s->Nl < s->N ? (s->N - (uint64_t)q * s->Nl < s->Nl ? s->N - (uint64_t)q * s->Nl : s->Nl) : 0;
    uint64_t c = 0;
    for (uint64_t i = 0; i < nq; ++i) {
      const uint64_t bit = 1ull << (i & 63);
      uint64_t v = 0;
      if ((i & 63) == 0 && pre[i / 64] != c) return GOSSIP_EINVAL; /* the prefix the sender wrote */
      if (full[i / 64] & bit) v = fm;
      else if (nz[i / 64] & bit) {
        if (c >= counts[q]) return GOSSIP_EINVAL; /* more mixed nodes than words sent */
        v = s->cc_vals[q * s->cc_stride + c++];
      }
      img[i] = v;
    }
    for (uint64_t i = nq; i < s->Nl; ++i) img[i] = 0;
    if (c != counts[q]) return GOSSIP_EINVAL;
  }
  s->cc_planned = 0;
  return GOSSIP_OK;
}

/* gossip_set_param: the engine's tuning knobs.  sparse_frac, link_gbps, cc_frac, xd_shards,
 * xd_filter_frac and replicate matter here (plan.h picks the sharded round
 * protocol from them, which the gloo tests exercise); the rest steer engine kernel
 * choices that this restatement does not have, and are accepted as no-ops. */
int oracle_set_param(oracle_sim_t* s, const char* name, double value) {
  if (!s || !name) return GOSSIP_EINVAL;
  if (!strcmp(name, "sparse_frac")) {
    s->pl.sparse_frac = value;
    s->pl.sparse_frac_set = 1;
    return GOSSIP_OK;
  }
  if (!strcmp(name, "link_gbps")) {
    if (value < 0) return GOSSIP_EINVAL;
    s->pl.link_gbps = value;
    return GOSSIP_OK;
  }
  if (!strcmp(name, "replicate")) { /* < 0: by the cost model, 0: never, > 0: every dense round */
    s->pl.replicate = value < 0 ? -1 : value > 0 ? 1 : 0;
    return GOSSIP_OK;
  }
  if (!strcmp(name, "cc_frac")) {
    if (value < 0 || value > 1) return GOSSIP_EINVAL;
    s->pl.cc_frac = value;
    return GOSSIP_OK;
  }
  if (!strcmp(name, "xd_shards")) {
    if (value < 0 || value > 1024) return GOSSIP_EINVAL;
    s->pl.xd_shards = (uint32_t)value;
    return GOSSIP_OK;
  }
  if (!strcmp(name, "xd_filter_frac")) {
    if (value < 0 || value > 1) return GOSSIP_EINVAL;
    s->pl.xd_filter_frac = value;
    return GOSSIP_OK;
  }
  /* the engine's performance knobs (path choice, grids): no effect on the rounds' results */
  const char* known[] = {"alld_frac",  "filter_frac", "ahead",        "ae_sparse",  "ae_cap",      "sparse_direct",
                         "mid_frac",   "bin_scan_frac", "ae_dense_bin", "ae_dense_cap", "ae_ahead", "ordered_collectives",
                         "ae_dense_filter", "rccl_dev_collectives", "scan_queue", "place_tries", "timing"};
  for (size_t i = 0; i < sizeof known / sizeof known[0]; ++i)
    if (!strcmp(name, known[i])) return GOSSIP_OK;
  return GOSSIP_EINVAL;
}

int oracle_set_faults(oracle_sim_t* s, uint32_t edge_loss, uint32_t partitions) {
  if (!s) return GOSSIP_EINVAL;
  if ((edge_loss || partitions > 1) &&
      (s->mode == GOSSIP_MODE_ANTIENTROPY || (s->mode == GOSSIP_MODE_FLOOD && !s->flood_edges)))
    return GOSSIP_ENOTSUP; /* FLOOD retries need the per-edge state: create with faults or stall_rounds */
  s->cfg.edge_loss = edge_loss;
  s->cfg.partitions = partitions;
  s->pl.edge_loss = edge_loss, s->pl.partitions = partitions;
  return GOSSIP_OK;
}

int oracle_step(oracle_sim_t* s, uint32_t max_rounds, gossip_round_stats_t* stats,
                uint64_t* infected, uint32_t* rounds_done) {
  if (!s) return GOSSIP_EINVAL;
  if (s->G != 1) return GOSSIP_ESTATE;
  if (s->mode == GOSSIP_MODE_FLOOD && !s->has_topo) return GOSSIP_ESTATE;
  uint64_t* partial = (uint64_t*)malloc(oracle_partial_len(s) * 8);
  if (!partial) return GOSSIP_ENOMEM;
  uint32_t r = 0;
  int rc = GOSSIP_OK;
  while (r < max_rounds) {
    gossip_round_stats_t st;
    oracle_exchange_buffers(s, NULL, NULL, NULL);
    if ((rc = oracle_round_compute(s, partial)) != GOSSIP_OK) break;
    oracle_round_commit(s, partial, &st);
    if (stats) stats[r] = st;
    if (infected) memcpy(infected + (size_t)r * s->R, partial + 4, (size_t)s->R * 8);
    ++r;
    if (st.converged || (s->mode == GOSSIP_MODE_FLOOD && st.messages == 0)) break;
  }
  free(partial);
  if (rounds_done) *rounds_done = r;
  return rc;
}

int oracle_read_bitset(oracle_sim_t* s, uint64_t node, uint64_t* out, uint32_t nwords) {
  if (!s || !out || node < s->lo || node >= s->hi || nwords < s->W) return GOSSIP_EINVAL;
  for (uint32_t w = 0; w < s->W; ++w) out[w] = s->S[(size_t)w * s->Nl + (node - s->lo)];
  return GOSSIP_OK;
}

int oracle_read_shard(oracle_sim_t* s, uint64_t* out, uint64_t n_words) {
  if (!s || !out || n_words < (uint64_t)s->W * s->nown) return GOSSIP_EINVAL;
  for (uint32_t w = 0; w < s->W; ++w)
    memcpy(out + (size_t)w * s->nown, s->S + (size_t)w * s->Nl, s->nown * 8);
  return GOSSIP_OK;
}

int oracle_shard_range(const oracle_sim_t* s, uint64_t* lo, uint64_t* hi) {
  if (!s) return GOSSIP_EINVAL;
  if (lo) *lo = s->lo;
  if (hi) *hi = s->hi;
  return GOSSIP_OK;
}

int oracle_state_hash(oracle_sim_t* s, uint64_t* out) {
  if (!s || !out) return GOSSIP_EINVAL;
  uint64_t h = 0;
  if (s->mode == GOSSIP_MODE_ANTIENTROPY) {
    for (uint64_t n = 0; n < s->N; ++n)
      for (uint32_t c = 0; c < s->R; ++c) {
        uint32_t v = s->V[n * s->R + c];
        if (v) h += oracle_mix64((uint64_t)v + ((uint64_t)c * s->N + n) * GOLD64);
      }
    *out = h;
    return GOSSIP_OK;
  }
  for (uint32_t w = 0; w < s->W; ++w)
    for (uint64_t i = 0; i < s->nown; ++i) {
      uint64_t x = s->S[(size_t)w * s->Nl + i];
      if (x) h += oracle_mix64(x + ((uint64_t)w * s->N + s->lo + i) * GOLD64);
    }
  *out = h;
  return GOSSIP_OK;
}

int oracle_read_versions(oracle_sim_t* s, uint64_t node, uint32_t* out, uint32_t ncomp, uint32_t* alive) {
  if (!s || !out || !s->V || node >= s->N || ncomp < s->R) return GOSSIP_EINVAL;
  if (s->aex && (node < s->lo || node >= s->hi)) return GOSSIP_EINVAL;
  memcpy(out, s->V + (node - (s->aex ? s->lo : 0)) * s->R, (size_t)s->R * 4);
  if (alive) *alive = s->aex ? (uint32_t)alive_bit(s, node) : s->alive[node];
  return GOSSIP_OK;
}

uint32_t oracle_round_index(const oracle_sim_t* s) { return s ? s->t : 0; }

int oracle_read_rows(oracle_sim_t* s, uint32_t* out, uint64_t n_values) {
  if (!s || !out || !s->V || n_values < s->nown * s->R) return GOSSIP_EINVAL;
  memcpy(out, s->V + (s->aex ? 0 : s->lo * s->R), (size_t)s->nown * s->R * 4);
  return GOSSIP_OK;
}

/* ---------------- sharded ANTIENTROPY (include/gossip.h gossip_ae_*) --------
 * Rows sharded in 64-aligned blocks; every shard churns the alive flags of all N nodes (a
 * per-node Philox draw) and receives every shard's stale words per round.  An exchange
 * (n, p_j(n,t)) of two alive nodes with a stale end and p on another shard is a request item
 * {p, n, V_t[n]} to p's owner, who max-merges it into p and answers V_t[p]. */
static inline int alive_bit(const oracle_sim_t* s, uint64_t n) { return (s->aex_img[2 * (n >> 6)] >> (n & 63)) & 1; }
static inline int stale_bit(const oracle_sim_t* s, uint64_t n) { return (s->aex_img[2 * (n >> 6) + 1] >> (n & 63)) & 1; }

static void aex_own_stale(oracle_sim_t* s, const uint32_t* V) {
  uint64_t* own = s->aex_img + (size_t)s->rank * s->Nl / 32;
  for (uint64_t w = 0; w < s->Nl / 64; ++w) own[2 * w + 1] = 0;
  for (uint64_t i = 0; i < s->nown; ++i)
    for (uint32_t c = 0; c < s->R; ++c)
      if (V[i * s->R + c] != s->target[c]) {
        own[2 * (i >> 6) + 1] |= 1ull << (i & 63);
        break;
      }
}

/* every own node alive (before round 0's churn) */
static void aex_own_fill_alive(oracle_sim_t* s) {
  if (!s->aex_img) return; /* (allocation failed: create reports it) */
  uint64_t* own = s->aex_img + (size_t)s->rank * s->Nl / 32;
  for (uint64_t w = 0; w < s->Nl / 64; ++w) own[2 * w] = 0;
  for (uint64_t i = 0; i < s->nown; ++i) own[2 * (i >> 6)] |= 1ull << (i & 63);
  s->aex_churned = UINT32_MAX;
}

uint32_t oracle_ae_item_words(const oracle_sim_t* s, uint32_t which) {
  return s && s->aex ? (which == 0 ? s->rw : s->pw) : 0;
}

int oracle_ae_local_target(oracle_sim_t* s, uint32_t* out) {
  if (!s || !out || !s->aex) return GOSSIP_EINVAL;
  memset(out, 0, (size_t)s->R * 4);
  for (uint64_t i = 0; i < s->nown; ++i)
    for (uint32_t c = 0; c < s->R; ++c)
      if (s->V[i * s->R + c] > out[c]) out[c] = s->V[i * s->R + c];
  return GOSSIP_OK;
}

int oracle_ae_set_target(oracle_sim_t* s, const uint32_t* target) {
  if (!s || !target || !s->aex) return GOSSIP_EINVAL;
  memcpy(s->target, target, (size_t)s->R * 4);
  aex_own_stale(s, s->V);
  s->aex_target_ok = 1;
  return GOSSIP_OK;
}

int oracle_ae_requests(oracle_sim_t* s, void** send, uint64_t* send_counts) {
  if (!s || !send || !send_counts || !s->aex || !s->aex_target_ok) return GOSSIP_EINVAL;
  if (s->aex_churned != s->t) return GOSSIP_ESTATE; /* oracle_exchange_buffers (and its all-gather) first */
  const uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)};
  const uint32_t K = s->R;
  memcpy(s->Vn, s->V, (size_t)s->nown * K * 4);
  s->aex_msgs = 0;
  s->nreq = s->nloc = 0;
  for (uint32_t q = 0; q < s->G; ++q) send_counts[q] = 0;
  /* pass 0: messages and own-own pairs; pass q + 1: the requests to owner q, in node order */
  for (uint32_t pass = 0; pass <= s->G; ++pass) {
    for (uint64_t i = 0; i < s->nown; ++i) {
      const uint64_t n = s->lo + i;
      if (!alive_bit(s, n)) continue;
      uint32_t x[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; j < s->k; ++j) {
        if ((j & 3) == 0) {
          uint32_t ctr[4] = {(uint32_t)n, s->t, 0u, j >> 2};
          oracle_philox4x32_10(ctr, key, x);
        }
        const uint32_t p = peer_from_word(x[j & 3], s->N, (uint32_t)n);
        if (!alive_bit(s, p)) continue;
        if (pass == 0) ++s->aex_msgs;
        if (!stale_bit(s, n) && !stale_bit(s, p)) continue;
        const uint32_t q = (uint32_t)(p / s->Nl);
        if (pass == 0) {
          if (q == s->rank) {
            s->loc[2 * s->nloc] = (uint32_t)i;
            s->loc[2 * s->nloc + 1] = (uint32_t)(p - s->lo);
            ++s->nloc;
          }
        } else if (q == pass - 1 && q != s->rank) {
          uint32_t* it = s->req + s->nreq * s->rw;
          it[0] = p;
          it[1] = (uint32_t)n;
          memcpy(it + 2, s->V + i * K, (size_t)K * 4);
          ++s->nreq;
          ++send_counts[q];
        }
      }
    }
  }
  *send = s->req;
  return GOSSIP_OK;
}

int oracle_ae_request_recv(oracle_sim_t* s, uint64_t items, void** recv) {
  if (!s || !recv || !s->aex) return GOSSIP_EINVAL;
  if (items > s->in_cap || !s->in) {
    free(s->in);
    free(s->resp_out);
    s->in = (uint32_t*)calloc((items + 1) * s->rw, 4);
    s->resp_out = (uint32_t*)calloc((items + 1) * s->pw, 4);
    if (!s->in || !s->resp_out) return GOSSIP_ENOMEM;
    s->in_cap = items;
  }
  s->nin = items;
  *recv = s->in;
  return GOSSIP_OK;
}

int oracle_ae_serve(oracle_sim_t* s, void** send) {
  if (!s || !send || !s->aex || !s->in) return GOSSIP_EINVAL;
  const uint32_t K = s->R;
  for (uint64_t m = 0; m < s->nin; ++m) {
    const uint32_t* it = s->in + m * s->rw;
    const uint64_t pl = it[0] - s->lo;
    for (uint32_t c = 0; c < K; ++c) {
      s->resp_out[m * s->pw + c] = s->V[pl * K + c];
      if (it[2 + c] > s->Vn[pl * K + c]) s->Vn[pl * K + c] = it[2 + c];
    }
  }
  *send = s->resp_out;
  return GOSSIP_OK;
}

int oracle_ae_response_recv(oracle_sim_t* s, void** recv) {
  if (!s || !recv || !s->aex) return GOSSIP_EINVAL;
  *recv = s->resp_in;
  return GOSSIP_OK;
}

int oracle_ae_finish(oracle_sim_t* s, uint64_t* partial) {
  if (!s || !partial || !s->aex) return GOSSIP_EINVAL;
  const uint32_t K = s->R;
  for (uint64_t m = 0; m < s->nreq; ++m) {
    const uint64_t nl = s->req[m * s->rw + 1] - s->lo;
    for (uint32_t c = 0; c < K; ++c)
      if (s->resp_in[m * s->pw + c] > s->Vn[nl * K + c]) s->Vn[nl * K + c] = s->resp_in[m * s->pw + c];
  }
  for (uint64_t e = 0; e < s->nloc; ++e) {
    const uint64_t nl = s->loc[2 * e], pl = s->loc[2 * e + 1];
    for (uint32_t c = 0; c < K; ++c) {
      const uint32_t a = s->V[nl * K + c], b = s->V[pl * K + c];
      if (b > s->Vn[nl * K + c]) s->Vn[nl * K + c] = b;
      if (a > s->Vn[pl * K + c]) s->Vn[pl * K + c] = a;
    }
  }
  memset(partial, 0, oracle_partial_len(s) * 8);
  for (uint64_t i = 0; i < s->nown; ++i) {
    const uint64_t n = s->lo + i;
    int isfull = 1;
    for (uint32_t c = 0; c < K; ++c) {
      const uint32_t v = s->Vn[i * K + c];
      if (v && (s->cfg.flags & GOSSIP_FLAG_HASH)) partial[3] += oracle_mix64((uint64_t)v + ((uint64_t)c * s->N + n) * GOLD64);
      if (v != s->target[c]) isfull = 0;
      else if (alive_bit(s, n)) partial[4 + c]++;
    }
    if (alive_bit(s, n)) {
      partial[1]++;
      partial[0] += isfull;
    }
  }
  partial[2] = s->aex_msgs;
  aex_own_stale(s, s->Vn);
  return GOSSIP_OK;
}
