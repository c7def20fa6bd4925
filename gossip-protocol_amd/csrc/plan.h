/* plan.h — the round planner of the random modes: the mean-field predictor, the per-rank cost model of
 * a sharded round and the choice of its kind (0 / 1 / 3 / 4 / 5 / 6 / 7, include/gossip.h).  Host
 * arithmetic only, C99 and C++17: engine.hip and oracle/gossip_oracle.c both plan through it, so host
 * shards take the engine's kinds.  It only steers which path computes a round, never a result bit:
 * every kind computes the same S_{t+1}.  Built without fused multiply-add on both sides. */
#ifndef GOSSIP_PLAN_H_
#define GOSSIP_PLAN_H_

#include <math.h>
#include <stdint.h>

/* What the planner reads: set at create, by gossip_set_param / gossip_set_faults, and rep_img_ok by
 * the rounds themselves. */
typedef struct plan_cfg {
  uint64_t N, Nl;           /* nodes, nodes per shard (not the own count: every rank must reach the same plan) */
  uint32_t G, k, R, mode;   /* shards, fanout, rumors (<= 64: W == 1), GOSSIP_MODE_PUSH / PULL / PUSHPULL */
  uint32_t edge_loss, partitions; /* lost edges thin the predictor's fanout */
  double sparse_frac;       /* rare fraction at or below which a round runs sparse (plan_sparse_frac) */
  int sparse_frac_set;      /* set by gossip_set_param: the fixed threshold decides, not the cost model */
  double alld_frac;         /* sparse rounds with k * rare >= alld_frac * N commit every group's D */
  double filter_frac;       /* dense rounds filter edges by the peer's class above this empty / full fraction */
  int filter_frac_set;      /* else off past 2^25 nodes (plan_filter_frac) */
  double xd_filter_frac;    /* exchange rounds likewise (their probe hits a G-shard class image) */
  uint32_t xd_shards;       /* G at which dense rounds become exchange rounds (0 = never) */
  double cc_frac;           /* class-coded all-gather with at most this global fraction of mixed nodes */
  int replicate;            /* -1 by the cost model, 0 never, 1 every dense round */
  double link_gbps;         /* per link; 0 = the fixed sparse_frac thresholds */
  double mid_frac;          /* sparse rounds test the mid-level summary once this share of peers hits the LDS one */
  double bscan_frac;        /* ... and take the binned scan at this share */
  /* what the caller can run */
  int sharded;              /* sharded sparse rounds (G > 1, W == 1, a random mode) */
  int can_sparse;           /* sparse rounds at all (a frontier, or sharded) */
  int can_xd, can_rep;      /* exchange rounds; replicated rounds (the one-GPU binned round fits N, k) */
  uint32_t glog;            /* the rare summary: 2^glog nodes per bit */
  int has_mid;              /* ... and whether it has a mid level */
  int rep_img_ok;           /* state: the image holds S_t of every node (the last round was replicated) */
  double fullpull_frac;     /* pulling modes: a full-majority round with at most this share of non-full nodes resolves
                             * them from their own draws (plan_choose_fullpull) */
} plan_cfg;

/* (build knob for sweeps and A/B runs; 0 = never) */
#ifndef GOSSIP_FULLPULL_FRAC
#define GOSSIP_FULLPULL_FRAC 0.3
#endif

static inline void plan_defaults(plan_cfg* c) {
  c->sparse_frac = 1.0 / 16;
  c->alld_frac = 1.0 / 128;  /* (sweep: profiles/r05_ad/) */
  c->filter_frac = 0.3;
  c->xd_filter_frac = 0.6;   /* (G = 8 sweep) */
  c->xd_shards = 6;
  c->cc_frac = 0.75;
  c->replicate = -1;
  c->link_gbps = 76.0;
  c->mid_frac = 0.5;
  c->bscan_frac = 0.6;
  c->fullpull_frac = GOSSIP_FULLPULL_FRAC;
}

/* Totals the path choice needs: full and nonzero counts, per-rumor infected. */
typedef struct plan_est {
  double full, nz, inf[64];
} plan_est;

/* (std::min / std::max: the second argument wins only when strictly smaller / larger, also with NaN) */
static inline double plan_min(double a, double b) { return b < a ? b : a; }
static inline double plan_max(double a, double b) { return a < b ? b : a; }
static inline uint32_t plan_rumors(const plan_cfg* c) { return c->R < 64 ? c->R : 64; }
static inline int plan_pushes(const plan_cfg* c) { return c->mode == 1 || c->mode == 3; } /* PUSH, PUSHPULL */
static inline int plan_pulls(const plan_cfg* c) { return c->mode == 2 || c->mode == 3; }  /* PULL, PUSHPULL */

/* from a totals vector: [0] full nodes, [4 + r] holders of rumor r, [4 + R] nonzero nodes */
static inline plan_est plan_est_of(const plan_cfg* c, const uint64_t* tot) {
  plan_est x;
  x.full = (double)tot[0];
  x.nz = (double)tot[4 + c->R];
  for (uint32_t r = 0; r < plan_rumors(c); ++r) x.inf[r] = (double)tot[4 + r];  /* (the planner runs with W == 1) */
  return x;
}

/* One round of the mean-field model of the random modes, per rumor: a node misses rumor r after the
 * round iff it held no copy, none of its k pulls hit a holder (u^k) and no holder pushed to it
 * (e^{-k(1-u)}).  Lost edges thin the fanout; a partition keeps ~1/P of the peers. */
static inline plan_est plan_predict(const plan_cfg* c, const plan_est* x) {
  plan_est y;
  const double keep = (1.0 - (double)c->edge_loss / 4294967296.0) * (c->partitions > 1 ? 1.0 / c->partitions : 1.0);
  const double N = (double)c->N, k = (double)c->k * keep;
  double all_miss = 1.0, all_hit = 1.0;
  for (uint32_t r = 0; r < plan_rumors(c); ++r) {
    const double u = 1.0 - x->inf[r] / N;
    double v = u;
    if (plan_pulls(c)) v *= pow(u, k);
    if (plan_pushes(c)) v *= exp(-k * (1.0 - u));
    y.inf[r] = (1.0 - v) * N;
    all_miss *= v;
    all_hit *= 1.0 - v;
  }
  y.nz = N * (1.0 - all_miss);
  y.full = N * all_hit;
  return y;
}

/* dense rounds become exchange rounds */
static inline int plan_dense_xd(const plan_cfg* c) { return c->can_xd && c->xd_shards && c->G >= c->xd_shards; }

/* The sparse-round threshold: gossip_set_param's, else the default of the dense round kind: a sharded
 * dense round that all-gathers the state costs more than an exchange round, so sparse rounds pay off
 * up to a larger rare fraction before it: 1/4, against 1/25 before exchange rounds (a round with ~5 %
 * rare nodes is cheaper as a class-filtered exchange round; profiles/r02_xd, r02_xdfilt). */
static inline double plan_sparse_frac(const plan_cfg* c) {
  if (c->sparse_frac_set || !c->sharded) return c->sparse_frac;
  return plan_dense_xd(c) ? 0.04 : 0.25;
}

/* The one-shard dense filter's threshold: gossip_set_param's, else 0.3 while the occupancy bitmaps (N/8
 * bytes each) fit an XCD's 4 MiB L2; past that every probe is a 64-B fetch from the MALL or HBM and the
 * probes cost more than the edges they drop (2^27 nodes: emit 2.3 -> 6.3 ms, serve + apply -1.6 ms;
 * profiles/r03_a/rounds.txt). */
static inline double plan_filter_frac(const plan_cfg* c) {
  if (c->filter_frac_set) return c->filter_frac;
  return c->N <= (1ull << 25) ? c->filter_frac : 2.0;
}

/* dense rounds: probe the peer's class in emit when many edges would move nothing (bit 0: pulls from
 * empty peers early in a run, bit 1: pushes into full peers late) */
static inline uint32_t plan_dense_filter(const plan_cfg* c, const plan_est* x, double frac) {
  const double N = (double)c->N, empty = 1.0 - x->nz / N, full = x->full / N;
  return (plan_pulls(c) && empty > frac ? 1u : 0u) | (plan_pushes(c) && full > frac ? 2u : 0u);
}

/* sparse when the smaller rare class is at most sparse_frac * N; maj = which class is rare; all_d once
 * the rare ends' pushes (~k per rare node) reach alld_frac * N */
static inline int plan_choose_sparse(const plan_cfg* c, const plan_est* x, uint32_t* maj, int* all_d) {
  const double lo = x->nz, hi = (double)c->N - x->full, rare = plan_min(lo, hi);
  *maj = c->can_sparse && hi < lo ? 1u : 0u;
  *all_d = c->can_sparse && rare * (double)c->k >= c->alld_frac * (double)c->N;
  return c->can_sparse && rare <= plan_sparse_frac(c) * (double)c->N;
}

/* One-shard pulling modes (the caller checks what it can run): a full-majority round whose non-full
 * share is at most fullpull_frac takes the pull shortcut (a non-full node with a full
 * pulled peer ends full), whatever plan_choose_sparse says.  A sparse_frac set by gossip_set_param caps
 * the share (0 keeps such rounds dense); set to 1 it sends every full-majority round there. */
static inline int plan_choose_fullpull(const plan_cfg* c, const plan_est* x) {
  const double lo = x->nz, hi = (double)c->N - x->full;
  double frac = c->fullpull_frac;
  if (c->sparse_frac_set) frac = c->sparse_frac >= 1.0 ? 1.0 : plan_min(frac, c->sparse_frac);
  return c->can_sparse && plan_pulls(c) && hi < lo && hi <= frac * (double)c->N;
}

/* the share of peers that hit a summary bit of 2^glog nodes when a share r of the nodes is rare */
static inline double plan_group_hit(double r, uint32_t glog) { return 1.0 - pow(1.0 - r, (double)(1u << glog)); }

/* ... of a one-shard sparse round under maj: the binned scan takes over at bscan_frac */
static inline double plan_bscan_hit(const plan_cfg* c, const plan_est* x, uint32_t maj) {
  const double N = (double)c->N, rare = maj ? N - x->full : x->nz;
  return plan_group_hit(plan_min(plan_max(rare / N, 0.0), 1.0), c->glog);
}

/* Per-rank cost model of one sharded round, in ms: device time from the measured rates
 * plus link time = the bytes the rank sends over its links / (link_gbps x the G - 1 links it uses, at
 * most 7).  Device rates: a sparse round costs 2.3 ps per own node (the Philox floor; round 0 at 2^27
 * on one GPU: 311 us) plus up to 70 ps per own node as the rare share r grows, x (1 - e^(-r / 0.05))
 * (the summaries saturate: G = 2 x 2^26 at r = 3.7 / 19 / 25 %: 2.41 / 5.0 / 4.83 ms,
 * profiles/r05_shard/probe_G2_fixed.txt); a dense round on the state image 7.3 ps per image node + 47 ps
 * per own node (N = 2 / 4 ranks x 2^26 / 2^25: 4.14 / 2.56 ms, profiles/r04_ad/); an exchange round
 * 48.5 ps per own node + 20 ps per item kept by the class filter (fitted on the G = 8 probe: unfiltered
 * 1.15 ms, at 34 % kept 0.93 ms per 2^24-node rank, profiles/r05_probes/: a pull-only edge into an empty
 * peer and a push-only one into a full peer are never sent); a replicated round (kinds 5 / 6 / 7,
 * DESIGN.md §5.7) the one-GPU round over all N nodes (5.1 ms at 2^27: 38 ps per node) plus the own-slice
 * totals, and the state all-gather while the image is not whole.  Link bytes per rank: sparse = the
 * rare-list all-gather (16 B per rare node of the shard to each other shard) + the off-shard pushes (16-B
 * items, ~k per rare node); state all-gather = 8 B per own node to each other shard (class-coded: its
 * bitmaps + prefixes, 20 B per 64 nodes, + 8 B per mixed node); exchange = 40 (G - 1) / G B per own
 * node (12-B items out, 8-B replies back, k = 2). */
typedef struct plan_costs {
  double sparse, dense, rep;                 /* modelled ms per rank: device + link */
  double sparse_link, dense_link, rep_link;  /* their link parts */
  int dense_xd, dense_cc;                    /* the dense round priced: exchange / class-coded / state all-gather */
} plan_costs;

static inline plan_costs plan_round_costs(const plan_cfg* c, const plan_est* x) {
  const double N = (double)c->N, G = (double)c->G, Nl = (double)c->Nl, k = (double)c->k;
  const double rare = plan_min(x->nz, N - x->full), rare_own = rare / G;
  const double bw = c->link_gbps * 1e6 * plan_min(G - 1.0, 7.0);  /* bytes per ms */
  plan_costs p;
  p.sparse_link = (16.0 * rare_own * (G - 1.0) + 16.0 * k * rare_own * (G - 1.0) / G) / bw;
  p.sparse = Nl * (2.3e-9 + 7.0e-8 * (1.0 - exp(-rare / N / 0.05))) + p.sparse_link;
  p.dense_xd = plan_dense_xd(c);
  const double mixed = plan_max(0.0, x->nz - x->full);
  p.dense_cc = !p.dense_xd && c->cc_frac > 0 && mixed / N <= c->cc_frac;
  if (p.dense_xd) {  /* (k <= 8: one keep byte per sender carries the filter's probes) */
    const uint32_t filt = c->k <= 8 ? plan_dense_filter(c, x, c->xd_filter_frac) : 0u;
    const double ef = 1.0 - x->nz / N, ff = x->full / N, mf = plan_max(0.0, 1.0 - ef - ff);
    const double kept = mf + ef * ((filt & 1u) ? 1.0 - ef : 1.0) + ff * ((filt & 2u) ? 1.0 - ff : 1.0);
    p.dense_link = 40.0 * (G - 1.0) / G * Nl * kept / bw;
    p.dense = Nl * (4.85e-8 + 2.0e-8 * kept) + p.dense_link;
  } else {
    const double slice = p.dense_cc ? 20.0 / 64.0 * Nl + 8.0 * mixed / G : 8.0 * Nl;
    p.dense_link = slice * (G - 1.0) / bw;
    p.dense = 7.3e-9 * N + 4.7e-8 * Nl + p.dense_link;
  }
  /* entering replication gathers the image class-coded where the dense round would (kind 7), else whole (5) */
  const double cc_slice = 20.0 / 64.0 * Nl + 8.0 * mixed / G;
  p.rep_link = c->rep_img_ok ? 0.0 : (p.dense_cc ? cc_slice : 8.0 * Nl) * (G - 1.0) / bw;
  p.rep = 3.8e-8 * N + 1.5e-9 * Nl + p.rep_link;
  return p;
}

/* What replicating saves over the dense rounds after this one (kind 6 instead of a sharded dense round
 * each), as far as the predictor sees them: up to 8 rounds, until one that the model would run sparse. */
static inline double plan_rep_gain_ahead(const plan_cfg* c, plan_est x) {
  double gain = 0.0;
  for (int i = 0; i < 8; ++i) {
    x = plan_predict(c, &x);
    const plan_costs p = plan_round_costs(c, &x);
    const double rep6 = p.rep - p.rep_link;
    if (p.sparse < plan_min(p.dense, rep6)) break;  /* the dense phase ends */
    gain += plan_max(0.0, p.dense - rep6);
  }
  return gain;
}

/* One sharded round as planned from the global totals of S_t. */
typedef struct plan_round {
  int kind;                    /* 0 dense, 1 sparse, 3 exchange, 4 class-coded, 5 / 6 / 7 replicated */
  int sparse, rep, xd, cc;     /* the round's parts (cc with rep: kind 7) */
  uint32_t maj, xd_filt;       /* sparse: which class is rare; exchange: the edge filter */
  int all_d, mid;              /* sparse: commit every group's D; test peers in the mid-level summary */
  double sparse_ms, dense_ms;  /* the model's sparse and dense round */
  double ms, link_ms;          /* the round as planned, and its link part */
} plan_round;

static inline plan_round plan_sharded_round(const plan_cfg* c, const uint64_t* tot) {
  plan_round p;
  const plan_est x = plan_est_of(c, tot);
  const double N = (double)c->N;
  p.sparse = plan_choose_sparse(c, &x, &p.maj, &p.all_d);
  /* (link_gbps 0: the model's prices are reported, not used) */
  const plan_costs m = plan_round_costs(c, &x);
  const int model = !c->sparse_frac_set && c->link_gbps > 0;
  /* replicated dense rounds: forced (replicate 1), or by the model: with a whole image (kind 6) while
   * one costs less than the sharded dense round; entering (kind 5 / 7: the all-gather plus the whole
   * round) where what it costs over the sharded round is won back over the dense rounds the predictor
   * sees ahead.  The per-node fits come from 2^24-2^27-node runs: below 2^22 nodes only when forced */
  const double rep6 = m.rep - m.rep_link;
  int rep_auto = c->replicate < 0 && model && c->N >= (1ull << 22) && rep6 < m.dense;
  if (rep_auto && !c->rep_img_ok) rep_auto = m.rep - m.dense < plan_rep_gain_ahead(c, x);
  const int rep_any = c->replicate != 0 && c->can_rep && (c->replicate == 1 || rep_auto);
  if (model) p.sparse = m.sparse < (rep_any ? plan_min(m.dense, m.rep) : m.dense);  /* the cost model decides instead */
  p.rep = !p.sparse && rep_any;
  p.sparse_ms = m.sparse;
  p.dense_ms = m.dense;
  p.mid = c->has_mid && plan_group_hit(plan_min(1.0, plan_min(x.nz, N - x.full) / N), c->glog) >= c->mid_frac;
  p.xd = !p.sparse && !p.rep && m.dense_xd;
  /* exchange rounds drop the one-way edges into empty / full peers when many nodes are (exact totals) */
  p.xd_filt = p.xd && c->k <= 8 ? plan_dense_filter(c, &x, c->xd_filter_frac) : 0u;
  /* dense on the state image: class-coded when few nodes are mixed (neither empty nor full); kind 7
   * enters replication over that all-gather: the image expanded whole, then the replicated round */
  const double mixed = (x.nz - x.full) / N;
  const int rep_cc = p.rep && !c->rep_img_ok && m.dense_cc;
  p.cc = (!p.sparse && !p.xd && !p.rep && c->cc_frac > 0 && mixed <= c->cc_frac) || rep_cc;
  p.kind = p.sparse ? 1 : p.rep ? (c->rep_img_ok ? 6 : rep_cc ? 7 : 5) : p.xd ? 3 : p.cc ? 4 : 0;
  p.ms = p.sparse ? m.sparse : p.rep ? m.rep : m.dense;
  p.link_ms = p.sparse ? m.sparse_link : p.rep ? m.rep_link : m.dense_link;
  return p;
}

#endif  /* GOSSIP_PLAN_H_ */
