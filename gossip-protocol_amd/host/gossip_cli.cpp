// gossip_cli — native host driver of libgossip_hip.so through the C ABI only
// (include/gossip.h), the way a compiled front-end (the reference is Go, bound
// with cgo: INTEGRATION.md) drives the engine.  Runs full disseminations and
// prints one JSON line per run.
//
//   gossip_cli [--nodes N] [--rumors R] [--mode push|pull|pushpull|flood-grid|MODE-grid]
//              [--fanout K] [--seed S] [--runs M] [--hash]
//              [--topo-peers]   with push-grid, pull-grid or pushpull-grid: random gossip over
//                               the grid, K of a node's grid neighbours per round
//                               (GOSSIP_FLAG_TOPO_PEERS); prints the messages sent
//              [--monger P [--blind]]   with push, or push-grid --topo-peers: rumor mongering
//                               (GOSSIP_FLAG_MONGER), a counted contact cools the sender with
//                               probability P (--blind: every attempt counts, else feedback); runs
//                               to quiescence and prints the residue and the messages per node.
//                               With pull, or pull-grid --topo-peers: pull rumor mongering
//                               (GOSSIP_FLAG_MONGER_PULL), the node that answered cools with
//                               probability P once per round in which a pull did not need the rumor
//                               and none did (--blind: every pull that arrives counts); runs until
//                               no node is hot; the messages are the replies that carried a rumor.
//                               With pushpull, or pushpull-grid --topo-peers: push-pull rumor mongering
//                               (GOSSIP_FLAG_MONGER_PUSHPULL), both ends of an exchange send their hot
//                               rumors and both cool as the answering node of pull does; runs until no
//                               node is hot; the messages are the exchanges with a hot end
//              [--monger-limit M]   with --monger: the counter rule (gossip_set_monger_limit), a
//                               rumor cools once M (1..15) counted contacts have passed the coin;
//                               the paper's pure counter is --monger 1 --monger-limit M
//              [--conn-limit C [--hunt H]]   with --monger: a node accepts at most C (1..8) incoming
//                               connections per round, and the initiator of a refused edge tries up
//                               to H (0..15) further peers (gossip_set_monger_connections); the line
//                               then carries both values and the last round's attempts, accepted and
//                               refused edges and hunts
//              [--shards G [--devices d0,d1,...]]   G shards in this process, every round
//                                                   driven by the library (gossip_group_*:
//                                                   RCCL over distinct devices, else copies)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gossip.h"

static int die(gossip_engine_t* e, const char* what, int rc) {
  std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, gossip_last_error(e));
  return 1;
}

static int die_group(gossip_group_t* g, const char* what, int rc) {
  std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, gossip_group_last_error(g));
  return 1;
}

int main(int argc, char** argv) {
  uint64_t nodes = 1ull << 20, seed = 0x5EED0001;
  uint32_t rumors = 1, fanout = 3, runs = 3, shards = 1;
  std::vector<int32_t> devices;
  std::string mode = "push";
  bool hash = false, topo_peers = false, blind = false;
  double monger = -1.0;  // < 0: off
  uint32_t monger_limit = 1;
  bool limit_given = false;
  uint32_t conn_limit = 0, hunt = 0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() { return i + 1 < argc ? argv[++i] : (char*)"0"; };
    if (a == "--nodes") nodes = std::strtoull(next(), nullptr, 0);
    else if (a == "--rumors") rumors = (uint32_t)std::strtoul(next(), nullptr, 0);
    else if (a == "--mode") mode = next();
    else if (a == "--fanout") fanout = (uint32_t)std::strtoul(next(), nullptr, 0);
    else if (a == "--seed") seed = std::strtoull(next(), nullptr, 0);
    else if (a == "--runs") runs = (uint32_t)std::strtoul(next(), nullptr, 0);
    else if (a == "--hash") hash = true;
    else if (a == "--topo-peers") topo_peers = true;
    else if (a == "--monger") monger = std::strtod(next(), nullptr);
    else if (a == "--blind") blind = true;
    else if (a == "--monger-limit") {
      monger_limit = (uint32_t)std::strtoul(next(), nullptr, 0);
      limit_given = true;
    }
    else if (a == "--conn-limit") conn_limit = (uint32_t)std::strtoul(next(), nullptr, 0);
    else if (a == "--hunt") hunt = (uint32_t)std::strtoul(next(), nullptr, 0);
    else if (a == "--shards") shards = (uint32_t)std::strtoul(next(), nullptr, 0);
    else if (a == "--devices") {
      for (char* p = next(); *p;) {
        devices.push_back((int32_t)std::strtol(p, &p, 0));
        if (*p == ',') ++p;
      }
    }
    else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }
  gossip_config_t cfg;
  std::memset(&cfg, 0, sizeof cfg);
  cfg.n_nodes = nodes;
  cfg.n_rumors = rumors;
  cfg.fanout = fanout;
  cfg.seed = seed;
  cfg.device = -1;
  cfg.shard_count = 1;
  const size_t dash = mode.rfind("-grid");
  const bool grid = dash != std::string::npos && dash + 5 == mode.size();
  const std::string base = grid ? mode.substr(0, dash) : mode;
  if (base != "push" && base != "pull" && base != "pushpull" && !(grid && base == "flood")) {
    std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
  }
  if (topo_peers != (grid && base != "flood")) {
    std::fprintf(stderr, "--topo-peers goes with push-grid, pull-grid or pushpull-grid (and they with it)\n");
    return 2;
  }
  const bool monger_pull = monger >= 0 && base == "pull", monger_pp = monger >= 0 && base == "pushpull";
  const bool by_hot = monger_pull || monger_pp;  // quiescence is judged by the hot nodes
  cfg.flags = (hash ? GOSSIP_FLAG_HASH : 0) | (topo_peers ? GOSSIP_FLAG_TOPO_PEERS : 0) |
              (monger < 0 ? 0 : monger_pp ? GOSSIP_FLAG_MONGER_PUSHPULL : monger_pull ? GOSSIP_FLAG_MONGER_PULL : GOSSIP_FLAG_MONGER);
  if ((monger >= 0 && (base == "flood" || shards > 1 || monger > 1.0)) || (blind && monger < 0)) {
    std::fprintf(stderr, "--monger P (0 <= P <= 1) goes with --mode push, pull or pushpull, or push-grid, pull-grid or "
                         "pushpull-grid --topo-peers, on one shard, --blind with --monger\n");
    return 2;
  }
  if (limit_given && (monger < 0 || monger_limit < 1 || monger_limit > 15)) {
    std::fprintf(stderr, "--monger-limit M (1 <= M <= 15) goes with --monger\n");
    return 2;
  }
  if ((conn_limit || hunt) && (monger < 0 || conn_limit < 1 || conn_limit > 8 || hunt > 15)) {
    std::fprintf(stderr, "--conn-limit C (1 <= C <= 8) goes with --monger, --hunt H (0 <= H <= 15) with --conn-limit\n");
    return 2;
  }
  cfg.mode = base == "push" ? GOSSIP_MODE_PUSH : base == "pull" ? GOSSIP_MODE_PULL
           : base == "pushpull" ? GOSSIP_MODE_PUSHPULL : GOSSIP_MODE_FLOOD;
  if (shards > 1) {  // the library runs every sharded round
    if (grid) {
      std::fprintf(stderr, "--shards: random modes over all nodes only\n");
      return 2;
    }
    if (!devices.empty() && devices.size() != shards) {
      std::fprintf(stderr, "--devices wants %u ordinals\n", shards);
      return 2;
    }
    gossip_group_t* g = nullptr;
    if (int rc = gossip_group_create(&cfg, shards, devices.empty() ? nullptr : devices.data(), 0, &g))
      return die_group(nullptr, "gossip_group_create", rc);
    std::vector<gossip_round_stats_t> st(4096);
    for (uint32_t run = 0; run < runs; ++run) {
      for (uint32_t r = 0; r < shards; ++r) {
        gossip_engine_t* e = gossip_group_engine(g, r);
        if (int rc = gossip_reset(e)) return die(e, "gossip_reset", rc);
        if (int rc = gossip_inject_random(e)) return die(e, "gossip_inject_random", rc);
      }
      uint32_t done = 0;
      const auto t0 = std::chrono::steady_clock::now();
      if (int rc = gossip_group_step(g, (uint32_t)st.size(), st.data(), nullptr, &done))
        return die_group(g, "gossip_group_step", rc);
      const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      const gossip_round_stats_t& last = st[done ? done - 1 : 0];
      std::printf("{\"run\":%u,\"mode\":\"%s\",\"nodes\":%llu,\"rumors\":%u,\"shards\":%u,\"transport\":%d,"
                  "\"rounds\":%u,\"converged\":%u,\"node_updates_per_s\":%.4e,\"seconds\":%.6f,"
                  "\"state_hash\":\"0x%016llx\"}\n",
                  run, mode.c_str(), (unsigned long long)nodes, rumors, shards, gossip_group_transport(g), done,
                  last.converged, (double)nodes * done / s, s, (unsigned long long)last.state_hash);
    }
    gossip_group_destroy(g);
    return 0;
  }
  gossip_engine_t* e = nullptr;
  if (int rc = gossip_create(&cfg, &e)) return die(nullptr, "gossip_create", rc);
  if (grid) {  // Maelstrom-style grid topology (main.go:132-149 receives it)
    const uint64_t w = (uint64_t)std::ceil(std::sqrt((double)nodes));
    std::vector<uint32_t> row{0}, col;
    for (uint64_t i = 0; i < nodes; ++i) {
      const uint64_t r = i / w, c = i % w;
      if (r > 0) col.push_back((uint32_t)(i - w));
      if (i + w < nodes) col.push_back((uint32_t)(i + w));
      if (c > 0) col.push_back((uint32_t)(i - 1));
      if (c + 1 < w && i + 1 < nodes) col.push_back((uint32_t)(i + 1));
      row.push_back((uint32_t)col.size());
    }
    if (int rc = gossip_set_topology_csr(e, row.data(), col.data(), nodes, col.size()))
      return die(e, "gossip_set_topology_csr", rc);
  }
  std::vector<gossip_round_stats_t> st(4096);
  std::vector<uint64_t> infected;  // --monger: the per-rumor counts of every round, for the residue
  if (monger >= 0) {
    const double x = std::floor(monger * 4294967296.0 + 0.5);
    if (int rc = gossip_set_monger(e, x >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)x, blind ? 1u : 0u))
      return die(e, "gossip_set_monger", rc);
    if (limit_given)
      if (int rc = gossip_set_monger_limit(e, monger_limit)) return die(e, "gossip_set_monger_limit", rc);
    if (conn_limit)
      if (int rc = gossip_set_monger_connections(e, conn_limit, hunt)) return die(e, "gossip_set_monger_connections", rc);
    infected.resize(st.size() * rumors);
  }
  for (uint32_t run = 0; run < runs; ++run) {
    if (int rc = gossip_reset(e)) return die(e, "gossip_reset", rc);
    if (grid || cfg.mode == GOSSIP_MODE_PUSH || rumors == 1) {
      for (uint32_t r = 0; r < rumors; ++r)
        if (int rc = gossip_inject(e, (uint64_t)r % nodes, r)) return die(e, "gossip_inject", rc);
    } else if (int rc = gossip_inject_random(e)) {
      return die(e, "gossip_inject_random", rc);
    }
    uint32_t done = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = gossip_step(e, (uint32_t)st.size(), st.data(), infected.empty() ? nullptr : infected.data(), &done))
      return die(e, "gossip_step", rc);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const gossip_round_stats_t& last = st[done ? done - 1 : 0];
    uint64_t messages = 0;  // FLOOD and --topo-peers count them (0 for random gossip over all nodes)
    for (uint32_t r = 0; r < done; ++r) messages += st[r].messages;
    if (monger >= 0) {  // rounds to quiescence, who never heard each rumor, what it cost
      uint64_t worst = 0, sum = 0, hot = 0;
      if (by_hot)  // quiescent: no node is hot (a round may send nothing while rumors are hot)
        if (int rc = gossip_monger_hot_nodes(e, &hot)) return die(e, "gossip_monger_hot_nodes", rc);
      for (uint32_t r = 0; done && r < rumors; ++r) {
        const uint64_t miss = nodes - infected[(size_t)(done - 1) * rumors + r];
        worst = miss > worst ? miss : worst;
        sum += miss;
      }
      char conn[192] = "";  // --conn-limit: what the last round did under the limit
      if (conn_limit) {
        uint64_t cn[4];
        if (int rc = gossip_monger_connections(e, cn)) return die(e, "gossip_monger_connections", rc);
        std::snprintf(conn, sizeof conn, ",\"conn_limit\":%u,\"hunt\":%u,\"last_attempts\":%llu,\"last_accepted\":%llu,"
                      "\"last_refused\":%llu,\"last_hunts\":%llu",
                      conn_limit, hunt, (unsigned long long)cn[0], (unsigned long long)cn[1], (unsigned long long)cn[2],
                      (unsigned long long)cn[3]);
      }
      std::printf("{\"run\":%u,\"mode\":\"%s\",\"monger\":%.6f,\"blind\":%u,\"monger_limit\":%u,\"nodes\":%llu,"
                  "\"rumors\":%u,"
                  "\"rounds\":%u,\"quiescent\":%u,\"converged\":%u,\"residue_max\":%llu,\"residue_mean\":%.3f,"
                  "\"messages\":%llu,\"messages_per_node\":%.4f,\"seconds\":%.6f,\"state_hash\":\"0x%016llx\"%s}\n",
                  run, mode.c_str(), monger, blind ? 1u : 0u, monger_limit, (unsigned long long)nodes, rumors, done,
                  done && (by_hot ? hot == 0 : last.messages == 0) ? 1u : 0u, last.converged, (unsigned long long)worst,
                  (double)sum / rumors, (unsigned long long)messages, (double)messages / (double)nodes, s,
                  (unsigned long long)last.state_hash, conn);
      continue;
    }
    std::printf("{\"run\":%u,\"mode\":\"%s\",\"nodes\":%llu,\"rumors\":%u,\"rounds\":%u,\"converged\":%u,"
                "\"messages\":%llu,\"node_updates_per_s\":%.4e,\"seconds\":%.6f,\"state_hash\":\"0x%016llx\"}\n",
                run, mode.c_str(), (unsigned long long)nodes, rumors, done, last.converged,
                (unsigned long long)messages, (double)nodes * done / s, s, (unsigned long long)last.state_hash);
  }
  gossip_destroy(e);
  return 0;
}
