// launch_plan_dump.cpp — what csrc/launch_plan.h plans for a grid of configurations, one line per grid point, as a stand-alone host
// program over the wavefront emulator's build (tools/launch_plan_dump.py compiles this file and engine.hip with
// -fsanitize=address,undefined and runs it; no device, no launch, no Python in the process).  tests/test_launch_plan.py compares the
// lines with the recorded ones (tests/golden/launch_plan.txt.xz).  Per accepted point: the configuration, then every number of the
// LaunchPlan, the one-cluster kernel, and per packed row `name:eligible:min_clusters`.  Exits 1 when the grid misses a node program, a
// packed row (as eligible) or a one-cluster kernel, or when two packed rows other than duo / bcast8 are eligible for one configuration.
#include <cstdio>
#include <set>
#include <string>

#include "../maelstrom_amd/csrc/launch_plan.h"

namespace {

uint32_t workload_of(uint32_t program) {
  switch (program) {
    case MSIM_NODE_ECHO: return MSIM_WL_ECHO;
    case MSIM_NODE_G_SET: return MSIM_WL_G_SET;
    case MSIM_NODE_RAFT: case MSIM_NODE_LIN_KV_PROXY: return MSIM_WL_LIN_KV;
    case MSIM_NODE_TXN_SINGLE_KEY: case MSIM_NODE_TXN_MULTI_KEY: case MSIM_NODE_TXN_DATOMIC: return MSIM_WL_TXN_LIST_APPEND;
    case MSIM_NODE_PN_COUNTER: return MSIM_WL_PN_COUNTER;
    case MSIM_NODE_FLAKE_IDS: case MSIM_NODE_TSO_IDS: return MSIM_WL_UNIQUE_IDS;
    case MSIM_NODE_TXN_RW_HAT: return MSIM_WL_TXN_RW_REGISTER;
    case MSIM_NODE_KAFKA: return MSIM_WL_KAFKA;
    default: return MSIM_WL_BROADCAST;
  }
}

}  // namespace

int main() {
  const uint32_t nodes[] = {1, 2, 3, 5, 7, 8, 16, 25, 32, 33, 64, 100, 127}, flag_set[] = {0, 0x200, 0x4000, 0x8000};
  std::set<uint32_t> programs;
  std::set<std::string> rows, kernels;
  unsigned long points = 0, clashes = 0;
  for (uint32_t program = 0; program < MSIM_N_NODE_PROGRAMS; program++)
    for (uint32_t workers = 1; workers <= 3; workers++)
      for (uint32_t n : nodes)
        for (uint32_t bits = 0; bits < 32; bits++)
          for (uint32_t flags : flag_set) {
            const bool nemesis = bits & 1, journal = bits & 2, exponential = bits & 4, loss = bits & 8, small_inbox = bits & 16;
            msim_config c;
            msim_config_defaults(&c, workload_of(program), n);
            c.node_program = program; c.concurrency = workers * n;
            if (nemesis) c.nemesis_mask = MSIM_NEMESIS_PARTITION;
            if (journal) c.journal_capacity = 8192;
            if (exponential) { c.latency_dist = MSIM_LAT_EXPONENTIAL; c.latency_mean_ms = 10; }
            if (loss) c.p_loss_q32 = (uint32_t)(0.05 * 4294967296.0);
            if (small_inbox) c.inbox_capacity = 2;
            char err[256];
            if (msim_config_finalize(&c, err, sizeof err) != MSIM_OK) continue;
            points++; programs.insert(program);
            const LaunchPlan p = msim_plan_launch(c, flags);
            const KParams &k = p.kp;
            std::printf("prog=%u c=%u n=%u nem=%d jrn=%d exp=%d loss=%d inbox=%u flags=0x%x | rc=%d", program, c.concurrency, n, nemesis, journal, exponential, loss, c.inbox_capacity, flags, p.rc);
            if (p.rc != MSIM_OK) std::printf(" \"%s\" scratch=%llu", p.err, (unsigned long long)k.scratch_words);
            else std::printf(" scratch=%llu spill_off=%llu off=%u,%u,%u lds=%zu tcap=%u ccap=%u raft_log=%u gen=%u nem=%u", (unsigned long long)k.scratch_words,
                             (unsigned long long)k.spill_off, k.off_inbox, k.off_seen, k.off_misc, p.lds, k.mk_tcap, k.mk_ccap, k.raft_log_cap, k.gen_period2_us, k.nem_period2_us);
            const char *one = p.program ? msim_one_cluster_launcher(*p.program, c).name : "?";   // (no row: a program msim_config_finalize should have refused)
            if (p.program) kernels.insert(one);
            std::printf(" | %s |", one);
            unsigned eligible = 0;
            for (const PackedLayout &l : MSIM_PACKED_LAYOUTS) {
              const bool e = l.eligible(c);
              std::printf(" %s:%d:%u", l.name, e, l.min_clusters(c));
              if (e) { rows.insert(l.name); eligible += &l != &MSIM_DUO || !MSIM_BCAST8.eligible(c); }   // (duo beside bcast8 counts once)
            }
            std::printf("\n");
            if (eligible > 1) { clashes++; std::fprintf(stderr, "launch_plan_dump: %u packed rows eligible at prog=%u c=%u n=%u bits=%u\n", eligible, program, c.concurrency, n, bits); }
          }
  int bad = clashes != 0;
  if (programs.size() != MSIM_N_NODE_PROGRAMS) { bad = 1; std::fprintf(stderr, "launch_plan_dump: %zu of %u node programs in the grid\n", programs.size(), MSIM_N_NODE_PROGRAMS); }
  for (const PackedLayout &l : MSIM_PACKED_LAYOUTS) if (!rows.count(l.name)) { bad = 1; std::fprintf(stderr, "launch_plan_dump: packed row %s never eligible\n", l.name); }
  for (const NodeProgram &np : MSIM_NODE_PROGRAMS)
    for (const Launcher1 *l : {&np.one, &np.many, &np.wide}) if (l->fn && !kernels.count(l->name)) { bad = 1; std::fprintf(stderr, "launch_plan_dump: one-cluster kernel %s never taken\n", l->name); }
  std::fprintf(stderr, "launch_plan_dump: %lu points, %zu node programs, %zu packed rows, %zu one-cluster kernels, %lu clashes\n", points, programs.size(), rows.size(), kernels.size(), clashes);
  return bad;
}
