// engine_internal.h — private to libmaelsim: engine.hip and the simulation kernels' units (through sim_kernels.h / wave_common.h),
// the checkers — checker.hip, the device checkers and the host checkers lin_check.cpp, txn_check.cpp, kafka_check.cpp, pn_check.cpp — (through
// check_run.h), gather.cpp, guard.cpp.
#ifndef MSIM_ENGINE_INTERNAL_H
#define MSIM_ENGINE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <string>

#include "../../include/maelsim.h"
#include "engine_limits.h"

typedef uint32_t u32;
typedef uint64_t u64;

struct msim_ctx {
  msim_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;   // gather.cpp's own timing events
  hipEvent_t ev_null = nullptr;                  // run_impl: what the null stream holds when a launch is queued (the launch waits for it on the device)
  // device buffers of the last run
  uint32_t n_inst = 0, cap_inst = 0;
  uint64_t first_instance = 0;
  msim_op *d_rows = nullptr;
  uint32_t *d_payload = nullptr;
  msim_net_stats *d_stats = nullptr;
  msim_inst_meta *d_meta = nullptr;
  uint32_t *d_scratch = nullptr;
  uint64_t scratch_words_per_inst = 0;
  msim_check_result *d_check = nullptr;
  msim_event *d_journal = nullptr;
  // duo.hip's flood table: made once, before the context's first launch (engine.hip ensure_flood_table), a constant of the configuration
  // from then on: it outlives the slabs above, MSIM_POISON does not fill it, msim_destroy frees it.  Null where no launch reads one.
  uint32_t *d_duo_table = nullptr; bool duo_table_tried = false;
  // host (pinned) mirrors
  msim_op *h_rows = nullptr;
  uint32_t *h_payload = nullptr;
  msim_net_stats *h_stats = nullptr;
  msim_inst_meta *h_meta = nullptr;
  msim_check_result *h_check = nullptr;
  msim_event *h_journal = nullptr;
  uint64_t *h_row_off = nullptr, *h_pay_off = nullptr, *h_ev_off = nullptr;  // compacted offsets per instance
  // fetch path: device-side compaction buffers + grow-only capacities (bytes) of the pinned mirrors
  void *d_check_scratch = nullptr; size_t cap_check_scratch = 0;  // checker.hip: read records per instance
  void *d_perf_scratch = nullptr; size_t cap_perf_scratch = 0;    // perf_check_dev.hip: latency records per instance, the results behind them
  void *d_compact = nullptr; uint64_t *d_off = nullptr;
  void *d_compact2 = nullptr; uint64_t *d_off2 = nullptr; size_t cap_compact2 = 0, cap_off2 = 0;   // the payload's own pair (both compactions are queued before the first copy)
  bool fetch_pending = false;      // msim_fetch_begin has queued the copies; msim_fetch waits for them
  size_t cap_compact = 0, cap_off = 0, cap_h_rows = 0, cap_h_payload = 0, cap_h_journal = 0, cap_h_meta = 0;
  // multi-GPU gather (gather.cpp): RCCL communicator of this rank, the rank's compacted slabs, the root's receive buffers
  void *comm = nullptr; int comm_rank = 0, comm_world = 1;
  void *d_grows = nullptr, *d_gpay = nullptr; uint64_t *d_goff = nullptr; size_t cap_grows = 0, cap_gpay = 0, cap_goff = 0;
  uint64_t g_row_units = 0, g_pay_words = 0;   // compacted sizes of the last msim_compact_on_device
  void *d_all[4] = {nullptr, nullptr, nullptr, nullptr}; size_t cap_all[4] = {0, 0, 0, 0};   // rows, payload, meta, stats of every rank (root)
  uint64_t *d_sizes = nullptr;   // world x 4 u64 for the size all-gather
  bool fetched = false, checked = false, check_fetched = false, ran = false;
  // the set-full / echo check queued behind its simulation at launch time (engine.hip run_impl, msim_check): `ran_own_stream` the last
  // launch is on the context's own stream; `check_armed` the caller checked such a launch, so the next one queues its check straight
  // behind the simulation kernel; `check_queued` that check is in the queue and msim_check has not taken it yet
  bool ran_own_stream = false, check_armed = false, check_queued = false;
  float sim_ms = 0.f, check_ms = 0.f;
  bool sim_ms_stale = false;        // the last launch was msim_run_async: sim_ms is read from ev0 / ev1 on demand
  uint32_t dev_flags = 0;           // msim_set_dev_flags: ORed with the MSIM_DEV_FLAGS of the environment (developer switches)
  uint32_t txn_big = 0;             // txn_check_dev.hip: histories of the last check whose tables did not fit LDS (HBM-table kernel)
  uint32_t lin_host_rechecks = 0;   // lin_check_dev.hip: histories of the last check the host search had to finish
  bool check_classify = false;      // msim_set_check_classify: txn-rw-register records name the allowed cycle classes too; txn-list-append's and kafka's unclean histories are analysed on the device
  std::string err;
};

// Host threads one engine context may use for its host-side checkers: the hardware threads divided by the ranks sharing
// the node (LOCAL_WORLD_SIZE, set by torch.distributed.run), or MSIM_HOST_THREADS if set.
#include <cstdio>
#include <cstdlib>
#include <thread>
static inline unsigned msim_host_threads() {
  if (const char *e = std::getenv("MSIM_HOST_THREADS")) { const int v = std::atoi(e); if (v > 0) return (unsigned)v; }
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  // a container's CPU quota (cgroup v2 cpu.max = "<quota> <period>"): more runnable threads than granted CPUs only get throttled
  if (std::FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    long long q = 0, per = 0;
    if (std::fscanf(f, "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) { const unsigned lim = (unsigned)((q + per - 1) / per); if (lim >= 1 && lim < nt) nt = lim; }
    std::fclose(f);
  }
  if (const char *e = std::getenv("LOCAL_WORLD_SIZE")) { const int v = std::atoi(e); if (v > 1) nt = nt / (unsigned)v ? nt / (unsigned)v : 1; }
  return nt;
}

// The developer switches in force for a context: those set through msim_set_dev_flags ORed with MSIM_DEV_FLAGS of the environment
// (read once per process).  0x100 round limit x20, 0x200 one cluster per wavefront, 0x400 fail instead of falling back to it,
// 0x800 checkers on the host cores, 0x1000 time the checkers' passes (and count their launches) on stderr and name the kernel each launch
// took (`[layout] <kernel> <n>`) and the flood table a context makes (`[duo] flood table: <k> of <n> origins`, duo.hip), 0x2000 the checkers' HBM-table kernels / the lin-kv search's tiny pools, 0x10000 at most 7 histories per
// launch in the chunked checker loops (txn LDS and HBM-table passes, rw, unique-ids HBM tables: a partial last chunk, first > 0).  The
// rw-register classification (rw_check_dev.hip): 0x2000 a matrix of 16 transactions per cyclic component and larger ones to the host,
// 0x20000 a matrix of 16 with the search in the workspace behind it, as every component beyond 256 has it.  0x40000 the set-full / echo
// check is launched where msim_check is called, never queued behind its simulation (a context under it never arms).  Under 0x1000 the
// route of every such check is named too: `[check] queued <n>` (run_impl), `[check] taken <n>` / `[check] launched <n>` (msim_check).
static inline uint32_t msim_dev_flags(const msim_ctx *ctx) {
  static const uint32_t env = []() { const char *e = std::getenv("MSIM_DEV_FLAGS"); return e ? (uint32_t)std::strtoul(e, nullptr, 0) : 0u; }();   // (decimal, 0x.. or 0..)
  return env | (ctx ? ctx->dev_flags : 0u);
}

// MSIM_POISON=<byte> (developer check for reads of memory no kernel of a launch wrote, read once per process): the byte, or -1
static inline int msim_poison_byte() {
  static const int poison = []() { const char *p = std::getenv("MSIM_POISON"); return p ? (int)(std::strtoul(p, nullptr, 0) & 0xFFu) : -1; }();
  return poison;
}

// engine.hip: compacts the used prefix of every instance's row / payload slab into ctx->d_grows / ctx->d_gpay on the device
// (instance order); *row_units = 16-byte rows, *pay_words = u32 words.  Synchronises ctx->stream.
int msim_compact_on_device(msim_ctx *ctx, uint64_t *row_units, uint64_t *pay_words);
// gather.cpp
void msim_gather_free(msim_ctx *ctx);
// checker.hip: the set-full / echo checker over the context's slabs.  msim_check_reserve sizes d_check_scratch for n histories (it may
// free and allocate: never between a simulation and the check queued behind it); msim_check_enqueue queues the kernel between ev2 and
// ev3 on `stream` and never waits; msim_check_wait waits for ev3 and marks the run checked; msim_check_launch = enqueue on the context's
// stream + wait; msim_check_take_or_arm: 1 a queued check taken and waited for, 0 none queued (the context armed where it may be), < 0 an error
int msim_check_reserve(msim_ctx *ctx, uint32_t n);
int msim_check_enqueue(msim_ctx *ctx, hipStream_t stream);
int msim_check_wait(msim_ctx *ctx);
int msim_check_take_or_arm(msim_ctx *ctx);
int msim_check_launch(msim_ctx *ctx);
// lin_check.cpp (host search) / lin_check_dev.hip (one wavefront per history)
// (keys / max_keys / n_keys: msim_explain_lin_kv's key records, a slab of max_keys per history; null / 0 / null: the plain check)
int msim_check_lin_kv_host(msim_ctx *ctx, msim_lin_key_result *keys = nullptr, uint32_t max_keys = 0, uint32_t *n_keys = nullptr);
int msim_check_lin_kv_device(msim_ctx *ctx, msim_lin_key_result *keys = nullptr, uint32_t max_keys = 0, uint32_t *n_keys = nullptr);
// txn_check.cpp (host analysis) / txn_check_dev.hip (device: proves a list-append history clean, else hands it to the host)
int msim_check_txn_host(msim_ctx *ctx);
// (cycles / steps / max_steps: msim_explain_txn's witness cycles, a slab of max_steps per history; null / null / 0: the plain check)
int msim_check_txn_device(msim_ctx *ctx, msim_cycle_result *cycles = nullptr, msim_cycle_step *steps = nullptr, uint32_t max_steps = 0);
// rw_check_dev.hip (device: proves a rw-register history free of what the consistency model proscribes, else hands it to the host)
int msim_check_rw_device(msim_ctx *ctx, msim_cycle_result *cycles = nullptr, msim_cycle_step *steps = nullptr, uint32_t max_steps = 0);
// kafka_check.cpp (host)
int msim_check_kafka_host(msim_ctx *ctx);
int msim_explain_kafka_host(msim_ctx *ctx, msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings);   // (hdr null: msim_check_kafka_host)
// kafka_check_dev.hip (device pass + host checker for what it cannot prove clean)
int msim_check_kafka_device(msim_ctx *ctx);
// unique_check_dev.hip, pn_check_dev.hip
int msim_check_unique_device(msim_ctx *ctx);
int msim_check_pn_device(msim_ctx *ctx);
// txn_check.cpp
// pn_check.cpp
int msim_check_pn_host(msim_ctx *ctx);
int msim_check_unique_host(msim_ctx *ctx);
int msim_explain_pn_host(msim_ctx *ctx, msim_pn_explain *hdr, void *records, uint32_t max_records);
int msim_explain_unique_host(msim_ctx *ctx, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups);

// guard.cpp: the library's device allocator — hipMalloc / hipFree unless MSIM_GUARD asks for fenced slabs (developer's electric fence for HBM)
hipError_t msim_dev_malloc_impl(void **out, size_t bytes);
hipError_t msim_dev_free(void *ptr);
template <typename T> static inline hipError_t msim_dev_malloc(T **out, size_t bytes) { return msim_dev_malloc_impl(reinterpret_cast<void **>(out), bytes); }

#define MSIM_HIP_TRY(ctx, call)                                                        \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                 \
      return MSIM_E_HIP;                                                               \
    }                                                                                  \
  } while (0)

#endif
