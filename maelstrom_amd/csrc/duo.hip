// duo.hip — TWO clusters per wavefront: the headline layout of the simulation kernel.
//
// Same hot path as sim_kernel_colo<> (engine.hip): net.clj:189-247 (send!/recv!, per-destination queues ordered by
// (deadline, id), head-of-line blocking), process.clj:136-166 (one input per node per round), client.clj:41-172 (sync RPC
// clients), core.clj:67-80 (generator phases) and the fire-and-forget broadcast node (doc/03-broadcast/01-broadcast.md:
// 525-547, 02-performance.md:61-67 and :22-28) — round for round what DESIGN.md §2 and the CPU oracle specify.
//
// Why a second layout.  A 25-node cluster fills 25 of a wavefront's 64 lanes, and everything that is uniform per cluster
// (time, phase, generator, cursors) was scalar work paid once per cluster and round: the colocated kernel ran at the
// CU's scalar issue limit.  Here lanes 0-31 simulate one cluster and lanes 32-63 another, and what is
// uniform per CLUSTER lives in VGPRs (every lane of a half holds the same value): one instruction stream, vector
// instructions, serves both clusters; a "ballot" is the cluster's 32-bit half of the wave ballot.  Nothing crosses
// between the halves: the two clusters share the program counter and nothing else.
//
// Scope (the host picks this kernel when all of it holds, else the kernels of engine.hip run):
//   * node program broadcast fire-and-forget (with or without skip-sender), colocated clients (concurrency == n_nodes <= 32);
//   * constant, uniform or exponential latency (bounded below the RPC timeouts), no loss, no nemesis, net journal off.
// With constant latency message ids are unobservable (no per-message RNG draw, no journal, arrival order = id order) and a
// node's queue is a FIFO.  With random latency (RND) every message's latency is drawn from its id (net.clj:178-187), so ids are
// assigned in the canonical order (a prefix sum over the senders of a round) and a node's queue is a bag ordered by
// (deadline, arrival sequence) — the arrival sequence at one node orders its envelopes exactly as their ids do.  No client can
// time out (an RPC completes within one maximal latency of virtual time), a client's reply is handled by the lane that
// sent the request, and a round is:
//   R0  per-cluster time: stay at T while something is due, else jump to the next delivery / scheduler event;
//   R1  generator (one op) / phase actions                          — GENERAL rounds only
//   R2  marked clients invoke: the request reaches its own node     — GENERAL rounds only
//   R3  every node with a due envelope handles it (dedup, fan-out);
//       COMMIT: receivers PULL the senders' fan-outs with ds_bpermute (one per topology neighbour), append to their
//       own LDS ring; idle receivers poll (pop the ring head / the pending client request);
//       the nodes' seen sets live in HBM scratch, one region per cluster (the LDS holds the queues alone);
//   R4  completions -> history rows (staged in LDS, 1 KiB coalesced appends)   — GENERAL rounds only
// A wave-round is GENERAL if either cluster needs it; pure gossip rounds of both clusters take the short body.  At latency 0 a GENERAL
// round whose every acting cluster is quiescent and only runs its generator's op (nearly all of them) is an OP ROUND instead: the
// gossip body plus the op's pick, broadcast or read and two history rows, without R1-R4's general machinery.
// Between two such ops every envelope in flight in the cluster carries the op's value, and the latency-0 DEG4 instantiation keeps
// the cluster in FLOOD MODE: a node's queue is a count, its set word stays in a register.  A wave-round is then one of
//   flood gossip round   every live cluster in flood mode, none wants a GENERAL round: R0, dedup from the register, the pulls, a count
//   flood op round       the same plus the op of each acting cluster, which (re-)enters flood mode with the op's value
//   gossip / op round    the generic bodies (rings in LDS, set word re-read): some cluster is not in flood mode; they take one that is as it is
//   GENERAL round        the full body; it first writes the queues of the clusters in flood mode out to their rings
// (details at "FLOOD MODE" below; every round, delivery and message is still simulated: only the queue's representation differs; the one
// exception is a REMEMBERED flood, see "FLOOD MEMO" at the end of this comment).
// In that instantiation an op round also takes a RUN OF READS at once: a read leaves a quiescent cluster quiescent, so its next round is
// its generator's next op; while the op at hand is a read and the one behind it is again an op round's, the read is executed as a cluster
// round of its own (its rows at its own time, its payload from its own node's set, the time jump, the round count) before the wave-round's
// one gossip round and the op that ends the run.  The block of 32 generator draws of a cluster lives in LDS there, and what the rare paths
// derive from the lane number alone (the spill pointer, the instance's key, constant row words) is computed where it is used: the
// registers that frees are what the run needs at 80 VGPRs (see "READ RUNS" below).
// There, too, the two clusters PAIR their op rounds: a half that is ready for its op while its partner is in the middle of a flood waits
// (it is parked: the wave-rounds are the partner's gossip rounds) until the partner is ready as well, so that one op wave-round serves
// both (see "PAIRED OP ROUNDS" at the exit test of the gossip loop).
// And there the flood gossip rounds of a wavefront run in a loop of their own, the FLOOD STRETCH: between two such rounds nothing that R0 and
// the exit test look at can change unless a half runs out of due envelopes or a parked half's count-down ends, so the loop's back edge
// tests just that; inside it the flood bodies publish fan-out masks instead of envelopes (see "FLOOD STRETCH" at the flood gossip body and
// DUO_FLOOD_ARRIVALS).
// That instantiation is TRIMMED of vector instructions the result does not need: no body counts the delivered envelopes (servers_recv follows
// from the arrivals and what is left undelivered when the cluster stops), a flood's set word goes to HBM once, before something can read it
// there, and an op wave-round derives its half's offsets once (see "TRIM" in sim_kernel_duo).
// Its op wave-rounds, finally, have a body for the case that pairing has made the rule, the QUIET OP ROUND: every live half acts, from flood
// mode, so nothing is due or queued anywhere in the wavefront; the gossip part and the exchange are left out, a lane reads off its own
// adjacency mask whether the picked node's broadcast reaches it, and takes the envelope as the poll would have (see "QUIET OP ROUND" in
// the op round of sim_kernel_duo; every other op wave-round keeps the superset body).
// And the round that ends a flood stretch because a half has run out of due envelopes has, in the steady state of the main phase, a path
// of its own, the STEADY LEAVE: the tail of an op round notes per half (sd_m) that the half's next round can only be an op round's, and
// for such a half the stretch's exit does what R0's block and the exit test would have done, and nothing else: the time jump, the round
// count, the count-down, then the park of the dry half or the release of the parked one and the op round of both.  Everything else goes
// through the loop's head as ever (see "STEADY LEAVE" at the exit of the flood stretch and sd_m).
// FLOOD MEMO.  In that instantiation, at last, a flood is simulated ONCE per origin and pair of clusters, then applied.  A quiet op round
// takes a broadcast only from a quiescent cluster, there is no draw per message and no nemesis, so what the flood does to the cluster
// (every node's set gains the value's bit, n_arr and rounds rise, nothing is left queued or held) is a function of the topology and the
// picked node alone.  The wavefront records, in a table in LDS that its two clusters share, what its own simulation of the first flood from
// an origin did, per lane, and a later broadcast from that origin by a steady half applies the record in the op round itself: the rounds,
// deliveries and messages of that flood are not simulated again.  Two halves that come out of an op round with nothing in flight (reads,
// replayed broadcasts) go straight to their next op round, the DIRECT WAY ON (see "FLOOD MEMO" in sim_kernel_duo; -DDUO_NO_MEMO
// compiles all of it out, -DDUO_MEMO_VERIFY makes the emulator and -DDUO_PROF builds simulate a remembered flood and compare).
// STEADY RUN.  A remembered broadcast being as cheap as a read, the loop of the read runs takes it as a cluster round too: a half goes from
// one block of 32 draws to the next inside the loop, and the quiet body, the tail and the head of an op wave-round are paid once per
// block (see "STEADY RUN" at the read runs of sim_kernel_duo; -DDUO_NO_STEADY_RUN compiles it out).
// BLOCK PLAN.  What that loop does op after op is closed-form over the block of draws, so in front of it lane k of a half plans draw k:
// prefix sums give its op's time, value count, rows and payload offset, it tests on them what the loop tests, and the longest prefix of ops
// that all pass is committed at once (62 rows by 31 lanes, the reads' payload written as the all-ones sets it must hold, under facts about
// the sets that are checked per half; the loop stays the fallback for whatever the plan declines; see "BLOCK PLAN" in front of the steady
// run's loop of sim_kernel_duo; -DDUO_NO_BLOCK_PLAN compiles it out).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>

#include "wave_common.h"
#include "log2_table.h"

namespace {

__constant__ u32 duo_log2_q24[257];

enum { DK_PLAIN = 0, DK_BCAST = 1, DK_READ = 2, DK_READ_FINAL = 3, DK_INIT = 4, DK_TOPO = 5 };  // kind of an envelope (bits 24-26)
constexpr u32 DUO_DROP_ONE = 1u << 8;   // the flood instantiation: a lane's my_flags counts the envelopes it dropped in units of this, above the flag bits
static_assert(DUO_DROP_ONE > MSIM_FLAG_JOURNAL_OVERFLOW && DUO_DROP_ONE == 1u << 8, "the drop count lies above every flag, from bit 8 on");
#ifndef DUO_BAG_N
#define DUO_BAG_N 16
#endif
constexpr u32 DUO_BAG = DUO_BAG_N;   // random latencies: envelopes of a node's queue that live in LDS (a power of two, 4 .. 16; the rest spills to HBM behind a cached minimum)
// History rows go from their lanes to HBM unstaged (two 16-byte rows per operation; the L2 merges them into lines: WRITE_SIZE stays at the
// algorithmic bytes): 9.00 -> 8.90 ms per 4096 clusters against staging 64 rows in LDS.
// The flood instantiation of the latency-0 kernel: flood mode (see "FLOOD MODE" in sim_kernel_duo) and everything built on it, the read runs,
// the paired op rounds, the flood stretch, the trims, the quiet op round and the steady leave.  -DDUO_NO_FLOOD compiles all of it out: the
// latency-0, degree <= 4 instantiation is then the generic code the five other instantiations run, the live reference of the tests.
#ifdef DUO_NO_FLOOD
constexpr bool DUO_FLOOD_ON = false;
#else
constexpr bool DUO_FLOOD_ON = true;
#endif
// The flood memo of the flood instantiation (see "FLOOD MEMO" in sim_kernel_duo): a flood from an origin the wavefront has simulated before
// is applied from the record of that simulation, and two halves with nothing in flight go from one op round to the next directly;
// -DDUO_NO_MEMO compiles it out for A/B runs (the kernel is then the previous one, instruction for instruction).
// (the -DDUO_PROF_STRETCH and -DDUO_PROF_STEADY builds count the rounds of simulated floods, inside stretches and at their exits: they leave the
//  memo out, since a remembered flood has no rounds to count; -DDUO_PROF_MEMO is the profile build of this path)
#if defined(DUO_NO_MEMO) || defined(DUO_PROF_STRETCH) || defined(DUO_PROF_STEADY)
constexpr bool DUO_MEMO_ON = false;
#else
constexpr bool DUO_MEMO_ON = true;
#endif
// what the kernel's MEMO is for the instantiation that has it: msim_launch_duo gives that one the table's LDS
constexpr bool DUO_MEMO_BUILD = DUO_MEMO_ON && DUO_FLOOD_ON;
constexpr u32 DUO_MEMO_BYTES = 32u * 32u * 2u;   // [origin][lane] of 16 bits
#if defined(DUO_MEMO_VERIFY) && (defined(MSIM_HIPEMU) || defined(DUO_PROF))
constexpr bool DUO_MEMO_CHECK = true;    // a remembered flood is simulated all the same and compared with its record
#else
constexpr bool DUO_MEMO_CHECK = false;
#endif
// The steady run of the memo instantiation (see "STEADY RUN" at the read runs of sim_kernel_duo): the loop of the read runs also takes a
// broadcast whose flood is remembered, as a cluster round of its own, so that a half goes through a whole block of draws inside the loop;
// -DDUO_NO_STEADY_RUN compiles it out for A/B runs (the kernel is then the previous one, instruction for instruction).  The verifying
// build (DUO_MEMO_CHECK) takes no broadcast into a run: it simulates every remembered flood.
// (the -DDUO_PROF builds split the op wave-rounds by the body that took them, with the cycles of each kind and the count of quiet ones:
//  they leave the steady run out, as the -DDUO_PROF_STRETCH and -DDUO_PROF_STEADY builds leave the memo out, since it leaves a few dozen op
//  wave-rounds per wavefront to split, one per block of draws; -DDUO_PROF_RUN is the profile build of this path)
#if defined(DUO_NO_STEADY_RUN) || (defined(DUO_PROF) && !defined(DUO_PROF_RUN))
constexpr bool DUO_SRUN_ON = false;
#else
constexpr bool DUO_SRUN_ON = true;
#endif
// The block plan of the steady-run instantiation (see "BLOCK PLAN" in front of the steady run's loop in sim_kernel_duo): the ops of a block
// of draws that the loop would take one after the other are taken at once, lane k planning draw k; -DDUO_NO_BLOCK_PLAN compiles it out for
// A/B runs (the kernel is then the previous one, instruction for instruction).
// -DDUO_BLOCK_PLAN_NO_FACTS (developer / tests) treats every half's sets as not uniform: the plan is compiled in and always declines.
#ifdef DUO_NO_BLOCK_PLAN
constexpr bool DUO_BPLAN_ON = false;
#else
constexpr bool DUO_BPLAN_ON = true;
#endif
constexpr u32 DUO_BPLAN_BYTES = 32u * 4u;   // [origin]: what a remembered flood adds to its half's sum of n_arr | its rounds << 16
// FLOOD TABLE.  A record is a function of the topology, the fan-out rule and the picked node alone (see "WHY A RECORD DOES NOT DEPEND ON THE
// STATE" in sim_kernel_duo), so the memo tables of all wavefronts of all launches of a context are one table.  It is made once per context
// (msim_duo_make_flood_table): one wavefront of this kernel runs two clusters of the context's configuration on slabs of its own, and its
// epilogue copies what its recording path has left in LDS (the records, the block plan's totals, mm_known and mm_full) to a device buffer
// of the context; every later wavefront starts from a copy of that buffer instead of an empty table.  Nothing else changes: an origin the
// table lacks is recorded by the wavefront that meets it, as before.  The buffer: DUO_TABLE_HDR words of header (mm_known, mm_full, the
// N and the topology | echoback << 8 it was made for), the records, the totals.
// -DDUO_NO_FLOOD_TABLE compiles it out for A/B runs (the kernel is then the previous one, instruction for instruction).  The -DDUO_PROF
// builds leave it out, since their tests count a wavefront's own recordings; -DDUO_PROF_TABLE is the profile build of this path.
#if defined(DUO_NO_FLOOD_TABLE) || (defined(DUO_PROF) && !defined(DUO_PROF_TABLE))
constexpr bool DUO_TABLE_ON = false;
#else
constexpr bool DUO_TABLE_ON = true;
#endif
constexpr u32 DUO_TABLE_HDR = 4u;   // words
constexpr u32 DUO_TABLE_BYTES = DUO_TABLE_HDR * 4u + DUO_MEMO_BYTES + DUO_BPLAN_BYTES;
constexpr u32 DUO_TABLE_COPY16 = (DUO_MEMO_BYTES + (DUO_BPLAN_ON ? DUO_BPLAN_BYTES : 0u)) / 16u;   // what a wavefront has of it in LDS, 16 bytes a lane and pass
static_assert(DUO_MEMO_BYTES % 16u == 0 && DUO_BPLAN_BYTES % 16u == 0 && DUO_TABLE_COPY16 <= 192u, "the table is copied 16 bytes a lane, three passes at most");
constexpr u32 DUO_SRUN_FAR = 8192u;  // more than one run can add to a cluster's rounds: 31 ops of a block x (a record of at most 255 rounds + 1)
#ifndef DUO_PAIR_WAIT
// Wave-rounds.  A wait that ends in a shared op round leaves the two clusters in step (their floods start together, so the next wait is the
// difference of two floods' lengths); one that runs out was paid for nothing and leaves them out of step.  Measured, the longer the
// better, on the headline grid (no wait there exceeds 10) and on a line of 24 nodes, whose floods take up to 25 rounds: 24 is the first
// cap that does not cost that shape anything (profiles/r13_pair_wait_sweep.jsonl).  It bounds the wait where floods are longer still.
#define DUO_PAIR_WAIT 24
#endif
static_assert(DUO_PAIR_WAIT >= 1 && DUO_PAIR_WAIT <= 1024, "the wait cap of a parked half");
#ifndef DUO_LDS_PAD
#define DUO_LDS_PAD 0   // A/B builds (-DDUO_LDS_PAD=<bytes>): unused LDS per wavefront, fewer wavefronts per CU (msim_launch_duo)
#endif

struct DuoParams {
  KParams k;
  u32 n_inst;        // clusters in this launch (the last wavefront may hold one)
  u32 R;             // LDS ring entries per node (power of two >= inbox_capacity)
  u32 S;             // HBM spill entries per node behind the ring (R + S = inbox_capacity + spill_capacity)
  u32 half_bytes;    // LDS bytes per cluster
  u32 off_ring;      // byte offset of the queues inside a cluster's LDS region
  u32 sets_off;      // word offset of the cluster's set region inside its instance's scratch (msim_duo_extra_scratch_words)
  u32 inst_bytes;    // scratch bytes per instance: the distance between the set regions of a wavefront's two clusters
  u32 deg;           // maximum degree of the topology
  u32 echoback;      // node program without skip-sender
  u32 round_limit;
  u32 off_seq;       // RND: byte offset of the arrival-sequence array (u16 per ring entry) inside a cluster's LDS region
  u32 off_log2;      // RND: byte offset of the Q24 log2 table (one per wavefront, behind both clusters)
  u32 off_dc;        // flood instantiation: byte offset of the block of 32 generator draws inside a cluster's LDS region
  u32 off_memo;      // memo instantiation: byte offset of the wavefront's table of remembered floods (behind both clusters' regions)
  u32 table_fill;    // memo instantiation: this launch MAKES the flood table: its one wavefront's epilogue writes `table` (else the prologue reads it)
  u32 *table;        // memo instantiation: the context's flood table (see "FLOOD TABLE"), or null: every wavefront starts with an empty one
};

// -ln(u), u = (r+1)/2^32, Q16, integer only: the sampler of engine.hip / the oracle over a copy of the table in LDS
__device__ __forceinline__ u32 duo_neg_ln_q16(u32 r, const u32 *tab) {
  if (r == 0xFFFFFFFFu) return 0;
  const u32 v = r + 1;
  const u32 e = 31 - __clz(v);
  const u32 m = v << (31 - e);
  const u32 idx = (m >> 23) & 0xFF;
  const u32 f = (m >> 7) & 0xFFFF;
  const u32 l0 = tab[idx], l1 = tab[idx + 1];
  const u32 lg = (e << 24) + l0 + (u32)(((u64)(l1 - l0) * f) >> 16);
  const u32 d = (32u << 24) - lg;
  return (u32)(((u64)d * 2977044472ull) >> 40);
}

// the cluster's half of a wave ballot
__device__ __forceinline__ u32 hb(bool pred, bool hi) {
  const u64 b = __ballot(pred);
  return hi ? (u32)(b >> 32) : (u32)b;
}
// true in every lane of a half iff pred holds in some lane of that half; scalar work only (the result is a lane mask in SGPRs)
__device__ __forceinline__ bool half_any(bool pred) {
  const u64 b = __ballot(pred);
  const u32 lo = (u32)b ? 0xFFFFFFFFu : 0u, up = (u32)(b >> 32) ? 0xFFFFFFFFu : 0u;
  return __builtin_amdgcn_inverse_ballot_w64(((u64)up << 32) | lo);
}
// min over the 32 lanes of the caller's half (result uniform per half)
__device__ __forceinline__ u32 half_min(u32 v, bool hi) {
  v = min(v, dpp_mov<0xB1, 0xF, 0xF, false>(v, v));   // quad_perm [1,0,3,2]
  v = min(v, dpp_mov<0x4E, 0xF, 0xF, false>(v, v));   // quad_perm [2,3,0,1]
  v = min(v, dpp_mov<0x141, 0xF, 0xF, false>(v, v));  // row_half_mirror
  v = min(v, dpp_mov<0x140, 0xF, 0xF, false>(v, v));  // row_mirror
  const u32 lo = min(rdlane(v, 0), rdlane(v, 16)), up = min(rdlane(v, 32), rdlane(v, 48));
  return hi ? up : lo;
}
// A ballot of one compare is that compare's lane mask; a ballot of a bool built from several compares (a & b, a | b) costs two more
// vector instructions (the mask is turned into 0 / 1 and compared again).  Hot paths therefore combine the ballots of single compares
// with scalar operations: bal(a) & bal(b) == bal(a & b), bal(a) | bal(b) == bal(a | b).
__device__ __forceinline__ u64 bal(bool pred) { return __ballot(pred); }
// The lane mask of ONE unsigned compare as one instruction: the compare intrinsic is its own ballot.  bal(a == b) is a compare and a ballot;
// where a and b stand through a loop the optimizer hoists the compare out of it as a bool, and the ballot left behind turns that bool into
// 0 / 1 and compares again (two vector instructions per use).  code_: 32 ==, 33 !=, 36 <, 37 <= (unsigned).
#ifdef MSIM_HIPEMU
#define DUO_BAL_CMP(a_, op_, b_, code_) bal((u32)(a_) op_ (u32)(b_))
#else
#define DUO_BAL_CMP(a_, op_, b_, code_) ((u64)__builtin_amdgcn_uicmp((u32)(a_), (u32)(b_), code_))
#endif
// A per-cluster boolean kept as a lane mask in SGPRs (all 32 bits of a half set or clear): a test of it costs scalar work only, bal() of it is
// the mask itself, and a per-lane use reads the lane's bit (lane_in)
__device__ __forceinline__ u64 hm2(bool lo, bool up) { return (lo ? 0xFFFFFFFFull : 0ull) | (up ? 0xFFFFFFFF00000000ull : 0ull); }
__device__ __forceinline__ bool lane_in(u64 m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// a value every lane holds alike, as one the compiler knows to be so (an SGPR)
#ifdef MSIM_HIPEMU
#define DUO_UNIFORM(x_) (x_)
#else
#define DUO_UNIFORM(x_) ((u32)__builtin_amdgcn_readfirstlane((int)(x_)))
#endif
__device__ __forceinline__ u32 bperm(u32 byte_addr, u32 v) { return (u32)__builtin_amdgcn_ds_bpermute((int)byte_addr, (int)v); }

// element idx_ of an array, as the base plus a 32-bit BYTE offset (the whole array is below 4 GiB): the form whose address is the base in
// SGPRs and one VGPR
template <typename Tp>
__device__ __forceinline__ Tp *duo_at(Tp *base, u32 idx) {
  return reinterpret_cast<Tp *>(reinterpret_cast<unsigned char *>(base) + (size_t)(u32)(idx * (u32)sizeof(Tp)));
}

// Latency 0: at least 6 wavefronts per SIMD (<= 80 VGPRs), what three launches of 2048 wavefronts in flight need; with the op round
// beside the GENERAL body the register allocator otherwise takes 86 to 92 (no spills at 80)
// (the -DDUO_PROF builds: 4 per SIMD, 128 VGPRs.  Their counters are per-lane registers, and at 80 they went to scratch memory, 36 bytes per
//  lane before the flood stretch and 156 with its counters: the cycles such a build reported were its own spills' as much as the kernel's.
//  tools/duo_prof_report.py runs one launch at a time, two wavefronts per SIMD, so the bound costs its figures nothing)
#ifdef DUO_PROF
#define DUO_LAT0_WAVES 4
#else
#define DUO_LAT0_WAVES 6
#endif
template <bool LAT0, bool DEG4, bool RND>
__global__ void __launch_bounds__(64, LAT0 ? DUO_LAT0_WAVES : 1) sim_kernel_duo(const DuoParams dp) {
  static_assert(!(RND && LAT0), "random latency needs deadlines");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KParams &p = dp.k;
  const u32 lane = threadIdx.x, i = lane & 31u;
  const bool hi = lane >= 32u;
  const u32 N = p.N, W = p.W, R = dp.R, Rm = dp.R - 1u, S = dp.S;
  const bool is_node = i < N;
  const u32 inst_raw = blockIdx.x * 2u + (hi ? 1u : 0u);
  const bool real = inst_raw < dp.n_inst;
  const u32 inst = real ? inst_raw : dp.n_inst - 1u;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt = (1u << i) - 1u;
  const u32 all_nodes = N >= 32 ? 0xFFFFFFFFu : ((1u << N) - 1u);
  const u32 max_values = p.cfg.max_values, max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 rate = p.cfg.rate_mhz;
  const u32 lat_us = LAT0 ? 0u : p.cfg.latency_mean_ms * 1000u;
  // a sender's "src to skip" field never equals 64: without skip-sender every neighbour takes the value
  const u32 me16 = dp.echoback ? (64u << 16) : (i << 16);
  const u32 round_limit = dp.round_limit;

  // The instantiation with a flood mode (see below), and with all that is built on it: its op rounds take a run of reads at once and wait
  // for each other, so that one op round serves both halves; the gossip rounds of a flood run in a loop of their own; the op wave-round
  // of quiescent flood halves has a body of its own; a flood stretch is left for a park or an op round without R0 and the exit test.
  constexpr bool FLOOD = DUO_FLOOD_ON && LAT0 && DEG4 && !RND;
  // TRIM (of the flood instantiation; every part is output-identical to counting and storing round by round, as the other instantiations do):
  //   (A) n_rsv is not counted round by round.  Every server envelope counted in n_arr at its commit is received exactly once unless it is
  //       still queued or held when its cluster stops, or was dropped at a full queue (MSIM_FLAG_INBOX_OVERFLOW).  At latency 0 a lane's queue and hand hold in_n + sp_n + [deliver_at != INF] envelopes, of which `busy` is its own client's
  //       request (a busy client's request is queued or held: the node completes it in the round it handles it).  The two places that clear
  //       a stopped half's queue add that number to the count of dropped envelopes above my_flags' flag bits, an envelope dropped at a full
  //       queue adds one there (a dropped request: one, which `busy` takes off again), the epilogue puts the count into n_rsv, and
  //       servers_recv = sum(n_arr) - sum(n_rsv): what a count per round gives, for flagged instances too.  n_rsv is thus no register
  //       across the rounds, the one the op round's third body needs at 80 VGPRs.
  //   (B) the flood bodies do not store sw.  A half in flood mode holds in sw, in EVERY lane, its column's word of value next_value - 1 (word 0
  //       while next_value == 0), and writes it back with one wave-wide store at the points after which its HBM copy can be read: the head
  //       of an op round in which it acts (before the read runs and the read op's copy) and DUO_MATERIALISE.  An acting half in flood
  //       mode takes the op's word from sw instead of loading it; any acting half loads THAT word, not the op's value's: the two differ only
  //       when the value opens a new word, and a word no value has fallen in yet is 0 in every lane (a broadcast value is fresh).
  //   (C) the half's 0 / ~0 is derived once per op wave-round and GENERAL body (duo_upm, from a lane number the optimizer cannot see
  //       through, so that nothing of it lives across the gossip loop), and rows and payload are addressed as the wavefront's base plus a
  //       32-bit byte offset (msim_launch_duo checks that the two slabs of a wavefront stay below 4 GiB).
  constexpr bool MEMO = DUO_MEMO_ON && FLOOD;                    // ... and simulate a flood once per origin, then apply what that simulation did
  constexpr bool SRUN = DUO_SRUN_ON && MEMO && !DUO_MEMO_CHECK;   // ... and take a remembered broadcast as a cluster round of the read runs' loop
  constexpr bool BPLAN = DUO_BPLAN_ON && SRUN;                   // ... and plan the steady ops of a block of draws across the lanes
  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  // FLOOD: the cluster's rows and payload are addressed like its sets, from the wavefront's base (SGPRs: the lower cluster's) and the
  // half's 0 / ~0, so that no lane keeps a 64-bit pointer to them (the registers: 80 with room for the flood bodies)
  msim_op *const w_rows = p.rows + (size_t)(blockIdx.x * 2u) * max_rows;
  u32 *const w_pay = p.payload + (size_t)(blockIdx.x * 2u) * max_pay;
  // (the half's share of the offset comes from duo_upm, see TRIM (C), so that it is not kept in a register across the rounds; only live
  //  clusters write rows or payload, and an upper half that holds no cluster is never live)
#define DUO_UP(x_) (duo_upm & (x_))
#define DUO_UPM_NOW() u32 duo_upm = 0; if (FLOOD) { DUO_LANE_NOW(um_l); duo_upm = 0u - (um_l >> 5); }
#define DUO_ROW(idx_) (reinterpret_cast<uint4 *>(FLOOD ? duo_at(w_rows, DUO_UP(max_rows) + (idx_)) : g_rows + (idx_))[0])
#define DUO_PAY(idx_) ((FLOOD ? duo_at(w_pay, DUO_UP(max_pay) + (idx_)) : g_pay + (idx_))[0])
  // HBM spill behind the LDS ring: {deadline, envelope} pairs in the node's slice of the spill area
  u64 *const my_spill = reinterpret_cast<u64 *>(reinterpret_cast<uint4 *>(p.scratch + (size_t)inst * p.scratch_words + p.spill_off) +
                                                    (size_t)(is_node ? i : 0) * p.spill_cap);

  // FLOOD: what the rare paths derive from the lane number alone is computed where it is used, from a lane number the optimizer cannot
  // see through, so that no register holds it across the rounds.  These two are the ONLY second definitions of `lane` and `inst` (above):
  // whoever changes how a lane finds its instance changes them here as well.
#define DUO_LANE_NOW(l_) u32 l_ = threadIdx.x; MSIM_OPAQUE(l_)
#define DUO_INST_OF(l_) (blockIdx.x * 2u + ((l_) >> 5) < dp.n_inst ? blockIdx.x * 2u + ((l_) >> 5) : dp.n_inst - 1u)
  // The flood instantiation computes the pointer where the (rare) spill code uses it, from a lane number the optimizer cannot see through:
  // no register pair holds it across the rounds
#define DUO_MY_SPILL(ptr_)                                                                                                \
    u64 *ptr_ = my_spill;                                                                                                 \
    if (MEMO) {                                                                                                           \
      /* (the memo instantiation: the wavefront's base in SGPRs and a 32-bit byte offset, like the sets; the 64-bit form below took two  \
         registers more than the superset op round's checked append has to spare there.  The offset fits 32 bits: dp.inst_bytes, the   \
         distance to the upper cluster's scratch, is below 2 GiB (msim_launch_duo returns MSIM_LAYOUT_DOES_NOT_FIT otherwise), and the    \
         node's slice starts inside the instance's own spill area, node * spill_cap * 16 < 32 nodes x 65536 envelopes x 16 B = 32 MiB) */ \
      DUO_LANE_NOW(ms_l); const u32 ms_i = ms_l & 31u;                                                                    \
      const u32 ms_off = (DUO_INST_OF(ms_l) - blockIdx.x * 2u) * dp.inst_bytes + (ms_i < N ? ms_i : 0u) * p.spill_cap * 16u;          \
      ptr_ = reinterpret_cast<u64 *>(reinterpret_cast<unsigned char *>(p.scratch + (size_t)(blockIdx.x * 2u) * p.scratch_words + p.spill_off) + (size_t)ms_off); \
    } else if (FLOOD) {                                                                                                   \
      DUO_LANE_NOW(ms_l); const u32 ms_i = ms_l & 31u;                                                                    \
      ptr_ = reinterpret_cast<u64 *>(reinterpret_cast<uint4 *>(p.scratch + (size_t)DUO_INST_OF(ms_l) * p.scratch_words + p.spill_off) + \
                                     (size_t)(ms_i < N ? ms_i : 0) * p.spill_cap);                                          \
    }
  // LDS of one cluster: [32 rings]
  unsigned char *const hmem = smem + (hi ? dp.half_bytes : 0u);
  // The nodes' seen sets: W x 32 words of HBM scratch per cluster, word-major ([word][lane]: lane i's column is node i's set, or a
  // dummy set of a lane that holds no node), so that a wave-wide access to one word of every node's set is one 128-byte line per
  // cluster.  Addressed as the wavefront's base (SGPRs: the set region of its lower cluster) + a 32-bit byte offset per lane; the
  // upper half's region lies inst_bytes further on (an upper half without a cluster shares the lower one's region and writes nothing).
  unsigned char *const sets = reinterpret_cast<unsigned char *>(p.scratch + (size_t)(blockIdx.x * 2u) * p.scratch_words + dp.sets_off);
  const u32 set_half = (inst - blockIdx.x * 2u) * dp.inst_bytes;   // byte offset of the cluster's region
  const u32 set_lane = set_half + i * 4u;                           // byte offset of word 0 of this lane's set
#define DUO_SET(boff_) (*reinterpret_cast<u32 *>(sets + (size_t)(u32)(boff_)))
  // slot-major rings: slot s of lane i at [s * 32 + i] (a wave-wide access to one slot position is contiguous)
  u32 *const ring32 = reinterpret_cast<u32 *>(hmem + dp.off_ring) + i;       // LAT0: the envelope word
  u64 *const ring64 = reinterpret_cast<u64 *>(hmem + dp.off_ring) + i;       // else deadline | envelope << 32
  // RND: the node's queue is a bag of R entries (ring64[0 .. in_n)) with their arrival sequence numbers beside them; lanes that
  // hold no node share one dummy bag; the spill holds {key, sequence} in 16 bytes
  // (slot-major: slot j of node i at [j * (N + 1) + i] — a wave-wide access to one slot is contiguous, free of bank conflicts;
  //  lane-major bags of 128 bytes put every lane on the same banks)
  const u32 BS = N + 1u;   // lanes per slot: the nodes and one dummy shared by the lanes that hold no node
  u32 *const bag_dl = reinterpret_cast<u32 *>(hmem + dp.off_ring) + (is_node ? i : N);             // deadlines: what recv! scans
  u32 *const bag_e = bag_dl + DUO_BAG * BS;                                                           // envelope words
  unsigned short *const bag_seq = reinterpret_cast<unsigned short *>(hmem + dp.off_seq) + (is_node ? i : N);
#define BAGDL(j_) bag_dl[(j_) * BS]
#define BAGE(j_) bag_e[(j_) * BS]
#define BAGSEQ(j_) bag_seq[(j_) * BS]
  u32 *const my_spill12 = p.scratch + (size_t)inst * p.scratch_words + p.spill_off + (size_t)(is_node ? i : 0) * p.spill_cap * 4;   // {deadline, envelope, sequence} x S
  u32 *const log2_tab = reinterpret_cast<u32 *>(smem + dp.off_log2);

  if (real) for (u32 w = 0; w < W; w++) DUO_SET(set_lane + w * 128u) = 0;   // (whatever the scratch held before: nothing is read unwritten)
  if (RND) for (u32 k = lane; k < 257u; k += 64) log2_tab[k] = duo_log2_q24[k];
  if (RND) for (u32 k = i; k < DUO_BAG * BS; k += 32) reinterpret_cast<u32 *>(hmem + dp.off_ring)[k] = INF;   // every bag slot is free
  __syncthreads();

  const u32 adj = is_node ? topo_adj(p.cfg.topology, N, i) : 0u;
  const u32 hbase4 = (lane & 32u) << 2;  // byte address of the half's lane 0 for ds_bpermute
  // DEG4 (every node has <= 4 neighbours, lane 31 holds no node): the neighbours in ascending order as bpermute addresses
  // (an unused slot points at lane 31, which never publishes) and the constant part of an envelope received from each
  u32 nbl[4] = {0, 0, 0, 0}, kc[4] = {0, 0, 0, 0}, nb_adj[4] = {0, 0, 0, 0};   // nb_adj (RND): the neighbour's own adjacency mask
  if (DEG4) {
    u32 rem = adj;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 s = rem ? (u32)__builtin_ctz(rem) : 31u;
      rem &= rem - 1u;
      nbl[k] = hbase4 + (s << 2); kc[k] = s << 16;
      if (RND) nb_adj[k] = s < N ? topo_adj(p.cfg.topology, N, s) : 0u;
    }
  }
  // FLOOD: the four neighbours' node numbers in one register (8 bits each, ascending like nbl), for the flood bodies, and what a node
  // leaves out of its fan-out: the bit of the envelope's src, or nothing without skip-sender
  // (there the generic bodies take an envelope's constant part from it as well: kc's four registers are what the stretch needs)
#ifdef MSIM_HIPEMU
  // the quiet op round leans on the neighbour relation being SYMMETRIC (bit a of adj(b) == bit b of adj(a)), as it is for every shape topo_adj builds
  // with at most four neighbours (grid, partial grids included, line, tree2/3/4: each edge is set from both ends); see the quiet op round
  if (FLOOD) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const u32 sy_a = bperm(nbl[k], adj);   // the adjacency mask of neighbour k (an unused slot: lane 31's, which is 0 and not looked at)
      if ((kc[k] >> 16) != 31u && ((sy_a >> i) & 1u) == 0) __builtin_trap();
    }
  }
#endif
  u32 nbp = 0;
  if (FLOOD) nbp = (kc[0] >> 16) | (kc[1] >> 8) | kc[2] | (kc[3] << 8);
#define DUO_KC(k_) (FLOOD ? ({ u32 kc_p = nbp; MSIM_OPAQUE(kc_p); ((kc_p >> (8 * (k_))) & 31u) << 16; }) : kc[k_])   /* (computed where it is used: not hoisted into four registers again) */
  const u32 fan_skip = dp.echoback ? 0u : 1u;

  // ---- per-lane state: node i and its client (u32 throughout: flags are 0 / 1) ----
  u32 deliver_at = INF;      // INF = recv! holds no envelope (then the queue is empty too: idle receivers poll at once)
  u32 cm = 0;                // the envelope recv! is sleeping on: value | src << 16 | kind << 24 (src 63 = the node's own client)
  u32 in_n = 0, head = 0;    // LDS ring
  u32 bag_used = 0;          // RND: the slots of the LDS bag that hold an envelope (in_n = their number)
  u32 sp_n = 0, s_head = 0;  // HBM spill ring (rare)
  u32 have_creq = 0, creq = 0, creq_t = 0;  // latency > 0: the client's request waits beside the FIFO of server envelopes
  u32 busy = 0;              // the client has an RPC outstanding
  u32 n_cl = 0, n_arr = 0, n_rsv = 0, my_flags = 0;  // client RPCs completed, server envelopes arrived / delivered
  // ---- per-cluster state (uniform within a half) ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, next_value = 0, sleep_until = 0;
  u32 n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 next_id = 0;           // RND: message ids (net.clj:103,197), every send! of the cluster in canonical order
  u32 my_seq = 0;            // RND (per lane): arrivals queued at this node so far
  u32 spm_dl = INF, spm_seq = 0, spm_e = 0, spm_i = 0;   // RND: the minimum of the spilled part of the bag, cached in registers
  u32 pbase = 0;             // RND (per lane): id of the first message this node sends in the current round
  const u32 lat_mean = p.cfg.latency_mean_ms;
  const bool lat_uniform = p.cfg.latency_dist == MSIM_LAT_UNIFORM;
  // the clusters still running, and those whose every round has to be a GENERAL one until the scheduler says otherwise: lane masks
  // (hm2 / lane_in); when the scheduler next acts (INF: it only waits).  All three change in GENERAL rounds and at time jumps only.
  u64 alive_m = bal(real), fg_m = alive_m;
  u32 alive_v = real ? 1u : 0u;   // lane_in(alive_m) as 0 / 1, for the round count of every wave-round (one add, no select)
  u32 sched_at = real ? 0u : INF;
  // The generator's draws (one 64-bit draw per generated op, stream S_GEN, counter gen_k) are computed 32 at a time: lane i of a cluster
  // holds draw dc_base + i, the scheduler fetches the one it needs with two ds_bpermute (mix64's three 64-bit multiplications cost a
  // round of the scheduler a quarter of its cycles when every lane computed the same draw)
  // The flood instantiation keeps the block in LDS (256 bytes per cluster; a cluster's draw is one ds_read_b64 of an address all its
  // lanes share) and so has two registers more for its op rounds.
  u32 dc_base = 0; u64 dc = draw64(key, S_GEN, (u64)i);
  // (addressed from a lane number the optimizer cannot see through: no register holds an address of it across the rounds)
#define DUO_DCL(idx_) (reinterpret_cast<u64 *>(smem + (duo_upm & dp.half_bytes) + dp.off_dc)[idx_])
#define DUO_DCL_MINE() (reinterpret_cast<u64 *>(smem + ({ u32 dl_l = threadIdx.x; MSIM_OPAQUE(dl_l); (dl_l >= 32u ? dp.half_bytes : 0u) + (dl_l & 31u) * 8u; }) + dp.off_dc)[0])
  if (FLOOD) { DUO_DCL_MINE() = dc; dc = 0; wave_lds_fence(); }
#define DUO_DRAW(k_, hi_, lo_) do {                                                                                       \
    if (FLOOD) { const u64 dd_v = DUO_DCL(((k_) - dc_base) & 31u); hi_ = (u32)(dd_v >> 32); lo_ = (u32)dd_v; }                 \
    else { const u32 dd_at = hbase4 + (((k_) - dc_base) << 2); hi_ = bperm(dd_at, (u32)(dc >> 32)); lo_ = bperm(dd_at, (u32)dc); } \
  } while (0)
#define DUO_DRAW_REFILL(cond_) do {                                                                                       \
    const bool dr_c = (cond_);                                                                                            \
    if (__ballot(dr_c)) {                                                                                                 \
      u64 dr_key = key;                                                                                                   \
      if (FLOOD) {   /* the instance's key again, from a lane number the optimizer cannot see through: once per 32 ops, no register between them */ \
        DUO_LANE_NOW(dr_l);                                                                                               \
        dr_key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + DUO_INST_OF(dr_l) + 1));                  \
      }                                                                                                                   \
      const u64 dr_new = draw64(dr_key, S_GEN, (u64)gen_k + i);                                                           \
      if (FLOOD) { if (dr_c) DUO_DCL_MINE() = dr_new; wave_lds_fence(); } else dc = dr_c ? dr_new : dc;                            \
      dc_base = dr_c ? gen_k : dc_base;                                                                                   \
    }                                                                                                                     \
  } while (0)
  // RND: the same for the messages' latency draws (stream S_LATENCY, counter = message id, net.clj:178-187): a gossip round sends 1.3
  // messages on average, and every lane of the wavefront computed a draw (mix64, the logarithm) for them — a third of the round's vector
  // instructions.  Lane i of a cluster holds the latency (ms) of message id lc_base + i; DUO_RND_IDS keeps the block under the round's ids.
  u32 lc_base = 0xFFFFFFC0u, lc = 0; bool lc_all = false;   // (no block yet: the first round with a send draws one)

  // Two reads are kept one round ahead of their use, so that a round's dependent chain holds one LDS round trip
  // (the ds_bpermute exchange) instead of three:
  //   sw = the word of the node's set that cm's value falls in (re-read after every change of cm or of the set; an L1 / L2 hit);
  //   nx = the head entry of the ring (valid while in_n != 0; an append to an empty ring sets it from registers).
  u32 sw = 0;
  u32 nx = 0, nx_dl = 0;
  // FLOOD MODE (latency 0, DEG4, rings of at least 8 entries).  At latency 0 an op round runs its op only when the cluster is quiescent:
  // nothing is held, nothing queued.  From then until the cluster's next op every server envelope in flight carries the op's value (the
  // flood of that broadcast), so a node's queue is a run of equal envelopes and need not be written out: it is the count in_n, nx is the
  // word of its head (only the first envelope a node ever handles for the value can be new to it, so only that one's src matters: a later
  // entry is a duplicate whatever its src), and "seen" is one bit of a word the node itself last wrote.  A node sends the value at most
  // once, so at most 4 envelopes ever reach a node during a flood: in_n <= 4 <= R - 4, the fast-path condition of DUO_ARRIVALS cannot
  // fail and sp_n stays 0 (overflow and the spill are only ever handled by the generic code).
  // fl_m = the halves in flood mode (a lane mask like alive_m).  For such a half
  //   * deliver_at, cm, in_n, n_arr, n_rsv, rounds mean what they always mean; sp_n == 0;
  //   * the ring slots [head, head + in_n) are NOT valid (nobody reads them), every queued envelope is DK_PLAIN with the flood's value;
  //   * sw is the node's set word for the flood value's word in EVERY lane, kept current in the register: no set word is loaded.
  // An op round puts its acting halves into flood mode (op_w, the word it loads for every lane, becomes sw).  When every live half is in
  // flood mode a wave-round runs a FLOOD body: no LDS store, no LDS load besides the pulls, no global load.  The generic gossip and op
  // rounds take a half in flood mode as it is (they keep its sw and nx in registers; what they store in its ring is never read); the
  // GENERAL body first MATERIALISES every such half: its in_n entries are written to the ring and the flag is cleared.
  const bool fl_ok = FLOOD && R >= 8u;
  u64 fl_m = 0;
  // PAIRED OP ROUNDS: the half that is parked, i.e. ready for its op and waiting for its partner (a lane mask like fl_m; 0: nobody), and the
  // wave-rounds it may still wait (counted down in every wave-round; far from 0 while nobody is parked)
  constexpr u32 PARK_IDLE = 0x7FFFFFFFu;
  u64 park_m = 0; u32 park_left = PARK_IDLE;
  // STEADY LEAVE: sd_m = the halves whose next round, once their flood has run dry, can only be an op round's (a lane mask of whole halves like
  // fl_m).  The tail of an op round sets a half's bit, on the state that round leaves, iff the half acted, no scheduler's view ran, and
  //   the half is in fl_m, next_value < max_values, n_rows + 2 <= max_rows, gen_k - dc_base < 32 (after the refill of the draws), and
  //   phase == PH_MAIN, gen_next < cutoff and busy == 0 in every lane, which hold where the bit is set without a compare (see the tail):
  // st_m's own terms (see the exit test) and what keeps the scheduler's view out of the way.  Why the bit still tells the truth when it is
  // used, at the exit of a flood stretch, about a half with nothing due:
  //   * phase, busy, next_value, n_rows, gen_k, dc_base, gen_next and cutoff are written by op rounds (the bit is set again at their tail,
  //     or cleared with the scheduler's view), by GENERAL bodies (their head clears every bit) and nowhere else: no gossip body, flood or
  //     generic, and nothing in R0 touches them.  fl_m is cleared by DUO_MATERIALISE alone, which only the GENERAL body calls;
  //   * fg_m grows in R0's block (the round limit) and in the scheduler's view: the block clears the bits of the halves it forces or finds
  //     stuck, the view's two callers clear all of them, and the use applies & ~fg_m again;
  //   * a half that does not act in an op round (it is in mid-flood beside its partner's op) keeps its bit: that round's gossip part is
  //     a gossip round to it.
  // So for a live half with its bit set and nothing due, st_m's five compares hold, and the sixth term, nothing due and no client busy,
  // holds by busy == 0 and the caller's own knowledge that nothing is due (a -DDUO_PROF build and the host-emulator build recompute all of
  // it at the use and trap if it differs).
  u64 sd_m = 0;
  // FLOOD MEMO.  mm_known = the origins whose flood this wavefront remembers (bit = node number; SGPRs, one mask for both halves: they run
  // the same configuration), mm_rec = the halves that are recording one (a lane mask of whole halves), mm_org = the origins they record
  // (lower half | upper half << 8).  The table in LDS holds 16 bits per origin and lane (the lane's number inside its half):
  //   while the origin is being recorded   n_arr & 0x7F | (rounds & 0xFF) << 8, as they stood just before the op round handed out the first hop;
  //   once it is remembered                 the rise of n_arr (<= 4: a node sends a value once) | the value's bit in sw at the end << 7 |
  //                                         the rise of rounds << 8 (the same in every lane of the row; < 256: a flood ends within N + 2 rounds).
  // RECORDING starts in the quiet op round, for a half that takes a broadcast from an origin not remembered (two halves with the same
  // one: the lower records), and ends where the steady leave finds that half dry and steady (dry_m, sd_m & ~fg_m): there the half holds
  // and queues nothing, so the rises are the whole flood's, and rounds stands at the dry point (sl_r1 less the round that is next).  A half
  // that reaches an op round's head or a GENERAL body still recording has not come by there: the recording is dropped (mm_rec is cleared)
  // and the origin stays unknown.  That covers every place that clears the half's bit of sd_m (the GENERAL body, and through it a
  // materialisation, a capacity stop and a dropped envelope, which only generic code meets; the tail's view branch and R0's forced or stuck
  // halves, which the steady leave then declines) and the round limit, which the steady leave declines as well.
  // WHY A RECORD DOES NOT DEPEND ON THE STATE.  The quiet op round acts on quiescent halves only: nothing queued, held or awaited in any
  // lane, and the value is fresh, so no node's set has its bit.  In this instantiation a message has no draw and no deadline, and a node
  // forwards a value once, to its neighbours less the sender (fan_skip), whatever else its set holds.  So which node handles which
  // envelope in which round follows from adj, fan_skip and the picked node; T stands through the flood; a flooding half is not parked, so
  // rounds rises by one per wave-round whichever body runs it (stretch, flood, generic or the gossip part of its partner's op round).
  // REPLAY (step 5 of the quiet op round) puts the half where its flood's dry point would: the rises are added, sw gains the bit where the
  // record has it, in_n stays 0 and deliver_at INF.  What it does not reproduce is cm and nx (the last envelope handled, the last queue
  // head).  Their readers behind a dry point: cm is read under `due` (deliver_at <= T) by every body and by the exit test's special-envelope
  // term, and a dry lane has nothing due; DUO_SEEN_WORD takes an address from cm's value for the generic bodies' prefetch of sw, which a
  // half in flood mode discards, and which is loaded again behind every change of cm once DUO_MATERIALISE has ended flood mode (cm's
  // value is an earlier one of the cluster, its word inside the set region); nx is read while in_n != 0 alone, and an arrival at an
  // empty queue sets it first.  n_arr and n_rsv are read by the epilogue (sums), in_n and deliver_at by the two places that stop a half
  // (what stays undelivered: nothing, as behind the simulated flood), sw by DUO_FLOOD_WB at the next op round's head (the replayed word is
  // the simulated one in every lane that holds a node; the other lanes' columns are never read).
  // The replaying half is dry at once, T standing at the op's time: a simulating partner finds it as it finds a half whose flood was short
  // (R0's block moves it to its next op, the exit test parks it).  The round limit: a replay takes place only if rounds + the longest
  // record replayed in this wave-round + the leaving round stays below round_limit in EVERY live half.  In its own half no look at the
  // limit during the flood could then have found anything; and the partner's limit is looked at whenever R0's block is entered, which the
  // replaying half's dry point used to cause that many rounds into the partner's flood and now causes at once: the partner's term makes
  // sure that neither look finds anything.  It also needs T < gen_next < cutoff, room for a value and two rows (sd_m's terms on the state
  // this round leaves: the half's next round is an op round's) so that no op or view of the half's OWN scheduler could have met the flood
  // in mid-run.  Its PARTNER's can: a partner that reaches the cutoff, a capacity or its round limit in the same op round forces GENERAL
  // bodies, with DUO_MATERIALISE, on a half in mid-flood.  The record applies all the same, and the argument rests on this: the generic
  // code simulates the same deliveries from the materialised queues (the same envelopes in the same rounds, n_arr counted at the commit), no
  // scheduler acts on the half (its sched_at lies ahead of T until the flood has run dry), and rounds still rises by one per wave-round.
  // The replayed half is dry in those GENERAL bodies, which then do nothing for it before its own next op.  (The -DDUO_MEMO_VERIFY trap in
  // the GENERAL body covers a scheduler that acts on the verifying half itself, act_b, and nothing else; a GENERAL body the partner forces
  // lets the verification run on, and the head of the half's next op round, or the GENERAL body that acts on it, compares or drops it.)
  u32 mm_known = 0, mm_org = 0; u64 mm_rec = 0;
  // (addressed from a lane number the optimizer cannot see through, where it is used: no register holds an address of it across the rounds)
#define DUO_MEMO_AT(org_, l_) (reinterpret_cast<unsigned short *>(smem + dp.off_memo)[(org_) * 32u + ((l_) & 31u)])
  // -DDUO_MEMO_VERIFY (emulator and -DDUO_PROF builds): the halves whose flood is simulated although it is remembered, their record and
  // where n_arr and rounds stood; compared when the half next acts (the head of an op round; a GENERAL body that acts on it in mid-flood traps)
  u64 vf_m = 0; u32 vf_e = 0, vf_n0 = 0, vf_r0 = 0, vf_bit = 0;
  // BLOCK PLAN (see there): mm_full = the remembered origins whose record has the value's bit in every node lane (a subset of mm_known);
  // bp_vw_lo / bp_vw_hi = how many leading words of the half's sets were SEEN to be all ones in every node lane when they were completed
  // (SGPRs); DUO_BPLAN_TOT(origin) = the sum of the origin's record over the half's lanes | its rounds << 16 (LDS, behind the memo table).
  u32 mm_full = 0, bp_vw_lo = 0, bp_vw_hi = 0;
#define DUO_BPLAN_TOT(org_) (reinterpret_cast<u32 *>(smem + dp.off_memo + DUO_MEMO_BYTES)[(org_) & 31u])
  // FLOOD TABLE: the wavefront starts from the context's table (see there) instead of an empty one: the records and the totals go from the
  // buffer to LDS as they lie there, 16 bytes a lane, the two masks come from its header.  The launch that makes the table starts empty.
  if constexpr (MEMO && DUO_TABLE_ON) {
    if (dp.table != nullptr && dp.table_fill == 0u) {
      DUO_LANE_NOW(tb_l);
      const uint4 *const tb_src = reinterpret_cast<const uint4 *>(dp.table + DUO_TABLE_HDR);
      uint4 *const tb_dst = reinterpret_cast<uint4 *>(smem + dp.off_memo);
      uint4 tb_v[3] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
#pragma unroll
      for (u32 k = 0; k < 3u; k++) if (tb_l + 64u * k < DUO_TABLE_COPY16) tb_v[k] = tb_src[tb_l + 64u * k];
#pragma unroll
      for (u32 k = 0; k < 3u; k++) if (tb_l + 64u * k < DUO_TABLE_COPY16) tb_dst[tb_l + 64u * k] = tb_v[k];
      mm_known = DUO_UNIFORM(dp.table[0]); mm_full = DUO_UNIFORM(dp.table[1]);
      wave_lds_fence();
    }
  }
  // a completed word is SEEN: a quiescent flood half of seen_m_ whose next_value is a multiple of 32 holds in sw the word its last value
  // has just completed, current in HBM; if that is the next word to count and it is all ones in all N node lanes, it is counted.  Called
  // wherever a steady half can stand at such a point: in front of the plan, where the loop takes a broadcast that opens a word, and behind
  // the loop (the round below may open the next word).  Two scalar tests per call unless a half stands at a boundary.
#ifdef DUO_BLOCK_PLAN_NO_FACTS
#define DUO_BPLAN_SEEN(seen_m_) do { } while (0)
#else
#define DUO_BPLAN_SEEN(seen_m_) do {                                                                                     \
    if constexpr (BPLAN) {                                                                                                \
      const u32 bs_v_lo = rdlane(next_value, 0), bs_v_hi = rdlane(next_value, 32);                                        \
      const bool bs_c_lo = (u32)(seen_m_) != 0 && bs_v_lo != 0 && (bs_v_lo & 31u) == 0 && bp_vw_lo + 1u == (bs_v_lo >> 5); \
      const bool bs_c_hi = (u32)((seen_m_) >> 32) != 0 && bs_v_hi != 0 && (bs_v_hi & 31u) == 0 && bp_vw_hi + 1u == (bs_v_hi >> 5); \
      if (bs_c_lo | bs_c_hi) {                                                                                            \
        const u64 bs_on = DUO_BAL_CMP(sw, ==, 0xFFFFFFFFu, 32);                                                           \
        if (bs_c_lo && (~(u32)bs_on & all_nodes) == 0) bp_vw_lo++;                                                        \
        if (bs_c_hi && (~(u32)(bs_on >> 32) & all_nodes) == 0) bp_vw_hi++;                                                \
      }                                                                                                                   \
    }                                                                                                                     \
  } while (0)
#endif
  // The helpers below are macros on purpose: as lambdas capturing the state by reference they left the closures (and with
  // them every captured variable) in scratch memory once the optimizer turned a select of two captured values into a select
  // of their addresses.
  // recv! took an envelope: (Thread/sleep (long dt)), net.clj:236-238
#define DUO_COMMIT_TIME(dl_) (LAT0 ? T : ((dl_) <= T ? T : T + (((dl_) - T) / 1000u) * 1000u))
#define DUO_RING_STORE(slot_, e_, dl_) do { if (LAT0) ring32[(slot_) * 32u] = (e_); else ring64[(slot_) * 32u] = (u64)(dl_) | ((u64)(e_) << 32); } while (0)
#define DUO_SEEN_WORD() DUO_SET(set_lane + ((cm & 0xFFE0u) << 2))   /* word (value >> 5) of the node's set */
  // slow, checked append: ring, then spill; used when a ring may fill up this round
#define DUO_PUSH_CHECKED(got_, e_, dl_) do {                                                                              \
    const bool pc_got = (got_); const u32 pc_e = (e_), pc_dl = (dl_);                                                     \
    if (RND) {   /* a bag: append with the node's arrival sequence number (orders equal deadlines like the ids do) */      \
      if (pc_got) {                                                                                                       \
        if (in_n < R) {   /* any free slot will do: a free slot's deadline is INF, `bag_used` says which ones are taken */      \
          const u32 pc_s = (u32)__builtin_ctz(~bag_used);                                                                 \
          BAGDL(pc_s) = pc_dl; BAGE(pc_s) = pc_e; BAGSEQ(pc_s) = (unsigned short)my_seq; bag_used |= 1u << pc_s; in_n++;  \
        }                                                                                                                 \
        else if (sp_n < S) {                                                                                              \
          my_spill12[3 * sp_n] = pc_dl; my_spill12[3 * sp_n + 1] = pc_e; my_spill12[3 * sp_n + 2] = my_seq & 0xFFFFu;     \
          if (sp_n == 0 || pc_dl < spm_dl) { spm_dl = pc_dl; spm_seq = my_seq & 0xFFFFu; spm_e = pc_e; spm_i = sp_n; }   /* (equal deadline: the older one stays) */ \
          sp_n++;                                                                                                         \
        }                                                                                                                 \
        else my_flags |= MSIM_FLAG_INBOX_OVERFLOW;                                                                        \
        my_seq++;                                                                                                         \
      }                                                                                                                   \
    } else {                                                                                                              \
      const bool pc_fit = (in_n < R) & (sp_n == 0);                                                                       \
      if (pc_got & pc_fit) {                                                                                              \
        DUO_RING_STORE((head + in_n) & Rm, pc_e, pc_dl);                                                                  \
        if (in_n == 0) { nx = pc_e; nx_dl = pc_dl; }                                                                      \
        in_n++;                                                                                                           \
      }                                                                                                                   \
      if (pc_got & !pc_fit) {                                                                                             \
        if (sp_n >= S) my_flags = (my_flags | MSIM_FLAG_INBOX_OVERFLOW) + (FLOOD ? DUO_DROP_ONE : 0u);   /* (FLOOD: the dropped envelopes are counted above the flag bits, see TRIM (A)) */ \
        else { u32 pc_idx = s_head + sp_n; if (pc_idx >= S) pc_idx -= S; DUO_MY_SPILL(pc_sp) pc_sp[pc_idx] = (u64)pc_dl | ((u64)pc_e << 32); sp_n++; } \
      }                                                                                                                   \
    }                                                                                                                     \
  } while (0)
  // idle receivers poll (net.clj:223-247): the minimum (deadline, id) = the FIFO head, or the client's request if its deadline
  // (its send time) is earlier; equal deadlines go to the envelope sent first, which is the queued server envelope.
  // Ends with the prefetch of the next head and of the set word of the (new) envelope.
#define DUO_POLL() do {                                                                                                   \
    const bool pl_idle = deliver_at == INF;                                                                               \
    if (RND) {                                                                                                            \
      /* recv! takes the minimum (deadline, id) of the bag — even if it is not due (net.clj:228-229) — and sleeps on it.  The 16      \
         deadlines of the LDS bag are read in one go (one wait) and reduced with 32-bit minima; only when the minimal deadline       \
         occurs twice (rare) do the arrival sequence numbers (16 bits, relative to the newest) decide. */                            \
      const bool pl_go = pl_idle & ((in_n | sp_n) != 0);                                                                  \
      if (__ballot(pl_go)) {                                                                                              \
        const u32 pl_sb = 32768u - my_seq;                                                                                \
        u32 pl_d[DUO_BAG];                                                                                                   \
        _Pragma("unroll") for (int pl_j = 0; pl_j < (int)DUO_BAG; pl_j++) pl_d[pl_j] = BAGDL(pl_j);   /* (free slots hold INF) */          \
        u32 pl_m[DUO_BAG / 2];                                                                                            \
        _Pragma("unroll") for (int pl_j = 0; pl_j < (int)(DUO_BAG / 2); pl_j++) pl_m[pl_j] = min(pl_d[pl_j], pl_d[pl_j + DUO_BAG / 2]);  \
        _Pragma("unroll") for (int pl_w = (int)(DUO_BAG / 4); pl_w >= 1; pl_w >>= 1)                                      \
          _Pragma("unroll") for (int pl_j = 0; pl_j < pl_w; pl_j++) pl_m[pl_j] = min(pl_m[pl_j], pl_m[pl_j + pl_w]);      \
        const u32 pl_dmin = pl_m[0];                                                                                      \
        u32 pl_bi = 0, pl_cnt = 0;                                                                                        \
        _Pragma("unroll") for (int pl_j = 0; pl_j < (int)DUO_BAG; pl_j++) { const bool pl_eq = pl_d[pl_j] == pl_dmin; pl_bi = pl_eq ? (u32)pl_j : pl_bi; pl_cnt += pl_eq ? 1u : 0u; } \
        u32 pl_bq = 0;   /* the winner's sequence number, relative; only read when it matters */                           \
        const bool pl_tie = pl_go & (in_n != 0) & ((pl_cnt > 1u) | (sp_n != 0 && spm_dl == pl_dmin));                      \
        if (__ballot(pl_tie)) {                                                                                           \
          if (pl_tie) {                                                                                                   \
            pl_bq = 0xFFFFFFFFu;                                                                                          \
            for (u32 pl_j = 0; pl_j < DUO_BAG; pl_j++) {                                                                      \
              if (BAGDL(pl_j) == pl_dmin) { const u32 pl_q = ((u32)BAGSEQ(pl_j) + pl_sb) & 0xFFFFu; if (pl_q < pl_bq) { pl_bq = pl_q; pl_bi = pl_j; } } \
            }                                                                                                             \
          }                                                                                                               \
        }                                                                                                                 \
        u32 pl_be = 0; bool pl_sp = false;                                                                                \
        /* the spilled part of the bag (HBM) takes part through its cached minimum: no memory access unless it wins */      \
        pl_sp = pl_go & (sp_n != 0) & ((in_n == 0) | (spm_dl < pl_dmin) | ((spm_dl == pl_dmin) & (((spm_seq + pl_sb) & 0xFFFFu) < pl_bq))); \
        if (pl_go) {                                                                                                      \
          if (!pl_sp) {   /* take it out of the LDS bag: its slot is free again */                                         \
            pl_be = BAGE(pl_bi);                                                                                          \
            BAGDL(pl_bi) = INF; bag_used &= ~(1u << pl_bi); in_n--;                                                       \
            cm = pl_be; deliver_at = DUO_COMMIT_TIME(pl_dmin);                                                            \
          } else { cm = spm_e; deliver_at = DUO_COMMIT_TIME(spm_dl); }                                                    \
        }                                                                                                                 \
        if (__ballot(pl_sp)) {   /* rare: a spilled envelope was taken — close the gap and find the new minimum of the spill */ \
          if (pl_sp) {                                                                                                    \
            sp_n--;                                                                                                       \
            if (spm_i != sp_n) { my_spill12[3 * spm_i] = my_spill12[3 * sp_n]; my_spill12[3 * spm_i + 1] = my_spill12[3 * sp_n + 1]; my_spill12[3 * spm_i + 2] = my_spill12[3 * sp_n + 2]; } \
            spm_dl = INF; u64 pl_mk = ~0ull;                                                                              \
            for (u32 pl_j = 0; pl_j < sp_n; pl_j++) {                                                                     \
              const u32 pl_d = my_spill12[3 * pl_j], pl_e2 = my_spill12[3 * pl_j + 1], pl_q = my_spill12[3 * pl_j + 2];   \
              const u64 pl_k = ((u64)pl_d << 20) | (u64)(((pl_q + pl_sb) & 0xFFFFu) << 4);                                \
              if (pl_k < pl_mk) { pl_mk = pl_k; spm_dl = pl_d; spm_seq = pl_q; spm_e = pl_e2; spm_i = pl_j; }             \
            }                                                                                                             \
          }                                                                                                               \
        }                                                                                                                 \
      }                                                                                                                   \
    } else if (LAT0) {                                                                                                    \
      const bool pl_can = pl_idle & (in_n != 0);                                                                          \
      cm = pl_can ? nx : cm; deliver_at = pl_can ? T : deliver_at;                                                        \
      head = (head + (pl_can ? 1u : 0u)) & Rm; in_n -= pl_can ? 1u : 0u;                                                  \
    } else {                                                                                                              \
      const u32 pl_hx = in_n != 0 ? nx_dl : INF;                                                                          \
      const bool pl_c = pl_idle & (have_creq != 0) & (creq_t < pl_hx);                                                    \
      const bool pl_r = pl_idle & !pl_c & (in_n != 0);                                                                    \
      const u32 pl_ex = pl_c ? creq_t : nx_dl;                                                                            \
      const u32 pl_e = pl_c ? creq : nx;                                                                                  \
      const u32 pl_t = DUO_COMMIT_TIME(pl_ex);                                                                            \
      cm = (pl_c | pl_r) ? pl_e : cm;                                                                                     \
      deliver_at = (pl_c | pl_r) ? pl_t : deliver_at;                                                                     \
      have_creq = pl_c ? 0u : have_creq;                                                                                  \
      head = (head + (pl_r ? 1u : 0u)) & Rm; in_n -= pl_r ? 1u : 0u;                                                      \
    }                                                                                                                     \
    if (!RND) {                                                                                                           \
      if (__ballot(sp_n != 0)) {   /* refill the ring from the spill: "ring empty" always means "queue empty" (rare) */    \
        DUO_MY_SPILL(pl_sp)                                                                                               \
        while (sp_n != 0 && in_n < R) {                                                                                   \
          const u64 pl_s = pl_sp[s_head];                                                                                 \
          s_head++; if (s_head >= S) s_head = 0; sp_n--;                                                                  \
          DUO_RING_STORE((head + in_n) & Rm, (u32)(pl_s >> 32), (u32)pl_s);                                               \
          in_n++;                                                                                                         \
        }                                                                                                                 \
      }                                                                                                                   \
      if (LAT0) { const u32 pl_h = ring32[head * 32u]; nx = (FLOOD && lane_in(fl_m)) ? nx : pl_h; }   /* (flood mode: the head entry stays in nx) */ \
      else { const u64 pl_h = ring64[head * 32u]; nx_dl = (u32)pl_h; nx = (u32)(pl_h >> 32); }                          \
    }                                                                                                                     \
    DUO_SW_PREFETCH();                                                                                                    \
  } while (0)
  // R3 for a broadcast envelope (gossip or the client's own): dedup against the node's set; pub_ = what the node publishes
  // to its neighbours: bit 31 | value | src to skip << 16, or 0; hball_ = the ballot of handle_, pubb_ = the ballot of pub_ != 0
  // (a half in flood mode keeps its set word in the register)
#define DUO_SW_PREFETCH() do { const u32 sl_w = DUO_SEEN_WORD(); sw = (FLOOD && lane_in(fl_m)) ? sw : sl_w; } while (0)
#define DUO_R3_SEEN(handle_, hball_, pub_, pubb_) do {                                                                    \
    const u32 r3_bit = 1u << (cm & 31u);                                                                                  \
    const bool r3_new = (handle_) & ((sw & r3_bit) == 0);                                                                 \
    pubb_ = (hball_) & bal((sw & r3_bit) == 0);                                                                           \
    if (r3_new) DUO_SEEN_WORD() = sw | r3_bit;                                                                           \
    pub_ = r3_new ? (0x80000000u | (cm & 0x3FFFFFu)) : 0u;                                                                \
    if (FLOOD) sw = r3_new ? (sw | r3_bit) : sw;                                                                          \
  } while (0)
  // ---- the flood bodies' parts (every live half in flood mode) ----
  // R3: the dedup from the register; the set word is written back later (see DUO_FLOOD_WB and TRIM (B): reads copy the sets from HBM)
#define DUO_FLOOD_R3(due_n_, due_b_, pub_, pubb_) do {                                                                    \
    const u32 fr_w = sw | (1u << (cm & 31u));                                                                             \
    const bool fr_new = (due_n_) & (fr_w != sw);                                                                          \
    pubb_ = (due_b_) & bal(fr_w != sw);                                                                                   \
    pub_ = fr_new ? (adj & ~(fan_skip << ((cm >> 16) & 31u))) : 0u;   /* the fan-out mask (see DUO_FLOOD_ARRIVALS) */           \
    sw = fr_new ? fr_w : sw;                                                                                              \
  } while (0)
  // TRIM (B): the write-back of sw by the lanes of wb_m_ (halves in flood mode), to the word of value next_value - 1
#define DUO_FLOOD_WB(wb_m_) do {                                                                                          \
    if (lane_in(wb_m_)) DUO_SET(set_lane + (((max(next_value, 1u) - 1u) & 0xFFE0u) << 2)) = sw;                           \
  } while (0)
  // COMMIT: the pulls of DUO_ARRIVALS; the arrivals are only counted, an empty queue's head entry is its first arrival
  // In the flood bodies a node publishes its FAN-OUT MASK, adj without the envelope's src (all of adj without skip-sender and
  // for the client's own broadcast; bit 31 is never set: lane 31 holds no node), not the envelope: the value is the flood's, the cluster's
  // next_value - 1, and need not travel.  "Neighbour k sends to me" is bit i of the word pulled from it; the arrivals are the number of
  // such k, and the first arrival's src is the lowest one's node number, from nbp.  The generic bodies keep the envelope format: the
  // publisher and the receivers of one wave-round are always in the same body, so the two formats never meet.
#define DUO_FLOOD_ARRIVALS(pub_) do {                                                                                     \
    const u32 fa_x[4] = {bperm(nbl[0], pub_), bperm(nbl[1], pub_), bperm(nbl[2], pub_), bperm(nbl[3], pub_)};             \
    const u32 fa_m = ((fa_x[0] >> i) & 1u) | (((fa_x[1] >> i) & 1u) << 8) | (((fa_x[2] >> i) & 1u) << 16) | (((fa_x[3] >> i) & 1u) << 24); \
    const u32 fa_src = (nbp >> (u32)__builtin_ctz(fa_m | 0x80000000u)) & 31u;   /* (no arrival: some number; nx means nothing while the queue stays empty) */ \
    nx = in_n == 0 ? ((next_value - 1u) | (fa_src << 16)) : nx;                                                           \
    in_n += (u32)__popc(fa_m); n_arr += (u32)__popc(fa_m);                                                                \
  } while (0)
  // the poll.  At latency 0 a node that holds an envelope has it due (deliver_at is the T of its commit or INF, and T never falls), so
  // after R3 every node is idle: the node takes the head of its queue if there is one.  No ring-head reload, no set-word prefetch.
#define DUO_FLOOD_POLL() do {                                                                                             \
    const bool fp_can = in_n != 0;                                                                                        \
    cm = fp_can ? nx : cm; deliver_at = fp_can ? T : INF; in_n = max(in_n, 1u) - 1u;   /* (one saturating subtraction) */ \
  } while (0)
  // leaving flood mode: the queued envelopes of every half in flood mode go to their ring (nx for each: see above); the fence orders
  // the stores before the reload of the ring head by the poll that follows
#define DUO_MATERIALISE() do {                                                                                            \
    if (FLOOD && fl_m != 0) {                                                                                             \
      PF_MAT_BEGIN                                                                                                        \
      const bool mt_on = lane_in(fl_m);                                                                                   \
      DUO_FLOOD_WB(fl_m);                                                                                                 \
      for (u32 mt_k = 0; __ballot(mt_on & (mt_k < in_n)); mt_k++)                                                         \
        if (mt_on & (mt_k < in_n)) ring32[((head + mt_k) & Rm) * 32u] = nx;                                               \
      wave_lds_fence();                                                                                                   \
      fl_m = 0;                                                                                                           \
      PF_MAT_END                                                                                                          \
    }                                                                                                                     \
  } while (0)
  // COMMIT of the fan-outs, receiver side: every node pulls what its neighbours publish, in ascending sender order (= id order,
  // net.clj:197), and appends it to its own queue.  got <=> the neighbour sends and does not skip this node:
  // z = (x & 0x803F0000) ^ (0x80000000 | me << 16) is > 0 exactly then (negative: not sending; 0: sending, skipping me).
  // RND: the message's id = the sender's first id of the round + the rank of this node in the sender's fan-out (ascending
  // destination, net.clj:197); its latency is drawn from the id (net.clj:178-187: uniform int in [0, 2 mean) or floor(mean * -ln u))
#define DUO_LAT_MS(r_) (lat_uniform ? scale32((r_), 2u * lat_mean) : (u32)(((u64)lat_mean * duo_neg_ln_q16((r_), log2_tab)) >> 16))
#define DUO_RND_DEADLINE(x_, base_, fanadj_, dl_) do {                                                                    \
    const u32 rd_src = ((x_) >> 16) & 63u;                                                                                \
    const u32 rd_fan = dp.echoback ? (fanadj_) : ((fanadj_) & ~(rd_src < 32u ? (1u << rd_src) : 0u));                      \
    const u32 rd_id = (base_) + __popc(rd_fan & lt);                                                                      \
    u32 rd_ms;                                                                                                            \
    if (lc_all) rd_ms = bperm(hbase4 + (((rd_id - lc_base) & 31u) << 2), lc);   /* the usual round: the draw is in the cluster's block */ \
    else rd_ms = DUO_LAT_MS(draw32(key, S_LATENCY, rd_id));                                                               \
    dl_ = T + rd_ms * 1000u;                                                                                              \
  } while (0)
#define DUO_ARRIVALS(pub_) do {                                                                                           \
    const u32 ar_dl = T + lat_us;                                                                                         \
    const u32 ar_zk = 0x80000000u | me16;                                                                                 \
    if (DEG4) {                                                                                                           \
      const u32 ar_x[4] = {bperm(nbl[0], pub_), bperm(nbl[1], pub_), bperm(nbl[2], pub_), bperm(nbl[3], pub_)};           \
      if (RND) {                                                                                                          \
        const u32 ar_b[4] = {bperm(nbl[0], pbase), bperm(nbl[1], pbase), bperm(nbl[2], pbase), bperm(nbl[3], pbase)};     \
        bool ar_g[4]; u32 ar_cnt = 0;                                                                                     \
        _Pragma("unroll") for (int ar_k = 0; ar_k < 4; ar_k++) { ar_g[ar_k] = (int)((ar_x[ar_k] & 0x803F0000u) ^ ar_zk) > 0; ar_cnt += ar_g[ar_k] ? 1u : 0u; } \
        n_arr += ar_cnt;                                                                                                  \
        if (!__ballot(ar_cnt > 1u)) {                                                                                     \
          /* the usual round: no node receives two envelopes — one latency draw serves every lane */                       \
          u32 ar_xx = 0, ar_bb = 0, ar_aa = 0, ar_cc = 0;                                                                 \
          _Pragma("unroll") for (int ar_k = 0; ar_k < 4; ar_k++) {                                                        \
            ar_xx = ar_g[ar_k] ? ar_x[ar_k] : ar_xx; ar_bb = ar_g[ar_k] ? ar_b[ar_k] : ar_bb;                             \
            ar_aa = ar_g[ar_k] ? nb_adj[ar_k] : ar_aa; ar_cc = ar_g[ar_k] ? DUO_KC(ar_k) : ar_cc;                             \
          }                                                                                                               \
          u32 ar_d; DUO_RND_DEADLINE(ar_xx, ar_bb, ar_aa, ar_d);                                                          \
          DUO_PUSH_CHECKED(ar_cnt != 0u, (ar_xx & 0xFFFFu) | ar_cc, ar_d);                                                \
        } else {                                                                                                          \
          _Pragma("unroll") for (int ar_k = 0; ar_k < 4; ar_k++) {                                                        \
            if (__ballot(ar_g[ar_k])) {                                                                                   \
              u32 ar_d; DUO_RND_DEADLINE(ar_x[ar_k], ar_b[ar_k], nb_adj[ar_k], ar_d);                                     \
              DUO_PUSH_CHECKED(ar_g[ar_k], (ar_x[ar_k] & 0xFFFFu) | DUO_KC(ar_k), ar_d);                                      \
            }                                                                                                             \
          }                                                                                                               \
        }                                                                                                                 \
      } else if (__builtin_expect(!__ballot((in_n + 4u > R) | (sp_n != 0)), 1)) {                                         \
        /* every ring has room for a full round of arrivals: plain stores at the tail, the count decides what stays; the     \
           tail runs unwrapped (head + in_n) and in_n is recovered from it once */                                        \
        const u32 ar_in0 = in_n;                                                                                          \
        u32 ar_s = head + in_n;                                                                                           \
        bool ar_g[4]; u32 ar_e[4];                                                                                        \
        _Pragma("unroll") for (int ar_k = 0; ar_k < 4; ar_k++) {                                                          \
          ar_g[ar_k] = (int)((ar_x[ar_k] & 0x803F0000u) ^ ar_zk) > 0;                                                     \
          ar_e[ar_k] = (ar_x[ar_k] & 0xFFFFu) | DUO_KC(ar_k);                                                                 \
          DUO_RING_STORE(ar_s & Rm, ar_e[ar_k], ar_dl);                                                                   \
          ar_s += ar_g[ar_k] ? 1u : 0u;                                                                                   \
        }                                                                                                                 \
        /* an empty ring's new head entry is its first arrival (nx means nothing while the ring stays empty) */          \
        const u32 ar_f = ar_g[0] ? ar_e[0] : ar_g[1] ? ar_e[1] : ar_g[2] ? ar_e[2] : ar_e[3];                             \
        nx = ar_in0 == 0 ? ar_f : nx; if (!LAT0) nx_dl = ar_in0 == 0 ? ar_dl : nx_dl;                                     \
        in_n = ar_s - head;                                                                                               \
        n_arr += in_n - ar_in0;                                                                                           \
      } else {                                                                                                            \
        _Pragma("unroll") for (int ar_k = 0; ar_k < 4; ar_k++) {                                                          \
          const bool ar_got = (int)((ar_x[ar_k] & 0x803F0000u) ^ ar_zk) > 0;                                              \
          n_arr += ar_got ? 1u : 0u;                                                                                      \
          DUO_PUSH_CHECKED(ar_got, (ar_x[ar_k] & 0xFFFFu) | DUO_KC(ar_k), ar_dl);                                             \
        }                                                                                                                 \
      }                                                                                                                   \
    } else {                                                                                                              \
      u32 ar_rem = adj;                                                                                                   \
      for (u32 ar_k = 0; ar_k < dp.deg; ar_k++) {                                                                         \
        const bool ar_has = ar_rem != 0;                                                                                  \
        const u32 ar_s = ar_has ? (u32)__builtin_ctz(ar_rem) : i;                                                         \
        ar_rem &= ar_rem - 1u;                                                                                            \
        const u32 ar_xx = bperm(hbase4 + (ar_s << 2), pub_);                                                              \
        const bool ar_got = ar_has & ((int)((ar_xx & 0x803F0000u) ^ ar_zk) > 0);                                          \
        u32 ar_d = ar_dl;                                                                                                 \
        if (RND) {                                                                                                        \
          const u32 ar_bb = bperm(hbase4 + (ar_s << 2), pbase);                                                           \
          const u32 ar_sadj = bperm(hbase4 + (ar_s << 2), adj);                                                           \
          if (__ballot(ar_got)) DUO_RND_DEADLINE(ar_xx, ar_bb, ar_sadj, ar_d);                                            \
        }                                                                                                                 \
        n_arr += ar_got ? 1u : 0u;                                                                                        \
        DUO_PUSH_CHECKED(ar_got, (ar_xx & 0xFFFFu) | (ar_s << 16), ar_d);                                                 \
      }                                                                                                                   \
    }                                                                                                                     \
  } while (0)
  // RND: ids of this round's sends in canonical order (node order; a node's fan-out in ascending destination, then its reply):
  // pbase = the node's first id; the cluster's id counter moves past all of them
#define DUO_RND_IDS(pub_, rep_) do {                                                                                      \
    const u32 id_src = (cm >> 16) & 63u;                                                                             \
    const u32 id_fan = (pub_) == 0 ? 0u : (dp.echoback ? adj : (adj & ~(id_src < 32u ? (1u << id_src) : 0u)));            \
    const u32 id_cnt = __popc(id_fan) + ((rep_) ? 1u : 0u);                                                               \
    const u32 id_incl = scan32(id_cnt);                                                                                   \
    pbase = next_id + id_incl - id_cnt;                                                                                   \
    const u32 id_lo = rdlane(id_incl, 31), id_up = rdlane(id_incl, 63);                                                   \
    const u32 id_first = next_id;                                                                                         \
    next_id += hi ? id_up : id_lo;                                                                                        \
    /* the latencies of the round's ids come from the cluster's block of 32 (lane i holds the one of id lc_base + i): a block that \
       does not reach the round's last id is drawn again from the round's first id on; a round of more than 32 sends draws its own */ \
    const bool id_rf = next_id - lc_base > 32u;                                                                           \
    if (__ballot(id_rf)) { const u32 id_nl = DUO_LAT_MS(draw32(key, S_LATENCY, id_first + i)); lc = id_rf ? id_nl : lc; lc_base = id_rf ? id_first : lc_base; } \
    lc_all = !__ballot(next_id - lc_base > 32u);                                                                          \
  } while (0)

#ifdef DUO_PROF   // developer build (tools/variant_lib.sh prof duo.hip -DDUO_PROF): wave-round counts and cycles of the two round bodies -> meta
  u64 pf_t0 = __builtin_readcyclecounter(), pf_gen = 0, pf_op = 0; u32 pf_ngen = 0, pf_nop = 0, pf_nwave = 0;
  u64 pf_it = 0, pf_fg = 0, pf_fop = 0, pf_mat = 0; u32 pf_nfg = 0, pf_nfop = 0, pf_nmat = 0;   // flood gossip rounds, flood op rounds, materialisations
  u32 pf_nrun = 0;   // reads of this lane's cluster that ran ahead of their wave-round's op (read runs)
  u64 pf_pk = 0; u32 pf_npark = 0, pf_npk = 0, pf_wmax = 0, pf_nop2 = 0;   // parked gossip rounds and their cycles, the parks, the longest wait, op wave-rounds that carried two ops
  u32 pf_nst = 0, pf_nstr = 0, pf_ngg = 0; u64 pf_gg = 0;   // flood stretches, the rounds taken inside them, generic gossip rounds and their cycles
  u32 pf_nquiet = 0;   // flood op rounds that took the quiet body (counted in pf_nfop as well)
  u32 pf_nspark = 0, pf_nsleave = 0; u64 pf_sx = 0; bool pf_sleft = false;   // steady parks (counted in pf_npark as well), steady leaves, the cycles of both from the stretch's exit on
  u32 pf_ndrop = 0;   // recordings dropped (the wavefront's): a half that acted, or met a GENERAL body, before the steady leave had taken its record
  u32 pf_nrec = 0, pf_nrep = 0, pf_nbout = 0;   // floods recorded (the wavefront's), floods replayed and broadcasts taken outside the quiet body (this lane's cluster's)
  u32 pf_nrunb = 0, pf_nit = 0;   // broadcasts of this lane's cluster taken in runs (counted in pf_nrep as well), iterations of the runs' loop (the wavefront's)
  u32 pf_nplan = 0, pf_nplanop = 0;   // block plans that took at least one op, the ops they took (the wavefront's; counted in pf_nrun / pf_nrunb as well: the loop's own are those less these)
  u64 pf_exit = 0;   // R0 and the exit test of the wave-rounds that leave the gossip loop (their op round or GENERAL body is counted from there on)
#define PF_MAT_BEGIN const u64 pf_m0 = __builtin_readcyclecounter();
#define PF_MAT_END pf_mat += __builtin_readcyclecounter() - pf_m0; pf_nmat++;
#else
#define PF_MAT_BEGIN
#define PF_MAT_END
#endif
#if defined(DUO_PROF2) || defined(DUO_PROF3)  // developer builds: cycles of the sections of the gossip round (PROF2) or of the GENERAL round (PROF3)
  u64 p2[8] = {0, 0, 0, 0, 0, 0, 0, 0}, p2_t = __builtin_readcyclecounter();   // -> meta of the wavefront's two instances (replaces DUO_PROF's numbers)
#define PX_MARK(i_) { const u64 p2_n = __builtin_readcyclecounter(); p2[i_] += p2_n - p2_t; p2_t = p2_n; }
#endif
#ifdef DUO_PROF2
#define P2_MARK(i_) PX_MARK(i_)
#else
#define P2_MARK(i_)
#endif
#ifdef DUO_PROF3
#define P3_MARK(i_) PX_MARK(i_)
#else
#define P3_MARK(i_)
#endif
  // the scheduler's view for the rounds to come (oracle: sched_resolve, sched_due): time-free phase transitions, the round limit, when
  // the scheduler acts next and which clusters have to run GENERAL rounds meanwhile; hbusy_b = bal(busy != 0)
#define DUO_SCHED_VIEW(hbusy_b_) do {                                                                                     \
    const u32 sv_hbusy = hi ? (u32)((hbusy_b_) >> 32) : (u32)(hbusy_b_);                                                  \
    for (;;) {                                                                                                            \
      bool sv_ch = false;                                                                                                 \
      if (lane_in(alive_m)) {                                                                                             \
        if (phase == PH_INIT_WAIT && sv_hbusy == 0) { phase = PH_TOPO; sv_ch = true; }                                    \
        if (phase == PH_TOPO_WAIT && sv_hbusy == 0) { phase = PH_MAIN_START; sv_ch = true; }                              \
        if (phase == PH_MAIN_START) { cutoff = T + p.cfg.time_limit_ms * 1000u; gen_next = T; phase = PH_MAIN; sv_ch = true; } \
        if (phase == PH_MAIN && !(rate > 0 && gen_next < cutoff) && !(rate == 0 && T < cutoff)) { phase = PH_DRAIN; sv_ch = true; } \
        if (phase == PH_DRAIN && sv_hbusy == 0) { phase = PH_SLEEP; sleep_until = T + p.cfg.quiesce_ms * 1000u; sv_ch = true; } \
        if (phase == PH_FINAL_WAIT && sv_hbusy == 0) { phase = PH_DONE; sv_ch = true; }                                   \
      }                                                                                                                   \
      if (!__ballot(sv_ch)) break;                                                                                        \
    }                                                                                                                     \
    alive_m &= ~bal(phase == PH_DONE);                                                                                    \
    const u64 sv_lim_b = alive_m & bal(rounds > round_limit);                                                             \
    flags |= lane_in(sv_lim_b) ? (u32)MSIM_FLAG_ROUND_LIMIT : 0u; alive_m &= ~sv_lim_b;                                   \
    const bool sv_gen_live = rate > 0 && gen_next < cutoff;                                                               \
    u32 sv_sa = INF;                                                                                                      \
    if (phase == PH_MAIN) {                                                                                               \
      if (sv_gen_live && (all_nodes & ~sv_hbusy) != 0) sv_sa = gen_next;                                                  \
      if (rate == 0) sv_sa = min(sv_sa, cutoff);                                                                          \
    } else if (phase == PH_INIT || phase == PH_TOPO || phase == PH_FINAL) sv_sa = T;                                      \
    else if (phase == PH_SLEEP) sv_sa = sleep_until;                                                                      \
    sched_at = lane_in(alive_m) ? sv_sa : INF;                                                                            \
    fg_m = alive_m & ~((rate > 0 ? bal(phase == PH_MAIN) & bal(gen_next < cutoff) : 0ull) | bal(phase == PH_SLEEP));      \
  } while (0)
  u32 mm_direct = 0;   // MEMO: the tail of an op round has done what leads to the next one (the direct way on); a scalar
  for (;;) {
    // the halves whose scheduler wants a GENERAL round, alive & (force_general | sched_at <= T): recomputed where its parts change (after a
    // GENERAL round, at a time jump, at the round limit); a gossip round adds the halves with a special envelope due
    u64 want_m = alive_m & (fg_m | bal(sched_at <= T));
    u64 op_m = 0, op_due = 0;   // LAT0: the halves that take an op round (see below; 0: the GENERAL body runs), the due envelopes
    // (MEMO: THE DIRECT WAY ON from the tail of an op round, see there: the next wave-round is the op round of both halves, nothing is due)
#ifdef DUO_PROF
    if (MEMO && mm_direct != 0) pf_it = __builtin_readcyclecounter();   // (no R0 and no exit test on the direct way: nothing goes to pf_exit)
#endif
    if (MEMO && mm_direct != 0) { op_m = ~0ull; mm_direct = 0; } else
    // ---- gossip rounds of both clusters, until one of them needs a GENERAL round ----
    for (;;) {
#ifdef DUO_PROF
      pf_nwave++; pf_it = __builtin_readcyclecounter(); bool pf_parked = park_m != 0;
#endif
      // R0: the cluster's time: stay at T while something is due, else jump to the next delivery / scheduler event.
      // Only looked at when one of the two clusters has nothing due (a scalar test on the halves of one ballot).
      P2_MARK(4)
      u64 due_b = bal(deliver_at <= T);   // (a mask, not a bool: a bool two paths define is turned into 0 / 1 and compared again)
      bool stuck_any = false;
      {
        // PAIRED OP ROUNDS: a parked half is quiescent with T at its sched_at: there is nothing for it in this block, so it counts as a half with
        // something due, and a parked round comes by here only when the partner has nothing due any more (its flood has ended) or the
        // wait has run out.  That is all a parked round adds to a gossip round: one scalar OR, the count-down and its test.  The parked
        // half is not in want_m meanwhile (see the exit test), so the round takes the gossip body; the block puts it back (T stands at
        // its sched_at), and the exit test releases it.
        const u64 db = FLOOD ? due_b | park_m : due_b;
        if (FLOOD) park_left--;
        if (__builtin_expect((u32)db == 0 || (u32)(db >> 32) == 0 || (FLOOD && park_left == 0), 0)) {
          {
          const u64 idle_b = alive_m & bal(sched_at > T) & hm2((u32)db == 0, (u32)(db >> 32) == 0);
          if (idle_b) {
            // latency 0: deliver_at is the T of the envelope's commit or INF, and T never falls, so a half with nothing due holds no
            // envelope at all: the next event is the scheduler's
            const u32 km = LAT0 ? sched_at : min(half_min(deliver_at, hi), sched_at);
            const u64 stuck_b = idle_b & bal(km == INF);   // nothing will ever happen (oracle: same flag, the round counts)
            const bool stuck = lane_in(stuck_b);
            flags |= stuck ? (u32)MSIM_FLAG_ROUND_LIMIT : 0u;
            sched_at = stuck ? INF : sched_at;
            rounds += stuck ? 1u : 0u;
            alive_m &= ~stuck_b; fg_m &= ~stuck_b; alive_v = stuck ? 0u : alive_v;
            if (FLOOD) sd_m &= ~stuck_b;
            T = lane_in(idle_b & ~stuck_b) ? km : T;
            stuck_any = stuck_b != 0;
            due_b = bal(deliver_at <= T);
          }
          // the round limit is looked at here and in GENERAL rounds (a stretch of pure gossip always ends in one of the two)
          // (not for a parked half: its round is counted, its op round decided; the limit is looked at again behind its op)
          fg_m |= alive_m & bal(rounds >= round_limit) & (FLOOD ? ~park_m : ~0ull);
          if (FLOOD) sd_m &= ~fg_m;
          want_m = alive_m & (fg_m | bal(sched_at <= T));
          }
        }
      }
      rounds += alive_v;
      const bool due_n = lane_in(due_b);
      // GENERAL if alive & (force_general | sched_at <= T | special), special = due_n & (cm >> 24) != DK_PLAIN
      if (const u64 gw_m = want_m | (alive_m & due_b & bal(cm > 0xFFFFFFu)); gw_m != 0 || stuck_any) {   // (a GENERAL round is a superset of a gossip round: harmless for the other cluster)
        // a parked half (below) is released here, whatever this round turns out to be; its round is not counted again
        bool released = false;
        if (FLOOD && park_m != 0) { alive_v = lane_in(park_m) ? 1u : alive_v; park_m = 0; park_left = PARK_IDLE; released = true; }
        bool parks = false;
        if (LAT0 && !RND && rate > 0 && !stuck_any) {
          // The steady state of latency 0: the scheduler acts right after its time jump, so the acting cluster is quiescent — no envelope
          // due (at latency 0 a node that holds one has it due), hence every node idle with an empty queue and every client free.  Its
          // generator's op is then all the cluster does this round: an op round.  Every half that wants a GENERAL round has to be in
          // that state (main phase, not forced, nothing due, no client busy, room for a value and two rows); else the GENERAL body runs.
          // (FLOOD: each of the five masks is one compare; as bal() they are five compares hoisted to the head of the outer loop and ten
          //  instructions here that turn the bools into masks again)
          u64 bz_b, st_m;
          if (FLOOD) {
            bz_b = DUO_BAL_CMP(busy, !=, 0u, 33);
            st_m = ~fg_m & DUO_BAL_CMP(phase, ==, PH_MAIN, 32) & DUO_BAL_CMP(next_value, <, max_values, 36) & DUO_BAL_CMP(n_rows + 2u, <=, max_rows, 37) & DUO_BAL_CMP(gen_k - dc_base, <, 32u, 36) &
                   hm2((u32)due_b == 0 && (u32)bz_b == 0, (u32)(due_b >> 32) == 0 && (u32)(bz_b >> 32) == 0);
          } else {
            bz_b = bal(busy != 0);
            st_m = ~fg_m & bal(phase == PH_MAIN) & bal(next_value < max_values) & bal(n_rows + 2u <= max_rows) & bal(gen_k - dc_base < 32u) &
                   hm2((u32)due_b == 0 && (u32)bz_b == 0, (u32)(due_b >> 32) == 0 && (u32)(bz_b >> 32) == 0);
          }
          op_m = (gw_m & ~st_m) == 0 ? gw_m : 0ull; op_due = due_b;
          // PAIRED OP ROUNDS.  The two clusters are independent, so the order in which they take their rounds is free, and an op wave-round
          // costs the wavefront the same whether it carries the op of one half or of both.  So when exactly one half wants a round, an op
          // round's, and its partner is alive (gw_m is a whole half, so nothing special is due anywhere; the partner does not want a
          // round, so at latency 0 it has envelopes due: it is in the middle of a flood), the ready half is PARKED: it leaves want_m, this
          // wave-round and the next ones take the gossip body, and R0's block (above) ends the wait when nothing is due at the partner
          // any more (its flood has ended: the block moves it to its own next op, or stops it, and this test chooses op_m from both halves
          // as ever) or after DUO_PAIR_WAIT wave-rounds (then the op goes alone).  A special envelope at the partner ends it here.
          // The invariant of a parked half: its round was counted by this iteration's R0 and alive_v is 0 for it until it is released
          // (above: after the releasing iteration's count), so rounds stays; T stands at its sched_at, and R0 leaves it there (sched_at
          // > T fails) and does not look at the round limit for it; it is quiescent (nothing held, nothing queued, no client busy),
          // so the flood and the generic gossip bodies do nothing for it: due is false in its lanes, it publishes nothing, pulls
          // nothing, the poll finds in_n == 0, and n_rsv, n_arr stay.  Nothing st_m looks at changes while it waits, so the releasing
          // test finds it eligible again.  Waiting is bounded twice: by the cap, and at latency 0 by the partner's flood, which handles
          // something in every round until it ends, within the topology's eccentricity + 2 rounds of its op.
          if (FLOOD && !released && op_m != 0 && alive_m == ~0ull && (gw_m == 0xFFFFFFFFull || gw_m == 0xFFFFFFFF00000000ull)) {
            park_m = gw_m; park_left = (u32)DUO_PAIR_WAIT; want_m &= ~gw_m; op_m = 0; parks = true;
            alive_v = lane_in(gw_m) ? 0u : alive_v;
#ifdef DUO_PROF
            pf_npark++; pf_parked = true; { const u64 pf_p0 = __builtin_readcyclecounter(); pf_exit += pf_p0 - pf_it; pf_it = pf_p0; }   // (R0 and the exit test of the parking round: with the leaving rounds')
#endif
          }
        }
        if (!parks) break;
      }
      if (FLOOD && (alive_m & ~fl_m) == 0) {
        // ---- FLOOD STRETCH: the flood gossip rounds of both clusters, one after the other, until something else than such a round is next.
        // This round is a flood gossip round: R0 and the exit test above have been through it.  What they would find in the NEXT one:
        //   * R0's block is entered exactly when a half has nothing due and is not parked, or the count-down reaches 0.  At latency 0 the
        //     poll leaves deliver_at = T in the lanes that took an envelope and INF in the others, and T stands outside the block, so the
        //     next round's due_b is this round's bal(in_n != 0), taken before the poll's decrement.  While both halves of that mask | park_m
        //     are non-zero and park_left is not about to reach 0, the block is not entered: T, sched_at, fg_m, alive_m, want_m and due_b
        //     stay what they are, stuck_any is false, and the round limit, which only that block looks at, is not looked at.
        //   * the exit test's gw_m is want_m, which is 0 here (else this round had left or parked: a parked half is out of want_m), or a
        //     special envelope due.  THE FLOOD INVARIANT: a half in flood mode holds DK_PLAIN envelopes only (nx is value | src << 16 with
        //     src < 32, whichever body set it), and every live half is in flood mode here, so no special envelope can be due (a build
        //     with -DDUO_PROF, or for the host emulator, asserts it).  fl_m and alive_m change in op rounds and GENERAL bodies only.
        // So the next round is again a flood gossip round, and all it needs of this one is the mask of the lanes with something due: the
        // loop carries that mask, cm, nx, in_n, sw and the two counters, and its back edge tests the two halves and the count-down.
        // deliver_at is not kept inside: on leaving it is T where the mask is set and INF elsewhere, what the polls would have left.
        // rounds gets the rounds of the stretch at once (alive_v each: 0 for a parked or finished half, as in R0), park_left goes down by
        // one per round.  The round that ends the stretch is not begun here: it enters the loop at its head, as ever, with the state R0
        // expects, so the limit is looked at, the time moved, a half parked or released at the very rounds it was before.
        // A half that is finished (or holds no cluster) is NOT counted as a half with something due, although R0's block does nothing FOR
        // it: the block also looks at the round limit of its live partner, in every round of such a wavefront, and so stops that partner
        // at rounds == round_limit exactly; a stretch over those rounds would stop it later (the one-cluster round-limit sweep of
        // tests/test_duo_op_plan_hipemu.py sees the difference).  A wavefront with one live cluster therefore takes its rounds one by one.
        u64 st_due = due_b; u32 st_more = 0;
#ifdef DUO_PROF
        pf_nst++;
#endif
        // (a steady park comes back to this wrapper with `continue`; every other stretch passes it once and leaves by the `break` at its
        //  end.  THE CONVENTION BELOW IS OFF BY ONE ON PURPOSE: the stretch's exit keeps park_left and st_more as the loop's last
        //  park_left-- and st_more++ left them, i.e. with the NEXT round's count-down and count already taken, and the steady leave is
        //  written on those values (park_left against 0, sl_r1 = rounds with the next round counted, round_limit < sl_r1); where it declines
        //  it takes both back (park_left++, rounds = sl_r1 - alive_v) so that the loop's head finds what it expects, and the -DDUO_PROF
        //  counters allow for it too (pf_wmax).  Written on the values after `park_left++; st_more--` instead, the compiler kept wrapper
        //  and stretch as two loops and closed the inner one with s_mov + s_branch: a taken branch more on every round's back edge
        //  (profiles/r31_isa_static.txt).  Whoever changes one of these places changes all of them.)
        for (;;) {
        for (;;) {
          const bool st_n = lane_in(st_due);
#if defined(DUO_PROF) || defined(MSIM_HIPEMU)
          if (st_n && lane_in(alive_m) && cm > 0xFFFFFFu) __builtin_trap();   // the flood invariant
#endif
          u32 pub; u64 pub_b; DUO_FLOOD_R3(st_n, st_due, pub, pub_b);
          if (pub_b) DUO_FLOOD_ARRIVALS(pub);
          st_due = bal(in_n != 0);   // the poll (DUO_FLOOD_POLL without deliver_at): whoever has a queue takes its head
          const bool st_can = lane_in(st_due);
          cm = st_can ? nx : cm; in_n = max(in_n, 1u) - 1u;   /* (one saturating subtraction) */
          // the back edge: the head of the next round (its count-down, its count) and the test that would send it into R0's block
          const u64 st_db = st_due | park_m;
          park_left--; st_more++;
          if (min((u32)st_db, (u32)(st_db >> 32)) == 0 || park_left == 0) break;
#ifdef DUO_PROF
          pf_nwave++;
#endif
        }
        // (the round that ends the stretch begins at the loop's head: its count-down and its count are taken there; they are what the steady
        //  leave needs, and are taken back where it declines, so that the back edge above keeps its one value of each)
#ifdef DUO_PROF
        // one reading per stretch (one per round cost a round of this loop more than the round itself); a half is parked or released at the
        // exit test only, so a stretch is parked as a whole or not at all
        { const u64 pf_s1 = __builtin_readcyclecounter();   // (the steady leave is counted from here)
          // (st_more and park_left stand with the next round's count and count-down taken: the wait so far is one round less than it looks)
          if (pf_parked) { pf_pk += pf_s1 - pf_it; pf_npk += st_more; pf_wmax = max(pf_wmax, (u32)DUO_PAIR_WAIT - park_left); }
          else { pf_fg += pf_s1 - pf_it; pf_nfg += st_more; }
          pf_nstr += st_more;
          pf_it = pf_s1; }
#endif
        deliver_at = lane_in(st_due) ? T : INF;
        // STEADY LEAVE.  The round that is next begins at the loop's head, and when the stretch ended because a half has run dry (dry_m: no
        // lane of it has something due, and it is not parked), nearly all that R0's block and the exit test do there is to find out again
        // what the half's last op round left behind.  With both halves alive, the count-down not about to run out (the head's park_left--
        // and its test), every dry half steady (sd_m & ~fg_m, see sd_m) and no unparked half at the round limit (ONE compare over both
        // halves: R0's block looks at the live partner's limit too, whenever it is entered), the answers are known:
        //   * want_m is 0 inside a stretch, so sched_at > T in both halves, and a dry half at latency 0 holds nothing (deliver_at == INF),
        //     so the block's idle_b is dry_m, km is sched_at, which an op round's tail set to gen_next (never INF: nobody is stuck), and
        //     T moves to it; due_b stays st_due; fg_m gets nothing from the limit; want_m becomes the dry halves and a parked one;
        //   * rounds += alive_v, and gw_m is want_m: the flood invariant rules out a special envelope at the partner;
        //   * st_m holds in the dry halves by sd_m, and in a parked half because nothing it looks at has changed since the test that
        //     parked it (see PAIRED OP ROUNDS).
        // So the head would either PARK the dry half (its partner still has envelopes due and is not parked: gw_m is one half) and come
        // back to this loop with st_due as it is, or, with dry_m | park_m covering both halves, release the parked half and LEAVE for an
        // op round of both (op_m = ~0, op_due = 0: the quiet body by its own test).  Exactly that is done here, and nothing else: the same
        // time jump, round count and count-down at the same round, the same park_m, park_left and alive_v (the stretch's last park_left--
        // and st_more++ ARE that round's count-down and count: sl_r1 is rounds with that round counted, so the limit test reads
        // round_limit < sl_r1, and park_left is tested against 0; where the path declines both are taken back).  Everything else (a dry half
        // that is not steady, a finished or absent partner, the count-down at 0, the limit reached) goes to the loop's head as ever,
        // where R0's block is entered by the same test that ended the stretch and rebuilds want_m.  No round, delivery or message is
        // skipped or batched: this removes tests.  All of it sits behind the stretch's exit; the back edge above is untouched.
        {
          const u64 dry_m = ~park_m & hm2((u32)st_due == 0, (u32)(st_due >> 32) == 0);
          const u32 sl_r1 = rounds + st_more * alive_v;   // the stretch's rounds and the next round's count
          if (alive_m == ~0ull && park_left != 0u && dry_m != 0 && (dry_m & ~(sd_m & ~fg_m)) == 0 &&
              (~park_m & DUO_BAL_CMP(round_limit, <, sl_r1, 36)) == 0) {
#if defined(DUO_PROF) || defined(MSIM_HIPEMU)
            {   // the steady invariant: what R0's block and the exit test would have found
              const bool sl_dry = lane_in(dry_m), sl_op = lane_in(dry_m | park_m);
              if (sl_op && ((in_n | sp_n | busy) != 0 || deliver_at != INF)) __builtin_trap();
              if (sl_dry && (sched_at <= T || sched_at == INF)) __builtin_trap();
              if (!sl_op && lane_in(st_due) && cm > 0xFFFFFFu) __builtin_trap();
              if (sl_op && (lane_in(fg_m) || phase != PH_MAIN || next_value >= max_values || n_rows + 2u > max_rows || gen_k - dc_base >= 32u)) __builtin_trap();
              if ((dry_m & st_due) != 0 || (park_m & st_due) != 0) __builtin_trap();
            }
#endif
            if constexpr (MEMO) {
              // FLOOD MEMO: a recording half is dry and steady: its flood is over, what it did becomes the record of its origin
              if (const u64 mm_fin = mm_rec & dry_m) {
                DUO_LANE_NOW(mf_l);
                u32 mf_e = 0;
                if (lane_in(mm_fin)) {
                  const u32 mf_org = (mm_org >> ((mf_l >> 5) << 3)) & 31u;
                  const u32 mf_b = DUO_MEMO_AT(mf_org, mf_l);
                  mf_e = ((n_arr - mf_b) & 0x7Fu) | (((sw >> ((next_value - 1u) & 31u)) & 1u) << 7) | (((sl_r1 - 1u - (mf_b >> 8)) & 0xFFu) << 8);
                  DUO_MEMO_AT(mf_org, mf_l) = (unsigned short)mf_e;
                }
                if constexpr (BPLAN) {   // BLOCK PLAN: the record's sum over the half and whether every node lane has the value's bit
                  const u32 mf_s = scan32(mf_e & 0x7Fu);
                  const u64 mf_b7 = bal((mf_e & 0x80u) != 0);
                  if ((u32)mm_fin) {
                    const u32 mf_t = rdlane(mf_s, 31) | ((rdlane(mf_e, 0) >> 8) << 16);
                    if (mf_l == 0u) DUO_BPLAN_TOT(mm_org & 31u) = mf_t;
                    if ((~(u32)mf_b7 & all_nodes) == 0) mm_full |= 1u << (mm_org & 31u);
                  }
                  if ((u32)(mm_fin >> 32)) {
                    const u32 mf_t = rdlane(mf_s, 63) | ((rdlane(mf_e, 32) >> 8) << 16);
                    if (mf_l == 32u) DUO_BPLAN_TOT((mm_org >> 8) & 31u) = mf_t;
                    if ((~(u32)(mf_b7 >> 32) & all_nodes) == 0) mm_full |= 1u << ((mm_org >> 8) & 31u);
                  }
                }
                if ((u32)mm_fin) mm_known |= 1u << (mm_org & 31u);
                if ((u32)(mm_fin >> 32)) mm_known |= 1u << ((mm_org >> 8) & 31u);
                mm_rec &= ~mm_fin;
                wave_lds_fence();   // (the other half may read the row in its next op round)
#ifdef DUO_PROF
                pf_nrec += ((u32)mm_fin ? 1u : 0u) + ((u32)(mm_fin >> 32) ? 1u : 0u);
#endif
              }
            }
            T = lane_in(dry_m) ? sched_at : T;
            rounds = sl_r1;
#ifdef DUO_PROF
            pf_nwave++;
#endif
            if ((dry_m | park_m) == ~0ull) {   // leave: both halves take their op
              if (park_m != 0) { alive_v = 1u; park_m = 0; park_left = PARK_IDLE; }   // (the parked half's round is not counted again; both halves are alive)
              op_m = ~0ull; op_due = 0;
#ifdef DUO_PROF
              pf_nsleave++; pf_sleft = true;
#endif
            } else {   // park: the dry half waits for its partner's flood
              park_m = dry_m; park_left = (u32)DUO_PAIR_WAIT; alive_v = lane_in(dry_m) ? 0u : alive_v; st_more = 0;
#ifdef DUO_PROF
              pf_npark++; pf_nspark++; pf_parked = true; { const u64 pf_p0 = __builtin_readcyclecounter(); pf_sx += pf_p0 - pf_it; pf_it = pf_p0; }
#endif
              continue;
            }
          } else { park_left++; rounds = sl_r1 - alive_v; }
        }
        break;
        }
        if (op_m != 0) break;   // (a steady leave: op_m is 0 wherever else this point is reached, a parking exit test included)
      } else {   // ---- a round in which both clusters only gossip ----
        P2_MARK(0)
        u32 pub; u64 pub_b; DUO_R3_SEEN(due_n, due_b, pub, pub_b);
        deliver_at = due_n ? INF : deliver_at;
        if (!FLOOD) n_rsv += due_n ? 1u : 0u;
        P2_MARK(1)
        if (pub_b) {
          if (RND) DUO_RND_IDS(pub, false);
          P2_MARK(2)
          DUO_ARRIVALS(pub);
        }
        P2_MARK(3)
        DUO_POLL();
#ifdef DUO_PROF
        if (pf_parked) { pf_pk += __builtin_readcyclecounter() - pf_it; pf_npk++; pf_wmax = max(pf_wmax, (u32)DUO_PAIR_WAIT + 1u - park_left); }
        else { pf_gg += __builtin_readcyclecounter() - pf_it; pf_ngg++; }   // (the generic gossip rounds, counted directly: -DDUO_PROF_STRETCH reports them)
#endif
      }
    }
    if (!alive_m) break;
#ifdef DUO_PROF
    const u64 pf_a = __builtin_readcyclecounter();
    if (pf_sleft) { pf_sx += pf_a - pf_it; pf_sleft = false; } else pf_exit += pf_a - pf_it;   // (a steady leave's cycles: from the stretch's exit)
#endif
    if (LAT0 && !RND && op_m != 0) {
      // ---- an op round: the gossip round of both clusters, plus the op of each cluster in op_m.  It computes what the GENERAL body
      //      computes for such a cluster: every worker is free, so the pick is the node of that rank, and it is idle, so its recv! takes
      //      the request at once and the node completes it in this round (busy goes 1 -> 0 within the round) ----
      const bool opn = lane_in(op_m);
      if constexpr (MEMO) {
#ifdef DUO_PROF
        pf_ndrop += ((u32)(mm_rec & op_m) ? 1u : 0u) + ((u32)((mm_rec & op_m) >> 32) ? 1u : 0u);
#endif
        mm_rec &= ~op_m;   // a half that acts without having come by the steady leave's record: the recording is dropped (see FLOOD MEMO)
        if constexpr (DUO_MEMO_CHECK) {
          if (vf_m & op_m) {   // the simulated flood against its record: the rises, the leaving round, the end state
            if (lane_in(vf_m & op_m) && (n_arr - vf_n0 != (vf_e & 0x7Fu) || rounds - vf_r0 != (vf_e >> 8) + 1u || in_n != 0 || deliver_at != INF ||
                                         ((sw >> vf_bit) & 1u) != ((vf_e >> 7) & 1u))) __builtin_trap();
            vf_m &= ~op_m;
          }
        }
      }
      DUO_UPM_NOW();   // TRIM (C)
      if (FLOOD && (op_m & fl_m) != 0) DUO_FLOOD_WB(op_m & fl_m);   // TRIM (B): the read runs, the read op's copy read the sets from HBM
      // READ RUNS.  An acting cluster is quiescent, and a read leaves it so: the picked node copies its set to the payload, two rows
      // appear, and the cluster's next round is its generator's next op.  While the op at hand is a read AND the op after it will
      // again be an op round's (its draw is in the cluster's block, it falls before the cutoff, its rows and this read's payload fit,
      // the round limit is not reached: what the exit test and the scheduler's view would find), the read is executed here, as a
      // cluster round of its own: rows at its own time, the payload from the set of its own node, then the time jump to the next op
      // and the round count.  The op that ends the run (a broadcast, or the last read before one of the conditions fails) is the op
      // of the round below, so a run of k reads and the broadcast behind it cost the wavefront one wave-round instead of k + 1; the
      // other half gets its one gossip round from it either way.
      // What the condition leans on: next_value < max_values was checked by st_m when this op round was chosen, and a read does not
      // change next_value; the payload of the op that ENDS the run is checked by the round below (its overflow flag and all); DUO_DRAW
      // masks its index with 31, so a lane of a half that does not act reads some draw of the block and never outside it; and the three
      // places that look at the round limit agree: a read runs ahead only while rounds < round_limit, which is exactly when R0 of the
      // cluster's next round would not force a GENERAL round (rounds >= round_limit) and the scheduler's view would not stop it (>).
      // STEADY RUN (the memo instantiation).  A broadcast whose flood is remembered is as cheap as a read: two rows, next_value, the set word's
      // bit and the recorded rises.  So the loop takes it as a cluster round too, and a half goes from one block of 32 draws to the next
      // inside the loop: the quiet body, the tail, the head and the write-back (B) are paid once per block, not once per op.  A half's op
      // at hand is taken if it is
      //   (a) a read, under the read runs' conditions, unchanged; or
      //   (b) a broadcast, in an op wave-round that is `quiet` at entry (fl_ok, every live half acts, all in flood mode: the replay's own
      //       precondition; sr_m), from an origin in mm_known, whose op after it is again an op round's: its draw is in the block (k < 31),
      //       T < next < cutoff (no op of the half's own scheduler could have met the flood in mid-run), rows for both ops, and a value
      //       left for the op after (st_m's term: a broadcast moves next_value), and with every live half FAR from the round limit: rounds +
      //       DUO_SRUN_FAR < round_limit, tested once per op round.  One run adds at most 31 x (255 + 1) rounds to a half, so no look at the
      //       limit, the half's own or its partner's, could have found anything in any round the run stands for; under a low
      //       MSIM_DUO_ROUND_LIMIT the run takes reads only and the limit is found where it always was.
      // A broadcast's iteration does for its half what the quiet body's steps 1, 3, 4, the replay and the direct way on do: the pick, n_cl,
      // gen_k, next_value, the two rows at T, the set word (0 where the value opens a word; the record's bit, which the picked node's own
      // lane carries as well: its record was taken from an sw with the bit set), n_arr and rounds by the record, then T = next and the next
      // round's count.  A half's rounds do not depend on its partner's (a parked round is the one the direct way on counts), so the two halves
      // take their iterations independently.  gen_next and sched_at are set by the op that ends the run, in the round below, as for reads.
      // Whatever else the op at hand is (an origin not remembered, the block's last draw, the cutoff, a capacity) ends that half's run and is
      // the op of the round below, as before.  A recording cannot be open here: the head has dropped those of the acting halves.
      // THE SETS.  Reads copy from HBM, and inside a run sw can be newer than HBM (sr_dirty, a scalar mask of whole halves): a read's
      // iteration writes sw back first (it sees the bits of the broadcasts before it), a broadcast that opens a word writes the completed
      // word back before sw is reset, and the run's end leaves nothing dirty for the round below.
      if constexpr (SRUN) {
        u64 sr_m = 0, sr_dirty = 0;
        if (fl_ok && (alive_m & ~op_m) == 0 && (op_m & ~fl_m) == 0 && (alive_m & ~DUO_BAL_CMP(rounds + DUO_SRUN_FAR, <, round_limit, 36)) == 0) sr_m = op_m;
        // BLOCK PLAN.  What the loop below does op after op is closed-form over the block of draws: op k + 1 depends on op k through prefix
        // sums alone (the time, the values, the rows, the payload, the rounds).  So in front of the loop lane k of a half in sr_m reads draw k
        // of the block (k0 = gen_k - dc_base <= k < 31), scans give it its op's time, value count, row index and payload offset as they stand
        // if every op before it is taken, and it tests on them EXACTLY what the loop tests on its op: k < 31, next < cutoff, n_rows + 4 <=
        // max_rows; for a read the payload's room (rounds < round_limit follows from sr_m's FAR term: a block adds less than DUO_SRUN_FAR);
        // for a broadcast an origin in mm_full, T < next and next_value + 1 < max_values.  The plan takes the longest prefix [k0, m) of ops
        // that all pass (a ballot, its trailing ones) and commits it at once; op m and all behind it are the loop's and the round's below,
        // on the state the loop would have left there, so every stop is found where it always was.
        // THE SETS.  A planned read does not copy its node's set, it writes what that set must hold: inside a quiet run every node has taken
        // every value in, so a set is all ones up to a last, partial word.  That is not assumed.  A half plans only while, checked,
        //   * every completed word of its sets was SEEN to be all ones in all N node lanes: bp_vw_lo / bp_vw_hi count the leading words seen
        //     so (DUO_BPLAN_SEEN), where an acting flood half stands at next_value a multiple of 32 with the completed word in sw, current in
        //     HBM: in front of the plan, behind the loop, where the loop opens a word, and where a plan completes one in its middle; a word
        //     completed anywhere else is counted later, one per op wave-round, from what the lanes themselves wrote back to HBM;
        //   * sw is the same in all N node lanes (one compare against the half's first lane), so one scalar per half is every node's word;
        //   * the origin's record has the value's bit in all N node lanes (mm_full, filled where mm_known is).
        // A half for which one of these fails takes the loop for the block, whose result is the parent's by construction.  With them, a
        // payload word is all ones unless it is the last word of a read whose value count is no multiple of 32; that word is the half's sw
        // at entry (if the read's count lies in the entry word) with the bits of the block's broadcasts before the read.  Each word's value
        // is built before it is stored, one store per word.  A word completed inside the plan is written back, all ones, before sw starts
        // the next one, and the block's end leaves sw dirty for the loop's own write-backs (sr_dirty), as a broadcast's iteration does.
        // THE SUMS.  n_cl and n_arr are read by the epilogue alone, as sums over the half (n_arr also by a recording, as a lane's own rise
        // while its half simulates, which no plan falls into).  So the lane that plans an op counts its pick, and the lane that plans a
        // broadcast adds the whole half's rise: DUO_BPLAN_TOT(origin), the record's sum over the lanes, kept beside the record (one LDS
        // read per lane, no loop over broadcasts or origins: of per broadcast, per distinct origin and per origin at the run's end, each of
        // which walks the block's ~15 broadcasts with a table row read per lane, this costs one read and one add per plan).
        if constexpr (BPLAN) {
          DUO_LANE_NOW(bp_l);
          const u32 bp_i = bp_l & 31u;
          const bool bp_up = bp_l >= 32u;
          const u32 bp_v_lo = rdlane(next_value, 0), bp_v_hi = rdlane(next_value, 32);
          const u32 bp_s_lo = rdlane(sw, 0), bp_s_hi = rdlane(sw, 32);
          const u32 bp_sh = bp_up ? bp_s_hi : bp_s_lo;   // the half's set word: every node lane's, once checked
          const u64 bp_un = DUO_BAL_CMP(sw, ==, bp_sh, 32);
          bool bp_u_lo = (~(u32)bp_un & all_nodes) == 0, bp_u_hi = (~(u32)(bp_un >> 32) & all_nodes) == 0;
#ifdef DUO_BLOCK_PLAN_NO_FACTS
          bp_u_lo = false; bp_u_hi = false;
#endif
          DUO_BPLAN_SEEN(op_m & fl_m);   // (B) has written their sw back
#ifndef DUO_BLOCK_PLAN_NO_FACTS
          // A half whose count lags (a word was completed where nobody looked: a GENERAL body, a generic op round) catches up one word per
          // op wave-round, from HBM: word bp_vw of an acting flood half lies below the word sw stands for, so its lanes wrote it back
          // before sw moved on and nothing writes it again; each lane loads its own column's word, the one it stored itself.
          if (const u64 bp_lag = op_m & fl_m & hm2(bp_vw_lo < (bp_v_lo >> 5), bp_vw_hi < (bp_v_hi >> 5))) {
            u32 bp_lw = 0xFFFFFFFFu;
            if (lane_in(bp_lag)) bp_lw = DUO_SET(set_lane + (bp_up ? bp_vw_hi : bp_vw_lo) * 128u);
            const u64 bp_lon = DUO_BAL_CMP(bp_lw, ==, 0xFFFFFFFFu, 32);
            if ((u32)bp_lag && (~(u32)bp_lon & all_nodes) == 0) bp_vw_lo++;
            if ((u32)(bp_lag >> 32) && (~(u32)(bp_lon >> 32) & all_nodes) == 0) bp_vw_hi++;
          }
#endif
          const u64 bp_m = sr_m & hm2(bp_u_lo && bp_vw_lo == (bp_v_lo >> 5), bp_u_hi && bp_vw_hi == (bp_v_hi >> 5));
          if (bp_m) {
            const u64 bp_d = DUO_DCL_MINE();
            const u32 bp_lo = (u32)bp_d, bp_k0 = gen_k - dc_base;
            const bool bp_val = lane_in(bp_m) && bp_i >= bp_k0 && bp_i < 31u;
            const u32 bp_dt = bp_val ? __umulhi((u32)(bp_d >> 32), p.gen_period2_us) : 0u;
            const bool bp_rd = (bp_lo & 1u) != 0;
            const u32 bp_node = scale32(bp_lo, N);
            const bool bp_kn = ((mm_full >> bp_node) & 1u) != 0;
            const u32 bp_b1 = bp_val && !bp_rd ? 1u : 0u;
            // (inclusive scans inside the half; a lane outside [k0, 31) adds nothing, so its own figures are the sums of those below it)
            const u32 bp_next = T + scan32(bp_dt);
            const u32 bp_T = bp_next - bp_dt;
            const u32 bp_v = next_value + scan32(bp_b1) - bp_b1;
            const u32 bp_w = (bp_v + 31u) >> 5;
            const u32 bp_pw = bp_val && bp_rd ? bp_w : 0u;
            const u32 bp_po = n_payload + scan32(bp_pw) - bp_pw;
            u32 bp_e = 0;
            if (bp_b1 != 0 && bp_kn) bp_e = DUO_BPLAN_TOT(bp_node);
            const u32 bp_es = scan32(bp_e) - bp_e;
            const u32 bp_row = n_rows + 2u * (bp_i - bp_k0);
            const bool bp_ok = bp_val && bp_next < cutoff && bp_row + 4u <= max_rows &&
                               (bp_rd ? bp_po + bp_w <= max_pay : (bp_kn && bp_T < bp_next && bp_v + 1u < max_values));
            const u64 bp_okb = bal(bp_ok), bp_bcb = bal(bp_b1 != 0);
            // per half, on the scalar unit: m, the lanes taken, their broadcasts; a word completed in mid-plan must come out all ones
#define DUO_BP_HALF(h_, l0_, okb_, bcb_)                                                                                  \
            const u32 bp_k_##h_ = min(rdlane(bp_k0, l0_), 31u);                                                          \
            u32 bp_m_##h_ = (u32)__builtin_ctz(~((okb_) | ((1u << bp_k_##h_) - 1u)));                                    \
            u32 bp_nb_##h_ = (u32)__popc((bcb_) & ((1u << bp_m_##h_) - 1u) & ~((1u << bp_k_##h_) - 1u));                 \
            bool bp_x_##h_ = bp_nb_##h_ != 0 && (bp_v_##h_ & 31u) != 0 && ((bp_v_##h_ + bp_nb_##h_ - 1u) >> 5) != (bp_v_##h_ >> 5); \
            if (bp_x_##h_ && (bp_s_##h_ | ~((1u << (bp_v_##h_ & 31u)) - 1u)) != 0xFFFFFFFFu) { bp_m_##h_ = bp_k_##h_; bp_nb_##h_ = 0; bp_x_##h_ = false; } \
            const u32 bp_tk_##h_ = ((1u << bp_m_##h_) - 1u) & ~((1u << bp_k_##h_) - 1u);                                 \
            const u32 bp_c_##h_ = bp_m_##h_ - bp_k_##h_;                                                                 \
            const bool bp_o_##h_ = bp_nb_##h_ != 0 && ((bp_v_##h_ & 31u) == 0 || bp_x_##h_);                             \
            const u32 bp_g_##h_ = bp_nb_##h_ == 0 ? 0u : ((2u << ((bp_v_##h_ + bp_nb_##h_ - 1u) & 31u)) - 1u) & ~(bp_o_##h_ ? 0u : (1u << (bp_v_##h_ & 31u)) - 1u);
            DUO_BP_HALF(lo, 0, (u32)bp_okb, (u32)bp_bcb)
            DUO_BP_HALF(hi, 32, (u32)(bp_okb >> 32), (u32)(bp_bcb >> 32))
#undef DUO_BP_HALF
            const u64 bp_tk = (u64)bp_tk_lo | ((u64)bp_tk_hi << 32);
            if (bp_tk) {
              const bool bp_t = lane_in(bp_tk);
              if (bp_t) {   // the op's two rows, from the lane that planned it
                const u64 tns = (u64)bp_T * 1000ull;
                const u32 tlo = (u32)tns, thi = (u32)(tns >> 32);
                const u32 fk = bp_rd ? (u32)MSIM_F_READ : (u32)MSIM_F_BROADCAST;
                DUO_ROW(bp_row) = make_uint4(tlo, thi, MSIM_T_INVOKE | (fk << 2) | (bp_node << 12), bp_rd ? MSIM_NO_VALUE : bp_v);
                DUO_ROW(bp_row + 1u) = make_uint4(tlo, thi | (bp_rd ? bp_w << 16 : 0u), MSIM_T_OK | (fk << 2) | (bp_node << 12), bp_rd ? bp_po : bp_v);
              }
              n_cl += bp_t ? 1u : 0u;
              n_arr += bp_t ? bp_e & 0xFFFFu : 0u;
              // a word completed in mid-plan: all ones in every node lane (tested above on the half's word), written back before sw is reset
              if (bp_x_lo | bp_x_hi) {
                if (lane_in(hm2(bp_x_lo, bp_x_hi))) DUO_SET(set_lane + ((next_value & 0xFFE0u) << 2)) = sw | ~((1u << (next_value & 31u)) - 1u);
                bp_vw_lo += bp_x_lo ? 1u : 0u; bp_vw_hi += bp_x_hi ? 1u : 0u;
              }
              // the last word of a read's payload, where its value count is no multiple of 32
              const u32 bp_same = (bp_v >> 5) == (next_value >> 5) && (next_value & 31u) != 0 ? 0xFFFFFFFFu : 0u;
              const u32 bp_pv = (bp_sh & bp_same) | (((1u << (bp_v & 31u)) - 1u) & ~(((1u << (next_value & 31u)) - 1u) & bp_same));
              // the state behind op m - 1: lane m's own figures
              const u32 bp_ma = (bp_up ? 32u + bp_m_hi : bp_m_lo) << 2, bp_c = bp_up ? bp_c_hi : bp_c_lo;
              sw = lane_in(hm2(bp_o_lo, bp_o_hi)) ? 0u : sw;
              sw |= bp_up ? bp_g_hi : bp_g_lo;
              sr_dirty |= hm2(bp_nb_lo != 0, bp_nb_hi != 0);
              T = bperm(bp_ma, bp_T);
              next_value = bperm(bp_ma, bp_v);
              n_payload = bperm(bp_ma, bp_po);
              rounds += bp_c + (bperm(bp_ma, bp_es) >> 16);
              n_rows += 2u * bp_c;
              gen_k += bp_c;
              // the payload: the reads of both halves side by side, every word by the lane of its position
              for (u32 bp_r_lo = bp_tk_lo & ~(u32)bp_bcb, bp_r_hi = bp_tk_hi & ~(u32)(bp_bcb >> 32); (bp_r_lo | bp_r_hi) != 0; bp_r_lo &= bp_r_lo - 1u, bp_r_hi &= bp_r_hi - 1u) {
                const u32 bp_ra = (bp_up ? 32u + (u32)__builtin_ctz(bp_r_hi | 0x80000000u) : (u32)__builtin_ctz(bp_r_lo | 0x80000000u)) << 2;
                const u32 bp_xo = bperm(bp_ra, bp_po), bp_xv = bperm(bp_ra, bp_v), bp_xp = bperm(bp_ra, bp_pv);
                const bool bp_xn = lane_in(hm2(bp_r_lo != 0, bp_r_hi != 0));
                const u32 bp_xw = bp_xn ? (bp_xv + 31u) >> 5 : 0u;
                const u32 bp_xl = (bp_xv & 31u) != 0 ? bp_xw - 1u : 0xFFFFFFFFu;
                for (u32 w = bp_i; bal(w < bp_xw); w += 32)
                  if (w < bp_xw) DUO_PAY(bp_xo + w) = w == bp_xl ? bp_xp : 0xFFFFFFFFu;
              }
#ifdef DUO_PROF
              pf_nplan += (bp_c_lo ? 1u : 0u) + (bp_c_hi ? 1u : 0u); pf_nplanop += bp_c_lo + bp_c_hi;
              { const u32 pf_b = bp_up ? bp_nb_hi : bp_nb_lo; pf_nrunb += pf_b; pf_nrep += pf_b; pf_nrun += bp_c - pf_b; }
#endif
            }
          }
        }
        for (;;) {
          const u32 rr_k = gen_k - dc_base;
          u32 rr_hi, rr_lo; DUO_DRAW(gen_k, rr_hi, rr_lo);
          const u32 rr_next = T + __umulhi(rr_hi, p.gen_period2_us);
          const u32 rr_words = (next_value + 31u) >> 5;
          const u32 rr_node = scale32(rr_lo, N);
          const u64 rr_rd = DUO_BAL_CMP(rr_lo & 1u, !=, 0u, 33);
          const u64 rr_c = op_m & bal(rr_k < 31u) & bal(rr_next < cutoff) & bal(n_rows + 4u <= max_rows);
          const u64 rr_b = rr_c & rr_rd & bal(n_payload + rr_words <= max_pay) & bal(rounds < round_limit);
          u64 sb_b = 0;
          if (sr_m) sb_b = sr_m & rr_c & ~rr_rd & DUO_BAL_CMP((mm_known >> rr_node) & 1u, !=, 0u, 33) & DUO_BAL_CMP(T, <, rr_next, 36) &
                           DUO_BAL_CMP(next_value + 1u, <, max_values, 36);
          const u64 sr_go = rr_b | sb_b;
          if (!sr_go) break;
          const bool rr_go = lane_in(sr_go), rr_rdn = lane_in(rr_b);
          const bool rr_sel = rr_go && i == rr_node;
          n_cl += rr_sel ? 1u : 0u;
          if (const u64 sr_wb = sr_dirty & (rr_b | (sb_b & DUO_BAL_CMP(next_value & 31u, ==, 0u, 32)))) { DUO_FLOOD_WB(sr_wb); sr_dirty &= ~sr_wb; }
          if constexpr (BPLAN) { if (const u64 sr_open = sb_b & DUO_BAL_CMP(next_value & 31u, ==, 0u, 32)) DUO_BPLAN_SEEN(sr_open); }   // (the word is complete and current in HBM)
          wave_lds_fence();
          for (u32 w = i; rr_b & bal(w < rr_words); w += 32)
            if (rr_rdn && w < rr_words) DUO_PAY(n_payload + w) = DUO_SET(set_half + w * 128u + rr_node * 4u);
          const u32 rr_val = next_value;
          if (rr_sel) {
            u32 rr_i = i; MSIM_OPAQUE(rr_i);   // (the rows' constant words are built here, not kept in registers across the rounds)
            const u64 tns = (u64)T * 1000ull;
            const u32 tlo = (u32)tns, thi = (u32)(tns >> 32);
            const u32 fk = rr_rdn ? (u32)MSIM_F_READ : (u32)MSIM_F_BROADCAST;
            DUO_ROW(n_rows) = make_uint4(tlo, thi, MSIM_T_INVOKE | (fk << 2) | (rr_i << 12), rr_rdn ? MSIM_NO_VALUE : rr_val);
            DUO_ROW(n_rows + 1u) = make_uint4(tlo, thi | (rr_rdn ? rr_words << 16 : 0u), MSIM_T_OK | (fk << 2) | (rr_i << 12), rr_rdn ? n_payload : rr_val);
          }
          n_payload += rr_rdn ? rr_words : 0u;
          if (sb_b) {   // the remembered flood of each broadcasting half (sb_e is 0 in the other half's lanes)
            DUO_LANE_NOW(sb_l);
            u32 sb_e = 0;
            if (lane_in(sb_b)) sb_e = DUO_MEMO_AT(rr_node, sb_l);
#ifdef MSIM_HIPEMU
            if (rr_sel && !rr_rdn && ((sb_e >> 7) & 1u) == 0) __builtin_trap();   // the picked node's own lane carries the bit
#endif
            sw = lane_in(sb_b & DUO_BAL_CMP(rr_val & 31u, ==, 0u, 32)) ? 0u : sw;
            sw |= ((sb_e >> 7) & 1u) << (rr_val & 31u);
            n_arr += sb_e & 0x7Fu;
            rounds += sb_e >> 8;
            next_value += lane_in(sb_b) ? 1u : 0u;
            sr_dirty |= sb_b;
#ifdef DUO_PROF
            pf_nrunb += lane_in(sb_b) ? 1u : 0u; pf_nrep += lane_in(sb_b) ? 1u : 0u;
#endif
          }
          n_rows += rr_go ? 2u : 0u;
          gen_k += rr_go ? 1u : 0u;
          T = rr_go ? rr_next : T;      // (the next round's R0: nothing is due, the scheduler acts at the generator's next op)
          rounds += rr_go ? 1u : 0u;
#ifdef DUO_PROF
          pf_nrun += rr_rdn ? 1u : 0u; pf_nit++;
#endif
        }
        if (sr_dirty) DUO_FLOOD_WB(sr_dirty);
        DUO_BPLAN_SEEN(op_m & fl_m);   // (a plan or the loop may have ended on a completed word, which the round below may leave behind)
      } else
      if (FLOOD) {
        for (;;) {
          const u32 rr_k = gen_k - dc_base;
          u32 rr_hi, rr_lo; DUO_DRAW(gen_k, rr_hi, rr_lo);
          const u32 rr_next = T + __umulhi(rr_hi, p.gen_period2_us);
          const u32 rr_words = (next_value + 31u) >> 5;
          const u64 rr_b = op_m & bal((rr_lo & 1u) != 0) & bal(rr_k < 31u) & bal(rr_next < cutoff) & bal(n_rows + 4u <= max_rows) &
                           bal(n_payload + rr_words <= max_pay) & bal(rounds < round_limit);
          if (!rr_b) break;
          const bool rr_go = lane_in(rr_b);
          const u32 rr_node = scale32(rr_lo, N);
          const bool rr_sel = rr_go && i == rr_node;
          n_cl += rr_sel ? 1u : 0u;
          wave_lds_fence();
          for (u32 w = i; rr_b & bal(w < rr_words); w += 32)
            if (rr_go && w < rr_words) DUO_PAY(n_payload + w) = DUO_SET(set_half + w * 128u + rr_node * 4u);
          if (rr_sel) {
            u32 rr_i = i; MSIM_OPAQUE(rr_i);   // (the rows' constant words are built here, not kept in registers across the rounds)
            const u64 tns = (u64)T * 1000ull;
            const u32 tlo = (u32)tns, thi = (u32)(tns >> 32);
            DUO_ROW(n_rows) = make_uint4(tlo, thi, MSIM_T_INVOKE | ((u32)MSIM_F_READ << 2) | (rr_i << 12), MSIM_NO_VALUE);
            DUO_ROW(n_rows + 1u) = make_uint4(tlo, thi | (rr_words << 16), MSIM_T_OK | ((u32)MSIM_F_READ << 2) | (rr_i << 12), n_payload);
          }
          n_payload += rr_go ? rr_words : 0u;
          n_rows += rr_go ? 2u : 0u;
          gen_k += rr_go ? 1u : 0u;
          T = rr_go ? rr_next : T;      // (the next round's R0: nothing is due, the scheduler acts at the generator's next op)
          rounds += rr_go ? 1u : 0u;
#ifdef DUO_PROF
          pf_nrun += rr_go ? 1u : 0u;
#endif
        }
      }
      // QUIET OP ROUND.  The body below is a superset: it serves a half that acts beside one in mid-flood, a half outside flood mode, halves
      // that only gossip, and both queue representations.  Pairing has made one situation the rule: EVERY live half acts, from flood mode.
      // By st_m such a half is quiescent, so in every lane of it in_n == 0, sp_n == 0, deliver_at == INF and busy == 0, and nothing is due in
      // the wavefront (op_due == 0; a -DDUO_PROF build and the host-emulator build trap if any of that is false).  Then the round's gossip
      // part has nothing to do, and the exchange would only find what every lane can read off its own registers: the one publisher of a
      // half is the picked node of its broadcast, whose client's request fans out to all of its adj, so a lane receives exactly one envelope
      // iff its half's op is a broadcast and bit `picked` of its OWN adj is set (the neighbour relation is symmetric, see topo_adj); the poll
      // would take that envelope out of a queue that held nothing else: cm = value | picked << 16 (DK_PLAIN), deliver_at = T, in_n stays 0
      // (nx means nothing while the queue is empty and is not written).  The pick, the read, the rows, the set word and the tail are the
      // superset body's; every round, delivery and message is simulated as before, only the detour through the exchange goes.  The state is
      // updated in place, and the path meets the superset body's only in front of the tail they share.  The tests are scalar, on masks in SGPRs;
      // every other op wave-round (one op, a half outside flood mode, the first op behind a GENERAL body) takes the body below as it is.
      bool quiet = false;
      if constexpr (FLOOD) quiet = fl_ok && (alive_m & ~op_m) == 0 && (op_m & ~fl_m) == 0;
      u64 dw_m = 0;   // MEMO: the halves this round leaves with nothing in flight: a read, a replayed broadcast (the quiet body knows them)
#ifdef DUO_PROF
      bool pf_flr = false;
#endif
      if (FLOOD && quiet) {
#if defined(DUO_PROF) || defined(MSIM_HIPEMU)
        if (op_due != 0 || (opn && ((in_n | sp_n | busy) != 0 || deliver_at != INF))) __builtin_trap();   // the quiet invariant
#endif
        // 1. the op's draw and pick
        u32 r_hi, r_lo; DUO_DRAW(gen_k, r_hi, r_lo);
        const u32 picked = scale32(r_lo, N);
        const u64 rd_m = op_m & DUO_BAL_CMP(r_lo & 1u, !=, 0u, 33);   // the halves whose op is a read, a broadcast (whole halves)
        const u64 bc_m = op_m & ~rd_m;
        const u64 sel_b = op_m & DUO_BAL_CMP(i, ==, picked, 32);
        const bool sel = lane_in(sel_b);
        const u32 val = next_value;
        next_value += lane_in(bc_m) ? 1u : 0u;
        gen_k += opn ? 1u : 0u;
        gen_next = opn ? T + __umulhi(r_hi, p.gen_period2_us) : gen_next;
        n_cl += sel ? 1u : 0u;
        // 2. a read -> read_ok with the whole set of the picked node, copied by the cluster's lanes; the cluster publishes nothing
        u32 cmp_value = val, cmp_len = 0;
        if (const u64 rs_b = sel_b & rd_m) {
          wave_lds_fence();
          const u32 words = (next_value + 31u) >> 5;
          const bool ok = n_payload + words <= max_pay;   // payload_alloc of the oracle
          const u64 ok_b = rs_b & bal(ok);
          if (lane_in(rs_b)) {
            if (!ok) my_flags |= MSIM_FLAG_PAYLOAD_OVERFLOW;
            cmp_value = ok ? n_payload : 0u; cmp_len = words;
          }
          const u64 cp_b = hm2((u32)ok_b != 0, (u32)(ok_b >> 32) != 0);   // the clusters that copy a set
          const bool cp = lane_in(cp_b);
          for (u32 w = i; cp_b & bal(w < words); w += 32)
            if (cp && w < words) DUO_PAY(n_payload + w) = DUO_SET(set_half + w * 128u + picked * 4u);
          n_payload += cp ? words : 0u;
        }
        // 3. the invocation and the completion row
        if (sel) {
          u32 r4_i = i; MSIM_OPAQUE(r4_i);   // (the rows' constant words are built here, not kept in registers across the rounds)
          const bool is_rd = lane_in(rd_m);
          const u64 tns = (u64)T * 1000ull;
          const u32 tlo = (u32)tns, thi = (u32)(tns >> 32);
          const u32 fk = is_rd ? (u32)MSIM_F_READ : (u32)MSIM_F_BROADCAST;
          DUO_ROW(n_rows) = make_uint4(tlo, thi, MSIM_T_INVOKE | (fk << 2) | (r4_i << 12), is_rd ? MSIM_NO_VALUE : val);
          DUO_ROW(n_rows + 1u) = make_uint4(tlo, thi | (cmp_len << 16), MSIM_T_OK | (fk << 2) | (r4_i << 12), cmp_value);
        }
        n_rows += opn ? 2u : 0u;
        // 4. the set word of the flood to come (B): the word of value next_value - 1, or 0 where a broadcast's value opens a new word, with
        //    the picked node's own bit
        sw = lane_in(bc_m & DUO_BAL_CMP(val & 31u, ==, 0u, 32)) ? 0u : sw;
        sw |= lane_in(sel_b & bc_m) ? 1u << (val & 31u) : 0u;
        // 5. the broadcast's delivery: the picked node's neighbours hold its envelope, due in the cluster's next round
        //    FLOOD MEMO: unless the flood from this origin is remembered and may be replayed; then all of it is applied here
        u64 rp_m = 0;
        if constexpr (MEMO) {
          const u64 kn_m = bc_m & DUO_BAL_CMP((mm_known >> picked) & 1u, !=, 0u, 33);   // whole halves: picked is the cluster's
          const u64 cand_m = kn_m & DUO_BAL_CMP(next_value, <, max_values, 36) & DUO_BAL_CMP(n_rows + 2u, <=, max_rows, 37) &
                             DUO_BAL_CMP(gen_next, <, cutoff, 36) & DUO_BAL_CMP(T, <, gen_next, 36);
          if (cand_m) {
            DUO_LANE_NOW(mr_l);
            u32 mr_e = 0;
            if (lane_in(cand_m)) mr_e = DUO_MEMO_AT(picked, mr_l);
            const u32 mr_k = max(rdlane(mr_e, 0), rdlane(mr_e, 32)) >> 8;   // the longest flood replayed (a half that does not replay: 0)
            rp_m = (alive_m & ~DUO_BAL_CMP(rounds + mr_k + 1u, <, round_limit, 36)) == 0 ? cand_m : 0ull;
            if constexpr (DUO_MEMO_CHECK) {   // simulate it all the same; the head of the half's next op round compares
              if (rp_m) {
                const bool vf_on = lane_in(rp_m);
                vf_e = vf_on ? mr_e : vf_e; vf_n0 = vf_on ? n_arr : vf_n0; vf_r0 = vf_on ? rounds : vf_r0; vf_bit = vf_on ? (val & 31u) : vf_bit;
                vf_m |= rp_m;
              }
            }
#ifdef DUO_PROF
            pf_nrep += lane_in(rp_m) ? 1u : 0u;
#endif
            if constexpr (DUO_MEMO_CHECK) rp_m = 0;
            if (rp_m) {   // (mr_e is 0 in the lanes of a half that does not replay)
              n_arr += mr_e & 0x7Fu;
              sw |= ((mr_e >> 7) & 1u) << (val & 31u);
              rounds += mr_e >> 8;
            }
          }
          if (const u64 un_m = bc_m & ~kn_m) {   // an origin not remembered (rare): record this flood, see FLOOD MEMO
            const u32 ms_lo = rdlane(picked, 0), ms_up = rdlane(picked, 32);
            const u64 ms_m = (un_m == ~0ull && ms_lo == ms_up) ? 0xFFFFFFFFull : un_m;   // (one row, one recorder)
            DUO_LANE_NOW(ms_l);
            if (lane_in(ms_m)) DUO_MEMO_AT(picked, ms_l) = (unsigned short)((n_arr & 0x7Fu) | ((rounds & 0xFFu) << 8));
            mm_rec = ms_m; mm_org = ms_lo | (ms_up << 8);
          }
          dw_m = rd_m | rp_m;
        }
        const bool rcv = lane_in(bc_m & ~rp_m & DUO_BAL_CMP((adj >> picked) & 1u, !=, 0u, 33));
        n_arr += rcv ? 1u : 0u;
        cm = rcv ? (val | (picked << 16)) : cm;
        deliver_at = rcv ? T : deliver_at;
        // 6. the tail (the next block of draws, the scheduler's view) is the one below, shared with the superset body
#ifdef DUO_PROF
        pf_flr = true; pf_nquiet++;
#endif
      } else {
      // the word of the nodes' sets that the op's value falls in, fetched first: only the picked node's store at the end of the round
      // waits for it (a broadcast value is fresh — no node has seen it — so the node's dedup does not need it)
      u32 op_w = 0;
      if (FLOOD) {   // TRIM (B): the word of value next_value - 1: in sw already in flood mode, and 0 where the op's value opens a new word
        op_w = sw;
        if (op_m & ~fl_m) { if (opn && !lane_in(fl_m)) op_w = DUO_SET(set_lane + (((max(next_value, 1u) - 1u) & 0xFFE0u) << 2)); }
      } else
      if (opn) op_w = DUO_SET(set_lane + ((next_value & 0xFFE0u) << 2));
      const bool fl_round = FLOOD && (alive_m & ~fl_m) == 0;   // every live half is in flood mode: the flood op round
      u32 r_hi, r_lo; DUO_DRAW(gen_k, r_hi, r_lo);   // (the op's draw is in the cluster's block of 32; the GENERAL body draws the next block)
      const bool sel = opn && i == scale32(r_lo, N);
      const bool is_rd = (r_lo & 1u) != 0;
      const bool bc = sel & !is_rd;
      const u32 val = next_value;
      next_value += opn && !is_rd ? 1u : 0u;
      gen_k += opn ? 1u : 0u;
      gen_next = opn ? T + __umulhi(r_hi, p.gen_period2_us) : gen_next;
      n_cl += sel ? 1u : 0u;
      // R3: the gossip of both clusters (the picked nodes are idle: due_n is false there), then the picked node's broadcast
      const bool due_n = lane_in(op_due);
      u32 pub; u64 pub_b;
      if (fl_round) DUO_FLOOD_R3(due_n, op_due, pub, pub_b);
      else { DUO_R3_SEEN(due_n, op_due, pub, pub_b); deliver_at = due_n ? INF : deliver_at; }
      if (!FLOOD) n_rsv += due_n ? 1u : 0u;
      pub = bc ? (fl_round ? adj : (0x80000000u | (63u << 16) | val)) : pub;   // (the flood bodies publish fan-out masks)
      pub_b |= bal(bc);
#ifdef DUO_PROF
      pf_nbout += half_any(bc) ? 1u : 0u;
#endif
      // a read -> read_ok with the whole set, copied by the cluster's lanes (one reader per cluster)
      u32 cmp_value = val, cmp_len = 0;
      if (const u64 rd_b = bal(sel) & bal(is_rd)) {
        wave_lds_fence();
        const u32 words = (next_value + 31u) >> 5;
        const bool ok = n_payload + words <= max_pay;   // payload_alloc of the oracle
        const u64 ok_b = rd_b & bal(ok);
        if (sel && is_rd) {
          if (!ok) my_flags |= MSIM_FLAG_PAYLOAD_OVERFLOW;
          cmp_value = ok ? n_payload : 0u; cmp_len = words;
        }
        const u32 ok_lo = (u32)ok_b, ok_up = (u32)(ok_b >> 32), okm = hi ? ok_up : ok_lo;
        const u32 r1 = okm ? (u32)__builtin_ctz(okm) : 0u;
        const u64 cp_b = hm2(ok_lo != 0, ok_up != 0);   // the clusters that copy a set
        for (u32 w = i; cp_b & bal(w < words); w += 32)
          if (lane_in(cp_b) && w < words) DUO_PAY(n_payload + w) = DUO_SET(set_half + w * 128u + r1 * 4u);
        n_payload += okm ? words : 0u;
      }
      // R4: the invocation and the completion row
      if (sel) {
        u32 r4_i = i; if (FLOOD) MSIM_OPAQUE(r4_i);   // (FLOOD: the rows' constant words are built here, not kept in registers across the rounds)
        const u64 tns = (u64)T * 1000ull;
        const u32 tlo = (u32)tns, thi = (u32)(tns >> 32);
        const u32 fk = is_rd ? (u32)MSIM_F_READ : (u32)MSIM_F_BROADCAST;
        DUO_ROW(n_rows) = make_uint4(tlo, thi, MSIM_T_INVOKE | (fk << 2) | (r4_i << 12), is_rd ? MSIM_NO_VALUE : val);
        DUO_ROW(n_rows + 1u) = make_uint4(tlo, thi | (cmp_len << 16), MSIM_T_OK | (fk << 2) | (r4_i << 12), cmp_value);
      }
      n_rows += opn ? 2u : 0u;
      // FLOOD: the picked node's new set word and every other lane's (unchanged) one: what the store writes and what sw becomes
      if (FLOOD) op_w = lane_in(op_m & DUO_BAL_CMP(r_lo & 1u, ==, 0u, 32) & DUO_BAL_CMP(val & 31u, ==, 0u, 32)) ? 0u : op_w;
      const u32 op_w1 = FLOOD ? (op_w | (bc ? 1u << (val & 31u) : 0u)) : 0u;
      if (fl_round) {
        if (pub_b) DUO_FLOOD_ARRIVALS(pub);
        DUO_FLOOD_POLL();
      } else {
        if (pub_b) DUO_ARRIVALS(pub);
        if (bc) DUO_SET(set_lane + ((val & 0xFFE0u) << 2)) = FLOOD ? op_w1 : (op_w | (1u << (val & 31u)));
        DUO_POLL();
      }
      // the acting clusters are quiescent but for this op: they are in flood mode from here on (a read: with nothing in flight).  The word
      // of the op's value is every lane's set word for the flood to come (no node has handled anything in this round)
      if (fl_ok) { sw = opn ? op_w1 : sw; fl_m |= op_m; }
#ifdef DUO_PROF
      pf_flr = fl_round;
#endif
      }
      // FLOOD: a cluster that has used up its block of the generator's draws draws the next one here (once per 32 ops), where the round's
      // temporaries are dead; without flood mode its next op takes the GENERAL body, which draws it and leaves flood mode
      if (FLOOD) {
        DUO_DRAW_REFILL(opn & (gen_k - dc_base >= 32u));
      }
      // the scheduler's view: an acting cluster acts again at its generator's next op (every worker is free again); the others are as
      // they were.  The full view runs when it would run in the GENERAL body (an op moved gen_next to or past cutoff)
      if (alive_m & (bal(phase != PH_MAIN) | bal(gen_next >= cutoff) | bal(rounds > round_limit))) {
        const u64 hbusy_b = bal(busy != 0);
        DUO_SCHED_VIEW(hbusy_b);
        alive_v = lane_in(alive_m) ? 1u : 0u;
        if (~alive_m) {
          if (!lane_in(alive_m)) { if (FLOOD) my_flags += (in_n + sp_n + (deliver_at != INF ? 1u : 0u) - busy) * DUO_DROP_ONE;   /* what stays undelivered (A) */
                                   deliver_at = INF; in_n = 0; sp_n = 0; have_creq = 0; bag_used = 0; }
        }
        if (FLOOD) sd_m = 0;
      } else {
        sched_at = opn ? gen_next : sched_at;
        // STEADY LEAVE: the acting halves' bits of sd_m, on the state this round leaves (see sd_m); a half that did not act keeps its bit
        // (three of sd_m's terms need no compare here.  phase == PH_MAIN and gen_next < cutoff: this is the else branch of the test above,
        //  which has just found both in every lane of every live half.  busy == 0: an acting half had no busy client when this op round was
        //  chosen, by st_m's sixth term or by its bit of sd_m, and an op round leaves busy as it is; looking at it here kept it in a register
        //  through the superset body, which sent that body's rarest path to scratch.  The emulator and -DDUO_PROF builds check all three at the use)
        if constexpr (FLOOD)
          sd_m = (sd_m & ~op_m) | (op_m & fl_m & DUO_BAL_CMP(next_value, <, max_values, 36) & DUO_BAL_CMP(n_rows + 2u, <=, max_rows, 37) & DUO_BAL_CMP(gen_k - dc_base, <, 32u, 36));
      }
#ifdef DUO_PROF
      if (pf_flr) { pf_fop += __builtin_readcyclecounter() - pf_a; pf_nfop++; } else { pf_op += __builtin_readcyclecounter() - pf_a; pf_nop++; }
      pf_nop2 += op_m == ~0ull ? 1u : 0u;
#endif
      // THE DIRECT WAY ON (FLOOD MEMO).  Both halves have come out of the quiet body with nothing in flight (dw_m: a read or a replayed
      // broadcast each) and steady (sd_m, which the tail has just set on the state this round leaves: the view did not run, so alive_m is
      // what it was, both halves, and nobody is parked: both acted).  The loop's head would find two dry halves: R0's block moves each T
      // to its sched_at (gen_next, never INF and never behind T), looks at the round limit of both, the round is counted, the exit test
      // finds st_m in both halves by sd_m and nothing due, and nobody to park: an op round of both, the quiet body by its own test.  That
      // is what the steady leave does for two dry halves, and it is done here in its words: the same time jump and round count, the same
      // decline at the limit (round_limit < rounds with the next round counted), and whatever is declined goes to the loop's head untouched.
      // (park_left, far from 0 while nobody is parked, is not counted down for these rounds: it is set again before anybody looks at it)
      if constexpr (MEMO) {
        if (dw_m == ~0ull && sd_m == ~0ull && fg_m == 0 && DUO_BAL_CMP(round_limit, <, rounds + 1u, 36) == 0) {
#if defined(DUO_PROF) || defined(MSIM_HIPEMU)
          if (alive_m != ~0ull || park_m != 0 || (in_n | sp_n | busy) != 0 || deliver_at != INF || sched_at < T || sched_at == INF || phase != PH_MAIN ||
              next_value >= max_values || n_rows + 2u > max_rows || gen_k - dc_base >= 32u) __builtin_trap();   // what R0's block and the exit test would have found
#endif
          T = sched_at;
          rounds += 1u;
          mm_direct = DUO_UNIFORM(1u);   // (op_m = ~0, op_due = 0: in front of the gossip loop, which is passed by)
#ifdef DUO_PROF
          pf_nwave++;
#endif
        }
      }
    } else {   // ---- a round in which a cluster's scheduler acts or a node handles its client's request ----
    P3_MARK(0)   // [0] = the gossip rounds
    DUO_MATERIALISE();
    if (FLOOD) sd_m = 0;   // (this body changes what the bits stand for, see sd_m)
#ifdef DUO_PROF
    if (MEMO) pf_ndrop += ((u32)mm_rec ? 1u : 0u) + ((u32)(mm_rec >> 32) ? 1u : 0u);
#endif
    if (MEMO) mm_rec = 0;   // (and a flood it takes part in is not recorded, see FLOOD MEMO)
    // (FLOOD: what this body derives from the lane number alone is built here, not kept in registers across the rounds)
    DUO_UPM_NOW();   // TRIM (C)
    u32 gi = i; if (FLOOD) MSIM_OPAQUE(gi);
    const u32 g_lt = FLOOD ? (1u << gi) - 1u : lt;
    u32 inv_row = 0, inv_packed = 0, inv_value = 0;
    u32 cmp_row = 0, cmp_packed = 0, cmp_value = 0, cmp_len = 0;
    // ---- R1: scheduler (core.clj:67-80): phase actions, one generated op ----
    u32 mark = 0, m_kind = 0, m_val = 0;
    const u64 act_b = alive_m & bal(sched_at <= T);
    const bool act = lane_in(act_b);
    if constexpr (MEMO && DUO_MEMO_CHECK) {   // a scheduler that acts on a half whose remembered flood is still under way: a replay would have been wrong
      if (lane_in(vf_m & act_b) && (in_n != 0 || deliver_at != INF)) __builtin_trap();
      vf_m &= ~act_b;
    }
    if (act_b & bal(phase != PH_MAIN)) {   // rare: db setup, topology, final reads
      if (act && phase == PH_INIT) { mark = is_node; m_kind = DK_INIT; phase = PH_INIT_WAIT; }
      else if (act && phase == PH_TOPO) { mark = is_node; m_kind = DK_TOPO; phase = PH_TOPO_WAIT; }
      else if (act && (phase == PH_SLEEP || phase == PH_FINAL)) { mark = is_node; m_kind = DK_READ_FINAL; phase = PH_FINAL_WAIT; }  // broadcast.clj:240
    }
    if (act_b & bal(phase == PH_MAIN)) {
      const u32 free_mask = all_nodes & ~hb(busy != 0, hi);
      const bool gen = act && phase == PH_MAIN && rate > 0 && gen_next < cutoff && gen_next <= T && free_mask != 0;
      // one 64-bit draw per generated op: high word -> stagger, low word -> worker pick / gen/mix
      DUO_DRAW_REFILL(gen_k - dc_base >= 32u);   // (uniform within a cluster)
      u32 r_hi, r_lo; DUO_DRAW(gen_k, r_hi, r_lo);
      const u32 pick = scale32(r_lo, __popc(free_mask));
      const bool sel = gen && is_node && busy == 0 && (u32)__popc(free_mask & g_lt) == pick;
      const bool is_rd = (r_lo & 1u) != 0;
      const bool ovf = gen && !is_rd && next_value >= max_values;
      if (bal(next_value >= max_values)) { flags |= ovf ? (u32)MSIM_FLAG_VALUES_OVERFLOW : 0u; alive_m &= ~bal(ovf); }   // (rare: out of values)
      mark = sel && !ovf ? 1u : mark;
      m_kind = gen ? (is_rd ? DK_READ : DK_BCAST) : m_kind;
      m_val = gen && !is_rd ? next_value : m_val;
      next_value += gen && !is_rd && !ovf ? 1u : 0u;
#ifdef DUO_PROF
      pf_nbout += gen && !is_rd && !ovf ? 1u : 0u;
#endif
      gen_k += gen ? 1u : 0u;
      gen_next = gen ? T + __umulhi(r_hi, p.gen_period2_us) : gen_next;
    }
    P3_MARK(1)   // [1] = R1 scheduler
    // ---- R2: marked clients invoke; the request reaches this lane's own node (no latency: a client is involved) ----
    if (const u64 inv_b = bal(mark != 0) & alive_m) {
      const bool inv = lane_in(inv_b);
      busy = inv ? 1u : busy;
      const bool is_op = inv && m_kind <= DK_READ_FINAL;
      inv_row = is_op ? 1u : 0u;
      inv_packed = MSIM_T_INVOKE | ((m_kind == DK_BCAST ? MSIM_F_BROADCAST : MSIM_F_READ) << 2) | ((m_kind == DK_READ_FINAL ? 1u : 0u) << 11) | (gi << 12);
      inv_value = m_kind == DK_BCAST ? m_val : MSIM_NO_VALUE;
      const u32 e = (m_kind == DK_BCAST ? m_val : 0u) | (63u << 16) | (m_kind << 24);
      if (RND) next_id += __popc(hb(inv, hi));   // the requests' ids, slot order (their latency is 0: no draw)
      if (LAT0 || RND) {
        const bool direct = inv & (deliver_at == INF);   // an idle node's recv! takes the request at once (its queue is empty)
        cm = direct ? e : cm; deliver_at = direct ? T : deliver_at;
        DUO_PUSH_CHECKED(inv & !direct, e, T);
      } else {
        if (inv && have_creq != 0) my_flags |= MSIM_FLAG_INBOX_OVERFLOW;   // cannot happen without client timeouts
        have_creq = inv ? 1u : have_creq; creq = inv ? e : creq; creq_t = inv ? T : creq_t;
      }
      // LAT0 / RND: nobody has to poll here — an idle node took its request directly (only the set word of its new envelope is
      // missing), every other node holds an envelope already; constant latency > 0: the request waits beside the FIFO, recv! chooses
      if (LAT0 || RND) DUO_SW_PREFETCH(); else DUO_POLL();
    }

    P3_MARK(2)   // [2] = R2 invoke + poll
    // ---- R3: one input per node: the due envelope ----
    const u64 due_b = alive_m & bal(deliver_at <= T);
    const bool due_n = lane_in(due_b);
    const u32 kind = cm >> 24;
    const u32 v = cm & 0xFFFFu;
    u32 pub; u64 pub_b; DUO_R3_SEEN(due_n & (kind <= DK_BCAST), due_b & bal(kind <= DK_BCAST), pub, pub_b);
    deliver_at = due_n ? INF : deliver_at;
    if (!FLOOD) n_rsv += (due_n && kind == DK_PLAIN) ? 1u : 0u;
    const bool req = due_n && kind != DK_PLAIN;   // a request of this lane's client: handled, answered and completed in this round
    n_cl += req ? 1u : 0u;
    busy = req ? 0u : busy;
    cmp_row = (req && kind == DK_BCAST) ? 1u : 0u;
    cmp_packed = MSIM_T_OK | (MSIM_F_BROADCAST << 2) | (gi << 12); cmp_value = v;
    // read -> read_ok with the whole set: the cluster's lanes copy the node's set (scratch) -> HBM payload
    // (the readers' and the copying clusters' masks come from ballots of single compares: a ballot of a bool built from several costs two
    //  vector instructions more)
    if (const u64 rd_b = due_b & bal(kind - (u32)DK_READ < 2u)) {   // the lanes whose request is a read (kind DK_READ or DK_READ_FINAL)
      wave_lds_fence();
      const bool rd = lane_in(rd_b);
      const u32 rdm = hi ? (u32)(rd_b >> 32) : (u32)rd_b;
      const u32 words = (next_value + 31u) >> 5;
      const u32 my_rank = __popc(rdm & g_lt);
      const bool ok = n_payload + (my_rank + 1u) * words <= max_pay;   // payload_alloc of the oracle, reader by reader
      const u32 my_off = ok ? n_payload + my_rank * words : 0u;
      const u64 ok_b = rd_b & bal(ok);
      if (rd) {
        if (!ok) my_flags |= MSIM_FLAG_PAYLOAD_OVERFLOW;
        cmp_row = 1; cmp_packed = MSIM_T_OK | (MSIM_F_READ << 2) | ((kind == DK_READ_FINAL ? 1u : 0u) << 11) | (gi << 12);
        cmp_value = my_off; cmp_len = words;
      }
      const u32 ok_lo = (u32)ok_b, ok_up = (u32)(ok_b >> 32), okm = hi ? ok_up : ok_lo;
      u32 m = okm;
      if (((ok_lo & (ok_lo - 1u)) | (ok_up & (ok_up - 1u))) == 0) {   // the usual round: at most one reader per cluster — lane w copies word w of its set
        const u32 r1 = okm ? (u32)__builtin_ctz(okm) : 0u;
        const u64 cp_b = hm2(ok_lo != 0, ok_up != 0);   // the clusters that copy a set
        for (u32 w = i; cp_b & bal(w < words); w += 32)
          if (lane_in(cp_b) && w < words) DUO_PAY(n_payload + w) = DUO_SET(set_half + w * 128u + r1 * 4u);
        m = 0;
      }
      while (__ballot(m != 0)) {
        const bool on = m != 0;
        const u32 r = on ? (u32)__builtin_ctz(m) : 0u;
        m &= m - 1u;
        const u32 r_off = bperm(hbase4 + (r << 2), my_off);
        for (u32 w = i; __ballot(on && w < words); w += 32)
          if (on && w < words) DUO_PAY(r_off + w) = DUO_SET(set_half + w * 128u + r * 4u);
      }
      n_payload += __popc(okm) * words;
    }

    P3_MARK(3)   // [3] = R3 (dedup, read copies)
    if (RND) { if (__ballot((pub != 0) | req)) DUO_RND_IDS(pub, req); }
    if (pub_b) DUO_ARRIVALS(pub);
    P3_MARK(4)   // [4] = ids + arrivals
    DUO_POLL();
    P3_MARK(5)   // [5] = poll

    // ---- R4 + history rows: invocations (slot order), then completions (slot order) ----
    if (__ballot((inv_row | cmp_row) != 0)) {
      const u32 imask = hb(inv_row != 0, hi), cmask = hb(cmp_row != 0, hi);
      const u32 ni = __popc(imask), nr = ni + __popc(cmask);
      const bool ovf = lane_in(alive_m) && nr != 0 && n_rows + nr > max_rows;
      if (bal(n_rows + nr > max_rows)) { flags |= ovf ? (u32)MSIM_FLAG_ROWS_OVERFLOW : 0u; alive_m &= ~bal(ovf); }   // (rare: out of rows)
      const u64 tns = (u64)T * 1000ull;
      const u32 tlo = (u32)tns, thi = (u32)(tns >> 32);
      if (inv_row != 0 && !ovf) DUO_ROW(n_rows + __popc(imask & g_lt)) = make_uint4(tlo, thi, inv_packed, inv_value);
      if (cmp_row != 0 && !ovf) DUO_ROW(n_rows + ni + __popc(cmask & g_lt)) = make_uint4(tlo, thi | (cmp_len << 16), cmp_packed, cmp_value);
      const u32 new_n = ovf ? n_rows : n_rows + nr;
      n_rows = new_n;
    }

    P3_MARK(6)   // [6] = rows
    // ---- the scheduler's view for the rounds to come: time-free phase transitions (oracle: sched_resolve), when it
    //      acts next (sched_due), and whether plain gossip rounds may run meanwhile ----
    const u64 hbusy_b = bal(busy != 0);
    if (alive_m & (bal(phase != PH_MAIN) | (rate > 0 ? bal(gen_next >= cutoff) : bal(true)) | bal(rounds > round_limit))) {
      DUO_SCHED_VIEW(hbusy_b);
    } else {
      // every live cluster of the wavefront is in the main phase with its generator running (nearly every GENERAL round): the
      // scheduler acts again when the generator's next op is due and a worker is free, plain gossip rounds may run meanwhile
      sched_at = lane_in(alive_m & hm2((all_nodes & ~(u32)hbusy_b) != 0, (all_nodes & ~(u32)(hbusy_b >> 32)) != 0)) ? gen_next : INF;
      fg_m = 0;
    }
    alive_v = lane_in(alive_m) ? 1u : 0u;
    if (~alive_m) {
      if (!lane_in(alive_m)) { if (FLOOD) my_flags += (in_n + sp_n + (deliver_at != INF ? 1u : 0u) - busy) * DUO_DROP_ONE;   // what stays undelivered (A)
                               deliver_at = INF; in_n = 0; sp_n = 0; have_creq = 0; bag_used = 0; }   // a finished cluster takes no further part
    }
    P3_MARK(7)   // [7] = the scheduler's view
#ifdef DUO_PROF
    pf_gen += __builtin_readcyclecounter() - pf_a; pf_ngen++;
#endif
    }
    if (!alive_m) break;
  }
#ifdef DUO_PROF
  const u64 pf_tot = __builtin_readcyclecounter() - pf_t0;
  const u32 pf_nrun_all = rdlane(pf_nrun, 0) + rdlane(pf_nrun, 32);
  const u32 pf_nrunb_all = rdlane(pf_nrunb, 0) + rdlane(pf_nrunb, 32);
#endif

  // ---- epilogue: net stats, meta ----
  __syncthreads();
  // (FLOOD, see TRIM (A): a dropped envelope is not received either; what a stopped half left undelivered is counted there as well, `- busy`
  //  and all, so the field is read as a signed number)
  if (FLOOD) n_rsv += (u32)((int)my_flags >> 8);
  const u32 sc_cl = wave_incl_scan(n_cl), sc_arr = wave_incl_scan(n_arr), sc_rsv = wave_incl_scan(n_rsv);
  const u32 lo_cl = rdlane(sc_cl, 31), lo_arr = rdlane(sc_arr, 31), lo_rsv = rdlane(sc_rsv, 31);
  const u32 t_cl = hi ? rdlane(sc_cl, 63) - lo_cl : lo_cl;
  const u32 t_arr = hi ? rdlane(sc_arr, 63) - lo_arr : lo_arr;
  const u32 t_rsv = hi ? rdlane(sc_rsv, 63) - lo_rsv : lo_rsv;
  for (u32 b = 1; b <= MSIM_FLAG_JOURNAL_OVERFLOW; b <<= 1) if (hb((my_flags & b) != 0, hi)) flags |= b;
  u32 eo_l = lane; if (FLOOD) MSIM_OPAQUE(eo_l);   // (FLOOD: not even the lane-derived index is carried through the rounds)
  const u32 inst_out = FLOOD ? blockIdx.x * 2u + (eo_l >> 5) : inst;   // (real: the same; FLOOD: recomputed from the lane, nothing is kept across the rounds for it)
  if (real && i == 0) {
    // every client RPC is a request and a reply, each sent and received once (no loss, no timeouts in this layout)
    msim_net_stats st;
    st.clients_send = 2ull * t_cl; st.clients_recv = 2ull * t_cl;
    st.servers_send = t_arr; st.servers_recv = FLOOD ? t_arr - t_rsv : t_rsv;   // (FLOOD: n_rsv holds what stayed undelivered, see TRIM (A))
    st.all_send = st.clients_send + st.servers_send; st.all_recv = st.clients_recv + st.servers_recv;
    p.stats[inst_out] = st;
    msim_inst_meta m; m.n_rows = n_rows; m.n_payload_words = n_payload; m.flags = flags; m.n_rounds = rounds;
    m.n_events = 0; m.reserved[0] = 0; m.reserved[1] = 0; m.reserved[2] = 0;
#ifdef DUO_PROF
    // GENERAL bodies | op rounds << 16, wave-rounds | the reads of both clusters that ran inside a read run << 16, their cycles / 1024
    // (GENERAL | op << 16: 5 bits, saturating: generic op rounds are rare) | quiet op rounds << 21 (11 bits, saturating; they are among the
    // flood op rounds), all cycles / 4096 | parks << 16 (11 bits) | the longest wait of a parked half << 27 (5 bits, saturating) (tools/duo_prof_report.py)
    // the wavefront's upper instance: flood gossip rounds | parked gossip rounds << 16, flood op rounds | op wave-rounds with two ops << 16
    // (12 bits) | materialisations << 28 (4 bits, saturating; their cycles are part of the GENERAL bodies'), cycles / 1024 (flood gossip
    // rounds | the leaving rounds' R0 << 16), cycles / 1024 (flood op rounds | parked gossip rounds << 16)
    // with -DDUO_PROF_STRETCH as well, the lower instance carries instead of the GENERAL bodies' and op rounds' figures: flood stretches |
    // the rounds taken inside them << 16, and generic gossip rounds | their cycles / 1024 << 16 (tools/duo_prof_report.py with STRETCH=1)
    // with -DDUO_PROF_STEADY as well, the lower instance carries instead of the GENERAL bodies' and generic op rounds' cycles and the quiet
    // count: steady parks (11 bits, saturating; they are among the parks) | steady leaves << 11 (11 bits, saturating) | the cycles of both,
    // from the stretch's exit on, / 4096 << 22 (10 bits, saturating) (tools/duo_prof_report.py with STEADY=1)
    (void)pf_mat; (void)pf_nst; (void)pf_nstr; (void)pf_ngg; (void)pf_gg; (void)pf_nspark; (void)pf_nsleave; (void)pf_sx; (void)pf_nrec; (void)pf_nrep; (void)pf_nbout; (void)pf_ndrop;
    if (!hi) { m.n_events = pf_ngen | (pf_nop << 16); m.reserved[0] = pf_nwave | (pf_nrun_all << 16); m.reserved[1] = ((u32)(pf_gen >> 10) & 0xFFFFu) | (min((u32)(pf_op >> 10), 31u) << 16) | (min(pf_nquiet, 2047u) << 21);
               m.reserved[2] = ((u32)(pf_tot >> 12) & 0xFFFFu) | (min(pf_npark, 2047u) << 16) | (min(pf_wmax, 31u) << 27);
#ifdef DUO_PROF_STEADY
               m.reserved[1] = min(pf_nspark, 2047u) | (min(pf_nsleave, 2047u) << 11) | (min((u32)(pf_sx >> 12), 1023u) << 22);
#endif
#ifdef DUO_PROF_STRETCH
               m.n_events = min(pf_nst, 65535u) | (min(pf_nstr, 65535u) << 16); m.reserved[1] = min(pf_ngg, 65535u) | (min((u32)(pf_gg >> 10), 65535u) << 16);
#endif
             }
    else { m.n_events = pf_nfg | (pf_npk << 16); m.reserved[0] = pf_nfop | (min(pf_nop2, 4095u) << 16) | (min(pf_nmat, 15u) << 28); m.reserved[1] = ((u32)(pf_fg >> 10) & 0xFFFFu) | ((u32)(pf_exit >> 10) << 16);
           m.reserved[2] = ((u32)(pf_fop >> 10) & 0xFFFFu) | ((u32)(pf_pk >> 10) << 16); }
#ifdef DUO_PROF_MEMO
    // with -DDUO_PROF_MEMO as well, BOTH instances carry in reserved[1], instead of cycles: the cluster's replayed floods (16 bits, saturating) |
    // its broadcasts taken outside the quiet body << 16 (8 bits, saturating) | the floods the wavefront recorded << 24 (tools/duo_prof_report.py with MEMO=1);
    // the upper instance's reserved[2] is the number of recordings the wavefront dropped
    m.reserved[1] = min(pf_nrep, 65535u) | (min(pf_nbout, 255u) << 16) | (min(pf_nrec, 255u) << 24);
    if (hi) m.reserved[2] = pf_ndrop;   // (the upper instance, instead of the flood op rounds' and parked rounds' cycles: the recordings the wavefront dropped)
#endif
#ifdef DUO_PROF_RUN
    // with -DDUO_PROF_RUN as well, the lower instance's reserved[2] carries, instead of all cycles, the parks and the longest wait: the iterations
    // of the runs' loop (16 bits, saturating) | the broadcasts of both clusters taken in runs << 16 (tools/duo_prof_report.py with MEMO=1 RUN=1)
    if (!hi) m.reserved[2] = min(pf_nit, 65535u) | (min(pf_nrunb_all, 65535u) << 16);
#ifdef DUO_PROF_PLAN
    // with -DDUO_PROF_PLAN as well (every word of the -DDUO_PROF_RUN build is taken), the upper instance's reserved[2] carries, instead of the
    // recordings dropped: the block plans that took an op (16 bits, saturating) | the ops they took << 16 (reads and broadcasts of both
    // clusters; they are among the runs' reads and broadcasts, so the loop's own ops are those less these) (tools/duo_prof_report.py with PLAN=1)
    else m.reserved[2] = min(pf_nplan, 65535u) | (min(pf_nplanop, 65535u) << 16);
#endif
#endif
    (void)pf_nrunb_all; (void)pf_nit; (void)pf_nplan; (void)pf_nplanop;
#endif
#if defined(DUO_PROF2) || defined(DUO_PROF3)
    if (!hi) { m.n_events = (u32)(p2[0] >> 6); m.reserved[0] = (u32)(p2[1] >> 6); m.reserved[1] = (u32)(p2[2] >> 6); m.reserved[2] = (u32)(p2[3] >> 6); }
    else { m.n_events = (u32)(p2[4] >> 6); m.reserved[0] = (u32)(p2[5] >> 6); m.reserved[1] = (u32)(p2[6] >> 6); m.reserved[2] = (u32)(p2[7] >> 6); }
#endif
    p.meta[inst_out] = m;
  }
  // FLOOD TABLE: the launch that makes the table is this one wavefront; what its recording path has left in LDS becomes the context's
  // table (the row of an origin whose recording never ended is there as well, and no bit of mm_known stands for it)
  if constexpr (MEMO && DUO_TABLE_ON) {
    if (dp.table_fill != 0u && dp.table != nullptr) {
      DUO_LANE_NOW(tf_l);
      const uint4 *const tf_src = reinterpret_cast<const uint4 *>(smem + dp.off_memo);
      uint4 *const tf_dst = reinterpret_cast<uint4 *>(dp.table + DUO_TABLE_HDR);
#pragma unroll
      for (u32 k = 0; k < 3u; k++) if (tf_l + 64u * k < DUO_TABLE_COPY16) tf_dst[tf_l + 64u * k] = tf_src[tf_l + 64u * k];
      if (tf_l == 0u) reinterpret_cast<uint4 *>(dp.table)[0] = make_uint4(mm_known, BPLAN ? mm_full : 0u, N, p.cfg.topology | (dp.echoback << 8));
    }
  }
}

}  // namespace

// Extra per-instance scratch words: the cluster's node sets, W words x 32 lanes (duo.hip's set region; 128-byte aligned by scratch_words())
uint64_t msim_duo_extra_scratch_words(const msim_config &c) { return (uint64_t)(c.max_values / 32u) * 32u; }

// Whether the duo layout simulates this configuration (see the header of this file).
bool msim_duo_eligible(const msim_config &c) {
  if (c.node_program != MSIM_NODE_BCAST_FF && c.node_program != MSIM_NODE_BCAST_FF_ECHOBACK) return false;
  if (c.n_nodes > 32 || c.concurrency != c.n_nodes) return false;
  if (c.p_loss_q32 != 0 || c.nemesis_mask != 0 || c.journal_capacity != 0) return false;
  // an RPC completes within one (maximal) latency of virtual time: no client timeout can fire (client.clj:96-103, db.clj:54).
  // constant: the mean; uniform: below 2 x mean; exponential: mean x -ln(2^-32) < 22.2 x mean
  const uint64_t worst = c.latency_dist == MSIM_LAT_CONSTANT ? c.latency_mean_ms : c.latency_dist == MSIM_LAT_UNIFORM ? 2ull * c.latency_mean_ms : 23ull * c.latency_mean_ms;
  if (worst >= c.client_timeout_ms || worst >= 10000u) return false;
  if (c.latency_dist != MSIM_LAT_CONSTANT && (uint64_t)c.inbox_capacity + c.spill_capacity >= 16384u) return false;   // 16-bit arrival sequence numbers
  if (c.max_values > 65536u) return false;   // a value travels in 16 bits of the envelope word
  return true;
}

static uint32_t duo_degree(const msim_config &c) {
  uint32_t d = 0;
  for (uint32_t a = 0; a < c.n_nodes; a++) {
    uint32_t m = 0, n = c.n_nodes;
    switch (c.topology) {   // same shapes as topo_adj (broadcast.clj:40-185)
      case MSIM_TOPO_GRID: { uint32_t side = 1; while (side * side < n) side++; const uint32_t i = a / side, j = a % side;
        m = (j + 1 < side && a + 1 < n) + (j > 0) + (a + side < n) + (i > 0); } break;
      case MSIM_TOPO_LINE: m = (a + 1 < n) + (a > 0); break;
      case MSIM_TOPO_TOTAL: m = n - 1; break;
      default: { const uint32_t b = c.topology == MSIM_TOPO_TREE2 ? 2 : c.topology == MSIM_TOPO_TREE3 ? 3 : 4;
        m = a > 0; for (uint32_t k = 1; k <= b; k++) m += b * a + k < n; }
    }
    if (m > d) d = m;
  }
  return d;
}

template <bool LAT0, bool DEG4, bool RND>
static hipError_t duo_launch(const DuoParams &dp, dim3 grid, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&sim_kernel_duo<LAT0, DEG4, RND>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sim_kernel_duo<LAT0, DEG4, RND>), grid, dim3(64), lds, st, dp);
  return hipGetLastError();
}

// Launches the duo kernel for n clusters on `st`; returns MSIM_LAYOUT_DOES_NOT_FIT if the cluster state does not fit (the caller
// then runs the one-cluster-per-wavefront kernels).  `fill`: the launch that makes the flood table kp.duo_table (product limits; nothing is
// launched, and *fill_memo stays false, where the configuration does not take the memo instantiation).
static hipError_t duo_launch_any(const KParams &kp, uint32_t n, hipStream_t st, bool fill, bool *fill_memo) {
  const msim_config &c = kp.cfg;
  DuoParams dp;
  dp.k = kp; dp.n_inst = n;
  const bool rnd = c.latency_dist != MSIM_LAT_CONSTANT;
  const bool lat0 = !rnd && c.latency_mean_ms == 0;
  const uint32_t cap_tot = c.inbox_capacity + c.spill_capacity;
  // LDS of one cluster = [queues]; the node sets live in HBM scratch (msim_duo_extra_scratch_words).  The
  // queues are sized by the rule of the layout that kept the sets in LDS too: as many ring entries per node as fit beside the sets in
  // 10 KiB per cluster, at least 8, at most inbox_capacity (rounded up to a power of two); what does not fit goes to the HBM spill area.
  // R, S and with them the fit test below (and so which kernel runs a configuration) are the same as then; only the sets' bytes left.
  // Three launches of 4096 clusters resident at once want 24 wavefronts per CU (6 per SIMD, what the registers of the lat-0
  // instantiation allow), at most 6.8 KB of LDS each.  The headline shape (lat 0, inbox 6: R = 8) takes 2 KiB per wavefront; constant
  // latency > 0 (R = 16: 8 KiB, 20 per CU = the 5 per SIMD its registers allow) and RND (9.4 KB) shrink by the sets as well.
  const size_t set_bytes_v1 = (((size_t)kp.N * (kp.W | 1u) + 32) * 4 + 15) & ~(size_t)15;   // what the sets took of the LDS budget
  const size_t fixed = set_bytes_v1;
  const size_t per_entry = rnd ? 0 : (size_t)32 * (lat0 ? 4 : 8);   // (RND: bags of a fixed 16 entries)
  const size_t budget = (20 * 1024 - (rnd ? 257 * 4 + 16 : 0)) / 2;
  uint32_t R = rnd ? DUO_BAG : 8;
  while (!rnd && R < 64 && R < cap_tot && fixed + ((per_entry * (R * 2) + 15) & ~(size_t)15) + 32 <= budget && (rnd || R < c.inbox_capacity)) R <<= 1;
  if (!rnd && R > cap_tot) { R = 2; while (R * 2 <= cap_tot) R <<= 1; }
  if (rnd && R > cap_tot) R = cap_tot ? cap_tot : 1;
  dp.S = cap_tot > R ? cap_tot - R : 0;
  // the spill area is spill_capacity x 16 bytes per node: 8-byte ring entries (constant latency) or 12-byte bag entries (RND)
  if ((size_t)dp.S * (rnd ? 12 : 8) > (size_t)c.spill_capacity * 16) return MSIM_LAYOUT_DOES_NOT_FIT;
  if (rnd) MSIM_UPLOAD_ONCE(duo_log2_q24, msim_log2_q24, sizeof(msim_log2_q24));   // (1 KiB, once per device)
  size_t off = 0;
  dp.off_ring = (u32)off; off += rnd ? (size_t)(kp.N + 1) * DUO_BAG * 8 : (size_t)32 * R * (lat0 ? 4 : 8);
  dp.off_seq = (u32)off; if (rnd) off += (((size_t)(kp.N + 1) * DUO_BAG * 2) + 15) & ~(size_t)15;
  dp.R = R;
  off = (off + 15) & ~(size_t)15;
  dp.half_bytes = (u32)off;
  // the fit test of the layout that kept the sets in LDS, unchanged: which kernel runs a configuration does not depend on where the sets live
  if (2 * (off + set_bytes_v1) + (rnd ? 257 * 4 + 12 : 0) > 160 * 1024) return MSIM_LAYOUT_DOES_NOT_FIT;
  // the set regions: the last msim_duo_extra_scratch_words(c) words of every instance's scratch (scratch_words() of engine.hip adds them
  // last), reached with 32-bit byte offsets from the wavefront's lower cluster.  A finalized configuration's scratch stays far below
  // 2 GiB per instance (spill <= 32 nodes x 65536 envelopes x 16 B, queues bounded by the LDS check of msim_run, max_values <= 8160):
  // the test below cannot fail for one that reaches this kernel.
  if (kp.scratch_words * 4 >= (1ull << 31)) return MSIM_LAYOUT_DOES_NOT_FIT;
  // TRIM (C): rows and payload of a wavefront's two clusters are reached with 32-bit byte offsets from the lower cluster's
  if (2ull * c.max_rows * 16ull >= (1ull << 32) || 2ull * c.max_payload_words * 4ull >= (1ull << 32)) return MSIM_LAYOUT_DOES_NOT_FIT;
  dp.sets_off = (u32)(kp.scratch_words - msim_duo_extra_scratch_words(c));
  dp.inst_bytes = (u32)(kp.scratch_words * 4);
  const bool deg4 = duo_degree(c) <= 4 && kp.N <= 31;   // (lane 31 must hold no node: unused neighbour slots point at it)
  // the flood instantiation keeps each cluster's block of 32 generator draws in LDS, behind its queues (256 bytes; lat 0 rings are at most
  // 8 KiB per cluster, so this never decides the fit test above: which kernel runs a configuration stays as it was)
  dp.off_dc = 0;
  if (DUO_FLOOD_ON && lat0 && deg4) { dp.off_dc = (u32)off; off += 32 * 8; dp.half_bytes = (u32)off; }
  dp.off_log2 = (u32)(2 * off);
  // the memo instantiation's table of remembered floods, one per wavefront, behind both clusters' regions (the headline shape: 2560 + 2048
  // bytes per wavefront, 24 wavefronts per CU as before; the fit test above is not touched: which kernel runs a configuration stays as it was)
  const bool memo = DUO_MEMO_BUILD && lat0 && deg4;
  dp.off_memo = memo ? (u32)(2 * off) : 0u;
  dp.deg = duo_degree(c);
  dp.echoback = c.node_program == MSIM_NODE_BCAST_FF_ECHOBACK;
  dp.round_limit = (kp.dev_flags & 0x100u) ? 2000000u : ROUND_LIMIT;
  // developer / tests: MSIM_DUO_ROUND_LIMIT=<rounds> stops every cluster of this layout at that round (MSIM_FLAG_ROUND_LIMIT), so that the
  // limit can be made to fall anywhere, e.g. inside a run of reads (read at every launch: a test sweeps it within one process)
  bool dev_limit = false;
  if (const char *rl = std::getenv("MSIM_DUO_ROUND_LIMIT")) { const unsigned long v = std::strtoul(rl, nullptr, 0); if (v > 0 && v < ROUND_LIMIT) { dp.round_limit = (u32)v; dev_limit = true; } }
  // the flood table: read by the memo instantiation alone; the launch that makes it runs under the product's round limit.  A launch under
  // MSIM_DUO_ROUND_LIMIT starts from empty tables, as before: WHERE a cluster that the limit stops is stopped follows the alignment of the
  // two halves' rounds (a half's limit is looked at where R0's block is entered), a half that replays its first floods is aligned with
  // its partner otherwise than one that records them, and the limit sweeps of the tests hold builds against each other limit for limit,
  // stopped instances included (measured with the table under the limits, -DDUO_PAIR_WAIT=2, two headline clusters: the same flags and
  // unflagged instances everywhere, a stopped cluster stopped up to three rounds later at 37 of the 121 limits; at the default wait none)
  // MSIM_DUO_TABLE_UNDER_LIMIT=1 (developer / tests, read at every launch like the limit): such a launch reads the table all the same, so that
  // a test can hold the replay from a table's record against the build without the table near a limit (flags and unflagged instances).
  if (dev_limit) { const char *tu = std::getenv("MSIM_DUO_TABLE_UNDER_LIMIT"); if (tu && std::strtoul(tu, nullptr, 0) != 0) dev_limit = false; }
  dp.table = memo && DUO_TABLE_ON && (fill || !dev_limit) ? kp.duo_table : nullptr;   // (a context's table is made whatever the first launch runs under)
  dp.table_fill = fill ? 1u : 0u;
  if (fill) {
    if (!dp.table) return hipSuccess;
    *fill_memo = true;
    dp.round_limit = ROUND_LIMIT;
  }
  size_t lds = 2 * off + (rnd ? 257 * 4 + 12 : 0);
  if (memo) lds += DUO_MEMO_BYTES;
  if (memo && DUO_BPLAN_ON) lds += DUO_BPLAN_BYTES;   // the block plan's totals per origin, behind the table (4736 bytes per wavefront at the headline shape)
  lds = std::min(lds + (size_t)DUO_LDS_PAD, (size_t)160 * 1024);
  const dim3 grid((n + 1) / 2);
  if (rnd) return deg4 ? duo_launch<false, true, true>(dp, grid, lds, st) : duo_launch<false, false, true>(dp, grid, lds, st);
  if (lat0) return deg4 ? duo_launch<true, true, false>(dp, grid, lds, st) : duo_launch<true, false, false>(dp, grid, lds, st);
  return deg4 ? duo_launch<false, true, false>(dp, grid, lds, st) : duo_launch<false, false, false>(dp, grid, lds, st);
}

hipError_t msim_launch_duo(const KParams &kp, uint32_t n, hipStream_t st) { return duo_launch_any(kp, n, st, false, nullptr); }

// Makes the flood table of a context (see "FLOOD TABLE" and wave_common.h): one wavefront, two clusters `first` and `first` + 1 of the
// configuration on slabs of their own, which are freed again; the table comes from the library's allocator like every slab.
hipError_t msim_duo_make_flood_table(const KParams &plan_kp, uint64_t first, hipStream_t st, u32 **table, u32 *origins) {
  *table = nullptr; *origins = 0;
  const msim_config &c = plan_kp.cfg;
  if (!(DUO_TABLE_ON && DUO_MEMO_BUILD) || !msim_duo_eligible(c)) return hipSuccess;
  // (whether the configuration takes the memo instantiation is the launcher's to say: *fill_memo below)
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_rows = up(2 * (size_t)c.max_rows * sizeof(msim_op)), b_pay = up(2 * (size_t)c.max_payload_words * 4);
  const size_t b_stats = up(2 * sizeof(msim_net_stats)), b_meta = up(2 * sizeof(msim_inst_meta)), b_scr = up(2 * (size_t)plan_kp.scratch_words * 4);
  unsigned char *slab = nullptr; u32 *tab = nullptr;
  hipError_t e = msim_dev_malloc(&tab, DUO_TABLE_BYTES);
  if (e == hipSuccess) e = msim_dev_malloc(&slab, b_rows + b_pay + b_stats + b_meta + b_scr);
  if (e == hipSuccess) e = hipMemsetAsync(tab, 0, DUO_TABLE_BYTES, st);
  // (MSIM_POISON: the wavefront's own slabs start from the byte the context's slabs start from, the table does not)
  if (e == hipSuccess && msim_poison_byte() >= 0) e = hipMemsetAsync(slab, msim_poison_byte(), b_rows + b_pay + b_stats + b_meta + b_scr, st);
  bool memo = false;
  if (e == hipSuccess) {
    KParams kp = plan_kp;
    kp.first_instance = first;
    unsigned char *q = slab;
    kp.rows = reinterpret_cast<msim_op *>(q); q += b_rows;
    kp.payload = reinterpret_cast<u32 *>(q); q += b_pay;
    kp.stats = reinterpret_cast<msim_net_stats *>(q); q += b_stats;
    kp.meta = reinterpret_cast<msim_inst_meta *>(q); q += b_meta;
    kp.scratch = reinterpret_cast<u32 *>(q);
    kp.journal = nullptr; kp.duo_table = tab;
    e = duo_launch_any(kp, 2, st, true, &memo);
    if (e == MSIM_LAYOUT_DOES_NOT_FIT) e = hipSuccess;   // (the launches of this context take other kernels)
  }
  u32 hdr[DUO_TABLE_HDR] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && memo) e = hipMemcpy(hdr, tab, sizeof(hdr), hipMemcpyDeviceToHost);
  if (slab) { const hipError_t ef = msim_dev_free(slab); if (e == hipSuccess) e = ef; }
  if (e == hipSuccess && memo && (hdr[2] != plan_kp.N || hdr[3] != (c.topology | ((c.node_program == MSIM_NODE_BCAST_FF_ECHOBACK ? 1u : 0u) << 8)))) e = hipErrorUnknown;   // (the wavefront did not reach its epilogue)
  if (e != hipSuccess || !memo) { if (tab) (void)msim_dev_free(tab); return e; }
  *table = tab; *origins = hdr[0];
  return hipSuccess;
}
