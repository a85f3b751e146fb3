// dtg4.hip — FOUR clusters of the Datomic-style txn-list-append node with SEVERAL WORKERS PER NODE per wavefront: demo/ruby/datomic_list_append.rb
// as the reference's own runs invoke it (doc/05-datomic/01-single-node.md:257,322: one node, --concurrency 10n), in 16-lane groups.
//
// Same program and the same rounds as dtg_kernel<> (sim_kernel_dtg.inc; specification: oracle/dt_nodes.inc): the node's lock and its arrival-order
// waiting queue, the persistent hash tree in lww-kv, the root pointer in lin-kv, Promise#await's 5 s — its node and services are the same text,
// dt_node.inc / dt_input.inc (the node's index is its lane in the group).  What changes is the mapping, as in txng4.hip / svc4.hip (the time step, the network, the
// partition nemesis and the history rows are shared: group16.h, group16_*.inc): a cluster is n nodes + its worker slots + lin-kv + lww-kv <= 16 endpoints, one lane each of a 16-lane
// group — 1 node with 10 workers is 13 — and a wavefront carries four clusters.
//
// Scope (engine.hip picks this kernel when all of it holds, else dtg_kernel<> runs): concurrency a multiple of n above n, n + concurrency + 2 <= 16,
// net journal off, at least MSIM_DTG4_MIN_CLUSTERS clusters in the launch (half of that with two nodes or more).
//
// LDS of a wavefront: envelope queues slot-major (RQ envelopes per endpoint, the rest spills to HBM), per node the lock holder's cursor, the waiting
// ring of 64 transactions and the save stack (DG_WORDS words), per cluster the generator's key pool and the nemesis shuffle.  Tree records, write
// lists, the cas tables and the append log live in HBM scratch (dt_kernel<>'s layout); history rows go straight to HBM.
//
// Envelope (16 B): x = deadline, y = (id << 8) | type, z = a, w = b | (src << 24); src = the sender's lane in its group (lin-kv: n + slots, lww-kv: + 1).
#include <hip/hip_runtime.h>

#include "sim_kernels.h"
#include "group16.h"

namespace {

constexpr u32 GS = 16u;           // lanes per cluster
#ifndef D4_RQ
#define D4_RQ 2u
#endif
#ifndef D4_WAVES
#define D4_WAVES 4
#endif
constexpr u32 RQ = D4_RQ;         // LDS envelopes per endpoint
constexpr u32 D4_CLIENT_CAP = 32u;   // Reusable lin-kv clients (lin_kv.clj:74-76) collect late replies between RPCs (the oracle's limit)
struct D4Params {
  KParams k;
  u32 n_inst;
  u32 off_curs, off_gen, off_misc;   // LDS byte offsets (queues at 0)
  u32 node_spill, client_spill;               // HBM spill entries per server endpoint / client behind the RQ LDS slots
  u64 client_spill_off;                       // word offset of the clients' spill area inside the per-instance scratch
  u32 round_limit;
};

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(D4_WAVES))) dtg4_kernel(const D4Params rp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const KParams &p = rp.k;
  const u32 lane = threadIdx.x, l = lane & (GS - 1u), grp = lane >> 4, gbase = lane & 48u;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const u32 LIN = N + CS;                                                     // lane of lin-kv in the group; lww-kv is LIN + 1
  const bool is_node = l < N;
  const bool is_client = l >= N && l < N + CS;
  const bool is_lin = l == LIN, is_lww = l == LIN + 1u;
  const bool is_server = is_node || is_lin || is_lww;   // endpoints that poll all the time and see latency
  const u32 slot = l - N;
  const bool is_worker = is_client && slot < C;
  const u32 inst_raw = blockIdx.x * 4u + grp;
  const bool real = inst_raw < rp.n_inst;
  const u32 inst = real ? inst_raw : rp.n_inst - 1u;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt = (1u << l) - 1u;
  const u32 worker_mask = ((1u << C) - 1u) << N;
  const u32 all_nodes = (1u << N) - 1u;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key, mv = p.cfg.max_values;
  const u32 TC = p.mk_tcap;   // tree nodes a node may create
  const u32 rpc_timeout_ms = p.cfg.client_timeout_ms;
  const u32 round_limit = rp.round_limit;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_kv = g_scr;                                           // [max_values][mw]: element | version << 8
  u32 *const g_kvn = g_kv + (size_t)mv * mw;                         // [max_values]
  u32 *const g_first = g_kvn + mv;                                   // [max_values] version at which the key entered the tree (DT_NONE: never)
  unsigned char *const g_hash = reinterpret_cast<unsigned char *>(g_first + mv);   // [max_values] Tree.hash of the key
  u32 *const g_rec = g_scr + (((size_t)mv * mw + 2u * mv + (mv + 3u) / 4u + 3u) & ~(size_t)3);   // [N][TC][DT_RW] tree nodes by pointer, on a 16-byte boundary
  u32 *const g_wl = g_rec + (size_t)N * TC * DT_RW;                  // [N][DT_MAXW] the pointers a node writes this round
  u32 *const g_cas = g_wl + (size_t)N * DT_MAXW;                     // [N][DT_CASQ] x {msg_id, from, transaction}: what a node's cas requests carry beside `to`
  const u32 my_spill_cap = is_server ? rp.node_spill : (is_client ? rp.client_spill : 0u);
  uint4 *const my_spill = is_server ? reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)(is_node ? l : N + (l - LIN)) * rp.node_spill
                                    : reinterpret_cast<uint4 *>(g_scr + rp.client_spill_off) + (size_t)(is_client ? slot : 0) * rp.client_spill;

  // LDS
  uint4 *const my_q = reinterpret_cast<uint4 *>(smem) + lane;                                         // slot s at my_q[s * 64]
  u32 *const curs_g = reinterpret_cast<u32 *>(smem + rp.off_curs) + grp * N * DG_WORDS;                 // [node of the group][DG_WORDS]
  u32 *const cu = curs_g + (is_node ? l : 0) * DG_WORDS;
  u32 *const my_wl = g_wl + (size_t)(is_node ? l : 0) * DT_MAXW;
  u32 *const gen = reinterpret_cast<u32 *>(smem + rp.off_gen) + grp * 36;                             // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + rp.off_misc) + grp * GS;

  for (u32 i = lane; i < 4 * N * DG_WORDS; i += 64) reinterpret_cast<u32 *>(smem + rp.off_curs)[i] = 0;
  gen[l] = l; gen[16 + l] = 1;
  if (l == 0) gen[32] = p.cfg.key_count;
  if (real) {
    for (u32 i = l; i < mv; i += GS) { g_kvn[i] = 0; g_first[i] = DT_NONE; g_hash[i] = (unsigned char)dt_hash(i); }
    for (u32 i = l; i < N * DT_CASQ * 3u; i += GS) g_cas[i] = 0;
  }
  __syncthreads();

  // ---- endpoint state ----
  bool has_c = false; u32 deliver_at = 0; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, part = 0;
  u32 node_msgid = 0;
  u32 next_p = 0;                                      // node: @ptr (:332, :352-355)
  u32 wait_until = INF;                                // node: when the lock holder's Promise#await gives up (promise.rb:5,17-30), INF: not waiting
  u32 casn = 0;                                        // node: cas requests so far
  u32 root = 0, root_exists = 0, cur_v = 0;            // lin-kv lane: the root pointer; versions so far
  u32 svc_ctr = 0;                                     // lww-kv lane: rand-int draws so far
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_value = 0, process = slot, m_value = 0;
  const u32 dest_node = is_client ? slot % N : 0u;     // worker t -> node t mod N; a crashed process's successor (process + C) keeps it, C being a multiple of N
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- per-cluster state (uniform within a group) ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  bool alive = real;

#define SERVER_SRC(src) ((src) < N || (src) >= LIN)   // whether sender lane src is a server: the nodes, lin-kv and lww-kv
  #include "group16_net.inc"
  auto visible = [&](u32 k, u32 from) -> u32 {
    const u32 cnt = g_kvn[k];
    u32 n = 0;
    while (n < cnt && (g_kv[k * mw + n] >> 8) <= from) n++;
    return n;
  };

  for (;;) {
    if (!__ballot(alive)) break;

    #include "group16_phase.inc"
    if (alive && GB((my_flags & MSIM_FLAG_ARENA_OVERRUN) != 0)) alive = false;   // an engine capacity was exceeded: what follows would not be the program's behaviour

    #include "group16_time.inc"
    my_t = min(my_t, wait_until);   // (a node's timer is a normal event)
    #include "group16_jump.inc"

    bool inv_row = false; u32 inv_packed = 0, inv_value = 0, inv_len = 0;
    bool cmp_row = false; u32 cmp_packed = 0, cmp_value = 0, cmp_len = 0;
    u32 nem_rows = 0, nem_f = 0, nem_v1 = 0, nem_v2 = 0, nem_len2 = 0;

    auto complete = [&](u32 type, u32 err, u32 ref) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (MSIM_F_TXN << 2) | (err << 7) | (process << 12);
      cmp_value = ref & 0xFFFFFFu; cmp_len = ref >> 24;
      if (type == MSIM_T_INFO) process += C;  // crashed process; the Reusable client itself lives on
    };

    if (alive && timeout_round) {
      if (busy && timeout_at <= T) complete(MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_value);
    }
    bool normal = alive && !timeout_round;   // this cluster runs R1-R4 in this wave-round
    if (__ballot(normal)) {
      // ---- R1: scheduler ----
      const bool act = normal && due <= T;
      if (__ballot(act && phase == PH_INIT)) {
        if (act && phase == PH_INIT) { if (is_client && slot < N) { mark = true; kind = K_INIT; } phase = PH_INIT_WAIT; }
      }
      #include "group8_nemesis.inc"
      {
        const bool gen_now = act && phase == PH_MAIN && gen_live && gen_next <= T && free_mask != 0;
        if (__ballot(gen_now)) {
          const u32 nfree = __popc(free_mask);
          const u32 kk = gen_k;
          const u64 h = draw64(key, S_GEN, kk);
          const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
          const u32 pick = scale32(r_lo, nfree);
          const bool sel = gen_now && is_worker && !busy && (u32)__popc(free_mask & lt) == pick;
          // the transaction ([upstream] elle list-append gen): lane 0 of the group writes the micro-ops and owns the key pool
          const u32 n_mops = 1 + scale32((u32)(draw64(key, S_GEN2, kk) >> 32), p.cfg.max_txn_length);
          u32 bad = 0;
          if (gen_now && n_payload + n_mops > max_pay) bad = MSIM_FLAG_PAYLOAD_OVERFLOW;
          else if (gen_now && l == 0) {
            const u32 kc = p.cfg.key_count;
            for (u32 j = 0; j < n_mops; j++) {
              const u64 h3 = draw64(key, S_GEN3, (u64)kk * 8 + j);
              const u32 x = scale32((u32)(h3 >> 32), (1u << kc) - 1) + 1;
              const u32 ki = 31 - (u32)__clz((int)x);
              const u32 k = gen[ki];
              if (h3 & 1) {
                const u32 v = gen[16 + ki];
                gen[16 + ki] = v + 1;
                g_pay[n_payload + j] = 1u | (k << 1) | (v << 16);
                if (v + 1 > mw) {
                  const u32 nk = gen[32];
                  if (nk >= p.cfg.max_values) { bad = MSIM_FLAG_VALUES_OVERFLOW; break; }
                  gen[ki] = nk; gen[32] = nk + 1; gen[16 + ki] = 1;
                }
              } else g_pay[n_payload + j] = (k << 1) | (0xFFu << 16);
            }
          }
          bad = GGET(bad, 0);
          if (gen_now && bad) { flags |= bad; phase = PH_DONE; alive = false; normal = false; }
          if (sel && !bad) { mark = true; kind = K_OP; m_value = n_payload | (n_mops << 24); }
          if (gen_now && !bad) { gen_k++; n_payload += n_mops; gen_next = T + __umulhi(r_hi, p.gen_period2_us); }
        }
      }

      // ---- R2: marked clients invoke ----
      if (__ballot(mark && normal)) {
        const bool inv = mark && normal;
        u32 rq_dest = 0, rq_type = 0, rq_a = 0;
        if (inv) {
          mark = false; busy = true;
          if (kind == K_INIT) { rq_dest = slot; rq_type = M_INIT; next_msg_id = 0; }
          else {
            c_value = m_value;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (MSIM_F_TXN << 2) | (process << 12); inv_value = c_value & 0xFFFFFFu; inv_len = c_value >> 24;
            rq_dest = dest_node; rq_type = M_TXN; rq_a = c_value;
          }
          want = ++next_msg_id;
          timeout_at = T + (kind == K_OP ? rpc_timeout_ms : 10000u) * 1000u;
          s_send_cl++;
        }
        const u32 rq_pack = rq_dest | (rq_type << 8);
        u32 im = GB(inv);
        const u32 n_inv = __popc(im);
        u32 idx = 0;
        while (__ballot(im != 0)) {
          const bool on = im != 0;
          const u32 s = on ? (u32)__builtin_ctz(im) : 0u; im &= im - 1u;
          const u32 pk = GGET(rq_pack, s), a = GGET(rq_a, s), b = GGET(want, s);
          if (on && l == (pk & 0xFF)) arrive(next_id + idx, pk >> 8, a, b, s);
          idx++;
        }
        next_id += n_inv;
        poll();
      }

      // ---- R3: one input per node, then one for each service (endpoint order: lin-kv, lww-kv) ----
      bool rep = false, svc_rep = false;   // node -> a client, service -> node
      u32 r_to = 0, r_type = 0, r_a = 0, r_b = 0;    // the answer to the client
      u32 n_out = 0, o_dest = 0;           // node -> service: n_out messages, all to the same service; one in registers (o1_*) or DT_MAXW writes in my_wl[]
      u32 o1_type = 0, o1_a = 0, o1_b = 0, o_wlo = 0;
      u32 o_type = 0, o_a = 0, o_b = 0, o_to = 0, need_words = 0, done_ref = 0, done_rv = 0;   // service -> node; the completed transaction's payload
      auto reply = [&](u32 type, u32 a, u32 cmsg) { rep = true; r_type = type; r_a = a; r_to = cmsg >> 24; r_b = cmsg & 0xFFFFFFu; };   // (cmsg = the client's msg_id | its endpoint << 24)
      // what dt_node.inc / dt_input.inc ask of the kernel
#define REPLY_OK(type, cmsg) reply(type, 0, cmsg)
#define REPLY_ERROR(code, cmsg) reply(M_ERROR, code, cmsg)
#define CLIENT_REF(qb, qsrc) ((qb) | ((qsrc) << 24))   // a client is an endpoint: it rides in the top byte of the stored msg_id
#define NODE_IX l   // a node's index is its lane in the group
#define DT_WAIT_RING
      #include "dt_node.inc"

      const bool await_over = is_node && normal && wait_until <= T;   // a node's due timer comes before its due message
      const bool take = is_server && normal && !await_over && has_c && deliver_at <= T;
      if (await_over) {   // Promise#await gave up (promise.rb:24-29): RPCError.timeout => error 0 to the client (node.rb:172), the lock is free
        reply(M_ERROR, 0, cu[DC_CMSG]);
        unlock();
      } else if (take) {
        const uint4 q = cm; has_c = false;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        #include "dt_input.inc"
      }

      // completed transactions: payload words allocated in node order, each node writes its own
      if (__ballot(need_words != 0)) {
        const u32 incl = row_scan(need_words);
        const u32 total = GGET(incl, GS - 1u);
        #include "dt_reads.inc"
      }

      // COMMIT: ids in lane order (nodes, lin-kv, lww-kv); a node's messages in the order it emitted them: the answer to a client,
      // then what the next step sends to a service
      {
        const u32 rcnt = rep ? 1u : 0u;
        const u32 cnt = is_node ? rcnt + n_out : (svc_rep ? 1u : 0u);
        if (__ballot(cnt != 0)) {
          const u32 incl = row_scan(cnt);
          const u32 total = GGET(incl, GS - 1u);
          const u32 my_off = incl - cnt;
          if (is_node) { s_send_cl += rcnt; s_send_sv += n_out; } else s_send_sv += cnt;
          __syncthreads();   // (the write lists of this round are in HBM scratch; a workgroup is one wavefront)
          u32 ts = GB(is_node && cnt != 0);
          while (__ballot(ts != 0)) {   // every sending node in turn: its answer to a client (taken in by that client's lane), then its messages to a service (taken in by the service's lane)
            const bool on = ts != 0;
            const u32 s = on ? (u32)__builtin_ctz(ts) : 0u; ts &= ts - 1u;
            const u32 rc = GGET(rcnt, s), off = GGET(my_off, s);
            const u32 to = GGET(r_to, s), ty = GGET(r_type, s), a = GGET(r_a, s), b = GGET(r_b, s);
            if (on && rc && l == to) arrive(next_id + off, ty, a, b, s);
            const u32 kn = GGET(n_out, s);
            const u32 dst = GGET(o_dest, s), t1 = GGET(o1_type, s), a1 = GGET(o1_a, s), b1 = GGET(o1_b, s), wlo = GGET(o_wlo, s);
            if (on && kn && l == LIN + dst) {
              if (wlo == 0u) arrive(next_id + off + rc, t1, a1, b1, s);
              else { const u32 *const wl = g_wl + (size_t)s * DT_MAXW;
                for (u32 k = 0; k < kn; k++) arrive(next_id + off + rc + k, M_WRITE, wl[k], wlo + k, s); }
            }
          }
          // service -> node
          u32 sv = GB(svc_rep);
          while (__ballot(sv != 0)) {
            const bool on = sv != 0;
            const u32 s = on ? (u32)__builtin_ctz(sv) : 0u; sv &= sv - 1u;
            const u32 ty = GGET(o_type, s), a = GGET(o_a, s), b = GGET(o_b, s), d = GGET(o_to, s), off = GGET(my_off, s);
            if (on && l == d) arrive(next_id + off, ty, a, b, s);
          }
          next_id += total;
        }
        if (normal) poll();
      }

      // ---- R4: clients' recv! loops ----
      for (;;) {
        const bool dl = normal && is_client && has_c && deliver_at <= T;
        if (!__ballot(dl)) break;
        if (dl) {
          const uint4 q = cm; has_c = false;
          s_recv_cl++;
          const u32 qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
          if (busy && qb == want) {  // else stale (client.clj:105-107)
            if (qtype == M_TXN_OK) complete(MSIM_T_OK, 0, qa);
            else if (qtype == M_ERROR) {
              if (qa == 0u) complete(MSIM_T_INFO, MSIM_ERR_TIMEOUT, c_value);   // code 0 :timeout is not :definite? (errors.edn:2-4)
              else complete(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : qa == 30 ? MSIM_ERR_TXN_CONFLICT : qa == 14 ? MSIM_ERR_ABORT : MSIM_ERR_PRECONDITION_FAILED, c_value);
            } else complete(MSIM_T_OK, 0, c_value);  // init_ok
          }
          poll();
        }
      }
    }
    #include "group16_rows.inc"
  }

  #include "group16_stats.inc"
}

}  // namespace

// Whether four clusters per wavefront simulate this configuration (see the header of this file).
bool msim_dtg4_eligible(const msim_config &c) {
  if (c.node_program != MSIM_NODE_TXN_DATOMIC || c.journal_capacity != 0 || c.concurrency <= c.n_nodes) return false;
  return c.n_nodes >= 1 && c.n_nodes + c.concurrency + 2 <= GS;
}

// Extra per-instance scratch words the layout needs behind dtg_kernel<>'s spill area: the clients' whole inboxes and the part of the servers'
// LDS inboxes of dtg_kernel<> that does not fit this kernel's RQ slots.
uint64_t msim_dtg4_extra_scratch_words(const msim_config &c) {
  return ((uint64_t)(c.n_nodes + 2) * c.inbox_capacity + (uint64_t)c.concurrency * D4_CLIENT_CAP) * 4;
}

hipError_t msim_launch_dtg4(const KParams &kp, uint32_t n, hipStream_t st) {
  const msim_config &c = kp.cfg;
  D4Params rp;
  rp.k = kp; rp.n_inst = n;
  const uint32_t cap_tot = c.inbox_capacity + c.spill_capacity;
  rp.node_spill = cap_tot > RQ ? cap_tot - RQ : 0;             // <= spill_capacity + inbox_capacity entries per server endpoint
  rp.client_spill = D4_CLIENT_CAP > RQ ? D4_CLIENT_CAP - RQ : 0;
  rp.client_spill_off = kp.spill_off + (uint64_t)(kp.N + 2) * rp.node_spill * 4;
  size_t off = (size_t)RQ * 64 * 16;
  rp.off_curs = (u32)off; off += (size_t)4 * kp.N * DG_WORDS * 4;
  rp.off_gen = (u32)off; off += (size_t)4 * 36 * 4;
  rp.off_misc = (u32)off; off += 64 * 4;
  rp.round_limit = (kp.dev_flags & 0x100u) ? 4000000u : ROUND_LIMIT;
  const size_t lds = off;
  if (lds > 64 * 1024) return MSIM_LAYOUT_DOES_NOT_FIT;
  const bool rnd = c.latency_dist != MSIM_LAT_CONSTANT || c.p_loss_q32 != 0;
  if (rnd) MSIM_UPLOAD_ONCE(d_log2_q24, msim_log2_q24, sizeof(msim_log2_q24));   // (1 KiB, once per device)
  const dim3 grid((n + 3) / 4), block(64);
  if (c.nemesis_mask) { if (rnd) hipLaunchKernelGGL((dtg4_kernel<true, true>), grid, block, lds, st, rp); else hipLaunchKernelGGL((dtg4_kernel<true, false>), grid, block, lds, st, rp); }
  else { if (rnd) hipLaunchKernelGGL((dtg4_kernel<false, true>), grid, block, lds, st, rp); else hipLaunchKernelGGL((dtg4_kernel<false, false>), grid, block, lds, st, rp); }
  return hipGetLastError();
}
