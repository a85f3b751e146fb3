// sim_kernel_mkg.inc — the multi-key transactional node (sim_kernel_mk.inc: demo/js/multi_key_txn.js:1-246 over lin-kv + lww-kv) with SEVERAL
// WORKERS PER NODE (`--concurrency k n`).  Included by sim_kernels.h after sim_kernel_mk.inc, whose slot layout (SK_*) it
// uses and whose node and services are the same text (mk_node.inc, mk_input.inc, mk_reads.inc), in the lane layout of sim_kernel_dtg.inc / sim_kernel_txng.inc: a lane is an ENDPOINT — nodes 0 .. N-1,
// client worker slots N .. N+CS-1 (worker t talks to node t mod N), lin-kv at N+CS, lww-kv at N+CS+1 — every endpoint has a queue, clients
// poll only while an RPC is outstanding, COMMIT is receiver-side.  A node has up to MKG_SLOTS transactions in flight (with one worker per
// node: MK_SLOTS = 8, mk_kernel<> / mk8_kernel<>), the first MK_SL of them in LDS.
// Specification: oracle/mk_nodes.inc, bit for bit (tests/test_parity_gpu.py::test_multi_key_txn_many_workers_parity, tests/test_hipemu_parity.py).

#define MKG_SLOTS 64u

template <bool NEM, bool NET_RANDOM, int KEYS>
__global__ void __launch_bounds__(64) mkg_kernel(const KParams p) {
  constexpr u32 MK_KEYS = (u32)KEYS, MKW = 10u + 9u * MK_KEYS;
  constexpr u32 SK_WR = SK_KEY + MK_KEYS, SK_FA = SK_WR + MK_KEYS, SK_SORD = SK_FA + MK_KEYS, SK_NORD = SK_SORD + MK_KEYS, SK_RDRPC = SK_NORD + MK_KEYS,
                SK_RDTID = SK_RDRPC + MK_KEYS, SK_WRRPC = SK_RDTID + MK_KEYS, SK_WRTID = SK_WRRPC + MK_KEYS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const slots = reinterpret_cast<u32 *>(smem + p.off_seen);            // [N][MK_SL][MKW]: the transactions in flight (SK_*), slots 0 .. MK_SL-1
  u32 *const mout = slots + p.N * MK_SL * MKW;                              // [N][MK_KEYS][3]: what a node sends to a service this round {type, a, b}
  u32 *const gen = mout + p.N * MK_KEYS * 3u;                                // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const u32 LIN = N + CS;  // endpoint (= lane) of lin-kv; lww-kv is LIN + 1
  const bool is_node = lane < N, is_client = lane >= N && lane < LIN, is_lin = lane == LIN, is_lww = lane == LIN + 1u;
  const bool is_server = is_node || is_lin || is_lww;   // endpoints that poll all the time
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u64 lt_mask = (1ull << lane) - 1;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u32 all_nodes = (1u << N) - 1;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key, mw1 = mw + 1u, mv = p.cfg.max_values;
  const u32 TC = p.mk_tcap, CC = p.mk_ccap;   // thunks a node may create; slots of its thunk cache (a power of two)

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_kv = g_scr;                                           // [max_values][mw]: element | version << 8
  u32 *const g_kvn = g_kv + (size_t)mv * mw;                         // [max_values]
  u32 *const g_pos = g_kvn + mv;                                     // [max_values] position of the key in the root map
  u32 *const g_first = g_pos + mv;                                   // [max_values] version at which it entered (MK_NONE: never)
  u32 *const g_updn = g_first + mv;                                  // [max_values] thunks committed for the key
  u32 *const g_upd_v = g_updn + mv;                                  // [max_values][mw + 1] their versions
  u32 *const g_upd_t = g_upd_v + (size_t)mv * mw1;                   // [max_values][mw + 1] their ids
  u32 *const g_cache = g_upd_t + (size_t)mv * mw1;                   // [N][CC] the nodes' thunk caches
  unsigned char *const g_rep = reinterpret_cast<unsigned char *>(g_cache + (size_t)N * CC);   // [N][TC] replica holding thunk <node>.<i>
  u32 *const xslots = g_cache + (size_t)N * CC + (((size_t)N * TC + 15u) / 16u) * 4u;         // [N][MKG_SLOTS - MK_SL][MKW]: slots MK_SL .. MKG_SLOTS-1
  // slot si of node nd: LDS for the first MK_SL, HBM scratch beyond (a generic pointer: flat loads / stores reach both)
  auto slot_of = [&](u32 nd, u32 si) -> u32 * { return si < MK_SL ? slots + (nd * MK_SL + si) * MKW : xslots + ((size_t)nd * (MKG_SLOTS - MK_SL) + (si - MK_SL)) * MKW; };
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 qidx = is_node ? lane : is_lww ? N + 1u : N;   // queue of a server endpoint (lin-kv: N, lww-kv: N + 1)
  const u32 my_cap = is_server ? p.cap_node : T_CLIENT_CAP;
  const u32 my_spill_cap = is_server ? p.spill_cap : 0u;
  uint4 *const my_inbox = inbox + (is_server ? qidx * p.cap_node : is_client ? (N + 2) * p.cap_node + slot * T_CLIENT_CAP : 0u);
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qidx * p.spill_cap;
  const u32 my_node = is_node ? lane : 0u;
  u32 *const my_cache = g_cache + (size_t)(is_node ? lane : 0) * CC;

  for (u32 i = lane; i < N * MK_SL * MKW; i += 64) slots[i] = 0;
  for (u32 i = lane; i < N * (MKG_SLOTS - MK_SL); i += 64) xslots[(size_t)i * MKW + SK_HDR] = 0;
  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  for (u32 i = lane; i < mv; i += 64) { g_kvn[i] = 0; g_updn[i] = 0; g_first[i] = MK_NONE; g_pos[i] = MK_NONE; }
  for (u32 r = 0; r < N; r++) for (u32 i = lane; i < N * (TC >> 5); i += 64) g_cache[(size_t)r * CC + i] = 0;   // (the bitmaps at the head of every node's area)
  for (u32 i = lane; i < N * TC / 4u; i += 64) reinterpret_cast<u32 *>(g_rep)[i] = 0xFFFFFFFFu;
  __syncthreads();

  // ---- node / service state ----
  u32 deliver_at = INF; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, node_msgid = 0, part = 0;
  u32 root_v = 0, next_tid = 0;                        // node: the cached root's version, thunk ids handed out
  u32 root_exists = 0, cur_v = 0, n_order = 0;         // lin-kv lane: the root
  u32 svc_ctr = 0;                                     // lww-kv lane: rand-int draws so far
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_value = 0, process = slot, m_value = 0;
  const u32 dest_node = is_client ? slot % N : 0u;     // worker t -> node t mod N; a crashed process's successor (process + C) keeps it, C being a multiple of N
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

#define PAYS_LATENCY(src) (((src) < N || (src) >= LIN) && is_server)   // neither end is a client (group64_net.inc)
#define ENDPOINT_LANES   // a lane is one endpoint: node, worker slot or service
#define POLL_LANE (is_server || busy)   // the lanes that take from their queue (group64_poll.inc)
  #include "group64_net.inc"
  #include "group64_poll.inc"
  // elements of `k` visible at version `from`: versions only grow along a key's row, so the answer is a count — the row is read with
  // independent loads (one round trip) instead of one dependent load per element
  auto visible = [&](u32 k, u32 from) -> u32 {
    if (from == V_NIL) return 0u;
    const u32 cnt = g_kvn[k];
    u32 n = 0;
    if (mw <= 16u) {
      u32 row[16];
#pragma unroll
      for (u32 i = 0; i < 16u; i++) row[i] = i < cnt ? g_kv[k * mw + i] : 0xFFFFFFFFu;
#pragma unroll
      for (u32 i = 0; i < 16u; i++) n += (i < cnt && (row[i] >> 8) <= from) ? 1u : 0u;
      return n;
    }
    while (n < cnt && (g_kv[k * mw + n] >> 8) <= from) n++;
    return n;
  };

  for (;;) {
    #include "group64_phase.inc"

    // ---- R0: time ----
    #include "group64_time.inc"
    #include "group64_jump.inc"

    bool inv_row = false; u32 inv_packed = 0, inv_value = 0, inv_len = 0;
    bool cmp_row = false; u32 cmp_packed = 0, cmp_value = 0, cmp_len = 0;
    u32 nem_rows = 0, nem_f = 0, nem_v1 = 0, nem_v2 = 0, nem_len2 = 0;

#define CRASH_STRIDE C
    #include "list_append_client.inc"

    if (timeout_round) {
      if (busy && timeout_at <= T) complete(MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_value);
    } else {
      // ---- R1: scheduler ----
      if (due <= T) {
        switch (phase) {
          case PH_INIT: if (is_client && slot < N) { mark = true; kind = K_INIT; } phase = PH_INIT_WAIT; break;
          case PH_MAIN: {
            #include "group64_nemesis.inc"
            if (gen_live && gen_next <= T && free_mask) {
              const u32 nfree = (u32)__popcll(free_mask);
              const u32 kk = gen_k++;
              const u64 h = draw64(key, S_GEN, kk);
              const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
              const u32 pick = scale32(r_lo, nfree);
              const bool sel = is_worker && !busy && (u32)__popcll(free_mask & lt_mask) == pick;
              // the transaction ([upstream] elle list-append gen): lane 0 writes the micro-ops and owns the key pool
              #include "group64_txn_gen.inc"
              if (bad) { flags |= bad; phase = PH_DONE; break; }
              if (sel) { mark = true; kind = K_OP; m_value = n_payload | (n_mops << 24); }
              n_payload += n_mops;
              gen_next = T + __umulhi(r_hi, p.gen_period2_us);
            }
          } break;
          default: break;
        }
        if (phase == PH_DONE) break;
      }

      // ---- R2: marked clients invoke; the request goes to the worker's node ----
      u64 inv_mask = __ballot(mark);
      if (inv_mask) {
        u32 rq_dest = 0, rq_type = 0, rq_a = 0;
        if (mark) {
          mark = false; busy = true;
          if (kind == K_INIT) { rq_dest = slot; rq_type = M_INIT; next_msg_id = 0; }
          else {
            c_value = m_value;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (MSIM_F_TXN << 2) | (process << 12); inv_value = c_value & 0xFFFFFFu; inv_len = c_value >> 24;
            rq_dest = dest_node; rq_type = M_TXN; rq_a = c_value;
          }
          want = ++next_msg_id;
          timeout_at = T + (kind == K_OP ? p.cfg.client_timeout_ms : 10000u) * 1000u;
          s_send_cl++;
        }
        const u32 rq_pack = rq_dest | (rq_type << 8);
        ev_base = n_ev; id_base = next_id; n_ev += (u32)__popcll(inv_mask);
        while (inv_mask) {
          const u32 s = (u32)__builtin_ctzll(inv_mask); inv_mask &= inv_mask - 1;
          const u32 pk = rdlane(rq_pack, s);
          const u32 a = rdlane(rq_a, s), b = rdlane(want, s);
          if (lane == (pk & 0xFF)) arrive(next_id, pk >> 8, a, b, s);
          next_id++;
        }
        poll();
      }

      // ---- R3: one input per node, then one for each service (endpoint order: lin-kv, lww-kv) ----
      bool rep = false, svc_rep = false;   // node -> a client (rep_dest), service -> node
      u32 rep_dest = 0;
      u32 n_out = 0, o_dest = 0;           // node -> service: n_out messages in mout[lane][..], all to the same service
      u32 o_type = 0, o_a = 0, o_b = 0, o_to = 0, need_words = 0, done_slot = 0;
#define MK_NSLOTS MKG_SLOTS
#define REPLY_TO(cmsg) { rep = true; rep_dest = (cmsg) >> 24; o_b = (cmsg) & 0xFFFFFFu; }
#define CLIENT_REF(qb, qsrc) ((qb) | ((qsrc) << 24))   // a client is an endpoint: it rides in the top byte of the stored msg_id
      #include "mk_node.inc"
      const u64 jd_mask = jcap ? __ballot(is_server && deliver_at <= T) : 0ull;
      if (is_server && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
        #include "mk_input.inc"
      }
      n_ev += (u32)__popcll(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = wave_incl_scan(need_words);
        const u32 total = rdlane(incl, 63);
        #include "mk_reads.inc"
      }

      // COMMIT: ids in lane order (nodes, lin-kv, lww-kv); a node's messages in the order it emitted them; every receiver takes its own in
      {
        const u32 cnt = is_node ? (rep ? 1u : n_out) : (svc_rep ? 1u : 0u);
        const u32 incl = wave_incl_scan(cnt);
        const u32 total = rdlane(incl, 63);
        if (total) {
          const u32 my_off = incl - cnt;
          ev_base = n_ev; id_base = next_id; n_ev += total;
          if (rep) s_send_cl++; else s_send_sv += cnt;
          // node -> service: the service lane takes each node's run in node order
          u64 ts = __ballot(is_node && !rep && n_out != 0);
          while (ts) {
            const u32 s = (u32)__builtin_ctzll(ts); ts &= ts - 1;
            const u32 dst = rdlane(o_dest, s), kn = rdlane(n_out, s), off = rdlane(my_off, s);
            if (lane == LIN + dst) {
              const u32 *const mo = mout + s * (MK_KEYS * 3u);
              for (u32 k = 0; k < kn; k++) arrive(next_id + off + k, mo[k * 3u], mo[k * 3u + 1u], mo[k * 3u + 2u], s);
            }
          }
          // service -> node
          u64 sv = __ballot(svc_rep);
          while (sv) {
            const u32 s = (u32)__builtin_ctzll(sv); sv &= sv - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), d = rdlane(o_to, s), off = rdlane(my_off, s);
            if (lane == d) arrive(next_id + off, ty, a, b, s);
          }
          // node -> the client whose transaction (or init) it answers: no latency; lost like any other message (net.clj:214)
          u64 rp = __ballot(rep);
          while (rp) {
            const u32 s = (u32)__builtin_ctzll(rp); rp &= rp - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), d = rdlane(rep_dest, s), off = rdlane(my_off, s);
            if (lane == d) arrive(next_id + off, ty, a, b, s);
          }
          next_id += total;
        }
        poll();
      }
      // ---- R4: the clients' recv! loops (client.clj:94-107) ----
      for (;;) {
        const bool dl = is_client && deliver_at <= T;
        const u64 dm = __ballot(dl);
        if (!dm) break;
        if (dl) {
          const uint4 q = cm; deliver_at = INF;
          if (jcap) jwrite(n_ev + (u32)__popcll(dm & lt_mask), 1, q.y, q.z, q.w & 0xFFFFFFu, q.w >> 24, lane);
          client_deliver(q.y & 0xFFu, q.z, q.w & 0xFFFFFFu);   // (a reply nobody awaits any more is skipped: stale)
          poll();
        }
        n_ev += (u32)__popcll(dm);
      }
    }

    #include "group64_rows.inc"
  }

  #include "group64_stats.inc"
}
#include "group64_end.inc"
