// sim_kernel_txng.inc — the single-root txn-list-append node (sim_kernel_txn.inc: demo/clojure/single_key_txn.clj:116-180 over lin-kv) with SEVERAL
// WORKERS PER NODE (`--concurrency k n`).  Included by sim_kernels.h after sim_kernel_dtg.inc, whose lane layout and round machinery it shares: a lane
// is an ENDPOINT — nodes 0 .. N-1, client worker slots N .. N+CS-1 (worker t talks to node t mod N), lin-kv at N+CS — every endpoint has a queue,
// clients poll only while an RPC is outstanding, COMMIT is receiver-side.  The node and the service are sim_kernel_txn.inc's, statement for
// statement: every request in its own future (read the root, apply, cas with create_if_not_exists; a lost race answers error 30), up to
// TG_SLOTS transactions in flight per node (with one worker per node: 8, txn_kernel<> / txn8_kernel<>).
// Specification: oracle/txn_nodes.inc, bit for bit (tests/test_parity_gpu.py::test_single_key_txn_many_workers_parity, tests/test_hipemu_parity.py).

#define TG_SLOTS 64u

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) txng_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  uint4 *const slots = reinterpret_cast<uint4 *>(smem + p.off_seen);        // [N][TG_SLOTS] {client msg | client << 24, txn_ref, rpc_id, from | stage << 16 | used << 24}
  u32 *const gen = reinterpret_cast<u32 *>(smem + p.off_seen + p.N * TG_SLOTS * 16);   // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const u32 LIN = N + CS;                                                     // endpoint (= lane) of lin-kv
  const bool is_node = lane < N, is_client = lane >= N && lane < LIN, is_lin = lane == LIN;
  const bool is_server = is_node || is_lin;                                   // endpoints that poll all the time
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u64 lt_mask = (1ull << lane) - 1;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u32 all_nodes = (1u << N) - 1;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key, mv = p.cfg.max_values;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_kv = g_scr;                          // [max_values][mw]: element | version << 8 (the one append log, DESIGN.md §2.4)
  u32 *const g_kvn = g_kv + (size_t)mv * mw;        // [max_values] elements so far
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 qidx = is_node ? lane : N;   // queue of a server endpoint (lin-kv: N)
  const u32 my_cap = is_server ? p.cap_node : T_CLIENT_CAP;
  const u32 my_spill_cap = is_server ? p.spill_cap : 0u;
  uint4 *const my_inbox = inbox + (is_server ? qidx * p.cap_node : is_client ? (N + 1) * p.cap_node + slot * T_CLIENT_CAP : 0u);
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qidx * p.spill_cap;
  uint4 *const my_slots = slots + (is_node ? lane : 0) * TG_SLOTS;

  for (u32 i = lane; i < N * TG_SLOTS; i += 64) slots[i] = make_uint4(0, 0, 0, 0);
  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  for (u32 i = lane; i < mv; i += 64) g_kvn[i] = 0;
  __syncthreads();

  // ---- endpoint state ----
  bool has_c = false; u32 deliver_at = 0; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, node_msgid = 0, part = 0;
  u32 root = V_NIL;                                    // lin-kv lane: the version of "root" (V_NIL: the key does not exist)
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
#define COMMIT_FLAG   // has_c says whether an envelope is committed
#define POLL_LANE (is_server || busy)   // the lanes that take from their queue (group64_poll.inc)
  #include "group64_net.inc"
  #include "group64_poll.inc"
  auto visible = [&](u32 k, u32 from) -> u32 {
    if (from == V_NIL) return 0u;
    const u32 cnt = g_kvn[k];
    u32 n = 0;
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
#define OWN_CLIENT_DELIVER   // recv! is spelled out in R4: as a lambda it is other device code
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

      // ---- R3: one input per node, then one for the service (endpoint order) ----
      bool rep = false; u32 rep_dest = 0, rep_type = 0, rep_a = 0, rep_b = 0;   // what this server endpoint sends (at most one message a round)
      u32 need_words = 0, done_slot = 0;
      const bool take = is_server && has_c && deliver_at <= T;
      const u64 jd_mask = jcap ? __ballot(take) : 0ull;
      if (take) {
        const uint4 q = cm; has_c = false;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
        if (is_node) {
          switch (qtype) {
            case M_INIT: rep = true; rep_dest = qsrc; rep_type = M_INIT_OK; rep_b = qb; break;
            case M_TXN: {   // every request in its own future (:98-100): read the root (:150-157)
              u32 i = 0; while (i < TG_SLOTS && (my_slots[i].w >> 24)) i++;
              if (i == TG_SLOTS) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; break; }
              const u32 rid = ++node_msgid;
              my_slots[i] = make_uint4(qb | (qsrc << 24), qa, rid, (1u << 16) | (1u << 24));
              rep = true; rep_dest = LIN; rep_type = M_READ; rep_a = 0; rep_b = rid;
            } break;
            case M_READ_OK: case M_CAS_OK: case M_ERROR: {
              u32 i = 0;
              while (i < TG_SLOTS) { const uint4 s = my_slots[i]; if ((s.w >> 24) && s.z == qb) break; i++; }
              if (i == TG_SLOTS) break;  // handle-reply!: no such rpc
              uint4 s = my_slots[i];
              if (((s.w >> 16) & 0xFF) == 1) {
                u32 from;
                if (qtype == M_READ_OK) from = qa;
                else if (qtype == M_ERROR && qa == 20) from = V_NIL;
                else { rep = true; rep_dest = s.x >> 24; rep_type = M_ERROR; rep_a = qa; rep_b = s.x & 0xFFFFFFu; my_slots[i] = make_uint4(0, 0, 0, 0); break; }
                const u32 rid = ++node_msgid;
                s.z = rid; s.w = from | (2u << 16) | (1u << 24);
                my_slots[i] = s;
                rep = true; rep_dest = LIN; rep_type = M_CAS; rep_a = from | (i << 16); rep_b = rid;   // cas-service!, :159-169
              } else {
                rep = true; rep_dest = s.x >> 24; rep_b = s.x & 0xFFFFFFu;
                if (qtype == M_CAS_OK) {  // the completed transaction goes into the payload area (sized here, written below)
                  rep_type = M_TXN_OK; done_slot = i;
                  const u32 off0 = s.y & 0xFFFFFFu, n = s.y >> 24, from = s.w & 0xFFFFu;
                  for (u32 j = 0; j < n; j++) {
                    const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
                    need_words++;
                    if (!(w & 1)) {
                      u32 len = visible(k, from);
                      for (u32 e = 0; e < j; e++) { const u32 we = g_pay[off0 + e]; if ((we & 1) && ((we >> 1) & 0x7FFFu) == k) len++; }
                      need_words += (len + 3) / 4;
                    }
                  }
                } else { rep_type = M_ERROR; rep_a = qa == 22 ? 30u : qa; my_slots[i] = make_uint4(0, 0, 0, 0); }   // "root altered", :178-180
              }
            } break;
            default: break;
          }
        } else {  // the lin-kv service (service.clj:31-61 over the key "root")
          rep = true; rep_dest = qsrc; rep_b = qb;
#define TXN_REF_OF(node, i) slots[(node) * TG_SLOTS + (i)].y
          #include "txn_lin.inc"
        }
      }
      n_ev += (u32)__popcll(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = wave_incl_scan(need_words);
        const u32 total = rdlane(incl, 63);
        #include "txn_reads.inc"
      }

      // COMMIT: one message per server endpoint at most; ids in lane order (nodes, then the service)
      {
        const u64 reps0 = __ballot(rep);
        if (reps0) {
          const u32 my_off = (u32)__popcll(reps0 & lt_mask);
          ev_base = n_ev; id_base = next_id; n_ev += (u32)__popcll(reps0);
          if (rep) { if (rep_dest >= N && rep_dest < LIN) s_send_cl++; else s_send_sv++; }
          const u32 rep_pack = rep_dest | (rep_type << 8);
          u64 reps = reps0;
          while (reps) {
            const u32 s = (u32)__builtin_ctzll(reps); reps &= reps - 1;
            const u32 pk = rdlane(rep_pack, s), o = rdlane(my_off, s);
            const u32 r_a = rdlane(rep_a, s), r_b = rdlane(rep_b, s);
            if (lane == (pk & 0xFF)) arrive(next_id + o, pk >> 8, r_a, r_b, s);
          }
          next_id += (u32)__popcll(reps0);
        }
        poll();
      }

      // ---- R4: the clients' recv! loops (client.clj:94-107) ----
      for (;;) {
        const bool dl = is_client && has_c && deliver_at <= T;
        const u64 dm = __ballot(dl);
        if (!dm) break;
        if (dl) {
          const uint4 q = cm; has_c = false;
          s_recv_cl++;
          const u32 qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
          if (jcap) jwrite(n_ev + (u32)__popcll(dm & lt_mask), 1, q.y, qa, qb, q.w >> 24, lane);
          if (busy && qb == want) {  // else stale (client.clj:105-107)
            if (qtype == M_TXN_OK) complete(MSIM_T_OK, 0, qa);
            else if (qtype == M_ERROR)
              if (qa == 0u) complete(MSIM_T_INFO, MSIM_ERR_TIMEOUT, c_value);   // code 0 :timeout is not :definite? (errors.edn:2-4)
              else complete(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : qa == 30 ? MSIM_ERR_TXN_CONFLICT : qa == 14 ? MSIM_ERR_ABORT : MSIM_ERR_PRECONDITION_FAILED, c_value);
            else complete(MSIM_T_OK, 0, c_value);  // init_ok
          }
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
