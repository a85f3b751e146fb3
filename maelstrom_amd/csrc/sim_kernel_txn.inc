// sim_kernel_txn.inc — txn-list-append (SURVEY.md §8a rows a17/a18, BASELINE configs[4]).  Included by engine.hip.
//
//   node     demo/clojure/single_key_txn.clj:116-180: read "root" from lin-kv -> apply the txn -> cas root
//            (create_if_not_exists) -> txn_ok, or error 30 when the cas lost the race (code 22)
//   service  service.clj:31-61 (PersistentKV read/cas), :141-155 (Linearizable), :245-263 (service thread)
//   client   workload/txn_list_append.clj:94-126 (Reusable client, txn! RPC); generator: [upstream] elle list-append
//
// Lanes: lane i < N = node i + its client (one worker per node, as in sim_kernel_colo<>); lane N = the lin-kv service,
// endpoint 2N (after the client slots).  Node <-> service envelopes cross lanes with latency/loss like any server
// traffic (util.clj:7-16); no partition ever names the service.  COMMIT ids run in lane order = endpoint order.
//
// The database value is never materialised: successful cas operations form a chain, so a state is a prefix of ONE
// append log.  version = appends committed so far (V_NIL: "root" does not exist); an element stores the version that
// made it visible; the list of key k at version v is the prefix of k's elements with version <= v.  Elements live in
// HBM scratch (kv[key][i], kvn[key]); the per-node tables of transactions in flight live in LDS.
// Same specification as oracle/txn_nodes.inc, bit for bit.

#define TXN_SLOTS 8u
#define V_NIL 0xFFFFu
#define T_CLIENT_CAP 32u  // Reusable clients keep collecting late replies (client.clj:94-107)
enum { M_TXN = 23, M_TXN_OK = 24 };  // after the raft RPC types (include/maelsim.h MSIM_M_*)
enum { S_GEN3 = 3 };

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) txn_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  uint4 *const slots = reinterpret_cast<uint4 *>(smem + p.off_seen);       // [N][TXN_SLOTS] {client_msg, txn_ref, rpc_id, from | stage << 16 | used << 24}
  u32 *const gen = reinterpret_cast<u32 *>(smem + p.off_seen + p.N * TXN_SLOTS * 16);  // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N;
  const bool is_node = lane < N, is_svc = lane == N;
  const u32 SVC = 2 * N;  // the service's endpoint index
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u32 all_nodes = (1u << N) - 1;
  const u32 worker_mask = all_nodes;   // one worker per node: the client on the node's lane
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_kv = g_scr;                                           // [max_values][mw]: element | version << 8
  u32 *const g_kvn = g_scr + (size_t)p.cfg.max_values * mw;          // [max_values]
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = p.cap_node, my_spill_cap = p.spill_cap;
  const u32 qlane = lane <= N ? lane : 0;
  uint4 *const my_inbox = inbox + qlane * my_cap;                                     // node / service queue
  uint4 *const my_cinbox = inbox + (N + 1) * my_cap + (is_node ? lane : 0) * T_CLIENT_CAP;
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qlane * my_spill_cap;
  uint4 *const my_slots = slots + (is_node ? lane : 0) * TXN_SLOTS;
  const u32 my_client = N + lane;

  for (u32 i = lane; i < N * TXN_SLOTS; i += 64) slots[i] = make_uint4(0, 0, 0, 0);
  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  for (u32 i = lane; i < p.cfg.max_values; i += 64) g_kvn[i] = 0;
  __syncthreads();

  // ---- node / service state ----
  u32 deliver_at = INF; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, node_msgid = 0, part = 0, root = V_NIL;
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_value = 0, process = lane, m_value = 0, cin_n = 0;
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

#define PAYS_LATENCY(src) ((src) < N || (src) == SVC)   // neither end is a client (group64_net.inc)
#define POLL_LANE (lane <= N)   // the lanes that take from their queue (group64_poll.inc)
  #include "group64_net.inc"
  #include "group64_poll.inc"
  // elements of `k` visible at version `from`
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

#define CRASH_STRIDE N
    #include "list_append_client.inc"

    if (timeout_round) {
      if (busy && timeout_at <= T) complete(MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_value);
    } else {
      // ---- R1: scheduler ----
      if (due <= T) {
        switch (phase) {
          case PH_INIT: if (is_node) { mark = true; kind = K_INIT; } phase = PH_INIT_WAIT; break;
          case PH_MAIN: {
            #include "group64_nemesis.inc"
            if (gen_live && gen_next <= T && free_mask) {
              const u32 nfree = __popc(free_mask);
              const u32 kk = gen_k++;
              const u64 h = draw64(key, S_GEN, kk);
              const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
              const u32 pick = scale32(r_lo, nfree);
              const bool sel = is_node && !busy && (u32)__popc(free_mask & lt32) == pick;
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

      // ---- R2: marked clients invoke; the request goes to this lane's own node ----
      const u32 inv_mask = (u32)__ballot(mark);
      if (inv_mask) {
        ev_base = n_ev; id_base = next_id; n_ev += __popc(inv_mask);
        if (mark) {
          mark = false; busy = true;
          u32 rq_type, rq_a = 0;
          if (kind == K_INIT) { rq_type = M_INIT; next_msg_id = 0; }
          else {
            c_value = m_value;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (MSIM_F_TXN << 2) | (process << 12); inv_value = c_value & 0xFFFFFFu; inv_len = c_value >> 24;
            rq_type = M_TXN; rq_a = c_value;
          }
          want = ++next_msg_id;
          timeout_at = T + (kind == K_OP ? p.cfg.client_timeout_ms : 10000u) * 1000u;
          s_send_cl++;
          arrive(next_id + __popc(inv_mask & lt32), rq_type, rq_a, want, my_client, lane);
        }
        next_id += __popc(inv_mask);
        poll();
      }

      // ---- R3: one input per node, then one for the service (endpoint order) ----
      bool to_svc = false, rep = false, svc_rep = false;   // node -> service, node -> own client, service -> node
      u32 rep_type = 0, rep_a = 0, rep_b = 0, o_dest = 0, need_words = 0, done_slot = 0;
      const u32 jd_mask = jcap ? (u32)__ballot(lane <= N && deliver_at <= T) : 0u;
      if (lane <= N && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < SVC) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, is_svc ? SVC : lane);
        if (is_node) {
          switch (qtype) {
            case M_INIT: rep = true; rep_type = M_INIT_OK; rep_b = qb; break;
            case M_TXN: {
              u32 i = 0; while (i < TXN_SLOTS && (my_slots[i].w >> 24)) i++;
              if (i == TXN_SLOTS) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; break; }
              const u32 rid = ++node_msgid;
              my_slots[i] = make_uint4(qb, qa, rid, (1u << 16) | (1u << 24));
              to_svc = true; rep_type = M_READ; rep_a = 0; rep_b = rid;
            } break;
            case M_READ_OK: case M_CAS_OK: case M_ERROR: {
              u32 i = 0;
              while (i < TXN_SLOTS) { const uint4 s = my_slots[i]; if ((s.w >> 24) && s.z == qb) break; i++; }
              if (i == TXN_SLOTS) break;  // handle-reply!: no such rpc
              uint4 s = my_slots[i];
              if (((s.w >> 16) & 0xFF) == 1) {
                u32 from;
                if (qtype == M_READ_OK) from = qa;
                else if (qtype == M_ERROR && qa == 20) from = V_NIL;
                else { rep = true; rep_type = M_ERROR; rep_a = qa; rep_b = s.x; my_slots[i] = make_uint4(0, 0, 0, 0); break; }
                const u32 rid = ++node_msgid;
                s.z = rid; s.w = from | (2u << 16) | (1u << 24);
                my_slots[i] = s;
                to_svc = true; rep_type = M_CAS; rep_a = from | (i << 16); rep_b = rid;
              } else {
                rep = true; rep_b = s.x;
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
                } else { rep_type = M_ERROR; rep_a = qa == 22 ? 30u : qa; my_slots[i] = make_uint4(0, 0, 0, 0); }
              }
            } break;
            default: break;
          }
        } else {  // the lin-kv service (service.clj:31-61 over the key "root")
          svc_rep = true; o_dest = qsrc; rep_b = qb;
#define TXN_REF_OF(node, i) slots[(node) * TXN_SLOTS + (i)].y
          #include "txn_lin.inc"
        }
      }
      n_ev += __popc(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = scan32(need_words);
        const u32 total = rdlane(incl, 31);
        #include "txn_reads.inc"
      }

      // COMMIT: ids in lane order (nodes, then the service)
      bool c_arr = false; u32 ca_y = 0, ca_a = 0, ca_b = 0;
      {
        const u32 cnt = (to_svc || rep || svc_rep) ? 1u : 0u;
        const u32 smask = (u32)__ballot(cnt != 0);
        if (smask) {
          const u32 my_off = __popc(smask & lt32);
          ev_base = n_ev; id_base = next_id; n_ev += __popc(smask);
          if (rep) s_send_cl++; else if (cnt) s_send_sv++;
          // node -> service: the service lane takes them in node order
          u32 ts = (u32)__ballot(to_svc);
          while (ts) {
            const u32 s = (u32)__builtin_ctz(ts); ts &= ts - 1;
            const u32 ty = rdlane(rep_type, s), a = rdlane(rep_a, s), b = rdlane(rep_b, s), off = rdlane(my_off, s);
            if (is_svc) arrive(next_id + off, ty, a, b, s, SVC);
          }
          // service -> node
          const u32 sv = (u32)__ballot(svc_rep);
          if (sv) {
            const u32 ty = rdlane(rep_type, N), a = rdlane(rep_a, N), b = rdlane(rep_b, N), d = rdlane(o_dest, N), off = rdlane(my_off, N);
            if (lane == d) arrive(next_id + off, ty, a, b, SVC, d);
          }
          // node -> its own client: no latency; lost like any other message (net.clj:214)
          if (rep) {
            const u32 id = next_id + my_off;
            if (jcap) jwrite(ev_base + my_off, 0, (id << 8) | rep_type, rep_a, rep_b, lane, my_client);
            if (!(NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss)) { c_arr = true; ca_y = (id << 8) | rep_type; ca_a = rep_a; ca_b = rep_b; }
          }
          next_id += __popc(smask);
        }
        poll();
      }

      // ---- R4: the clients' recv! loops (client.clj:94-107) ----
      if (__ballot(c_arr || (busy && cin_n > 0))) {
        for (;;) {
          const bool stale = busy && cin_n > 0;
          const bool fresh = !stale && busy && c_arr;
          const u32 dm = (u32)__ballot(stale || fresh);
          if (!dm) break;
          if (stale) {
            u32 best = 0;
            uint2 bk = *reinterpret_cast<const uint2 *>(&my_cinbox[0]);
            for (u32 i = 1; i < cin_n; i++) {
              const uint2 kk = *reinterpret_cast<const uint2 *>(&my_cinbox[i]);
              if (kk.x < bk.x || (kk.x == bk.x && kk.y < bk.y)) { bk = kk; best = i; }
            }
            const uint4 e = my_cinbox[best];
            cin_n--;
            if (best != cin_n) my_cinbox[best] = my_cinbox[cin_n];
            if (jcap) jwrite(n_ev + __popc(dm & lt32), 1, e.y, e.z, e.w & 0xFFFFFFu, e.w >> 24, my_client);
            client_deliver(e.y & 0xFFu, e.z, e.w & 0xFFFFFFu);
          } else if (fresh) {
            c_arr = false;
            if (jcap) jwrite(n_ev + __popc(dm & lt32), 1, ca_y, ca_a, ca_b, lane, my_client);
            client_deliver(ca_y & 0xFFu, ca_a, ca_b);
          }
          n_ev += __popc(dm);
        }
        if (c_arr) {  // nobody is in recv!: the envelope waits for the next RPC (and is skipped there as stale)
          if (cin_n >= T_CLIENT_CAP) my_flags |= MSIM_FLAG_INBOX_OVERFLOW;
          else my_cinbox[cin_n++] = make_uint4(T, ca_y, ca_a, ca_b | (lane << 24));
        }
      }
    }

    #include "group64_rows.inc"
  }

  #include "group64_stats.inc"
}
#include "group64_end.inc"
