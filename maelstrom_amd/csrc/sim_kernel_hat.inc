// sim_kernel_hat.inc — txn-rw-register served by the highly-available-transactions node (SURVEY.md §8f rank 4; the
// reference's own demo for this workload, core.clj:115-121).  Included by engine.hip.
//
//   node     demo/clojure/txn_rw_register_hat.clj: txn :120-130 (apply locally at a fresh [lamport, node] timestamp,
//            last write wins per register, remember as unreplicated to every other node, txn_ok), the 100 ms replication
//            thread :92-118 (send one peer ALL txns it has not acknowledged), replicate :132-150 (apply at the txn's own
//            timestamp, relay what is still pending elsewhere, replicate_ack to every other node), replicate_ack :152-172
//   client   workload/txn_rw_register.clj:108-139 (Reusable, txn! RPC); generator: [upstream] elle rw-register gen —
//            the list-append key pool with writes in place of appends
//
// Lanes: lane i < N = node i + its client (one worker per node, as in txn_kernel<>).  Every txn of the cluster gets a
// slot g in one table in HBM scratch (timestamp, where its micro-ops sit in the payload area); a node's unreplicated
// map is the byte array pend[node][g] = mask of nodes still to reach.  A replicate message carries (offset, count) of a
// list of words g | mask << 24 in the replication area; its acks refer to the same list.  Registers live in HBM too
// (kv[node][key] = lamport << 11 | node << 8 | value, 0 = never written); L2 keeps the working set.  Timer ticks of a
// node with nothing unreplicated are not simulated (armed / disarmed with the set, oracle/hat_nodes.inc explains why that
// is the same behaviour).  Same specification as oracle/hat_nodes.inc, bit for bit.

enum { M_REPLICATE_ACK = 27 };  // include/maelsim.h MSIM_M_REPLICATE_ACK
#define HAT_TICK_US 100000u
#define HAT_SHORT 8u   // list entries / txn slots a node's own lane walks; longer ones go to the wavefront passes

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) hat_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const gen = reinterpret_cast<u32 *>(smem + p.off_seen);  // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N;
  const bool is_node = lane < N;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u64 lt_mask = (1ull << lane) - 1;
  const u32 all_nodes = (1u << N) - 1;
  const u32 worker_mask = all_nodes;   // one worker per node: the client on the node's lane
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key;
  const u32 K = p.cfg.max_values, G = max_rows / 2, area_cap = p.cfg.replication_words;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_kv = g_scr + (size_t)(is_node ? lane : 0) * K;                     // this node's registers
  u32 *const g_tab = g_scr + (size_t)N * K;                                        // [G][2]: ts, micro-ops ref
  unsigned char *const pend_all = reinterpret_cast<unsigned char *>(g_tab + 2 * (size_t)G);  // [N][G]
  unsigned char *const g_pend = pend_all + (size_t)(is_node ? lane : 0) * G;
  u32 *const g_area = g_tab + 2 * (size_t)G + ((size_t)N * G + 3) / 4;              // replicate lists
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = p.cap_node, my_spill_cap = p.spill_cap;
  const u32 qlane = is_node ? lane : 0;
  uint4 *const my_inbox = inbox + qlane * my_cap;
  uint4 *const my_cinbox = inbox + N * my_cap + qlane * T_CLIENT_CAP;
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qlane * my_spill_cap;
  const u32 my_client = N + lane;

  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  for (u32 i = lane; i < N * K; i += 64) g_scr[i] = 0;
  for (u32 i = lane; i < ((size_t)N * G + 3) / 4; i += 64) g_tab[2 * (size_t)G + i] = 0;
  __syncthreads();

  // ---- node state ----
  u32 deliver_at = INF; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, part = 0;
  u32 lamport = 0, lo = 0, npend = 0, timer_next = INF;
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_value = 0, process = lane, m_value = 0, cin_n = 0;
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0, n_txn = 0, n_area = 0;

#define PAYS_LATENCY(src) ((src) < N)   // neither end is a client (group64_net.inc)
  #include "group64_net.inc"
  auto poll = [&]() {
    if (have_pm) {
      have_pm = false;
      if (deliver_at == INF && (in_n | sp_n) == 0) try_commit(pm);
      else lds_push(pm);
    }
    while (is_node && deliver_at == INF && (in_n | sp_n) != 0) {
      u32 best = 0; bool in_spill = false;
      u64 bk = ~0ull;
      for (u32 i = 0; i < in_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_inbox[i]);
        const u64 k2 = ((u64)kk.x << 32) | kk.y;
        if (k2 < bk) { bk = k2; best = i; }
      }
      spill_min(my_spill, sp_n, bk, best, in_spill);
      uint4 e;
      if (in_spill) { e = my_spill[best]; sp_n--; if (best != sp_n) my_spill[best] = my_spill[sp_n]; }
      else { e = my_inbox[best]; in_n--; if (best != in_n) my_inbox[best] = my_inbox[in_n]; }
      try_commit(e);
    }
  };

  for (;;) {
    #include "group64_phase.inc"

    // ---- R0: time ----
    #include "group64_time.inc"
    my_t = min(my_t, timer_next);
    #include "group64_jump.inc"

    bool inv_row = false; u32 inv_packed = 0, inv_value = 0, inv_len = 0;
    bool cmp_row = false; u32 cmp_packed = 0, cmp_value = 0, cmp_len = 0;
    u32 nem_rows = 0, nem_f = 0, nem_v1 = 0, nem_v2 = 0, nem_len2 = 0;

    auto complete = [&](u32 type, u32 err, u32 ref) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (MSIM_F_TXN << 2) | (err << 7) | (process << 12);
      cmp_value = ref & 0xFFFFFFu; cmp_len = ref >> 24;
      if (type == MSIM_T_INFO) process += N;  // crashed process; the Reusable client itself lives on
    };
    // the client's recv! consumes one envelope (client.clj:94-107)
    auto client_deliver = [&](u32 qtype, u32 qa, u32 qb) {
      s_recv_cl++;
      if (busy && qb == want) {
        if (qtype == M_TXN_OK) complete(MSIM_T_OK, 0, qa);
        else complete(MSIM_T_OK, 0, c_value);  // init_ok
      }
    };

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
              // the transaction ([upstream] elle rw-register gen): lane 0 writes the micro-ops and owns the key pool
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

      // ---- R3: one input per node: a due replication tick, else the due message ----
      bool rep = false; u32 dmask = 0;  // reply to the own client / node -> node sends (same type, a, b to every dest in dmask)
      u32 o_type = 0, o_a = 0, o_b = 0;
#define REPLY_TO(cmsg) { rep = true; o_b = (cmsg); }   // (the client lives in the node's lane)
#define CLIENT_REF(qb, qsrc) (qb)
      #include "hat_node.inc"

      // COMMIT: ids in node order, then destination order
      bool c_arr = false; u32 ca_y = 0, ca_a = 0, ca_b = 0;
      {
        const u32 cnt = rep ? 1u : (u32)__popc(dmask);
        const u32 smask = (u32)__ballot(cnt != 0);
        if (smask) {
          const u32 incl = scan32(cnt), my_off = incl - cnt, total = rdlane(incl, 31);
          ev_base = n_ev; id_base = next_id; n_ev += total;
          if (rep) s_send_cl++; else s_send_sv += cnt;
          u32 ns = (u32)__ballot(dmask != 0);
          while (ns) {  // node -> node: every receiver takes its envelope from each sender, in sender order
            const u32 s = (u32)__builtin_ctz(ns); ns &= ns - 1;
            const u32 dm = rdlane(dmask, s), ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), off = rdlane(my_off, s);
            if (is_node && ((dm >> lane) & 1u)) arrive(next_id + off + __popc(dm & lt32), ty, a, b, s, lane);
          }
          // node -> its own client: no latency; lost like any other message (net.clj:214)
          if (rep) {
            const u32 id = next_id + my_off;
            if (jcap) jwrite(ev_base + my_off, 0, (id << 8) | o_type, o_a, o_b, lane, my_client);
            if (!(NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss)) { c_arr = true; ca_y = (id << 8) | o_type; ca_a = o_a; ca_b = o_b; }
          }
          next_id += total;
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
