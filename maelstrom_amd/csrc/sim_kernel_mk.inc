// sim_kernel_mk.inc — txn-list-append over the multi-key transactional node (SURVEY.md §8a row a18, the canonical variant).
// Included by engine.hip after sim_kernel_txn.inc (whose message types, V_NIL and T_CLIENT_CAP it shares).
//
//   node      demo/js/multi_key_txn.js:1-246 == demo/clojure/multi_key_txn.clj: immutable thunks in lww-kv, one root map key ->
//             thunk id in lin-kv; getState / applyTxn / writeThunks / casRoot, retry from a fresh root when the cas is lost
//   services  lin-kv service.clj:31-61,141-155; lww-kv service.clj:214-243 (two replicas that never exchange state, three rand-int
//             draws per request) over :65-114
//
// Lanes: lane i < N = node i + its client; lane N = lin-kv (endpoint 2N), lane N + 1 = lww-kv (endpoint 2N + 1).
// The specification is oracle/mk_nodes.inc, statement by statement: root values are versions (number of value-changing cas so
// far), the root map is the global key order restricted to a version, thunk values are never materialised.  One input can make
// a node send up to MK_KEYS messages, all to the same service (thunk reads in root order, thunk writes in state order): they go
// through mout[] in LDS and the service lane takes the run in at COMMIT.

#define MK_SLOTS 8u   // transactions in flight per node (the oracle's limit) ...
#define MK_SL 2u      // ... of which in LDS; the others (in use only while clients time out) in HBM scratch
#define MK_NONE 0xFFFFFFFFu
// A transaction slot is 10 header words and 9 arrays of KEYS words (KEYS = the distinct keys a transaction can touch: 4 for the default
// --max-txn-length 4, else 8).  Round 3: with 8 slots of 84 words per node in LDS a cluster took 21.6 KiB and a CU held 7 clusters of a
// kernel that waits for memory; two slots of 46 words leave it 9.6 KiB.
enum { SK_HDR = 0 /* used | stage << 8: 1 thunk reads, 2 thunk writes, 3 cas, 4 root read */, SK_NK = 1, SK_NSTATE = 2, SK_NNEW = 3, SK_RDOUT = 4, SK_WROUT = 5,
       SK_CMSG = 6, SK_REF = 7, SK_RV = 8, SK_RPC = 9, SK_KEY = 10 };
enum { D_LIN = 0, D_LWW = 1 };
static inline uint32_t mk_slot_words(uint32_t keys) { return 10u + 9u * keys; }
static inline uint32_t mk_keys_for(const msim_config &c) { return c.max_txn_length <= 4u ? 4u : 8u; }

template <bool NEM, bool NET_RANDOM, int KEYS>
__global__ void __launch_bounds__(64) mk_kernel(const KParams p) {
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
  const u32 N = p.N;
  const bool is_node = lane < N, is_lin = lane == N;
  const u32 LIN = 2 * N;  // endpoint index of lin-kv (lane N); lww-kv is LIN + 1 (lane N + 1)
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u32 all_nodes = (1u << N) - 1;
  const u32 worker_mask = all_nodes;   // one worker per node: the client on the node's lane
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
  u32 *const xslots = g_cache + (size_t)N * CC + (((size_t)N * TC + 15u) / 16u) * 4u;         // [N][MK_SLOTS - MK_SL][MKW]: slots MK_SL .. MK_SLOTS-1
  // slot si of node nd: LDS for the first MK_SL, HBM scratch beyond (a generic pointer: flat loads / stores reach both)
  auto slot_of = [&](u32 nd, u32 si) -> u32 * { return si < MK_SL ? slots + (nd * MK_SL + si) * MKW : xslots + ((size_t)nd * (MK_SLOTS - MK_SL) + (si - MK_SL)) * MKW; };
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = p.cap_node, my_spill_cap = p.spill_cap;
  const u32 qlane = lane <= N + 1u ? lane : 0;
  uint4 *const my_inbox = inbox + qlane * my_cap;                                     // node / service queue
  uint4 *const my_cinbox = inbox + (N + 2) * my_cap + (is_node ? lane : 0) * T_CLIENT_CAP;
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qlane * my_spill_cap;
  const u32 my_node = is_node ? lane : 0u;
  u32 *const my_cache = g_cache + (size_t)(is_node ? lane : 0) * CC;
  const u32 my_client = N + lane;

  for (u32 i = lane; i < N * MK_SL * MKW; i += 64) slots[i] = 0;
  for (u32 i = lane; i < N * (MK_SLOTS - MK_SL); i += 64) xslots[(size_t)i * MKW + SK_HDR] = 0;
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
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_value = 0, process = lane, m_value = 0, cin_n = 0;
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

#define PAYS_LATENCY(src) ((src) < N || (src) >= LIN)   // neither end is a client (group64_net.inc)
#define POLL_LANE (lane <= N + 1u)   // the lanes that take from their queue (group64_poll.inc)
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

      // ---- R3: one input per node, then one for each service (endpoint order: lin-kv, lww-kv) ----
      bool rep = false, svc_rep = false;   // node -> own client, service -> node
      u32 n_out = 0, o_dest = 0;           // node -> service: n_out messages in mout[lane][..], all to the same service
      u32 o_type = 0, o_a = 0, o_b = 0, o_to = 0, need_words = 0, done_slot = 0;
#define MK_NSLOTS MK_SLOTS
#define REPLY_TO(cmsg) { rep = true; o_b = (cmsg); }   // (the client lives in the node's lane)
#define CLIENT_REF(qb, qsrc) (qb)
      #include "mk_node.inc"
      const u32 jd_mask = jcap ? (u32)__ballot(lane <= N + 1u && deliver_at <= T) : 0u;
      if (lane <= N + 1u && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, is_node ? lane : N + lane);
        #include "mk_input.inc"
      }
      n_ev += __popc(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = scan32(need_words);
        const u32 total = rdlane(incl, 31);
        #include "mk_reads.inc"
      }

      // COMMIT: ids in lane order (nodes, lin-kv, lww-kv); a node's messages in the order it emitted them
      bool c_arr = false; u32 ca_y = 0, ca_a = 0, ca_b = 0;
      {
        const u32 cnt = is_node ? (rep ? 1u : n_out) : (svc_rep ? 1u : 0u);
        const u32 incl = scan32(cnt);
        const u32 total = rdlane(incl, 31);
        if (total) {
          const u32 my_off = incl - cnt;
          ev_base = n_ev; id_base = next_id; n_ev += total;
          if (rep) s_send_cl++; else s_send_sv += cnt;
          // node -> service: the service lane takes each node's run in node order
          u32 ts = (u32)__ballot(is_node && !rep && n_out != 0);
          while (ts) {
            const u32 s = (u32)__builtin_ctz(ts); ts &= ts - 1;
            const u32 dst = rdlane(o_dest, s), kn = rdlane(n_out, s), off = rdlane(my_off, s);
            if (lane == N + dst) {
              const u32 *const mo = mout + s * (MK_KEYS * 3u);
              for (u32 k = 0; k < kn; k++) arrive(next_id + off + k, mo[k * 3u], mo[k * 3u + 1u], mo[k * 3u + 2u], s, LIN + dst);
            }
          }
          // service -> node
          u32 sv = (u32)__ballot(svc_rep);
          while (sv) {
            const u32 s = (u32)__builtin_ctz(sv); sv &= sv - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), d = rdlane(o_to, s), off = rdlane(my_off, s);
            if (lane == d) arrive(next_id + off, ty, a, b, N + s, d);
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
