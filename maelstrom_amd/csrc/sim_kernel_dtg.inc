// sim_kernel_dtg.inc — the Datomic-style txn-list-append node (sim_kernel_dt.inc, SURVEY.md §8a row a18) with SEVERAL WORKERS PER NODE
// (`--concurrency 10n`, the reference's own invocation for this workload: doc/05-datomic/01-single-node.md:257,322).  Included by sim_kernels.h
// after sim_kernel_dt.inc, whose scratch layout, record format and stages it uses; the node and the two services are the same text, dt_node.inc / dt_input.inc.
//
// What several workers change is the lane layout, not the program: with one worker per node a client lives in its node's lane (dt_kernel<>);
// here a lane is an ENDPOINT — nodes 0 .. N-1, client worker slots N .. N+CS-1 (worker t talks to node t mod N, [upstream] interpreter), lin-kv at
// N+CS, lww-kv at N+CS+1 (the oracle's endpoint numbers, oracle/dt_nodes.inc) — as in svc_kernel<> (sim_kernel_svc.inc), whose round machinery
// this kernel takes: every endpoint has a queue, clients poll only while an RPC is outstanding, COMMIT is receiver-side over the senders' lanes.
// It is where the node's @txn_lock and its arrival-order waiting queue (datomic_list_append.rb:347-372, node.rb:147-183) carry load: ten
// requests reach one node within a millisecond and are served one after the other.  The waiting ring holds DG_WAITQ transactions per node.
// Specification: oracle/dt_nodes.inc, bit for bit (tests/test_parity_gpu.py::test_datomic_many_workers_parity, tests/test_hipemu_parity.py).

#define DG_WAITQ 64u
enum { DG_WQN = DC_OWN + 8 /* waiting: count | ring head << 8 */, DG_WQ /* DG_WAITQ x {client msg | client << 24, txn ref} */,
       DG_STK = DG_WQ + 2 * DG_WAITQ /* (DT_MAXDEPTH + 1) x {pointer, next child} */, DG_WORDS = DG_STK + 2 * (DT_MAXDEPTH + 1) };

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) DT_OCC dtg_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const curs = reinterpret_cast<u32 *>(smem + p.off_seen);             // [N][DG_WORDS]
  u32 *const gen = curs + p.N * DG_WORDS;                                     // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const u32 LIN = N + CS;                                                     // endpoint (= lane) of lin-kv; lww-kv is LIN + 1
  const bool is_node = lane < N, is_client = lane >= N && lane < LIN, is_lin = lane == LIN, is_lww = lane == LIN + 1u;
  const bool is_server = is_node || is_lin || is_lww;                         // endpoints that poll all the time
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u64 lt_mask = (1ull << lane) - 1;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u32 all_nodes = (1u << N) - 1;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key, mv = p.cfg.max_values;
  const u32 TC = p.mk_tcap;   // tree nodes a node may create

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  // the per-instance scratch of dt_kernel<> (sim_kernel_dt.inc), same layout
  u32 *const g_kv = g_scr;                                           // [max_values][mw]: element | version << 8
  u32 *const g_kvn = g_kv + (size_t)mv * mw;                         // [max_values]
  u32 *const g_first = g_kvn + mv;                                   // [max_values] version at which the key entered the tree (DT_NONE: never)
  unsigned char *const g_hash = reinterpret_cast<unsigned char *>(g_first + mv);   // [max_values] Tree.hash of the key
  u32 *const g_rec = g_scr + (((size_t)mv * mw + 2u * mv + (mv + 3u) / 4u + 3u) & ~(size_t)3);   // [N][TC][DT_RW] tree nodes by pointer, on a 16-byte boundary
  u32 *const g_wl = g_rec + (size_t)N * TC * DT_RW;                  // [N][DT_MAXW] the pointers a node writes this round
  u32 *const g_cas = g_wl + (size_t)N * DT_MAXW;                     // [N][DT_CASQ] x {msg_id, from, transaction}: what a node's cas requests carry beside `to`
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 qidx = is_node ? lane : is_server ? N + (lane - LIN) : 0u;   // queue of a server endpoint (lin-kv: N, lww-kv: N + 1)
  const u32 my_cap = is_server ? p.cap_node : T_CLIENT_CAP;
  const u32 my_spill_cap = is_server ? p.spill_cap : 0u;
  uint4 *const my_inbox = inbox + (is_server ? qidx * p.cap_node : is_client ? (N + 2) * p.cap_node + slot * T_CLIENT_CAP : 0u);
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qidx * p.spill_cap;
  u32 *const cu = curs + (is_node ? lane : 0) * DG_WORDS;
  u32 *const my_wl = g_wl + (size_t)(is_node ? lane : 0) * DT_MAXW;

  for (u32 i = lane; i < N * DG_WORDS; i += 64) curs[i] = 0;
  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  for (u32 i = lane; i < mv; i += 64) { g_kvn[i] = 0; g_first[i] = DT_NONE; g_hash[i] = (unsigned char)dt_hash(i); }
  for (u32 i = lane; i < N * DT_CASQ * 3u; i += 64) g_cas[i] = 0;
  __syncthreads();

  // ---- endpoint state ----
  bool has_c = false; u32 deliver_at = 0; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, node_msgid = 0, part = 0;
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
    const u32 cnt = g_kvn[k];
    u32 n = 0;
    while (n < cnt && (g_kv[k * mw + n] >> 8) <= from) n++;
    return n;
  };

  for (;;) {
    #include "group64_phase.inc"
    if (__ballot((my_flags & MSIM_FLAG_ARENA_OVERRUN) != 0)) break;   // an engine capacity was exceeded: what follows would not be the program's behaviour

    // ---- R0: time ----
    #include "group64_time.inc"
    bool timeout_round = false;   // group64_jump.inc with the node's timer (Promise#await giving up) as a second event of the lane: merged into my_t it is other device code
    if (due > T && !__ballot(my_t <= T || wait_until <= T)) {
      u32 k = my_t == INF ? INF : my_t * 2;
      if (wait_until != INF) k = min(k, wait_until * 2);   // (a node's timer is a normal event)
      if (busy) k = min(k, timeout_at * 2 + 1);
      u32 km = wave_min(k);
      if (due != INF) km = min(km, due * 2);
      if (km == INF) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
      timeout_round = (km & 1) != 0;
      T = max(T, km >> 1);
    }

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
#define NODE_IX lane   // a node's index is its lane
#define DT_WAIT_RING
      #include "dt_node.inc"

      const bool await_over = is_node && wait_until <= T;   // a node's due timer comes before its due message (DESIGN.md §2.2 R3)
      const bool take = is_server && !await_over && has_c && deliver_at <= T;
      const u64 jd_mask = jcap ? __ballot(take) : 0ull;
      if (await_over) {   // Promise#await gave up (promise.rb:24-29): RPCError.timeout => error 0 to the client (node.rb:172), the lock is free
        reply(M_ERROR, 0, cu[DC_CMSG]);
        unlock();
      } else if (take) {
        const uint4 q = cm; has_c = false;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
        #include "dt_input.inc"
      }
      n_ev += (u32)__popcll(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = wave_incl_scan(need_words);
        const u32 total = rdlane(incl, 63);
        #include "dt_reads.inc"
      }

      // COMMIT: ids in lane order (nodes, lin-kv, lww-kv); a node's messages in the order it emitted them: the answer to a client,
      // then what the next step sends to a service
      {
        const u32 rcnt = rep ? 1u : 0u;
        const u32 cnt = is_node ? rcnt + n_out : (svc_rep ? 1u : 0u);
        const u32 incl = wave_incl_scan(cnt);
        const u32 total = rdlane(incl, 63);
        if (total) {
          const u32 my_off = incl - cnt;
          ev_base = n_ev; id_base = next_id; n_ev += total;
          if (is_node) { s_send_cl += rcnt; s_send_sv += n_out; } else s_send_sv += cnt;
          __syncthreads();   // (the write lists of this round are in HBM scratch)
          u64 ts = __ballot(is_node && cnt != 0);
          while (ts) {   // every sending node in turn: its answer to a client (taken in by that client's lane), then its messages to a service (taken in by the service's lane)
            const u32 s = (u32)__builtin_ctzll(ts); ts &= ts - 1;
            const u32 rc = rdlane(rcnt, s), off = rdlane(my_off, s);
            if (rc) {
              const u32 to = rdlane(r_to, s), ty = rdlane(r_type, s), a = rdlane(r_a, s), b = rdlane(r_b, s);
              if (lane == to) arrive(next_id + off, ty, a, b, s);
            }
            const u32 kn = rdlane(n_out, s);
            if (kn) {
              const u32 dst = rdlane(o_dest, s), t1 = rdlane(o1_type, s), a1 = rdlane(o1_a, s), b1 = rdlane(o1_b, s), wlo = rdlane(o_wlo, s);
              if (lane == LIN + dst) {
                if (wlo == 0u) arrive(next_id + off + rc, t1, a1, b1, s);
                else { const u32 *const wl = g_wl + (size_t)s * DT_MAXW;
                  for (u32 k = 0; k < kn; k++) arrive(next_id + off + rc + k, M_WRITE, wl[k], wlo + k, s); }
              }
            }
          }
          // service -> node
          u64 sv = __ballot(svc_rep);
          while (sv) {
            const u32 s = (u32)__builtin_ctzll(sv); sv &= sv - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), d = rdlane(o_to, s), off = rdlane(my_off, s);
            if (lane == d) arrive(next_id + off, ty, a, b, s);
          }
          next_id += total;
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
