// sim_kernel_dtg.inc — the Datomic-style txn-list-append node (sim_kernel_dt.inc, SURVEY.md §8a row a18) with SEVERAL WORKERS PER NODE
// (`--concurrency 10n`, the reference's own invocation for this workload: doc/05-datomic/01-single-node.md:257,322).  Included by sim_kernels.h
// after sim_kernel_dt.inc, whose scratch layout, record format, stages and node / service transition code it repeats statement for statement.
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

    auto complete = [&](u32 type, u32 err, u32 ref) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (MSIM_F_TXN << 2) | (err << 7) | (process << 12);
      cmp_value = ref & 0xFFFFFFu; cmp_len = ref >> 24;
      if (type == MSIM_T_INFO) process += C;  // crashed process; the Reusable client itself lives on
    };

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
      auto rec_of = [&](u32 ptr) -> u32 * { return g_rec + ((size_t)(ptr >> 20) * TC + (ptr & 0xFFFFFu)) * DT_RW; };
      auto is_new = [&](u32 ptr) -> bool { return (ptr >> 20) == lane && (ptr & 0xFFFFFu) >= cu[DC_PSTART]; };
      auto has_key = [&](u32 k) -> bool {   // the key is in the lineage of the working tree
        if (g_first[k] <= cu[DC_RV]) return true;   // (DT_NONE is above every version)
        const u32 no = cu[DC_NOWN];
        for (u32 i = 0; i < no; i++) if (cu[DC_OWN + i] == k) return true;
        return false;
      };
      auto br_index = [&](u32 w0, u32 h) -> u32 {   // branch_index (:231-247) with the split's bounds (:170-181)
        const u32 lo = (w0 >> 8) & 0xFFu, hi = (w0 >> 16) & 0xFFu, bs = (hi - lo) / 8u;
        for (u32 i = 0; i < 7u; i++) if (h < lo + (i + 1u) * bs) return i;
        return 7u;
      };
      auto send1 = [&](u32 dest, u32 type, u32 a, u32 b) { o_dest = dest; n_out = 1; o1_type = type; o1_a = a; o1_b = b; };
      auto reply = [&](u32 type, u32 a, u32 cmsg) { rep = true; r_type = type; r_a = a; r_to = cmsg >> 24; r_b = cmsg & 0xFFFFFFu; };   // (cmsg = the client's msg_id | its endpoint << 24)
      auto start_txn = [&](u32 cmsg, u32 ref) {   // the lock is ours: current_tree (:358-365)
        cu[DC_STAGE] = DS_ROOT; cu[DC_CMSG] = cmsg; cu[DC_REF] = ref; cu[DC_J] = 0; cu[DC_NOWN] = 0;
        const u32 rid = ++node_msgid; cu[DC_RPC] = rid;
        send1(D_LIN, M_READ, 0, rid);
        wait_until = T + DT_AWAIT_US;
      };
      auto unlock = [&]() {   // the next waiting transaction takes the lock (:348, :371), in arrival order
        cu[DC_STAGE] = DS_IDLE;
        wait_until = INF;
        const u32 wq = cu[DG_WQN], cnt = wq & 0xFFu, head = wq >> 8;
        if (cnt) {
          const u32 cmsg = cu[DG_WQ + 2u * head], ref = cu[DG_WQ + 2u * head + 1u];
          cu[DG_WQN] = (cnt - 1u) | (((head + 1u) & (DG_WAITQ - 1u)) << 8);
          start_txn(cmsg, ref);
        }
      };
      auto load = [&](u32 ptr) {   // Tree.load with a cache miss (:83-101)
        const u32 rid = ++node_msgid;
        cu[DC_STAGE] = DS_LOAD; cu[DC_TARGET] = ptr; cu[DC_RPC] = rid;
        send1(D_LWW, M_READ, ptr, rid);
        wait_until = T + DT_AWAIT_US;
      };
      // walks to the key's leaf; the first tree node on the way that has to be fetched, DT_NONE if the path is in memory
      auto descend = [&](u32 k) -> u32 {
        const u32 h = g_hash[k];
        u32 pt = cu[DC_T];
        for (u32 d = 0; d < DT_MAXDEPTH; d++) {
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0], w3 = __hip_atomic_load(r + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (word 3 is the one word of a record that changes after its creation, by L2 atomics: read past the L1)
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          if (!is_new(pt) && !((w3 >> (2u + lane)) & 1u)) return pt;   // neither created by this transaction nor loaded by this node
          if ((w0 & 1u) == 0u) return DT_NONE;
          const u32 ci = br_index(w0, h);
          pt = ch[0];
#pragma unroll
          for (u32 c = 1; c < 8u; c++) pt = c == ci ? ch[c] : pt;
        }
        my_flags |= MSIM_FLAG_ARENA_OVERRUN;
        return DT_NONE;
      };
      // assoc (:158-197, :256-268) along a path that is in memory (sim_kernel_dt.inc)
      auto assoc = [&](u32 k) {
        const u32 h = g_hash[k];
        u32 n = 0, pt = cu[DC_T];
        for (; n + 1u < DT_MAXDEPTH; n++) {
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0];
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          if ((w0 & 1u) == 0u) break;
          const u32 ci = br_index(w0, h);
          pt = ch[0];
#pragma unroll
          for (u32 c = 1; c < 8u; c++) pt = c == ci ? ch[c] : pt;
        }
        const u32 *const lf = rec_of(pt);
        const u32 lw0 = lf[0], lcount = lf[1];
        if (lw0 & 1u) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; return; }
        const bool has = has_key(k);
        const u32 L = (has || lcount < 8u) ? 1u : 9u, base = next_p, ver = cu[DC_RV] + 1u;
        if (base + L + n >= TC) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; return; }   // engine capacity
        const u32 lo = (lw0 >> 8) & 0xFFu, hi = (lw0 >> 16) & 0xFFu;
        auto put = [&](u32 idx, u32 w0, u32 cnt) -> u32 * { u32 *const r = g_rec + ((size_t)lane * TC + idx) * DT_RW; r[0] = w0; r[1] = cnt; r[2] = ver; __hip_atomic_store(r + 3, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return r; };   // (word 3: lww-kv replica in bits 0-1, 3 = not written; bit 2 + i: node i has loaded it)
        if (L == 1u) put(base + 1u, lw0, lcount + (has ? 0u : 1u));
        else {   // eight leaves under a new branch: the lineage's keys of this range (and the new one) by sub-range
          const u32 bs = (hi - lo) / 8u, nk = gen[32];
          u64 c_lo = 0, c_hi = 0;   // 4 x 16-bit counters each
          for (u32 q = 0; q < nk; q++) {
            if (q != k && !has_key(q)) continue;
            const u32 hq = g_hash[q];
            if (hq < lo || hq >= hi) continue;
            const u32 ci = bs ? min((hq - lo) / bs, 7u) : 7u;
            if (ci < 4u) c_lo += 1ull << (16u * ci); else c_hi += 1ull << (16u * (ci - 4u));
          }
          u32 *const br = put(base + 9u, 1u | (lo << 8) | (hi << 16), 0u);
          for (u32 i = 0; i < 8u; i++) {
            const u32 b_lo = lo + i * bs, b_hi = i == 7u ? hi : b_lo + bs;
            const u32 cnt = (u32)((i < 4u ? c_lo >> (16u * i) : c_hi >> (16u * (i - 4u))) & 0xFFFFu);
            put(base + 1u + i, (b_lo << 8) | (b_hi << 16), cnt);
            br[4u + i] = (lane << 20) | (base + 1u + i);
          }
        }
        pt = cu[DC_T];
        for (u32 i = 0; i < n; i++) {   // a copy of every branch above, pointing at the new child
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0], ci = br_index(w0, h);
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          u32 *const nr = put(base + L + (n - i), w0, 0u);
          const u32 child_new = (lane << 20) | (i + 1u == n ? base + L : base + L + (n - i - 1u));
#pragma unroll
          for (u32 c = 0; c < 8u; c++) nr[4u + c] = c == ci ? child_new : ch[c];
          pt = ch[0];
#pragma unroll
          for (u32 c = 1; c < 8u; c++) pt = c == ci ? ch[c] : pt;
        }
        next_p = base + L + n;
        cu[DC_T] = (lane << 20) | next_p;
        if (!has) { const u32 no = cu[DC_NOWN]; if (no < 8u) { cu[DC_OWN + no] = k; cu[DC_NOWN] = no + 1u; } }
      };
      // save! (:212-224, :291-320): the new tree nodes the final tree reaches, children before their parent (sim_kernel_dt.inc)
      auto save = [&]() {
        u32 *const stk = cu + DG_STK;
        u32 sp = 1, wn = 0;
        const u32 wlo = node_msgid + 1u;
        stk[0] = cu[DC_T]; stk[1] = 0x100u;   // (0x100: not looked at yet)
        while (sp) {
          const u32 pt = stk[2u * (sp - 1u)];
          u32 mask = stk[2u * (sp - 1u) + 1u];
          const u32 *const r = rec_of(pt);
          const u32 w0 = r[0];
          u32 ch[8];
#pragma unroll
          for (u32 c = 0; c < 8u; c++) ch[c] = r[4u + c];
          if (mask & 0x100u) {
            mask = 0;
            if (w0 & 1u) {
#pragma unroll
              for (u32 c = 0; c < 8u; c++) mask |= is_new(ch[c]) ? 1u << c : 0u;
            }
          }
          if (mask) {
            const u32 ci = (u32)__builtin_ctz(mask);
            u32 nxt = ch[0];
#pragma unroll
            for (u32 c = 1; c < 8u; c++) nxt = c == ci ? ch[c] : nxt;
            stk[2u * (sp - 1u) + 1u] = mask & (mask - 1u);
            if (sp > DT_MAXDEPTH) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; stk[2u * (sp - 1u) + 1u] = 0; continue; }
            stk[2u * sp] = nxt; stk[2u * sp + 1u] = 0x100u; sp++;
            continue;
          }
          if (wn >= DT_MAXW) my_flags |= MSIM_FLAG_ARENA_OVERRUN; else my_wl[wn++] = pt;
          sp--;
        }
        node_msgid += wn;
        cu[DC_STAGE] = DS_SAVE; cu[DC_WLO] = wlo; cu[DC_WN] = wn; cu[DC_WOUT] = wn;
        o_dest = D_LWW; n_out = wn; o_wlo = wlo;
        wait_until = T + DT_AWAIT_US;   // `tree2.save!.await` (:366)
      };
      auto reply_txn_ok = [&]() {   // the completed transaction: its reads see the version read + its own appends
        reply(M_TXN_OK, 0, cu[DC_CMSG]);
        done_ref = cu[DC_REF]; done_rv = cu[DC_RV];
        const u32 off0 = done_ref & 0xFFFFFFu, n = done_ref >> 24;
        for (u32 j = 0; j < n; j++) {
          const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
          need_words++;
          if (!(w & 1u)) {
            u32 len = visible(k, done_rv);
            for (u32 e = 0; e < j; e++) { const u32 we = g_pay[off0 + e]; if ((we & 1u) && ((we >> 1) & 0x7FFFu) == k) len++; }
            need_words += (len + 3u) / 4u;
          }
        }
      };
      // apply_txn (:391-415) from micro-op j on; stops at the first tree node that has to be fetched
      auto apply = [&]() {
        const u32 ref = cu[DC_REF], off0 = ref & 0xFFFFFFu, n = ref >> 24;
        u32 j = cu[DC_J];
        while (j < n) {
          const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
          const u32 miss = descend(k);   // t[k] — for an append too (:405)
          if (miss != DT_NONE) { cu[DC_J] = j; load(miss); return; }
          if (w & 1u) assoc(k);
          j++;
        }
        cu[DC_J] = j;
        if (cu[DC_T] == cu[DC_P1]) { reply_txn_ok(); unlock(); return; }   // nothing appended: no write, no cas
        save();
      };

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
        if (is_node) {
          const u32 st = cu[DC_STAGE];
          switch (qtype) {
            case M_INIT:
              if (lane != 0u) { reply(M_INIT_OK, 0, qb | (qsrc << 24)); break; }
              {   // the first node writes the initial state (:337-345): Tree.empty, then the root pointer
                u32 *const r = g_rec;
                r[0] = (128u << 16); r[1] = 0; r[2] = 0; __hip_atomic_store(r + 3, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u32 rid = ++node_msgid;
                cu[DC_STAGE] = DS_INIT_LEAF; cu[DC_CMSG] = qb | (qsrc << 24); cu[DC_RPC] = rid;
                send1(D_LWW, M_WRITE, 0, rid);
              } break;
            case M_TXN:
              if (st == DS_IDLE) start_txn(qb | (qsrc << 24), qa);
              else { const u32 wq = cu[DG_WQN], cnt = wq & 0xFFu;
                if (cnt == DG_WAITQ) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
                else { const u32 sl = ((wq >> 8) + cnt) & (DG_WAITQ - 1u); cu[DG_WQ + 2u * sl] = qb | (qsrc << 24); cu[DG_WQ + 2u * sl + 1u] = qa; cu[DG_WQN] = wq + 1u; } }
              break;
            case M_READ_OK: case M_WRITE_OK: case M_CAS_OK: case M_ERROR:
              switch (st) {
                case DS_INIT_LEAF:
                  if (qb != cu[DC_RPC]) break;
                  { const u32 rid = ++node_msgid; cu[DC_STAGE] = DS_INIT_ROOT; cu[DC_RPC] = rid; send1(D_LIN, M_WRITE, 0, rid); }
                  break;
                case DS_INIT_ROOT:
                  if (qb != cu[DC_RPC]) break;
                  cu[DC_STAGE] = DS_IDLE; reply(M_INIT_OK, 0, cu[DC_CMSG]);
                  break;
                case DS_ROOT:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype != M_READ_OK) { reply(M_ERROR, 14, cu[DC_CMSG]); unlock(); break; }   // "Unsure how to handle" (:364)
                  cu[DC_P1] = qa; cu[DC_T] = qa; cu[DC_PSTART] = next_p + 1u;
                  { const u32 *const rr = rec_of(qa); const u32 rv2 = rr[2], rw3 = __hip_atomic_load(rr + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); cu[DC_RV] = rv2; if ((rw3 >> (2u + lane)) & 1u) apply(); else load(qa); }
                  break;
                case DS_LOAD:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype == M_READ_OK) { atomicOr(rec_of(cu[DC_TARGET]) + 3, 1u << (2u + lane)); apply(); }   // @@cache[ptr] = tree (:95)
                  else load(cu[DC_TARGET]);   // "Retrying read of tree node" (:97)
                  break;
                case DS_SAVE:
                  if (qb < cu[DC_WLO] || qb >= cu[DC_WLO] + cu[DC_WN]) break;
                  { const u32 left = cu[DC_WOUT] - 1u; cu[DC_WOUT] = left;
                    if (left == 0u) { const u32 rid = ++node_msgid; cu[DC_STAGE] = DS_CAS; cu[DC_RPC] = rid;   // advance_root! (:376-388): cas root from the pointer read to the new one
                      { u32 *const ce = g_cas + ((size_t)lane * DT_CASQ + (casn++ % DT_CASQ)) * 3u; ce[0] = rid; ce[1] = cu[DC_P1]; ce[2] = cu[DC_REF]; }
                      send1(D_LIN, M_CAS, cu[DC_T], rid); wait_until = T + DT_AWAIT_US; } }
                  break;
                case DS_CAS:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype == M_CAS_OK) reply_txn_ok();
                  else reply(M_ERROR, 30, cu[DC_CMSG]);   // txn_conflict (:385)
                  unlock();
                  break;
                default: break;   // "Ignoring reply ... with no callback" (node.rb:160-162)
              }
              break;
            default: break;
          }
        } else if (is_lin) {   // lin-kv over the key "root" (service.clj:31-61)
          svc_rep = true; o_to = qsrc; o_b = qb;
          if (qtype == M_READ) {
            if (!root_exists) { o_type = M_ERROR; o_a = 20; } else { o_type = M_READ_OK; o_a = root; }
          } else if (qtype == M_WRITE) { root = qa; root_exists = 1u; o_type = M_WRITE_OK; o_a = 0; }
          else {   // cas, no create_if_not_exists: self-contained (:376-388) — `from` and the transaction under the msg_id in the sender's table
            u32 c_from = 0, c_ref = 0; bool c_hit = false;
            { const u32 *const ce = g_cas + (size_t)qsrc * DT_CASQ * 3u;
#pragma unroll
              for (u32 i = 0; i < DT_CASQ; i++) { const u32 e0 = ce[3u * i], e1 = ce[3u * i + 1u], e2 = ce[3u * i + 2u]; if (e0 == qb) { c_hit = true; c_from = e1; c_ref = e2; } } }
            if (!c_hit) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; o_type = M_ERROR; o_a = 22; }   // engine capacity: DT_CASQ outstanding cas requests per node
            else if (!root_exists) { o_type = M_ERROR; o_a = 20; }
            else if (root != c_from) { o_type = M_ERROR; o_a = 22; }
            else {
              const u32 ref = c_ref, off0 = ref & 0xFFFFFFu, n = ref >> 24, v = ++cur_v;
              root = qa;
              for (u32 i = 0; i < n; i++) { const u32 w = g_pay[off0 + i];
                if (w & 1u) { const u32 k = (w >> 1) & 0x7FFFu, c = g_kvn[k]; if (g_first[k] == DT_NONE) g_first[k] = v;
                  g_kv[k * mw + c] = ((w >> 16) & 0xFFu) | (v << 8); g_kvn[k] = c + 1u; } }
              o_type = M_CAS_OK; o_a = 0;
            }
          }
        } else {   // lww-kv (service.clj:214-243 as written): merge-source, merge-dest, then the replica that serves the request
          svc_rep = true; o_to = qsrc; o_b = qb;
          svc_ctr += 2u;
          const u32 r = scale32(draw32(key, 12u /* S_SVC */, svc_ctr++), 2);
          u32 *const rp = rec_of(qa) + 3;   // (the replica bits; the nodes set their "loaded" bits in the same word: atomics)
          if (qtype == M_WRITE) { atomicAnd(rp, ~3u); atomicOr(rp, r); o_type = M_WRITE_OK; o_a = qa; }
          else if ((__hip_atomic_load(rp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 3u) == r) { o_type = M_READ_OK; o_a = qa; }
          else { o_type = M_ERROR; o_a = 20; }
        }
      }
      n_ev += (u32)__popcll(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = wave_incl_scan(need_words);
        const u32 total = rdlane(incl, 63);
        if (total) {
          if (n_payload + total > max_pay) { flags |= MSIM_FLAG_PAYLOAD_OVERFLOW; if (need_words) r_a = 0; }
          else {
            if (need_words) {
              const u32 off0 = done_ref & 0xFFFFFFu, n = done_ref >> 24;
              u32 pp = n_payload + incl - need_words;
              r_a = pp | (need_words << 24);
              for (u32 j = 0; j < n; j++) {
                const u32 w = g_pay[off0 + j], k = (w >> 1) & 0x7FFFu;
                if (w & 1u) { g_pay[pp++] = w; continue; }
                const u32 vis = visible(k, done_rv);
                u32 e = 0, acc = 0;
                const u32 hdr = pp++;
                for (u32 i = 0; i < vis; i++) { acc |= (g_kv[k * mw + i] & 0xFFu) << (8 * (e & 3)); if ((++e & 3) == 0) { g_pay[pp++] = acc; acc = 0; } }
                for (u32 i = 0; i < j; i++) { const u32 wi = g_pay[off0 + i];
                  if ((wi & 1u) && ((wi >> 1) & 0x7FFFu) == k) { acc |= ((wi >> 16) & 0xFFu) << (8 * (e & 3)); if ((++e & 3) == 0) { g_pay[pp++] = acc; acc = 0; } } }
                if (e & 3) g_pay[pp++] = acc;
                g_pay[hdr] = (k << 1) | ((e ? e : 0xFFu) << 16);  // a key without elements reads nil
              }
            }
            n_payload += total;
          }
        }
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
