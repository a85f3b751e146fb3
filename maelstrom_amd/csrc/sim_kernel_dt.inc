// sim_kernel_dt.inc — txn-list-append over the Datomic-style transactor node (SURVEY.md §8a row a18: the node core.clj:113-114 runs).
// Included by sim_kernels.h after sim_kernel_mk.inc (whose lane layout, message types and client code it shares).
//
//   node      demo/ruby/datomic_list_append.rb:47-424: a persistent hash tree (RING_SIZE 128, BRANCH_FACTOR 8, CRC32 of the key's
//             decimal string) of immutable nodes in lww-kv under fresh pointers "<node>-<n>", the root pointer in lin-kv; a
//             transaction takes the node's lock (:348), reads the root pointer (:358-365), loads the tree nodes on its keys' paths
//             lazily — a sync RPC per node that is not in the cache of what this node has LOADED, repeated until read_ok (:83-101,
//             :231-247) — copies the paths it appends to (:158-197, :256-268), writes the new nodes children first, all writes in
//             flight (:212-224, :291-320), and cas-es the root (:376-388); anything but cas_ok answers error 30; every blocking step gives up
//             after 5 s (Promise#await, promise.rb:5,17-30: error 0, the lock is free again)
//   services  lin-kv service.clj:31-61,141-155 (read / write / cas); lww-kv service.clj:214-243 over :65-114 (two replicas that
//             never exchange state, three rand-int draws per request)
//
// Lanes: lane i < N = node i + its client; lane N = lin-kv (endpoint 2N), lane N + 1 = lww-kv (endpoint 2N + 1).
// The specification is oracle/dt_nodes.inc, statement by statement: a pointer is (node << 20) | n ("empty" = 0); a tree node is a
// 12-word record in HBM scratch {kind | lo << 8 | hi << 16, keys in a leaf, version, replica, eight child pointers}; which keys a
// leaf holds follows from the lineage (keys first committed at a version <= the one read, + this transaction's own); list values are
// never materialised.  A node's cache is one bit per pointer.  A round's new tree nodes go to lww-kv through a pointer list in HBM
// scratch (their msg_ids are consecutive), the service lane takes the run in at COMMIT.

#define DT_WAITQ 8u
#define DT_MAXDEPTH 40u
#define DT_MAXW 256u
#define DT_NONE 0xFFFFFFFFu
#define DT_AWAIT_US 5000000u   // Promise::TIMEOUT (promise.rb:5)
#define DT_RW 12u     // words per tree-node record
#define DT_CASQ 4u    // cas requests of one node whose `from` / transaction are remembered (oracle/dt_nodes.inc)
enum { DS_IDLE = 0, DS_ROOT, DS_LOAD, DS_SAVE, DS_CAS, DS_INIT_LEAF, DS_INIT_ROOT };
// a node's transaction (the lock holder) in LDS
enum { DC_STAGE = 0, DC_CMSG, DC_REF, DC_RPC, DC_P1, DC_RV, DC_T, DC_TARGET, DC_PSTART, DC_WLO, DC_WN, DC_WOUT, DC_J, DC_NOWN, DC_OWN /* 8 */, DC_WQN = DC_OWN + 8, DC_WQ /* DT_WAITQ x {client msg, txn ref} */,
       DC_STK = DC_WQ + 2 * DT_WAITQ /* (DT_MAXDEPTH + 1) x {pointer, next child} */, DC_WORDS = DC_STK + 2 * (DT_MAXDEPTH + 1) };

// Tree.hash (:60-64): Zlib.crc32(k.to_s) % RING_SIZE
__device__ __forceinline__ u32 dt_hash(u32 k) {
  u32 dig[5], n = 0;
  do { dig[n++] = k % 10u; k /= 10u; } while (k);
  u32 c = 0xFFFFFFFFu;
  for (u32 i = n; i-- > 0;) {
    c ^= 48u + dig[i];
#pragma unroll
    for (u32 b = 0; b < 8; b++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return (~c) & 127u;
}
// tree nodes a node may create (engine capacity): the appends it can see, a path each, with room for the splits
// (an append copies its path: depth 4 up to 8 x 64 keys — root, sixteen-wide, two-wide, leaf — then a two-wide range grows a chain link
// per key beyond eight, :164-197)
static inline uint32_t dt_tcap(const msim_config &c) {
  const double ops = (double)c.rate_mhz * (double)c.time_limit_ms / 1e6 * 1.125 + 64.0;
  const double keys = c.key_count + ops * c.max_txn_length / 2.0 / c.max_writes_per_key;
  const double depth = 4.0 + (keys / 64.0 > 8.0 ? keys / 64.0 - 8.0 : 0.0);
  // transactions per node x appends per transaction ((L + 1) / 4: 1 .. L micro-ops, half of them appends) x a path each, twice over for the
  // transactions that lose the root cas and the uneven share of a node (an option sweep found the first form of this estimate short at
  // --max-txn-length 1: profiles/r05_fuzz_sweep.txt)
  uint32_t t = 256; while (t < ops / c.n_nodes * ((c.max_txn_length + 1) / 4.0) * depth * 2.0 + 64.0) t <<= 1;
  return t;
}
static inline uint64_t dt_scratch_words(const msim_config &c) {
  const uint64_t mv = c.max_values, tc = dt_tcap(c), n = c.n_nodes;
  return ((mv * c.max_writes_per_key + mv + mv + (mv + 3) / 4 + 3) & ~3ull) + n * tc * DT_RW + n * DT_MAXW + n * DT_CASQ * 3 + 4;   // (the tree nodes start on a 16-byte boundary: dt8.hip reads a record as three 16-byte words)
}

// A register budget for four wavefronts per SIMD: the kernel waits for dependent HBM loads (a walk down the tree per micro-op) with 7 of 64
// lanes live — cfg5 x 32768 clusters: 1570 ms at the compiler's own 180 registers (two wavefronts), 1131 ms at three, 1040 ms at four
// (gpurun_out/r5e/dt_occ.txt; tools/variant_lib.sh dtwN k_dt.hip -DDT_WAVES_PER_EU=N).
#ifndef DT_WAVES_PER_EU
#define DT_WAVES_PER_EU 4
#endif
#define DT_OCC __attribute__((amdgpu_waves_per_eu(DT_WAVES_PER_EU)))
template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) DT_OCC dt_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const curs = reinterpret_cast<u32 *>(smem + p.off_seen);             // [N][DC_WORDS]
  u32 *const gen = curs + p.N * DC_WORDS;                                     // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N;
  const bool is_node = lane < N, is_lin = lane == N;
  const u32 LIN = 2 * N;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u32 all_nodes = (1u << N) - 1;
  const u32 worker_mask = all_nodes;   // one worker per node: the client on the node's lane
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key, mv = p.cfg.max_values;
  const u32 TC = p.mk_tcap;   // tree nodes a node may create

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
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = p.cap_node, my_spill_cap = p.spill_cap;
  const u32 qlane = lane <= N + 1u ? lane : 0;
  uint4 *const my_inbox = inbox + qlane * my_cap;
  uint4 *const my_cinbox = inbox + (N + 2) * my_cap + (is_node ? lane : 0) * T_CLIENT_CAP;
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qlane * my_spill_cap;
  u32 *const cu = curs + (is_node ? lane : 0) * DC_WORDS;
  u32 *const my_wl = g_wl + (size_t)(is_node ? lane : 0) * DT_MAXW;
  const u32 my_client = N + lane;

  for (u32 i = lane; i < N * DC_WORDS; i += 64) curs[i] = 0;
  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  for (u32 i = lane; i < mv; i += 64) { g_kvn[i] = 0; g_first[i] = DT_NONE; g_hash[i] = (unsigned char)dt_hash(i); }
  for (u32 i = lane; i < N * DT_CASQ * 3u; i += 64) g_cas[i] = 0;
  __syncthreads();

  // ---- node / service state ----
  u32 deliver_at = INF; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, node_msgid = 0, part = 0;
  u32 next_p = 0;                                      // node: @ptr (:332, :352-355)
  u32 wait_until = INF;                                // node: when the lock holder's Promise#await gives up (promise.rb:5,17-30), INF: not waiting
  u32 casn = 0;                                        // node: cas requests so far
  u32 root = 0, root_exists = 0, cur_v = 0;            // lin-kv lane: the root pointer; versions so far
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
      if (type == MSIM_T_INFO) process += N;  // crashed process; the Reusable client itself lives on
    };
    auto client_deliver = [&](u32 qtype, u32 qa, u32 qb) {
      s_recv_cl++;
      if (busy && qb == want) {
        if (qtype == M_TXN_OK) complete(MSIM_T_OK, 0, qa);
        else if (qtype == M_ERROR)
          if (qa == 0u) complete(MSIM_T_INFO, MSIM_ERR_TIMEOUT, c_value);   // code 0 :timeout is not :definite? (errors.edn:2-4)
          else complete(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : qa == 30 ? MSIM_ERR_TXN_CONFLICT : qa == 14 ? MSIM_ERR_ABORT : MSIM_ERR_PRECONDITION_FAILED, c_value);
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
      u32 r_type = 0, r_a = 0, r_b = 0;    // the answer to the client
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
      auto start_txn = [&](u32 cmsg, u32 ref) {   // the lock is ours: current_tree (:358-365)
        cu[DC_STAGE] = DS_ROOT; cu[DC_CMSG] = cmsg; cu[DC_REF] = ref; cu[DC_J] = 0; cu[DC_NOWN] = 0;
        const u32 rid = ++node_msgid; cu[DC_RPC] = rid;
        send1(D_LIN, M_READ, 0, rid);
        wait_until = T + DT_AWAIT_US;
      };
      auto unlock = [&]() {   // the next waiting transaction takes the lock (:348, :371)
        cu[DC_STAGE] = DS_IDLE;
        wait_until = INF;
        const u32 wqn = cu[DC_WQN];
        if (wqn) {
          const u32 cmsg = cu[DC_WQ], ref = cu[DC_WQ + 1];
          for (u32 i = 1; i < wqn; i++) { cu[DC_WQ + 2 * (i - 1)] = cu[DC_WQ + 2 * i]; cu[DC_WQ + 2 * (i - 1) + 1] = cu[DC_WQ + 2 * i + 1]; }
          cu[DC_WQN] = wqn - 1;
          start_txn(cmsg, ref);
        }
      };
      auto load = [&](u32 ptr) {   // Tree.load with a cache miss (:83-101)
        const u32 rid = ++node_msgid;
        cu[DC_STAGE] = DS_LOAD; cu[DC_TARGET] = ptr; cu[DC_RPC] = rid;
        send1(D_LWW, M_READ, ptr, rid);
        wait_until = T + DT_AWAIT_US;
      };
      // walks to the key's leaf; the first tree node on the way that has to be fetched, DT_NONE if the path is in memory.  One round trip per
      // level: a record's kind / range, its flags word (which nodes have loaded it) and its eight children are loaded together.
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
      // assoc (:158-197, :256-268) along a path that is in memory.  New pointers go leaf first, then upwards: with n branches above a
      // leaf level of L new nodes (1, or 8 leaves + their branch) the leaf level takes base+1 .. base+L, the branch at depth i
      // base+L+(n-i) — known before the walk down that writes the copies.
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
      // save! (:212-224, :291-320): the new tree nodes the final tree reaches, children before their parent.  A stack entry is a tree node and
      // the mask of its new children still to visit (a branch's eight children are loaded together: one round trip per visit).
      auto save = [&]() {
        u32 *const stk = cu + DC_STK;
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
        rep = true; r_type = M_TXN_OK; r_b = cu[DC_CMSG];
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

      const u32 jd_mask = jcap ? (u32)__ballot(lane <= N + 1u && deliver_at <= T && !(is_node && wait_until <= T)) : 0u;
      const bool await_over = is_node && wait_until <= T;   // a node's due timer comes before its due message (DESIGN.md §2.2 R3)
      if (await_over) {   // Promise#await gave up (promise.rb:24-29): RPCError.timeout => error 0 to the client (node.rb:172), the lock is free
        rep = true; r_type = M_ERROR; r_a = 0; r_b = cu[DC_CMSG];
        unlock();
      } else if (lane <= N + 1u && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, is_node ? lane : N + lane);
        if (is_node) {
          const u32 st = cu[DC_STAGE];
          switch (qtype) {
            case M_INIT:
              if (lane != 0u) { rep = true; r_type = M_INIT_OK; r_b = qb; break; }
              {   // the first node writes the initial state (:337-345): Tree.empty, then the root pointer
                u32 *const r = g_rec;
                r[0] = (128u << 16); r[1] = 0; r[2] = 0; __hip_atomic_store(r + 3, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u32 rid = ++node_msgid;
                cu[DC_STAGE] = DS_INIT_LEAF; cu[DC_CMSG] = qb; cu[DC_RPC] = rid;
                send1(D_LWW, M_WRITE, 0, rid);
              } break;
            case M_TXN:
              if (st == DS_IDLE) start_txn(qb, qa);
              else { const u32 wqn = cu[DC_WQN];
                if (wqn == DT_WAITQ) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
                else { cu[DC_WQ + 2u * wqn] = qb; cu[DC_WQ + 2u * wqn + 1u] = qa; cu[DC_WQN] = wqn + 1u; } }
              break;
            case M_READ_OK: case M_WRITE_OK: case M_CAS_OK: case M_ERROR:
              switch (st) {
                case DS_INIT_LEAF:
                  if (qb != cu[DC_RPC]) break;
                  { const u32 rid = ++node_msgid; cu[DC_STAGE] = DS_INIT_ROOT; cu[DC_RPC] = rid; send1(D_LIN, M_WRITE, 0, rid); }
                  break;
                case DS_INIT_ROOT:
                  if (qb != cu[DC_RPC]) break;
                  cu[DC_STAGE] = DS_IDLE; rep = true; r_type = M_INIT_OK; r_b = cu[DC_CMSG];
                  break;
                case DS_ROOT:
                  if (qb != cu[DC_RPC]) break;
                  if (qtype != M_READ_OK) { rep = true; r_type = M_ERROR; r_a = 14; r_b = cu[DC_CMSG]; unlock(); break; }   // "Unsure how to handle" (:364)
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
                  else { rep = true; r_type = M_ERROR; r_a = 30; r_b = cu[DC_CMSG]; }   // txn_conflict (:385)
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
          else {   // cas, no create_if_not_exists.  The request is self-contained (:376-388): its `from` and its transaction come from the sender's
            // table of cas requests under the msg_id, not from what the sender holds NOW (it may have given up on this cas and moved on)
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
      n_ev += __popc(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = scan32(need_words);
        const u32 total = rdlane(incl, 31);
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

      // COMMIT: ids in lane order (nodes, lin-kv, lww-kv); a node's messages in the order it emitted them: the answer to its client,
      // then what the next step sends to a service
      bool c_arr = false; u32 ca_y = 0, ca_a = 0, ca_b = 0;
      {
        const u32 rcnt = rep ? 1u : 0u;
        const u32 cnt = is_node ? rcnt + n_out : (svc_rep ? 1u : 0u);
        const u32 incl = scan32(cnt);
        const u32 total = rdlane(incl, 31);
        if (total) {
          const u32 my_off = incl - cnt;
          ev_base = n_ev; id_base = next_id; n_ev += total;
          if (is_node) { s_send_cl += rcnt; s_send_sv += n_out; } else s_send_sv += cnt;
          // node -> service: the service lane takes each node's run in node order
          __syncthreads();   // (the write lists of this round are in HBM scratch)
          u32 ts = (u32)__ballot(is_node && n_out != 0);
          while (ts) {
            const u32 s = (u32)__builtin_ctz(ts); ts &= ts - 1;
            const u32 dst = rdlane(o_dest, s), kn = rdlane(n_out, s), off = rdlane(my_off, s) + rdlane(rcnt, s);
            const u32 t1 = rdlane(o1_type, s), a1 = rdlane(o1_a, s), b1 = rdlane(o1_b, s), wlo = rdlane(o_wlo, s);
            if (lane == N + dst) {
              if (wlo == 0u) arrive(next_id + off, t1, a1, b1, s, LIN + dst);
              else { const u32 *const wl = g_wl + (size_t)s * DT_MAXW;
                for (u32 k = 0; k < kn; k++) arrive(next_id + off + k, M_WRITE, wl[k], wlo + k, s, LIN + dst); }
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
            if (jcap) jwrite(ev_base + my_off, 0, (id << 8) | r_type, r_a, r_b, lane, my_client);
            if (!(NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss)) { c_arr = true; ca_y = (id << 8) | r_type; ca_a = r_a; ca_b = r_b; }
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
