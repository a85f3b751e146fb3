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

#define CRASH_STRIDE N
#define NODE_GIVES_UP
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
      u32 r_type = 0, r_a = 0, r_b = 0;    // the answer to the client
      u32 n_out = 0, o_dest = 0;           // node -> service: n_out messages, all to the same service; one in registers (o1_*) or DT_MAXW writes in my_wl[]
      u32 o1_type = 0, o1_a = 0, o1_b = 0, o_wlo = 0;
      u32 o_type = 0, o_a = 0, o_b = 0, o_to = 0, need_words = 0, done_ref = 0, done_rv = 0;   // service -> node; the completed transaction's payload
      // what dt_node.inc / dt_input.inc ask of the kernel: the answer goes to the client in the node's own lane, a client reference is its msg_id
#define REPLY_OK(type, cmsg) { rep = true; r_type = type; r_b = cmsg; }   // (r_a: filled in when the payload is laid out)
#define REPLY_ERROR(code, cmsg) { rep = true; r_type = M_ERROR; r_a = code; r_b = cmsg; }
#define CLIENT_REF(qb, qsrc) (qb)
#define NODE_IX lane   // a node's index is its lane
      #include "dt_node.inc"

      const u32 jd_mask = jcap ? (u32)__ballot(lane <= N + 1u && deliver_at <= T && !(is_node && wait_until <= T)) : 0u;
      const bool await_over = is_node && wait_until <= T;   // a node's due timer comes before its due message (DESIGN.md §2.2 R3)
      if (await_over) {   // Promise#await gave up (promise.rb:24-29): RPCError.timeout => error 0 to the client (node.rb:172), the lock is free
        REPLY_ERROR(0, cu[DC_CMSG]);
        unlock();
      } else if (lane <= N + 1u && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < LIN) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, is_node ? lane : N + lane);
        #include "dt_input.inc"
      }
      n_ev += __popc(jd_mask);

      // completed transactions: payload words allocated in node order, each node writes its own
      {
        const u32 incl = scan32(need_words);
        const u32 total = rdlane(incl, 31);
        #include "dt_reads.inc"
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
