// sim_kernel_svc.inc — the lin-kv workload served by proxying to a Maelstrom-provided key-value service (SURVEY.md §8a
// row a17).  Included by engine.hip after sim_kernel_raft.inc, whose general layout, lin-kv clients and generator it shares.
//
//   node      demo/ruby/lin_kv_proxy.rb:8-43: read / write / cas from a client -> rpc! the body to the service (msg_id =
//             ++next_msg_id, callback stored under it); the service's reply is relayed to the client with its msg_id.
//   services  service.clj:31-61 PersistentKV behind  lin-kv = Linearizable (:141-155),  seq-kv = Sequential (:161-210, ring
//             of 32 states, non-mutating requests may be served from any state since the requesting node's last one),
//             lww-kv = Eventual over LWWKV (:65-114,:214-243; 2 replicas that — as the reference is written — never merge).
// Lanes: nodes, client slots, then ONE service lane (endpoint N + CS).  Service state in LDS: lin-kv 256 B; seq-kv ring
// 32 x 256 B + one index per node; lww-kv 2 x 256 B.  Callbacks: 32 per node in LDS, slot = rpc id mod 32.
// TSO = the unique-ids workload over the lin-tso service (service.clj:116-132): the same relay node with `generate` -> {type "ts"}
// -> `generate_ok` {id <ts>}, the service lane hands out 0, 1, 2, ...; clients and generator of workload/unique_ids.clj.
// Same specification as oracle/svc_nodes.inc, bit for bit.

#define PX_SLOTS 32u
// Envelopes of a client's inbox kept in LDS; the other R_CLIENT_CAP - PX_CL (the Reusable client collects late replies between RPCs: 32 in all, the
// oracle's limit) spill to HBM scratch behind the servers' spill (round 6: 32 LDS slots for each of the ten clients of the demo shape were 5 KiB of a
// cluster's 11.5 — a client's inbox holds one envelope nearly always)
#ifndef PX_CL   // (tests: a -DPX_CL=1u build of k_svc.hip + engine.hip sends every second envelope of a client through the spill)
#define PX_CL 4u
#endif
enum { S_SVC = 12 };
enum { M_TS = 28, M_TS_OK = 29 };   // include/maelsim.h MSIM_M_TS*

template <bool NEM, bool NET_RANDOM, bool TSO>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) svc_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  uint2 *const cbs = reinterpret_cast<uint2 *>(smem + p.off_seen);                    // [N][PX_SLOTS] {rpc_id | client << 24, client_msg | used << 31}
  // service states, 256 B each: states 32 and 33 (lin-kv / the lww replicas / seq-kv's scratch) come first, seq-kv's ring 0..31 behind them —
  // and only seq-kv has it (round 6: 8 KiB of LDS less per cluster for the other services, the reference's demo shape among them)
  unsigned char *const kvs0 = smem + p.off_seen + p.N * PX_SLOTS * 8;
  const u32 n_states = (!TSO && p.cfg.proxy_service == MSIM_SVC_SEQ_KV) ? 34u : 2u;
#define KVS(i_) (kvs0 + (((i_) >= 32u ? (i_) - 32u : (i_) + 2u) * 256u))
  u32 *const cidx = reinterpret_cast<u32 *>(kvs0 + n_states * 256);                   // seq-kv: last state index seen per node
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const u32 SVC = N + CS;
  const bool is_node = lane < N;
  const bool is_client = lane >= N && lane < N + CS;
  const bool is_svc = lane == SVC;
  const bool is_server = is_node || is_svc;   // endpoints that poll all the time and see latency
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u64 lt_mask = (1ull << lane) - 1;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u32 all_nodes = (1u << N) - 1;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz;
  u32 rpc_timeout_ms = 10 * lat_mean; if (rpc_timeout_ms < 1000) rpc_timeout_ms = 1000;   // lin_kv.clj:54
  if (TSO) rpc_timeout_ms = p.cfg.client_timeout_ms;                                       // client.clj:18-20

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;

  const u32 qidx = is_node ? lane : N;   // queue index of a server endpoint (the service is queue N)
  const u32 my_cap = is_server ? p.cap_node : PX_CL;
  const u32 my_spill_cap = is_server ? p.spill_cap : (is_client ? R_CLIENT_CAP - PX_CL : 0u);
  uint4 *const my_inbox = inbox + (is_server ? qidx * p.cap_node : (is_client ? (N + 1) * p.cap_node + slot * PX_CL : 0));
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (is_server ? (size_t)qidx * p.spill_cap : (size_t)(N + 1) * p.spill_cap + (size_t)(is_client ? slot : 0) * (R_CLIENT_CAP - PX_CL));
  uint2 *const my_cbs = cbs + (is_node ? lane : 0) * PX_SLOTS;

  for (u32 i = lane; i < N * PX_SLOTS; i += 64) cbs[i] = make_uint2(0, 0);
  for (u32 i = lane; i < n_states * 64; i += 64) reinterpret_cast<u32 *>(kvs0)[i] = 0xFFFFFFFFu;
  for (u32 i = lane; i < 64; i += 64) cidx[i] = 0;
  __syncthreads();

  // ---- endpoint state ----
  bool has_c = false; u32 deliver_at = 0; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, part = 0;
  u32 node_msgid = 0, last_index = 0, svc_ctr = 0;   // node: rpc ids; service lane: seq-kv's newest state, rand-int draws so far
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_f = 0, c_value = 0, process = slot;
  u32 dest_node = is_client ? slot % N : 0; const u32 c_mod_n = C % N;
  u32 m_f = 0, m_value = 0, key_reg = INF;
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0, cur_key = 0, key_procs = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

#define PAYS_LATENCY(src) (((src) < N || (src) == SVC) && is_server)   // neither end is a client (group64_net.inc)
#define ENDPOINT_LANES   // a lane is one endpoint: node, worker slot or service
#define COMMIT_FLAG   // has_c says whether an envelope is committed
#define POLL_LANE (is_server || busy)   // the lanes that take from their queue (group64_poll.inc)
  #include "group64_net.inc"
  #include "group64_poll.inc"
  // PersistentKV/handle on the 256-byte state m (service.clj:31-61); returns whether the state changed
  auto kv_handle = [&](unsigned char *m, u32 type, u32 a, u32 &rt, u32 &ra) -> bool {
    const u32 k = a & 0xFF, v1 = (a >> 8) & 0xFF, v2 = (a >> 16) & 0xFF;
    const u32 cur = m[k];
    ra = 0;
    if (type == M_READ) { if (cur == 0xFF) { rt = M_ERROR; ra = 20; } else { rt = M_READ_OK; ra = cur; } return false; }
    if (type == M_WRITE) { m[k] = (unsigned char)v1; rt = M_WRITE_OK; return cur != v1; }
    if (cur == 0xFF) { rt = M_ERROR; ra = 20; return false; }
    if (cur != v1) { rt = M_ERROR; ra = 22; return false; }
    m[k] = (unsigned char)v2; rt = M_CAS_OK; return v1 != v2;
  };

  for (;;) {
    #include "group64_phase.inc"

    // ---- R0: time ----
    #include "group64_time.inc"
    #include "group64_jump.inc"

    bool inv_row = false; u32 inv_packed = 0, inv_value = 0;
    const u32 inv_len = 0, cmp_len = 0;   // this program's rows carry no length (group64_rows.inc)
    bool cmp_row = false; u32 cmp_packed = 0, cmp_value = 0;
    u32 nem_rows = 0, nem_f = 0, nem_v1 = 0, nem_v2 = 0, nem_len2 = 0;

    auto complete = [&](u32 type, u32 err, u32 value) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (c_f << 2) | (err << 7) | (process << 12); cmp_value = value;
      if (type == MSIM_T_INFO) { process += C; dest_node += c_mod_n; if (dest_node >= N) dest_node -= N; }  // Reusable: client stays open
    };

    if (timeout_round) {
      if (busy && timeout_at <= T) complete(c_f == MSIM_F_READ ? MSIM_T_FAIL : MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_value);  // lin_kv.clj:52
    } else {
      // ---- R1: scheduler ----
      if (due <= T) {
        switch (phase) {
          case PH_INIT: if (is_client && slot < N) { mark = true; kind = K_INIT; } phase = PH_INIT_WAIT; break;
          case PH_MAIN: {
            #include "group64_nemesis.inc"
            if (gen_live && gen_next <= T && free_mask) {
              // [upstream] jepsen.tests.linearizable-register: one key per group of 2n threads; first n threads read, the
              // rest mix [w cas cas]; values 0..4; (gen/process-limit 20) retires a key after 20 distinct processes
              const u32 nfree = __popcll(free_mask);
              const u32 kk = gen_k++;
              const u64 h = draw64(key, S_GEN, kk);
              const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
              const u32 pick = scale32(r_lo, nfree);
              const bool sel = is_worker && !busy && (u32)__popcll(free_mask & lt_mask) == pick;
              if (TSO) {   // (gen/repeat {:f :generate}), unique_ids.clj:71
                if (sel) { mark = true; kind = K_OP; m_f = MSIM_F_GENERATE; m_value = MSIM_NO_VALUE; }
                gen_next = T + __umulhi(r_hi, p.gen_period2_us);
                break;
              }
              const u64 selm = __ballot(sel);
              const u32 sl = (u32)__builtin_ctzll(selm);                       // the chosen lane
              const u32 s_proc = rdlane(process, sl), s_reg = rdlane(key_reg, sl);
              bool fresh_key = false;
              if (s_reg != s_proc) {  // this process has not used the current key yet
                if (key_procs == 20) {
                  if (cur_key >= 255) { flags |= MSIM_FLAG_VALUES_OVERFLOW; phase = PH_DONE; break; }   // keys travel in 8 bits (oracle: same flag, same stop)
                  cur_key++; key_procs = 0; fresh_key = true;
                }
                key_procs++;
              }
              if (fresh_key) key_reg = INF;
              const u64 h2 = draw64(key, S_GEN2, kk);
              const u32 v1 = scale32((u32)(h2 >> 32), 5), v2 = (((u32)(h2 >> 20) & 0xFFFu) * 5u) >> 12, kx = cur_key & 0xFFu;
              if (sel) {
                key_reg = process;
                mark = true; kind = K_OP;
                if (slot < N) { m_f = MSIM_F_READ; m_value = kx | 0xFFFF00u; }
                else if (scale32((u32)h2, 3) == 0) { m_f = MSIM_F_WRITE; m_value = kx | (v1 << 8) | 0xFF0000u; }
                else { m_f = MSIM_F_CAS; m_value = kx | (v1 << 8) | (v2 << 16); }
              }
              gen_next = T + __umulhi(r_hi, p.gen_period2_us);
            }
          } break;
          default: break;
        }
        if (phase == PH_DONE) break;   // the generator ran out of keys
      }

      // ---- R2: marked clients invoke ----
      u64 inv_mask = __ballot(mark);
      if (inv_mask) {
        u32 rq_dest = 0, rq_type = 0, rq_a = 0;
        if (mark) {
          mark = false; busy = true;
          if (kind == K_INIT) { rq_dest = slot; rq_type = M_INIT; next_msg_id = 0; }
          else {
            c_f = m_f; c_value = m_value;
            rq_dest = dest_node;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (c_f << 2) | (process << 12); inv_value = c_value;
            rq_type = TSO ? (u32)M_GENERATE : c_f == MSIM_F_WRITE ? (u32)M_WRITE : c_f == MSIM_F_CAS ? (u32)M_CAS : (u32)M_READ;
            rq_a = TSO ? 0u : c_value;
          }
          want = ++next_msg_id;
          timeout_at = T + (kind == K_OP ? rpc_timeout_ms : 10000u) * 1000u;
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

      // ---- R3: one input per node (lin_kv_proxy.rb), then one for the service (endpoint order) ----
      bool rep = false; u32 rep_dest = 0, rep_type = 0, rep_a = 0, rep_b = 0;
      u64 jd_mask = 0;
      if (jcap) jd_mask = __ballot(is_server && has_c && deliver_at <= T);
      if (is_server && has_c && deliver_at <= T) {
        const uint4 q = cm; has_c = false;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0x7Fu, qa = q.z;
        if (qsrc >= N && qsrc < SVC) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
        if (is_node) {
          if (qtype == M_INIT) { rep = true; rep_dest = qsrc; rep_type = M_INIT_OK; rep_b = qb; }
          else if (TSO ? qtype == M_GENERATE : (qtype == M_READ || qtype == M_WRITE || qtype == M_CAS)) {  // proxy!, lin_kv_proxy.rb:27-38 / generate -> ts
            const u32 rid = ++node_msgid;
            // engine capacity: the 32 newest callbacks per node (an evicted one is flagged only if its reply still arrives)
            my_cbs[rid % PX_SLOTS] = make_uint2((rid & 0xFFFFFFu) | (qsrc << 24), (qb & 0xFFFFFFu) | 0x80000000u);
            rep = true; rep_dest = SVC; rep_type = TSO ? (u32)M_TS : qtype; rep_a = TSO ? 0u : qa; rep_b = rid;
          } else if (TSO ? qtype == M_TS_OK : (qtype == M_READ_OK || qtype == M_WRITE_OK || qtype == M_CAS_OK || qtype == M_ERROR)) {
            const uint2 c = my_cbs[qb % PX_SLOTS];
            if ((c.y >> 31) && (c.x & 0xFFFFFFu) == qb) {
              my_cbs[qb % PX_SLOTS] = make_uint2(0, 0);
              rep = true; rep_dest = c.x >> 24; rep_type = TSO ? (u32)M_GENERATE_OK : qtype; rep_a = qa; rep_b = c.y & 0x7FFFFFFFu;
            } else if (qb + PX_SLOTS <= node_msgid) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
          }
        } else {  // the service
          u32 rt = 0, ra = 0;
          bool answer = true;
          if (TSO) { if (qtype == M_TS) { rt = M_TS_OK; ra = last_index++; } else answer = false; }   // PersistentTSO, service.clj:116-123 (the lane's `last_index` is the next timestamp)
          else if (p.cfg.proxy_service == MSIM_SVC_LIN_KV) kv_handle(KVS(32u), qtype, qa, rt, ra);
          else if (p.cfg.proxy_service == MSIM_SVC_SEQ_KV) {  // Sequential, service.clj:161-210
            const u32 ci = cidx[qsrc];
            const u32 index = ci + scale32(draw32(key, S_SVC, svc_ctr++), last_index - ci + 1);
            const u32 held = last_index + 1 < 32 ? last_index + 1 : 32;
            if (last_index - index >= held) answer = false;  // state no longer in the ring: exception in the worker, no reply
            else {
              unsigned char *tmp = KVS(33u);  // scratch state
              for (u32 i = 0; i < 64; i++) reinterpret_cast<u32 *>(tmp)[i] = reinterpret_cast<const u32 *>(KVS(index % 32))[i];
              if (!kv_handle(tmp, qtype, qa, rt, ra)) cidx[qsrc] = index;
              else {
                for (u32 i = 0; i < 64; i++) reinterpret_cast<u32 *>(tmp)[i] = reinterpret_cast<const u32 *>(KVS(last_index % 32))[i];
                kv_handle(tmp, qtype, qa, rt, ra);
                last_index++;
                for (u32 i = 0; i < 64; i++) reinterpret_cast<u32 *>(KVS(last_index % 32))[i] = reinterpret_cast<const u32 *>(tmp)[i];
                cidx[qsrc] = last_index;
              }
            }
          } else {  // Eventual over LWWKV, 2 replicas; the merge is computed and discarded (service.clj:222-235)
            svc_ctr += 2;  // merge-source, merge-dest
            const u32 i = scale32(draw32(key, S_SVC, svc_ctr++), 2);
            kv_handle(KVS(32u + i), qtype, qa, rt, ra);
          }
          if (answer) { rep = true; rep_dest = qsrc; rep_type = rt; rep_a = ra; rep_b = qb; }
        }
      }
      n_ev += (u32)__popcll(jd_mask);

      // COMMIT: one message per server endpoint at most; ids in lane order (nodes, then the service)
      {
        const u64 reps0 = __ballot(rep);
        if (reps0) {
          const u32 my_off = (u32)__popcll(reps0 & lt_mask);
          ev_base = n_ev; id_base = next_id; n_ev += (u32)__popcll(reps0);
          if (rep) { if (rep_dest >= N && rep_dest < SVC) s_send_cl++; else s_send_sv++; }
          const u32 rep_pack = rep_dest | (rep_type << 8);
          u64 reps = reps0;
          while (reps) {
            const u32 s = (u32)__builtin_ctzll(reps); reps &= reps - 1;
            const u32 pk = rdlane(rep_pack, s), o = rdlane(my_off, s);
            const u32 r_a = rdlane(rep_a, s), r_b = rdlane(rep_b, s);
            if (lane == (pk & 0xFF)) arrive(next_id + o, pk >> 8, r_a, r_b, s == N + CS ? SVC : s);
          }
          next_id += (u32)__popcll(reps0);
        }
        poll();
      }

      // ---- R4: clients' recv! loops ----
      for (;;) {
        const bool dl = is_client && has_c && deliver_at <= T;
        const u64 dm = __ballot(dl);
        if (!dm) break;
        if (dl) {
          const uint4 q = cm; has_c = false;
          s_recv_cl++;
          const u32 qb = q.w & 0xFFFFFFu, qtype = q.y & 0x7Fu, qa = q.z;
          if (jcap) jwrite(n_ev + (u32)__popcll(dm & lt_mask), 1, q.y, qa, qb, q.w >> 24, lane);
          if (busy && qb == want) {  // else stale (client.clj:105-107)
            if (TSO && qtype == M_GENERATE_OK) complete(MSIM_T_OK, 0, qa);   // unique_ids.clj:53-57
            else if (qtype == M_READ_OK) complete(MSIM_T_OK, 0, (c_value & 0xFFu) | ((qa & 0xFFu) << 8) | 0xFF0000u);   // [k v], lin_kv.clj:56-61
            else if (qtype == M_ERROR) complete(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : MSIM_ERR_PRECONDITION_FAILED, c_value);
            else complete(MSIM_T_OK, 0, c_value);
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
