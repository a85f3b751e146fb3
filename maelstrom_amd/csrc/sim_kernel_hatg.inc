// sim_kernel_hatg.inc — txn-rw-register over the highly-available-transactions node (sim_kernel_hat.inc: demo/clojure/txn_rw_register_hat.clj)
// with SEVERAL WORKERS PER NODE (`--concurrency k n`).  Included by sim_kernels.h after sim_kernel_hat.inc, whose node is the same
// text, hat_node.inc (a transaction is applied and answered in the round it arrives: nothing is in flight per node), in the lane layout of
// sim_kernel_dtg.inc / txng / mkg: a lane is an ENDPOINT — nodes 0 .. N-1, client worker slots N .. N+CS-1 (worker t talks to node t mod N) —
// every endpoint has a queue, clients poll only while an RPC is outstanding, COMMIT is receiver-side.
// Specification: oracle/hat_nodes.inc, bit for bit (tests/test_parity_gpu.py::test_rw_register_many_workers_parity, tests/test_hipemu_parity.py).

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) hatg_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const gen = reinterpret_cast<u32 *>(smem + p.off_seen);  // active[16], next_val[16], next_key
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const bool is_node = lane < N, is_client = lane >= N && lane < N + CS;
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u64 lt_mask = (1ull << lane) - 1;
  const u32 all_nodes = (1u << N) - 1;
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
  const u32 my_cap = is_node ? p.cap_node : T_CLIENT_CAP, my_spill_cap = is_node ? p.spill_cap : 0u;
  const u32 qlane = is_node ? lane : 0;
  uint4 *const my_inbox = inbox + (is_node ? lane * p.cap_node : is_client ? N * p.cap_node + slot * T_CLIENT_CAP : 0u);
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qlane * p.spill_cap;

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
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_value = 0, process = slot, m_value = 0;
  const u32 dest_node = is_client ? slot % N : 0u;     // worker t -> node t mod N; a crashed process's successor (process + C) keeps it, C being a multiple of N
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0, n_txn = 0, n_area = 0;

#define PAYS_LATENCY(src) ((src) < N && is_node)   // neither end is a client (group64_net.inc)
#define ENDPOINT_LANES   // a lane is one endpoint: node, worker slot or service
  #include "group64_net.inc"
  auto poll = [&]() {
    const bool elig = is_node || busy;   // clients are in recv! only while an RPC is outstanding (client.clj:94-95)
    if (have_pm) {
      have_pm = false;
      if (elig && deliver_at == INF && (in_n | sp_n) == 0) try_commit(pm);
      else lds_push(pm);
    }
    while (elig && deliver_at == INF && (in_n | sp_n) != 0) {
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
    bool timeout_round = false;   // group64_jump.inc with the node's replicate timer as a second event of the lane (sim_kernel_hat.inc merges it into my_t; here that is other device code)
    if (due > T && !__ballot(my_t <= T || timer_next <= T)) {
      u32 k = min(my_t, timer_next); k = k == INF ? INF : k * 2;
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

      // ---- R3: one input per node: a due replication tick, else the due message ----
      bool rep = false; u32 dmask = 0, rep_dest = 0;  // reply to a client (rep_dest) / node -> node sends (same type, a, b to every dest in dmask)
      u32 o_type = 0, o_a = 0, o_b = 0;
#define REPLY_TO(cmsg) { rep = true; rep_dest = (cmsg) >> 24; o_b = (cmsg) & 0xFFFFFFu; }
#define CLIENT_REF(qb, qsrc) ((qb) | ((qsrc) << 24))   // a client is an endpoint: it rides in the top byte of the stored msg_id
      #include "hat_node.inc"

      // COMMIT: ids in node order, then destination order; every receiver takes its own in
      {
        const u32 cnt = rep ? 1u : (u32)__popc(dmask);
        const u32 smask = (u32)__ballot(cnt != 0);
        if (smask) {
          const u32 incl = scan32(cnt), my_off = incl - cnt, total = rdlane(incl, 31);   // (only nodes send here: lanes below 8)
          ev_base = n_ev; id_base = next_id; n_ev += total;
          if (rep) s_send_cl++; else s_send_sv += cnt;
          u32 ns = (u32)__ballot(dmask != 0);
          while (ns) {  // node -> node: every receiver takes its envelope from each sender, in sender order
            const u32 s = (u32)__builtin_ctz(ns); ns &= ns - 1;
            const u32 dm = rdlane(dmask, s), ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), off = rdlane(my_off, s);
            if (is_node && ((dm >> lane) & 1u)) arrive(next_id + off + __popc(dm & lt32), ty, a, b, s);
          }
          // node -> the client it answers: no latency; lost like any other message (net.clj:214)
          u32 rp = (u32)__ballot(rep);
          while (rp) {
            const u32 s = (u32)__builtin_ctz(rp); rp &= rp - 1;
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
          const uint4 e = cm; deliver_at = INF;
          if (jcap) jwrite(n_ev + (u32)__popcll(dm & lt_mask), 1, e.y, e.z, e.w & 0xFFFFFFu, e.w >> 24, lane);
          client_deliver(e.y & 0xFFu, e.z, e.w & 0xFFFFFFu);   // (a reply nobody awaits any more is skipped: stale)
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
