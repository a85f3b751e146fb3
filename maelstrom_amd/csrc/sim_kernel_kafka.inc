// sim_kernel_kafka.inc — the kafka workload (SURVEY.md §8f rank 4).  Included by engine.hip after sim_kernel_txn.inc (whose
// T_CLIENT_CAP it shares).
//
//   node      demo/clojure/kafka.clj:1-172 over demo/clojure/node.clj:110-195: logs in 32-message chunks under lin-kv keys (send = read
//             the chunk of the cached offset, cas it one message longer; poll = read the chunk of every requested offset, one after
//             the other), committed offsets under the lin-kv key "offsets" (read, cas to the element-wise maximum)
//   service   lin-kv: service.clj:31-61 (PersistentKV read / cas), :141-155, :245-263
//   client    workload/kafka.clj:155-245: send / poll (+ commit_offsets when something was polled) / assign (list_committed_offsets
//             unless :seek-to-beginning?) / crash; not Reusable
//   generator [upstream] jepsen.tests.kafka as workload/kafka.clj:288-311 configures it, restated (parity unpinned)
//
// The specification is oracle/kafka_nodes.inc, statement by statement; this file is the same text for a wavefront.
// Lanes: lane i < N = node i + its client (one worker per node); lane N = lin-kv (endpoint 2N).  A chunk's value is its element
// count, the "offsets" map its version (value-changing commits so far) + per key the (version, offset) pairs that changed it; the
// logs and those pairs live in HBM scratch, everything else in LDS / registers.

#define KF_SLOTS 8u
#define KF_KEYS 8u
#define KF_CHUNK 32u
#define KF_ABSENT 0xFFFFu
#define KF_OFFSETS_KEY 0x80000000u
#define KF_SEND_NONE (0x7FFu << 17)
#define KSW 8u   // words per request handler: client msg_id, request block, rpc msg_id, flags, from | msg << 16, offset, chunk counts x 8
enum { M_SEND = 30, M_SEND_OK, M_POLL, M_POLL_OK, M_LIST_OFFSETS, M_LIST_OFFSETS_OK, M_COMMIT_OFFSETS, M_COMMIT_OFFSETS_OK };
enum { KK_SEND = 1, KK_POLL = 2, KK_LIST = 3, KK_COMMIT = 4 };
enum { PH_KF_FINAL = PH_DONE + 1 };
// flags word of a handler: used | kind << 1 | stage << 4 | key << 6 | j << 9 | nk << 13
#define KS_USED(w_) ((w_) & 1u)
#define KS_KIND(w_) (((w_) >> 1) & 7u)
#define KS_STAGE(w_) (((w_) >> 4) & 3u)
#define KS_KEY(w_) (((w_) >> 6) & 7u)
#define KS_J(w_) (((w_) >> 9) & 15u)
#define KS_NK(w_) (((w_) >> 13) & 0xFFu)
#define KS_MAKE(kind_, stage_, key_, j_, nk_) (1u | ((kind_) << 1) | ((stage_) << 4) | ((key_) << 6) | ((j_) << 9) | ((nk_) << 13))

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) kafka_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const slots = reinterpret_cast<u32 *>(smem + p.off_seen);       // [N][KF_SLOTS][KSW] request handlers in flight
  u32 *const cache = slots + p.N * KF_SLOTS * KSW;                      // [N][KF_KEYS] offset-cache (kafka.clj:28-42)
  u32 *const coff = cache + p.N * KF_KEYS;                              // [N][KF_KEYS] the clients' offsets, in the order of their keys
  u32 *const gen = coff + p.N * KF_KEYS;                                // active[16], next_val[16], next_key
  u32 *const klen = gen + 36;                                           // [KF_KEYS] lin-kv: messages of every key's log
  u32 *const nupd = klen + KF_KEYS;                                     // [KF_KEYS] entries of the key's committed-offset list
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N;
  const bool is_node = lane < N, is_svc = lane == N;
  const u32 SVC = 2 * N;  // the service's endpoint index
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u32 all_nodes = (1u << N) - 1;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz, mw = p.cfg.max_writes_per_key, cap = mw + 1u;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_log = g_scr;                                           // [KF_KEYS][cap] the messages
  u32 *const g_upd = g_scr + (size_t)KF_KEYS * cap;                    // [KF_KEYS][cap + 1] version << 16 | committed offset
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = p.cap_node, my_spill_cap = p.spill_cap;
  const u32 qlane = lane <= N ? lane : 0;
  uint4 *const my_inbox = inbox + qlane * my_cap;                                     // node / service queue
  uint4 *const my_cinbox = inbox + (N + 1) * my_cap + (is_node ? lane : 0) * T_CLIENT_CAP;
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qlane * my_spill_cap;
  u32 *const my_slots = slots + (is_node ? lane : 0) * KF_SLOTS * KSW;
  u32 *const my_cache = cache + (is_node ? lane : 0) * KF_KEYS;
  u32 *const my_coff = coff + (is_node ? lane : 0) * KF_KEYS;
  const u32 my_client = N + lane;

  for (u32 i = lane; i < N * KF_SLOTS * KSW + 2 * N * KF_KEYS; i += 64) slots[i] = 0;
  if (lane < 16) { gen[lane] = lane; gen[16 + lane] = 1; }
  if (lane == 0) gen[32] = p.cfg.key_count;
  if (lane < KF_KEYS) { klen[lane] = 0; nupd[lane] = 0; }
  __syncthreads();

  // ---- node / service state ----
  u32 deliver_at = INF; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, node_msgid = 0, part = 0;
  u32 off_exists = 0, off_ver = 0;   // lin-kv lane: the key "offsets"
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_f = 0, c_value = 0, process = lane, m_f = 0, m_value = 0, cin_n = 0;
  u32 kc_n = 0, kc_keys = 0, kc_stage = 0, kc_fin = 0, kc_done = 0, kc_ref = 0;   // offsets map: kc_n keys (3 bits each in kc_keys), values in my_coff
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0, sleep_until = 0, final_deadline = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

#define PAYS_LATENCY(src) ((src) < N || (src) == SVC)   // neither end is a client (group64_net.inc)
#define POLL_LANE (lane <= N)   // the lanes that take from their queue (group64_poll.inc)
  #include "group64_net.inc"
  #include "group64_poll.inc"
  // lin-kv: elements of chunk `ch` of key `k` (0: the lin-kv key does not exist)
  auto chunk_count = [&](u32 k, u32 ch) -> u32 {
    const u32 lo = ch * KF_CHUNK, len = klen[k];
    return len <= lo ? 0u : min(len - lo, KF_CHUNK);
  };
  // committed offset of key `k` in the "offsets" map at version `ver`: 1 + offset, 0 = no entry
  // (the list grows by one entry per commit that moves the key, versions ascending: the newest entry answers every commit — which asks at
  //  the current version — with one load, a reader of an older version bisects; walking the list was hundreds of dependent HBM round
  //  trips on the service's lane for every acknowledged poll late in a run)
  auto committed_at = [&](u32 k, u32 ver) -> u32 {
    const u32 n = nupd[k];
    if (!n) return 0u;
    const u32 *const u = g_upd + (size_t)k * (cap + 1);
    const u32 last = u[n - 1u];
    if ((last >> 16) <= ver) return 1u + (last & 0xFFFFu);
    u32 a = 0, b = n - 1u;   // u[b] is newer than ver; a = entries known to be at or below it
    while (a < b) { const u32 mid = (a + b) >> 1; if ((u[mid] >> 16) <= ver) a = mid + 1u; else b = mid; }
    return a ? 1u + (u[a - 1u] & 0xFFFFu) : 0u;
  };

  for (;;) {
    const u32 busy_mask = (u32)__ballot(busy);
    const u32 pend_mask = (u32)__ballot(mark);   // clients between the two RPCs of a poll

    // ---- time-free phase transitions ----
    if (!(phase == PH_MAIN && ((rate > 0 && gen_next < cutoff) || (NEM && nem_next < cutoff)))) {
      for (bool again = true; again;) {
        again = false;
        switch (phase) {
          case PH_INIT_WAIT: if (!busy_mask) { phase = PH_MAIN_START; again = true; } break;
          case PH_MAIN_START:
            cutoff = T + p.cfg.time_limit_ms * 1000u; gen_next = T; nem_next = T;
            next_msg_id = 0; loss_on = 1; phase = PH_MAIN; again = true; break;
          case PH_MAIN: {
            const bool gl = rate > 0 && gen_next < cutoff, nl = NEM && nem_next < cutoff;
            if (gl || nl) break;
            if (rate == 0 && T < cutoff) break;
            phase = PH_DRAIN; again = true;
          } break;
          case PH_DRAIN:
            if (busy_mask) break;
            phase = NEM ? PH_NEM_FINAL : PH_SLEEP;
            if (phase == PH_SLEEP) sleep_until = T + p.cfg.quiesce_ms * 1000u;
            again = true; break;
          case PH_KF_FINAL:   // every worker has polled until nothing came (or the 10 s of workload/kafka.clj:305-306 are over)
            if (!__ballot(is_node && (busy || (!kc_done && T < final_deadline)))) { phase = PH_DONE; again = true; }
            break;
          default: break;
        }
      }
      if (phase == PH_DONE) break;
    }
    if (++rounds > ROUND_LIMIT) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }

    // ---- R0: time ----
    const bool gen_live = rate > 0 && gen_next < cutoff;
    const bool nem_live = NEM && nem_next < cutoff;
    const u32 free_mask = all_nodes & ~busy_mask;
    u32 due = INF;
    switch (phase) {
      case PH_INIT: case PH_NEM_FINAL: case PH_FINAL: due = T; break;
      case PH_SLEEP: due = sleep_until; break;
      case PH_KF_FINAL: if (T < final_deadline && __ballot(is_node && !busy && !kc_done)) due = T; break;
      case PH_MAIN:
        if (nem_live) due = max(nem_next, T);
        if (gen_live && free_mask) due = min(due, max(gen_next, T));
        if (rate == 0 && !nem_live) due = min(due, cutoff);
        break;
      default: break;
    }
    bool timeout_round = false;
    if (due > T && !pend_mask && !__ballot(deliver_at <= T)) {
      u32 k = deliver_at == INF ? INF : deliver_at * 2;
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

    auto complete = [&](u32 type, u32 err, u32 value, u32 len) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (c_f << 2) | (err << 7) | (process << 12);
      cmp_value = value; cmp_len = len;
      if (type == MSIM_T_INFO) {   // crashed process: a new process id and a fresh client (not Reusable, workload/kafka.clj:239-243)
        process += N; next_msg_id = 0; cin_n = 0;
        kc_n = 0; kc_stage = 0;
      }
    };
    // what the op's :fail / :info carries: the value it was invoked with
    auto abort_op = [&](u32 type, u32 err) {
      kc_stage = 0;
      if (c_f == MSIM_F_SEND) complete(type, err, c_value | KF_SEND_NONE, 0);
      else if (c_value == MSIM_NO_VALUE) complete(type, err, MSIM_NO_VALUE, 0);
      else complete(type, err, c_value & 0xFFFFFFu, c_value >> 24);
    };
    // the client's recv! consumes one envelope (client.clj:94-107)
    auto client_deliver = [&](u32 qtype, u32 qa, u32 qb) {
      s_recv_cl++;
      if (!(busy && qb == want)) return;
      if (kind != K_OP) { complete(MSIM_T_OK, 0, c_value, 0); return; }   // init_ok
      switch (qtype) {
        case M_SEND_OK: kc_stage = 0; complete(MSIM_T_OK, 0, c_value | (qa << 17), 0); break;
        case M_POLL_OK: {
          u32 pp = qa & 0xFFFFFFu; const u32 end = pp + (qa >> 24); bool any = false;
          while (pp < end) {   // advance the local offsets to max polled + 1, :181-186
            const u32 h = g_pay[pp], k = h & 7u, n = (h >> 8) & 0xFFu, o = h >> 16;
            pp += 1u + (n + 1u) / 2u;
            if (!n) continue;
            any = true;
            for (u32 j = 0; j < kc_n; j++) if (((kc_keys >> (3u * j)) & 7u) == k && o + n > my_coff[j]) my_coff[j] = o + n;
          }
          if (kc_fin) kc_done = any ? 0u : 1u;
          if (any) { kc_stage = 2; kc_ref = qa; mark = true; }   // (when (seq offsets) (commit_offsets! ...)): the next RPC of this op
          else { kc_stage = 0; complete(MSIM_T_OK, 0, (qa >> 24) ? (qa & 0xFFFFFFu) : MSIM_NO_VALUE, qa >> 24); }
        } break;
        case M_COMMIT_OFFSETS_OK: kc_stage = 0; complete(MSIM_T_OK, 0, kc_ref & 0xFFFFFFu, kc_ref >> 24); break;
        case M_LIST_OFFSETS_OK: {   // offsets := {k (or (offsets k) (committed k) 0)} over the op's keys, in their order, :211-219
          const u32 ref = qa & 0xFFFFFFu, n = qa >> 24;
          u32 nkeys = 0, no[KF_KEYS];
#pragma unroll
          for (u32 j = 0; j < KF_KEYS; j++) {
            no[j] = 0;
            if (j < n) {
              const u32 w = g_pay[ref + j], k = w & 7u; u32 o = (w >> 31) ? ((w >> 8) & 0x7FFFFFu) : 0u;
              for (u32 e = 0; e < kc_n; e++) if (((kc_keys >> (3u * e)) & 7u) == k) o = my_coff[e];
              nkeys |= k << (3u * j); no[j] = o;
            }
          }
#pragma unroll
          for (u32 j = 0; j < KF_KEYS; j++) if (j < n) my_coff[j] = no[j];
          kc_n = n; kc_keys = nkeys;
          kc_stage = 0; complete(MSIM_T_OK, 0, c_value & 0xFFFFFFu, c_value >> 24);
        } break;
        case M_ERROR:
          abort_op(MSIM_T_FAIL, qa == 11 ? MSIM_ERR_TEMPORARILY_UNAVAILABLE : qa == 20 ? MSIM_ERR_KEY_DOES_NOT_EXIST : qa == 30 ? MSIM_ERR_TXN_CONFLICT : MSIM_ERR_PRECONDITION_FAILED);
          break;
        default: break;
      }
    };

    if (timeout_round) {
      if (busy && timeout_at <= T) {
        if (kind != K_OP) complete(MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_value, 0);
        else abort_op(c_f == MSIM_F_ASSIGN ? MSIM_T_FAIL : MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT);   // (c/with-errors op #{:assign} ..), :205
      }
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
              // one operation ([upstream] jepsen.tests.kafka, oracle/kafka_nodes.inc kf_generate): every lane computes it, lane 0 owns the key pool
              const u64 h2 = draw64(key, S_GEN2, kk);
              const u64 pc = (u64)N * 65536ull * 1000ull / (30ull * (u64)rate);
              u32 f = 0, val = MSIM_NO_VALUE, bad = 0;
              if (((h2 >> 48) & 0xFFFFu) < pc) f = MSIM_F_CRASH;
              else if (((h2 >> 44) & 0xFu) < 2) {   // an :assign of a non-empty subset of the keys seen so far, in key order
                const u32 nk = gen[32];
                u32 m = (u32)(h2 >> 8) & ((1u << nk) - 1u);
                if (!m) m = 1u << (((u32)h2 >> 4) % nk);
                const u32 n = (u32)__popc(m);
                if (n_payload + n > max_pay) bad = MSIM_FLAG_PAYLOAD_OVERFLOW;
                else {
                  if (lane < nk && ((m >> lane) & 1)) g_pay[n_payload + __popc(m & lt32)] = lane;
                  f = MSIM_F_ASSIGN; val = n_payload | (n << 24); n_payload += n;
                }
              } else if (!((h2 >> 43) & 1)) f = MSIM_F_POLL;
              else {
                const u32 kc = p.cfg.key_count;
                const u64 h3 = draw64(key, S_GEN3, (u64)kk * 8);
                const u32 x = scale32((u32)(h3 >> 32), (1u << kc) - 1) + 1;
                const u32 ki = 31 - (u32)__clz((int)x);
                const u32 k = gen[ki], v = gen[16 + ki], nk = gen[32];
                __syncthreads();
                if (v + 1 > mw && nk >= KF_KEYS) bad = MSIM_FLAG_VALUES_OVERFLOW;
                else if (lane == 0) {
                  gen[16 + ki] = v + 1;
                  if (v + 1 > mw) { gen[ki] = nk; gen[32] = nk + 1; gen[16 + ki] = 1; }   // key used up: a fresh one takes its place in the pool
                }
                __syncthreads();
                f = MSIM_F_SEND; val = k | (v << 6);
              }
              if (bad) { flags |= bad; phase = PH_DONE; break; }
              if (sel) { mark = true; kind = K_OP; m_f = f; m_value = val; }
              gen_next = T + __umulhi(r_hi, p.gen_period2_us);
            }
          } break;
          case PH_NEM_FINAL:
            part = 0; nem_rows = 2; nem_f = MSIM_F_STOP_PARTITION; nem_v1 = MSIM_NO_VALUE; nem_v2 = MSIM_NO_VALUE; nem_len2 = 0;
            phase = PH_SLEEP; sleep_until = T + p.cfg.quiesce_ms * 1000u; break;
          case PH_SLEEP:
            if (T < sleep_until) break;
            phase = PH_FINAL;
            // fallthrough
          case PH_FINAL: {   // [upstream] the final generator: every worker assigns all keys from the beginning (then polls, PH_KF_FINAL)
            const u32 n = gen[32];
            if (n_payload + N * n > max_pay) { flags |= MSIM_FLAG_PAYLOAD_OVERFLOW; phase = PH_DONE; break; }
            if (is_node) {
              for (u32 i = 0; i < n; i++) g_pay[n_payload + lane * n + i] = i | 0x80000000u;
              mark = true; kind = K_OP; kc_fin = 1; m_f = MSIM_F_ASSIGN; m_value = (n_payload + lane * n) | (n << 24);
            }
            n_payload += N * n;
            final_deadline = T + 10000000u; phase = PH_KF_FINAL;
          } break;
          case PH_KF_FINAL:
            if (is_node && !busy && !kc_done && T < final_deadline) { mark = true; kind = K_OP; m_f = MSIM_F_POLL; m_value = MSIM_NO_VALUE; }
            break;
          default: break;
        }
        if (phase == PH_DONE) break;
      }

      // ---- R2: marked clients invoke (or send the second RPC of a poll); the request goes to this lane's own node ----
      const u32 inv_mask0 = (u32)__ballot(mark);
      if (inv_mask0) {
        // poll requests carry the client's {key offset} map: payload words in slot order
        const bool is_poll = mark && kind == K_OP && kc_stage != 2 && m_f == MSIM_F_POLL;
        const u32 pw = is_poll ? kc_n : 0u;
        const u32 pincl = scan32(pw), ptotal = rdlane(pincl, 31);
        bool pay_ok = true;
        if (ptotal) { if (n_payload + ptotal > max_pay) { flags |= MSIM_FLAG_PAYLOAD_OVERFLOW; pay_ok = false; } }
        bool send_rpc = false; u32 rq_type = 0, rq_a = 0;
        if (mark) {
          mark = false; busy = true; send_rpc = true;
          if (kind == K_INIT) { rq_type = M_INIT; next_msg_id = 0; }
          else if (kc_stage == 2) { rq_type = M_COMMIT_OFFSETS; rq_a = kc_ref; }   // :223-230
          else {
            c_f = m_f; c_value = m_value;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (c_f << 2) | (process << 12);
            if (c_f == MSIM_F_SEND) { inv_value = c_value | KF_SEND_NONE; inv_len = 0; rq_type = M_SEND; rq_a = c_value; kc_stage = 1; }
            else if (c_f == MSIM_F_POLL) {
              const u32 off = pay_ok ? n_payload + pincl - pw : 0u;
              if (pay_ok) for (u32 j = 0; j < kc_n; j++) g_pay[off + j] = ((kc_keys >> (3u * j)) & 7u) | (my_coff[j] << 8);
              c_value = kc_n ? (off | (kc_n << 24)) : MSIM_NO_VALUE;
              inv_value = kc_n ? off : MSIM_NO_VALUE; inv_len = kc_n;
              rq_type = M_POLL; rq_a = kc_n ? c_value : 0u; kc_stage = 1;
            } else if (c_f == MSIM_F_ASSIGN) {
              const u32 ref = c_value & 0xFFFFFFu, n = c_value >> 24;
              inv_value = ref; inv_len = n;
              if (g_pay[ref] >> 31) {   // (reset! offsets (zipmap value (repeat 0))), :207-209
                u32 nkeys = 0;
                for (u32 j = 0; j < n; j++) { nkeys |= (g_pay[ref + j] & 7u) << (3u * j); my_coff[j] = 0; }
                kc_n = n; kc_keys = nkeys;
                send_rpc = false; complete(MSIM_T_OK, 0, ref, n);
              } else { rq_type = M_LIST_OFFSETS; rq_a = c_value; kc_stage = 1; }
            } else {   // :crash, :222
              inv_value = MSIM_NO_VALUE; inv_len = 0;
              send_rpc = false; complete(MSIM_T_INFO, 0, MSIM_NO_VALUE, 0);
            }
          }
        }
        if (pay_ok) n_payload += ptotal;
        const u32 inv_mask = (u32)__ballot(send_rpc);
        if (inv_mask) { ev_base = n_ev; id_base = next_id; n_ev += __popc(inv_mask); }
        if (send_rpc) {
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
      u32 o_type = 0, o_a = 0, o_b = 0, o_dest = 0, need_words = 0, done_slot = 0;
      const u32 jd_mask = jcap ? (u32)__ballot(lane <= N && deliver_at <= T) : 0u;
      const bool svc_due = is_svc && deliver_at <= T;
      if (is_node && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < SVC) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, lane);
#define KF_NSLOTS KF_SLOTS
#define REPLY_TO(cmsg) { rep = true; o_b = (cmsg); }   // (the client lives in the node's lane)
#define CLIENT_REF(qb, qsrc) (qb)
        #include "kafka_node.inc"
      }
      // poll_ok / list_committed_offsets_ok blocks: payload words allocated in node order, each node writes its own
      {
        const u32 incl = scan32(need_words);
        const u32 total = rdlane(incl, 31);
        #include "kafka_blocks.inc"
      }
      __syncthreads();   // the service reads the handlers' tables (LDS) after the nodes have written them
      // the lin-kv service (service.clj:31-61 over the chunk keys and "offsets"): one request per round, after the nodes
      if (is_svc && svc_due) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        s_recv_sv++;
        if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, SVC);
        #include "kafka_svc.inc"
      }
      __syncthreads();
      n_ev += __popc(jd_mask);

      // COMMIT: ids in lane order (nodes, then the service)
      bool c_arr = false; u32 ca_y = 0, ca_a = 0, ca_b = 0;
      {
        const u32 cnt = (to_svc || rep || svc_rep) ? 1u : 0u;
        const u32 smask = (u32)__ballot(cnt != 0);
        if (smask) {
          const u32 my_off = __popc(smask & lt32);
          ev_base = n_ev; id_base = next_id; n_ev += __popc(smask);
          if (rep) s_send_cl++; else if (cnt) s_send_sv++;
          u32 ts = (u32)__ballot(to_svc);
          while (ts) {
            const u32 s = (u32)__builtin_ctz(ts); ts &= ts - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), off = rdlane(my_off, s);
            if (is_svc) arrive(next_id + off, ty, a, b, s, SVC);
          }
          const u32 sv = (u32)__ballot(svc_rep);
          if (sv) {
            const u32 ty = rdlane(o_type, N), a = rdlane(o_a, N), b = rdlane(o_b, N), d = rdlane(o_dest, N), off = rdlane(my_off, N);
            if (lane == d) arrive(next_id + off, ty, a, b, SVC, d);
          }
          if (rep) {
            const u32 id = next_id + my_off;
            if (jcap) jwrite(ev_base + my_off, 0, (id << 8) | o_type, o_a, o_b, lane, my_client);
            if (!(NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss)) { c_arr = true; ca_y = (id << 8) | o_type; ca_a = o_a; ca_b = o_b; }
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
          if (cin_n >= 8u) my_flags |= MSIM_FLAG_INBOX_OVERFLOW;
          else my_cinbox[cin_n++] = make_uint4(T, ca_y, ca_a, ca_b | (lane << 24));
        }
      }
    }

    #include "group64_rows.inc"
  }

  #include "group64_stats.inc"
}
#include "group64_end.inc"
