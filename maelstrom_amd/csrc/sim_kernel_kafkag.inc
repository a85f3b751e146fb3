// sim_kernel_kafkag.inc — the kafka workload (sim_kernel_kafka.inc: demo/clojure/kafka.clj over lin-kv) with SEVERAL WORKERS PER NODE
// (`--concurrency k n`).  Included by sim_kernels.h after sim_kernel_kafka.inc, whose node and service are the same text (kafka_node.inc,
// kafka_blocks.inc, kafka_svc.inc) and whose clients and generator it repeats for a worker's lane, in the lane layout of sim_kernel_dtg.inc /
// txng / mkg / hatg: a lane is an ENDPOINT — nodes 0 .. N-1, client worker slots
// N .. N+CS-1 (a worker's process p talks to node p mod N), lin-kv at N+CS — every endpoint has a queue, clients poll only while an RPC is
// outstanding, COMMIT is receiver-side.  A node has up to KFG_SLOTS request handlers in flight (with one worker per node: KF_SLOTS = 8).
// Specification: oracle/kafka_nodes.inc, bit for bit (tests/test_parity_gpu.py::test_kafka_many_workers_parity, tests/test_hipemu_parity.py).

#define KFG_SLOTS 64u

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64) kafkag_kernel(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const slots = reinterpret_cast<u32 *>(smem + p.off_seen);       // [N][KFG_SLOTS][KSW] request handlers in flight
  u32 *const cache = slots + p.N * KFG_SLOTS * KSW;                     // [N][KF_KEYS] offset-cache (kafka.clj:28-42)
  u32 *const coff = cache + p.N * KF_KEYS;                              // [CS][KF_KEYS] the clients' offsets, in the order of their keys
  u32 *const gen = coff + p.CS * KF_KEYS;                               // active[16], next_val[16], next_key
  u32 *const klen = gen + 36;                                           // [KF_KEYS] lin-kv: messages of every key's log
  u32 *const nupd = klen + KF_KEYS;                                     // [KF_KEYS] entries of the key's committed-offset list
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const u32 SVC = N + CS;  // the service's endpoint (= lane)
  const bool is_node = lane < N, is_client = lane >= N && lane < SVC, is_svc = lane == SVC;
  const bool is_server = is_node || is_svc;
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;   // (masks over key indices only)
  const u64 lt_mask = (1ull << lane) - 1;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
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
  const u32 qidx = is_node ? lane : N;   // queue of a server endpoint (lin-kv: N)
  const u32 my_cap = is_server ? p.cap_node : T_CLIENT_CAP, my_spill_cap = is_server ? p.spill_cap : 0u;
  uint4 *const my_inbox = inbox + (is_server ? qidx * p.cap_node : is_client ? (N + 1) * p.cap_node + slot * T_CLIENT_CAP : 0u);
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)qidx * p.spill_cap;
  u32 *const my_slots = slots + (is_node ? lane : 0) * KFG_SLOTS * KSW;
  u32 *const my_cache = cache + (is_node ? lane : 0) * KF_KEYS;
  u32 *const my_coff = coff + (is_client ? slot : 0) * KF_KEYS;

  for (u32 i = lane; i < N * KFG_SLOTS * KSW + N * KF_KEYS + CS * KF_KEYS; i += 64) slots[i] = 0;
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
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_f = 0, c_value = 0, process = slot, m_f = 0, m_value = 0;
  u32 kc_n = 0, kc_keys = 0, kc_stage = 0, kc_fin = 0, kc_done = 0, kc_ref = 0;   // offsets map: kc_n keys (3 bits each in kc_keys), values in my_coff
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0, sleep_until = 0, final_deadline = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

#define PAYS_LATENCY(src) (((src) < N || (src) == SVC) && is_server)   // neither end is a client (group64_net.inc)
#define ENDPOINT_LANES   // a lane is one endpoint: node, worker slot or service
#define POLL_LANE (is_server || busy)   // the lanes that take from their queue (group64_poll.inc)
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
    const u64 busy_mask = __ballot(busy);
    const u64 pend_mask = __ballot(mark);   // clients between the two RPCs of a poll

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
            if (!__ballot(is_worker && (busy || (!kc_done && T < final_deadline)))) { phase = PH_DONE; again = true; }
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
    const u64 free_mask = worker_mask & ~busy_mask;
    u32 due = INF;
    switch (phase) {
      case PH_INIT: case PH_NEM_FINAL: case PH_FINAL: due = T; break;
      case PH_SLEEP: due = sleep_until; break;
      case PH_KF_FINAL: if (T < final_deadline && __ballot(is_worker && !busy && !kc_done)) due = T; break;
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
        process += C; next_msg_id = 0; in_n = 0;   // (s->inbox[..].n = 0: what waited in the old client's inbox is gone; an envelope already taken is not)
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
              // one operation ([upstream] jepsen.tests.kafka, oracle/kafka_nodes.inc kf_generate): every lane computes it, lane 0 owns the key pool
              const u64 h2 = draw64(key, S_GEN2, kk);
              const u64 pc = (u64)C * 65536ull * 1000ull / (30ull * (u64)rate);
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
            if (n_payload + C * n > max_pay) { flags |= MSIM_FLAG_PAYLOAD_OVERFLOW; phase = PH_DONE; break; }
            if (is_worker) {
              for (u32 i = 0; i < n; i++) g_pay[n_payload + slot * n + i] = i | 0x80000000u;
              mark = true; kind = K_OP; kc_fin = 1; m_f = MSIM_F_ASSIGN; m_value = (n_payload + slot * n) | (n << 24);
            }
            n_payload += C * n;
            final_deadline = T + 10000000u; phase = PH_KF_FINAL;
          } break;
          case PH_KF_FINAL:
            if (is_worker && !busy && !kc_done && T < final_deadline) { mark = true; kind = K_OP; m_f = MSIM_F_POLL; m_value = MSIM_NO_VALUE; }
            break;
          default: break;
        }
        if (phase == PH_DONE) break;
      }

      // ---- R2: marked clients invoke (or send the second RPC of a poll); the request goes to this lane's own node ----
      const u64 inv_mask0 = __ballot(mark);
      if (inv_mask0) {
        // poll requests carry the client's {key offset} map: payload words in slot order
        const bool is_poll = mark && kind == K_OP && kc_stage != 2 && m_f == MSIM_F_POLL;
        const u32 pw = is_poll ? kc_n : 0u;
        const u32 pincl = wave_incl_scan(pw), ptotal = rdlane(pincl, 63);
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
        u64 inv_mask = __ballot(send_rpc);
        if (inv_mask) { ev_base = n_ev; id_base = next_id; n_ev += (u32)__popcll(inv_mask); }
        u32 rq_pack = 0;
        if (send_rpc) {
          want = ++next_msg_id;
          timeout_at = T + (kind == K_OP ? p.cfg.client_timeout_ms : 10000u) * 1000u;
          s_send_cl++;
          rq_pack = (kind == K_INIT ? slot : process % N) | (rq_type << 8);   // (dest = process mod N, kafka_nodes.inc / [upstream] interpreter)
        }
        while (inv_mask) {   // every node takes its workers' requests in, in slot order
          const u32 s = (u32)__builtin_ctzll(inv_mask); inv_mask &= inv_mask - 1;
          const u32 pk = rdlane(rq_pack, s);
          const u32 a = rdlane(rq_a, s), b = rdlane(want, s);
          if (lane == (pk & 0xFF)) arrive(next_id, pk >> 8, a, b, s);
          next_id++;
        }
        poll();
      }

      // ---- R3: one input per node, then one for the service (endpoint order) ----
      bool to_svc = false, rep = false, svc_rep = false;   // node -> service, node -> a client (rep_dest), service -> node
      u32 rep_dest = 0;
      u32 o_type = 0, o_a = 0, o_b = 0, o_dest = 0, need_words = 0, done_slot = 0;
      const u64 jd_mask = jcap ? __ballot(is_server && deliver_at <= T) : 0ull;
      const bool svc_due = is_svc && deliver_at <= T;
      if (is_node && deliver_at <= T) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        if (qsrc >= N && qsrc < SVC) s_recv_cl++; else s_recv_sv++;
        if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
#define KF_NSLOTS KFG_SLOTS
#define REPLY_TO(cmsg) { rep = true; rep_dest = (cmsg) >> 24; o_b = (cmsg) & 0xFFFFFFu; }
#define CLIENT_REF(qb, qsrc) ((qb) | ((qsrc) << 24))   // a client is an endpoint: it rides in the top byte of the stored msg_id
        #include "kafka_node.inc"
      }
      // poll_ok / list_committed_offsets_ok blocks: payload words allocated in node order, each node writes its own
      {
        const u32 incl = wave_incl_scan(need_words);
        const u32 total = rdlane(incl, 63);
        #include "kafka_blocks.inc"
      }
      __syncthreads();   // the service reads the handlers' tables (LDS) after the nodes have written them
      // the lin-kv service (service.clj:31-61 over the chunk keys and "offsets"): one request per round, after the nodes
      if (is_svc && svc_due) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
        s_recv_sv++;
        if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, SVC);
        #include "kafka_svc.inc"
      }
      __syncthreads();
      n_ev += (u32)__popcll(jd_mask);

      // COMMIT: ids in lane order (nodes, then the service); every receiver takes its own in
      {
        const u32 cnt = (to_svc || rep || svc_rep) ? 1u : 0u;
        const u64 smask = __ballot(cnt != 0);
        if (smask) {
          const u32 my_off = (u32)__popcll(smask & lt_mask);
          ev_base = n_ev; id_base = next_id; n_ev += (u32)__popcll(smask);
          if (rep) s_send_cl++; else if (cnt) s_send_sv++;
          u64 ts = __ballot(to_svc);
          while (ts) {
            const u32 s = (u32)__builtin_ctzll(ts); ts &= ts - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), off = rdlane(my_off, s);
            if (is_svc) arrive(next_id + off, ty, a, b, s);
          }
          if (__ballot(svc_rep)) {
            const u32 ty = rdlane(o_type, SVC), a = rdlane(o_a, SVC), b = rdlane(o_b, SVC), d = rdlane(o_dest, SVC), off = rdlane(my_off, SVC);
            if (lane == d) arrive(next_id + off, ty, a, b, SVC);
          }
          // node -> the client it answers: no latency; lost like any other message (net.clj:214)
          u64 rp = __ballot(rep);
          while (rp) {
            const u32 s = (u32)__builtin_ctzll(rp); rp &= rp - 1;
            const u32 ty = rdlane(o_type, s), a = rdlane(o_a, s), b = rdlane(o_b, s), d = rdlane(rep_dest, s), off = rdlane(my_off, s);
            if (lane == d) arrive(next_id + off, ty, a, b, s);
          }
          next_id += (u32)__popcll(smask);
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

    // ---- history rows: the nemesis' rows and the invocations, then the completions — two passes, because a round of the final phase has up
    //      to C rows of each (every worker's assign / poll and, answered at once, its completion) and the staging ring holds 128 ----
    {
      const u64 imask = __ballot(inv_row), cmask = __ballot(cmp_row);
      const u32 ni = (u32)__popcll(imask), nc = (u32)__popcll(cmask);
      if (nem_rows + ni + nc) {
        if (n_rows + nem_rows + ni + nc > max_rows) { flags |= MSIM_FLAG_ROWS_OVERFLOW; break; }
        const u32 tlo = (u32)((u64)T * 1000ull), thi = (u32)(((u64)T * 1000ull) >> 32);
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
          const u32 nr = pass == 0 ? nem_rows + ni : nc;
          if (!nr) continue;
          if (pass == 0) {
            if (NEM && nem_rows && lane == 0) {
              const u32 pk = MSIM_T_INFO | (nem_f << 2) | (MSIM_PROCESS_NEMESIS << 12);
              stage[n_rows % STAGE_ROWS] = make_uint4(tlo, thi, pk, nem_v1);
              stage[(n_rows + 1) % STAGE_ROWS] = make_uint4(tlo, thi | (nem_len2 << 16), pk, nem_v2);
            }
            if (inv_row) stage[(n_rows + nem_rows + (u32)__popcll(imask & lt_mask)) % STAGE_ROWS] = make_uint4(tlo, thi | (inv_len << 16), inv_packed, inv_value);
          } else if (cmp_row) stage[(n_rows + (u32)__popcll(cmask & lt_mask)) % STAGE_ROWS] = make_uint4(tlo, thi | (cmp_len << 16), cmp_packed, cmp_value);
          const u32 new_n = n_rows + nr;
          if ((new_n >> 6) != (n_rows >> 6)) {
            __syncthreads();
            for (u32 blk = n_rows >> 6; blk < (new_n >> 6); blk++) {
              const u32 gi = blk * 64 + lane;
              if (gi < max_rows) reinterpret_cast<uint4 *>(g_rows)[gi] = stage[gi % STAGE_ROWS];
            }
            __syncthreads();
          }
          n_rows = new_n;
        }
      }
    }
  }

  #include "group64_stats.inc"
}
#include "group64_end.inc"
