// sim_kernel_general.inc - the general layout of the simulation kernel (lane = endpoint; any concurrency): the kernel every other
// layout of this directory is a specialisation of.  Included by sim_kernels.h; instantiated by k_general_*.hip.
// =====================================================================================================
// The simulation kernel: one wavefront = one cluster.  PROG = node program (MSIM_NODE_*), NEM = the
// partition nemesis is compiled in, NET_RANDOM = latency is drawn per message and/or messages can be lost
// (false: constant latency, no loss — no per-message RNG in the hot path).  Follows DESIGN.md §2 step by step; the CPU oracle implements the
// same text independently.
//
// One round (DESIGN.md §2.2):
//   R0 pick the time: stay at T while anything is due, else jump to the next event (DPP min)
//   R1 scheduler (generator interpreter, nemesis) — wave-uniform, scalar
//   R2 marked clients invoke -> COMMIT -> idle receivers poll
//   R3 one input per node (timer or due message) -> COMMIT -> idle receivers poll
//   R4 clients run their recv! loop -> completion rows
// so an RPC to an idle node completes inside one round, and a gossip hop costs one round.
// =====================================================================================================
template <int PROG, bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64, 3) sim_kernel(const KParams p) {   // (three wavefronts per SIMD = 168 registers: at four, 20-60 B of private memory per lane in the round loop — tools/private_memory_audit.py)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const seen = reinterpret_cast<u32 *>(smem + p.off_seen);
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  // batched gossip (broadcast.py, DESIGN.md §2.4): per link an acknowledged prefix of the node's arrival log, one RPC in flight
  constexpr bool IS_BATCH = PROG == MSIM_NODE_BCAST_BATCH;
  constexpr bool IS_BCAST = (PROG >= MSIM_NODE_BCAST_FF && PROG <= MSIM_NODE_BCAST_RPC_ALL) || IS_BATCH;
  constexpr bool IS_RPC = PROG == MSIM_NODE_BCAST_ACK_RETRY || PROG == MSIM_NODE_BCAST_RPC_ALL;
  constexpr bool IS_ACK = PROG == MSIM_NODE_BCAST_ACK_RETRY;
  constexpr bool IS_PN = PROG == MSIM_NODE_PN_COUNTER;    // pn_counter.rb: same replication skeleton as g-set, counters instead of a set
  constexpr bool IS_GSET = PROG == MSIM_NODE_G_SET || IS_PN;  // "CRDT with a 5 s replicate timer"
  constexpr bool IS_ECHO = PROG == MSIM_NODE_ECHO;
  constexpr bool IS_FLAKE = PROG == MSIM_NODE_FLAKE_IDS;  // flake_ids.clj: unique-ids workload, Reusable clients (unique_ids.clj:59-61)
  constexpr bool HAS_FINAL = IS_BCAST || IS_GSET;
  constexpr bool FINAL_FLAG = IS_BCAST || IS_PN;  // :final? true on the last reads (broadcast.clj:240, pn_counter.clj:137)
  constexpr bool HAS_TIMERS = IS_ACK || IS_GSET || IS_BATCH;
  constexpr bool REP_FIRST = IS_ACK || IS_BATCH;  // the ack variant and batched gossip reply before they gossip
  constexpr u32 FAN_TYPE = IS_GSET ? M_REPLICATE : IS_BATCH ? M_BROADCAST_MANY : M_BROADCAST;
  // fan-outs of these programs only ever go to topology neighbours
  constexpr bool TOPO_BOUND = PROG == MSIM_NODE_BCAST_FF || PROG == MSIM_NODE_BCAST_FF_ECHOBACK || IS_ACK || IS_BATCH;
  // programs whose server<->server traffic is plain gossip (no msg_id, no reply): eligible for the cascade loop
  constexpr bool FAST_OK = PROG == MSIM_NODE_BCAST_FF || PROG == MSIM_NODE_BCAST_FF_ECHOBACK;

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS, W = p.W;
  const bool is_node = lane < N;
  const bool is_client = lane >= N && lane < N + CS;
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u64 lt_mask = (1ull << lane) - 1;
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u32 all_nodes = N >= 32 ? 0xFFFFFFFFu : ((1u << N) - 1);
  const u32 max_values = p.cfg.max_values, max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  // ack/retry scratch: unacked[N][V], fifo[N][V][2]; g-set scratch: snapshots[tick][N][W]
  u32 *const g_unacked = g_scr + (size_t)lane * max_values;
  u32 *const g_fifo = g_scr + (size_t)N * max_values + (size_t)lane * max_values * 2;
  // batched gossip scratch: arrival logs u16[N][V], then links uint4[N][N] = {acknowledged prefix, end of the batch in flight,
  // its RPC id, its deadline} of link (node, peer)
  uint16_t *const g_log = reinterpret_cast<uint16_t *>(g_scr);
  uint4 *const g_link = reinterpret_cast<uint4 *>(g_scr + (size_t)N * (max_values / 2));

  const u32 jcap = p.cfg.journal_capacity;  // net journal (journal.clj:53,220-239); 0 = off
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = is_node ? p.cap_node : CLIENT_INBOX_CAP;
  const u32 my_spill_cap = is_node ? p.spill_cap : 0u;
  uint4 *const my_inbox = inbox + (is_node ? lane * p.cap_node : (is_client ? N * p.cap_node + slot * CLIENT_INBOX_CAP : 0));
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)(is_node ? lane : 0) * p.spill_cap;  // HBM spill behind the LDS queue
  u32 *const my_seen = seen + (is_node ? lane : 0) * W;

  for (u32 i = lane; i < N * W; i += 64) seen[i] = 0;
  if (IS_ACK) { if (is_node) for (u32 v = 0; v < max_values; v++) g_unacked[v] = 0; }
  if (IS_BATCH) { if (is_node) for (u32 k = 0; k < N; k++) g_link[lane * N + k] = make_uint4(0, 0, 0, INF); }
  __syncthreads();

  const u32 adj = is_node ? topo_adj(p.cfg.topology, N, lane) : 0;
  // which lanes can ever address a fan-out to this node
  const u32 cand_all = is_node ? (TOPO_BOUND ? adj : (all_nodes & ~(1u << lane))) : 0u;
  const u32 c_mod_n = C % N;

  // ---- per-lane endpoint state ----
  bool has_c = false; u32 deliver_at = 0; uint4 cm = make_uint4(0, 0, 0, 0);  // the envelope recv! is sleeping on
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);                    // smallest arrival of this commit
  u32 in_n = 0, sp_n = 0;                                                     // queued envelopes in LDS / in the HBM spill
  u32 node_msgid = 0, timer_next = INF, tick = 0, part = 0;
  u32 flake_time = 0, flake_count = 0;  // flake_ids.clj:10-14
  u32 fifo_head = 0, fifo_tail = 0, retry_time = INF;
  u32 logn = 0, infl = 0;  // batched gossip: length of the arrival log, links with an RPC in flight (bit = peer)
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_f = 0, c_value = 0, process = slot, c_final = 0;
  u32 dest_node = is_client ? slot % N : 0;  // nodes[process mod n] [upstream], kept incrementally
  u32 m_f = 0, m_value = 0, m_final = 0;
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, next_value = 0, nem_next = 0, nem_j = 0;
  u32 sleep_until = 0, loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;  // journal cursor; :send events of a COMMIT sit at ev_base + (id - id_base)

#define PAYS_LATENCY(src) ((src) < N && is_node)   // neither end is a client (group64_net.inc)
#define ENDPOINT_LANES   // a lane is one endpoint: node, worker slot or service
#define COMMIT_FLAG   // has_c says whether an envelope is committed
  #include "group64_net.inc"
  // idle receivers poll (net.clj:223-247): min (deadline, id) over queued + just-arrived envelopes
  auto poll = [&]() {
    const bool elig = is_node || busy;  // clients only poll inside recv! (client.clj:94-95)
    if (have_pm) {
      have_pm = false;
      if (elig && !has_c && (in_n | sp_n) == 0) try_commit(pm);  // common case: nothing queued, no LDS traffic
      else lds_push(pm);
    }
    while (elig && !has_c && (in_n | sp_n) != 0) {
      u32 best = 0; bool in_spill = false;
      u64 bk = ~0ull;
      for (u32 i = 0; i < in_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_inbox[i]);
        const u64 k2 = ((u64)kk.x << 32) | kk.y;
        if (k2 < bk) { bk = k2; best = i; }
      }
      spill_min(my_spill, sp_n, bk, best, in_spill);  // deep queues only (long head-of-line sleeps)
      uint4 e;
      if (in_spill) { e = my_spill[best]; sp_n--; if (best != sp_n) my_spill[best] = my_spill[sp_n]; }
      else { e = my_inbox[best]; in_n--; if (best != in_n) my_inbox[best] = my_inbox[in_n]; }
      try_commit(e);
    }
  };
  // COMMIT of the nodes' fan-outs, receiver side: every node pulls from the lanes that may address it.
  // ids = next_id + id_off(sender) + rank of the receiver inside the sender's fan mask (net.clj:197).
  auto commit_fan = [&](u32 fan_mask, u32 fan_a, u32 fan_b0, u32 id_off) {
    const u32 send = (u32)__ballot(fan_mask != 0);
    u32 cand = cand_all & send;
    while (__ballot(cand != 0)) {
      const bool has = cand != 0;
      const u32 s = has ? (u32)__builtin_ctz(cand) : 0u;
      cand &= cand - 1;
      const u32 fs = lane_get(fan_mask, s);
      const u32 as = lane_get(fan_a, s);
      const u32 os = lane_get(id_off, s);
      u32 bs = 0;
      if (IS_RPC || IS_BATCH) bs = lane_get(fan_b0, s);
      if (has && ((fs >> lane) & 1)) {
        const u32 rank = __popc(fs & lt32);
        // batched gossip: the batch is [acknowledged prefix of link (s, lane), fan_a = s's log length), the RPC ids ascend with the peer
        const u32 a = IS_BATCH ? (g_link[s * N + lane].x | (as << 16)) : as;
        arrive(next_id + os + rank, FAN_TYPE, a, (IS_RPC || IS_BATCH) ? bs + rank : 0u, s);
      }
    }
  };

  for (;;) {
    const u64 busy_mask = __ballot(busy);  // only client lanes are ever busy

    // ---- time-free phase transitions (oracle: sched_resolve) ----
    if (!(phase == PH_MAIN && ((rate > 0 && gen_next < cutoff) || (NEM && nem_next < cutoff)))) {
      for (bool again = true; again;) {
        again = false;
        switch (phase) {
          case PH_INIT_WAIT: if (!busy_mask) { phase = IS_BCAST ? PH_TOPO : PH_MAIN_START; again = true; } break;
          case PH_TOPO_WAIT: if (!busy_mask) { phase = PH_MAIN_START; again = true; } break;
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
            if (busy_mask & worker_mask) break;
            phase = (NEM && HAS_FINAL) ? PH_NEM_FINAL : HAS_FINAL ? PH_SLEEP : PH_DONE;
            if (phase == PH_SLEEP) sleep_until = T + p.cfg.quiesce_ms * 1000u;
            again = true; break;
          case PH_FINAL_WAIT: if (!(busy_mask & worker_mask)) { phase = PH_DONE; again = true; } break;
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
      case PH_INIT: case PH_TOPO: case PH_NEM_FINAL: case PH_FINAL: due = T; break;
      case PH_SLEEP: due = sleep_until; break;
      case PH_MAIN:
        if (nem_live) due = max(nem_next, T);
        if (gen_live && free_mask) due = min(due, max(gen_next, T));
        if (rate == 0 && !nem_live) due = min(due, cutoff);
        break;
      default: break;
    }
    u32 my_t = has_c ? deliver_at : INF;  // this lane's next "normal" event
    if (HAS_TIMERS && is_node) my_t = min(my_t, min(timer_next, retry_time));
    #include "group64_jump.inc"

    bool inv_row = false; u32 inv_packed = 0, inv_value = 0;               // invoke row of this round
    const u32 inv_len = 0;   // an invocation carries no length (group64_rows.inc)
    bool cmp_row = false; u32 cmp_packed = 0, cmp_value = 0, cmp_len = 0;  // completion row of this round
    u32 nem_rows = 0, nem_f = 0, nem_v1 = 0, nem_v2 = 0, nem_len2 = 0;

    // completion of a client op (oracle: client_complete)
    auto complete = [&](u32 type, u32 err, u32 value, u32 len) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) my_flags |= MSIM_FLAG_ROUND_LIMIT; return; }
      cmp_row = true; cmp_packed = type | (c_f << 2) | (err << 7) | (c_final << 11) | (process << 12);
      cmp_value = value; cmp_len = len;
      if (type == MSIM_T_INFO) {  // crashed process: new process id, fresh client [upstream interpreter]
        process += C; dest_node += c_mod_n; if (dest_node >= N) dest_node -= N;
        if (!IS_FLAKE) { next_msg_id = 0; in_n = 0; }  // Reusable clients (unique_ids.clj:59-61) are not re-opened
      }
    };

    if (timeout_round) {
      if (busy && timeout_at <= T) {  // client.clj:96-103 + :158-162
        const bool idem = IS_BCAST && c_f == MSIM_F_READ;
        complete(idem ? MSIM_T_FAIL : MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_f == MSIM_F_READ ? MSIM_NO_VALUE : c_value, 0);
      }
    } else {
      // ---- R1: scheduler (generator interpreter, nemesis) — wave-uniform ----
      if (due <= T) {
        switch (phase) {
          case PH_INIT: if (is_client && slot < N) { mark = true; kind = K_INIT; } phase = PH_INIT_WAIT; break;
          case PH_TOPO: if (is_client && slot < N) { mark = true; kind = K_TOPO; } phase = PH_TOPO_WAIT; break;
          case PH_MAIN: {
            #include "group64_nemesis.inc"
            if (gen_live && gen_next <= T && free_mask) {
              // one 64-bit draw per generated op: high word -> stagger, low word -> pick / mix / echo payload
              const u32 nfree = __popcll(free_mask);
              const u32 kk = gen_k++;
              const u64 h = draw64(key, S_GEN, kk);
              const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
              const u32 pick = scale32(r_lo, nfree);
              const bool sel = is_worker && !busy && (u32)__popcll(free_mask & lt_mask) == pick;
              u32 f, val = MSIM_NO_VALUE;
              bool ok = true;
              if (IS_ECHO) { f = MSIM_F_ECHO; val = (r_lo >> 4) & 127; }
              else if (IS_FLAKE) f = MSIM_F_GENERATE;  // (gen/repeat {:f :generate}), unique_ids.clj:72
              else if (IS_PN && p.cfg.workload == MSIM_WL_G_COUNTER) {
                // g_counter.clj:37-41: (gen/filter ...) skips negative adds and takes the mix's next op at once
                u32 rr = r_lo, a = 0;
                int d = (int)((((rr >> 4) & 0xFFFFu) * 10u) >> 16) - 5;
                while (!(rr & 1) && d < 0 && a < 15) { a++; rr = (u32)draw64(key, S_GEN2, (u64)kk * 16 + a); d = (int)((((rr >> 4) & 0xFFFFu) * 10u) >> 16) - 5; }
                if ((rr & 1) || d < 0) f = MSIM_F_READ; else { f = MSIM_F_ADD; val = (u32)d; }
              }
              else if (r_lo & 1) f = MSIM_F_READ;
              else {
                f = IS_BCAST ? MSIM_F_BROADCAST : MSIM_F_ADD;
                if (IS_PN) val = (u32)((int)((((r_lo >> 4) & 0xFFFFu) * 10u) >> 16) - 5);  // (- (rand-int 10) 5), pn_counter.clj:134-135
                else if (next_value >= max_values) { flags |= MSIM_FLAG_VALUES_OVERFLOW; ok = false; }
                else val = next_value++;
              }
              if (!ok) { phase = PH_DONE; break; }
              if (sel) { mark = true; kind = K_OP; m_f = f; m_value = val; m_final = 0; }
              gen_next = T + __umulhi(r_hi, p.gen_period2_us);
            }
          } break;
          case PH_NEM_FINAL:
            part = 0; nem_rows = 2; nem_f = MSIM_F_STOP_PARTITION; nem_v1 = MSIM_NO_VALUE; nem_v2 = MSIM_NO_VALUE;
            phase = PH_SLEEP; sleep_until = T + p.cfg.quiesce_ms * 1000u; break;
          case PH_SLEEP:
            if (T < sleep_until) break;
            phase = PH_FINAL;
            [[fallthrough]];
          case PH_FINAL:
            if (is_worker) { mark = true; kind = K_OP; m_f = MSIM_F_READ; m_value = MSIM_NO_VALUE; m_final = FINAL_FLAG ? 1 : 0; }
            phase = PH_FINAL_WAIT; break;
          default: break;
        }
        if (phase == PH_DONE) break;
      }

      // ---- R2: marked clients invoke; COMMIT (ids in slot order); idle receivers poll ----
      u64 inv_mask = __ballot(mark);
      if (inv_mask) {
        u32 rq_dest = 0, rq_type = 0, rq_a = 0;
        if (mark) {  // oracle: client_invoke
          mark = false; busy = true;
          if (kind == K_INIT) { rq_dest = slot; rq_type = M_INIT; next_msg_id = 0; }
          else if (kind == K_TOPO) { rq_dest = slot; rq_type = M_TOPOLOGY; next_msg_id = 0; }
          else {
            c_f = m_f; c_value = m_value; c_final = m_final;
            rq_dest = dest_node;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (c_f << 2) | (c_final << 11) | (process << 12); inv_value = c_value;
            rq_type = c_f == MSIM_F_ECHO ? M_ECHO : c_f == MSIM_F_BROADCAST ? M_BROADCAST : c_f == MSIM_F_ADD ? M_ADD : c_f == MSIM_F_GENERATE ? M_GENERATE : M_READ;
            rq_a = (c_f == MSIM_F_READ || c_f == MSIM_F_GENERATE) ? 0u : c_value;
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

      // ---- R3: one input per node: a due timer, else the due committed envelope ----
      u32 fan_mask = 0, fan_a = 0, fan_b0 = 0;
      bool rep = false; u32 rep_dest = 0, rep_type = 0, rep_a = 0, rep_b = 0;
      bool rd = false;
      u64 jd_mask = 0;  // nodes delivering an envelope this round (their :recv events come first, node order)
      if (jcap) jd_mask = __ballot(is_node && !((IS_GSET || IS_BATCH) && timer_next <= T) && !(IS_ACK && retry_time <= T) && has_c && deliver_at <= T);
      u32 bsend = 0;                                  // batched gossip: links that send a new batch in this input
      bool grew = false, mrg = false; u32 mrg_a = 0;  // ... the log grew / a broadcast_many range to merge (wavefront pass below)
      if (is_node) {
        if (IS_GSET && timer_next <= T) {  // g_set.rb:33-38
          timer_next = T + 5000000u;
          u32 *snap = g_scr + ((size_t)tick * N + lane) * W;
          for (u32 w = 0; w < W; w++) snap[w] = my_seen[w];
          fan_mask = all_nodes & ~(1u << lane); fan_a = tick; tick++;
        } else if (IS_ACK && retry_time <= T) {  // gossip thread wakes (02-performance.md:421-438)
          const u32 slot_i = (fifo_head % max_values) * 2;
          const u32 v = g_fifo[slot_i];
          fifo_head++;
          const u32 un = g_unacked[v];
          if (un) {
            fan_mask = un; fan_a = v; fan_b0 = node_msgid + 1; node_msgid += __popc(un);
            const u32 ts = (fifo_tail % max_values) * 2;
            g_fifo[ts] = v; g_fifo[ts + 1] = T + 1000000u; fifo_tail++;
          }
          retry_time = fifo_head < fifo_tail ? g_fifo[(fifo_head % max_values) * 2 + 1] : INF;
        } else if (IS_BATCH && timer_next <= T) {  // the node's timer input: every RPC whose 1 s ran out (maelstrom.py:89-98) is sent again
          u32 m = infl, tmin = INF;
          while (m) {
            const u32 k = (u32)__builtin_ctz(m); m &= m - 1;
            const u32 dl = g_link[lane * N + k].w;
            if (dl <= T) bsend |= 1u << k; else tmin = min(tmin, dl);
          }
          timer_next = tmin;
        } else if (has_c && deliver_at <= T) {
          const uint4 q = cm; has_c = false;
          const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
          if (qsrc >= N) s_recv_cl++; else s_recv_sv++;  // journal :recv (net.clj:244)
          if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
          if (IS_BATCH && qtype == M_BROADCAST_MANY) {  // broadcast.py:27-31: merged by the wavefront below, then broadcast_many_ok
            mrg = true; mrg_a = qa; rep = true; rep_dest = qsrc; rep_type = M_BROADCAST_MANY_OK; rep_b = qb;
          } else if (IS_BATCH && qtype == M_BROADCAST_MANY_OK) {  // broadcast.py:59-60: the batch in flight is acknowledged; a late reply (maelstrom.py:100,153) does nothing
            if ((infl >> qsrc) & 1) {
              uint4 l = g_link[lane * N + qsrc];
              if (l.z == qb) {
                l.x = l.y; l.w = INF; g_link[lane * N + qsrc] = l;
                infl &= ~(1u << qsrc);
                if (l.x < logn) bsend = 1u << qsrc;  // more arrived meanwhile: the next batch goes at once
                u32 m = infl, tmin = INF;
                while (m) { const u32 k = (u32)__builtin_ctz(m); m &= m - 1; tmin = min(tmin, g_link[lane * N + k].w); }
                timer_next = tmin;
              }
            }
          } else
          switch (qtype) {
            case M_INIT:
              if (IS_GSET) timer_next = T;
              rep = true; rep_dest = qsrc; rep_type = M_INIT_OK; rep_b = qb; break;
            case M_TOPOLOGY: rep = true; rep_dest = qsrc; rep_type = M_TOPOLOGY_OK; rep_b = qb; break;
            case M_ECHO: rep = true; rep_dest = qsrc; rep_type = M_ECHO_OK; rep_a = qa; rep_b = qb; break;
            case M_GENERATE: {  // flake_ids.clj:16-31: [max(now in s, last time), counter within that second, node]
              u32 t = T / 1000000u;
              if (t < flake_time) t = flake_time;
              flake_count = t == flake_time ? flake_count + 1 : 0u; flake_time = t;
              rep = true; rep_dest = qsrc; rep_type = M_GENERATE_OK; rep_a = (t << 20) | ((flake_count & 0x7FFFu) << 5) | lane; rep_b = qb;
            } break;
            case M_READ:
              rep = true; rep_dest = qsrc; rep_type = M_READ_OK; rep_b = qb;
              if (IS_PN) { u32 v = 0; for (u32 i = 0; i < N; i++) v += my_seen[i] - my_seen[N + i]; rep_a = v; }  // increments - decrements
              else rd = true;
              break;
            case M_ADD:
              if (IS_PN) { const int d = (int)qa; if (d >= 0) my_seen[lane] += (u32)d; else my_seen[N + lane] += (u32)(-d); }  // own slot of inc / dec
              else my_seen[qa >> 5] |= 1u << (qa & 31);
              rep = true; rep_dest = qsrc; rep_type = M_ADD_OK; rep_a = qa; rep_b = qb; break;
            case M_REPLICATE: {
              const u32 *snap = g_scr + ((size_t)qa * N + qsrc) * W;
              if (IS_PN) merge_snapshot<true>(my_seen, snap, W);  // element-wise max
              else merge_snapshot<false>(my_seen, snap, W);
            } break;
            case M_BROADCAST: {
              const u32 v = qa, bitm = 1u << (v & 31);
              if (IS_BATCH) {  // broadcast.py:12-24
                const u32 wv = my_seen[v >> 5];
                if (!(wv & bitm)) { my_seen[v >> 5] = wv | bitm; if (logn < max_values) g_log[(size_t)lane * max_values + logn] = (uint16_t)v; logn++; grew = true; }
                rep = true; rep_dest = qsrc; rep_type = M_BROADCAST_OK; rep_a = v; rep_b = qb;
                break;
              }
              const u32 wv = my_seen[v >> 5];
              if (!(wv & bitm)) {
                my_seen[v >> 5] = wv | bitm;
                u32 tg = PROG == MSIM_NODE_BCAST_RPC_ALL ? (all_nodes & ~(1u << lane)) : adj;
                if (PROG != MSIM_NODE_BCAST_FF_ECHOBACK && qsrc < N) tg &= ~(1u << qsrc);
                fan_mask = tg; fan_a = v;
                if (IS_RPC) { fan_b0 = node_msgid + 1; node_msgid += __popc(tg); }
                if (IS_ACK && tg) {
                  g_unacked[v] = tg;
                  const u32 ts = (fifo_tail % max_values) * 2;
                  g_fifo[ts] = v; g_fifo[ts + 1] = T + 1000000u;
                  if (fifo_head == fifo_tail) retry_time = T + 1000000u;
                  fifo_tail++;
                }
              }
              if (qb != 0) { rep = true; rep_dest = qsrc; rep_type = M_BROADCAST_OK; rep_a = v; rep_b = qb; }
            } break;
            case M_BROADCAST_OK: if (IS_ACK) g_unacked[qa] &= ~(1u << qsrc); break;
            default: break;
          }
        }
      }

      if (IS_BATCH) {
        // merge the received ranges, one receiver at a time, 64 values per step: every lane tests one value against the receiver's
        // set, the new ones are compacted by a prefix count and appended to its arrival log (a batch has no duplicates)
        u64 mm = __ballot(mrg);
        if (mm) {
          __syncthreads();  // the senders' logs and the sets in LDS were written by other lanes
          while (mm) {
            const u32 r = (u32)__builtin_ctzll(mm); mm &= mm - 1;
            const u32 s = rdlane(rep_dest, r), ra = rdlane(mrg_a, r);
            const u32 from = ra & 0xFFFFu, to = min(ra >> 16, max_values);
            const uint16_t *src_log = g_log + (size_t)s * max_values;
            uint16_t *dst_log = g_log + (size_t)r * max_values;
            u32 *rset = seen + r * W;
            const u32 n0 = rdlane(logn, r);
            u32 n = n0;
            for (u32 b = from; b < to; b += 64) {
              const u32 i = b + lane;
              const u32 v = i < to ? (u32)src_log[i] : 0u;
              const bool fresh = i < to && !((rset[v >> 5] >> (v & 31)) & 1u);
              const u64 fm = __ballot(fresh);
              if (fresh) {
                const u32 at = n + (u32)__popcll(fm & lt_mask);
                if (at < max_values) dst_log[at] = (uint16_t)v;
                atomicOr(&rset[v >> 5], 1u << (v & 31));
              }
              n += (u32)__popcll(fm);
            }
            if (lane == r) { logn = n; grew = n != n0; }
          }
        }
        // a grown log wakes every idle link (broadcast.py:16-17,51-56); new RPCs in ascending peer order, ids from the node's one counter
        if (is_node) {
          if (grew) bsend = adj & ~infl;
          if (bsend) {
            u32 m = bsend, id = node_msgid;
            while (m) {
              const u32 k = (u32)__builtin_ctz(m); m &= m - 1;
              uint4 l = g_link[lane * N + k];
              l.y = logn; l.z = ++id; l.w = T + 1000000u;
              g_link[lane * N + k] = l;
            }
            fan_mask = bsend; fan_a = logn; fan_b0 = node_msgid + 1; node_msgid = id;
            infl |= bsend; timer_next = min(timer_next, T + 1000000u);
          }
        }
        if (__ballot(bsend != 0)) __syncthreads();  // the receivers read the senders' acknowledged prefixes (commit_fan)
      }
      n_ev += (u32)__popcll(jd_mask);
      // read results: the whole wave copies the node's set LDS -> HBM payload (256 B per instruction)
      {
        u64 rdmask = __ballot(rd);
        if (rdmask) {
          __syncthreads();
          const u32 words = (next_value + 31) >> 5;
          while (rdmask) {
            const u32 r = (u32)__builtin_ctzll(rdmask); rdmask &= rdmask - 1;
            u32 off = 0;
            if (n_payload + words > max_pay) flags |= MSIM_FLAG_PAYLOAD_OVERFLOW;
            else {
              off = n_payload; n_payload += words;
              for (u32 w = lane; w < words; w += 64) g_pay[off + w] = seen[r * W + w];
            }
            if (lane == r) rep_a = off | (words << 24);
          }
        }
      }

      // COMMIT node sends (net.clj:189-221): ids in node order, then emission order
      {
        const u32 fan_cnt = __popc(fan_mask);
        const u32 cnt = fan_cnt + (rep ? 1u : 0u);
        if (__ballot(cnt != 0)) {
          const u32 incl = scan32(cnt);  // senders are node lanes (< 32)
          ev_base = n_ev; id_base = next_id; n_ev += rdlane(incl, 31);
          if (is_node) { s_send_sv += fan_cnt; if (rep) { if (rep_dest >= N) s_send_cl++; else s_send_sv++; } }
          if (__ballot(fan_mask != 0)) commit_fan(fan_mask, fan_a, fan_b0, incl - cnt + ((REP_FIRST && rep) ? 1u : 0u));
          u64 reps = __ballot(rep);
          if (reps) {
            const u32 rep_pack = rep_dest | (rep_type << 8);
            const u32 rep_off = incl - cnt + (REP_FIRST ? 0u : fan_cnt);
            while (reps) {
              const u32 s = (u32)__builtin_ctzll(reps); reps &= reps - 1;
              const u32 pk = rdlane(rep_pack, s), o = rdlane(rep_off, s);
              const u32 r_a = rdlane(rep_a, s), r_b = rdlane(rep_b, s);
              if (lane == (pk & 0xFF)) arrive(next_id + o, pk >> 8, r_a, r_b, s);
            }
          }
          next_id += rdlane(incl, 31);
        }
        poll();  // every round: a node that just went idle may still have queued envelopes
      }

      // ---- R4: clients run their recv! loops (client.clj:94-107); envelope k of every client before envelope k+1 ----
      for (;;) {
        const bool dl = is_client && has_c && deliver_at <= T;
        const u64 dm = __ballot(dl);
        if (!dm) break;
        if (dl) {
          const uint4 q = cm; has_c = false;
          s_recv_cl++;
          const u32 qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
          if (jcap) jwrite(n_ev + (u32)__popcll(dm & lt_mask), 1, q.y, qa, qb, q.w >> 24, lane);
          if (busy && qb == want) {  // else: stale reply, keep polling (client.clj:105-107)
            if (qtype == M_READ_OK) { if (IS_PN) complete(MSIM_T_OK, 0, qa, 0); else complete(MSIM_T_OK, 0, qa & 0xFFFFFFu, qa >> 24); }
            else if (qtype == M_ECHO_OK || qtype == M_GENERATE_OK) complete(MSIM_T_OK, 0, qa, 0);
            else complete(MSIM_T_OK, 0, c_value, 0);
          }
          poll();
        }
        n_ev += (u32)__popcll(dm);
      }
    }

    #include "group64_rows.inc"

    // ---- cascade loop: while the scheduler is quiet at T and only plain gossip is due, every round is
    //      R3 + COMMIT + poll (no scheduler, no clients, no rows).  Same rounds the loop above would run. ----
    if (FAST_OK && !timeout_round) {
      const u64 bm = __ballot(busy);
      bool quiet = false;
      u32 d2 = INF;  // when the scheduler next wants to act (the clients' busy set cannot change inside this loop)
      if (phase == PH_MAIN) {
        const bool gl = rate > 0 && gen_next < cutoff, nl = NEM && nem_next < cutoff;
        if (gl || nl) {
          if (nl) d2 = max(nem_next, T);
          if (gl && (worker_mask & ~bm)) d2 = min(d2, max(gen_next, T));
          quiet = d2 > T;
        }
      } else if (phase == PH_SLEEP) { d2 = sleep_until; quiet = d2 > T; }
      while (quiet) {
        bool due_now = has_c && deliver_at <= T;  // only node lanes hold an envelope across rounds
        if (!__ballot(due_now)) {
          // R0 inside the loop: jump to the next delivery if it precedes the scheduler and every client timeout
          u32 k = has_c ? deliver_at * 2 : INF;
          if (busy) k = min(k, timeout_at * 2 + 1);
          const u32 km = wave_min(k);
          if (km == INF || (km & 1) || (km >> 1) >= d2) break;
          T = km >> 1;
          due_now = has_c && deliver_at <= T;
        }
        const bool plain = (cm.y & 0xFFu) == M_BROADCAST && (cm.w & 0xFFFFFFu) == 0;
        if (__ballot(due_now && !plain)) break;
        if (++rounds > ROUND_LIMIT) { flags |= MSIM_FLAG_ROUND_LIMIT; phase = PH_DONE; break; }
        const u32 v = cm.z;
        u32 fan = 0;
        if (jcap) {
          const u64 dmj = __ballot(due_now);
          if (due_now) jwrite(n_ev + (u32)__popcll(dmj & lt_mask), 1, cm.y, v, 0, cm.w >> 24, lane);
          n_ev += (u32)__popcll(dmj);
        }
        if (due_now) {
          has_c = false; s_recv_sv++;
          const u32 wv = my_seen[v >> 5], bitm = 1u << (v & 31);
          if (!(wv & bitm)) {
            my_seen[v >> 5] = wv | bitm;
            fan = PROG == MSIM_NODE_BCAST_FF_ECHOBACK ? adj : (adj & ~(1u << (cm.w >> 24)));
          }
        }
        if (__ballot(fan != 0)) {
          const u32 cnt = __popc(fan);
          const u32 incl = scan32(cnt);
          s_send_sv += cnt;
          ev_base = n_ev; id_base = next_id; n_ev += rdlane(incl, 31);
          commit_fan(fan, v, 0, incl - cnt);
          next_id += rdlane(incl, 31);
        }
        poll();
      }
      if (phase == PH_DONE) break;
    }
  }

  // ---- epilogue: flush the partial row block, reduce counters, write stats + meta ----
  __syncthreads();
  {
    const u32 blk = n_rows >> 6;
    const u32 gi = blk * 64 + lane;
    if (gi < n_rows) reinterpret_cast<uint4 *>(g_rows)[gi] = stage[gi % STAGE_ROWS];
  }
  const u32 t_send_cl = wave_sum(s_send_cl), t_send_sv = wave_sum(s_send_sv);
  const u32 t_recv_cl = wave_sum(s_recv_cl), t_recv_sv = wave_sum(s_recv_sv);
  for (u32 b = 1; b <= MSIM_FLAG_JOURNAL_OVERFLOW; b <<= 1) if (__ballot((my_flags & b) != 0)) flags |= b;
  if (lane == 0) {
    msim_net_stats st;
    st.all_send = (u64)t_send_cl + t_send_sv; st.all_recv = (u64)t_recv_cl + t_recv_sv;
    st.clients_send = t_send_cl; st.clients_recv = t_recv_cl;
    st.servers_send = t_send_sv; st.servers_recv = t_recv_sv;
    p.stats[inst] = st;
    msim_inst_meta m; m.n_rows = n_rows; m.n_payload_words = n_payload; m.flags = flags; m.n_rounds = rounds;
    m.n_events = jcap ? n_ev : 0; m.reserved[0] = 0; m.reserved[1] = 0; m.reserved[2] = 0;
    p.meta[inst] = m;
  }
}
#include "group64_end.inc"
