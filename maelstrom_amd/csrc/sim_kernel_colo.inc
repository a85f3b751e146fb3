// sim_kernel_colo.inc — included by engine.hip (same translation unit: shares the RNG, DPP and topology helpers).
//
// "Colocated" layout of the simulation kernel, used when concurrency == n_nodes (the reference's default
// `--concurrency 1n`, [upstream] jepsen.cli): worker t always talks to node t (nodes[process mod n], and
// process only ever changes by +concurrency), so lane i holds node i AND client slot i.  Every client RPC is
// then lane-local — request, node handler, reply and completion never cross lanes — and only server<->server
// traffic uses the cross-lane COMMIT.  Semantics, ids, row order and RNG are exactly those of DESIGN.md §2
// (and of sim_kernel<> above, which stays the general layout); only the placement of client state differs.
//
// Extra specialisation: LEAN = constant latency, no loss.  All arrivals of a round then share one deadline and
// come in id order, so the first arrival is the queue minimum without comparing keys.

// ---- the quiet stretch as a function of its own ------------------------------------------------------------------
// Between unusual events (phase changes, final reads, a busy client, anything the short paths do not cover) a fire-and-
// forget broadcast cluster at constant latency does only two things: lone client operations on an idle cluster and the
// gossip cascades they start.  quiet_run<> executes whole sequences of such rounds — the same rounds, ids, rows, payload
// and counters as the loop in sim_kernel_colo<>, which it returns to, without side effects, at the first round it cannot
// take — with only the state those rounds touch in registers.  Calls are rare, so the state travels by reference.
struct QuietIO {
  u32 deliver_at, cm_y, cm_z, cm_w, in_n, sp_n, special;                       // per lane: node
  u32 process, next_msg_id, c_f, c_value, did_op;                               // per lane: client (did_op: it ran an operation in here)
  u32 T, next_id, rounds, n_rows, n_payload, gen_k, gen_next, next_value;       // wave-uniform
  u32 send_cl, recv_cl, send_sv, recv_sv, fast, d2, stop;                       // counters to add; cascade mode; stop = 1: round limit
};
struct QuietK {  // constants of the run
  u64 key; msim_op *g_rows; u32 *g_pay; uint4 *my_spill; u32 *g_flags;
  u32 off_inbox, off_seen, off_seen_all, W, adj, lane, N, my_cap, my_spill_cap, lat_us, cutoff, gen_period2_us, max_rows, max_pay, max_values, all_nodes;
};

template <bool ECHOBACK>
__device__ __attribute__((noinline)) void quiet_run(QuietIO &io, const QuietK &kc, u32 cin_n) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const my_inbox = reinterpret_cast<uint4 *>(smem + kc.off_inbox);
  u32 *const my_seen = reinterpret_cast<u32 *>(smem + kc.off_seen);
  const u32 *const seen = reinterpret_cast<const u32 *>(smem + kc.off_seen_all);
  const u32 lane = kc.lane, adj = kc.adj;
  const bool is_node = lane < kc.N;
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
#define UNI(x) ((u32)__builtin_amdgcn_readfirstlane((int)(x)))
  const u32 N = UNI(kc.N), W = UNI(kc.W), my_cap = UNI(kc.my_cap), lat_us = UNI(kc.lat_us);
  const u32 cutoff = UNI(kc.cutoff), gen_period2_us = UNI(kc.gen_period2_us), max_rows = UNI(kc.max_rows), max_pay = UNI(kc.max_pay);
  const u32 max_values = UNI(kc.max_values), all_nodes = UNI(kc.all_nodes);
  const u64 key = ((u64)UNI((u32)(kc.key >> 32)) << 32) | UNI((u32)kc.key);
  msim_op *const g_rows = kc.g_rows; u32 *const g_pay = kc.g_pay;

  u32 deliver_at = io.deliver_at, cm_y = io.cm_y, cm_z = io.cm_z, cm_w = io.cm_w, in_n = io.in_n, sp_n = io.sp_n;
  bool special = io.special != 0;
  u32 process = io.process, next_msg_id = io.next_msg_id, c_f = io.c_f, c_value = io.c_value, did_op = 0;
  u32 T = UNI(io.T), next_id = UNI(io.next_id), rounds = UNI(io.rounds), n_rows = UNI(io.n_rows), n_payload = UNI(io.n_payload);
  u32 gen_k = UNI(io.gen_k), gen_next = UNI(io.gen_next), next_value = UNI(io.next_value), d2 = UNI(io.d2);
  bool fast = UNI(io.fast) != 0;
  u32 send_cl = 0, recv_cl = 0, send_sv = 0, recv_sv = 0, stop = 0;
#undef UNI

  // every round in here starts with room for a full round of arrivals (one per neighbour) in the LDS part of each queue —
  // checked below, else the round goes back to the loop — so a push is a plain store: no capacity branches on the hot path
  const u32 room_need = __popc(adj);
  auto lds_push = [&](u32 x, u32 y, u32 z, u32 w) { my_inbox[in_n++] = make_uint4(x, y, z, w); };
  auto try_commit = [&](u32 x, u32 y, u32 z, u32 w) {
    cm_y = y; cm_z = z; cm_w = w;
    special = !((y & 0xFFu) == M_BROADCAST && (w & 0xFFFFFFu) == 0);
    if (lat_us == 0) deliver_at = T;
    else deliver_at = x <= T ? T : T + ((x - T) / 1000u) * 1000u;
  };
  auto poll_queue = [&]() {   // idle with a queue: recv! takes the minimum (deadline, id)
    if (is_node && deliver_at == INF && in_n != 0) {
      u32 best = 0;
      u64 bk = ~0ull;
      for (u32 i = 0; i < in_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_inbox[i]);
        const u64 k2 = ((u64)kk.x << 32) | kk.y;
        if (k2 < bk) { bk = k2; best = i; }
      }
      const uint4 e = my_inbox[best];   // (no spilled part in here: checked at the top of the round)
      in_n--; if (best != in_n) my_inbox[best] = my_inbox[in_n];
      try_commit(e.x, e.y, e.z, e.w);
    }
  };

  for (;;) {
    if (__ballot(is_node && (sp_n != 0 || in_n + room_need > my_cap))) break;   // a queue may spill this round: the loop's paths handle that
    if (fast) {
      // ---- a cascade round (see the inline version in sim_kernel_colo<>) ----
      bool due_now = deliver_at <= T;
      if (!__ballot(due_now)) {
        const u32 k = deliver_at == INF ? INF : deliver_at * 2;   // no client is busy in here: no timeout keys
        const u32 km = __ballot(k != INF) ? wave_min(k) : INF;
        if (km == INF || (km >> 1) >= d2) { fast = false; continue; }
        T = km >> 1;
        due_now = deliver_at <= T;
      }
      if (__ballot(due_now && special)) { fast = false; continue; }
      recv_sv += __popc((u32)__ballot(due_now));
      if (++rounds > ROUND_LIMIT) { stop = 1; break; }
      const u32 v = cm_z;
      u32 fan = 0;
      if (due_now) {
        deliver_at = INF;
        const u32 wv = my_seen[v >> 5], bitm = 1u << (v & 31);
        if (!(wv & bitm)) {
          my_seen[v >> 5] = wv | bitm;
          fan = ECHOBACK ? adj : (adj & ~(1u << (cm_w >> 24)));
        }
      }
      const u32 send = (u32)__ballot(fan != 0);
      bool got = false; u32 g_y = 0, g_z = 0, g_w = 0;
      const u32 in0 = in_n | sp_n;
      if (send) {
        const u32 cnt = __popc(fan);
        const u32 incl = scan32(cnt);
        const u32 pk = v | ((incl - cnt) << 16);
        u32 cand = adj & send;
        while (__ballot(cand != 0)) {
          const bool has = cand != 0;
          const u32 s = has ? (u32)__builtin_ctz(cand) : 0u;
          cand &= cand - 1;
          const u32 fs = lane_get(fan, s), ps = lane_get(pk, s);
          if (has && ((fs >> lane) & 1)) {
            const u32 y = ((next_id + (ps >> 16) + __popc(fs & lt32)) << 8) | M_BROADCAST;
            if (!got) { got = true; g_y = y; g_z = ps & 0xFFFFu; g_w = s << 24; }
            else lds_push(T + lat_us, y, ps & 0xFFFFu, s << 24);
          }
        }
        const u32 total = rdlane(incl, 31);
        next_id += total; send_sv += total;
      }
      if (got) {
        if (deliver_at == INF && in0 == 0) try_commit(T + lat_us, g_y, g_z, g_w); else lds_push(T + lat_us, g_y, g_z, g_w);
      }
      if (__ballot(deliver_at == INF && (in_n | sp_n) != 0)) poll_queue();
      continue;
    }

    // ---- the next round is a general one: take it only if it is a lone client operation, else hand back untouched ----
    if (!(gen_next < cutoff)) break;                                          // generator exhausted: phase transitions follow
    const u32 due = max(gen_next, T);                                         // every worker is free in here
    u32 T2 = T;
    const bool any_due = __ballot(is_node && deliver_at <= T) != 0;
    if (due > T && !any_due) {                                                // R0: jump to the earliest event
      const u32 k = deliver_at == INF ? INF : deliver_at * 2;
      u32 km = __ballot(k != INF) ? wave_min(k) : INF;
      km = min(km, due * 2);
      T2 = max(T, km >> 1);
    }
    if (due > T2) break;                                                      // a delivery comes first: general round
    if (__ballot(is_node && deliver_at <= T2)) break;                         // something else is due at the same instant
    const u32 kk = gen_k;
    const u64 h = draw64(key, S_GEN, kk);
    const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
    const u32 pick = scale32(r_lo, N);                                        // nfree = N
    const bool sel = is_node && lane == pick;
    const bool rd_op = (r_lo & 1) != 0;
    const u32 words = (next_value + 31) >> 5;
    const bool fits = (rd_op ? n_payload + words <= max_pay : next_value < max_values) && n_rows + 2 <= max_rows;
    if (!fits || !__ballot(sel && deliver_at == INF && (in_n | sp_n) == 0 && cin_n == 0)) break;
    if (rounds + 1 > ROUND_LIMIT) break;                                      // let the loop raise it
    // committed: this round is ours
    rounds++; T = T2; gen_k++;
    const u32 sl = pick;
    const u32 f = rd_op ? MSIM_F_READ : MSIM_F_BROADCAST;
    const u32 val = rd_op ? MSIM_NO_VALUE : next_value;
    if (!rd_op) next_value++;
    const u32 base = next_id + 1;
    const u32 fan_s = rd_op ? 0u : rdlane(adj, sl);
    const u32 cnt = __popc(fan_s);
    u32 off = 0;
    if (rd_op) {
      __syncthreads();
      off = n_payload; n_payload += words;
      for (u32 w = lane; w < words; w += 64) g_pay[off + w] = seen[sl * W + w];
    }
    const u32 tlo = (u32)((u64)T * 1000ull), thi = (u32)(((u64)T * 1000ull) >> 32);
    if (sel) {
      did_op = 1; c_f = f; c_value = val; ++next_msg_id;
      if (!rd_op) my_seen[val >> 5] |= 1u << (val & 31);
      stage[n_rows % STAGE_ROWS] = make_uint4(tlo, thi, MSIM_T_INVOKE | (f << 2) | (process << 12), val);
      stage[(n_rows + 1) % STAGE_ROWS] = make_uint4(tlo, thi | ((rd_op ? words : 0u) << 16), MSIM_T_OK | (f << 2) | (process << 12), rd_op ? off : val);
    }
    {
      const u32 new_n = n_rows + 2;
      if ((new_n >> 6) != (n_rows >> 6)) {
        __syncthreads();
        const u32 gi = (n_rows >> 6) * 64 + lane;
        if (gi < max_rows) reinterpret_cast<uint4 *>(g_rows)[gi] = stage[gi % STAGE_ROWS];
        __syncthreads();
      }
      n_rows = new_n;
    }
    if (cnt) {
      if (is_node && ((fan_s >> lane) & 1)) {
        const u32 y = ((base + __popc(fan_s & lt32)) << 8) | M_BROADCAST;
        if (deliver_at == INF && (in_n | sp_n) == 0) try_commit(T + lat_us, y, val, sl << 24); else lds_push(T + lat_us, y, val, sl << 24);
      }
    }
    next_id += 2 + cnt;
    send_cl += 2; recv_cl += 2; send_sv += cnt;
    gen_next = T + __umulhi(r_hi, gen_period2_us);
    // the round's tail: cascade mode while the scheduler stays quiet
    d2 = gen_next < cutoff ? max(gen_next, T) : INF;
    fast = gen_next < cutoff && d2 > T;
    (void)all_nodes;
  }
  io.deliver_at = deliver_at; io.cm_y = cm_y; io.cm_z = cm_z; io.cm_w = cm_w; io.in_n = in_n; io.sp_n = sp_n; io.special = special ? 1u : 0u;
  io.process = process; io.next_msg_id = next_msg_id; io.c_f = c_f; io.c_value = c_value; io.did_op = did_op;
  io.T = T; io.next_id = next_id; io.rounds = rounds; io.n_rows = n_rows; io.n_payload = n_payload; io.gen_k = gen_k; io.gen_next = gen_next;
  io.next_value = next_value; io.send_cl = send_cl; io.recv_cl = recv_cl; io.send_sv = send_sv; io.recv_sv = recv_sv;
  io.fast = fast ? 1u : 0u; io.d2 = d2; io.stop = stop;
}

// ---- cascade rounds as a function of their own --------------------------------------------------------------------
// The plain-gossip rounds between two scheduler events touch a small part of the cluster state (each node's recv!
// register and queue, the seen-sets, a few counters).  Inlined into the round loop they inherit its register allocation:
// every value the big loop carries is copied around this hot body too (the kernel is VALU-issue bound and a third of its
// VALU instructions were such copies).  As a separate function the body keeps only what it uses in registers; the state
// crosses the call by value, in registers.  Constant latency, no loss, scan queues, journal off (the headline case);
// everything else stays on the inline path in sim_kernel_colo<>.
struct CascIO {
  u32 deliver_at, cm_y, cm_z, cm_w, in_n, sp_n, special;     // per lane (node)
  u32 T, next_id, rounds, recv_sv, send_sv, stop;            // wave-uniform; stop = 1: round limit
};

template <bool ECHOBACK>
__device__ __attribute__((noinline)) CascIO cascade_lean(CascIO io, u32 off_inbox, uint4 *my_spill, u32 off_seen, u32 adj, u32 lane,
                                                        u32 my_cap, u32 my_spill_cap, u32 lat_us, u32 d2_in, u32 to_key, u32 *g_flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const my_inbox = reinterpret_cast<uint4 *>(smem + off_inbox);
  u32 *const my_seen = reinterpret_cast<u32 *>(smem + off_seen);
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  u32 deliver_at = io.deliver_at, cm_y = io.cm_y, cm_z = io.cm_z, cm_w = io.cm_w, in_n = io.in_n, sp_n = io.sp_n;
  bool special = io.special != 0;
  u32 T = (u32)__builtin_amdgcn_readfirstlane((int)io.T), next_id = (u32)__builtin_amdgcn_readfirstlane((int)io.next_id);
  u32 rounds = (u32)__builtin_amdgcn_readfirstlane((int)io.rounds), recv_sv = 0, send_sv = 0, stop = 0;
  const u32 d2 = (u32)__builtin_amdgcn_readfirstlane((int)d2_in);
  lat_us = (u32)__builtin_amdgcn_readfirstlane((int)lat_us);
  my_cap = (u32)__builtin_amdgcn_readfirstlane((int)my_cap); my_spill_cap = (u32)__builtin_amdgcn_readfirstlane((int)my_spill_cap);

  auto lds_push = [&](u32 x, u32 y, u32 z, u32 w) {
    if (in_n < my_cap) { my_inbox[in_n++] = make_uint4(x, y, z, w); return; }
    if (sp_n < my_spill_cap) { my_spill[sp_n++] = make_uint4(x, y, z, w); return; }
    atomicOr(g_flags, MSIM_FLAG_INBOX_OVERFLOW);
  };
  auto try_commit = [&](u32 x, u32 y, u32 z, u32 w) {
    cm_y = y; cm_z = z; cm_w = w;
    special = !((y & 0xFFu) == M_BROADCAST && (w & 0xFFFFFFu) == 0);
    if (lat_us == 0) deliver_at = T;
    else deliver_at = x <= T ? T : T + ((x - T) / 1000u) * 1000u;
  };

  for (;;) {
    bool due_now = deliver_at <= T;
    if (!__ballot(due_now)) {
      u32 k = deliver_at == INF ? INF : deliver_at * 2;
      k = min(k, to_key);
      const u32 km = __ballot(k != INF) ? wave_min(k) : INF;
      if (km == INF || (km & 1) || (km >> 1) >= d2) break;
      T = km >> 1;
      due_now = deliver_at <= T;
    }
    if (__ballot(due_now && special)) break;
    recv_sv += __popc((u32)__ballot(due_now));
    if (++rounds > ROUND_LIMIT) { stop = 1; break; }
    const u32 v = cm_z;
    u32 fan = 0;
    if (due_now) {
      deliver_at = INF;
      const u32 wv = my_seen[v >> 5], bitm = 1u << (v & 31);
      if (!(wv & bitm)) {
        my_seen[v >> 5] = wv | bitm;
        fan = ECHOBACK ? adj : (adj & ~(1u << (cm_w >> 24)));
      }
    }
    const u32 send = (u32)__ballot(fan != 0);
    bool got = false; u32 g_y = 0, g_z = 0, g_w = 0;
    const u32 in0 = in_n | sp_n;
    if (send) {
      const u32 cnt = __popc(fan);
      const u32 incl = scan32(cnt);
      const u32 pk = v | ((incl - cnt) << 16);
      u32 cand = adj & send;
      while (__ballot(cand != 0)) {
        const bool has = cand != 0;
        const u32 s = has ? (u32)__builtin_ctz(cand) : 0u;
        cand &= cand - 1;
        const u32 fs = lane_get(fan, s), ps = lane_get(pk, s);
        if (has && ((fs >> lane) & 1)) {
          const u32 y = ((next_id + (ps >> 16) + __popc(fs & lt32)) << 8) | M_BROADCAST;
          if (!got) { got = true; g_y = y; g_z = ps & 0xFFFFu; g_w = s << 24; }
          else lds_push(T + lat_us, y, ps & 0xFFFFu, s << 24);
        }
      }
      const u32 total = rdlane(incl, 31);
      next_id += total; send_sv += total;
    }
    if (got) {
      if (deliver_at == INF && in0 == 0) try_commit(T + lat_us, g_y, g_z, g_w); else lds_push(T + lat_us, g_y, g_z, g_w);
    }
    if (__ballot(deliver_at == INF && (in_n | sp_n) != 0)) {
      if (deliver_at == INF && (in_n | sp_n) != 0) {   // idle with a queue: recv! takes the minimum (deadline, id)
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
        try_commit(e.x, e.y, e.z, e.w);
      }
    }
  }
  io.deliver_at = deliver_at; io.cm_y = cm_y; io.cm_z = cm_z; io.cm_w = cm_w; io.in_n = in_n; io.sp_n = sp_n; io.special = special ? 1u : 0u;
  io.T = T; io.next_id = next_id; io.rounds = rounds; io.recv_sv = recv_sv; io.send_sv = send_sv; io.stop = stop;
  return io;  // by value both ways: the state travels in registers, not through scratch memory
}

// Wavefronts per SIMD the register budget is cut for.  Four (128 registers) left 16-232 B of private memory per lane in the round loops of
// most instantiations (tools/private_memory_audit.py) — a memory round trip per round; three (168) leaves none, and a cluster's LDS
// keeps a SIMD at two or three wavefronts anyway.
#ifndef COLO_MIN_WAVES
#define COLO_MIN_WAVES 3
#endif
template <int PROG, bool NEM, bool NET_RANDOM, bool QFIFO>
__global__ void __launch_bounds__(64, COLO_MIN_WAVES) sim_kernel_colo(const KParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  u32 *const seen = reinterpret_cast<u32 *>(smem + p.off_seen);
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  constexpr bool IS_BCAST = PROG >= MSIM_NODE_BCAST_FF && PROG <= MSIM_NODE_BCAST_RPC_ALL;
  constexpr bool IS_RPC = PROG == MSIM_NODE_BCAST_ACK_RETRY || PROG == MSIM_NODE_BCAST_RPC_ALL;
  constexpr bool IS_ACK = PROG == MSIM_NODE_BCAST_ACK_RETRY;
  constexpr bool IS_PN = PROG == MSIM_NODE_PN_COUNTER;    // pn_counter.rb: same replication skeleton as g-set, counters instead of a set
  constexpr bool IS_GSET = PROG == MSIM_NODE_G_SET || IS_PN;  // "CRDT with a 5 s replicate timer"
  constexpr bool IS_ECHO = PROG == MSIM_NODE_ECHO;
  constexpr bool IS_FLAKE = PROG == MSIM_NODE_FLAKE_IDS;  // flake_ids.clj: unique-ids workload, Reusable clients (unique_ids.clj:59-61)
  constexpr bool HAS_FINAL = IS_BCAST || IS_GSET;
  constexpr bool FINAL_FLAG = IS_BCAST || IS_PN;  // :final? true on the last reads (broadcast.clj:240, pn_counter.clj:137)
  constexpr bool HAS_TIMERS = IS_ACK || IS_GSET;
  constexpr bool REP_FIRST = IS_ACK;
  constexpr u32 FAN_TYPE = IS_GSET ? M_REPLICATE : M_BROADCAST;
  constexpr bool TOPO_BOUND = PROG == MSIM_NODE_BCAST_FF || PROG == MSIM_NODE_BCAST_FF_ECHOBACK || IS_ACK;
  constexpr bool FAST_OK = PROG == MSIM_NODE_BCAST_FF || PROG == MSIM_NODE_BCAST_FF_ECHOBACK;
  constexpr bool LEAN = !NET_RANDOM;
  // FIFO queues need a receiver's arrivals in key order inside one COMMIT: fan-outs are pulled in sender order; the acknowledged programs'
  // node -> node replies are taken in by the same loop (commit_fan: a sender's reply and its fan-out go to different nodes, so "sender
  // order" is id order at every receiver)
  constexpr bool FIFO = QFIFO && LEAN;  // chosen by the host when deep queues are expected (queue scans dominate then)

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, W = p.W;  // C == CS == N in this layout
  const bool is_node = lane < N;  // = "this lane is endpoint pair (node lane, client N+lane)"
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u32 all_nodes = N >= 32 ? 0xFFFFFFFFu : ((1u << N) - 1);
  const u32 max_values = p.cfg.max_values, max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz;
  const u32 lat_us = lat_mean * 1000u;

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const g_unacked = g_scr + (size_t)lane * max_values;
  u32 *const g_fifo = g_scr + (size_t)N * max_values + (size_t)lane * max_values * 2;

  const u32 jcap = p.cfg.journal_capacity;  // net journal (journal.clj:53,220-239); 0 = off
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;
  const u32 my_cap = p.cap_node;
  uint4 *const my_inbox = inbox + (is_node ? lane : 0) * p.cap_node;                                        // node queue
  uint4 *const my_cinbox = inbox + N * p.cap_node + (is_node ? lane : 0) * CLIENT_INBOX_CAP;                // client queue
  const u32 my_spill_cap = p.spill_cap;
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)(is_node ? lane : 0) * p.spill_cap;  // HBM spill
  u32 *const my_seen = seen + (is_node ? lane : 0) * W;

  for (u32 i = lane; i < N * W; i += 64) seen[i] = 0;
  if (IS_ACK) { if (is_node) for (u32 v = 0; v < max_values; v++) g_unacked[v] = 0; }
  __syncthreads();

  const u32 adj = is_node ? topo_adj(p.cfg.topology, N, lane) : 0;
  const u32 cand_all = is_node ? (TOPO_BOUND ? adj : (all_nodes & ~(1u << lane))) : 0u;
  const u32 my_client = N + lane;  // endpoint index of this lane's client

  // ---- node state ----
  u32 deliver_at = INF;                       // INF = recv! holds no envelope
  uint4 cm = make_uint4(0, 0, 0, 0);          // the envelope recv! is sleeping on
  bool special = false;                       // cm is not plain gossip (cascade loop must leave it to the general round)
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0;
  // LEAN (constant latency, no loss): server envelopes reach a node in key order, so its queue is a FIFO ring
  // (LDS ring [f_head, f_head+in_n), then the HBM spill ring [s_head, s_head+sp_n)); the one client request a node
  // can have pending sits in `creq`.  poll is O(1) instead of a scan.
  u32 f_head = 0, s_head = 0; bool have_creq = false, pm_direct = false; uint4 creq = make_uint4(0, 0, 0, 0);
  u32 sph_x = 0, sph_y = 0, sph_z = 0, sph_w = 0;   // FIFO: the spill ring's head envelope, fetched when it BECAME the head — a poll never waits for HBM (four words, not a uint4: that one ended up in private memory)
  u32 node_msgid = 0, timer_next = INF, tick = 0, part = 0;
  u32 flake_time = 0, flake_count = 0;  // flake_ids.clj:10-14
  // the retry FIFO of the acknowledged gossip (value, wake time; in HBM): its head — value rt_v, wake time retry_time, who has not
  // acknowledged rt_un — and the entry behind it (rt_v2, rt_t2) are kept in registers, fetched when they MOVED UP, so that a wake-up
  // waits for nothing; acknowledgements of the head's value clear their bit in rt_un as well as at the L2
  u32 fifo_head = 0, fifo_tail = 0, retry_time = INF, rt_v = 0, rt_un = 0, rt_v2 = 0, rt_t2 = 0;
  u32 fifo_hi = 0, fifo_ti = 0;   // (fifo_head / fifo_tail modulo max_values: the ring's slots, kept by compare-and-wrap — a division by a run-time value is forty instructions)
  // ---- client state (slot = lane) ----
  bool busy = false; u32 kind = K_NONE;
  // the msg_id a busy client waits for is its latest one (client.clj:61-64): no separate register
  u32 timeout_at = 0, next_msg_id = 0, c_f = 0, c_value = 0, process = lane, c_final = 0;
  u32 cin_n = 0;
  // net stats are cluster totals: wave-uniform accumulators fed by ballots (SALU), not per-lane counters.
  // Overflow flags are raised on rare paths only: they go straight to a word of the instance's meta record.
  u32 t_send_cl = 0, t_send_sv = 0, t_recv_cl = 0, t_recv_sv = 0;
  u32 *const g_flags = &p.meta[inst].reserved[0];
  if (lane == 0) *g_flags = 0;
  auto raise = [&](u32 bit) { atomicOr(g_flags, bit); };
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, next_value = 0, nem_next = 0, nem_j = 0;
  u32 sleep_until = 0, loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;  // journal cursor; :send events of a COMMIT sit at ev_base + (id - id_base)

  auto jwrite = [&](u32 idx, u32 recv, u32 y, u32 a, u32 b, u32 src, u32 dest) {
    if (idx < jcap) g_ev[idx] = make_uint4(T, (y & ~0x80u) | (recv << 7), a, src | (dest << 8) | ((b & 0xFFFFu) << 16));
    else raise(MSIM_FLAG_JOURNAL_OVERFLOW);
  };
  // a gossip task (value v, to be woken at `when`, `un` = who has not acknowledged) joins the retry FIFO
  auto retry_push = [&](u32 v, u32 when, u32 un) {
    const u32 ts = fifo_ti * 2, n = fifo_tail - fifo_head;
    g_fifo[ts] = v; g_fifo[ts + 1] = when;
    fifo_ti = fifo_ti + 1 == max_values ? 0u : fifo_ti + 1;
    if (n == 0) { rt_v = v; retry_time = when; rt_un = un; }
    else if (n == 1) { rt_v2 = v; rt_t2 = when; }
    fifo_tail++;
  };
  // the head wakes: returns its value and who has not acknowledged it; the entry behind it moves up
  auto retry_pop = [&](u32 &v, u32 &un) {
    v = rt_v; un = rt_un;
    fifo_head++; fifo_hi = fifo_hi + 1 == max_values ? 0u : fifo_hi + 1;
    const u32 n = fifo_tail - fifo_head;
    if (n == 0) { retry_time = INF; return; }
    rt_v = rt_v2; retry_time = rt_t2;
    rt_un = __hip_atomic_load(&g_unacked[rt_v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (acknowledgements clear their bits with atomics at the L2)
    if (n >= 2) { const u32 i2 = fifo_hi + 1 == max_values ? 0u : fifo_hi + 1; const uint2 nh = *reinterpret_cast<const uint2 *>(&g_fifo[i2 * 2]); rt_v2 = nh.x; rt_t2 = nh.y; }
  };
  auto retry_ack = [&](u32 v, u32 src) {   // unacked.delete dest: no value returned, nobody waits for HBM
    atomicAnd(&g_unacked[v], ~(1u << src));
    if (fifo_head != fifo_tail && v == rt_v) rt_un &= ~(1u << src);
  };
  auto lds_push = [&](const uint4 m) {
    if (FIFO) {  // once something spilled, later envelopes must queue behind it
      if (sp_n == 0 && in_n < my_cap) { u32 i = f_head + in_n; if (i >= my_cap) i -= my_cap; my_inbox[i] = m; in_n++; return; }
      if (sp_n < my_spill_cap) { u32 i = s_head + sp_n; if (i >= my_spill_cap) i -= my_spill_cap; my_spill[i] = m; if (sp_n == 0) { sph_x = m.x; sph_y = m.y; sph_z = m.z; sph_w = m.w; } sp_n++; return; }
      raise(MSIM_FLAG_INBOX_OVERFLOW); return;
    }
    if (in_n < my_cap) { my_inbox[in_n++] = m; return; }
    if (sp_n < my_spill_cap) { my_spill[sp_n++] = m; return; }
    raise(MSIM_FLAG_INBOX_OVERFLOW);
  };
  auto try_commit = [&](const uint4 e) {
    const u32 src = e.w >> 24;
    if (NEM && src < N && ((part >> src) & 1)) return;  // partitioned: dropped, no :recv (net.clj:234)
    cm = e;
    if (IS_RPC) special = !(src < N && ((e.y & 0xFFu) == M_BROADCAST || (e.y & 0xFFu) == M_BROADCAST_OK));   // (anything a client is part of needs the general round)
    else special = !((e.y & 0xFFu) == M_BROADCAST && (e.w & 0xFFFFFFu) == 0);
    // (Thread/sleep (long dt)) net.clj:236-238; with zero latency every deadline has already passed when it is polled
    if (LEAN && lat_us == 0) deliver_at = T;
    else deliver_at = e.x <= T ? T : T + ((e.x - T) / 1000u) * 1000u;
  };
  // an envelope for THIS lane's node arrives (net.clj:189-221)
  auto arrive = [&](u32 id, u32 type, u32 a, u32 b, u32 src) {
    u32 lat = 0;
    if (src < N) {
      if (LEAN || lat_dist == MSIM_LAT_CONSTANT) lat = lat_mean;
      else if (lat_dist == MSIM_LAT_UNIFORM) lat = scale32(draw32(key, S_LATENCY, id), 2 * lat_mean);
      else lat = (u32)(((u64)lat_mean * neg_ln_q16(draw32(key, S_LATENCY, id))) >> 16);
    }
    if (jcap) jwrite(ev_base + (id - id_base), 0, (id << 8) | type, a, b, src, lane);  // :send precedes the loss decision (net.clj:208)
    if (NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss) return;
    uint4 m = make_uint4(T + lat * 1000u, (id << 8) | type, a, b | (src << 24));
    if (FIFO) {
      if (src >= N) {  // the request of this lane's own client: at most one can be pending
        if (have_creq) raise(MSIM_FLAG_INBOX_OVERFLOW);
        creq = m; have_creq = true; return;
      }
      if (!have_pm) {  // first server envelope of this COMMIT: it may be committed straight from registers
        pm = m; have_pm = true; pm_direct = deliver_at == INF && (in_n | sp_n) == 0 && !have_creq; return;
      }
      if (!pm_direct && pm.y != 0) { lds_push(pm); pm.y = 0; }  // keep arrival order: pm first
      lds_push(m); return;
    }
    if (!have_pm) { pm = m; have_pm = true; return; }
    if (m.x < pm.x || (m.x == pm.x && m.y < pm.y)) { const uint4 t = m; m = pm; pm = t; }
    lds_push(m);
  };
  // the node's recv! polls (net.clj:223-247)
  auto poll = [&]() {
    if (FIFO) {
      if (have_pm) {
        have_pm = false;
        if (pm.y != 0) { if (pm_direct) try_commit(pm); else lds_push(pm); }
      }
      while (is_node && deliver_at == INF && ((in_n | sp_n) != 0 || have_creq)) {
        uint4 h = make_uint4(INF, INF, 0, 0);
        if (in_n) h = my_inbox[f_head]; else if (sp_n) h = make_uint4(sph_x, sph_y, sph_z, sph_w);
        if (have_creq && (creq.x < h.x || (creq.x == h.x && creq.y < h.y))) { have_creq = false; try_commit(creq); continue; }
        if (in_n) { in_n--; f_head++; if (f_head >= my_cap) f_head = 0; }
        else { sp_n--; s_head++; if (s_head >= my_spill_cap) s_head = 0; if (sp_n) { const uint4 nx = my_spill[s_head]; sph_x = nx.x; sph_y = nx.y; sph_z = nx.z; sph_w = nx.w; } }   // (the next head: needed a round from now at the earliest)
        try_commit(h);
      }
      return;
    }
    if (have_pm) {
      have_pm = false;
      if (is_node && deliver_at == INF && (in_n | sp_n) == 0) try_commit(pm);
      else lds_push(pm);
    }
    while (is_node && deliver_at == INF && (in_n | sp_n) != 0) {
      u32 best = 0; bool in_spill = false;
      u64 bk = ~0ull;  // (deadline, id << 8 | type) as one 64-bit key: ids are unique, so the type bits never decide
      for (u32 i = 0; i < in_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_inbox[i]);
        const u64 k = ((u64)kk.x << 32) | kk.y;
        if (k < bk) { bk = k; best = i; }
      }
      spill_min(my_spill, sp_n, bk, best, in_spill);  // deep queues only (long head-of-line sleeps)
      uint4 e;
      if (in_spill) { e = my_spill[best]; sp_n--; if (best != sp_n) my_spill[best] = my_spill[sp_n]; }
      else { e = my_inbox[best]; in_n--; if (best != in_n) my_inbox[best] = my_inbox[in_n]; }
      try_commit(e);
    }
  };
  // receiver-side COMMIT of fan-outs (see sim_kernel<>)
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
      if (IS_RPC) bs = lane_get(fan_b0, s);
      if (has && ((fs >> lane) & 1)) {
        const u32 rank = __popc(fs & lt32);
        arrive(next_id + os + rank, FAN_TYPE, as, IS_RPC ? bs + rank : 0u, s);
      }
    }
  };
  // the acknowledged programs: fan-outs AND node -> node replies (rp_pack = addressee | type << 8 | 1 << 31, or 0), every receiver
  // walking its possible senders in ascending order — a receiver's arrivals are then in id order (FIFO queues)
  auto commit_fan_rpc = [&](u32 fan_mask, u32 fan_a, u32 fan_b0, u32 id_off, u32 rp_pack, u32 rp_a, u32 rp_b, u32 rp_off) {
    const u32 send = (u32)__ballot(fan_mask != 0 || rp_pack != 0);
    u32 cand = cand_all & send;
    while (__ballot(cand != 0)) {
      const bool has = cand != 0;
      const u32 s = has ? (u32)__builtin_ctz(cand) : 0u;
      cand &= cand - 1;
      const u32 fs = lane_get(fan_mask, s), as = lane_get(fan_a, s), os = lane_get(id_off, s), bs = lane_get(fan_b0, s);
      const u32 pk = lane_get(rp_pack, s), ra = lane_get(rp_a, s), rb = lane_get(rp_b, s), ro = lane_get(rp_off, s);
      if (has && ((fs >> lane) & 1)) {
        const u32 rank = __popc(fs & lt32);
        arrive(next_id + os + rank, FAN_TYPE, as, bs + rank, s);
      } else if (has && (pk >> 31) && (pk & 0xFFu) == lane) arrive(next_id + ro, (pk >> 8) & 0xFFu, ra, rb, s);
    }
  };

  bool fast = false; u32 d2 = INF;  // cascade mode (set at the end of a general round), scheduler's next action time
  constexpr bool QUIET_OK = FAST_OK && LEAN && !FIFO && !NEM;
  bool skip_quiet = false;  // quiet_run<> just handed a round back: the loop below must take it
  QuietK qk;
  if (QUIET_OK) {
    qk.key = key; qk.g_rows = g_rows; qk.g_pay = g_pay; qk.my_spill = my_spill; qk.g_flags = g_flags;
    qk.off_inbox = (u32)(reinterpret_cast<unsigned char *>(my_inbox) - smem); qk.off_seen = (u32)(reinterpret_cast<unsigned char *>(my_seen) - smem);
    qk.off_seen_all = (u32)(reinterpret_cast<unsigned char *>(seen) - smem); qk.W = W; qk.adj = adj; qk.lane = lane; qk.N = N;
    qk.my_cap = my_cap; qk.my_spill_cap = my_spill_cap; qk.lat_us = lat_us; qk.cutoff = 0; qk.gen_period2_us = p.gen_period2_us;
    qk.max_rows = max_rows; qk.max_pay = max_pay; qk.max_values = max_values; qk.all_nodes = all_nodes;
  }
#ifdef COLO_PROF   // developer build (tools/variant_lib.sh cprof k_general_c.hip -DCOLO_PROF; tools/colo_prof_report.py): cycles of a wavefront by kind of round
  u64 cpc[6] = {0, 0, 0, 0, 0, 0}, cp_t = __builtin_readcyclecounter(); u32 cp_fast = 0;
#define CP_MARK(i_) { const u64 cp_n = __builtin_readcyclecounter(); cpc[i_] += cp_n - cp_t; cp_t = cp_n; }
#else
#define CP_MARK(i_)
#endif
  for (;;) {
    CP_MARK(4)   // [4] = everything that is not a gossip round of the acknowledged programs
    // the pending-arrival register is dead between rounds: say so, or it is carried around every loop
    forget(pm); have_pm = false;
    // ---- quiet stretches (lone client operations + their gossip cascades) run in quiet_run<> ----
    if (QUIET_OK && !skip_quiet && !jcap && phase == PH_MAIN && rate > 0 && !(p.dev_flags & 4) &&
        !__ballot(busy || (is_node && (sp_n != 0 || in_n + __popc(adj) > my_cap)))) {   // (quiet_run<> needs room for a round of arrivals in LDS)
      QuietIO io;
      io.deliver_at = deliver_at; io.cm_y = cm.y; io.cm_z = cm.z; io.cm_w = cm.w; io.in_n = in_n; io.sp_n = sp_n; io.special = special ? 1u : 0u;
      io.process = process; io.next_msg_id = next_msg_id; io.c_f = c_f; io.c_value = c_value; io.did_op = 0;
      io.T = T; io.next_id = next_id; io.rounds = rounds; io.n_rows = n_rows; io.n_payload = n_payload; io.gen_k = gen_k; io.gen_next = gen_next;
      io.next_value = next_value; io.send_cl = 0; io.recv_cl = 0; io.send_sv = 0; io.recv_sv = 0; io.fast = fast ? 1u : 0u; io.d2 = d2; io.stop = 0;
      qk.cutoff = cutoff;
      quiet_run<PROG == MSIM_NODE_BCAST_FF_ECHOBACK>(io, qk, cin_n);
      deliver_at = io.deliver_at; cm.y = io.cm_y; cm.z = io.cm_z; cm.w = io.cm_w; in_n = io.in_n; sp_n = io.sp_n; special = io.special != 0;
      process = io.process; next_msg_id = io.next_msg_id; c_f = io.c_f; c_value = io.c_value;
      if (io.did_op) { kind = K_OP; c_final = 0; }
      T = rdlane(io.T, 0); next_id = rdlane(io.next_id, 0); rounds = rdlane(io.rounds, 0); n_rows = rdlane(io.n_rows, 0); n_payload = rdlane(io.n_payload, 0);
      gen_k = rdlane(io.gen_k, 0); gen_next = rdlane(io.gen_next, 0); next_value = rdlane(io.next_value, 0);
      t_send_cl += rdlane(io.send_cl, 0); t_recv_cl += rdlane(io.recv_cl, 0); t_send_sv += rdlane(io.send_sv, 0); t_recv_sv += rdlane(io.recv_sv, 0);
      fast = rdlane(io.fast, 0) != 0; d2 = rdlane(io.d2, 0);
      if (rdlane(io.stop, 0)) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
      skip_quiet = true;
      continue;
    }
    // ---- cascade rounds (plain gossip while the scheduler is quiet at T): same loop, short body ----
    if (FAST_OK && fast && LEAN && !FIFO && !NEM && !jcap && !(p.dev_flags & 1)) {
      // the headline case runs its cascade rounds in cascade_lean<> (see there): state out, rounds, state back in
      CascIO io;
      io.deliver_at = deliver_at; io.cm_y = cm.y; io.cm_z = cm.z; io.cm_w = cm.w; io.in_n = in_n; io.sp_n = sp_n; io.special = special ? 1u : 0u;
      io.T = T; io.next_id = next_id; io.rounds = rounds; io.recv_sv = 0; io.send_sv = 0; io.stop = 0;
      io = cascade_lean<PROG == MSIM_NODE_BCAST_FF_ECHOBACK>(io, (u32)(reinterpret_cast<unsigned char *>(my_inbox) - smem), my_spill,
                                                       (u32)(reinterpret_cast<unsigned char *>(my_seen) - smem), adj, lane, my_cap, my_spill_cap, lat_us, d2,
                                                       busy ? timeout_at * 2 + 1 : INF, g_flags);
      deliver_at = io.deliver_at; cm.y = io.cm_y; cm.z = io.cm_z; cm.w = io.cm_w; in_n = io.in_n; sp_n = io.sp_n; special = io.special != 0;
      T = rdlane(io.T, 0); next_id = rdlane(io.next_id, 0); rounds = rdlane(io.rounds, 0);
      t_recv_sv += rdlane(io.recv_sv, 0); t_send_sv += rdlane(io.send_sv, 0);
      if (rdlane(io.stop, 0)) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
      fast = false;
      continue;
    }
    // ---- gossip rounds of the acknowledged programs (02-performance.md:406-441 / broadcast.rb:29-47) while the scheduler is quiet: only
    //      nodes talk to nodes — gossip, acknowledgements, the retry timer — so R3 and its COMMIT are all there is to a round; the
    //      general round below (scheduler, clients, rows: ~10 000 cycles) takes everything else.  Under partitions this variant is
    //      ~70 000 rounds per cluster, nearly all of this kind. ----
    if (IS_RPC && fast) {
      u32 my_t = is_node ? deliver_at : INF;
      if (IS_ACK && is_node) my_t = min(my_t, retry_time);
      bool due_now = my_t <= T;
      if (!__ballot(due_now)) {
        u32 k = my_t == INF ? INF : my_t * 2;
        if (busy) k = min(k, timeout_at * 2 + 1);
        const u32 km = __ballot(k != INF) ? wave_min(k) : INF;
        if (km == INF || (km & 1) || (km >> 1) >= d2) { fast = false; continue; }
        T = km >> 1;
        due_now = my_t <= T;
      }
      const bool waking = IS_ACK && is_node && retry_time <= T;       // (the timer comes first, as in the general round)
      const bool delivering = is_node && !waking && deliver_at <= T;
      if (__ballot(delivering && special)) { fast = false; continue; }
      if (++rounds > ROUND_LIMIT) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
      CP_MARK(0)   // [0] = gossip round: time
      const u32 dm = (u32)__ballot(delivering);
      t_recv_sv += __popc(dm);
      u32 fan_mask = 0, fan_a = 0, fan_b0 = 0;
      bool rep = false; u32 rep_dest = 0, rep_a = 0, rep_b = 0;
      if (waking) {
        u32 v, un;
        retry_pop(v, un);
        if (un) { fan_mask = un; fan_a = v; fan_b0 = node_msgid + 1; node_msgid += __popc(un); retry_push(v, T + 1000000u, un); }
      } else if (delivering) {
        const uint4 q = cm; deliver_at = INF;
        const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qa = q.z;
        if (jcap) jwrite(n_ev + __popc(dm & lt32), 1, q.y, qa, qb, qsrc, lane);
        if ((q.y & 0xFFu) == M_BROADCAST) {
          const u32 bitm = 1u << (qa & 31), wv = my_seen[qa >> 5];
          if (!(wv & bitm)) {
            my_seen[qa >> 5] = wv | bitm;
            const u32 tg = (PROG == MSIM_NODE_BCAST_RPC_ALL ? (all_nodes & ~(1u << lane)) : adj) & ~(1u << qsrc);
            fan_mask = tg; fan_a = qa; fan_b0 = node_msgid + 1; node_msgid += __popc(tg);
            if (IS_ACK && tg) { __hip_atomic_store(&g_unacked[qa], tg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); retry_push(qa, T + 1000000u, tg); }   // (see the general round's copy of this line)
          }
          if (qb != 0) { rep = true; rep_dest = qsrc; rep_a = qa; rep_b = qb; }
        } else if (IS_ACK) retry_ack(qa, qsrc);   // M_BROADCAST_OK
      }
      if (jcap) n_ev += __popc(dm);
      CP_MARK(1)   // [1] = gossip round: the wake-ups and deliveries
      {
        const u32 fan_cnt = __popc(fan_mask), cnt = fan_cnt + (rep ? 1u : 0u);
        if (__ballot(cnt != 0)) {
          const u32 incl = scan32(cnt), total = rdlane(incl, 31);
          ev_base = n_ev; id_base = next_id; n_ev += total;
          t_send_sv += total;
          commit_fan_rpc(fan_mask, fan_a, fan_b0, incl - cnt + ((REP_FIRST && rep) ? 1u : 0u), rep ? (0x80000000u | rep_dest | ((u32)M_BROADCAST_OK << 8)) : 0u, rep_a, rep_b,
                         incl - cnt + (REP_FIRST ? 0u : fan_cnt));
          next_id += total;
        }
        CP_MARK(2)   // [2] = gossip round: COMMIT
        poll();
        CP_MARK(3)   // [3] = gossip round: polls
      }
#ifdef COLO_PROF
      cp_fast++;
#endif
      continue;
    }
    if (FAST_OK && fast) {
      bool due_now = deliver_at <= T;
      if (!__ballot(due_now)) {
        // R0 inside the loop: jump to the next delivery if it precedes the scheduler and every client timeout
        u32 k = deliver_at == INF ? INF : deliver_at * 2;
        if (busy) k = min(k, timeout_at * 2 + 1);
        const u32 km = __ballot(k != INF) ? wave_min(k) : INF;
        if (km == INF || (km & 1) || (km >> 1) >= d2) { fast = false; continue; }
        T = km >> 1;
        due_now = deliver_at <= T;
      }
      if (__ballot(due_now && special)) { fast = false; continue; }
      t_recv_sv += __popc((u32)__ballot(due_now));
      if (++rounds > ROUND_LIMIT) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
      const u32 v = cm.z;
      u32 fan = 0;
      if (jcap) {
        const u32 dmj = (u32)__ballot(due_now);
        if (due_now) jwrite(n_ev + __popc(dmj & lt32), 1, cm.y, v, 0, cm.w >> 24, lane);
        n_ev += __popc(dmj);
      }
      if (due_now) {
        deliver_at = INF;
        const u32 wv = my_seen[v >> 5], bitm = 1u << (v & 31);
        if (!(wv & bitm)) {
          my_seen[v >> 5] = wv | bitm;
          fan = PROG == MSIM_NODE_BCAST_FF_ECHOBACK ? adj : (adj & ~(1u << (cm.w >> 24)));
        }
      }
      const u32 send = (u32)__ballot(fan != 0);
      if (FIFO) {
        // all arrivals share the deadline T+lat and come in id order: FIFO push, first one possibly straight to recv!
        if (send) {
          const u32 cnt = __popc(fan);
          const u32 incl = scan32(cnt);
          const u32 pk = v | ((incl - cnt) << 16);
          ev_base = n_ev; n_ev += rdlane(incl, 31);
          u32 cand = adj & send;
          while (__ballot(cand != 0)) {
            const bool has = cand != 0;
            const u32 s = has ? (u32)__builtin_ctz(cand) : 0u;
            cand &= cand - 1;
            const u32 fs = lane_get(fan, s), ps = lane_get(pk, s);
            if (has && ((fs >> lane) & 1)) {
              const u32 y = ((next_id + (ps >> 16) + __popc(fs & lt32)) << 8) | M_BROADCAST;
              if (jcap) jwrite(ev_base + (ps >> 16) + __popc(fs & lt32), 0, y, ps & 0xFFFFu, 0, s, lane);
              const uint4 m = make_uint4(T + lat_us, y, ps & 0xFFFFu, s << 24);
              if (!have_pm) { pm = m; have_pm = true; pm_direct = deliver_at == INF && (in_n | sp_n) == 0 && !have_creq; }
              else { if (!pm_direct && pm.y != 0) { lds_push(pm); pm.y = 0; } lds_push(m); }
            }
          }
          next_id += rdlane(incl, 31); t_send_sv += rdlane(incl, 31);
        }
        if (__ballot(have_pm || (deliver_at == INF && ((in_n | sp_n) != 0 || have_creq)))) poll();
      } else if (LEAN) {
        // all arrivals share the deadline T+lat and come in id order: the first one is the queue minimum.  It is kept in
        // registers and committed ONCE after the loop: instructions inside the sender loop issue for the whole wave every
        // iteration, whatever the number of lanes that need them
        bool got = false; u32 g_y = 0, g_z = 0, g_w = 0;
        const u32 in0 = in_n | sp_n;
        if (send) {
          const u32 cnt = __popc(fan);
          const u32 incl = scan32(cnt);
          const u32 pk = v | ((incl - cnt) << 16);
          ev_base = n_ev; n_ev += rdlane(incl, 31);
          u32 cand = adj & send;
          while (__ballot(cand != 0)) {
            const bool has = cand != 0;
            const u32 s = has ? (u32)__builtin_ctz(cand) : 0u;
            cand &= cand - 1;
            const u32 fs = lane_get(fan, s), ps = lane_get(pk, s);
            if (has && ((fs >> lane) & 1)) {
              const u32 y = ((next_id + (ps >> 16) + __popc(fs & lt32)) << 8) | M_BROADCAST;
              if (jcap) jwrite(ev_base + (ps >> 16) + __popc(fs & lt32), 0, y, ps & 0xFFFFu, 0, s, lane);
              if (!got) { got = true; g_y = y; g_z = ps & 0xFFFFu; g_w = s << 24; }
              else lds_push(make_uint4(T + lat_us, y, ps & 0xFFFFu, s << 24));
            }
          }
          next_id += rdlane(incl, 31); t_send_sv += rdlane(incl, 31);
        }
        if (got) {
          const uint4 e = make_uint4(T + lat_us, g_y, g_z, g_w);
          if (deliver_at == INF && in0 == 0) try_commit(e); else lds_push(e);
        }
        if (__ballot(deliver_at == INF && (in_n | sp_n) != 0)) poll();
      } else {
        if (send) {
          const u32 cnt = __popc(fan);
          const u32 incl = scan32(cnt);
          ev_base = n_ev; id_base = next_id; n_ev += rdlane(incl, 31);
          commit_fan(fan, v, 0, incl - cnt);
          next_id += rdlane(incl, 31); t_send_sv += rdlane(incl, 31);
        }
        poll();
      }
      continue;
    }
    const u32 busy_mask = (u32)__ballot(busy);

    // ---- time-free phase transitions ----
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
            if (busy_mask) break;
            phase = (NEM && HAS_FINAL) ? PH_NEM_FINAL : HAS_FINAL ? PH_SLEEP : PH_DONE;
            if (phase == PH_SLEEP) sleep_until = T + p.cfg.quiesce_ms * 1000u;
            again = true; break;
          case PH_FINAL_WAIT: if (!busy_mask) { phase = PH_DONE; again = true; } break;
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
      case PH_INIT: case PH_TOPO: case PH_NEM_FINAL: case PH_FINAL: due = T; break;
      case PH_SLEEP: due = sleep_until; break;
      case PH_MAIN:
        if (nem_live) due = max(nem_next, T);
        if (gen_live && free_mask) due = min(due, max(gen_next, T));
        if (rate == 0 && !nem_live) due = min(due, cutoff);
        break;
      default: break;
    }
    u32 my_t = deliver_at;
    if (HAS_TIMERS) my_t = min(my_t, min(timer_next, retry_time));
    bool timeout_round = false;
    if (due > T && !__ballot(my_t <= T)) {
      u32 k = my_t == INF ? INF : my_t * 2;
      if (busy) k = min(k, timeout_at * 2 + 1);
      u32 km = __ballot(k != INF) ? wave_min(k) : INF;  // a fully idle cluster (the usual state between operations) has nothing to reduce
      if (due != INF) km = min(km, due * 2);
      if (km == INF) { flags |= MSIM_FLAG_ROUND_LIMIT; break; }
      timeout_round = (km & 1) != 0;
      T = max(T, km >> 1);
    }

    bool mark = false; u32 m_f = 0, m_value = 0, m_final = 0;  // R1 -> R2 of the same round
    bool inv_row = false; u32 inv_packed = 0, inv_value = 0;
    bool cmp_row = false; u32 cmp_packed = 0, cmp_value = 0, cmp_len = 0;
    u32 nem_rows = 0, nem_f = 0, nem_v1 = 0, nem_v2 = 0, nem_len2 = 0;

    auto complete = [&](u32 type, u32 err, u32 value, u32 len) {
      busy = false;
      if (kind != K_OP) { if (type != MSIM_T_OK) raise(MSIM_FLAG_ROUND_LIMIT); return; }
      cmp_row = true; cmp_packed = type | (c_f << 2) | (err << 7) | (c_final << 11) | (process << 12);
      cmp_value = value; cmp_len = len;
      if (type == MSIM_T_INFO) { process += N; if (!IS_FLAKE) { next_msg_id = 0; cin_n = 0; } }  // crashed process; fresh client unless Reusable
    };
    // the client's recv! consumes one envelope (client.clj:94-107)
    auto client_deliver = [&](u32 qtype, u32 qa, u32 qb) {
      if (busy && qb == next_msg_id) {
        if (qtype == M_READ_OK) { if (IS_PN) complete(MSIM_T_OK, 0, qa, 0); else complete(MSIM_T_OK, 0, qa & 0xFFFFFFu, qa >> 24); }
        else if (qtype == M_ECHO_OK || qtype == M_GENERATE_OK) complete(MSIM_T_OK, 0, qa, 0);
        else complete(MSIM_T_OK, 0, c_value, 0);
      }
    };

    // ---- a lone client operation on a quiet cluster (most generator events at low latency): the same round — R1 picks
    //      the worker, R2 its request reaches its own node (lane-local, no latency), R3 the idle node handles it at once
    //      and its reply completes the operation in R4 — with nothing else due.  Identical ids, rows, payload and
    //      counters as the general path below, which still takes every round this does not fit. ----
    bool lone_op = false;
    if (FAST_OK && LEAN && !timeout_round && due <= T && phase == PH_MAIN && gen_live && gen_next <= T && free_mask &&
        !(NEM && nem_live && nem_next <= T) && !jcap && !(p.dev_flags & 2) && !__ballot(is_node && deliver_at <= T)) {
      const u32 nfree = __popc(free_mask);
      const u32 kk = gen_k;
      const u64 h = draw64(key, S_GEN, kk);
      const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
      const u32 pick = scale32(r_lo, nfree);
      const bool sel = is_node && !busy && (u32)__popc(free_mask & lt32) == pick;
      const bool rd_op = (r_lo & 1) != 0;
      const u32 words = (next_value + 31) >> 5;
      const bool fits = rd_op ? n_payload + words <= max_pay : next_value < max_values;
      // the worker's node must be idle with nothing queued, its client must have no stale reply waiting
      if (fits && __ballot(sel && deliver_at == INF && (in_n | sp_n) == 0 && cin_n == 0)) {
        lone_op = true;
        gen_k++;
        const u32 sl = (u32)__builtin_ctz((u32)__ballot(sel));
        const u32 f = rd_op ? MSIM_F_READ : MSIM_F_BROADCAST;
        const u32 val = rd_op ? MSIM_NO_VALUE : next_value;
        if (!rd_op) next_value++;
        const u32 base = next_id + 1;                                          // ids of the node's own sends (the request took next_id)
        const u32 fan_s = rd_op ? 0u : rdlane(adj, sl);                        // a client is no neighbour: nothing to skip
        const u32 cnt = __popc(fan_s);
        u32 off = 0;
        if (rd_op) {
          __syncthreads();
          off = n_payload; n_payload += words;
          for (u32 w = lane; w < words; w += 64) g_pay[off + w] = seen[sl * W + w];
        }
        if (sel) {
          kind = K_OP; c_f = f; c_value = val; c_final = 0; ++next_msg_id;
          inv_row = true; inv_packed = MSIM_T_INVOKE | (f << 2) | (process << 12); inv_value = val;
          if (!rd_op) my_seen[val >> 5] |= 1u << (val & 31);
          cmp_row = true; cmp_packed = MSIM_T_OK | (f << 2) | (process << 12);
          cmp_value = rd_op ? off : val; cmp_len = rd_op ? words : 0u;
        }
        // the gossip fan-out: ids in destination order, then the reply to the client (fan first for these programs)
        if (cnt) {
          ev_base = n_ev; id_base = next_id;
          if (is_node && ((fan_s >> lane) & 1)) arrive(base + __popc(fan_s & lt32), M_BROADCAST, val, 0, sl);  // (lanes >= 32 would alias the shift)
          poll();
        }
        next_id += 2 + cnt;
        t_send_cl += 2; t_recv_cl += 2; t_send_sv += cnt;
        gen_next = T + __umulhi(r_hi, p.gen_period2_us);
      }
    }

    if (lone_op) {
    } else if (timeout_round) {
      if (busy && timeout_at <= T) {
        const bool idem = IS_BCAST && c_f == MSIM_F_READ;
        complete(idem ? MSIM_T_FAIL : MSIM_T_INFO, MSIM_ERR_NET_TIMEOUT, c_f == MSIM_F_READ ? MSIM_NO_VALUE : c_value, 0);
      }
    } else {
      // ---- R1: scheduler ----
      if (due <= T) {
        switch (phase) {
          case PH_INIT: if (is_node) { mark = true; kind = K_INIT; } phase = PH_INIT_WAIT; break;
          case PH_TOPO: if (is_node) { mark = true; kind = K_TOPO; } phase = PH_TOPO_WAIT; break;
          case PH_MAIN: {
            #include "group64_nemesis.inc"
            if (gen_live && gen_next <= T && free_mask) {
              const u32 nfree = __popc(free_mask);
              const u32 kk = gen_k++;
              const u64 h = draw64(key, S_GEN, kk);
              const u32 r_hi = (u32)(h >> 32), r_lo = (u32)h;
              const u32 pick = scale32(r_lo, nfree);
              const bool sel = is_node && !busy && (u32)__popc(free_mask & lt32) == pick;
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
            if (is_node) { mark = true; kind = K_OP; m_f = MSIM_F_READ; m_value = MSIM_NO_VALUE; m_final = FINAL_FLAG ? 1 : 0; }
            phase = PH_FINAL_WAIT; break;
          default: break;
        }
        if (phase == PH_DONE) break;
      }

      // ---- R2: marked clients invoke — lane-local: the request goes to this lane's own node ----
      const u32 inv_mask = (u32)__ballot(mark);
      if (inv_mask) {
        ev_base = n_ev; id_base = next_id; n_ev += __popc(inv_mask);
        if (mark) {
          mark = false; busy = true;
          u32 rq_type, rq_a = 0;
          if (kind == K_INIT) { rq_type = M_INIT; next_msg_id = 0; }
          else if (kind == K_TOPO) { rq_type = M_TOPOLOGY; next_msg_id = 0; }
          else {
            c_f = m_f; c_value = m_value; c_final = m_final;
            inv_row = true; inv_packed = MSIM_T_INVOKE | (c_f << 2) | (c_final << 11) | (process << 12); inv_value = c_value;
            rq_type = c_f == MSIM_F_ECHO ? M_ECHO : c_f == MSIM_F_BROADCAST ? M_BROADCAST : c_f == MSIM_F_ADD ? M_ADD : c_f == MSIM_F_GENERATE ? M_GENERATE : M_READ;
            rq_a = (c_f == MSIM_F_READ || c_f == MSIM_F_GENERATE) ? 0u : c_value;
          }
          const u32 want = ++next_msg_id;
          timeout_at = T + (kind == K_OP ? p.cfg.client_timeout_ms : 10000u) * 1000u;
          arrive(next_id + __popc(inv_mask & lt32), rq_type, rq_a, want, my_client);  // ids in slot order
        }
        next_id += __popc(inv_mask); t_send_cl += __popc(inv_mask);
        poll();
      }

      // ---- R3: one input per node ----
      u32 fan_mask = 0, fan_a = 0, fan_b0 = 0;
      bool rep = false; u32 rep_dest = 0, rep_type = 0, rep_a = 0, rep_b = 0;
      bool rd = false;
      u32 jd_mask = 0;  // nodes delivering an envelope this round (their :recv events come first, node order)
      const bool delivering = is_node && !(IS_GSET && timer_next <= T) && !(IS_ACK && retry_time <= T) && deliver_at <= T;
      const u32 rd_mask = (u32)__ballot(delivering), rc_mask = (u32)__ballot(delivering && (cm.w >> 24) >= N);  // all / from a client
      if (jcap) jd_mask = rd_mask;
      if (is_node) {
        if (IS_GSET && timer_next <= T) {
          timer_next = T + 5000000u;
          u32 *snap = g_scr + ((size_t)tick * N + lane) * W;
          for (u32 w = 0; w < W; w++) snap[w] = my_seen[w];
          fan_mask = all_nodes & ~(1u << lane); fan_a = tick; tick++;
        } else if (IS_ACK && retry_time <= T) {
          // the oldest gossip task wakes (02-performance.md:421-438): re-send to whoever has not acknowledged, and queue again
          u32 v, un;
          retry_pop(v, un);
          if (un) { fan_mask = un; fan_a = v; fan_b0 = node_msgid + 1; node_msgid += __popc(un); retry_push(v, T + 1000000u, un); }
        } else if (deliver_at <= T) {
          const uint4 q = cm; deliver_at = INF;
          const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0xFFu, qa = q.z;
          if (jcap) jwrite(n_ev + __popc(jd_mask & lt32), 1, q.y, qa, qb, qsrc, lane);
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
              const u32 wv = my_seen[v >> 5];
              if (!(wv & bitm)) {
                my_seen[v >> 5] = wv | bitm;
                u32 tg = PROG == MSIM_NODE_BCAST_RPC_ALL ? (all_nodes & ~(1u << lane)) : adj;
                if (PROG != MSIM_NODE_BCAST_FF_ECHOBACK && qsrc < N) tg &= ~(1u << qsrc);
                fan_mask = tg; fan_a = v;
                if (IS_RPC) { fan_b0 = node_msgid + 1; node_msgid += __popc(tg); }
                // The un-acked mask of (node, value): written here, cleared bit by bit by L2 atomics (retry_ack), read by agent-scope loads.
                // A node sees a value for the first time exactly once (the `seen` bit above), so a value is queued at most once in a node's FIFO —
                // which is what lets the FIFO head's register copy (rt_un) mirror g_unacked[rt_v].
                if (IS_ACK && tg) { __hip_atomic_store(&g_unacked[v], tg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); retry_push(v, T + 1000000u, tg); }
              }
              if (qb != 0) { rep = true; rep_dest = qsrc; rep_type = M_BROADCAST_OK; rep_a = v; rep_b = qb; }
            } break;
            case M_BROADCAST_OK: if (IS_ACK) retry_ack(qa, qsrc); break;
            default: break;
          }
        }
      }

      n_ev += __popc(jd_mask);
      t_recv_cl += __popc(rc_mask); t_recv_sv += __popc(rd_mask) - __popc(rc_mask);
      {
        u32 rdmask = (u32)__ballot(rd);
        if (rdmask) {
          __syncthreads();
          const u32 words = (next_value + 31) >> 5;
          while (rdmask) {
            const u32 r = (u32)__builtin_ctz(rdmask); rdmask &= rdmask - 1;
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

      // COMMIT node sends.  A reply to a client is lane-local (the client lives in the sender's lane).
      bool c_arr = false; u32 ca_y = 0, ca_a = 0, ca_b = 0;  // ca_y = (id << 8) | type
      {
        const u32 fan_cnt = __popc(fan_mask);
        const u32 cnt = fan_cnt + (rep ? 1u : 0u);
        if (__ballot(cnt != 0)) {
          const u32 incl = scan32(cnt);
          ev_base = n_ev; id_base = next_id; n_ev += rdlane(incl, 31);
          { const u32 to_cl = __popc((u32)__ballot(rep && rep_dest >= N)); t_send_cl += to_cl; t_send_sv += rdlane(incl, 31) - to_cl; }
          const u32 rep_off = incl - cnt + (REP_FIRST ? 0u : fan_cnt);
          if (IS_RPC) {
            const bool rpn = rep && rep_dest < N;
            if (__ballot(fan_mask != 0 || rpn)) commit_fan_rpc(fan_mask, fan_a, fan_b0, incl - cnt + ((REP_FIRST && rep) ? 1u : 0u), rpn ? (0x80000000u | rep_dest | (rep_type << 8)) : 0u, rep_a, rep_b, rep_off);
          } else if (__ballot(fan_mask != 0)) commit_fan(fan_mask, fan_a, fan_b0, incl - cnt + ((REP_FIRST && rep) ? 1u : 0u));
          if (rep && rep_dest >= N) {  // rep_dest == my_client: no latency; lost like any other message (net.clj:214)
            const u32 id = next_id + rep_off;
            if (jcap) jwrite(ev_base + rep_off, 0, (id << 8) | rep_type, rep_a, rep_b, lane, my_client);
            if (!(NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss)) { c_arr = true; ca_y = (id << 8) | rep_type; ca_a = rep_a; ca_b = rep_b; }
          }
          next_id += rdlane(incl, 31);
        }
        poll();
      }

      // ---- R4: the clients' recv! loops (client.clj:94-107): queued (stale, older) envelopes first, then the fresh
      //      reply; envelope k of every client is handled before envelope k+1 of any (journal order) ----
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
          n_ev += __popc(dm); t_recv_cl += __popc(dm);
        }
        if (c_arr) {  // nobody is in recv!: the envelope waits for the next RPC (and is skipped there as stale)
          if (cin_n >= CLIENT_INBOX_CAP) raise(MSIM_FLAG_INBOX_OVERFLOW);
          else my_cinbox[cin_n++] = make_uint4(T, ca_y, ca_a, ca_b | (lane << 24));
        }
      }
    }

    // ---- history rows ----
    {
      const u32 imask = (u32)__ballot(inv_row), cmask = (u32)__ballot(cmp_row);
      const u32 ni = __popc(imask);
      const u32 nr = nem_rows + ni + __popc(cmask);
      if (nr) {
        if (n_rows + nr > max_rows) { flags |= MSIM_FLAG_ROWS_OVERFLOW; break; }
        const u32 tlo = (u32)((u64)T * 1000ull), thi = (u32)(((u64)T * 1000ull) >> 32);
        if (NEM && nem_rows && lane == 0) {
          const u32 pk = MSIM_T_INFO | (nem_f << 2) | (MSIM_PROCESS_NEMESIS << 12);
          stage[n_rows % STAGE_ROWS] = make_uint4(tlo, thi, pk, nem_v1);
          stage[(n_rows + 1) % STAGE_ROWS] = make_uint4(tlo, thi | (nem_len2 << 16), pk, nem_v2);
        }
        if (inv_row) stage[(n_rows + nem_rows + __popc(imask & lt32)) % STAGE_ROWS] = make_uint4(tlo, thi, inv_packed, inv_value);
        if (cmp_row) stage[(n_rows + nem_rows + ni + __popc(cmask & lt32)) % STAGE_ROWS] = make_uint4(tlo, thi | (cmp_len << 16), cmp_packed, cmp_value);
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

    // ---- cascade loop (plain gossip rounds while the scheduler is quiet at T) ----
    if ((FAST_OK || IS_RPC) && !timeout_round) {
      const u32 bm = (u32)__ballot(busy);
      bool quiet = false;
      d2 = INF;  // when the scheduler next wants to act (the clients' busy set cannot change during cascade rounds)
      if (phase == PH_MAIN) {
        const bool gl = rate > 0 && gen_next < cutoff, nl = NEM && nem_next < cutoff;
        if (gl || nl) {
          if (nl) d2 = max(nem_next, T);
          if (gl && (all_nodes & ~bm)) d2 = min(d2, max(gen_next, T));
          quiet = d2 > T;
        }
      } else if (phase == PH_SLEEP) { d2 = sleep_until; quiet = d2 > T; }
      fast = quiet;
    }
    skip_quiet = false;
  }

  // ---- epilogue ----
  __syncthreads();
  {
    const u32 blk = n_rows >> 6;
    const u32 gi = blk * 64 + lane;
    if (gi < n_rows) reinterpret_cast<uint4 *>(g_rows)[gi] = stage[gi % STAGE_ROWS];
  }
  __threadfence_block();
  if (lane == 0) {
    msim_net_stats st;
    st.all_send = (u64)t_send_cl + t_send_sv; st.all_recv = (u64)t_recv_cl + t_recv_sv;
    st.clients_send = t_send_cl; st.clients_recv = t_recv_cl;
    st.servers_send = t_send_sv; st.servers_recv = t_recv_sv;
    p.stats[inst] = st;
    msim_inst_meta m; m.n_rows = n_rows; m.n_payload_words = n_payload; m.flags = flags | atomicOr(g_flags, 0u); m.n_rounds = rounds;
    m.n_events = jcap ? n_ev : 0; m.reserved[0] = 0; m.reserved[1] = 0; m.reserved[2] = 0;
#ifdef COLO_PROF
    st.all_send = cpc[0]; st.all_recv = cpc[1]; st.clients_send = cpc[2]; st.clients_recv = cpc[3]; st.servers_send = cpc[4]; st.servers_recv = cp_fast;
    p.stats[inst] = st;
#endif
    p.meta[inst] = m;
  }
}
