// sim_kernel_raft.inc — included by engine.hip.  The Raft lin-kv node program (SURVEY.md §8a row a16,
// BASELINE configs[3]) on the same round machinery as sim_kernel<> (DESIGN.md §2), restated from
// demo/ruby/raft.rb:1-497 == demo/python/raft.py:1-593:
//   raft.py:577-585  one main-loop iteration per node per round: process_msg | step_down_on_timeout |
//                    replicate_log | election | advance_commit_index | advance_state_machine
//   raft.py:251-336  role transitions, request_votes;  :449-531 request_vote / append_entries handlers;
//   raft.py:534-553  kv_req (leader appends, follower proxies with the client's src, else error 11);
//   raft.py:147-184  KVStore.apply (errors 20 / 22);  :343-354 reply on apply if leader.
// The callbacks' closures (raft.py:280-297, :395-410) travel as echo fields in the responses.
//
// Layout: one wavefront = one cluster, lane e = endpoint e (nodes, then client slots).  Per node in HBM scratch:
// the log (8 B entries) and a ring of message descriptors (request_vote / append_entries bodies incl. copied
// entries); in LDS: envelope queues, KV state (256 B/node), next_index / match_index.
//
// Envelope (16 B, as everywhere): x = deadline, y = (id << 8) | type, z = a, w = b | (src << 24).
//   request_vote        a = desc ref (units | seq << 16)             b = msg_id
//   request_vote_res    a = term | candidacy term << 16 | granted << 31   b = in_reply_to
//   append_entries      a = desc ref                                 b = msg_id
//   append_entries_res  a = term | desc units << 16 | success << 28  b = in_reply_to (16) | desc seq << 16
//   read/write/cas      a = key | v << 8 | v' << 16 (0xFF = nil)     b = msg_id
//   *_ok / error        a = value / code                             b = in_reply_to

#define R_CLIENT_CAP 32u   // Reusable lin-kv clients (lin_kv.clj:74-76) collect late replies between RPCs
#define R_ARENA_WORDS 16384u
enum { R_NASCENT = 0, R_FOLLOWER, R_CANDIDATE, R_LEADER };
enum { M_WRITE = 14, M_WRITE_OK, M_CAS, M_CAS_OK, M_ERROR, M_REQUEST_VOTE, M_REQUEST_VOTE_RES, M_APPEND_ENTRIES, M_APPEND_ENTRIES_RES };
enum { S_NODE = 11 };

template <bool NEM, bool NET_RANDOM>
__global__ void __launch_bounds__(64, 3) raft_kernel(const KParams p) {   // (as sim_kernel<>: 100-148 B of private memory at four)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *const stage = reinterpret_cast<uint4 *>(smem);
  uint4 *const inbox = reinterpret_cast<uint4 *>(smem + p.off_inbox);
  unsigned char *const kv_all = smem + p.off_seen;                      // N x 256 bytes: KVStore state, 0xFF = absent
  u32 *const nim = reinterpret_cast<u32 *>(smem + p.off_seen + p.N * 256);  // [node][peer][2]: next_index, match_index
  u32 *const aeref = nim + p.N * p.N * 2;                               // [node][peer]: descriptor ref of this round's append_entries
  u32 *const misc = reinterpret_cast<u32 *>(smem + p.off_misc);

  const u32 lane = threadIdx.x;
  const u32 inst = blockIdx.x;
  const u32 N = p.N, C = p.C, CS = p.CS;
  const bool is_node = lane < N;
  const bool is_client = lane >= N && lane < N + CS;
  const u32 slot = lane - N;
  const bool is_worker = is_client && slot < C;
  const u64 key = mix64(p.cfg.seed + 0x9E3779B97F4A7C15ull * (p.first_instance + inst + 1));
  const u64 lt_mask = (1ull << lane) - 1;
  const u32 lt32 = lane < 32 ? ((1u << lane) - 1) : 0xFFFFFFFFu;
  const u64 worker_mask = ((C >= 64 ? ~0ull : ((1ull << C) - 1)) << N);
  const u32 all_nodes = (1u << N) - 1;
  const u32 max_rows = p.cfg.max_rows, max_pay = p.cfg.max_payload_words;
  const u32 p_loss = p.cfg.p_loss_q32, lat_mean = p.cfg.latency_mean_ms, lat_dist = p.cfg.latency_dist;
  const u32 rate = p.cfg.rate_mhz;
  const u32 log_cap = p.raft_log_cap;
  u32 rpc_timeout_ms = 10 * lat_mean; if (rpc_timeout_ms < 1000) rpc_timeout_ms = 1000;   // lin_kv.clj:54

  msim_op *const g_rows = p.rows + (size_t)inst * max_rows;
  u32 *const g_pay = p.payload + (size_t)inst * max_pay;
  u32 *const g_scr = p.scratch + (size_t)inst * p.scratch_words;
  u32 *const my_log = g_scr + (size_t)(is_node ? lane : 0) * log_cap * 2;                 // entry i at (i-1)*2
  u32 *const arenas = g_scr + (size_t)N * log_cap * 2;
  u32 *const my_arena = arenas + (size_t)(is_node ? lane : 0) * R_ARENA_WORDS;
  const u32 jcap = p.cfg.journal_capacity;
  uint4 *const g_ev = p.journal + (size_t)inst * jcap;

  const u32 my_cap = is_node ? p.cap_node : R_CLIENT_CAP;
  const u32 my_spill_cap = is_node ? p.spill_cap : 0u;
  uint4 *const my_inbox = inbox + (is_node ? lane * p.cap_node : (is_client ? N * p.cap_node + slot * R_CLIENT_CAP : 0));
  uint4 *const my_spill = reinterpret_cast<uint4 *>(g_scr + p.spill_off) + (size_t)(is_node ? lane : 0) * p.spill_cap;
  unsigned char *const my_kv = kv_all + (is_node ? lane : 0) * 256;
  u32 *const my_nim = nim + (is_node ? lane : 0) * N * 2;

  for (u32 i = lane; i < N * 64; i += 64) reinterpret_cast<u32 *>(kv_all)[i] = 0xFFFFFFFFu;
  for (u32 i = lane; i < N * N * 3; i += 64) nim[i] = 0;
  if (is_node) { my_log[0] = 0; my_log[1] = 0; }  // the default entry {term 0, op nil} (raft.py:109-112)
  __syncthreads();

  // ---- endpoint state ----
  bool has_c = false; u32 deliver_at = 0; uint4 cm = make_uint4(0, 0, 0, 0);
  bool have_pm = false; uint4 pm = make_uint4(0, 0, 0, 0);
  u32 in_n = 0, sp_n = 0, part = 0;
  // ---- raft node state (raft.py:197-226) ----
  u32 role = R_NASCENT, term = 0, commit_index = 0, last_applied = 1, rng_ctr = 0, log_n = 1, last_term = 0;
  int voted_for = -1, leader = -1;
  u32 election_deadline = 0, step_down_deadline = 0, last_replication = 0, votes = 0;
  u32 node_msgid = 0, arena_head = 0, arena_seq = 0, act_time = INF;
  // ---- client state ----
  bool busy = false, mark = false; u32 kind = K_NONE;
  u32 want = 0, timeout_at = 0, next_msg_id = 0, c_f = 0, c_value = 0, process = slot;
  u32 dest_node = is_client ? slot % N : 0; const u32 c_mod_n = C % N;
  u32 m_f = 0, m_value = 0, key_reg = INF;   // key_reg: the process id this thread registered on the current key
  u32 s_send_cl = 0, s_send_sv = 0, s_recv_cl = 0, s_recv_sv = 0, my_flags = 0;
  // ---- wave-uniform state ----
  u32 T = 0, phase = PH_INIT, cutoff = 0, gen_next = 0, gen_k = 0, nem_next = 0, nem_j = 0, cur_key = 0, key_procs = 0;
  u32 loss_on = 0, next_id = 0, n_rows = 0, n_payload = 0, flags = 0, rounds = 0;
  u32 n_ev = 0, ev_base = 0, id_base = 0;

  auto jwrite = [&](u32 idx, u32 recv, u32 y, u32 a, u32 b, u32 src, u32 dest) {
    const u32 ty = y & 0x7Fu;
    if (ty >= M_REQUEST_VOTE) a = 0;  // raft RPC bodies live in descriptors; the journal keeps type, ids and route
    if (idx < jcap) g_ev[idx] = make_uint4(T, (y & ~0x80u) | (recv << 7), a, src | (dest << 8) | ((b & 0xFFFFu) << 16));
    else my_flags |= MSIM_FLAG_JOURNAL_OVERFLOW;
  };
#define PAYS_LATENCY(src) ((src) < N && is_node)   // neither end is a client (group64_net.inc)
#define ENDPOINT_LANES   // a lane is one endpoint: node, worker slot or service
#define COMMIT_FLAG   // has_c says whether an envelope is committed
#define OWN_JWRITE   // the jwrite above
#define POLL_LANE (is_node || busy)   // the lanes that take from their queue (group64_poll.inc)
  #include "group64_net.inc"
  #include "group64_poll.inc"

  // ---- raft helpers (node lanes) ----
  auto reset_election_deadline = [&]() {  // raft.py:251-253: now + 2 s * (random + 1)
    election_deadline = T + 2000000u + scale32(draw32(key, S_NODE, ((u64)lane << 32) | rng_ctr++), 2000000u);
  };
  auto become_follower = [&]() { role = R_FOLLOWER; leader = -1; reset_election_deadline(); };           // :303-310
  auto maybe_step_down = [&](u32 remote) { if (term < remote) { term = remote; voted_for = -1; become_follower(); } };  // :259-272
  auto become_leader = [&]() {                                                                            // :323-336
    role = R_LEADER; leader = -1; last_replication = 0;
    for (u32 i = 0; i < N; i++) { my_nim[i * 2] = log_n + 1; my_nim[i * 2 + 1] = 0; }
    step_down_deadline = T + 2000000u;
  };
  auto arena_alloc = [&](u32 words) -> u32 {  // ring of message descriptors; returns offset in words (multiple of 4)
    words = (words + 3) & ~3u;
    if (words > R_ARENA_WORDS) { my_flags |= MSIM_FLAG_ARENA_OVERRUN; return 0; }
    if (arena_head + words > R_ARENA_WORDS) arena_head = 0;
    const u32 off = arena_head; arena_head += words; arena_seq = (arena_seq + 1) & 0xFFu;
    return off;
  };
  auto log_term = [&](u32 i) -> u32 { return my_log[(i - 1) * 2] & 0xFFFFu; };

  for (;;) {
    #include "group64_phase.inc"

    // ---- R0: time ----
    #include "group64_time.inc"
    if (is_node) my_t = min(my_t, act_time);
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
            rq_type = c_f == MSIM_F_WRITE ? M_WRITE : c_f == MSIM_F_CAS ? M_CAS : M_READ;
            rq_a = c_value;
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

      // ---- R3: one main-loop iteration per node (raft.py:577-585): a message first, else the first action that applies ----
      u32 fan_mask = 0, fan_type = 0, fan_a = 0, fan_b0 = 0;       // fan_type M_APPEND_ENTRIES: per-peer descriptor refs in aeref[]
      bool rep = false; u32 rep_dest = 0, rep_type = 0, rep_a = 0, rep_b = 0, rep_src = lane;
      u64 jd_mask = 0;
      if (jcap) jd_mask = __ballot(is_node && has_c && deliver_at <= T);
      if (is_node) {
        if (has_c && deliver_at <= T) {
          const uint4 q = cm; has_c = false;
          const u32 qsrc = q.w >> 24, qb = q.w & 0xFFFFFFu, qtype = q.y & 0x7Fu, qa = q.z;
          if (qsrc >= N) s_recv_cl++; else s_recv_sv++;
          if (jcap) jwrite(n_ev + (u32)__popcll(jd_mask & lt_mask), 1, q.y, qa, qb, qsrc, lane);
          switch (qtype) {
            case M_INIT:  // raft_init, raft.py:432-447
              become_follower(); last_applied = 1;
              rep = true; rep_dest = qsrc; rep_type = M_INIT_OK; rep_b = qb; break;
            case M_REQUEST_VOTE: {  // raft.py:449-481
              const u32 *d = arenas + (size_t)qsrc * R_ARENA_WORDS + (qa & 0xFFFu) * 4;
              const u32 w0 = d[0], lli = d[1], w2 = d[2];
              if ((w2 >> 24) != ((qa >> 16) & 0xFFu)) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
              const u32 r_term = w0 & 0xFFFFu, llt = w0 >> 16;
              maybe_step_down(r_term);
              u32 grant = 0;
              if (r_term < term) {}
              else if (voted_for >= 0) {}
              else if (llt < last_term) {}
              else if (llt == last_term && lli < log_n) {}
              else { grant = 1; voted_for = (int)qsrc; reset_election_deadline(); }
              rep = true; rep_dest = qsrc; rep_type = M_REQUEST_VOTE_RES; rep_b = qb;
              rep_a = term | ((r_term & 0x7FFFu) << 16) | (grant << 31);
            } break;
            case M_REQUEST_VOTE_RES: {  // closure of request_votes, raft.py:280-297
              const u32 r_term = qa & 0xFFFFu, cand = (qa >> 16) & 0x7FFFu, granted = qa >> 31;
              step_down_deadline = T + 2000000u;
              maybe_step_down(r_term);
              if (role == R_CANDIDATE && term == cand && r_term == term && granted) {
                votes |= 1u << qsrc;
                if ((u32)__popc(votes) >= N / 2 + 1) become_leader();
              }
            } break;
            case M_APPEND_ENTRIES: {  // raft.py:483-531
              const u32 units = qa & 0xFFFu, seq = (qa >> 16) & 0xFFu;
              const u32 *d = arenas + (size_t)qsrc * R_ARENA_WORDS + units * 4;
              const u32 w0 = d[0], w1 = d[1], w2 = d[2];
              if ((w2 >> 24) != seq) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
              const u32 r_term = w0 & 0xFFFFu, prev_term = w0 >> 16, prev_idx = w1 & 0xFFFFu, cnt = w1 >> 16, lcommit = w2 & 0xFFFFFFu;
              maybe_step_down(r_term);
              u32 ok = 0;
              if (r_term >= term) {
                leader = (int)qsrc; reset_election_deadline();
                if (prev_idx >= 1 && prev_idx <= log_n && log_term(prev_idx) == prev_term) {
                  if (prev_idx + cnt > log_cap) my_flags |= MSIM_FLAG_ROWS_OVERFLOW;
                  else {
                    log_n = prev_idx;  // truncate(prev_log_index), then append
                    for (u32 i = 0; i < cnt; i++) { my_log[(log_n + i) * 2] = d[4 + i * 2]; my_log[(log_n + i) * 2 + 1] = d[5 + i * 2]; }
                    last_term = cnt ? (d[4 + (cnt - 1) * 2] & 0xFFFFu) : prev_term;
                    log_n += cnt;
                    if (commit_index < lcommit) commit_index = min(lcommit, log_n);
                    ok = 1;
                  }
                }
              }
              rep = true; rep_dest = qsrc; rep_type = M_APPEND_ENTRIES_RES;
              rep_a = term | (units << 16) | (ok << 28); rep_b = (qb & 0xFFFFu) | (seq << 16);
            } break;
            case M_APPEND_ENTRIES_RES: {  // handler closure of replicate_log, raft.py:395-410
              const u32 r_term = qa & 0xFFFFu, units = (qa >> 16) & 0xFFFu, ok = (qa >> 28) & 1u, seq = (qb >> 16) & 0xFFu;
              maybe_step_down(r_term);
              if (role == R_LEADER) {
                const u32 *d = my_arena + units * 4;
                const u32 w0 = d[0], w1 = d[1], w2 = d[2];
                if ((w2 >> 24) != seq) my_flags |= MSIM_FLAG_ARENA_OVERRUN;
                if ((w0 & 0xFFFFu) == term) {
                  step_down_deadline = T + 2000000u;
                  const u32 ni = (w1 & 0xFFFFu) + 1, cnt = w1 >> 16;
                  if (ok) { my_nim[qsrc * 2] = max(my_nim[qsrc * 2], ni + cnt); my_nim[qsrc * 2 + 1] = max(my_nim[qsrc * 2 + 1], ni - 1 + cnt); }
                  else if (my_nim[qsrc * 2] > 1) my_nim[qsrc * 2] -= 1;
                }
              }
            } break;
            case M_READ: case M_WRITE: case M_CAS: {  // kv_req, raft.py:534-553
              if (role == R_LEADER) {
                if (log_n >= log_cap) my_flags |= MSIM_FLAG_ROWS_OVERFLOW;
                else {
                  const u32 v1 = (qa >> 8) & 0xFFu, v2 = (qa >> 16) & 0xFFu;
                  my_log[log_n * 2] = term | (qtype << 16) | ((qa & 0xFFu) << 24);
                  my_log[log_n * 2 + 1] = (qb & 0xFFFFu) | (qsrc << 16) | ((v1 & 0xFu) << 24) | ((v2 & 0xFu) << 28);
                  log_n++; last_term = term;
                }
              } else if (leader >= 0) { rep = true; rep_dest = (u32)leader; rep_type = qtype; rep_a = qa; rep_b = qb; rep_src = qsrc; }  // proxy, client's src
              else { rep = true; rep_dest = qsrc; rep_type = M_ERROR; rep_a = 11; rep_b = qb; }
            } break;
            default: break;
          }
        } else if (act_time <= T) {
          bool done = false;
          if (role == R_LEADER && step_down_deadline < T) { become_follower(); done = true; }              // :371-377
          if (!done && role == R_LEADER && T - last_replication > 50000u) {                                 // replicate_log :379-424
            const u32 elapsed = T - last_replication;
            for (u32 i = 0; i < N; i++) if (i != lane) {
              const u32 ni = my_nim[i * 2];
              const u32 cnt = ni <= log_n ? log_n - ni + 1 : 0;
              if (cnt > 0 || elapsed > 1000000u) {
                const u32 off = arena_alloc(4 + cnt * 2);
                u32 *d = my_arena + off;
                d[0] = term | (log_term(ni - 1) << 16); d[1] = (ni - 1) | (cnt << 16); d[2] = commit_index | (arena_seq << 24); d[3] = 0;
                for (u32 k = 0; k < cnt; k++) { d[4 + k * 2] = my_log[(ni - 1 + k) * 2]; d[5 + k * 2] = my_log[(ni - 1 + k) * 2 + 1]; }
                aeref[lane * N + i] = (off >> 2) | (arena_seq << 16);
                fan_mask |= 1u << i;
              }
            }
            if (fan_mask) { fan_type = M_APPEND_ENTRIES; fan_b0 = node_msgid; node_msgid += __popc(fan_mask); last_replication = T; done = true; }
          }
          if (!done && election_deadline < T) {                                                             // election :360-369
            if (role == R_FOLLOWER || role == R_CANDIDATE) {  // become_candidate :312-321 + request_votes :274-299
              role = R_CANDIDATE; term += 1; voted_for = (int)lane; leader = -1;
              reset_election_deadline(); step_down_deadline = T + 2000000u;
              votes = 1u << lane;
              const u32 off = arena_alloc(4);
              u32 *d = my_arena + off;
              d[0] = term | (last_term << 16); d[1] = log_n; d[2] = arena_seq << 24; d[3] = 0;
              fan_mask = all_nodes & ~(1u << lane); fan_type = M_REQUEST_VOTE; fan_a = (off >> 2) | (arena_seq << 16);
              fan_b0 = node_msgid; node_msgid += N - 1;
            } else reset_election_deadline();
            done = true;
          }
          if (!done && role == R_LEADER) {                                                                  // advance_commit_index :379-387
            // median(match_index incl. our own log size), biased low: the (n - majority)-th smallest
            u32 m = 0; const u32 kth = N - (N / 2 + 1);
            for (u32 i = 0; i < N; i++) {
              const u32 vi = i == lane ? log_n : my_nim[i * 2 + 1];
              u32 rk = 0;
              for (u32 j = 0; j < N; j++) { const u32 vj = j == lane ? log_n : my_nim[j * 2 + 1]; rk += (vj < vi || (vj == vi && j < i)) ? 1u : 0u; }
              if (rk == kth) m = vi;
            }
            if (commit_index < m && log_term(m) == term) { commit_index = m; done = true; }
          }
          if (!done && last_applied < commit_index) {                                                       // advance_state_machine :343-354
            last_applied += 1;
            const u32 w0 = my_log[(last_applied - 1) * 2], w1 = my_log[(last_applied - 1) * 2 + 1];
            const u32 et = (w0 >> 16) & 0xFFu, ek = w0 >> 24, v1 = (w1 >> 24) & 0xFu, v2 = w1 >> 28;
            unsigned char cur = my_kv[ek];
            u32 rt, ra = 0;
            if (et == M_READ) { if (cur != 0xFF) { rt = M_READ_OK; ra = cur; } else { rt = M_ERROR; ra = 20; } }
            else if (et == M_WRITE) { my_kv[ek] = (unsigned char)v1; rt = M_WRITE_OK; }
            else { if (cur == 0xFF) { rt = M_ERROR; ra = 20; } else if (cur != v1) { rt = M_ERROR; ra = 22; } else { my_kv[ek] = (unsigned char)v2; rt = M_CAS_OK; } }
            if (role == R_LEADER) { rep = true; rep_dest = (w1 >> 16) & 0xFFu; rep_type = rt; rep_a = ra; rep_b = w1 & 0xFFFFu; }
          }
        }
        // when does this node's loop have something to do again, besides messages? (oracle: raft_next_time)
        if (role == R_NASCENT) act_time = INF;
        else {
          u32 t = election_deadline + 1;
          if (role == R_LEADER) {
            t = min(t, step_down_deadline + 1);
            bool pending = false;
            for (u32 i = 0; i < N; i++) if (i != lane && my_nim[i * 2] <= log_n) pending = true;
            t = min(t, last_replication + (pending ? 50001u : 1000001u));
            u32 m = 0; const u32 kth = N - (N / 2 + 1);
            for (u32 i = 0; i < N; i++) {
              const u32 vi = i == lane ? log_n : my_nim[i * 2 + 1];
              u32 rk = 0;
              for (u32 j = 0; j < N; j++) { const u32 vj = j == lane ? log_n : my_nim[j * 2 + 1]; rk += (vj < vi || (vj == vi && j < i)) ? 1u : 0u; }
              if (rk == kth) m = vi;
            }
            if (commit_index < m && log_term(m) == term) t = 0;
          }
          if (last_applied < commit_index) t = 0;
          act_time = t;
        }
      }
      n_ev += (u32)__popcll(jd_mask);

      // COMMIT node sends: ids in node order; a node emits either a fan-out or one single message per round
      {
        const u32 fan_cnt = __popc(fan_mask);
        const u32 cnt = fan_cnt + (rep ? 1u : 0u);
        if (__ballot(cnt != 0)) {
          __syncthreads();  // aeref[] written above is read by other lanes
          const u32 incl = scan32(cnt);
          const u32 excl = incl - cnt;
          ev_base = n_ev; id_base = next_id; n_ev += rdlane(incl, 31);
          if (is_node) {
            s_send_sv += fan_cnt;
            if (rep) { if (rep_dest >= N || rep_src >= N) s_send_cl++; else s_send_sv++; }
          }
          u64 fans = __ballot(fan_mask != 0);
          while (fans) {
            const u32 s = (u32)__builtin_ctzll(fans); fans &= fans - 1;
            const u32 f_mask = rdlane(fan_mask, s), f_type = rdlane(fan_type, s), f_a = rdlane(fan_a, s), f_b0 = rdlane(fan_b0, s);
            const u32 base = next_id + rdlane(excl, s);
            if (lane < N && ((f_mask >> lane) & 1)) {
              const u32 rank = __popc(f_mask & lt32);
              const u32 a = f_type == M_APPEND_ENTRIES ? aeref[s * N + lane] : f_a;
              arrive(base + rank, f_type, a, f_b0 + rank, s);
            }
          }
          u64 reps = __ballot(rep);
          if (reps) {
            const u32 rep_pack = rep_dest | (rep_type << 8) | (rep_src << 16);
            while (reps) {
              const u32 s = (u32)__builtin_ctzll(reps); reps &= reps - 1;
              const u32 pk = rdlane(rep_pack, s), o = rdlane(excl, s);
              const u32 r_a = rdlane(rep_a, s), r_b = rdlane(rep_b, s);
              if (lane == (pk & 0xFF)) arrive(next_id + o, (pk >> 8) & 0xFF, r_a, r_b, pk >> 16);
            }
          }
          next_id += rdlane(incl, 31);
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
            if (qtype == M_READ_OK) complete(MSIM_T_OK, 0, (c_value & 0xFFu) | ((qa & 0xFFu) << 8) | 0xFF0000u);   // [k v], lin_kv.clj:56-61
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
