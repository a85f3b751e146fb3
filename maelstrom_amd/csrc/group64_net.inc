// group64_net.inc — body fragment shared by the one-cluster-per-wavefront kernels (all but sim_kernel_colo.inc, whose FIFO queue and three
// try_commits are its own, and sim_kernel_wide.inc, whose lanes hold two endpoints each), included inside the kernel after the state
// declarations: the journal's event record (jwrite), an endpoint's queue (my_cap envelopes in LDS, the rest in its HBM spill area), the
// arrival of an envelope at THIS lane (net.clj:189-221: latency drawn from the message id between two servers, the journal's :send before
// the loss decision, the pending envelope that an idle endpoint takes at once) and recv!'s commitment to an envelope (net.clj:223-247).
// The kernel says how its lanes are laid out before the include:
//   PAYS_LATENCY(src)   whether an envelope from endpoint src to this lane pays latency (neither end is a client, util.clj:7-16)
//   ENDPOINT_LANES      defined where a lane is ONE endpoint (node, worker slot or service) out of up to 64: the journal's dest is the
//                       lane, only a node lane checks partitions, ballots are 64 bits wide (WB / WPOP / WLT) and busy_mask also has the
//                       busy clients that are not workers.  Not defined where lane i is node i AND its client, the services behind them:
//                       arrive() is told the endpoint, and every ballot fits a word
//   COMMIT_FLAG         defined where "an envelope is committed" is the kernel's has_c; otherwise it is deliver_at != INF
//   OWN_JWRITE          defined by a kernel that has declared its own jwrite (sim_kernel_raft.inc: RPC bodies are not journalled)
// group64_end.inc at the end of the kernel forgets these names again (the kernels of a unit follow one another in sim_kernels.h).
// Uses the kernel's names: jcap, g_ev, T, my_flags, my_inbox, my_cap, my_spill, my_spill_cap, in_n, sp_n, have_pm, pm, cm, deliver_at,
// part, key, N, lane, is_node, loss_on, p_loss, lat_mean, lat_dist, ev_base, id_base.
#ifdef ENDPOINT_LANES
#define WB(pred) __ballot(pred)
#define WPOP(m) ((u32)__popcll(m))
#define WLT lt_mask
#define WORKERS_OF(m) ((m) & worker_mask)
#else
#define WB(pred) ((u32)__ballot(pred))
#define WPOP(m) ((u32)__popc(m))
#define WLT lt32
#define WORKERS_OF(m) (m)
#endif
#ifdef COMMIT_FLAG
#define NOTHING_COMMITTED (!has_c)
#define COMMITTED_AT (has_c ? deliver_at : INF)
#else
#define NOTHING_COMMITTED (deliver_at == INF)
#define COMMITTED_AT deliver_at
#endif
#ifndef OWN_JWRITE
  // one journal event (event :id = idx); y = (message id << 8) | body type
  auto jwrite = [&](u32 idx, u32 recv, u32 y, u32 a, u32 b, u32 src, u32 dest) {
    if (idx < jcap) g_ev[idx] = make_uint4(T, (y & ~0x80u) | (recv << 7), a, src | (dest << 8) | ((b & 0xFFFFu) << 16));
    else my_flags |= MSIM_FLAG_JOURNAL_OVERFLOW;
  };
#endif
  auto lds_push = [&](const uint4 m) {
    if (in_n < my_cap) { my_inbox[in_n++] = m; return; }
    if (sp_n < my_spill_cap) { my_spill[sp_n++] = m; return; }
    my_flags |= MSIM_FLAG_INBOX_OVERFLOW;
  };
#ifdef ENDPOINT_LANES
  auto arrive = [&](u32 id, u32 type, u32 a, u32 b, u32 src) {
    const u32 dest = lane;
#else
  auto arrive = [&](u32 id, u32 type, u32 a, u32 b, u32 src, u32 dest) {   // dest: this lane's endpoint index (journal only)
#endif
    u32 lat = 0;
    if (PAYS_LATENCY(src)) {
      if (!NET_RANDOM || lat_dist == MSIM_LAT_CONSTANT) lat = lat_mean;
      else if (lat_dist == MSIM_LAT_UNIFORM) lat = scale32(draw32(key, S_LATENCY, id), 2 * lat_mean);
      else lat = (u32)(((u64)lat_mean * neg_ln_q16(draw32(key, S_LATENCY, id))) >> 16);
    }
    if (jcap) jwrite(ev_base + (id - id_base), 0, (id << 8) | type, a, b, src, dest);  // :send precedes the loss decision (net.clj:208)
    if (NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss) return;  // net.clj:214
    uint4 m = make_uint4(T + lat * 1000u, (id << 8) | type, a, b | (src << 24));
    if (!have_pm) { pm = m; have_pm = true; return; }
    if (m.x < pm.x || (m.x == pm.x && m.y < pm.y)) { const uint4 t = m; m = pm; pm = t; }
    lds_push(m);
  };
  auto try_commit = [&](const uint4 e) {
    const u32 src = e.w >> 24;
#ifdef ENDPOINT_LANES
    if (NEM && is_node && src < N && ((part >> src) & 1)) return;  // partitioned: dropped at take time, no :recv (net.clj:232-234)
#else
    if (NEM && src < N && ((part >> src) & 1)) return;  // partitioned (node <-> node only; `part` is 0 on a service's lane)
#endif
    cm = e;
#ifdef COMMIT_FLAG
    has_c = true;
#endif
    deliver_at = e.x <= T ? T : T + ((e.x - T) / 1000u) * 1000u;  // (Thread/sleep (long dt)) net.clj:236-238
  };
