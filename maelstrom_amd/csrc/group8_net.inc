// group8_net.inc — body fragment shared by the eight-clusters-per-wavefront kernels (hat8.hip, uid8.hip, crdt8.hip, bcast8.hip, kafka8.hip,
// mk8.hip; dt8.hip keeps a queue of its own shape, txn8.hip a copy with a one-key-at-a-time scan that is faster for it), included inside the kernel after the state declarations: the cluster's slice
// of a ballot (GB) and the pull of a value from a lane of the group (GGET), an endpoint's queue (RQ envelopes in LDS slot-major, the rest
// in the HBM spill area), the arrival of an envelope at THIS lane's node or service (net.clj:189-221: latency drawn from the message id,
// loss, the pending envelope that an idle endpoint takes at once), recv!'s commitment to the envelope with the minimal (deadline, id)
// (net.clj:223-247).  Uses the kernel's names: GS, gbase, my_q, my_spill, my_spill_cap, in_n, sp_n, have_pm, pm, cm, deliver_at, part, T,
// key, N, alive, loss_on, p_loss, lat_mean, lat_dist, my_flags, and two macros that the kernel defines before the include and #undef-s
// after it: SERVER_SRC(src), whether the sender endpoint src is a node or a service (neither end is a client: the message pays latency),
// and QUEUE_LANE, whether this lane owns a queue (a node or a service).
  auto GB = [&](bool pred) -> u32 { return (u32)(__ballot(pred) >> gbase) & ((1u << GS) - 1u); };   // the cluster's slice of a ballot
  auto GGET = [&](u32 v, u32 s) -> u32 { return (u32)__builtin_amdgcn_ds_bpermute((int)((gbase + s) << 2), (int)v); };   // v of lane s of my group

  auto q_push = [&](const uint4 m) {
    if (in_n < RQ) { my_q[in_n * 64u] = m; in_n++; return; }
    if (sp_n < my_spill_cap) { my_spill[sp_n++] = m; return; }
    my_flags |= MSIM_FLAG_INBOX_OVERFLOW;
  };
  auto arrive = [&](u32 id, u32 type, u32 a, u32 b, u32 src) {
    u32 lat = 0;
    if (SERVER_SRC(src)) {  // neither end is a client
      if (!NET_RANDOM || lat_dist == MSIM_LAT_CONSTANT) lat = lat_mean;
      else if (lat_dist == MSIM_LAT_UNIFORM) lat = scale32(draw32(key, S_LATENCY, id), 2 * lat_mean);
      else lat = (u32)(((u64)lat_mean * neg_ln_q16(draw32(key, S_LATENCY, id))) >> 16);
    }
    if (NET_RANDOM && loss_on && p_loss && draw32(key, S_LOSS, id) < p_loss) return;
    uint4 m = make_uint4(T + lat * 1000u, (id << 8) | type, a, b | (src << 24));
    if (!have_pm) { pm = m; have_pm = true; return; }
    if (m.x < pm.x || (m.x == pm.x && m.y < pm.y)) { const uint4 t = m; m = pm; pm = t; }
    q_push(m);
  };
  auto try_commit = [&](const uint4 e) {
    const u32 src = e.w >> 24;
    if (NEM && src < N && ((part >> src) & 1)) return;  // partitioned (node <-> node only): dropped at take time, no :recv (net.clj:232-234)
    cm = e;
    deliver_at = e.x <= T ? T : T + ((e.x - T) / 1000u) * 1000u;  // (Thread/sleep (long dt)) net.clj:236-238
  };
  auto poll = [&]() {
    if (have_pm) {
      have_pm = false;
      if (alive && deliver_at == INF && (in_n | sp_n) == 0) try_commit(pm);
      else q_push(pm);
    }
    while (alive && QUEUE_LANE && deliver_at == INF && (in_n | sp_n) != 0) {
      u32 best = 0; bool in_spill = false;
      uint2 bk = make_uint2(INF, INF);
      for (u32 i = 0; i < in_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_q[i * 64u]);
        if (kk.x < bk.x || (kk.x == bk.x && kk.y < bk.y)) { bk = kk; best = i; }
      }
      for (u32 i0 = 0; i0 < sp_n; i0 += 8) {   // deep queues only: eight spilled keys per round trip
        uint2 kq[8];
#pragma unroll
        for (u32 t = 0; t < 8; t++) kq[t] = *reinterpret_cast<const uint2 *>(&my_spill[min(i0 + t, sp_n - 1)]);
#pragma unroll
        for (u32 t = 0; t < 8; t++) if (i0 + t < sp_n && (kq[t].x < bk.x || (kq[t].x == bk.x && kq[t].y < bk.y))) { bk = kq[t]; best = i0 + t; in_spill = true; }
      }
      uint4 e;
      if (in_spill) { e = my_spill[best]; sp_n--; if (best != sp_n) my_spill[best] = my_spill[sp_n]; }
      else { e = my_q[best * 64u]; in_n--; if (best != in_n) my_q[best * 64u] = my_q[in_n * 64u]; }
      try_commit(e);
    }
  };

