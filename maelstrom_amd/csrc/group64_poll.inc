// group64_poll.inc — body fragment shared by the one-cluster-per-wavefront kernels, included after group64_net.inc: recv!'s choice of the
// envelope with the minimal (deadline, id) among the pending one, the queue's LDS slots and its HBM spill area (net.clj:223-247), one key
// per load.  The kernel names the lanes that take from their queue now, POLL_LANE (servers all the time, a client's endpoint only while
// it waits for a reply, client.clj:94-95); without ENDPOINT_LANES only such lanes are ever handed an envelope, so the pending one is
// taken without asking.  sim_kernel_general.inc, sim_kernel_hat.inc and sim_kernel_hatg.inc keep their own poll: theirs scans with 64-bit
// keys and spill_min()'s eight keys per trip (their queues run deep behind long sleeps and partitions), which is different code on the
// device.  Uses the kernel's names: have_pm, pm, in_n, sp_n, my_inbox, my_spill, try_commit, lds_push, NOTHING_COMMITTED.
  auto poll = [&]() {
#ifdef ENDPOINT_LANES
    const bool elig = POLL_LANE;
    if (have_pm) {
      have_pm = false;
      if (elig && NOTHING_COMMITTED && (in_n | sp_n) == 0) try_commit(pm);  // common case: nothing queued, no LDS traffic
      else lds_push(pm);
    }
    while (elig && NOTHING_COMMITTED && (in_n | sp_n) != 0) {
#else
    if (have_pm) {   // only a polling lane is ever handed an envelope: arrive() is called for a node's own client, by the service's lane
      have_pm = false;   // for itself and by the lane a reply names, all of them POLL_LANEs; the emulator build checks it
#ifdef MSIM_HIPEMU
      if (!(POLL_LANE)) __builtin_trap();
#endif
      if (NOTHING_COMMITTED && (in_n | sp_n) == 0) try_commit(pm);
      else lds_push(pm);
    }
    while (POLL_LANE && NOTHING_COMMITTED && (in_n | sp_n) != 0) {
#endif
      u32 best = 0; bool in_spill = false;
      uint2 bk = make_uint2(INF, INF);
      for (u32 i = 0; i < in_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_inbox[i]);
        if (kk.x < bk.x || (kk.x == bk.x && kk.y < bk.y)) { bk = kk; best = i; }
      }
      for (u32 i = 0; i < sp_n; i++) {
        const uint2 kk = *reinterpret_cast<const uint2 *>(&my_spill[i]);
        if (kk.x < bk.x || (kk.x == bk.x && kk.y < bk.y)) { bk = kk; best = i; in_spill = true; }
      }
      uint4 e;
      if (in_spill) { e = my_spill[best]; sp_n--; if (best != sp_n) my_spill[best] = my_spill[sp_n]; }
      else { e = my_inbox[best]; in_n--; if (best != in_n) my_inbox[best] = my_inbox[in_n]; }
      try_commit(e);
    }
  };
