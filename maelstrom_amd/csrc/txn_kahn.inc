// txn_kahn.inc — step F of txn_check_kernel (txn_check_dev.hip) and rw_body (rw_check_dev.hip): acyclic?  Kahn's algorithm over the CSR
// (off / adj) with its tables in the HBM workspace, 64 ready transactions per step: in-degrees (indeg) by atomics, the ready queue
// (queue) by ballots (lt: the lanes below this one).  Leaves `tail`, the transactions taken out: n iff the graph is acyclic.
// Text, not a function: as a function it compiled the kernels to other code than they had.
  u32 tail = 0;
  for (u32 base = 0; base < n; base += 64) {
    const u32 t = base + lane;
    const bool z = t < n && indeg[t] == 0;
    const u64 zm = __ballot(z);
    if (z) queue[tail + (u32)__popcll(zm & lt)] = t;
    tail += (u32)__popcll(zm);
  }
  __syncthreads();
  u32 head = 0;
  while (head < tail) {
    const u32 snap = tail;
    const u32 cnt = min(64u, snap - head);
    const bool on = lane < cnt;
    const u32 v = on ? queue[head + lane] : 0u;
    const u32 a0 = on ? off[v] : 0u, a1 = on ? off[v + 1] : 0u;
    for (u32 k = 0; __ballot(a0 + k < a1); k++) {
      bool push = false; u32 wv = 0;
      if (a0 + k < a1) { wv = adj[a0 + k]; push = atomicSub(&indeg[wv], 1u) == 1u; }
      const u64 pm = __ballot(push);
      if (push) queue[tail + (u32)__popcll(pm & lt)] = wv;
      tail += (u32)__popcll(pm);
    }
    head += cnt;
    __syncthreads();
  }
