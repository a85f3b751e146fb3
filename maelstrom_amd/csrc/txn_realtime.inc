// txn_realtime.inc — the realtime order in closed form, shared by txn_check_kernel, txn_check_lds_kernel, txn_classify_body.inc
// (txn_check_dev.hip) and rw_body (rw_check_dev.hip); one wavefront, lane = transaction.  sm[j] = earliest :ok completion among
// transactions j .. n-1 (smf[j]: how many transactions were invoked before that completion; sm[n] = NONE).  An :ok transaction's
// realtime successors are then the index range [t_first[t], sm[t_first[t]] == NONE ? n : smf[t_first[t]]).  Reads t_lt (type << 16),
// t_cmp, t_first of the `n` transactions.  Text, not a function: as a function it compiled the kernels to other code than they had.
  {
    u64 carry = ~0ull;
    for (int b = (int)((n + 63u) / 64u) - 1; b >= 0; b--) {
      const u32 t = (u32)b * 64u + lane;
      u64 v = (t < n && (t_lt[t] >> 16) == MSIM_T_OK) ? (((u64)t_cmp[t] << 32) | t_first[t]) : ~0ull;
      for (int o = 1; o < 64; o <<= 1) {
        const u32 ylo = (u32)__shfl_down((int)(u32)v, o), yhi = (u32)__shfl_down((int)(u32)(v >> 32), o);
        const u64 y = ((u64)yhi << 32) | ylo;
        if (lane + (u32)o < 64u) v = min(v, y);
      }
      v = min(v, carry);
      if (t < n) { sm[t] = (u32)(v >> 32); smf[t] = (u32)v; }
      carry = ((u64)wv_rl((u32)(v >> 32), 0) << 32) | wv_rl((u32)v, 0);
    }
    if (lane == 0) { sm[n] = NONE; smf[n] = n; }
  }
