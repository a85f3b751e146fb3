// txn_pairing.inc — step A's one serial walk, shared by txn_check_kernel, txn_classify_body.inc (txn_check_dev.hip) and rw_body
// (rw_check_dev.hip): the transaction rows of one block of 64 rows (`is`; `im` its invocations, `n` transactions before the block),
// taken in row order against the table of open calls in lane registers (o_used, o_proc, o_txn, o_len: lane = one open call, o_len the
// words of its request).  An invocation takes its process's slot or a free one; a completion closes its process's call and writes what
// became of the transaction.  Every lane holds its own row (row, idx, len, woff).  More than 64 calls open at once: `bad`, and the walk
// ends (the includer leaves its row loop).  Text, not a function: as a function it compiled the kernels to other code than they had.
      u64 m = __ballot(is);
      while (m) {
        const u32 j = (u32)__builtin_ctzll(m); m &= m - 1;
        const u32 z = wv_rl(row.z, j);
        const u32 jt = z & 3u, jp = z >> 12;
        const u64 hit = __ballot(o_used && o_proc == jp);
        if (jt == MSIM_T_INVOKE) {
          u32 s;
          if (hit) s = (u32)__builtin_ctzll(hit);
          else { const u64 used = __ballot(o_used); if (used == ~0ull) { bad = true; break; } s = (u32)__builtin_ctzll(~used); }
          const u32 tj = n + (u32)__popcll(im & ((1ull << j) - 1ull));
          const u32 jl = wv_rl(row.y, j) >> 16;
          if (lane == s) { o_used = true; o_proc = jp; o_txn = tj; o_len = jl; }
        } else if (hit) {
          const u32 s = (u32)__builtin_ctzll(hit);
          const u32 id = wv_rl(o_txn, s), ilen = wv_rl(o_len, s);
          if (lane == s) o_used = false;
          if (lane == j) {
            t_cmp[id] = idx; t_first[id] = n + (u32)__popcll(im & ((1ull << j) - 1ull));
            if (jt == MSIM_T_OK) { t_off[id] = woff; t_lt[id] = len | (MSIM_T_OK << 16); }   // the completed form replaces the requested one
            else t_lt[id] = ilen | (jt << 16);
          }
          c_ok += jt == MSIM_T_OK; c_fail += jt == MSIM_T_FAIL; c_info += jt == MSIM_T_INFO;
        }
      }
