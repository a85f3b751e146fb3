// txn_findings.inc — the findings flavour of txn_classify_kernel / rw_classify_kernel (txn_findings_kernel, rw_findings_kernel): the
// emission, the sort, the records of include/maelsim_txn_findings.h.  Text include of txn_check_dev.hip and rw_check_dev.hip, inside
// their namespaces (NONE, u32, u64 are theirs).  Kept at the top of a file of its own: the host wavefront emulator resolves lanes
// parked at different cross-lane operations lowest line first, and f_emit's lanes must go before the barrier the others wait at.
__device__ __forceinline__ u32 f_slot(u32 *cnt) {   // a slot for every lane that is here, one atomic for all of them
  const u64 here = __ballot(1);
  const u32 lane = threadIdx.x, leader = (u32)__builtin_ctzll(here);
  u32 base = 0;
  if (lane == leader) base = atomicAdd(cnt, (u32)__popcll(here));
  base = (u32)__shfl((int)base, (int)leader);
  return base + (u32)__popcll(here & ((1ull << lane) - 1ull));
}

// A history's region of the workspace, 8-byte aligned: the order keys [FCAP], the records [FCAP] as 12 words each, the wavefront's counter.
// The key packs the contract's order (bit position, key, inv_row, mop, count) into 64 bits: 4 | 12 (keys stay below KMAX) | 24 (the
// TRANSACTION: inv_row order is transaction order; none = all ones) | 16 (mop + 1: none sorts first, and a kind has it always or never)
// | 8 (count: it only decides between positions of a list, all below 254).  Two keys are equal only for two rows outside the payload
// area; the completion row decides between those.
constexpr u32 FCAP = MSIM_TXN_FINDINGS_CAPACITY, FREC = 12u;
constexpr u32 FWORDS = FCAP * (2u + FREC) + 2u;   // words of a region
struct FOut { msim_txn_explain *hdr; msim_txn_finding *recs; u32 max_findings; };   // the caller's slabs on the device
struct FRegion {
  u64 *keys; u32 *recs, *cnt;
  __device__ __forceinline__ explicit FRegion(u32 *behind) {   // (behind: the last table of the classification)
    keys = reinterpret_cast<u64 *>((reinterpret_cast<uintptr_t>(behind) + 7u) & ~(uintptr_t)7u);
    recs = reinterpret_cast<u32 *>(keys + FCAP); cnt = recs + FCAP * FREC;
  }
};
constexpr u32 F_G1A = 1u, F_G1B = 2u, F_INTERNAL = 6u, F_DUPLICATE = 7u, F_ORDER = 8u, F_DIRTY = 10u, F_VERSIONS = 11u;   // bit positions

// one finding, from divergent code: the lanes that are here take their slots together; beyond FCAP only the count goes on
__device__ __forceinline__ void f_emit(const FRegion &F, u32 bit, u32 key, u32 txn, u32 inv_row, u32 cmp_row, u32 mop, u32 o_inv, u32 o_cmp, u32 o_mop,
                                       u32 element, u32 o_element, u32 count) {
  const u32 s = f_slot(F.cnt);
  if (s >= FCAP) return;
  F.keys[s] = ((u64)bit << 60) | ((u64)(key & 0xFFFu) << 48) | ((u64)(txn & 0xFFFFFFu) << 24) | ((u64)((mop + 1u) & 0xFFFFu) << 8) | (u64)(count & 0xFFu);
  u32 *const r = F.recs + s * FREC;
  r[0] = 1u << bit; r[1] = key; r[2] = inv_row; r[3] = cmp_row; r[4] = mop; r[5] = o_inv; r[6] = o_cmp; r[7] = o_mop;
  r[8] = element; r[9] = o_element; r[10] = count; r[11] = 0;
}

// Behind the passes and a barrier, the whole wavefront: false = more findings than the region holds (the host walk's).  Else the records
// ranked by their keys — every lane counts the keys below its own — and the first max_findings written in order; the header with the
// true counts.
__device__ __forceinline__ bool f_finish(const FRegion &F, const FOut &o, u32 hist) {
  const u32 lane = threadIdx.x;
  const u32 nf = wv_max(atomicAdd(F.cnt, 0u));
  if (nf > FCAP) return false;
  u32 c1 = 0, c2 = 0, c6 = 0, c7 = 0, c8 = 0, c10 = 0, c11 = 0;
  for (u32 base = 0; base < nf; base += 64) {
    const u32 i = base + lane;
    const bool on = i < nf;
    const u64 mine = on ? F.keys[i] : 0ull;
    const u32 bit = (u32)(mine >> 60);
    c1 += (u32)__popcll(__ballot(on && bit == F_G1A)); c2 += (u32)__popcll(__ballot(on && bit == F_G1B)); c6 += (u32)__popcll(__ballot(on && bit == F_INTERNAL));
    c7 += (u32)__popcll(__ballot(on && bit == F_DUPLICATE)); c8 += (u32)__popcll(__ballot(on && bit == F_ORDER)); c10 += (u32)__popcll(__ballot(on && bit == F_DIRTY));
    c11 += (u32)__popcll(__ballot(on && bit == F_VERSIONS));
    if (on) {
      u32 rank = 0;
      for (u32 j = 0; j < nf; j++) { const u64 k = F.keys[j]; if (k < mine || (k == mine && F.recs[j * FREC + 3] < F.recs[i * FREC + 3])) rank++; }
      if (rank < o.max_findings) {
        u32 *const dst = reinterpret_cast<u32 *>(o.recs + (u64)hist * o.max_findings + rank);
        for (u32 w = 0; w < FREC; w++) dst[w] = F.recs[i * FREC + w];
      }
    }
  }
  if (lane == 0) {   // (the cycle bits' entries and the reserved words keep the zeros the slab was cleared to)
    msim_txn_explain *const h = o.hdr + hist;
    h->n_findings = min(nf, o.max_findings); h->truncated = nf > o.max_findings ? 1u : 0u;
    h->count[F_G1A] = c1; h->count[F_G1B] = c2; h->count[F_INTERNAL] = c6; h->count[F_DUPLICATE] = c7; h->count[F_ORDER] = c8; h->count[F_DIRTY] = c10; h->count[F_VERSIONS] = c11;
  }
  return true;
}
