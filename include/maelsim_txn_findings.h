/* maelsim_txn_findings.h — the transactional checkers' NON-CYCLE anomalies, explained: one record per anomaly found, naming the
 * transaction, the micro-op, the key, what was read and who wrote it — what elle's result map carries as :internal, :G1a, :G1b,
 * :duplicate-elements, :incompatible-order, :dirty-update and :cyclic-versions (doc/05-datomic/01-single-node.md:117-144, :260-287,
 * :358-366; 02-shared-state.md:226-233).  The cycle classes keep their witness cycle (msim_explain_txn*, maelsim.h).  maelsim.h includes
 * this file, no caller includes it on its own.  maelstrom_amd/_abi.py mirrors it in TXN_FINDINGS_RECORDS / TXN_FINDINGS_PROTOTYPES.
 *
 * Everything below is defined without reference to how it is found, so the host walk (csrc/txn_check.cpp) and the device kernels
 * (txn_findings_kernel, rw_findings_kernel) give the same bytes.
 *
 * Vocabulary.  TRANSACTIONS are numbered by their :invoke among the client txn rows (a row whose payload lies outside the payload
 *   area is skipped).  A transaction's FORM is its completed micro-ops if it completed :ok, else the invoked ones; one never completed is
 *   :info.  writer(k, v) = the highest-numbered transaction whose form appends / writes v to k, of any type.  final(w, k) = the last
 *   append / write of w to k.  ext(m) of a list read = its length without the trailing elements whose writer is the reading transaction
 *   itself.  longest(k) = the first read of k, in (transaction, micro-op) order, of maximal length among the reads of :ok transactions;
 *   ord(k) = its list.  Only reads of :ok transactions are judged.  Rows are indices into the history's rows (nemesis rows count);
 *   `mop` is the micro-op's index in the transaction's form; "none" is MSIM_NO_VALUE.  inv_row / cmp_row are the subject transaction's
 *   :invoke and completion rows (cmp_row none = never completed), other_* those of the second party.
 *
 * List-append (MSIM_WL_TXN_LIST_APPEND), one finding per
 *   INTERNAL            a read m that fails the transaction's own test.  other_mop = the latest earlier read of the key in the form, or
 *                       none (other_inv_row / other_cmp_row are the transaction's own rows, or none alike); count = a = the transaction's
 *                       appends to the key since that read, or since the start.  With an earlier read the test is list(m) == list(prev)
 *                       ++ those appends; without one, list(m) must end with them.  element = len(list(m)), other_element =
 *                       len(list(prev)) or none.
 *                       A row whose payload lies outside the payload area gives one finding with cmp_row = that row; key, inv_row, mop
 *                       and every other_* field none, element / other_element none, count 0 (several such rows: in row order).
 *   G1A                 a read m and a position e < ext(m) whose element x has no writer or a :fail writer: element = x, count = e,
 *                       other rows = the writer's or none; other_mop, other_element none.
 *   G1B                 a read m with ext > 0, x = list(m)[ext - 1], w = writer(k, x) exists, is not the reader, final(w, k) != x:
 *                       element = x, other_element = final(w, k), other rows = w's, other_mop = the micro-op of that final append,
 *                       count = ext - 1.
 *   DUPLICATE_ELEMENTS  (a) a read holding an element twice, one finding per read: other_element = b, the lowest position repeating an
 *                       earlier one; count = a, the lowest position b repeats; element = list[b]; other rows, other_mop none.
 *                       (b) a (k, v) appended by more than one micro-op over all forms: the subject is the lowest (transaction, mop)
 *                       that appends it, the other the next one in that order; element = v, other_element none, count = how many
 *                       micro-ops append it.
 *   INCOMPATIBLE_ORDER  a read m whose list is not a prefix of ord(k): other rows and other_mop = longest(k)'s; count = the first
 *                       position where they differ (len(ord(k)) if ord(k) is a proper prefix of list(m)); element = list(m)[count];
 *                       other_element = ord(k)[count], or none beyond its end.
 *   DIRTY_UPDATE        a key k and a position i where writer(ord[i]) is :fail and writer(ord[i + 1]) exists and is not :fail: the
 *                       subject is the later writer, the other the failed one; element = ord[i + 1], other_element = ord[i], count = i,
 *                       both mop fields none.
 * rw-register (MSIM_WL_TXN_RW_REGISTER; a register value >= 64 is MSIM_E_INVALID, as for msim_explain_rw_rows), one finding per
 *   INTERNAL            a read with an earlier micro-op on its key that disagrees with the latest such one: other_mop = that micro-op
 *                       (other rows the transaction's own); element = the value read (none for nil), other_element = the value it had
 *                       to be (none for nil); count 0.  A row whose payload lies outside the area: as above.
 *   G1A                 an external (no earlier micro-op on the key) non-nil read of v with no writer or a :fail writer: element = v,
 *                       other rows = the writer's or none, other_mop / other_element none, count 0.
 *   G1B                 an external read of v whose writer w is not :fail, is not the reader, and final(w, k) != v: element = v,
 *                       other_element = final(w, k), other rows = w's, other_mop = the micro-op of that final write, count 0.
 *   DUPLICATE_ELEMENTS  as (b) above, over writes.
 *   CYCLIC_VERSIONS     a key whose version graph (nil precedes every version; an :ok transaction whose external read of a non-nil
 *                       v1 — no G1A finding — is followed by its final write v2 != v1 puts v1 before v2) has a cycle: element = the smallest version on a cycle (0 = nil),
 *                       count = how many versions are on one; everything else none.
 * Order.  Findings ascend by (bit position of `anomaly`, key, inv_row, mop, count), as unsigned numbers (none = 0xFFFFFFFF last).
 * Truncation.  The first max_findings in that order are written; truncated = 1 if one is missing; count[] is always the TRUE number.
 *   max_findings = 0 is legal (findings may then be NULL) and gives the header only.  Records beyond n_findings are zero.
 * Invariant.  count[i] > 0 iff bit i of the record's error_count is set, for the seven non-cycle bits; the cycle bits' entries are 0. */
#ifndef MAELSIM_TXN_FINDINGS_H
#define MAELSIM_TXN_FINDINGS_H

typedef struct msim_txn_finding {          /* 48 bytes */
  uint32_t anomaly;                        /* exactly one of MSIM_ANOMALY_G1A, _G1B, _INTERNAL, _DUPLICATE_ELEMENTS, _INCOMPATIBLE_ORDER, _DIRTY_UPDATE, _CYCLIC_VERSIONS */
  uint32_t key;
  uint32_t inv_row, cmp_row, mop;          /* the subject transaction (its :invoke row, its completion row) and the micro-op index in its form */
  uint32_t other_inv_row, other_cmp_row, other_mop;   /* the second party; MSIM_NO_VALUE = none */
  uint32_t element, other_element, count;
  uint32_t reserved;                       /* 0 */
} msim_txn_finding;
typedef struct msim_txn_explain {          /* 64 bytes, one per history */
  uint32_t n_findings;                     /* records written to the history's slab */
  uint32_t truncated;                      /* 1: the slab was too short for all of them */
  uint32_t count[12];                      /* TRUE number of findings per anomaly, index = bit position of MSIM_ANOMALY_*; the cycle bits' entries are 0 */
  uint32_t reserved[2];                    /* 0 */
} msim_txn_explain;

/* The findings of one history the device kernels hold before they sort them (a region of the workspace); a history with more is the
 * host walk's. */
#define MSIM_TXN_FINDINGS_CAPACITY 1024u

/* Host-only: one history (workload = MSIM_WL_TXN_LIST_APPEND or MSIM_WL_TXN_RW_REGISTER, else MSIM_E_INVALID) by the walk of
 * msim_check_txn_rows / msim_check_rw_rows judged under `consistency_model`: *out is exactly what those write, *hdr and
 * findings[0 .. max_findings) as above.  Needs no device. */
int msim_explain_txn_findings_rows(uint32_t workload, const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words,
                                   uint32_t consistency_model, msim_check_result *out, msim_txn_explain *hdr, msim_txn_finding *findings,
                                   uint32_t max_findings);
/* As msim_classify_txn_batch / msim_classify_rw_batch (the same histories, out[i] and error cases) with the findings written on the
 * device (txn_findings_kernel / rw_findings_kernel: one wavefront per history the clean passes cannot prove clean; a list-append
 * history they prove clean keeps the zero header and costs what it costs there): hdr[i], and history i's records at findings +
 * i * max_findings.  Handed to the host walk above, counted in *n_host (may be null) and never approximated: exactly the shapes
 * msim_classify_txn_batch / msim_classify_rw_batch hand over, and a history of more than MSIM_TXN_FINDINGS_CAPACITY findings. */
int msim_explain_txn_findings_batch(int device, uint32_t workload, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload,
                                    const uint64_t *payload_offsets, uint32_t n_histories, uint32_t consistency_model, msim_check_result *out,
                                    uint32_t *n_host, msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings);
/* The same over the histories of the last run where they lie in HBM, under the context's workload and consistency model: hdr /
 * findings hold `n_out` histories.  Towards the context it behaves as msim_explain_txn: the same refusals, msim_check_results left as
 * msim_check after msim_set_check_classify(ctx, 1) would leave them. */
int msim_explain_txn_findings(msim_ctx *ctx, msim_txn_explain *hdr, msim_txn_finding *findings, uint32_t max_findings, uint32_t n_out);

#endif /* MAELSIM_TXN_FINDINGS_H */
