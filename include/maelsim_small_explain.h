/* maelsim_small_explain.h — the records and entries of the explained pn-counter / g-counter, unique-ids and echo verdicts.  maelsim.h
 * includes this file, no caller includes it on its own.  maelstrom_amd/_abi.py mirrors it in SMALL_EXPLAIN_RECORDS /
 * SMALL_EXPLAIN_PROTOTYPES.  The comments here are the contract: every record is defined by the history alone, never by how it is
 * found; the host walk (csrc/pn_check.cpp), the device kernels (pn_explain_kernel, unique_explain_kernel, echo_explain_kernel) and
 * tests/small_explain_ref.py give the same bytes.
 *
 * All three look at client rows only (process != MSIM_PROCESS_NEMESIS).  All three truncate as msim_explain_set_full does: the
 * segments of a history's slab are filled in their stated order, each with the room the ones before it left; `truncated` is 1 if a
 * record is missing; a capacity of 0 is legal and gives the header only; the records beyond the written counts are zero.  The true
 * counts stay where msim_check puts them, in msim_check_result. */
#ifndef MAELSIM_SMALL_EXPLAIN_H
#define MAELSIM_SMALL_EXPLAIN_H

/* ---- pn-counter / g-counter (workload/pn_counter.clj:84-125: :errors, :final-reads, :acceptable) ----------------------------------
 * A history's slab holds max_records records of 16 bytes in two segments:
 *   1. the final reads in row order: the rows with the final bit and type :ok (what attempt_count counts), each a msim_pn_read.
 *      :final-reads is their values, :errors the ops with in_set == 0.
 *   2. :acceptable — the maximal runs of consecutive acceptable integers as closed pairs, ascending (acceptable->vecs), each a
 *      msim_pn_range.  The acceptable set is {definite_sum} + every subset sum of the :info adds' deltas; stable_count is their number.
 * The reads come first: the worker threads bound them, the ranges are what a short slab should cut.  Every history has this
 * explanation, a valid one too (one without rows: no read, the range [0, 0]). */
typedef struct msim_pn_read {              /* 16 bytes */
  uint32_t row;                            /* row index into the history's rows (nemesis rows count) */
  int32_t value;                           /* the value read */
  uint32_t process;
  uint32_t in_set;                         /* 1: acceptable; 0: one of :errors */
} msim_pn_read;
typedef struct msim_pn_range {             /* 16 bytes */
  int64_t lower, upper;                    /* closed: lower <= v <= upper */
} msim_pn_range;
typedef struct msim_pn_explain {           /* 24 bytes, one per history */
  uint32_t n_reads, n_ranges;              /* records written to the history's slab: n_reads msim_pn_read, then n_ranges msim_pn_range */
  uint32_t truncated;                      /* 1: the slab was too short for all of them */
  uint32_t reserved;                       /* 0 */
  int64_t definite_sum;                    /* the sum of the :ok adds */
} msim_pn_explain;

/* ---- unique-ids ([upstream] jepsen.checker/unique-ids: :duplicated) ---------------------------------------------------------------
 * One record per packed :value of an :ok :generate that was acknowledged count >= 2 times (what duplicated_count counts), ordered by
 * count descending and, among equal counts, the larger packed id first: what (->> dups (sort-by val) reverse) yields over ids in
 * ascending order.  (jepsen's own order among equal counts follows a hash map; this order is the library's.)  A history without a
 * duplicate has a zero header. */
typedef struct msim_unique_dup {           /* 16 bytes */
  uint32_t id;                             /* the packed :value */
  uint32_t count;                          /* how often it was acknowledged */
  uint32_t first_row, second_row;          /* the rows of the first and the second :ok that carry it, by row index */
} msim_unique_dup;
typedef struct msim_unique_explain {       /* 8 bytes, one per history */
  uint32_t n_dups;                         /* records written */
  uint32_t truncated;
} msim_unique_explain;
#define MSIM_UNIQUE_EXPLAIN_MAX_DUPS 1024u /* unique_explain_kernel sorts this many duplicated ids in LDS; a history with more is the host walk's */

/* ---- echo (workload/echo.clj:44-63: :errors) --------------------------------------------------------------------------------------
 * One record per :echo invocation that error_count counts, in ascending invoke_row.  Invocation and completion are paired by worker
 * thread (process mod concurrency; a crashed process's successor is process + concurrency): a completion belongs to the thread's open
 * invocation.  An invocation whose completion is a :fail or an :info, one that never completes, and one whose :ok carries another
 * value are errors.  (A history in which a thread invokes again while its invocation is open — none of a jepsen run — forgets the open
 * one; a completion without an open invocation is passed over.)  A history without an error has a zero header. */
typedef struct msim_echo_error {           /* 16 bytes */
  uint32_t invoke_row;
  uint32_t complete_row;                   /* the :ok row that carries another value; MSIM_NO_VALUE: no completion, or not an :ok */
  uint32_t expected;                       /* the invocation's :value */
  uint32_t received;                       /* the :ok's; MSIM_NO_VALUE as complete_row */
} msim_echo_error;
typedef struct msim_echo_explain {         /* 8 bytes, one per history */
  uint32_t n_errors;                       /* records written */
  uint32_t truncated;
} msim_echo_explain;

/* Host-only, one history, no device needed: *out is what msim_check_pn_rows / msim_check_unique_rows write (echo: what msim_check
 * writes for the history), *hdr and records[0 .. max) as above (records may be NULL when the capacity is 0).  The verdict is the plain
 * walk's, which is handed the explanation as a sink. */
int msim_explain_pn_rows(const msim_op *rows, uint32_t n_rows, msim_check_result *out, msim_pn_explain *hdr, void *records, uint32_t max_records);
int msim_explain_unique_rows(const msim_op *rows, uint32_t n_rows, msim_check_result *out, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups);
int msim_explain_echo_rows(const msim_op *rows, uint32_t n_rows, uint32_t concurrency, msim_check_result *out, msim_echo_explain *hdr, msim_echo_error *errors, uint32_t max_errors);
/* As msim_check_pn_batch / msim_check_unique_batch / msim_check_set_full_batch for echo (the same slabs, out[i] and limits), with the
 * explanation written on the device: hdr[i], and history i's records at records + i * max (16 bytes each).  *n_host (may be null)
 * counts the histories the host walk explained instead, never approximated: a pn history whose window of acceptable values is 4096
 * wide or wider or that has more than 1024 :info adds; a unique-ids history of more than MSIM_UNIQUE_EXPLAIN_MAX_DUPS duplicated ids;
 * no echo history.  A unique-ids or echo batch without an unclean history launches what the plain entry launches and nothing else. */
int msim_explain_pn_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out,
                          msim_pn_explain *hdr, void *records, uint32_t max_records, uint32_t *n_host);
int msim_explain_unique_batch(int device, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories, msim_check_result *out,
                              msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups, uint32_t *n_host);
int msim_explain_echo_batch(int device, uint32_t concurrency, const msim_op *rows, const uint32_t *n_rows, uint32_t max_rows, uint32_t n_histories,
                            msim_check_result *out, msim_echo_explain *hdr, msim_echo_error *errors, uint32_t max_errors, uint32_t *n_host);
/* The same over the histories of the last run where they lie in HBM (a pn-counter or g-counter / unique-ids / echo context, else
 * MSIM_E_UNSUPPORTED): the arrays hold `n_out` histories (at least the run's, else MSIM_E_RANGE).  Towards the context each is
 * msim_check: msim_check_results holds the records msim_check writes, msim_check_host_rechecks counts the hand-overs. */
int msim_explain_pn(msim_ctx *ctx, msim_pn_explain *hdr, void *records, uint32_t max_records, uint32_t n_out);
int msim_explain_unique(msim_ctx *ctx, msim_unique_explain *hdr, msim_unique_dup *dups, uint32_t max_dups, uint32_t n_out);
int msim_explain_echo(msim_ctx *ctx, msim_echo_explain *hdr, msim_echo_error *errors, uint32_t max_errors, uint32_t n_out);

#endif /* MAELSIM_SMALL_EXPLAIN_H */
