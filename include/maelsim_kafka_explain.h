/* maelsim_kafka_explain.h — the records and entries of the explained kafka verdicts.  The contract (what a finding is, the order, the
 * truncation, the invariants) stands in maelsim.h above msim_check_unique_batch; maelsim.h includes this file, no caller includes it
 * on its own.  maelstrom_amd/_abi.py mirrors it in KAFKA_EXPLAIN_RECORDS / KAFKA_EXPLAIN_PROTOTYPES. */
#ifndef MAELSIM_KAFKA_EXPLAIN_H
#define MAELSIM_KAFKA_EXPLAIN_H

typedef struct msim_kafka_finding {        /* 32 bytes */
  uint32_t anomaly;                        /* exactly one MSIM_KAFKA_* bit */
  uint32_t key, offset, value, other;
  uint32_t row_a, row_b;                   /* row indices into the history's rows (nemesis rows count); MSIM_NO_VALUE = none */
  uint32_t reserved;                       /* 0 */
} msim_kafka_finding;
typedef struct msim_kafka_explain {        /* 48 bytes, one per history */
  uint32_t n_findings;                     /* records written to the history's slab */
  uint32_t truncated;                      /* 1: the slab was too short for all of them */
  uint32_t count[10];                      /* TRUE number of findings per anomaly, index = bit position; [9] (MALFORMED) is 0 or 1 */
} msim_kafka_explain;

/* Host-only: one kafka history by the plain walk of msim_check_kafka_rows' checker (csrc/kafka_check.cpp): *out is exactly what that
 * entry writes, *hdr and findings[0 .. max_findings) as above (findings may be NULL when max_findings is 0).  Needs no device. */
int msim_explain_kafka_rows(const msim_op *rows, uint32_t n_rows, const uint32_t *payload, uint32_t n_words, msim_check_result *out,
                            msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings);
/* As msim_classify_kafka_batch (the same arguments, records and error cases) with the explanation written on the device
 * (csrc/kafka_check_dev.hip, kafka_explain_kernel: one workgroup per history the clean pass cannot prove clean; a clean history costs
 * what it costs msim_check_kafka_batch): hdr[i], and history i's records at findings + i * max_findings.  Handed to
 * msim_explain_kafka_rows' walk, counted in *n_host (may be null) and never approximated: the three cases of msim_classify_kafka_batch,
 * an :ok send or a polled pair that names an offset or message >= 384 (the explaining tables take 357 bytes per offset of a CU's 160 KB), and a history
 * of more than 1024 findings (what the sort in LDS holds). */
int msim_explain_kafka_batch(int device, const msim_op *rows, const uint64_t *row_offsets, const uint32_t *payload, const uint64_t *payload_offsets,
                             uint32_t n_histories, uint32_t concurrency, msim_check_result *out, msim_kafka_explain *hdr,
                             msim_kafka_finding *findings, uint32_t max_findings, uint32_t *n_host);
/* The same over the histories of the last run where they lie in HBM (MSIM_WL_KAFKA, else MSIM_E_UNSUPPORTED): hdr / findings hold
 * `n_out` histories (at least the run's, else MSIM_E_RANGE).  Towards the context it is msim_check: msim_check_results holds the records
 * msim_check writes, msim_check_host_rechecks counts the hand-overs; with a concurrency beyond 64 (or the developer flag that keeps the
 * checks on the host cores) every history is explained by the host walk. */
int msim_explain_kafka(msim_ctx *ctx, msim_kafka_explain *hdr, msim_kafka_finding *findings, uint32_t max_findings, uint32_t n_out);

#endif /* MAELSIM_KAFKA_EXPLAIN_H */
