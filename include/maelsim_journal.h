/* maelsim_journal.h — the net journal's messages: every :send joined to its :recv, and the counts and delivery latencies that
 * follow from the pairs.  maelsim.h includes this file, no caller includes it on its own.  maelstrom_amd/_abi.py mirrors it in
 * JOURNAL_RECORDS / JOURNAL_PROTOTYPES.  The comments here are the contract: every record is defined by the journal alone, never by
 * how it is found; the host walk (csrc/journal.cpp), the device kernel (journal_messages_kernel, csrc/journal_dev.hip) and
 * tests/journal_ref.py give the same bytes.
 *
 * What the reference does with a journal: net/checker.clj:28-70 folds it into the :net stats (send-count, recv-count, msg-count for
 * all messages, those that involve a client, and the rest), net/viz.clj:27-56 (`messages`) joins every :recv to its :send.
 *
 * An event (msim_event) is a :recv if bit 7 of `msg` is set, else a :send; its message id is msg >> 8, its :id its position in the
 * journal.  CLASSES.  A client is an endpoint e with n_nodes <= e < n_nodes + client_slots; everything else — the nodes and the
 * services behind the client slots (lin-kv, seq-kv, lww-kv, lin-tso) — is a server (util.clj:7-16).  An event is a `clients` event
 * if its src or its dest is a client, else a `servers` event.  Arrays of three are indexed all / clients / servers, arrays of two
 * clients / servers.  For a context client_slots = max(concurrency, n_nodes).
 *
 * THE WALK.  The events are taken in journal order with a map id -> the latest :send of that id.
 *   A :send gets the next record (msim_journal_msg; n_msgs counts them all, the first max_msgs are written) and becomes the latest
 *     send of its id; dup_sends counts the sends whose id was sent before.
 *   A :recv whose id has no send so far is counted in orphan_recvs (what viz.clj:51 asserts against).  Else it belongs to the latest
 *     send of its id: if that record has no recv yet, the recv becomes its recv_event and latency_us = time_us(recv) - time_us(send),
 *     0 where the recv's time is the smaller; else extra_recvs counts it.
 *   So a record's recv_event is the first :recv of its id behind the send and before the next send of the same id, MSIM_NO_VALUE
 *   if there is none: the message was lost, dropped by a partition at poll time, or still queued when the journal ends.
 * A record's class is its SEND's: undelivered[] counts the records without a recv, latency[] describes those with one.
 * send_count[] / recv_count[] count the events of a class, msg_count[] the distinct ids among the events of a class
 * (net/checker.clj:28-41).  endpoints has bit e set for every src and dest that occurs (viz.clj:18-25).
 * latency[c].q_us are the quantiles 0, .5, .95, .99, 1 of the class's latencies by the library's rule sorted[min(n - 1, floor(n * q))],
 * n * q an IEEE double product, as for msim_check_result.stable_latency_ms; sum_us their sum; all 0 for a class without a delivery.
 *
 * A journal is WELL-FORMED iff dup_sends == orphan_recvs == extra_recvs == 0 and every event's id is < n_events; `valid` says so.
 * (Every journal of the engine is: ids are dense from 0 and a message is journalled at its send first.)  The records, the counts and
 * the latencies are defined — and written — for a journal that is not, too.
 *
 * The summary is complete whatever max_msgs is; the records beyond min(n_msgs, max_msgs) are zero. */
#ifndef MAELSIM_JOURNAL_H
#define MAELSIM_JOURNAL_H

#define MSIM_JOURNAL_TRUNCATED 1u         /* the run produced more events than journal_capacity holds (msim_inst_meta.flags 0x20): the first journal_capacity events are analysed.  Set by msim_journal_messages only */
#define MSIM_JOURNAL_TABLE_TRUNCATED 2u   /* more sends than max_msgs: the first max_msgs records are written */

typedef struct msim_journal_msg {          /* 32 bytes: one per :send event, in journal order */
  uint32_t id;                             /* the message id */
  uint32_t send_event;                     /* position of the :send */
  uint32_t recv_event;                     /* position of its :recv; MSIM_NO_VALUE: none */
  uint32_t send_time_us;
  uint32_t latency_us;                     /* MSIM_NO_VALUE without a recv */
  uint32_t kind;                           /* the send's msg & 0x7F (MSIM_M_*), bit 7 set if a client is involved */
  uint32_t route, a;                       /* the send's words */
} msim_journal_msg;

typedef struct msim_journal_summary {      /* 192 bytes, one per journal */
  uint32_t valid;                          /* 1: well-formed */
  uint32_t n_events;
  uint32_t flags;                          /* MSIM_JOURNAL_* */
  uint32_t n_msgs;                         /* :send events = records, written or not */
  uint32_t send_count[3], recv_count[3], msg_count[3], undelivered[3];   /* all / clients / servers */
  uint32_t dup_sends, orphan_recvs, extra_recvs;
  uint32_t n_nodes, client_slots;          /* as given: what the classes were drawn by */
  uint32_t reserved[3];                    /* 0 */
  uint32_t endpoints[8];                   /* bit e of word e / 32: endpoint e occurs */
  msim_latency_dist latency[2];            /* clients / servers, over the records with a recv */
} msim_journal_summary;

/* Host only, one journal, no device needed: the walk above.  Exact for every journal.  msgs may be NULL when max_msgs is 0. */
int msim_journal_messages_rows(const msim_event *events, uint32_t n_events, uint32_t n_nodes, uint32_t client_slots, msim_journal_summary *summary,
                               msim_journal_msg *msgs, uint32_t max_msgs);
/* n_journals journals given on the host, journal i the events [event_offsets[i], event_offsets[i + 1]) of `events`, analysed on
 * `device`: summaries[i], and journal i's records at msgs + i * max_msgs, as msim_journal_messages_rows writes them.  *n_host (may
 * be NULL) counts the journals the host walk did instead: exactly those that are not well-formed — never approximated, and a
 * well-formed journal is never handed over.  MSIM_E_RANGE: a journal of 2^31 events or more. */
int msim_journal_messages_batch(int device, const msim_event *events, const uint64_t *event_offsets, uint32_t n_journals, uint32_t n_nodes, uint32_t client_slots,
                                msim_journal_summary *summaries, msim_journal_msg *msgs, uint32_t max_msgs, uint32_t *n_host);
/* The same over the journals of the last run where they lie in HBM (instance i's at i * journal_capacity, min(n_events,
 * journal_capacity) events), ordered behind the context's stream (msim_run_async): no msim_fetch is needed, none is made.  The arrays
 * hold `n_out` journals (at least the run's, else MSIM_E_RANGE; MSIM_E_RANGE before msim_run too); MSIM_E_UNSUPPORTED if
 * journal_capacity is 0.  It is not a check: msim_check_results, the check's time and a check queued behind the run stay as they are. */
int msim_journal_messages(msim_ctx *ctx, msim_journal_summary *summaries, msim_journal_msg *msgs, uint32_t max_msgs, uint32_t n_out);

/* Host-only utility: one journal as the Lamport diagram of net/viz.clj:281-325, an SVG document (UTF-8) — a column per endpoint, a row
 * per event, an arrow per delivered message.  Same calling convention as msim_history_edn_rows: cap == 0 only queries *needed.  Needs
 * no device.  The geometry is the reference's (viz.clj:60-108,145-259), computed in doubles and printed to four decimals:
 *   window     the events of type init / init_ok are dropped; of the rest, those at a position < 10000 + 4 n_nodes + 1 are looked at,
 *              the first 10000 of them drawn; more than 10000 left: the orange notice "Additional network events not shown".  An
 *              event's step is its index among the drawn ones + 1.
 *   columns    the endpoints that occur among the drawn events in sort-clients order (util.clj:18-28): c0 c1 .. n0 n1 .. then the
 *              services by name; x = (index + 1/2) / count * 1200, y(step) = 20 (1.5 + step), height = 20 (7 + steps).
 *   messages   one <g transform="translate(x0 y0) rotate(angle)"> per :recv whose :send of the same id lies among the drawn events,
 *              from (the send's src, its step) to (the recv's dest, its step): a <rect> of width length - 4 and height 5 at y = -2.5,
 *              filled #FF1E90 for an error body, #81BFFC when a client is involved, #000 otherwise, with a <title>; the arrowhead
 *              <use xlink:href="#ahead"> at x = length; the label twice (its glow, then the text) at x = length / 2, turned by
 *              rotate(180 length/2 0) when the angle is not within (-90, 90).
 *   furniture  every endpoint's name every 50 steps (#000 at step 0, #aaa after), a #ccc line per endpoint from y(0) to
 *              y(steps + 1), the arrowhead and glow definitions.
 * A deliberate difference: the label is the body's :type alone and the title "src → dest type".  The reference prints the body with
 * pr-str, whose order of keys is that of a Clojure map and cannot be pinned here. */
int msim_journal_svg_rows(const msim_config *cfg, const msim_event *events, uint32_t n_events, char *out, size_t cap, size_t *needed);

#endif /* MAELSIM_JOURNAL_H */
