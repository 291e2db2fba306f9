/*
 * hip_serial.h -- C ABI of the MI355X serializable-isolation conflict validator.
 *
 * This library replaces the read-set check of comdb2's SERIALIZABLE isolation:
 *
 *   reference entry   int bdb_osql_serial_check(bdb_state_type *, void *ranges,
 *                         unsigned int *file, unsigned int *offset, int regop_only);
 *                     bdb/bdb_api.h:1824-1826, bdb/serializable.c:571-579
 *   reference plugin  SERIALCHECK serial_check_callback(char *tbname, int idxnum,
 *                         void *key, int keylen, void *ranges)
 *                     bdb/bdb_api.h:336-337, db/glue.c:2926-2963
 *   reference walk    osql_serial_check / serial_check_this_txn
 *                     bdb/serializable.c:341-569, 60-332
 *
 * Instead of re-walking the log once per transaction and scanning every read
 * range per logged write key, the library keeps the committed-write window
 * resident in HBM (sorted by (group, key), deduplicated to the max commit LSN
 * per key) and answers a whole batch of read sets with one range-overlap join
 * written as hand-written HIP kernels for gfx950.
 *
 * Every entry point is plain C: pointers and sizes, no torch or HIP types.
 * Return codes: 0 = success, negative = HSC_E* error.  For the check entry
 * points, rc_out[i] keeps the reference meaning: 0 = serializable, nonzero =
 * not serializable (callers never distinguish errors from conflicts,
 * db/toblock.c:4779-4805); on any device error every rc_out[i] is set to 1
 * (fail closed, as bdb/serializable.c:94-104,417-421 do for log errors).
 */
#ifndef HIP_SERIAL_H
#define HIP_SERIAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * Read-set types.  Layout-identical mirrors of db/comdb2.h:1105-1124 so that a
 * comdb2 caller passes its own CurRangeArr* straight through (the `hash`
 * member built by currangearr_build_hash, db/sqlglue.c:312-351, is not read:
 * the library recomputes the same first-table / [begin,end] spans itself).
 * ------------------------------------------------------------------------ */
typedef struct hsc_currange {
    char *tbname;   /* NUL-terminated table name                              */
    int idxnum;     /* index number; -1 table scan; -2 default (currange_new) */
    void *lkey;     /* lower bound bytes (NULL or lkeylen bytes)              */
    void *rkey;     /* upper bound bytes                                      */
    int lflag;      /* 1: lower bound open (unbounded)                        */
    int lkeylen;
    int rflag;      /* 1: upper bound open                                    */
    int rkeylen;
    int islocked;   /* whole table read (full scan / both ends hit)           */
} hsc_currange;

typedef struct hsc_currangearr {
    int size;
    int cap;
    unsigned int file;   /* snapshot LSN (bdb_get_current_lsn at begin)       */
    unsigned int offset;
    void *hash;          /* ignored                                           */
    hsc_currange **ranges;
} hsc_currangearr;

/* ---------------------------------------------------------------------------
 * Log record stream, decoded to struct-of-arrays.  One row per log record, in
 * LSN order -- the view bdb/serializable.c gets from DB_LOGC->get plus the
 * generated llog_*_read decoders (bdb/llog.src:26-225).  Keys of undo_add_ix /
 * undo_del_ix[_lk] are the ones bdb_reconstruct_add/delete would recover
 * (bdb/rowlocks.c:428-617).
 * ------------------------------------------------------------------------ */
enum {
    HSC_REC_TXN_REGOP = 10,          /* berkdb/dbinc_auto/txn_auto.h:6        */
    HSC_REC_TXN_REGOP_ROWLOCKS = 15, /* txn_auto.h:59                         */
    HSC_REC_TXN_REGOP_GEN = 16,      /* txn_auto.h:76                         */
    HSC_REC_UNDO_ADD_DTA = 10003,    /* bdb/llog.src:26                       */
    HSC_REC_UNDO_ADD_IX = 10004,
    HSC_REC_LTRAN_COMMIT = 10005,
    HSC_REC_LTRAN_START = 10006,
    HSC_REC_LTRAN_COMPREC = 10007,
    HSC_REC_UNDO_DEL_DTA = 10008,
    HSC_REC_UNDO_DEL_IX = 10009,
    HSC_REC_UNDO_UPD_DTA = 10010,
    HSC_REC_UNDO_UPD_IX = 10011,
    HSC_REC_UNDO_ADD_DTA_LK = 10013,
    HSC_REC_UNDO_ADD_IX_LK = 10014,
    HSC_REC_UNDO_DEL_DTA_LK = 10015,
    HSC_REC_UNDO_DEL_IX_LK = 10016,
    HSC_REC_UNDO_UPD_DTA_LK = 10017,
    HSC_REC_UNDO_UPD_IX_LK = 10018,
    /* berkdb physical records the index-key reconstruction walks
     * (bdb/rowlocks.c:209-426; layouts berkdb/db/db.src) */
    HSC_REC_DB_ADDREM = 41,          /* db.src:47-57                          */
    HSC_REC_DB_BIG = 43,             /* db.src:73-83                          */
    HSC_REC_DB_DEBUG = 47,           /* db.src:131                            */
    HSC_REC_DB_PG_FREE = 50,         /* db.src:177-184                        */
    HSC_REC_DB_PG_FREEDATA = 52      /* db.src:206-214                        */
};

typedef struct hsc_llog {
    size_t nrec;
    const uint64_t *lsn;      /* (file << 32) | offset, strictly increasing   */
    const uint32_t *rectype;  /* HSC_REC_*                                    */
    const uint64_t *prev;     /* regop*: prev_lsn; llog records: prevllsn     */
    const int16_t *isabort;   /* ltran_commit: isabort                        */
    const int32_t *table;     /* llog undo records: index into tbnames        */
    const int16_t *ix;        /* undo_*_ix*: index number (short on disk)     */
    const uint64_t *key_off;  /* undo_*_ix*: key byte offset into keys        */
    const int32_t *keylen;    /* undo_*_ix*: key length                       */
    const uint8_t *keys;
    const char *const *tbnames;
    int ntbnames;
    uint64_t end_lsn;         /* __log_txn_lsn (berkdb/log/log_put.c:509)     */
} hsc_llog;

/* ---------------------------------------------------------------------------
 * Flat read sets: many CurRangeArr's as struct-of-arrays (the OSQL_SERIAL
 * payload of db/osqlcomm.c:909-993 after decode, without heap CurRange's).
 * Ranges of read set t are rows [txn_off[t], txn_off[t+1]) in array order.
 *
 * Key pointers: lkey_off / rkey_off == HSC_KEY_NULL stands for a NULL key
 * pointer (its length must be 0; currange_new leaves keys NULL,
 * db/sqlglue.c:163-175); any other offset is a present key, also with length
 * 0 (serial_readset_get malloc(0)s one, db/osqlcomm.c:974).  Only the
 * coalesce comparator tells them apart: currange_cmp compares the lower keys
 * only when both pointers are non-NULL (db/sqlglue.c:228-236), so a NULL one
 * ties with every range of its index while a present empty key sorts before
 * the longer ones.  The check itself reads at most min(len, keylen) bytes and
 * treats both alike (db/glue.c:2951-2958).
 * ------------------------------------------------------------------------ */
#define HSC_KEY_NULL UINT64_MAX
typedef struct hsc_readsets {
    int ntxn;
    const int64_t *txn_off;   /* [ntxn+1]                                     */
    const uint64_t *snap;     /* [ntxn] snapshot LSN (file << 32 | offset)    */
    const int32_t *table;     /* [nranges] index into tbnames                 */
    const int32_t *idxnum;
    const int32_t *lflag, *rflag, *islocked;
    const int32_t *lkeylen, *rkeylen;
    const uint64_t *lkey_off, *rkey_off; /* byte offsets into keys           */
    const uint8_t *keys;
    const char *const *tbnames;
    int ntbnames;
} hsc_readsets;

/* OSQL_SERIAL payloads (one read set each) as the master receives them:
 * message i = buf[off[i] .. off[i] + len[i]), starting at the osql_serial_t
 * header (buf_size, arr_size, file, offset; db/osqlcomm.c:748-753,809-826)
 * followed by the serial_readset_put ranges (db/osqlcomm.c:909-946).  Every
 * 2/4/8-byte item is byte-swapped on the wire (buf_put,
 * bbinc/endian_core.amd64.h:17-44) -- keys and table names of those lengths
 * included. */
typedef struct hsc_serial_msgs {
    size_t nmsg;
    const uint8_t *buf;
    const uint64_t *off;
    const uint64_t *len;
} hsc_serial_msgs;

/* Decoded committed write (what serial_check_this_txn hands the callback). */
typedef struct hsc_write {
    const char *tbname;
    int idxnum;          /* -2 for dta records (key == NULL)                  */
    const void *key;     /* NULL for dta records                              */
    int keylen;
    uint64_t commit_lsn; /* LSN of the txn's regop record                     */
} hsc_write;

/* Device-resident probe batch (what the check entry points lower to).  All
 * pointers are device pointers on the context's GPU.  Key words are the key
 * bytes in big-endian 8-byte words, zero padded, held as native uint64 so that
 * numeric order of the words equals memcmp order of the bytes. */
typedef struct hsc_probe_batch {
    size_t n;                 /* range probes                                  */
    const uint64_t *lo;       /* [words][n]                                    */
    const uint64_t *hi;       /* [words][n]                                    */
    const uint32_t *gid;      /* [n] key group (table, index, key length)      */
    const uint64_t *snap;     /* [n] snapshot LSN of the owning read set       */
    const uint32_t *txn;      /* [n] read-set (transaction) index              */
    size_t n_lock;            /* table-lock probes                             */
    const uint32_t *lock_table;
    const uint64_t *lock_snap;
    const uint32_t *lock_txn;
    size_t n_txn;
    uint8_t *verdict;         /* [n_txn] out: 1 = not serializable             */
    uint64_t *bitmap;         /* [ceil(n_txn/64)] out (may be NULL)            */
} hsc_probe_batch;

/* Per-kernel device time of the last probe / window build, in ms.  Wide
 * layout: locate, plan, scatter, join, pack kernels.  Narrow layout: locate =
 * verdict clear, join = the single probe kernel, pack; plan = scatter = 0. */
typedef struct hsc_timing {
    float locate_ms, plan_ms, scatter_ms, join_ms, pack_ms, probe_total_ms;
    float ingest_ms;
    uint64_t records;         /* join records emitted by the last probe         */
    uint64_t tiles;           /* tiles in the resident window                   */
} hsc_timing;

typedef struct hsc_ctx hsc_ctx;

enum {
    HSC_OK = 0,
    HSC_EINVAL = -1,
    HSC_EDEVICE = -2,
    HSC_ENOMEM = -3,
    HSC_ELOG = -4,     /* malformed log stream (unknown record, broken link)  */
    HSC_ESTATE = -5    /* window not built                                    */
};

/* ---- context ------------------------------------------------------------ */
/* device = -1 creates a host-only context: log decode, dictionaries and
 * marshalling work; every device operation returns HSC_EDEVICE. */
int hsc_ctx_create(int device, hsc_ctx **out);
void hsc_ctx_destroy(hsc_ctx *ctx);
/* Launch on this hipStream_t (NULL = the context's own stream).  Probes are
 * stream-ordered on the stream current at the call.  Each stream that probes
 * gets its own probe lane (scratch buffers, up to 4 lanes; a fifth stream
 * takes over the least recently used lane after waiting for that lane's last
 * batch), so batches probed on different streams may run concurrently.
 * Window builds wait for every lane's last batch; the caller orders a window
 * change against later probes on other streams.  A stream stays in use by the
 * context until the next hsc_set_stream (which records its lane's fence on
 * it) or hsc_ctx_destroy: keep it valid until then. */
int hsc_set_stream(hsc_ctx *ctx, void *hip_stream);
const char *hsc_last_error(hsc_ctx *ctx);
int hsc_device_count(void);

/* ---- write window (replaces the per-call log walk) ---------------------- */
/* Decode a log stream: every committed write txn (regop whose prev record is
 * an ltran_commit with isabort == 0 and prevllsn.file != 0,
 * bdb/serializable.c:426-534) contributes its logical records' (table, ix,
 * key) at the regop's LSN.  Replaces the window. */
int hsc_window_ingest_log(hsc_ctx *ctx, const hsc_llog *log);
/* Raw log records as a log cursor returns them (DB_LOGC->get data): the
 * bdb/llog.src:26-225 layouts, the txn regop records
 * (berkdb/dbinc_auto/txn_auto.h:6-86) and any berkdb physical records, in the
 * gen_rec_endian.awk on-disk encoding of a little-endian host: u32/short
 * fields and DB_LSNs big-endian, genid_t native, DBT = u32 BE size + bytes.
 * Record i is lsn[i] (strictly increasing), bytes buf[off[i] .. off[i] +
 * len[i]).  undo_add_ix / undo_del_ix / undo_del_ix_lk carry no key: the
 * reference rebuilds it from the physical log at undolsn = the record's header
 * prev_lsn (bdb/serializable.c:123-130,174-181), walking the header prev_lsn
 * chain over __db_addrem / __db_big / __db_pg_free[data] records
 * (bdb_reconstruct_add / _delete, bdb/rowlocks.c:209-617); the decoder runs
 * the same walk over the records of this log and, for appends, of every raw
 * log decoded since the last ingest.  A key the walk does not fully define
 * (the reference would read its uninitialised key buffer) is HSC_ELOG.
 * recon_* (optional, sorted by undolsn) supplies keys directly: an entry for
 * a record's undolsn takes precedence over the walk. */
typedef struct hsc_raw_log {
    size_t nrec;
    const uint64_t *lsn;
    const uint64_t *off;
    const uint32_t *len;
    const uint8_t *buf;
    uint64_t end_lsn;
    size_t nrecon;
    const uint64_t *recon_lsn;
    const uint64_t *recon_off;
    const int32_t *recon_len;
    const uint8_t *recon_keys;
} hsc_raw_log;
/* Decode + ingest (replaces the window), = hsc_window_ingest_log of the
 * decoded stream. */
int hsc_window_ingest_raw(hsc_ctx *ctx, const hsc_raw_log *log);
/* Decode only: *out points at a context-owned hsc_llog valid until the next
 * decode on this context. */
int hsc_decode_log(hsc_ctx *ctx, const hsc_raw_log *log, const hsc_llog **out);
/* Append decoded writes (commit_lsn non-decreasing across calls).  On a
 * built window (log, raw, staged or device ingest) the rows go to a sorted
 * delta run on the device (one merge launch per call; the reference sees
 * every commit up to the end of the log on every check, bdb/serializable.c:
 * 390-539, and commits keep appending, bdb/tran.c:1545-1560) that every probe
 * checks beside the main window; past 65536 delta rows, or on a key longer
 * than the window's words, the next check folds the delta into the main
 * window with one device rebuild.  Decoded writes carry no record LSNs, so
 * after one the DB_SET-on-a-non-record rule (bdb/serializable.c:417-421) is
 * off for the window.  The window's end LSN advances to at least
 * commit_lsn + 1 of every appended write (a snapshot at or past the old end
 * must still see it: fail closed); hsc_window_set_end sets the exact end of
 * the log (curlsn of full checks). */
int hsc_window_append(hsc_ctx *ctx, const hsc_write *w, size_t n);
/* Append log records: the continuation of the window's log (LSNs above every
 * record taken so far; log->end_lsn is the new end).  Every txn a new regop
 * commits contributes its writes, its logical chain walked back into records
 * of earlier ingests / appends when it reaches them (SURVEY.md §8(f) 1,
 * incremental decode); record LSNs, poison rules and the delta run follow. */
int hsc_window_append_log(hsc_ctx *ctx, const hsc_llog *log);
/* Raw-record form of hsc_window_append_log (hsc_raw_log as for ingest). */
int hsc_window_append_raw(hsc_ctx *ctx, const hsc_raw_log *log);
/* Rows in the delta run (appended since the last build of the main window). */
size_t hsc_window_delta_rows(hsc_ctx *ctx);
/* Delta folding.  Appended rows live in a sorted delta run beside the main
 * window; once it holds `rows` rows (0 = the default, half the run's
 * capacity of 65536) it is folded into the main window.  background = 1
 * (default): the run is frozen and the main window rebuilt with it on a
 * second stream and host thread while checks go on against the old window +
 * frozen run + a fresh run; the rebuilt window is swapped in by the first
 * call after it finished.  background = 0: the next check merges the run
 * inline (a full rebuild on the check's path). */
int hsc_set_fold(hsc_ctx *ctx, size_t rows, int background);
/* out[4]: background folds started, background folds swapped in, inline
 * merges, build time of the last background fold in microseconds. */
int hsc_fold_stats(hsc_ctx *ctx, uint64_t out[4]);
/* The pending tail (narrow windows whose keys fit 4 words): an append's rows
 * are mirrored into mapped host memory that the small-batch kernel scans
 * beside the delta runs, and merged into the live run once 256 rows wait or a
 * batch that is not small runs.  out[3]: appends kept in the tail, merges of
 * the tail into the run, rows waiting now. */
int hsc_append_stats(hsc_ctx *ctx, uint64_t out[3]);
/* Path restrictions of one context, for tests and A/B runs (0 = every path
 * the library picks by itself).  NO_SMALL: batches skip the small-batch
 * kernel (and appends its pending tail); NO_PACKED_SORT: window builds use
 * the whole-row radix sort; TILE_DIR: narrow / compact tile locates search
 * the 16-ary directory instead of the bucket table (set before the build);
 * CO_SERIAL: every coalesced read set takes the per-thread msort replay;
 * CO_RUN_THREAD: one thread per run in the coalesce merge scan;
 * NO_COMP_NARROW: composite keys whose varying bits total <= 62 but span
 * more keep the compact / wide layouts instead of the narrow index over
 * compressed codes (set before the build); NO_CT_POINTS: compact tiles build
 * no point index, so point probes take join records (set before the build). */
#define HSC_PATH_NO_SMALL 1u
#define HSC_PATH_NO_PACKED_SORT 2u
#define HSC_PATH_TILE_DIR 4u
#define HSC_PATH_CO_SERIAL 8u
#define HSC_PATH_CO_RUN_THREAD 16u
#define HSC_PATH_NO_COMP_NARROW 32u
#define HSC_PATH_NO_CT_POINTS 64u
#define HSC_PATH_ALL 127u
int hsc_set_paths(hsc_ctx *ctx, unsigned flags);
/* How the last window build sorted its rows: 0 whole-row radix sort, 1 the
 * packed 64-bit key sort, 2 the compact-code merge sort (wide keys). */
int hsc_window_sort_path(hsc_ctx *ctx);
int hsc_window_set_end(hsc_ctx *ctx, uint64_t end_lsn);
int hsc_window_reset(hsc_ctx *ctx);
/* Sort + dedupe + summaries on the device; implied by the check calls. */
int hsc_window_build(hsc_ctx *ctx);
/* Register a key group ahead of a device-side ingest; returns gid >= 0. */
int hsc_register_group(hsc_ctx *ctx, const char *tbname, int idxnum, int keylen);
/* Device-side ingest of pre-padded keys (bench / sharded driver path):
 * gid[n], words[words][n], lsn[n] are DEVICE pointers, keys already packed as
 * described for hsc_probe_batch; gid values come from hsc_register_group.
 * Rows are versions in log order: of equal (gid, key) rows the last one is
 * the key's newest version.  Replaces the window. */
int hsc_window_ingest_device(hsc_ctx *ctx, size_t n, int words,
                             const uint32_t *gid, const uint64_t *key_words,
                             const uint64_t *lsn, uint64_t end_lsn);
/* Window layout.  AUTO: the narrow layout -- every (group, key) as one
 * 62-bit code under a 16-ary index, each range answered by one probe kernel
 * without bucketing -- whenever the whole window fits it (any single int64
 * index, any single group of keys whose varying bits span < 62 bits), else
 * WIDE (every key as its big-endian words, ranges bucketed by window tile).
 * A narrow window answers a sparse batch (< 8 ranges per 2048-row tile) with
 * one direct probe kernel and a dense one with the tile pipeline over codes.
 * A dense batch runs on 8-byte tile rows (u32 key delta, u32 commit rank)
 * when every 4096-row tile spans < 2^32 codes, else on the codes as 16-byte
 * rows.  WIDE forces the wide layout; NARROW_DIRECT / NARROW_TILES /
 * NARROW_CODES keep AUTO's layout choice but force that probe path (tiles:
 * 8-byte rows where they fit; codes: always 16-byte code rows) -- testing.  Verdicts are
 * identical; a change between WIDE and the others applies at the next window
 * build (host-staged windows rebuild; a device-ingested window returns
 * HSC_ESTATE and must be re-ingested).  hsc_window_layout reports WIDE,
 * NARROW or COMPACT (AUTO on a window too wide for 62-bit codes: each
 * (table, index, key length) group's keys keep only the bits that vary inside
 * the group -- hsc_compact.hip -- when that shortens the rows; WIDE disables
 * it). */
enum {
    HSC_LAYOUT_AUTO = 0,
    HSC_LAYOUT_WIDE = 1,
    HSC_LAYOUT_NARROW = 2,
    HSC_LAYOUT_NARROW_DIRECT = 3,
    HSC_LAYOUT_NARROW_TILES = 4,
    HSC_LAYOUT_NARROW_CODES = 5,
    HSC_LAYOUT_COMPACT = 6, /* reported only: AUTO's wide window as per-group compact codes */
    HSC_LAYOUT_COMPACT_WIDE = 7 /* AUTO, but compact windows probe through the wide tile
                                   pipeline instead of the compact tiles -- testing */
};
int hsc_set_layout(hsc_ctx *ctx, int layout);
int hsc_window_layout(hsc_ctx *ctx);         /* HSC_LAYOUT_WIDE, _NARROW or _COMPACT */
int hsc_window_code_words(hsc_ctx *ctx);     /* words per probed row (compact: WC) */
/* Compact windows: words of the compact-tile keys gid || code (1..3) that
 * dense batches probe (hsc_ctiles.hip), 0 if the window has none. */
int hsc_window_tile_key_words(hsc_ctx *ctx);
int hsc_window_words(hsc_ctx *ctx);          /* key words per key (>= 1)     */
size_t hsc_window_keys(hsc_ctx *ctx);        /* distinct (group, key) rows   */
uint64_t hsc_window_end(hsc_ctx *ctx);
uint64_t hsc_window_max_commit(hsc_ctx *ctx);
/* Window snapshot (checkpoint of the resident state; the reference keeps
 * none -- its state is the log): the rows of the built window in (group, key)
 * order, after folding any delta run.  all_versions = 0: one row per (group,
 * key), its newest version; 1: every version.  gid[cap], key_words[words *
 * cap] (word j of row i at [j * cap + i], big-endian key order), lsn[cap];
 * all three NULL returns only the count.  Returns the row count (> cap:
 * nothing copied) or a negative HSC_E* code. */
long hsc_window_export(hsc_ctx *ctx, int all_versions, uint32_t *gid, uint64_t *key_words,
                       uint64_t *lsn, size_t cap);
int hsc_table_id(hsc_ctx *ctx, const char *tbname); /* -1 if never written   */
const char *hsc_table_name(hsc_ctx *ctx, int table_id); /* NULL if unknown   */
/* Key group gid -> (table id, index, key length); 0 or HSC_EINVAL. */
int hsc_group_info(hsc_ctx *ctx, int gid, int *table_id, int *idxnum, int *keylen);
/* Per-table max commit LSN (dta writes included): copies min(n, ntables)
 * entries, returns ntables. */
int hsc_table_max(hsc_ctx *ctx, uint64_t *out, int n);
/* Max-merge per-table LSNs from other shards (multi-GPU lock probes). */
int hsc_merge_table_max(hsc_ctx *ctx, const uint64_t *in, int n);

/* ---- drop-in checks ----------------------------------------------------- */
/* Exactly bdb_osql_serial_check (bdb/serializable.c:571-579) for one read set:
 * ranges == NULL -> 0; regop_only -> nonzero iff a committed write txn follows
 * (*file,*offset); otherwise (*file,*offset) := end LSN, then the full check.
 * Concurrent callers (one per committing transaction, db/toblock.c:4777-4800)
 * are batched by a collector the context owns (hsc_collector_check below):
 * a lone caller runs its own single-set pass, callers that arrive while a pass
 * runs form the next one -- none waits on another's context lock.
 * hsc_set_autocollect(ctx, 0) makes every call its own pass instead. */
int hip_bdb_osql_serial_check(void *ctx, void *ranges, unsigned int *file,
                              unsigned int *offset, int regop_only);
/* regop_only (here, in hip_serial_check_batch and hsc_collector_check) is
 * answered in the caller's thread from a snapshot (end LSN, max commit LSN,
 * unreadable-regop LSN, DB_SET rule) that every entry changing the window
 * republishes before it returns: no collector queue, no context lock, no
 * window build (db/toblock.c:4779-4785 probes under the commit_lock write
 * lock).  Only a snapshot the published values cannot decide -- no commit
 * after it, inside a log whose record LSNs must be searched -- takes the
 * locked path.  out[0] = probes answered from the snapshot, out[1] = locked. */
int hsc_regop_stats(hsc_ctx *ctx, uint64_t out[2]);
/* The drop-in entry through the context's own collector (1, the default) or
 * one pass per call (0).  0 or HSC_EINVAL. */
int hsc_set_autocollect(hsc_ctx *ctx, int on);
/* n read sets in one device pass.  ranges[i] is a CurRangeArr* (may be NULL);
 * file/offset are arrays of n in/out snapshot LSNs, or NULL to use (and
 * update) ranges[i]->file / ->offset in place.  Per element the semantics and
 * side effects of the single call.  Returns 0 or a negative HSC_E* code. */
int hip_serial_check_batch(void *ctx, void *const *ranges, unsigned int *file,
                           unsigned int *offset, int regop_only, int n,
                           int *rc_out);
/* Batching collector for concurrent callers (the reference calls
 * bdb_osql_serial_check from every block-processor thread, db/toblock.c:
 * 4779-4836).  hsc_collector_check has bdb_osql_serial_check's signature and
 * contract for one read set; calls that arrive together are run as one
 * hip_serial_check_batch by one of their callers (group-commit leader: it
 * takes every queued call, up to max_batch -- 0 = 65536 -- after waiting up to
 * max_wait_us for more to arrive; 0 = no wait, batches form while the previous
 * one runs).  Thread-safe; destroy only after every caller has returned. */
typedef struct hsc_collector hsc_collector;
typedef struct hsc_collector_stats {
    uint64_t calls;      /* hsc_collector_check calls that queued */
    uint64_t batches;    /* device passes run for them */
    uint64_t max_batch;  /* largest batch */
    uint64_t busy_ns;    /* wall time with at least one batch in flight (the union of
                            the passes' intervals: busy_ns / elapsed <= 1) */
    uint64_t gate_ns;    /* leaders waiting for a device pass to end (in-flight bound) */
    uint64_t handout_ns; /* leaders waking their batches' callers */
    uint64_t pass_ns;    /* sum of the passes' durations (> busy_ns when they overlap) */
} hsc_collector_stats;
/* Small-batch path (batches of <= 1024 read sets over a narrow window: one
 * k_small_narrow launch over fine-grained host memory) phase totals since
 * the context was created: host marshal, slot copy + launch, and the wait
 * for the kernel's done word (hip_serial_check_batch releases the context
 * lock while it waits, so concurrent callers overlap). */
typedef struct hsc_small_stats_t {
    uint64_t calls, marshal_ns, launch_ns, wait_ns;
    uint64_t slot_waits; /* launches that found every slot in flight */
    uint64_t lock_ns;    /* hip_serial_check_batch calls (any path) waiting for the context lock */
} hsc_small_stats_t;
int hsc_small_stats(hsc_ctx *ctx, hsc_small_stats_t *out);
/* Marshal and batch phase totals since the context was created: marshal
 * calls (one per pipeline chunk), read sets, range probes written; the
 * parallel walk of the read sets into per-worker parts (CurRange pointer
 * walk, dictionary lookups, bound padding), the staging allocation, the SoA
 * assembly; and for the staged path the upload + launch and the wait for a
 * chunk's verdicts (device time + transfers not hidden behind the next
 * chunk's marshal).  column_batches / plan_batches: dense batches over a
 * narrow window whose join scanned its tiles' columns itself / that ran the
 * plan kernel first.  The rule, stated once: a batch is concentrated when
 * some tile received more than 1024 located records -- the records the
 * locate's end-tile step gave the tile, counted before any filter drops one --
 * and a concentrated batch sends the next 64 down the plan path.  fast_locates / general_locates: launches of
 * the narrow-tile locate by instance -- one built for the window's shape (1
 * or 2 key words, the last one varying, bucket table, no compressed codes,
 * 32-bit commit ranks) / the one that reads the shape at run time.
 * full_tile_joins: join blocks and overflow items of the narrow tiles that
 * staged a whole 4096-row tile because a record's snapshot was older than a
 * row outside the tile's recent list (the rest answered from the list of the
 * tile's 256 newest rows); a device counter, read when this is called. */
typedef struct hsc_batch_stats_t {
    uint64_t marshals, read_sets, ranges;
    uint64_t parts_ns, alloc_ns, assemble_ns, launch_ns, wait_ns;
    uint64_t column_batches, plan_batches;
    uint64_t fast_locates, general_locates;
    uint64_t full_tile_joins;
} hsc_batch_stats_t;
int hsc_batch_stats(hsc_ctx *ctx, hsc_batch_stats_t *out);
/* The join kernel of the column batches (column_batches above), since the
 * context was created.  wave_batches: joined a wave per tile, 8 tiles per
 * block; block_batches: joined a 512-thread block per tile; their sum is
 * column_batches.  A wave joins a tile of at most 128 records that the
 * locate's filter kept, all answered from the tile's recent list; any other
 * tile falls back to the whole block, in the same launch
 * (wave_fallback_tiles: a device counter, read when this is called).  The
 * rule, stated once: a batch is wide when some block fell back for 3 or more
 * of its 8 tiles, and a wide batch sends the next 64 column batches to the
 * block-per-tile join.  Batches whose locate was the general instance always
 * take it.  Both joins give the same verdicts. */
typedef struct hsc_join_stats_t {
    uint64_t wave_batches, block_batches;
    uint64_t wave_fallback_tiles;
} hsc_join_stats_t;
int hsc_join_stats(hsc_ctx *ctx, hsc_join_stats_t *out);

int hsc_collector_create(hsc_ctx *ctx, int max_batch, int max_wait_us, hsc_collector **out);
void hsc_collector_destroy(hsc_collector *col);
int hsc_collector_check(hsc_collector *col, void *ranges, unsigned int *file,
                        unsigned int *offset, int regop_only);
int hsc_collector_get_stats(hsc_collector *col, hsc_collector_stats *out);
/* Batches allowed on the device at once (1..8; default 4): their small-batch
 * kernels run side by side on streams of their own, and the next leader
 * marshals and launches while earlier batches' kernels run.  Full checks are
 * marshalled by their own callers before they queue. */
int hsc_collector_set_inflight(hsc_collector *col, int n);
/* Read/write conflict pairs before the OR-reduction:
 * every (read set t, writer commit LSN c) such that a write committed at c
 * (c > t's snapshot) has a key inside one of t's ranges -- all the pairs the
 * A0 join would find if serial_check_callback did not stop at the first hit
 * (db/glue.c:2926-2963), i.e. the rw-antidependency edges t -> writer.
 * Sorted by (t, c), unique.  Range probes only: table locks and the host-side
 * window rules (forced verdicts) yield a verdict but no pairs.  Output arrays
 * are owned by the context until its next call. */
int hsc_rw_edges(hsc_ctx *ctx, const hsc_readsets *rs, size_t *n_pairs, const uint32_t **txn,
                 const uint64_t **writer_lsn);

/* Replicant read-set coalesce on the device: currangearr_coalesce
 * (db/sqlglue.c:305-311) -- qsort by currange_cmp (:206-242, glibc's
 * top-down merge sort), currangearr_merge_neighbor (:247-304), twice -- of
 * every read set, with the reference's quirks (a right-key swap keeps the
 * surviving range's rkeylen; a range open at both ends becomes a table lock
 * that absorbs its table's other ranges).  Output arrays are owned by the
 * context until its next coalesce; key offsets point into rs->keys.  Every
 * range must name a table (the reference's strcmp would crash otherwise).
 * Sets of >= 256 ranges whose comparator is a consistent order (no unlocked
 * range with a present-but-empty lower key; locked ranges open at both ends)
 * sort and merge level-parallel with the same result; HSC_CO_SERIAL=1 in the
 * environment forces the per-set path (testing). */
typedef struct hsc_coalesced {
    int ntxn;
    const int64_t *txn_off;   /* [ntxn+1] */
    const int32_t *table, *idxnum, *lflag, *rflag, *islocked, *lkeylen, *rkeylen;
    const uint64_t *lkey_off, *rkey_off;
} hsc_coalesced;
int hsc_coalesce_readsets(hsc_ctx *ctx, const hsc_readsets *rs, hsc_coalesced *out);

/* Host threads that marshal a batch (0 = the box's CPUs: the affinity mask
 * capped by the cgroup CPU quota; HSC_THREADS overrides that default).  A
 * batch of >= 65536 read sets runs as a pipeline of 32768-set chunks over two
 * pinned staging sets: one chunk is marshalled while the previous one is
 * uploaded, joined and read back. */
int hsc_set_threads(hsc_ctx *ctx, int n);

/* Flat read sets (snapshots in rs->snap); rc_out[ntxn]; full checks only. */
int hsc_check_readsets(hsc_ctx *ctx, const hsc_readsets *rs, int *rc_out);

/* ---- marshalling + device probe (what the checks lower to) -------------- */
typedef struct hsc_marshalled {
    size_t n, n_lock, n_txn;
    int words;
    uint64_t *lo, *hi;        /* host [words][n] */
    uint32_t *gid;
    uint64_t *snap;
    uint32_t *txn;
    uint32_t *lock_table;
    uint64_t *lock_snap;
    uint32_t *lock_txn;
    uint8_t *forced;          /* [n_txn] verdicts decided on the host (1/0)   */
} hsc_marshalled;
/* Marshal flat read sets against the current window into probe SoA (host
 * memory owned by the library; valid until the next marshal / ctx destroy). */
int hsc_marshal_readsets(hsc_ctx *ctx, const hsc_readsets *rs,
                         const hsc_marshalled **out);
/* The host half of hip_serial_check_batch: CurRangeArr* ranges[n] (none
 * NULL) with snapshot LSNs snaps[n], marshalled as hsc_marshal_readsets does
 * (works on host-only contexts; the timing harness of the batch entry). */
int hsc_marshal_arrs(hsc_ctx *ctx, void *const *ranges, const uint64_t *snaps, int n,
                     const hsc_marshalled **out);
/* Run the join for a device-resident batch, asynchronously on the stream. */
int hsc_probe_device(hsc_ctx *ctx, const hsc_probe_batch *b);
/* verdict bytes -> bitmap (e.g. after a cross-GPU max all-reduce). */
int hsc_pack_verdicts(hsc_ctx *ctx, const uint8_t *verdict, size_t n_txn,
                      uint64_t *bitmap);
/* Multi-GPU verdict merge: out_dev[w] = OR over k < nparts of
 * parts_dev[k * words + w] -- the per-shard verdict bitmaps after an
 * all-gather (N x n_txn / 8 bytes per rank instead of a byte-wise max
 * all-reduce of N x n_txn).  Asynchronous on the context's stream. */
int hsc_or_bitmaps(hsc_ctx *ctx, const uint64_t *parts_dev, int nparts, size_t words,
                   uint64_t *out_dev);
int hsc_synchronize(hsc_ctx *ctx);
int hsc_get_timing(hsc_ctx *ctx, hsc_timing *t);
/* Enable per-kernel HIP event timing of probes (adds event records). */
int hsc_enable_timing(hsc_ctx *ctx, int on);

/* ---- multi-GPU context ---------------------------------
 * A multi context is an hsc_ctx: hip_serial_check_batch,
 * hip_bdb_osql_serial_check, hsc_collector_*, hsc_check_readsets /
 * _serial, hsc_window_ingest_log / _raw, hsc_window_append[_log|_raw],
 * hsc_register_group and the window accessors take it unchanged.  Its window
 * is cut into `world` contiguous pieces of the composite key space (gid, key
 * words) -- member d holds the keys K with sp[d-1] <= K < sp[d] -- one per
 * member context.  The context itself keeps the log decode, dictionaries and
 * window rules and marshals every batch on the host.  A range [g||lo, g||hi]
 * goes to the members whose pieces it overlaps (owner(g||lo) ..
 * owner(g||hi)), table locks to member 0 (it holds the global table maxima).
 * In one process the drop-in entries route while marshalling: each member
 * that holds any probe of the batch checks its share through its own one-GPU
 * path (the small-batch kernel for a lone call), and the verdicts are OR-ed.
 * Batches already resident on the GPUs are either routed there
 * (hsc_multi_probe_device: route kernels, then an exchange -- direct stores
 * between members of one process over xGMI peer access, RCCL grouped
 * ncclSend / ncclRecv between processes) or arrive routed
 * (hsc_multi_probe_routed); every member joins its probes against its piece
 * and the members' verdict bitmaps are OR-ed per read-set owner.  A per-rank
 * context (one process per GPU, hsc_multi_create_rank; librccl loaded at run
 * time) routes its drop-in batches on the devices.  Verdicts equal those of
 * one context holding the whole window.  Not on a multi
 * context: hsc_set_stream, hsc_probe_device, hsc_window_ingest_device (ingest
 * the members directly, then hsc_multi_adopt), hsc_rw_edges, the graph and
 * coalesce calls (use a member). */
/* n members on devices[0..n-1] (n <= 16; a device may repeat) in this
 * process.  Returns the context in *out (destroy with hsc_ctx_destroy). */
int hsc_multi_create(const int *devices, int n, hsc_ctx **out);
/* One member per process: this process is member `rank` of `world` on
 * `device`.  ids: the bytes hsc_multi_unique_ids wrote on one rank (every
 * rank passes the same ones; 2 x 128 bytes: one RCCL communicator per lane). */
int hsc_multi_unique_ids(void *out, size_t bytes);
int hsc_multi_create_rank(int device, int rank, int world, const void *ids, size_t bytes,
                          hsc_ctx **out);
int hsc_multi_world(hsc_ctx *ctx);   /* members of the partition */
int hsc_multi_rank(hsc_ctx *ctx);    /* global index of this process's first member */
int hsc_multi_local(hsc_ctx *ctx);   /* members in this process */
hsc_ctx *hsc_multi_member(hsc_ctx *ctx, int i);  /* i < hsc_multi_local */
/* The world - 1 ascending splitters (gid[S], words[W][S] big-endian key
 * words); default: equal-row quantiles of the ingested log's rows.  A
 * host-staged window is re-partitioned at the next check. */
int hsc_multi_set_splitters(hsc_ctx *ctx, size_t S, const uint32_t *gid, const uint64_t *words,
                            int W);
/* The members' windows, ingested directly (hsc_window_ingest_device on
 * hsc_multi_member, each holding exactly its piece's rows), become the
 * context's window; table maxima are max-merged over all members (an RCCL
 * all-reduce across ranks).  Collective on a per-rank context.  HSC_ESTATE
 * without splitters (world > 1); HSC_EINVAL when the members' key widths
 * differ or a member's first or last key lies outside its piece.  Appends
 * then go to the members (the context's append entries return HSC_ESTATE). */
int hsc_multi_adopt(hsc_ctx *ctx);
/* In-process contexts: HSC_MULTI_DIRECT (default: the device routing stores
 * into the other members' probe columns, the merge reads their bitmaps) or
 * HSC_MULTI_LOOPBACK (the per-rank form with peer copies in place of RCCL:
 * send blocks, k_route_unpack, owner slices gathered and OR-ed -- what a
 * per-rank context runs, on one process). */
#define HSC_MULTI_DIRECT 0
#define HSC_MULTI_LOOPBACK 1
int hsc_multi_set_transport(hsc_ctx *ctx, int transport);
/* Window placement.  HSC_MULTI_PIECES: each member holds its key-range piece
 * (the splitters); a batch's probes go to the pieces they overlap and the
 * verdicts are OR-ed.  HSC_MULTI_REPLICAS: every member holds the whole
 * window (builds and appends go to every member); a drop-in batch that fits
 * the small path goes whole to ONE member (the one with the fewest batches in
 * flight, round robin among equals: one member kernel per call), a larger
 * one is cut into per-member slices of its read sets, each checked by one
 * member against its replica -- no routing, no exchange, no OR across
 * members.  HSC_MULTI_AUTO (default): replicas when a host-staged window's
 * rows x (8 W + 16) bytes fit an eighth of the smallest member's device
 * memory, else pieces; an adopted window is pieces unless REPLICAS was set
 * (hsc_multi_adopt then needs every member to hold the same rows, no
 * splitters).  A host-staged window is re-placed at the next check.
 * hsc_multi_mode returns the placement in force (PIECES or REPLICAS). */
#define HSC_MULTI_AUTO 0
#define HSC_MULTI_PIECES 1
#define HSC_MULTI_REPLICAS 2
int hsc_multi_set_mode(hsc_ctx *ctx, int mode);
int hsc_multi_mode(hsc_ctx *ctx);
/* Device-resident batches, one per local member (pointers on its GPU), each
 * numbering its own read sets 0..b[i].n_txn-1: routed, probed and merged;
 * b[i].bitmap (ceil(n_txn / 64) words) receives the merged verdict bits of
 * member i's read sets.  lane (0 or 1): scratch set, so two batches can be in
 * flight; a lane is reused after its previous batch finished.  Returns once
 * the work is enqueued (the host waits for the routing counts only).
 * Collective on a per-rank context. */
int hsc_multi_probe_device(hsc_ctx *ctx, const hsc_probe_batch *b, int lane);
/* Device-resident batches routed when they were marshalled, one per local
 * member: b[i] holds exactly the probes whose [lo, hi] overlaps member i's
 * piece (hsc_multi_marshal_routed; table locks on member 0 only), read sets
 * numbered batch-wide: owner o owns [owner_base[o], owner_base[o + 1])
 * (world + 1 ascending multiples of 64 from 0), b[i].bitmap receives the
 * merged bits of member i's own read sets.  Every member probes its batch in
 * place; the bitmaps are OR-ed per owner (RCCL send / receive of the owners'
 * slices across ranks).  No routing and no probe exchange on the devices.
 * lane as for hsc_multi_probe_device; collective on a per-rank context. */
int hsc_multi_probe_routed(hsc_ctx *ctx, const hsc_probe_batch *b, const uint64_t *owner_base, int lane);
/* Marshal rs (hsc_marshal_readsets) and route it on the host: *out = the
 * columns of member `member` (read-set numbers + txn_base; table locks when
 * member == 0), host memory valid until the next marshal on ctx.  forced =
 * the whole batch's host-decided verdicts. */
int hsc_multi_marshal_routed(hsc_ctx *ctx, const hsc_readsets *rs, int member, uint32_t txn_base,
                             const hsc_marshalled **out);
/* member >= 0 above; member = -1 routes the batch to every member, *out =
 * member 0's columns and hsc_multi_routed_member the others' (same life). */
int hsc_multi_routed_member(hsc_ctx *ctx, int member, const hsc_marshalled **out);
/* Events around every member's probe of the routed pipelines (diagnostics,
 * per-member imbalance); out[i] = local member i's probe ms of the last batch
 * (waits for it). */
int hsc_multi_enable_timing(hsc_ctx *ctx, int on);
int hsc_multi_member_probe_ms(hsc_ctx *ctx, float *out, int n);
/* Host routing of the drop-in entries: out[8] = calls, member checks run,
 * probes routed, probe rows placed (> probes when ranges straddle pieces),
 * mean us routing per call, world, mean us launching the members, mean us
 * waiting for their verdicts. */
int hsc_multi_route_stats(hsc_ctx *ctx, double out[8]);
/* out[4]: routed batches, probes routed (sources), probe rows received
 * (destinations; > probes when ranges straddle pieces), local members. */
int hsc_multi_stats(hsc_ctx *ctx, uint64_t out[4]);
/* counts[s * world + d]: probes member s sent member d in the last batch. */
int hsc_multi_last_counts(hsc_ctx *ctx, uint32_t *counts, int n);
/* Host time per routed batch (diagnostics): out[0] device-routed batches,
 * then mean us enqueueing the lane waits, launching the route counts,
 * waiting for the counts the device publishes, enqueueing the rest of the
 * batch; out[5] hsc_multi_probe_routed batches, out[6] mean us enqueueing
 * one. */
int hsc_multi_phase_stats(hsc_ctx *ctx, double out[7]);
/* hsc_multi_probe_routed's host time per batch, split (us): out[0] batches,
 * out[1] lane_acquire (the members' cross-lane event waits), out[2] the
 * members' probe launches, out[3] the owners' merges and done events.  An
 * enqueue blocks when a hardware queue is full, so each phase holds that
 * wait too; bench.py times calls that start on an idle GPU for the pure
 * enqueue cost. */
int hsc_multi_routed_phase_stats(hsc_ctx *ctx, double out[4]);

/* ---- OSQL_SERIAL wire path --------------------------------------------
 * Decode only: *out points at context-owned read sets, valid until the next
 * decode on this context (HSC_EINVAL names the malformed message). */
int hsc_decode_serial(hsc_ctx *ctx, const hsc_serial_msgs *msgs, const hsc_readsets **out);
/* Decode + full check (regop_only = 0) of every message: rc_out[nmsg]. */
int hsc_check_serial(hsc_ctx *ctx, const hsc_serial_msgs *msgs, int *rc_out);

/* ---- dependency graph + SCC ------------------------
 * History of committed transactions as micro-ops (host pointers): txn ids
 * are commit order (a key's version order = its writers' commit order); a
 * read records the writer txn of the version it observed (-1 = initial), as
 * a Jepsen rw-register history with unique write values does.  Edges (Adya):
 * ww consecutive writers of a key, wr writer -> reader, rw reader -> next
 * writer after the observed version; self edges dropped, parallel edges
 * merged (type bits: 1 ww, 2 wr, 4 rw; 8 rt, the real-time order, only when
 * hsc_dep_graph_stage_realtime staged it).  scc_out[v] = the largest txn id of
 * v's strongly connected component; a component with more than one txn is a
 * dependency cycle -- hsc_dep_graph_anomalies (below) tells which anomaly
 * (G1c / G-single / G2) it is and returns one cycle of it. */
typedef struct hsc_history {
    size_t nops;
    uint32_t ntxn;
    const uint32_t *txn;
    const uint64_t *key;
    const uint8_t *is_write;
    const int64_t *observed;
} hsc_history;

typedef struct hsc_graph_stats {
    uint64_t edges;
    uint64_t ww, wr, rw;          /* edges carrying each type bit              */
    uint32_t nontrivial_sccs;     /* components with >= 2 txns                 */
    uint32_t txns_in_cycles;
    uint32_t rounds, iterations;  /* colouring rounds / frontier steps         */
    float build_ms, scc_ms;       /* device time                               */
    uint32_t cut_nodes;           /* hsc_dep_graph_scc_cut: nodes of the cover */
} hsc_graph_stats;

int hsc_dep_graph_scc(hsc_ctx *ctx, const hsc_history *h, uint32_t *scc_out,
                      hsc_graph_stats *stats);
/* Edges of the last full build, sorted by (src, dst): copies min(cap, n)
 * (n = 0 after a raw build). */
int hsc_dep_graph_edges(hsc_ctx *ctx, uint32_t *src, uint32_t *dst, uint32_t *type,
                        size_t cap, size_t *n);

/* Sharded SCC (config 4 over N GPUs).  Every WW/WR/RW edge belongs to one
 * key, so a history split by key gives each shard an exact part of the edge
 * set.  Txn ids are commit order; a cycle always contains a backward edge
 * (src > dst) and all its nodes lie inside [dst, src] of its backward edges,
 * so components of >= 2 txns live in the graph induced on the "cover" (the
 * nodes inside some backward edge's interval).  Per shard: build, cover
 * (u8 per txn, merged over shards with a MAX all-reduce), cut (the shard's
 * edges between covered nodes, exchanged with an all-gather), then the SCC of
 * the union of the cuts -- the same scc[] as hsc_dep_graph_scc of the whole
 * history.  Pointers named *_dev are device memory of the context's GPU. */
/* flags: HSC_GRAPH_FULL = sorted unique edges with types and CSR / CSC (what
 * hsc_dep_graph_edges returns, stats.edges/ww/wr/rw filled); 0 = the raw edge
 * rows only (duplicates, no sort: all cover / cut need; stats.build_ms only). */
#define HSC_GRAPH_FULL 1
/* HSC_GRAPH_NO_RW: reads give their wr edge only; the rw edges come from
 * staged pairs (hsc_dep_graph_stage_rw_pairs). */
#define HSC_GRAPH_NO_RW 2
int hsc_dep_graph_build(hsc_ctx *ctx, const hsc_history *h, int flags, hsc_graph_stats *stats);
/* The same from device-resident ops (observed: writer txn, 0xFFFFFFFF =
 * initial version); ops naming a txn >= ntxn -> HSC_EINVAL. */
int hsc_dep_graph_build_device(hsc_ctx *ctx, size_t nops, uint32_t ntxn, const uint32_t *txn_dev,
                               const uint64_t *key_dev, const uint8_t *is_write_dev,
                               const uint32_t *observed_dev, int flags, hsc_graph_stats *stats);
/* The validator's rw pairs as graph edges: the pairs of
 * the last hsc_rw_edges call -- still on the device -- become rw edges
 * readset_txn[t] -> commit_txn[i] (commit_lsn[i] == the writer's commit LSN;
 * commit_lsn sorted ascending; host arrays) and join the next
 * hsc_dep_graph_build / _build_device (merged with its own edges, type bits
 * OR-ed; self edges dropped).  A pair whose read set or LSN is not mapped ->
 * HSC_EINVAL.  Pairs name every writer after the snapshot, not only the next
 * version: the extra edges t -> later writers follow the ww chain and leave
 * the components unchanged. */
int hsc_dep_graph_stage_rw_pairs(hsc_ctx *ctx, uint32_t nrs, const uint32_t *readset_txn,
                                 size_t ncommit, const uint64_t *commit_lsn,
                                 const uint32_t *commit_txn);
/* Strict serializability: the real-time order as a fourth edge type.  Txn a
 * precedes txn b when a completed before b was invoked, complete[a] <
 * invoke[b] (host arrays of ntxn u64 in the history's txn ids, any monotonic
 * clock; complete[v] == HSC_RT_OPEN: v never completed -- a recovered :info
 * op -- and precedes nothing).  The relation is quadratic; what is staged is
 * its transitive reduction (the pairs not implied by two others: same closure,
 * so the same components and cycles), at most ntxn x the history's concurrency
 * edges, as edges of type bit 8 for the next hsc_dep_graph_build /
 * _build_device of exactly ntxn txns.  They join that build once, merged with
 * its own edges and any staged rw pairs (type bits OR-ed: wr | rt is a legal
 * type); a build of another ntxn fails with HSC_EINVAL and drops every staged
 * edge.  rw pairs and the order may both be staged before one build, in
 * either order; staging one kind again replaces that kind only.
 * invoke[v] > complete[v] -> HSC_EINVAL; a host-only context -> HSC_EDEVICE;
 * ntxn == 0 stages nothing for a build of no txns.  n_edges (may be NULL):
 * the edges staged; ms (may be NULL): device time of the sort, scan, count
 * and emit.  hsc_graph_stats counts ww / wr / rw as before (edges includes
 * every merged edge); hsc_dep_graph_edges returns bit 8 in type like any
 * other bit.  The sharded path (hsc_multi_graph_scc) takes no real-time
 * edges. */
#define HSC_RT_OPEN UINT64_MAX
int hsc_dep_graph_stage_realtime(hsc_ctx *ctx, uint32_t ntxn, const uint64_t *invoke,
                                 const uint64_t *complete, uint64_t *n_edges, float *ms);
/* scc_out[ntxn] of the last HSC_GRAPH_FULL build (stats as hsc_dep_graph_scc,
 * build_ms 0). */
int hsc_dep_graph_scc_built(hsc_ctx *ctx, uint32_t *scc_out, hsc_graph_stats *stats);
/* Which anomaly each dependency cycle of the last HSC_GRAPH_FULL build is
 * (its edges plus any staged rw pairs and real-time order, parallel edges
 * merged), and one witness cycle per component.  E1 = the edges carrying a
 * ww, wr or rt bit (type & 11); an anti edge has type == 4 exactly, so an rw
 * edge that the real-time order also forces (rw | rt) is E1.  Without staged
 * real-time edges E1 is the ww / wr edges; with them the bits below keep their
 * definitions over the widened E1 (a read that returns a version overwritten
 * before the read was invoked is the cycle r -rw-> w -rt-> r: G-single).
 * cls[v] is a mask:
 *   HSC_ANOM_G1C      v's component of (V, E1) has >= 2 txns (circular
 *                     information flow);
 *   HSC_ANOM_GSINGLE  an anti edge a -> b with scc[a] == scc[b] exists such
 *                     that b reaches v and v reaches a over E1 edges whose ends
 *                     lie in that component (a cycle with one anti-dependency:
 *                     read skew);
 *   HSC_ANOM_G2       v's component has >= 2 txns and holds an anti edge with
 *                     both ends inside it (write skew at the least).
 * A txn outside every component of >= 2 txns has cls 0; a component of >= 2
 * always has a bit (a cycle without an anti edge is an E1 cycle), and its
 * class comp_class[i] is the lowest bit of the OR of its members' cls.
 * There is no G0 bit: txn ids are commit order and a key's version order is
 * its writers' commit order, so every ww edge goes up in txn id and no cycle
 * is made of ww edges alone; an rt edge between completed txns goes up in
 * commit order as well (a completed before b was invoked, so before b
 * completed), so ww and rt edges together make no cycle either.
 * A build from a list-append history (hsc_dep_graph_build_lists) is the one
 * exception: its version orders come from the reads, not from txn ids, so its
 * ww edges may go down in id and a cycle of ww edges alone (G0) can exist.
 * Such a cycle is an E1 cycle and is classed HSC_ANOM_G1C here; telling G0
 * apart is left to the caller (jepsen.check_append_edn names it when the
 * witness cycle is ww only).
 * HSC_ANOM_WITNESS: per component one simple cycle of its class, wit_txn
 * [wit_off[i], wit_off[i + 1]).  Its closing edge last -> first is the lowest
 * edge, in the build's (src, dst) order, that is -- class G1c: an E1 edge
 * whose ends share a component of (V, E1); G-single: an anti edge a -> b with b
 * reaching a over E1 inside the component; G2: an anti edge inside the
 * component.  The rest is a shortest path first ~> last, over E1 edges of the
 * component (G1c, G-single) or all of its edges (G2); which of several
 * shortest paths is unspecified.
 * max_anti_batches: the G-single test takes the components' anti edges 64 to
 * a batch; > 0 stops after that many batches (anti_tested < anti_edges), and
 * the G-single bit and a component's class are then lower bounds.  0 = all.
 * The arrays are host memory owned by the context, valid until its next graph
 * call.  HSC_ESTATE after a raw build, HSC_EDEVICE on a host-only context.
 * The sharded path (hsc_multi_graph_scc) has no such call: it keeps no typed
 * edges. */
#define HSC_ANOM_G1C 1
#define HSC_ANOM_GSINGLE 2
#define HSC_ANOM_G2 4
#define HSC_ANOM_WITNESS 1            /* flags */
typedef struct hsc_anomalies {
    uint32_t ntxn;   const uint8_t *cls;          /* [ntxn] */
    uint32_t ncomp;  const uint32_t *comp_label;  /* [ncomp] ascending; = scc[] label (largest txn) */
    const uint8_t *comp_class;                    /* [ncomp] lowest bit of the members' OR */
    const uint32_t *wit_off;                      /* [ncomp+1]; all 0 without HSC_ANOM_WITNESS */
    const uint32_t *wit_txn;                      /* cycle nodes, starting at the closing edge's dst */
    const uint8_t  *wit_type;                     /* type bits of edge wit_txn[i] -> next (cyclically) */
    uint32_t comps[3], txns[3];                   /* components by class / txns carrying each bit */
    uint64_t anti_edges, anti_tested;             /* anti edges inside components / those tested */
    uint32_t core_nodes, reach_batches, sweeps, bfs_levels;
    float ms;                                     /* device time of the analysis, SCC included */
} hsc_anomalies;
int hsc_dep_graph_anomalies(hsc_ctx *ctx, unsigned flags, unsigned max_anti_batches, hsc_anomalies *out);
/* Snapshot isolation from the same typed edges (the last HSC_GRAPH_FULL build,
 * E1 = type & 11, an anti edge has type == 4 exactly, only edges whose ends
 * share a component of scc[] matter).  A dependency graph is allowed under
 * snapshot isolation iff every cycle has two adjacent anti-dependency edges
 * (Cerone and Gotsman; Elle's G-nonadjacent), so the level is violated iff
 * some cycle has no two cyclically consecutive anti edges: a cycle without an
 * anti edge (G1c), with one (G-single), or with several, none adjacent
 * (G-nonadjacent -- hsc_dep_graph_anomalies calls these G2 like plain write
 * skew).
 * Product graph P: txn v becomes (v,0) "reached by an E1 edge" and (v,1)
 * "reached by an anti edge"; an E1 edge u -> v gives (u,0) -> (v,0) and
 * (u,1) -> (v,0), an anti edge gives (u,0) -> (v,1) only.
 *   nonadj[v] = 1 iff (v,0) or (v,1) lies in a strongly connected component
 *               of P with >= 2 nodes -- iff v lies on a closed walk of the
 *               build's edges in which no two cyclically consecutive edges
 *               are anti edges (lift the walk by the type of each arriving
 *               edge; self edges are dropped, so it has >= 2 txns).
 *   comp_nonadj[i] = 1 iff a member of component i has the bit.  The
 *               component then holds a simple cycle without two adjacent anti
 *               edges (split a closed walk at a repeated txn: if one half has
 *               two anti edges at the split, both edges of the other half
 *               there are not anti edges; recurse on a good half).
 * Every txn with the G1c or G-single bit of hsc_dep_graph_anomalies has the
 * bit; a component of class G2 with the flag is G-nonadjacent; a component
 * without the flag has class G2 and is legal under snapshot isolation (write
 * skew only).  The answer is exact whatever max_anti_batches was given to
 * hsc_dep_graph_anomalies: no reach budget enters here.
 * Scope: this is the dependency-graph condition only.  The graph is built
 * from committed txns: aborted and intermediate reads (G1a, G1b) are reported
 * by hsc_dep_graph_resolve (below) for a history given with its values, not by
 * this call; internal consistency by hsc_dep_graph_internal / _internal_lists
 * (below).  With a staged real-time order the definitions hold unchanged
 * over the widened E1, and the verdict is strong snapshot isolation.
 * HSC_SI_WITNESS: per flagged component one simple cycle of >= 2 of its txns,
 * wit_txn[wit_off[i], wit_off[i + 1]), every step an edge of the build with
 * its type bits in wit_type, no two cyclically consecutive steps anti edges.
 * Which edge closes it and its length are unspecified.  An unflagged
 * component has an empty run.
 * comp_label equals hsc_anomalies.comp_label of the same build.  The arrays
 * are host memory owned by the context, never NULL, valid until its next
 * graph call; the results of hsc_dep_graph_anomalies stay valid across this
 * call.  HSC_ESTATE after a raw build, HSC_EDEVICE on a host-only context,
 * HSC_EINVAL for a NULL argument or a product graph (twice the txns in
 * cycles; their edges plus their E1 edges) past 32-bit ids.  The sharded path
 * (hsc_multi_graph_scc) has no such call: it keeps no typed edges. */
#define HSC_SI_WITNESS 1              /* flags */
typedef struct hsc_si_report {
    uint32_t ntxn;   const uint8_t *nonadj;       /* [ntxn] the bit defined above */
    uint32_t ncomp;  const uint32_t *comp_label;  /* [ncomp] ascending, = hsc_anomalies.comp_label */
    const uint8_t *comp_nonadj;                   /* [ncomp] some member has the bit */
    const uint32_t *wit_off;                      /* [ncomp+1]; empty run for an unflagged component; all 0 without the flag */
    const uint32_t *wit_txn;                      /* cycle txns */
    const uint8_t  *wit_type;                     /* type bits of edge wit_txn[i] -> next (cyclically) */
    uint32_t comps, txns;                         /* flagged components / txns carrying the bit */
    uint32_t core_nodes, product_nodes;           /* txns in cycles / nodes of P (twice as many) */
    uint64_t product_edges;                       /* core edges + core E1 edges */
    uint32_t scc_rounds, scc_iterations, bfs_levels;
    float ms;                                     /* device time, both SCC runs included */
} hsc_si_report;
int hsc_dep_graph_si(hsc_ctx *ctx, unsigned flags, hsc_si_report *out);
/* ---- version resolution: aborted and intermediate reads (G1a, G1b) ---------
 * The graph entries above take committed txns whose reads already name the
 * writer they observed.  This entry takes the history of every attempted txn
 * with the values it read and wrote, finds on the GPU the write each read
 * observed, flags aborted (G1a) and intermediate (G1b) reads, decides which
 * indeterminate txns committed, and lowers the committed part to the
 * device-resident ops hsc_dep_graph_build_device takes, so that every analysis
 * above runs unchanged on a history that came from values.
 * Premises:
 *   - the ops of one txn stand in program order in the arrays (they need not
 *     be contiguous);
 *   - the txns that count as committed (the set C below), taken in ascending
 *     id, are in commit order -- the rule of hsc_history;
 *   - written (key, value) pairs are unique over the whole history, aborted and
 *     unknown txns included (Elle's rw-register premise); the same value on
 *     two keys is fine.
 * Resolution.  Read op i of txn r has key k and value v.  v == HSC_VAL_INIT:
 * it observed the initial version, no flags.  Otherwise it observed the write
 * op j with key[j] == k && value[j] == v; no such j: HSC_RD_DANGLING.  With
 * w = txn[j]: w == r gives HSC_RD_INTERNAL and no other flag; otherwise
 * status[w] == HSC_TXN_ABORTED gives HSC_RD_ABORTED, and j not being the last
 * write of k by w in program order gives HSC_RD_INTERMEDIATE (both may be
 * set).  Flags are computed for every read, whatever the reader's status.
 * Committed set C: the least set that holds every OK txn and every UNKNOWN txn
 * one of whose writes is observed (w != r) by a read of a txn in C.  An UNKNOWN
 * txn in C is recovered, one outside C dropped; an ABORTED txn is never in C.
 * Anomalies: only reads of txns in C count.  G1a: a read with HSC_RD_ABORTED;
 * G1b: a read with HSC_RD_INTERMEDIATE; txn_g1[r] bit 1 / bit 2: r is in C and
 * has such a read.
 * Internal consistency (a txn that reads k after writing k must see its own
 * last write) is not checked by this entry, which only counts an internal
 * read: hsc_dep_graph_internal (below) checks it on the history this entry
 * uploaded.
 * Lowering: cid[t] = the dense rank of t among C in ascending id, 0xFFFFFFFF
 * outside C; txn_of_cid its inverse.  The kept ops, in array order, are all
 * ops of txns in C except reads flagged DANGLING or ABORTED; a kept op has
 * txn := cid[txn], a kept read observed := cid[w] (0xFFFFFFFF: the initial
 * version).  Intermediate and internal reads are kept (their wr edge is real;
 * the build drops self edges).  Several writes of one key by one txn are one
 * version (the build dedupes (key, txn)).
 * writes / reads count every op of the history; the g1a / g1b / dangling /
 * internal counts the reads of txns in C.
 * HSC_EINVAL: a NULL argument, txn[i] >= ntxn, a status above 2, a write of
 * HSC_VAL_INIT, a duplicated written (key, value), more than 2^31 - 1 ops or
 * txns.  HSC_EDEVICE: a host-only context.  nops == 0 and ntxn == 0 succeed.
 * The arrays are host memory owned by the context, never NULL except the three
 * per-op ones without HSC_RESOLVE_ARRAYS, valid until the next graph call.
 * The lowered ops stay on the device in buffers of their own: a plain
 * hsc_dep_graph_build does not disturb them, nor they it.  The sharded path
 * (hsc_multi_graph_scc) has no such entry. */
#define HSC_VAL_INIT     UINT64_MAX   /* a read that saw the initial state; not a legal written value */
#define HSC_TXN_OK       0
#define HSC_TXN_ABORTED  1
#define HSC_TXN_UNKNOWN  2            /* :info / crashed: may have committed */
#define HSC_RD_ABORTED      1
#define HSC_RD_INTERMEDIATE 2
#define HSC_RD_DANGLING     4
#define HSC_RD_INTERNAL     8
typedef struct hsc_vhistory {         /* every attempted txn, host pointers */
    size_t nops; uint32_t ntxn;
    const uint32_t *txn;              /* [nops] < ntxn */
    const uint64_t *key;              /* [nops] */
    const uint8_t  *is_write;         /* [nops] */
    const uint64_t *value;            /* [nops] write: the value written; read: the value returned */
    const uint8_t  *status;           /* [ntxn] HSC_TXN_* */
} hsc_vhistory;
#define HSC_RESOLVE_ARRAYS 1   /* flags: also copy the per-op arrays back */
#define HSC_RESOLVE_LIST_CAP 4096
typedef struct hsc_resolved {
    size_t nops, kept_ops;  uint32_t ntxn, ncommitted, recovered, aborted, dropped;
    uint64_t writes, reads;
    uint64_t g1a_reads, g1b_reads, dangling_reads, internal_reads;  /* reads of txns in C */
    uint32_t g1a_txns, g1b_txns;
    const uint8_t *fate;         /* [ntxn] 0 committed, 1 aborted, 2 dropped, 3 recovered */
    const uint32_t *cid;         /* [ntxn] */
    const uint32_t *txn_of_cid;  /* [ncommitted] */
    const uint8_t *txn_g1;       /* [ntxn] */
    uint32_t n_listed;           /* min(cap, reads of C flagged ABORTED | INTERMEDIATE | DANGLING) */
    const uint64_t *listed_op, *listed_wop;  /* ascending read op index; its write op (UINT64_MAX: none) */
    const uint32_t *obs_txn;     /* [nops] input ids; 0xFFFFFFFF initial or a write op; 0xFFFFFFFE none.  NULL without ARRAYS */
    const uint64_t *obs_op;      /* [nops] the write op observed, UINT64_MAX none */
    const uint8_t  *rflag;       /* [nops] HSC_RD_* */
    uint32_t sweeps;  float ms;  /* recovery sweeps run; device time of the whole call */
} hsc_resolved;
int hsc_dep_graph_resolve(hsc_ctx *ctx, const hsc_vhistory *h, unsigned flags, hsc_resolved *out);
/* hsc_dep_graph_build_device over the lowered ops of the last resolve (ncommitted txns); joins staged
 * rw pairs / real-time edges like any build.  HSC_ESTATE without a resolve. */
int hsc_dep_graph_build_resolved(hsc_ctx *ctx, int flags, hsc_graph_stats *stats);
/* How the last resolve sorted its writers: bit 0 the (key, value) lookup table,
 * bit 1 the (key, txn) finality rows -- set: as packed single words, clear: by
 * whole rows (or nothing to sort). */
int hsc_dep_graph_resolve_sort_path(hsc_ctx *ctx);
/* ---- list-append histories: the version order from the reads --------------
 * Every graph entry above rests on one premise: txn ids are commit order and a
 * key's version order is its writers' commit order.  A list-append history
 * (Elle's main workload) needs no such premise: every write appends a unique
 * element to its key's list, every read returns the whole list, and the
 * longest read of a key is that key's version order.  This entry recovers the
 * version orders on the GPU, flags the reads against them, decides which
 * indeterminate txns committed and emits the ww / wr / rw edges, which
 * hsc_dep_graph_build_lists turns into a build every analysis above runs on.
 * Premises:
 *   - the ops of one txn stand in program order in the arrays (they need not
 *     be contiguous);
 *   - appended (key, element) pairs are unique over the whole history, aborted
 *     and unknown txns included; the same element on two keys is fine;
 *   - nothing about txn ids: they may be in any order.
 * Spine.  S_k, the spine of key k, is the longest list among the reads of k by
 * HSC_TXN_OK txns; a tie goes to the lowest op index.  Reads by txns of any
 * other status are ignored throughout (no flags, no edges, not counted in the
 * flag counters).  A key no OK txn read has an empty spine and no rank; the
 * keys that have one are ranked in ascending key (keys, spine_op[rank]).
 * Read flags (reads of OK txns only).  HSC_LRD_INCOMPATIBLE: the list is not a
 * prefix of S_k (Elle's incompatible-order); such a read gets no other flag
 * and no edges.  A compatible read of length n takes its other flags from the
 * first n spine positions:
 *   HSC_RD_DANGLING      one of them holds an element nobody appended;
 *   HSC_LRD_DUPLICATE    one of them repeats an earlier position's element;
 *   HSC_RD_ABORTED       (G1a) one of them was appended by an ABORTED txn;
 *   HSC_RD_INTERMEDIATE  (G1b) position n - 1 was appended by w != the reader,
 *                        and that append is not w's last append to k in
 *                        program order;
 *   HSC_RD_INTERNAL      counted only (see the wr edge below).
 * Committed set C: the OK txns plus every UNKNOWN txn that has an append whose
 * element stands in its key's spine (recovered).  One pass, no sweeps: only OK
 * txns read.  fate, cid and txn_of_cid are as in hsc_resolved (cid: the dense
 * rank among C in ascending id); txn_g1[r] bit 1 / bit 2: r has a read flagged
 * ABORTED / INTERMEDIATE.
 * Chain of k: the spine positions, in spine order, whose element resolves to
 * an append, is that element's first occurrence in the spine, and was appended
 * by a txn in C.  ww edge: the writer of chain[c] -> the writer of
 * chain[c + 1] where the two differ.
 * wr / rw edges.  A compatible read by r with c chain entries among its first
 * n positions gives wr: writer(chain[c - 1]) -> r if c > 0, and rw: r ->
 * writer(chain[c]) if the chain has such an entry.  An empty read has n = 0
 * and c = 0: it anti-depends on the first writer.  Self edges are dropped;
 * internal_reads counts the reads whose chain[c - 1] was written by r itself
 * (they carry HSC_RD_INTERNAL).  Edges are in cid space.  ww / wr / rw count
 * the rows emitted, before the build merges parallel edges.
 * An append by a txn of C whose element stands in no spine has no known
 * position: it yields no edge and is counted in unobserved_appends.
 * appends / reads count every op of the history; elements = list_off[nops].
 * listed_op: up to HSC_RESOLVE_LIST_CAP read ops with a flag other than
 * INTERNAL, in ascending op index, their flags in listed_flag.
 * HSC_EINVAL: a NULL argument, txn[i] >= ntxn, a status above 2, a list_off
 * that is not ascending, a duplicated append, more than 2^31 - 1 ops, txns or
 * elements.  HSC_EDEVICE: a host-only context.  Empty histories succeed.  The
 * arrays are host memory owned by the context, never NULL (rflag and spine_op
 * hold nothing without HSC_RESOLVE_ARRAYS), valid until the next graph call.
 * The edge rows stay on the device in buffers of their own: a plain
 * hsc_dep_graph_build does not disturb them, nor they it.  The sharded path
 * (hsc_multi_graph_scc) has no such entry. */
#define HSC_LRD_INCOMPATIBLE 16
#define HSC_LRD_DUPLICATE    32
typedef struct hsc_lhistory {          /* every attempted txn, host pointers */
    size_t nops; uint32_t ntxn;
    const uint32_t *txn;               /* [nops] < ntxn; ids in ANY order */
    const uint64_t *key;               /* [nops] */
    const uint8_t  *is_write;          /* [nops] 1 = append */
    const uint64_t *value;             /* [nops] append: the element; read: ignored */
    const uint64_t *list_off;          /* [nops+1] ascending; read op i returned
                                          elems[list_off[i] .. list_off[i+1]); an append's run is empty */
    const uint64_t *elems;             /* [list_off[nops]] */
    const uint8_t  *status;            /* [ntxn] HSC_TXN_* */
} hsc_lhistory;
typedef struct hsc_lresolved {
    size_t nops;  uint32_t ntxn, ncommitted, recovered, aborted, dropped;
    uint64_t appends, reads, elements;
    uint32_t keys, incompatible_keys;             /* keys with a spine / with an incompatible read */
    uint64_t spine_elements, chain_entries, ww, wr, rw;
    uint64_t g1a_reads, g1b_reads, dangling_reads, duplicate_reads, incompatible_reads, internal_reads;
    uint64_t unobserved_appends;
    uint32_t g1a_txns, g1b_txns;
    const uint8_t *fate;         /* [ntxn] 0 committed, 1 aborted, 2 dropped, 3 recovered */
    const uint32_t *cid;         /* [ntxn] */
    const uint32_t *txn_of_cid;  /* [ncommitted] */
    const uint8_t *txn_g1;       /* [ntxn] */
    uint32_t n_listed;           /* min(cap, flagged reads) */
    const uint64_t *listed_op;   /* ascending read op index */
    const uint8_t *listed_flag;  /* its flags */
    const uint8_t *rflag;        /* [nops] HSC_RD_* | HSC_LRD_*; with HSC_RESOLVE_ARRAYS */
    const uint64_t *spine_op;    /* [keys] the read op that is the key's spine; with HSC_RESOLVE_ARRAYS */
    float ms;                    /* device time of the whole call */
} hsc_lresolved;
int hsc_dep_graph_resolve_lists(hsc_ctx *ctx, const hsc_lhistory *h, unsigned flags, hsc_lresolved *out);
/* A build of the last list resolve's ncommitted txns (cid space) from its edge
 * rows alone: no ops, the rows take the staged rw pairs' place.  A staged
 * real-time order (of ncommitted txns) joins as in any build; staged rw pairs
 * are refused with HSC_EINVAL and stay staged for a later build.
 * HSC_ESTATE when no list resolve came first.  The anomaly, snapshot-isolation
 * and SCC entries run unchanged on this build.  Here ww edges may go down in
 * id, so a cycle of ww edges alone (G0) is possible; hsc_dep_graph_anomalies
 * classes it G1c, since it is an E1 cycle (see the note there). */
int hsc_dep_graph_build_lists(hsc_ctx *ctx, int flags, hsc_graph_stats *stats);
/* ---- internal consistency: a txn's reads against its own earlier ops -------
 * Elle's :internal, the INT axiom of read atomic: it needs no version order and
 * no graph, only each txn's own ops.  Both entries are pure functions of the
 * history the last successful resolve of their kind uploaded
 * (hsc_dep_graph_internal: hsc_dep_graph_resolve; hsc_dep_graph_internal_lists:
 * hsc_dep_graph_resolve_lists): they read the device copy, upload nothing, and
 * leave what the resolve keeps for its build untouched.  Either may be called
 * any number of times until the next resolve of its kind, before or after the
 * build, the anomaly / SI entries and staged real-time edges, and answers the
 * same.  HSC_RD_INTERNAL and internal_reads of the resolves keep their meaning
 * (a read that observed its own txn's write, counted only).
 * For a txn t and a key k let o_1 .. o_m be t's ops on k in program order
 * (array order; they need not be contiguous).
 * Value histories.  A read o_j with j > 1 is constrained, its anchor o_{j-1}
 * (a read or a write); it is bad iff value[o_j] != value[o_{j-1}]
 * (HSC_VAL_INIT compares like any value).  A read with j = 1 is unconstrained.
 * bad / anchor_op are computed for every read whatever its txn's status; the
 * counters, txn_bad and the listed reads cover the reads of txns in the
 * resolve's committed set C, as the resolve's own counters do.
 * List histories.  Only HSC_TXN_OK txns are checked (the list resolve ignores
 * every other read throughout; such reads get bad = 0 and no anchor).  For a
 * read o_j let p be the latest earlier read among o_1 .. o_{j-1}, A the
 * elements appended by the ops strictly between p and o_j in order (from o_1
 * when there is no p), a = |A|:
 *   p exists:          constrained, anchor p; consistent iff len_j == len_p + a
 *                      and list_j == list_p || A element for element;
 *   no p, a > 0:       constrained, anchor o_1; consistent iff len_j >= a and
 *                      the last a elements of list_j equal A;
 *   no p, a == 0:      unconstrained.
 * A read is bad iff it is constrained and not consistent.  compared_elements =
 * the sum over constrained reads whose length condition holds of len_p + a
 * (p exists) or a (no p): a read that fails the length condition is bad
 * without an element compared, so the number is exact.
 * HSC_ESTATE: no successful resolve of the kind came before (also after one
 * that failed).  HSC_EDEVICE: a host-only context.  HSC_EINVAL: a NULL
 * argument.  An empty history succeeds with every field zero.  The arrays are
 * host memory owned by the context, never NULL (bad and anchor_op hold nothing
 * without HSC_INTERNAL_ARRAYS), valid until the next graph call.  The sharded
 * path (hsc_multi_graph_scc) has no such entry. */
#define HSC_INTERNAL_ARRAYS   1      /* flags: also copy the per-op arrays back */
#define HSC_INTERNAL_LIST_CAP 4096
typedef struct hsc_internal_report {
    size_t nops;  uint32_t ntxn;
    uint64_t checked_reads;        /* counted reads that are constrained */
    uint64_t bad_reads;            /* of those, the inconsistent ones */
    uint64_t compared_elements;    /* list histories (above); value histories: 0 */
    uint32_t bad_txns;
    const uint8_t  *txn_bad;       /* [ntxn] 1: a counted txn with a bad read */
    uint32_t n_listed;             /* min(cap, bad_reads) */
    const uint64_t *listed_op;     /* ascending read op index */
    const uint64_t *listed_anchor; /* its anchor op */
    const uint8_t  *bad;           /* [nops]; with HSC_INTERNAL_ARRAYS */
    const uint64_t *anchor_op;     /* [nops] UINT64_MAX: unconstrained or a write; with HSC_INTERNAL_ARRAYS */
    int sort_packed;               /* the (txn, key) sort ran as packed single words */
    float ms;                      /* device time of the whole call */
} hsc_internal_report;
int hsc_dep_graph_internal(hsc_ctx *ctx, unsigned flags, hsc_internal_report *out);
int hsc_dep_graph_internal_lists(hsc_ctx *ctx, unsigned flags, hsc_internal_report *out);

/* ---- linearizability of compare-and-set register histories -----------------
 * knossos' checker/linearizable over model/cas-register-comdb2, the checker of
 * the reference's register-tester, its nemesis variant, the filetest and (per
 * key, through independent/checker) the dirty-reads test
 * (linearizable/jepsen/src/comdb2/core.clj:564-613): a search over
 * linearizations, not a dependency graph.  DESIGN.md §5j.
 * ops: the ops that may have taken effect (the caller leaves :fail ops out),
 * each on one key; [invoke, complete] are history positions, complete ==
 * HSC_RT_OPEN: the op never completed (:info or unpaired) and may take effect
 * at any later point or never.  Equal positions overlap (calls are ordered
 * before returns).
 * Model (knossos/model.clj:67-93): the state is the register's value, init[key]
 * (NULL: every key starts HSC_LIN_NIL).  write a: state := a.  cas [a b]: legal
 * iff state == a, then state := b.  read a: legal iff a == HSC_LIN_NIL or
 * a == state (the reference's nil-read wildcard).
 * Search (knossos/linear.clj:66-129, 218-271): a configuration is (state, the
 * pending ops already linearized); the completion of op i keeps the
 * configurations that hold i and closes the others under linearizing pending
 * ops other than i, then i.  The first completion that leaves no configuration
 * is the key's failing op.
 * Each key is searched by one workgroup in one launch.  Its limits are
 * HSC_LIN_SLOTS ops pending at once on the key (open ops stay pending; open
 * reads are dropped first: they change nothing and nothing waits for them) and
 * HSC_LIN_CAP configurations alive inside one completion step; past either the
 * key's verdict is HSC_LIN_UNKNOWN with the cause, as knossos answers :unknown
 * when it runs out of memory -- never an error, never a wrong verdict, and the
 * other keys of the call are judged.
 * HSC_EINVAL: a NULL argument, key[i] >= nkeys, an unknown f, or invoke >=
 * complete on a closed op.  HSC_EDEVICE: a host-only context.  nops == 0 or
 * nkeys == 0 succeed.  The report's arrays are host memory owned by the
 * context, never NULL, valid until the next hsc_linear_check on it. */
#define HSC_LIN_READ  0
#define HSC_LIN_WRITE 1
#define HSC_LIN_CAS   2
#define HSC_LIN_NIL   INT64_MIN
#define HSC_LIN_SLOTS 32
#define HSC_LIN_CAP   4096
#define HSC_LIN_BAD     0   /* verdict */
#define HSC_LIN_OK      1
#define HSC_LIN_UNKNOWN 2
#define HSC_LIN_CAUSE_SLOTS   1   /* cause of an UNKNOWN key */
#define HSC_LIN_CAUSE_CONFIGS 2
typedef struct hsc_lin_ops {
    size_t nops;  uint32_t nkeys;
    const uint32_t *key;       /* [nops] 0 .. nkeys-1 */
    const uint8_t  *f;         /* [nops] HSC_LIN_READ / _WRITE / _CAS */
    const int64_t  *a, *b;     /* [nops] read: a = value; write: a = value; cas: a = cur, b = new */
    const uint64_t *invoke;    /* [nops] */
    const uint64_t *complete;  /* [nops] HSC_RT_OPEN: never completed */
    const int64_t  *init;      /* [nkeys] or NULL */
} hsc_lin_ops;
typedef struct hsc_lin_report {
    uint32_t nkeys;
    const uint8_t  *verdict;        /* [nkeys] */
    const uint8_t  *cause;          /* [nkeys] 0 unless UNKNOWN */
    const uint32_t *fail_op;        /* [nkeys] BAD: the op whose completion left no configuration; else ~0u */
    const uint32_t *prev_ok;        /* [nkeys] BAD: the key's last op completed before it (~0u: none); else ~0u */
    const uint32_t *peak_configs;   /* [nkeys] most configurations alive inside one step (UNKNOWN: of the steps done) */
    const uint32_t *final_configs;  /* [nkeys] the set at the end (BAD / UNKNOWN: as it stood before the op) */
    const uint64_t *state_off;      /* [nkeys + 1] */
    const int64_t  *state_val;      /* BAD keys: the distinct register values of the set before the failing op, ascending */
    uint32_t bad, unknown;          /* keys */
    uint64_t events;                /* calls and returns in the event programs launched */
    uint64_t expanded;              /* configurations expanded, over the completed steps */
    uint64_t dropped_open_reads;
    float ms;                       /* device time of the whole call */
} hsc_lin_report;
int hsc_linear_check(hsc_ctx *ctx, const hsc_lin_ops *ops, hsc_lin_report *out);

/* The wide tier: hsc_linear_check, then the keys it leaves HSC_LIN_UNKNOWN for
 * `slots` or `configs` searched again from their first event with the two hash
 * sets in device memory (one workgroup per key; DESIGN.md §5j "The wide
 * tier").  The step, the event order and the lowest-free-slot rule are the
 * same; the caps are HSC_LIN_WIDE_SLOTS ops pending at once, max_configs
 * configurations alive inside one step and HSC_LIN_WIDE_STATES distinct
 * non-nil values on the key (the state id is 15 bits of the configuration
 * word; cause HSC_LIN_CAUSE_STATES, the key is not launched).  A key the first
 * pass judges OK or BAD keeps those fields, bit for bit, with tier 0; an
 * escalated key has tier 1 and every field from the wide search, its events
 * and expansions in base.events and base.expanded in place of the first
 * pass's.  HSC_LIN_WIDE_ONLY skips the first pass: every key with events goes
 * wide.
 * Budget: after every completed step, a key whose expansions so far exceed
 * max_expanded is HSC_LIN_UNKNOWN / HSC_LIN_CAUSE_BUDGET with peak and final
 * as of the steps done.  A step expands at most max_configs entries and the
 * counts are of sets, so the verdict is deterministic and the launch bounded.
 * The default, 2^25, is 5.7 s of one key's worst case at the 5.9 M expansions/s
 * measured.
 * One key's tables take table_bytes = 32 * max_configs device bytes; a launch
 * round searches arena_bytes / table_bytes keys.
 * HSC_EINVAL as hsc_linear_check, and for a max_configs that is not a power of
 * two in [HSC_LIN_WIDE_MIN_CAP, HSC_LIN_WIDE_MAX_CAP], unknown flags, or a
 * non-zero arena_bytes below table_bytes.  The report's arrays are owned by
 * the context until its next linear call of either kind. */
#define HSC_LIN_WIDE_SLOTS    48          /* ops pending at once in the wide tier */
#define HSC_LIN_WIDE_MIN_CAP  8192u       /* max_configs: a power of two in [MIN, MAX] */
#define HSC_LIN_WIDE_MAX_CAP  (1u << 22)
#define HSC_LIN_WIDE_STATES   32767       /* distinct non-nil values of one key in the wide tier */
#define HSC_LIN_CAUSE_BUDGET  3           /* max_expanded passed */
#define HSC_LIN_CAUSE_STATES  4           /* more than HSC_LIN_WIDE_STATES values on the key */
#define HSC_LIN_WIDE_ONLY     1u          /* flags: skip the LDS tier, every key with events goes wide */
typedef struct hsc_lin_wide_limits {
    uint32_t max_configs;    /* 0: default 1 << 20 */
    uint32_t flags;
    uint64_t max_expanded;   /* per key; 0: default 1 << 25 */
    uint64_t arena_bytes;    /* device bytes for wide tables per round; 0: default 1 GiB */
} hsc_lin_wide_limits;
typedef struct hsc_lin_wide_report {
    hsc_lin_report base;       /* as hsc_linear_check's, every key's fields from the tier that judged it */
    const uint8_t *tier;       /* [nkeys] 0: LDS tier (or no events), 1: wide tier */
    uint32_t escalated;        /* keys sent to the wide tier */
    uint32_t resolved;         /* of them, no longer UNKNOWN */
    uint32_t rounds;           /* wide launches */
    uint64_t wide_expanded;
    uint64_t table_bytes;      /* device bytes of one key's wide tables */
    float wide_ms;             /* device time of the wide rounds; base.ms is the whole call */
} hsc_lin_wide_report;
int hsc_linear_check_wide(hsc_ctx *ctx, const hsc_lin_ops *ops, const hsc_lin_wide_limits *limits /* NULL: defaults */,
                          hsc_lin_wide_report *out);

/* ---- the accounting checkers: set, total-queue, bank -------------------------
 * The other two workloads of the reference's Jepsen suite
 * (linearizable/jepsen/src/comdb2/core.clj: set-client and sets-test :223-272,
 * the bank client, checker and tests :71-177, :274-318).  Neither is a graph or a search: both count.  DESIGN.md §5k.
 * hsc_tally_check is checker/set (jepsen/checker.clj:108-154) and, with
 * HSC_TALLY_MULTISET, checker/total-queue (:163-218).  Like the reference it
 * filters by :type and :f only and never pairs an invoke with its completion;
 * the caller hands over three arrays of values, in any order:
 *               set                         total-queue
 *   attempt     :invoke :add                :invoke :enqueue
 *   ack         :ok :add                    :ok :enqueue
 *   seen        the last :ok :read's set    :ok :dequeue
 * For a value let A, K, S be its occurrences in attempt, ack and seen, each
 * clamped to 1 without HSC_TALLY_MULTISET (a set holds a value once).  Its
 * multiplicity in the five classes:
 *   ok          min(S, A)                         (:134 / :185)
 *   unexpected  S if A == 0, else 0               (:137 / :190-193)
 *   duplicated  max(S - A, 0) if A > 0, else 0    (:197-199; always 0 for a set)
 *   lost        max(K - S, 0)                     (:140 / :203)
 *   recovered   max(min(S, A) - K, 0)             (:144 / :207)
 * K may exceed A (a completion without its invoke): the reference counts it so.
 * Per class: count = the sum of the multiplicities, distinct = the values
 * whose multiplicity is not zero, and the class as runs -- a run is a maximal
 * stretch of consecutive integers v, v + 1, ... of one multiplicity, (lo, hi,
 * mult), ascending (signed order; INT64_MAX is not followed by INT64_MIN),
 * what util/integer-interval-set-str (jepsen/util.clj:483-508) prints for a
 * set.  runs is exact; the first n_listed = min(runs, HSC_TALLY_LIST_CAP) are
 * listed.  attempts / acks / seen: the distinct values of each input for a
 * set, its elements with HSC_TALLY_MULTISET -- (count attempts) of the
 * reference either way, the denominator of its fractions.  distinct: the
 * distinct values of the three inputs together.  valid: no lost and no
 * unexpected value (:146 / :209).  The caller decides what a history without a
 * read means (:129-131); an empty seen is an empty read here.
 * HSC_EINVAL: a NULL argument (an array may be NULL when its length is 0), a
 * flag other than HSC_TALLY_MULTISET, or n_attempt + n_ack + n_seen >
 * 0x7FFFFFFF: the sort carries each row's index in 32 bits and every position
 * is scanned as a u32, the bound of the graph entries' op counts.
 * HSC_EDEVICE: a host-only context.  Empty inputs succeed with valid = 1.
 * The arrays are host memory owned by the context, never NULL, valid until
 * the next hsc_tally_check on it.  Nothing a resolve, a build or any other
 * entry left on the context is touched: the sort has rows of its own. */
#define HSC_TALLY_MULTISET 1u
#define HSC_TALLY_LIST_CAP 4096
enum { HSC_TALLY_OK, HSC_TALLY_UNEXPECTED, HSC_TALLY_DUPLICATED, HSC_TALLY_LOST, HSC_TALLY_RECOVERED, HSC_TALLY_NCLASS };
typedef struct hsc_tally_in {
    size_t n_attempt, n_ack, n_seen;
    const int64_t *attempt, *ack, *seen;
} hsc_tally_in;
typedef struct hsc_tally_class {
    uint64_t count, distinct, runs;
    uint32_t n_listed;             /* min(runs, HSC_TALLY_LIST_CAP) */
    const int64_t *lo, *hi;        /* [n_listed] ascending */
    const uint32_t *mult;          /* [n_listed] */
} hsc_tally_class;
typedef struct hsc_tally_report {
    uint64_t attempts, acks, seen, distinct;
    int valid;                     /* no lost, no unexpected */
    hsc_tally_class cls[HSC_TALLY_NCLASS];
    int sort_packed;               /* the (value, source) sort ran as packed single words */
    float ms;                      /* device time of the whole call */
} hsc_tally_report;
int hsc_tally_check(hsc_ctx *ctx, const hsc_tally_in *in, unsigned flags, hsc_tally_report *out);
/* hsc_bank_check is bank-checker (core.clj:152-177): read i holds the balances
 * balance[off[i] .. off[i + 1]) of an :ok :read, n and total are the test's
 * :model.  Per read, as the reference's cond: kind 1 (wrong-n) when its length
 * is not n, found = the length, and its sum is not looked at; else kind 2
 * (wrong-total) when its sum is not total; else 0; found = the sum for kinds 0
 * and 2.  Sums wrap in 64 bits, where the reference's (reduce + balances)
 * would throw an ArithmeticException (integer overflow) instead of answering.
 * negatives[i]: the balances of read i below zero, whatever its kind;
 * reads_with_negative: the reads with one.  Neither enters valid: the
 * reference's checker does not look at signs (its docstring does; the client
 * refuses a transfer that would go negative, :112-116), so a negative balance
 * is reported but is not the verdict.  valid: no bad read.  The first n_listed
 * = min(bad, HSC_BANK_LIST_CAP) bad reads are listed in read order.  A read
 * may have any length, 0 included, whatever n is.
 * HSC_EINVAL: a NULL argument (off and balance may be NULL when n_reads is 0,
 * balance when off[n_reads] is 0), an off that does not start at 0 or
 * descends, n_reads > 0x7FFFFFFF or off[n_reads] > 0xFFFFFFFF (the bad reads'
 * positions and a read's negatives are u32).  HSC_EDEVICE: a host-only
 * context.  n_reads == 0 succeeds with valid = 1.  The arrays are host memory
 * owned by the context, never NULL, valid until the next hsc_bank_check. */
#define HSC_BANK_LIST_CAP 4096
typedef struct hsc_bank_in {
    size_t n_reads;
    const uint64_t *off;           /* [n_reads + 1] */
    const int64_t *balance;        /* [off[n_reads]] */
    uint64_t n;  int64_t total;    /* the model */
} hsc_bank_in;
typedef struct hsc_bank_report {
    uint64_t n_reads, bad, wrong_n, wrong_total, reads_with_negative;
    int valid;
    const uint8_t *kind;           /* [n_reads] 0 fine, 1 wrong-n, 2 wrong-total */
    const int64_t *found;          /* [n_reads] */
    const uint32_t *negatives;     /* [n_reads] */
    uint32_t n_listed;
    const uint64_t *listed_read;   /* [n_listed] ascending */
    float ms;                      /* device time of the whole call */
} hsc_bank_report;
int hsc_bank_check(hsc_ctx *ctx, const hsc_bank_in *in, hsc_bank_report *out);

/* ---- the perf checker: latencies, latency quantiles, completion rates --------
 * checker/perf (jepsen/checker.clj:288-309), the member every composed checker
 * of core.clj carries beside its workload's own: the data sets of the three
 * graphs of jepsen/checker/perf.clj and its rate breakdown.  DESIGN.md §5l.
 * The history is one row per op in history order: type (HSC_OP_INVOKE / _OK /
 * _FAIL / _INFO), f (an id below nf), process (an id: the host interns any
 * value, an integer or :nemesis alike), client (nonzero when :process is an
 * integer -- the rate graph's (comp integer? :process), perf.clj:302) and time
 * in ns.
 * Pairing is util/history->latencies (jepsen/util.clj:553-587): an invoke
 * becomes its process's outstanding invoke (replacing an older one), any other
 * op pairs with its process's outstanding invoke and removes it.  Per op:
 * completion_of (the op that completed this invoke, else -1), invoke_of (the
 * invoke this op completed, else -1), latency (ns, signed and never clamped:
 * time[completion] - time[invoke]; 0 where completion_of is -1).  invokes =
 * paired + unpaired; orphans: the ops that are no invoke and completed none.
 * Windows: time t lies in window (long)(((double)t / 1e9) / dt), the
 * reference's two double divisions (perf.clj:15-25, :129-134, :307-309),
 * computed so on the device.  Accepted are the times whose window index is
 * below 2^32 under both q_dt and r_dt -- every int64 time when both windows are
 * at least 2.15 s -- a time past that is HSC_EINVAL.
 * Latency cells: the paired invokes by (f, window of the invoke's time under
 * q_dt).  cells is exact; the first cells_listed = min(cells,
 * HSC_PERF_CELL_CAP) are listed in (f, window) order with their count and, per
 * q[j], the latency at index min(count - 1, (long)floor(count * q[j])) of the
 * cell's ascending latencies (perf.clj:45-55): cell_lat[k * nq + j].
 * Rate cells: the ops that are no invoke and have client set, by (f, type,
 * window of their time under r_dt), listed like the latency cells (rate_cells
 * exact, rate_listed).  counts[f * 4 + type]: the ops of that f and type that
 * are no invoke, whatever client says (perf.clj:113-127; its ::all margins are
 * sums over this matrix).  t_max: the largest time, 0 for an empty history.
 * With HSC_PERF_ARRAYS also the raw partition (perf.clj:96-102): raw_op holds
 * the paired invokes grouped by g = f * 4 + type of their completion, history
 * order inside a group, group g at raw_op[raw_off[g] .. raw_off[g + 1]);
 * without it completion_of / invoke_of / latency / raw_op are empty and
 * raw_off is all zero.
 * HSC_PERF_CELL_CAP: a test of 8 :f values fills 65536 rate cells (three
 * completion types, 10 s windows) after 7.5 hours and as many latency cells
 * (30 s windows) after 68 hours; the suite's tests run minutes.  A longer
 * history still gets every exact scalar and the first cells.
 * HSC_EINVAL: a NULL argument (an array may be NULL when n is 0, q when nq is
 * 0), nf of 0 or above 65536, an f >= nf, a type above HSC_OP_INFO, a negative
 * time or one past the accepted windows, a q outside [0, 1] or NaN, nq above
 * 64, a window that is not a finite number above 0, a flag other than
 * HSC_PERF_ARRAYS, or n > 0x7FFFFFFF (every position is scanned as a u32).
 * HSC_EDEVICE: a host-only context.  An empty history succeeds with empty
 * outputs.  The arrays are host memory owned by the context, never NULL, valid
 * until the next hsc_perf_check on it.  Nothing a resolve, a build, a tally or
 * a linear check left on the context is touched: the sorts have rows of their
 * own. */
#define HSC_PERF_ARRAYS 1u
#define HSC_PERF_CELL_CAP 65536
#define HSC_PERF_MAX_Q 64
#define HSC_PERF_MAX_F 65536
enum { HSC_OP_INVOKE, HSC_OP_OK, HSC_OP_FAIL, HSC_OP_INFO };
enum { HSC_PERF_MS_ROWS, HSC_PERF_MS_PAIR, HSC_PERF_MS_CELLS, HSC_PERF_MS_RATE, HSC_PERF_MS_RAW, HSC_PERF_NPHASE };
typedef struct hsc_perf_in {
    size_t n;
    const uint8_t *type;           /* [n] */
    const uint32_t *f;             /* [n] below nf */
    const uint32_t *process;       /* [n] */
    const uint8_t *client;         /* [n] */
    const int64_t *time;           /* [n] ns, >= 0 */
    uint32_t nf;
    uint32_t nq;
    const double *q;               /* [nq] in [0, 1] */
    double q_dt, r_dt;             /* the quantile and the rate window, seconds */
} hsc_perf_in;
typedef struct hsc_perf_report {
    uint64_t n, invokes, paired, unpaired, orphans;
    int64_t t_max;
    uint64_t cells, rate_cells;
    uint32_t cells_listed, rate_listed;
    const uint32_t *cell_f, *cell_bucket, *cell_count;    /* [cells_listed] */
    const int64_t *cell_lat;                              /* [cells_listed * nq] */
    const uint32_t *rate_f, *rate_type, *rate_bucket, *rate_count;  /* [rate_listed] */
    const uint64_t *counts;                               /* [nf * 4] */
    size_t n_arrays;                                      /* n with HSC_PERF_ARRAYS, else 0 */
    const int32_t *completion_of, *invoke_of;             /* [n_arrays] */
    const int64_t *latency;                               /* [n_arrays] */
    size_t n_raw;                                         /* paired with HSC_PERF_ARRAYS, else 0 */
    const uint32_t *raw_op;                               /* [n_raw] */
    const uint32_t *raw_off;                              /* [nf * 4 + 1] */
    int sort_packed;               /* bit 0: the process sort ran as packed single words, 1: the latency cells', 2: the rate cells', 3: the raw partition's */
    float ms;                      /* device time of the whole call */
    float phase_ms[HSC_PERF_NPHASE]; /* of it: upload + rows, pairing, latency cells, rate, raw partition */
} hsc_perf_report;
int hsc_perf_check(hsc_ctx *ctx, const hsc_perf_in *in, unsigned flags, hsc_perf_report *out);

/* ---- the counter and queue checkers, per independent key ---------------------
 * checker/counter (jepsen/checker.clj:220-272) and checker/queue (:87-106), the
 * two members of checker.clj that are sequential reductions, each judged for
 * many keys in one call: what independent/checker (jepsen/independent.clj:
 * 252-290) wraps around them.  key[i] < nkeys names the row's subhistory; key
 * may be NULL when nkeys is 1.  Keys are judged independently and reported per
 * key; a key without rows is ok.  DESIGN.md §5m.
 * hsc_counter_check takes one row per op in history order: type (HSC_OP_*), f
 * (HSC_CNT_ADD / _READ / _OTHER), process (an id) and value, HSC_CNT_NIL
 * standing for nil.  Per key it is history/complete (knossos/history.clj:
 * 87-171) followed by the checker's loop (checker.clj:240-272).
 * Completion: a process's rows of one key without the :info rows must
 * alternate invoke, ok or fail, invoke, ...  A row is malformed, by kind:
 *   1  an invoke whose predecessor in that sequence is an invoke (history.clj:
 *      101-106 throws)
 *   2  an ok or fail whose predecessor is no invoke, or that has none (:114,
 *      :128)
 *   3  a fail whose value differs from its invoke's (:132)
 *   4  a completion whose f differs from its invoke's.  The reference does not
 *      check this and would build a nonsense triple from the two; here the row
 *      is malformed
 *   5  an add invoke, an ok add or an ok read whose effective value is nil
 *      (the loop's + and <= throw on it)
 * (a row of several kinds reports the smallest).  A key with a malformed row
 * has verdict HSC_CNT_UNKNOWN -- the reference throws and checker/check-safe
 * answers :unknown -- malformed_op[k] is the smallest such op index,
 * malformed_kind[k] that row's kind, and the key lists no reads.  Other keys:
 * malformed_op ~0u, kind 0.
 * Effective value: an invoke completed by an ok takes the completion's value
 * (history.clj:117-119); every other invoke keeps its own.
 * Bounds: upper after row i = the sum of the effective values of the key's add
 * invokes at or before i, those that later fail or end in :info included (the
 * reference never looks at :fails?); lower after row i = the sum of the values
 * of its ok adds at or before i.  Both wrap in 64 bits, as hsc_bank_check's
 * sums do, where the reference's + would throw on overflow.
 * Reads: every ok read at row j with its invoke at row i yields the triple
 * (lower after i, value[j], upper after j), listed per key in order of j:
 * key k's reads are [read_off[k], read_off[k + 1]) of lower / value / upper /
 * read_op (read_op = j).  A triple is an error unless lower <= value <= upper
 * (signed; both bounds inclusive).  errors[k] and bad_reads are exact; the
 * first n_listed = min(bad_reads, HSC_COUNTER_LIST_CAP) error reads are listed
 * as ascending indices into the read arrays.  Verdict HSC_CNT_BAD: a key with
 * an error read.  :max-absolute-error / :max-relative-error are named by the
 * reference's docstring and computed nowhere; nor here.
 * HSC_EINVAL: a NULL argument (an array may be NULL when n is 0, key when
 * nkeys is 1), nkeys of 0, a key >= nkeys, a type above HSC_OP_INFO, an f above
 * HSC_CNT_OTHER, or n > 0x7FFFFFFF -- all found on the host before any launch.
 * HSC_EDEVICE: a host-only context.  n == 0 succeeds with every key ok.  The
 * arrays are host memory owned by the context, never NULL, valid until the
 * next hsc_counter_check on it.  Nothing another entry left on the context is
 * touched: the sorts have rows of their own. */
#define HSC_COUNTER_LIST_CAP 4096
#define HSC_CNT_NIL INT64_MIN
enum { HSC_CNT_ADD, HSC_CNT_READ, HSC_CNT_OTHER };
enum { HSC_CNT_OK, HSC_CNT_BAD, HSC_CNT_UNKNOWN };  /* a key's verdict, both entries */
typedef struct hsc_counter_in {
    size_t n;
    const uint8_t *type;           /* [n] HSC_OP_* */
    const uint8_t *f;              /* [n] HSC_CNT_* */
    const uint32_t *process;       /* [n] */
    const int64_t *value;          /* [n] */
    const uint32_t *key;           /* [n] below nkeys; NULL: all 0 (nkeys == 1) */
    uint32_t nkeys;
} hsc_counter_in;
typedef struct hsc_counter_report {
    uint32_t nkeys;
    uint32_t bad, unknown;         /* keys by verdict */
    const uint8_t *verdict;        /* [nkeys] */
    const uint32_t *malformed_op;  /* [nkeys] ~0u: none */
    const uint8_t *malformed_kind; /* [nkeys] */
    const uint32_t *read_off;      /* [nkeys + 1] */
    uint64_t reads, bad_reads;
    const int64_t *lower, *value, *upper;  /* [reads] */
    const uint32_t *read_op;       /* [reads] the ok read's op index */
    const uint32_t *errors;        /* [nkeys] error reads of the key */
    uint32_t n_listed;
    const uint32_t *listed_read;   /* [n_listed] ascending */
    int sort_packed;               /* bit 0: the pairing sort ran as packed single words, 1: the key sort */
    float ms;                      /* device time of the whole call */
} hsc_counter_report;
int hsc_counter_check(hsc_ctx *ctx, const hsc_counter_in *in, hsc_counter_report *out);
/* hsc_queue_check takes only the rows checker/queue selects (checker.clj:
 * 95-100), in history order: every :invoke :enqueue, whatever became of it (a
 * failed enqueue is in the queue, as in the reference), and every :ok :dequeue;
 * per row f (HSC_Q_ENQUEUE / _DEQUEUE), value and key.  Per key it computes
 * (reduce model/step model rows) for jepsen/model.clj's unordered-queue
 * (:73-85) or, with HSC_QUEUE_FIFO, fifo-queue (:87-105).  Inconsistent absorbs
 * every later step, so a key's error is its first illegal dequeue in history
 * order: error_row[k] (an index into the rows, ~0u: none) and error_kind[k]:
 *   1  unordered: the value's pending count is 0; fifo: the queue's head is
 *      another value -- "can't dequeue V"
 *   2  fifo: the queue is empty -- "can't dequeue V from empty queue" (checked
 *      first, as the model's cond does)
 * final_len[k]: the elements left, 0 for a bad key.  With HSC_QUEUE_FINAL the
 * final queues too: key k's at [final_off[k], final_off[k + 1]) of final_val /
 * final_mult -- unordered: the distinct remaining values ascending (signed)
 * with their multiplicity; fifo: the remaining values in queue order,
 * multiplicity 1.  No cap: a final queue is at most the enqueues.  Without the
 * flag the two arrays are empty and final_off is all zero.
 * HSC_EINVAL: a NULL argument (an array may be NULL when n is 0, key when
 * nkeys is 1), nkeys of 0, a key >= nkeys, an f above HSC_Q_DEQUEUE, a flag
 * other than the two, or n > 0x7FFFFFFF -- found on the host before any
 * launch.  HSC_EDEVICE: a host-only context.  n == 0 succeeds with every key
 * ok.  Ownership as hsc_counter_check: valid until the next hsc_queue_check. */
#define HSC_QUEUE_FIFO 1u
#define HSC_QUEUE_FINAL 2u
enum { HSC_Q_ENQUEUE, HSC_Q_DEQUEUE };
typedef struct hsc_queue_in {
    size_t n;
    const uint8_t *f;              /* [n] HSC_Q_* */
    const int64_t *value;          /* [n] */
    const uint32_t *key;           /* [n] below nkeys; NULL: all 0 (nkeys == 1) */
    uint32_t nkeys;
} hsc_queue_in;
typedef struct hsc_queue_report {
    uint32_t nkeys;
    uint32_t bad;                  /* keys with an error */
    const uint8_t *verdict;        /* [nkeys] HSC_CNT_OK / HSC_CNT_BAD */
    const uint32_t *error_row;     /* [nkeys] ~0u: none */
    const uint8_t *error_kind;     /* [nkeys] 0 none, 1 absent / mismatch, 2 empty */
    const uint32_t *final_len;     /* [nkeys] */
    const uint32_t *final_off;     /* [nkeys + 1] */
    uint64_t n_final;              /* final_off[nkeys] */
    const int64_t *final_val;      /* [n_final] */
    const uint32_t *final_mult;    /* [n_final] */
    int sort_packed;               /* the entry's sort ran as packed single words */
    float ms;                      /* device time of the whole call */
} hsc_queue_report;
int hsc_queue_check(hsc_ctx *ctx, const hsc_queue_in *in, unsigned flags, hsc_queue_report *out);
/* cover_dev[ntxn of the last build] := 1 inside a backward edge's interval. */
int hsc_dep_graph_cover(hsc_ctx *ctx, uint8_t *cover_dev);
/* Edges of the last build with both ends covered, as rows src << 32 | dst
 * (sorted): *m of them, min(cap, *m) copied to rows_dev (NULL: count only). */
int hsc_dep_graph_cut(hsc_ctx *ctx, const uint8_t *cover_dev, uint64_t *rows_dev, size_t cap,
                      size_t *m);
/* scc_dev[ntxn] := largest txn of each txn's component in the graph whose
 * only edges between covered nodes are rows_dev[m] (~0 rows are padding);
 * uncovered txns are their own component.  HSC_EINVAL if a row leaves the
 * cover.  Leaves the last build's edges in place (own buffers). */
int hsc_dep_graph_scc_cut(hsc_ctx *ctx, uint32_t ntxn, const uint8_t *cover_dev,
                          const uint64_t *rows_dev, size_t m, uint32_t *scc_dev,
                          hsc_graph_stats *stats);

/* Sharded SCC on a multi context (config 4 over N GPUs behind the C ABI):
 * ops[i] = local member i's key shard of the history, device-resident on its
 * GPU (every WW/WR/RW edge belongs to one key).  Per member: raw build and
 * cover; covers OR-ed (RCCL MAX all-reduce across ranks, an OR over peer
 * buffers in one process); cuts; the union of the cuts (RCCL all-gather,
 * padded with ~0 rows, across ranks; peer copies to member 0 in one
 * process); its colouring SCC.  scc_dev[i] (ntxn u32 on member i's GPU;
 * scc_dev[0] required, others may be NULL) = the largest txn of each txn's
 * component, as hsc_dep_graph_scc of the whole history.  stats: member 0's
 * SCC stats, build_ms = the slowest local build, edges = rows of the cut
 * union.  Collective on a per-rank context. */
typedef struct hsc_ops_dev {
    size_t nops;
    const uint32_t *txn;       /* [nops] */
    const uint64_t *key;       /* [nops] */
    const uint8_t *is_write;   /* [nops] */
    const uint32_t *observed;  /* [nops] writer txn, 0xFFFFFFFF = initial version */
} hsc_ops_dev;
int hsc_multi_graph_scc(hsc_ctx *ctx, const hsc_ops_dev *ops, uint32_t ntxn, uint32_t *const *scc_dev,
                        hsc_graph_stats *stats);
/* Host ms of the last hsc_multi_graph_scc: build + cover, cover merge, cuts +
 * their union, SCC. */
int hsc_multi_graph_phase_ms(hsc_ctx *ctx, double out[4]);

/* ---- harness support (tests / bench; not on the check path) --------------
 * CurRangeArr objects as comdb2 holds a received read set (db/comdb2.h:1105-1124;
 * strdup'd table names, malloc'd keys, serial_readset_get db/osqlcomm.c:948-993),
 * one per read set of rs: *out = void *[ntxn] of hsc_currangearr *. */
int hsc_currangearrs_build(const hsc_readsets *rs, void ***out);
void hsc_currangearrs_free(void **arrs, int n);
/* nthreads caller threads, each checking read sets i = t, t + nthreads, ...
 * of arrs[n] `rounds` times with its own (file, offset) copies of the set's
 * snapshot -- through col (hsc_collector_check) when col != NULL, else one
 * hip_bdb_osql_serial_check per call.  rc_out[n] = last verdicts; per-call
 * latencies summarised in *res. */
typedef struct hsc_concurrent_result {
    double seconds;                             /* wall time of all threads */
    uint64_t calls;
    double lat_mean_us, lat_p50_us, lat_p99_us;  /* per call */
} hsc_concurrent_result;
int hsc_harness_concurrent(hsc_ctx *ctx, hsc_collector *col, void *const *arrs, int n,
                           int nthreads, int rounds, int regop_only, int *rc_out,
                           hsc_concurrent_result *res);
/* The master's commit protocol (db/toblock.c:4757-4836) replayed by nthreads
 * threads over a stream of events: events[k] >= 0 -- txn events[k] begins (its
 * CurRangeArr's snapshot := hsc_window_end); events[k] < 0 -- txn ~events[k]
 * commits.  Threads take events in order (a commit waits for its txn's begin).
 * A commit: commit_lock (a pthread rwlock) read-locked, released and
 * write-locked; while hip_bdb_osql_serial_check(regop_only = 1) on
 * &arr->file / &arr->offset says a newer commit exists: unlock, full check
 * (regop_only = 0; conflict -> abort, rc 1), write-lock again; then the txn's
 * writes are appended at commit LSN hsc_window_end + 1 (hsc_window_append)
 * and the lock released.  Per txn: rc_out (0 committed, 1 aborted),
 * commit_seq (its commit's index, -1 if aborted or without writes),
 * snap_out (the snapshot it began with), check_end_out (the end LSN its last
 * full check returned, 0 if none ran). */
typedef struct hsc_protocol_txn {
    void *arr;                /* CurRangeArr* (file / offset set at begin)   */
    const hsc_write *writes;  /* the txn's writes (commit_lsn ignored)       */
    int nwrites;
    int selectv;              /* arr is a selectv array: a txn without writes
                                 is still checked (one full check, no lock,
                                 db/sqloffload.c:505-524: rc_out 1 if it
                                 conflicts, check_end_out its end) unless arr
                                 is empty; it logs nothing, commit_seq -1.
                                 0: a txn without writes is never checked    */
} hsc_protocol_txn;
typedef struct hsc_protocol_result {
    double seconds;           /* first event to last commit                  */
    uint64_t commits, aborts, regop_probes, full_checks;
    double regop_p50_us, regop_p99_us, regop_p999_us, regop_max_us;
    double full_p50_us, full_p99_us;
    double hold_p50_us, hold_p99_us;  /* commit_lock write-held per commit   */
    double commit_p50_us, commit_p99_us;  /* commit event: first lock to done */
} hsc_protocol_result;
int hsc_harness_commit_protocol(hsc_ctx *ctx, const hsc_protocol_txn *txns, int ntxn,
                                const int *events, int nevents, int nthreads, int *rc_out,
                                int64_t *commit_seq, uint64_t *snap_out, uint64_t *check_end_out,
                                hsc_protocol_result *res);

#ifdef __cplusplus
}
#endif
#endif /* HIP_SERIAL_H */
