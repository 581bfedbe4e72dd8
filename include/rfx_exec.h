/*
 * rfx_exec.h -- the PLANNER of librfx.so (rayforce_amd/csrc/rfx_exec.c): one query over one or several row-range SHARDS.
 *
 * Three layers, top to bottom:
 *   rfx_ops.h   obj_p in, obj_p out: parses the reference's select dict, keeps host columns resident, builds result tables
 *   rfx_exec.h  device columns in, device results out: WHICH kernels run, in which order, under which scope, and how the
 *               shards' partial states merge -- this file.  Every host of the library (rfx_select, the Python test host, bench.py,
 *               a C host with its own object model) plans through these entry points; there is no second planner.
 *   rfx_hip.h   the kernels, one context = one device + one stream
 *
 * What the reference does in the same place: ray_select (core/query.c:607-654) fans a fold / a group index out over its pool's
 * workers in row chunks (pool_run, core/pool.c:369-424; aggr_map, core/aggr.c:375) and merges the per-worker partial states INSIDE
 * the one evaluator process (AGGR_COLLECT core/aggr.c:163-181, unop_fold's second level core/math.c:2206-2228, the sparse path's
 * re-insertion core/index.c:1866-1906).  A shard here is such a worker one level up: a device (or a slice of one) that owns the rows
 * [row0, row0 + n) of every column.
 *
 * Sharding models, all through the same calls:
 *   - ONE process, N devices (the evaluator process of INTEGRATION.md): rfx_exec_create over N contexts, rfx_exec_comm_init_all;
 *     dense group tables merge by ONE fused RCCL all-reduce over xGMI (rfx_dist_group_tables_allreduce_all), everything the host
 *     can fold itself (scopes, scalar partials, flags) is folded on the host.  Every shard is driven by its own host thread.
 *   - several shards on ONE device (RFX_SHARDS=k: how the merge logic is tested on a 1-GPU box): merged by a device kernel.
 *   - one process per device (torch.distributed launches, bench.py --gpus N): the lead context carries an inter-process communicator
 *     (rfx_dist_init, or a transport the host supplies) and the same merges run as collectives.
 *
 * Column addresses: a query's descriptors (rfx_pred_t, rfx_agg_t, key columns) are written with SHARD 0's device addresses; `cols`
 * lists, for every column the query names, its address on every shard.  With one shard `cols` may be NULL.
 * Shard s of an n-row table owns rows rfx_exec_split(n, S, s): equal spans of ceil(n / S) rounded up to 512 rows.
 */
#ifndef RFX_EXEC_H
#define RFX_EXEC_H

#include "rfx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#ifndef __HIPCC_RTC__
#pragma GCC visibility push(default) /* librfx.so is built with -fvisibility=hidden: what the headers under include/ declare is its WHOLE dynamic surface (plugins are
                                      * dlopen'ed RTLD_GLOBAL, core/dynlib.c:131 -- internals must not land in the host's namespace) */
#endif

#define RFX_MAX_SHARDS 16
#define RFX_GROUPS_OWN (RFX_MAX_SHARDS * (4 + 2 * RFX_MAX_KEYS + RFX_EXEC_MAX_AGGS))
#define RFX_EXEC_MAX_AGGS 32 /* more than RFX_MAX_AGGS outputs run as several passes over the same selection / the same groups */

typedef struct rfx_exec rfx_exec_t;

/* ---- shards ---- */
/* The contexts are BORROWED (the caller destroys them after rfx_exec_destroy); several may share a device. */
int rfx_exec_create(rfx_ctx_t *const *ctxs, int nshards, rfx_exec_t **out);
int rfx_exec_destroy(rfx_exec_t *x);
int rfx_exec_shards(const rfx_exec_t *x);
rfx_ctx_t *rfx_exec_ctx(const rfx_exec_t *x, int shard);
void rfx_exec_split(int64_t nrows, int nshards, int shard, int64_t *row0, int64_t *len);
/* one process, several devices: RCCL communicators among the first shard of every distinct device (no-op with one device) */
int rfx_exec_comm_init_all(rfx_exec_t *x);
/* Inter-process exchange (one process per device).  Default: the lead context's RCCL communicator (rfx_dist_init), identity without
 * one.  A host with its own channel (the tests: torch.distributed / gloo between two ranks that share a GPU) supplies these instead;
 * `user` is handed back.  Every function returns RFX_OK or an RFX_E* code.
 *   world_rank     how many processes, which one am I
 *   allgather_host bytes of host memory from every process, rank order
 *   allreduce      in place over n 8-byte cells of DEVICE memory on the lead context; type 0 i64 / 1 f64, op 0 SUM / 1 MIN / 2 MAX
 *   allgather_dev  bytes of device memory from every process, rank order, into d_out (world * bytes) */
typedef struct rfx_transport {
    void *user;
    int (*world_rank)(void *user, int *world, int *rank);
    int (*allgather_host)(void *user, const void *in, size_t bytes, void *out);
    int (*allreduce)(void *user, void *d_buf, int64_t n, int type, int op);
    int (*allgather_dev)(void *user, const void *d_in, size_t bytes, void *d_out);
} rfx_transport_t;
int rfx_exec_set_transport(rfx_exec_t *x, const rfx_transport_t *t); /* NULL: back to the default */
/* The inter-process side as the planner itself sees it (the host's transport, else the lead context's RCCL communicator unless that one is process-local):
 * how many processes share the table (1: no exchange), and `bytes` of host memory from each of them in rank order -- for a caller that must agree on a
 * small fact before it builds the query (rfx_select's reproducible sums: one scale for all ranks). */
int rfx_exec_ranks(rfx_exec_t *x, int *rank); /* (rank may be NULL) */
int rfx_exec_allgather_host(rfx_exec_t *x, const void *in, size_t bytes, void *out);

/* ---- the query ---- */
typedef struct rfx_qcol {
    const void *d[RFX_MAX_SHARDS]; /* the column's address on every shard; d[0] is what the descriptors name */
} rfx_qcol_t;

enum {
    RFX_Q_NO_SAMPLED_SCOPE = 1, /* always the exact key scope (index_scope_i64's full pass) */
    RFX_Q_REFUSE_NULL_KEY = 2,  /* a selected null group key ends the call with RFX_EXEC_NULL_KEY before anything is grouped (rfx_select hands
                                 * such queries to the host: the reference opens one group per null-key row, core/index.c:1808-1816) */
    RFX_Q_WANT_FIRST = 4,       /* rfx_groups_t.d_first is wanted (the groups' first rows: costs one more result column) */
    RFX_Q_NO_SMALL = 8,         /* never the one-launch rank + emit of small dense tables (tests) */
    RFX_Q_PROBE_FIRST = 16,     /* hashed path, one shard: also leave, per row, the first row of its group (rfx_groups_t.d_probe) */
    RFX_Q_SLICED = 32,          /* the caller reads the result through rfx_exec_groups_fetch_all only: the planner may leave it as SLICES -- after the
                                 * merge every device holds the whole tables, ranks them (the same order everywhere) and emits only ITS range of the
                                 * groups; fetch_all copies every slice into the host columns from the owning shard's own thread, over its own PCIe
                                 * link (rfx_groups_t.nslices / slice[]).  Without the flag -- or with one device, or with FIRST aggregates -- the
                                 * whole result is on shard 0 as before (nslices == 1) */
    RFX_Q_ROWS_DIRECT = 64,     /* rfx_exec_filter only: the compaction's masked-store write-out, whatever ships (measurements, tests) */
    RFX_Q_ROWS_RING = 128       /* ... its LDS-ring write-out */
};
#define RFX_EXEC_NULL_KEY 1 /* positive: not an error, see RFX_Q_REFUSE_NULL_KEY */

typedef struct rfx_query {
    const rfx_pred_t *preds; /* where: comparisons (flat / two-level / tree form of rfx_pred_t) ... */
    int32_t npred, logic;
    const int8_t *d_mask;    /* ... or a B8 selection mask evaluated by the caller (trees the fused form cannot carry): then npred == 0.  One shard only */
    const rfx_agg_t *aggs;   /* up to RFX_EXEC_MAX_AGGS */
    int32_t nagg;
    int32_t nkeys;           /* by: columns (0: scalar aggregates / where) */
    const void *const *d_keys; /* i64-like device columns */
    const int64_t *kxbar;    /* per key: > 0 = bucket width of (xbar key width); may be NULL */
    int64_t nrows;           /* rows of the whole table (all shards of this process) */
    const rfx_qcol_t *cols;  /* per-shard addresses; NULL with one shard */
    int32_t ncols;
    int32_t flags;           /* RFX_Q_* */
    const int64_t *key_scope; /* optional {min, max}: a scope of key 0 the caller remembers (a superset of any selection's): saves the scope pass when LDS-sized */
    int64_t row0;            /* rfx_exec_where only: the id of the table's row 0 (ids come out as row0 + row) */
    /* rfx_exec_filter_aggr only -- the selection as ROW IDS, shard by shard (a lazy MAPFILTER (values, ids) pair, core/filter.c:29-49): shard s
     * folds its columns gathered at the sel_count[s] GLOBAL row ids d_sel_ids[s] (on shard s's device; every one inside the shard's row range
     * -- the caller vouches for that; order kept: FIRST is the value at the first id of the first non-empty shard).  npred must be 0 */
    const int64_t *const *d_sel_ids;
    const int64_t *sel_count;
} rfx_query_t;

/* ---- scalar aggregates: select {aggs} from t where p ---- */
int rfx_exec_filter_aggr(rfx_exec_t *x, const rfx_query_t *q, rfx_value_t *values, int64_t *selected);

/* ---- where: ascending GLOBAL row ids, one run per shard (shard order = row order) ---- */
typedef struct rfx_ids {
    int32_t nshards;
    int64_t total;
    int64_t count[RFX_MAX_SHARDS];
    int64_t *d_ids[RFX_MAX_SHARDS]; /* on the shard's device; NULL when count == 0 */
} rfx_ids_t;
int rfx_exec_where(rfx_exec_t *x, const rfx_query_t *q, rfx_ids_t *out);
void rfx_exec_ids_free(rfx_exec_t *x, rfx_ids_t *ids);

/* ---- group-by: select {aggs} from t where p by keys ---- */
enum { RFX_PATH_NONE = 0, RFX_PATH_DENSE = 1, RFX_PATH_DENSE_SMALL = 2, RFX_PATH_HASH = 3, RFX_PATH_ROWHASH = 4 };
typedef struct rfx_groups {
    int64_t groups;
    int32_t path;                     /* RFX_PATH_* */
    int32_t nkeys, nagg;
    int64_t *d_keys;                  /* one key: the groups' keys.  Several: the composite key / the row hash (see d_keycols) */
    int64_t *d_keycols[RFX_MAX_KEYS]; /* several keys: the result's key columns */
    int64_t *d_first;                 /* global first row of every group (RFX_Q_WANT_FIRST, and always on the hashed paths) */
    void *d_results[RFX_EXEC_MAX_AGGS];
    int32_t result_type[RFX_EXEC_MAX_AGGS]; /* RFX_I64 | RFX_F64 */
    int64_t *d_probe;                 /* RFX_Q_PROBE_FIRST */
    int64_t capacity;                 /* hashed paths: the table size the query ended with */
    /* small dense tables: everything above points into ONE device block that is mirrored on the host -- read results through
     * rfx_exec_groups_fetch and they cost no further round trip */
    const char *d_block, *h_block;
    size_t block_bytes;
    /* device blocks to release, and the shard whose context each came from.  Worst case by construction: a result of RFX_MAX_SHARDS slices registers per
     * slice its first rows, RFX_MAX_KEYS key columns (twice on the row-hash route: the proof passes' blocks) and one result block per pass
     * (<= RFX_EXEC_MAX_AGGS passes) */
    void *own[RFX_GROUPS_OWN];
    int8_t own_shard[RFX_GROUPS_OWN];
    int32_t nown;
    /* RFX_Q_SLICED: column c of the result = the concatenation of slice[0..nslices)'s pieces; slice i holds the groups [g0, g0 + n) on shard
     * `shard`.  The column pointers above are slice 0's (with one slice: the whole columns, as without the flag) */
    int32_t nslices;
    struct rfx_gslice {
        int32_t shard;
        int64_t g0, n;
        int64_t *d_keys, *d_first;
        int64_t *d_keycols[RFX_MAX_KEYS];
        void *d_results[RFX_EXEC_MAX_AGGS];
    } slice[RFX_MAX_SHARDS];
} rfx_groups_t;
int rfx_exec_group_by(rfx_exec_t *x, const rfx_query_t *q, rfx_groups_t *out);
int rfx_exec_groups_fetch(rfx_exec_t *x, const rfx_groups_t *g, void *dst, const void *d_src, size_t bytes); /* device result -> host (syncs) */
/* n result columns to host memory in ONE call: dst[i] receives the whole column src[i] -- a column pointer out of `g` (d_keys, d_first,
 * d_keycols[k], d_results[a]), groups * 8 bytes.  Every slice is copied by the shard that owns it, on that shard's host thread and stream;
 * one wait per shard at the end instead of one per column.  Columns above 64 MB go through pinned staging with several host threads
 * writing the destination (first-touch page faults of a freshly allocated vector are taken in parallel). */
int rfx_exec_groups_fetch_all(rfx_exec_t *x, const rfx_groups_t *g, int n, const void *const *d_srcs, void *const *dsts);
/* The groups [g0, g0 + n) of a result as a result of its own: a VIEW on the same device blocks (it owns nothing: release the original, not the view), read
 * through rfx_exec_groups_fetch / _fetch_all like any other.  What one rank of several returns when every rank is to keep only ITS range of the answer
 * (rfx_ops_set_rank_slices).  Results of one slice only (RFX_EINVAL otherwise). */
int rfx_exec_groups_window(const rfx_groups_t *g, int64_t g0, int64_t n, rfx_groups_t *out);
void rfx_exec_groups_free(rfx_exec_t *x, rfx_groups_t *g);

/* ---- med (rfx_median.hip): one shard only (RFX_ELIMIT otherwise) ----
 * rfx_exec_median: the scalar `med` of an i64 column over the query's selection (its preds, or its d_mask) -- ray_med's rule (core/math.c:2529-2626).
 * rfx_exec_group_median: g->groups f64 cells into d_out (on shard 0) -- aggr_med's rule (core/aggr.c:2136-2247) over an i64 / timestamp (RFX_I64) or
 * f64 column; `g` is rfx_exec_group_by's result for the same query (one key column, no xbar, one slice), every selected row counted in its key's group.
 * Scratch beyond the kernels' (8 B per selected row + 24 B per group): dense keys a slot table of (key range) * 8 B, taken only when the range is at most
 * rows + groups; sparse keys a group index column of 8 B per row.  RFX_ENOMEM when the device cannot hold it (nothing is left allocated). */
int rfx_exec_median(rfx_exec_t *x, const rfx_query_t *q, const void *d_col, int32_t col_type, rfx_value_t *out);
int rfx_exec_group_median(rfx_exec_t *x, const rfx_query_t *q, const rfx_groups_t *g, const void *d_col, int32_t col_type, void *d_out);

/* ---- last, dev (rfx_lastdev.hip) ----
 * RFX_AGG_LAST in rfx_exec_filter_aggr: the cell at the last selected row, null or not (shard order = row order; one process).  In rfx_exec_group_by:
 * per group the cell at the highest selected row whose cell is non-null, null without one -- the reference's answer with one chunk (aggr_last,
 * core/aggr.c:851-930) -- planned as an i64 MAX over derived rows (8 B of scratch per row and distinct LAST column), under every
 * by: shape, over the shards of ONE device, in one process (RFX_ELIMIT otherwise); the result is whole on shard 0 (RFX_Q_SLICED is ignored, as with FIRST).
 * rfx_exec_dev: ray_dev's rule (core/math.c:2628-2699) over the query's selection (its preds, or its d_mask) of an i64 / timestamp (RFX_I64) or f64
 * column: l = non-null count, 0 -> null, 1 -> 0.0; favg = (f64)(wrapping i64 sum) / l resp. f64 sum / l; sqrt(sum (x - favg)^2 / l): two passes.
 * rfx_exec_group_dev: g->groups f64 cells into d_out (on shard 0) by aggr_dev's rule (core/aggr.c:2250-2350,2864-2929): per group sum (f64)x, sum
 * (f64)x * (f64)x and the non-null count n; 0 -> null, 1 -> 0.0, else mean = s/n, var = sq/n - mean * mean, var < 0 ? 0 : sqrt(var) (not Welford's: it
 * cancels where the reference's does); `g` is rfx_exec_group_by's result for the same query (any by: shape): the three sums ride through the same
 * group-by as hidden aggregates.  Scratch 16 B per row.  Both dev calls: one shard only (RFX_ELIMIT otherwise), as med. */
int rfx_exec_dev(rfx_exec_t *x, const rfx_query_t *q, const void *d_col, int32_t col_type, rfx_value_t *out);
int rfx_exec_group_dev(rfx_exec_t *x, const rfx_query_t *q, const rfx_groups_t *g, const void *d_col, int32_t col_type, void *d_out);

/* ---- sort (rfx_sort.hip, rfx_merge.hip) ----
 * rfx_exec_sort: d_perm (n i64 cells on shard 0) = the stable lexicographic order of the rows by d_cols[0] (most significant) .. d_cols[ncols-1],
 * all ascending or all descending -- one stable radix sort per column from the last to the first, each reading its keys through the running
 * permutation (core/order.c:266-321,354-409); ties keep ascending row order in both directions.  types[k]: RFX_I64 (also TIMESTAMP), RFX_F64, or a
 * key of at most 32 bits as rfx_hip_sort_index takes it -- RFX_I32 (raw 4-byte cells; DATE / TIME too), RFX_I32_WIDE (their widened 8-byte image),
 * RFX_I16, RFX_U8, RFX_B8; the columns of one call may mix them: every level picks its record form by its column's type.
 * rfx_exec_sort_values: d_out = the column's own cells in that order (asc / desc) IN THE COLUMN'S OWN WIDTH (4-byte cells from RFX_I32_WIDE too),
 * d_perm (may be NULL) the permutation as well.
 * Rows <= 2^32 - 1; scratch 24 B per row for an 8-byte key, 16 B for a narrower one (+ one more permutation of 8 B per row when ncols > 1), freed
 * before return; RFX_ENOMEM when it does not fit.
 * These two take ONE whole-column address per key, which a sharded context does not have: they refuse it (RFX_ELIMIT "sort over a sharded table").
 * rfx_exec_sort_shards: the same orders over row-range shards.  cols[k].d[s] is key column k's piece on shard s (rows rfx_exec_split(n, S, s)); every
 *   shard sorts its piece on its own thread with the kernels above (one key: rfx_hip_sort_values; several: the least-significant-first chain, then
 *   the key columns gathered into the run's order), runs on another device than shard 0's are copied over (rfx_hip_d2d), runs on shard 0's device are
 *   read where they lie, and ONE stable multiway merge (rfx_hip_merge_runs) by (key tuple, run, place in run) = (key tuple, global row) writes
 *   d_perm (n cells) and / or -- ncols == 1 only -- d_values on shard 0's device: the unsharded answer bit for bit.  Either output may be NULL, not
 *   both.  types[k]: RFX_I64 / RFX_F64 ONLY -- an I32-family column is given as its widened pieces under RFX_I64 (order and nulls survive the
 *   widening; the caller narrows merged cells), 1- and 2-byte keys are not taken.  One shard: the two calls above as they are.  ncols <=
 *   RFX_MAX_KEYS over shards, every piece <= 2^32 - 1 rows.  Scratch per shard 16 B per
 *   row of its piece (one key) or 8 * (ncols + 2) B (several) beside the sort's, + a copy of every cross-device run on shard 0, all freed before return;
 *   RFX_ENOMEM / RFX_ELIMIT as the sort's; RFX_ELIMIT "sort over several ranks" under a transport or an inter-process communicator.
 * RFX_XSTAT_SORTS / RFX_XSTAT_SORT_PASSES count what ran, RFX_XSTAT_SORT_MERGES the merges, RFX_XSTAT_NS_SORT_LOCAL / _NS_SORT_MERGE their wall time. */
int rfx_exec_sort(rfx_exec_t *x, const void *const *d_cols, const int32_t *types, int ncols, int descending, int64_t n, int64_t *d_perm);
int rfx_exec_sort_values(rfx_exec_t *x, const void *d_col, int32_t type, int descending, int64_t n, void *d_out, int64_t *d_perm);
int rfx_exec_sort_shards(rfx_exec_t *x, const rfx_qcol_t *cols, const int32_t *types, int ncols, int descending, int64_t n, int64_t *d_perm, void *d_values);

/* ---- join index (index_left_join_obj, core/index.c:2886-2928): d_ids[i] = first right row whose key tuple equals left row i's, else null.
 * RFX_ESTATE with *collision = 1: two key tuples share one 64-bit row hash (nothing may be used).  One shard. */
int rfx_exec_join_index(rfx_exec_t *x, const void *const *d_left_keys, const void *const *d_right_keys, int nkeys, int64_t nleft, int64_t nright,
                        int64_t *d_ids, int *collision);
/* ... over SHARDS: a broadcast join.  The BUILD side's key columns (drk) WHOLE on shard `shard`'s device, dlk this shard's nl rows of the left keys;
 * d_ids (on that device) receives per left row the first right row with an equal tuple -- a GLOBAL right row id -- or null.  Every shard builds the same
 * table and probes its own rows: no exchange.  To be called on the shard's thread (rfx_exec_run). */
int rfx_exec_join_index_shard(rfx_exec_t *x, int shard, const void *const *dlk, const void *const *drk, int nk, int64_t nl, int64_t nr, int64_t *d_ids, int *collision);

/* ---- asof join index, bin, binr (rfx_asof.hip): one shard only (RFX_ELIMIT "asof join over a sharded table" / "bin over a sharded table") ----
 * rfx_exec_asof_index (index_asof_join_obj, core/index.c:3194-3267): the right rows are grouped by their key tuple (nkeys 8-byte integer columns,
 * cells compared as raw integers: null equals null), every group's rows kept in ascending ROW order; d_ids[i] = the row the reference's
 * closed-interval binary search over left row i's group lands on -- last probe with d_right_time[row] <= d_left_time[i] -- or null (no group,
 * or no probe qualified).  Times are signed 64-bit integers (I64 / TIMESTAMP, or I32 / DATE / TIME widened), a null the smallest; the right
 * times need not be sorted, and then the probe sequence decides (see rfx_hip_seg_search).
 * BUILD: the equi-join index of the right keys against themselves (every right row's group = its group's first row), one stable sort of those
 * ids, the run boundaries, the right times gathered into group order.  PROBE: the equi-join index of the left keys against the right keys, then
 * one search per left row.  Scratch 48 B per right row + the sort's 24 B + the join index's, freed before return; RFX_ENOMEM when it does not fit,
 * RFX_ELIMIT above 2^32 - 1 right rows.  RFX_ESTATE with *collision = 1 as for rfx_exec_join_index.
 * rfx_exec_bin (ray_bin / ray_binr, core/items.c:1399-1644): d_out[j] = the search of d_y[j] over the whole of d_x by position -- right = 0: last
 * probe with x[mid] <= y, none = -1; right = 1: first probe with x[mid] >= y, none = nx.
 * RFX_XSTAT_ASOF_JOINS / _BINS / _SEARCHES count what ran, RFX_XSTAT_NS_ASOF_BUILD / _PROBE the two halves' wall time. */
int rfx_exec_asof_index(rfx_exec_t *x, const void *const *d_left_keys, const void *const *d_right_keys, int nkeys, const int64_t *d_left_time,
                        const int64_t *d_right_time, int64_t nleft, int64_t nright, int64_t *d_ids, int *collision);
int rfx_exec_bin(rfx_exec_t *x, const int64_t *d_x, int64_t nx, const int64_t *d_y, int64_t ny, int right, int64_t *d_out);

/* ---- window join (rfx_window.hip): one shard only (RFX_ELIMIT "window join over a sharded table") ----
 * rfx_exec_window_ranges (index_window_join_obj, core/index.c:3269-3347, and the searches of the INDEX_TYPE_WINDOW arms, core/aggr.c:133-160):
 * d_perm (nright cells) = the right rows in the stable order of (key tuple, d_right_time) -- the tuples' groups contiguous, in the order of their
 * first rows (the reference's xasc orders them by key; nothing downstream depends on the order of the groups); per left row i (d_li[i], d_ri[i])
 * = the first and last POSITION in that order of its window [d_left_lo[i], d_left_hi[i]] over its tuple's group, or (-1, -2) for the null row
 * (no group, or the reference's null tests).  closed = 0: window-join (the row prevailing at the window's start is inside); 1: window-join1.
 * Keys are 8-byte integer columns compared as raw integers (null equals null); times and bounds are signed 64-bit cells holding 32-bit values
 * (I32 / DATE / TIME widened, a null the smallest).  stats (host, 2 cells, may be NULL): windows longer than 16 rows, the longest window.
 * BUILD: the equi-join index of the right keys against themselves, one two-column stable sort, the run boundaries, the times gathered.
 * PROBE: the equi-join index of the left keys against the right keys, two searches per left row.  Scratch 56 B per right row + 8 B per left
 * row + the sort's and the join index's, freed before return.  RFX_ENOMEM / RFX_ELIMIT / RFX_ESTATE with *collision = 1 as rfx_exec_asof_index.
 * rfx_exec_window_fold: every aggregate of one value column (type RFX_I64 / RFX_F64, nright cells) over those windows in ONE launch.  d_perm:
 * the permutation above -- the column is gathered into a scratch copy (8 B per right row) first -- or NULL when d_vals is in that order
 * already.  d_outs: RFX_WAGG_N device pointers (include/rfx_hip.h), NULL = not wanted, nleft cells each.  long_windows: stats[0]. */
int rfx_exec_window_ranges(rfx_exec_t *x, const void *const *d_left_keys, const void *const *d_right_keys, int nkeys, const int64_t *d_left_lo,
                           const int64_t *d_left_hi, const int64_t *d_right_time, int64_t nleft, int64_t nright, int closed, int64_t *d_perm,
                           int64_t *d_li, int64_t *d_ri, int64_t *stats, int *collision);
int rfx_exec_window_fold(rfx_exec_t *x, const void *d_vals, int32_t type, const int64_t *d_perm, const int64_t *d_li, const int64_t *d_ri, int64_t nleft,
                         int64_t nright, int64_t long_windows, void *const *d_outs);

/* ---- set verbs (rfx_set.hip): one shard only (RFX_ELIMIT "distinct over a sharded column", ...) ----
 * Keys are 8-byte integer cells (I64 / SYMBOL / TIMESTAMP) compared as raw integers, null equal to null.  Every call takes the REFERENCE's route,
 * decided from the key scopes as it decides (MAX_RANGE = 2^20, core/index.c:36), and reports it in *route (may be NULL).
 * rfx_exec_distinct (index_distinct_i64, core/index.c:551-607): the distinct cells of d_a[0 .. na) followed by d_b[0 .. nb) (nb = 0: `distinct`;
 *   else `union`, the concatenation is never made) into d_out (na + nb cells of room), *nout of them.  range = max - min + 1 over EVERY cell:
 *   DENSE when range <= len or range <= 2^20 -- the values ascending; else HASH -- the keys in the slot order of the reference's linear-probing
 *   table of rfx_set_table_cells(len) cells filled in row order (nulls skipped), rebuilt by a parallel priority insert.
 * rfx_exec_member: want_first = 0, `in x y` (index_in_i64_i64, :1291-1361): d_out = nx B8 bytes (8-byte aligned), cell i = x[i] occurs in y;
 *   want_first = 1, `find x y` (index_find_i64, :1507-1574): d_out = ny I64 cells, cell j = the first row of x holding y[j], or null -- and NOTHING
 *   is written when nx = 0 (the reference answers I64(0) then).  DISJOINT: the two scopes do not meet (nobody is found, no table); DENSE: the
 *   intersection spans at most 2^20 -- a bitmap / a first-row table over it; else HASH.
 * rfx_exec_set_filter: the cells of x that occur (keep_members = 1: `sect`) / do not occur (0: `except`) in y, in x's order, into d_out (nx cells
 *   of room, not x itself), *nout of them: filter(x, in(x, y)) as ONE probe + ordered compaction of the values.  y_is_atom: y is the one cell `atom`.
 * RFX_ESTATE with *route = RFX_SET_ROUTE_UNDEFINED: the reference's own indexing would leave its table for these cells -- a hash route over a
 *   negative key (its probes start at (i64)key % size), for `find` over a null too, or a range that does not fit 64 bits: nothing is answered, the
 *   reason is in rfx_exec_last_error().  Scratch (hash routes: 16-24 B per set cell x 2..4) comes from the context's pool and is freed before return.
 * RFX_XSTAT_SET_DISTINCTS / _MEMBERS / _FILTERS count what ran, RFX_XSTAT_NS_SET_BUILD / _PROBE the two halves' wall time. */
enum { RFX_SET_ROUTE_UNDEFINED = -1, RFX_SET_ROUTE_NONE = 0, RFX_SET_ROUTE_DENSE = 1, RFX_SET_ROUTE_HASH = 2, RFX_SET_ROUTE_DISJOINT = 3, RFX_SET_ROUTE_ATOM = 4 };
int rfx_exec_distinct(rfx_exec_t *x, const int64_t *d_a, int64_t na, const int64_t *d_b, int64_t nb, int64_t *d_out, int64_t *nout, int *route);
int rfx_exec_member(rfx_exec_t *x, const int64_t *d_x, int64_t nx, const int64_t *d_y, int64_t ny, int want_first, void *d_out, int *route);
int rfx_exec_set_filter(rfx_exec_t *x, const int64_t *d_x, int64_t nx, const int64_t *d_y, int64_t ny, int y_is_atom, int64_t atom, int keep_members,
                        int64_t *d_out, int64_t *nout, int *route);
/* cells of the reference's table for `len` rows: the first prime >= ceil(len / 0.75) (ht_oa_create, core/hash.c:35-56; host only) */
int64_t rfx_set_table_cells(int64_t len);

/* ---- bucket verbs (rfx_bucket.hip) ----
 * rfx_exec_xrank (ray_xrank, core/order.c:598-649): d_out[i] = the bucket in [0, nb) of row i's rank among the n cells of d_col (RFX_I64, also TIMESTAMP, or
 *   RFX_F64) -- rfx_exec_sort of the one column, ascending, then the fused scatter (rank * nb) / n; scratch 8 B per row beside the sort's, freed before
 *   return; RFX_ENOMEM when it does not fit (the operator layer hands the verb to the host).  attrs: RFX_XRANK_ASC / RFX_XRANK_DESC say the column
 *   carries that attribute: the index formula alone runs and d_col is not read.  One shard only (RFX_ELIMIT "xrank over a sharded table").  nb > 0 and
 *   (n - 1) * nb < 2^63; n = 0 answers nothing without dividing.
 * rfx_exec_xbar / _round / _neg / _within: rfx_hip_xbar / rfx_hip_round_f64 / rfx_hip_neg / rfx_hip_within_i64 over every shard's rows.  The operands are
 *   given per shard: d_xs[s] is shard s's piece (rows rfx_exec_split(n, S, s)); a NULL array is an atom (xbar).  shard < 0: all shards, n the whole
 *   length, returns with the shards' streams idle when there is more than one; shard >= 0: that shard's piece alone, n ITS rows, enqueued on its
 *   context (the operator layer's pieces).  RFX_XSTAT_XRANKS / _XRANK_SORTED / _BUCKET_MAPS count what ran. */
enum { RFX_XRANK_ASC = 2, RFX_XRANK_DESC = 4 }; /* (the reference's ATTR_ASC / ATTR_DESC bits) */
int rfx_exec_xrank(rfx_exec_t *x, const void *d_col, int32_t type, int attrs, int64_t n, int64_t nb, int64_t *d_out);
/* which arm of ray_xbar_partial (core/math.c:1635-1782) a pair of operand types takes: x_type / y_type are the reference's type codes without the atom's
 * sign (I32 4, I64 5, DATE 7, TIME 8, TIMESTAMP 9, F64 10); fills desc's x_type, y_type, mid, y_time and out_bytes, *out_type = the result's type code
 * (infer_xbar_type).  RFX_EINVAL: the reference has no such arm (its type error). */
int rfx_exec_xbar_plan(int x_type, int y_type, rfx_xbar_desc_t *desc, int *out_type);
int rfx_exec_xbar(rfx_exec_t *x, const rfx_xbar_desc_t *desc, const void *const *d_xs, const void *const *d_ys, int64_t n, void *const *d_outs, int shard);
int rfx_exec_round(rfx_exec_t *x, int op, const void *const *d_ins, int64_t n, void *const *d_outs, int shard);
int rfx_exec_neg(rfx_exec_t *x, int32_t type, const void *const *d_ins, int64_t n, void *const *d_outs, int shard);
int rfx_exec_within(rfx_exec_t *x, const void *const *d_cols, int64_t lo, int64_t hi, int64_t n, void *const *d_masks, int shard);

/* ---- row verbs (rfx_rows.hip): filter, take, reverse ----
 * Columns are given with their cell kind (RFX_ROWS_8 / RFX_ROWS_4W / RFX_ROWS_1, include/rfx_hip.h): 8-byte cells; an I32-family column's widened 8-byte
 * copy, answered in 4-byte cells; B8 bytes.
 * rfx_exec_filter (ray_filter, core/items.c:338-396): the rows of `ncols` columns that q selects -- q is what rfx_exec_where takes: a byte mask (d_mask)
 *   or a predicate tree, so a fused where: feeds the compaction with no mask and no ids in between -- in row order.  pieces[k].d[s] is column k's address
 *   on shard s (its rows rfx_exec_split(q->nrows, S, s)); every shard selects and compacts its own rows (one bitmap and one scan per shard, however many
 *   columns: more than RFX_MAX_KEYS take several launches over them), and the result is the shards' pieces in shard order: count[s] cells of column k at
 *   rfx_exec_rows_piece(out, s, k) on shard s's device (NULL when count[s] == 0), exact-size, one block per shard, 256-byte aligned pieces.  Returns with
 *   the shards' streams idle when there is more than one.  RFX_Q_ROWS_DIRECT / RFX_Q_ROWS_RING in q->flags pick the write-out form.
 * rfx_exec_take (ray_take, core/items.c:398-734): d_outs[k][i] = cell (j0 + i) mod l of d_cols[k] for i < m -- the caller has turned the count (its
 *   sign, the cyclic start (l - m % l) * (count < 0)) or the [start amount] range (clamped) into j0 and m: 0 <= j0 < l unless m == 0.  rfx_exec_take_atom:
 *   m cells of an atom (`bits`: the cell in the low bytes).  rfx_exec_reverse (ray_reverse, core/compose.c:144-202): d_out[i] = cell l - 1 - i.
 *   One shard only: RFX_ELIMIT "take over a sharded table" / "reverse over a sharded table", as the sort.  Results 16-byte aligned.
 * RFX_XSTAT_ROWS_FILTERS / _TAKES / _REVERSES count the calls, RFX_XSTAT_ROWS_IN / _OUT the rows read and answered. */
typedef struct rfx_rows {
    int32_t nshards, ncols;
    int64_t total;                   /* selected rows over all shards */
    int64_t count[RFX_MAX_SHARDS];   /* ... per shard */
    void *d_block[RFX_MAX_SHARDS];   /* the shard's block on its device; NULL when count == 0 */
    size_t *col_off;                 /* [shard * ncols + col]: where the column's piece starts in the shard's block (bytes) */
} rfx_rows_t;
int rfx_exec_filter(rfx_exec_t *x, const rfx_query_t *q, const rfx_qcol_t *pieces, const int32_t *kinds, int ncols, rfx_rows_t *out);
void *rfx_exec_rows_piece(const rfx_rows_t *r, int shard, int col);
void rfx_exec_rows_free(rfx_exec_t *x, rfx_rows_t *r);
int rfx_exec_take(rfx_exec_t *x, const void *const *d_cols, const int32_t *kinds, int ncols, int64_t l, int64_t j0, int64_t m, void *const *d_outs);
int rfx_exec_take_atom(rfx_exec_t *x, int32_t kind, uint64_t bits, int64_t m, void *d_out);
int rfx_exec_reverse(rfx_exec_t *x, const void *d_col, int32_t kind, int64_t l, void *d_out);

/* ---- cast (rfx_cast.hip) ----
 * rfx_exec_cast: rfx_hip_cast over every shard's rows, like the element-wise bucket verbs: d_ins[s] / d_outs[s] are shard s's pieces (rows
 *   rfx_exec_split(n, S, s)) of the source and of the result; src_type / dst_type as rfx_hip_cast takes them (RFX_CAST_*, | RFX_CAST_WIDENED).  shard < 0:
 *   all shards, n the whole length, returns with the shards' streams idle when there is more than one; shard >= 0: that shard's piece alone, n ITS rows,
 *   enqueued on its context.  RFX_EINVAL: the reference has no such arm (rfx_hip_cast_arm); RFX_ELIMIT: several ranks.  RFX_XSTAT_CASTS counts. */
int rfx_exec_cast(rfx_exec_t *x, int32_t src_type, int32_t dst_type, const void *const *d_ins, int64_t n, void *const *d_outs, int shard);

/* ---- concat, raze (rfx_concat.hip) ----
 * rfx_exec_concat: the spans' cells end to end into d_out (rfx_hip_concat: one launch for any number of spans); kind = the bytes of a cell, 1, 2, 4 or 8.
 * rfx_exec_concat_cols: the table form -- every column its own spans, width and output, RFX_MAX_COLS columns per launch, more in further launches.
 * Both read across whole columns and run on one shard, one rank: several answer RFX_ELIMIT, "concat over a sharded column".  Enqueued on shard 0's
 * context.  RFX_XSTAT_CONCATS counts the calls (a table once), RFX_XSTAT_CONCAT_SPANS the spans given, RFX_XSTAT_CONCAT_CELLS the cells answered. */
int rfx_exec_concat(rfx_exec_t *x, const rfx_span_t *spans, int64_t nspans, int32_t kind, void *d_out);
int rfx_exec_concat_cols(rfx_exec_t *x, const rfx_concat_col_t *cols, int ncols);

/* ---- upsert, insert (rfx_upsert.hip; ray_upsert / ray_insert, core/update.c:556-750) ----
 * A batch of m rows against a table of n rows whose first nkeys columns are the key.  Three steps, each enqueued on shard 0's context:
 * rfx_exec_upsert_index: d_idx[j] = the first table row whose key tuple equals batch row j's, or the null (index_upsert_obj, core/index.c:3001-3065).  One
 *   key: the set verbs' `find` (rfx_exec_member, its routes and guards: RFX_ESTATE with *undefined = 1 where the reference's own indexing would leave its
 *   table).  2 .. RFX_MAX_KEYS keys: rfx_exec_join_index (RFX_ESTATE with *undefined = 2: two tuples share one row hash).  n == 0: all nulls, no lookup.
 *   Key cells are 8-byte integers (I64 / SYMBOL / TIMESTAMP).
 * rfx_exec_upsert_plan: rfx_hip_upsert_plan -- d_dest[j] and *appended = a.
 * rfx_exec_upsert_cols: every column's result of n + a cells: the table's n cells by the multi-span copy (rfx_exec_concat_cols), then -- on the same
 *   stream -- the column's null over the appended cells of an ABSENT column, and the batch cells placed by d_dest, RFX_MAX_COLS columns per launch: a KEY
 *   column takes appended rows only, a VALUE column matched rows too.  d_out 16-byte aligned, d_batch 16-byte aligned.
 * rfx_exec_insert_cols: the same with every batch row appended in order: no index, no plan (roles VALUE and ABSENT only).
 * Scratch is freed before return (RFX_ENOMEM when it does not fit).  One shard, one rank: several answer RFX_ELIMIT, "upsert over a sharded table".
 * RFX_XSTAT_UPSERTS / _UPSERT_MATCHED / _UPSERT_APPENDED / _INSERTS count; RFX_XSTAT_NS_UPSERT_INDEX / _PLAN / _PLACE: wall time to the stream idle. */
enum { RFX_UPSERT_KEY = 0, RFX_UPSERT_VALUE = 1, RFX_UPSERT_ABSENT = 2 };
typedef struct {
    const void *d_table; /* n cells (NULL when n == 0) */
    const void *d_batch; /* m cells; NULL: RFX_UPSERT_ABSENT */
    void *d_out;         /* n + a cells */
    int32_t width;       /* bytes of a cell: 1, 2, 4 or 8 */
    int32_t role;        /* RFX_UPSERT_* */
    uint64_t null_bits;  /* the column's null in the low bytes (ABSENT) */
} rfx_upsert_xcol_t;
int rfx_exec_upsert_index(rfx_exec_t *x, const void *const *d_table_keys, const void *const *d_batch_keys, int nkeys, int64_t n, int64_t m, int64_t *d_idx,
                          int *undefined);
int rfx_exec_upsert_plan(rfx_exec_t *x, const int64_t *d_idx, int64_t m, int64_t n, int64_t *d_dest, int64_t *appended);
int rfx_exec_upsert_cols(rfx_exec_t *x, const rfx_upsert_xcol_t *cols, int ncols, const int64_t *d_dest, int64_t m, int64_t n, int64_t appended);
int rfx_exec_insert_cols(rfx_exec_t *x, const rfx_upsert_xcol_t *cols, int ncols, int64_t m, int64_t n);

/* ---- row, collect (rfx_collect.hip; aggr_row / aggr_collect, core/aggr.c:3021-3136): every group's rows and cells, in group order ----
 * rfx_exec_group_partition: m elements with the dense group ids d_gid[i] in [0, groups) (element-aligned: element i is table row i, or row d_rows[i] of a
 *   filter) -> out->d_perm (m cells: the elements ordered by (group, element), stable) and out->d_offsets (groups + 1 cells: group g's elements are
 *   d_perm[d_offsets[g] .. d_offsets[g + 1])), both on shard 0, released by rfx_exec_group_partition_free.  The ids are checked on the device before
 *   anything is placed: one outside [0, groups) answers RFX_EINVAL ("a group id outside [0, groups)") and is never used as an index.  Returns with the
 *   stream idle.  m, groups < 2^31 (RFX_ELIMIT); scratch 20 B per element, freed before return; RFX_ENOMEM when it does not fit.
 * rfx_exec_group_collect: d_outs[k][j] = d_cols[k][src(j)] for j < part->m, src(j) = d_rows ? d_rows[d_perm[j]] : d_perm[j]; widths[k] = the bytes of
 *   column k's cells (1, 2, 4 or 8), the output in the same width, cell-aligned; want_rows: d_rows_out[j] = src(j) as i64 as well (`row`).  The columns hold
 *   col_len cells; d_rows (the filter's row ids, from outside) is checked against it first: one outside answers RFX_EINVAL and nothing is gathered.
 *   RFX_MAX_COLS outputs to a launch, more in further launches over the same permutation.  Enqueued on shard 0's context (no sync without d_rows).
 * One shard, one rank: several answer RFX_ELIMIT, "collect over a sharded table".
 * RFX_XSTAT_COLLECT_PARTITIONS / _COLLECT_PASSES count the partitions and the radix passes they ran, RFX_XSTAT_COLLECTS / _COLLECT_LAUNCHES the collect
 * calls and their gather launches. */
typedef struct rfx_partition {
    int64_t m, groups;
    int64_t *d_offsets; /* groups + 1 cells */
    int64_t *d_perm;    /* m cells (NULL when m == 0) */
} rfx_partition_t;
int rfx_exec_group_partition(rfx_exec_t *x, const int64_t *d_gid, int64_t m, int64_t groups, rfx_partition_t *out);
void rfx_exec_group_partition_free(rfx_exec_t *x, rfx_partition_t *p);
int rfx_exec_group_collect(rfx_exec_t *x, const rfx_partition_t *part, const int64_t *d_rows, int64_t col_len, const void *const *d_cols, const int32_t *widths,
                           int ncols, void *const *d_outs, int want_rows, int64_t *d_rows_out);

/* ---- counters since rfx_exec_create ---- */
enum {
    RFX_XSTAT_SCOPE_SAMPLED = 0, /* group-bys that ran under a sampled key scope */
    RFX_XSTAT_SCOPE_RETRIED = 1, /* ... whose pass reported a key outside it: run again under the exact scope */
    RFX_XSTAT_SCOPE_REMEMBERED = 2, /* group-bys that took the caller's remembered scope */
    RFX_XSTAT_HASH_GROWN = 3,    /* hashed tables that reported full and were grown */
    RFX_XSTAT_MERGES_KERNEL = 4, /* table sets merged by the same-device kernel */
    RFX_XSTAT_MERGES_RCCL = 5,   /* fused RCCL exchanges issued (process-local communicators) */
    RFX_XSTAT_MERGES_TRANSPORT = 6, /* inter-process exchanges issued */
    RFX_XSTAT_QUERIES = 7,
    RFX_XSTAT_SLICED = 8,        /* group-by results left as more than one slice */
    /* per-phase wall time of the calling thread, nanoseconds, accumulated over the group-bys since rfx_exec_timing(x, 1) (which zeroes
     * them): scope (samples, exact scopes, the scope exchange), pass (tables + scatter / aggregate kernels on every shard, to the last
     * shard's stream idle), merge (kernel merges, the fused exchange, copy-back), rank (slot ranking incl. its one round trip), emit
     * (+ key columns, FIRST values), fetch (rfx_exec_groups_fetch / _fetch_all: device -> host result).  With timing on every phase
     * ends with its shards' streams idle (a one-shard query otherwise runs on in stream order), so the sum is a little above the
     * untimed query */
    RFX_XSTAT_NS_SCOPE = 9,
    RFX_XSTAT_NS_PASS = 10,
    RFX_XSTAT_NS_MERGE = 11,
    RFX_XSTAT_NS_RANK = 12,
    RFX_XSTAT_NS_EMIT = 13,
    RFX_XSTAT_NS_FETCH = 14,
    RFX_XSTAT_NS_TOTAL = 15,     /* rfx_exec_group_by entry to exit, + the fetches */
    RFX_XSTAT_SORTS = 16,        /* sorts (one per key column of a multi-column sort) answered by the device path */
    RFX_XSTAT_SORT_PASSES = 17,  /* ... radix passes they executed (a digit every key agrees on costs none) */
    RFX_XSTAT_ASOF_JOINS = 18,   /* asof join indexes answered by the device path */
    RFX_XSTAT_BINS = 19,         /* bin / binr calls answered by the device path */
    RFX_XSTAT_SEARCHES = 20,     /* ... binary searches those two ran (left rows of an asof join with a right side, cells of a bin / binr) */
    RFX_XSTAT_NS_ASOF_BUILD = 21, /* wall time of the asof joins' build halves (right side only), nanoseconds, to the stream idle */
    RFX_XSTAT_NS_ASOF_PROBE = 22, /* ... and of their probe halves */
    RFX_XSTAT_SET_DISTINCTS = 23, /* distinct / union calls answered by the device path */
    RFX_XSTAT_SET_MEMBERS = 24,   /* in / find calls */
    RFX_XSTAT_SET_FILTERS = 25,   /* sect / except calls */
    RFX_XSTAT_NS_SET_BUILD = 26,  /* wall time of the set verbs' scope + build halves, nanoseconds, to the stream idle */
    RFX_XSTAT_NS_SET_PROBE = 27,  /* ... and of their probe / emit halves */
    RFX_XSTAT_XRANKS = 28,        /* xrank calls answered by the device path */
    RFX_XSTAT_XRANK_SORTED = 29,  /* ... of which an ASC / DESC attribute answered without a sort */
    RFX_XSTAT_BUCKET_MAPS = 30,   /* element-wise bucket maps run: xbar, floor / ceil / round, neg, within (one per call or operator piece) */
    RFX_XSTAT_ROWS_FILTERS = 31,  /* filter calls answered by the device path */
    RFX_XSTAT_ROWS_TAKES = 32,    /* take calls (a table counts once) */
    RFX_XSTAT_ROWS_REVERSES = 33, /* reverse calls */
    RFX_XSTAT_ROWS_IN = 34,       /* rows the row verbs read: the table's rows (filter), the column's length (take, reverse; an atom counts 1) */
    RFX_XSTAT_ROWS_OUT = 35,      /* ... and rows they answered */
    RFX_XSTAT_CASTS = 36,         /* casts run (one per call or operator piece) */
    RFX_XSTAT_SCOPE_SPARSE_SAMPLED = 37, /* group-bys whose sampled key range alone sent them to the hashed tables (no exact scope pass) */
    RFX_XSTAT_SORT_MERGES = 38,   /* sorts over shards answered by local sorts + one multiway merge (rfx_exec_sort_shards) */
    RFX_XSTAT_NS_SORT_LOCAL = 39, /* ... wall time of their local-sort phases (to every shard's stream idle), nanoseconds */
    RFX_XSTAT_NS_SORT_MERGE = 40, /* ... and of the cross-device copies, the merge and the clean-up */
    RFX_XSTAT_CONCATS = 41,       /* concat / raze calls answered by the device path (a table counts once) */
    RFX_XSTAT_CONCAT_SPANS = 42,  /* ... spans they were given, over all columns (empty ones and atoms included) */
    RFX_XSTAT_CONCAT_CELLS = 43,  /* ... and cells they answered, over all columns */
    RFX_XSTAT_UPSERTS = 44,         /* upsert calls answered by the device path */
    RFX_XSTAT_UPSERT_MATCHED = 45,  /* ... batch rows that matched a table row (the ones a later row overwrote included) */
    RFX_XSTAT_UPSERT_APPENDED = 46, /* ... and batch rows appended */
    RFX_XSTAT_INSERTS = 47,         /* insert calls answered by the device path */
    RFX_XSTAT_NS_UPSERT_INDEX = 48, /* wall time of the upserts' index step, nanoseconds, to the stream idle */
    RFX_XSTAT_NS_UPSERT_PLAN = 49,  /* ... of their plan step */
    RFX_XSTAT_NS_UPSERT_PLACE = 50, /* ... and of the copy, fill and place */
    RFX_XSTAT_COLLECT_PARTITIONS = 51, /* group partitions answered by the device path */
    RFX_XSTAT_COLLECT_PASSES = 52,     /* ... radix passes they ran (a digit every group id agrees on costs none) */
    RFX_XSTAT_COLLECTS = 53,           /* row / collect calls over a partition */
    RFX_XSTAT_COLLECT_LAUNCHES = 54,   /* ... gather launches they took (RFX_MAX_COLS outputs to a launch) */
    RFX_XSTAT_N = 55
};
/* what ONE phase hand-over to nshards - 1 worker threads costs the calling thread (microseconds; a bare pool without devices, `reps` empty
 * phases) -- the planner's own overhead per phase of a sharded query, which a one-GPU box can measure */
double rfx_exec_probe_handover_us(int nshards, int reps);
/* on = 1: zero the RFX_XSTAT_NS_* counters and time the phases from now on (a sync per phase); on = 0: stop */
void rfx_exec_timing(rfx_exec_t *x, int on);
/* fn(arg, shard) on EVERY shard at once -- shard 0 on the calling thread, the others on the planner's own shard threads (each with its shard's
 * context bound) -- the first failure's code back.  How the operator layer uploads a column: every shard's row range through its own device's
 * copy engine and PCIe link at the same time (rfx_pin / first touch), as the reference maps every column file where it lies (core/io.c:1310-1364). */
int rfx_exec_run(rfx_exec_t *x, int (*fn)(void *arg, int shard), void *arg);
int64_t rfx_exec_stat(const rfx_exec_t *x, int which);
/* forget which key columns' sampled scopes were reported too small (the planner does not sample those again: tests start over with this) */
void rfx_exec_forget_scopes(rfx_exec_t *x);
const char *rfx_exec_last_error(const rfx_exec_t *x);

#ifndef __HIPCC_RTC__
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* RFX_EXEC_H */
