/*
 * rfx_ops.h -- operator-level C ABI of librfx.so: the drop-in boundary for RayforceDB's select / where / by path.
 *
 * Every entry point has one of the reference's three operator shapes (core/ops.h:202-204)
 *
 *     obj_p f(obj_p)            unary_f          obj_p f(obj_p, obj_p)     binary_f          obj_p f(obj_p *, i64_t)   vary_f
 *
 * over the reference's 16-byte object header (include/rfx_abi.h), follows its ownership rule -- arguments are BORROWED,
 * the result is OWNED by the caller (core/eval.c:741-742,764-766,793-794) -- and reports errors by returning an object
 * of type TYPE_ERR obtained from the host's ray_err() (core/rayforce.h:292), never by longjmp / exit.  So a function
 * here can be bound with the reference's own plugin loader, unchanged:
 *
 *     (set gsel (loadfn "librfx.so" "rfx_select" 1))        ;; core/dynlib.c:153-216  dlopen(RTLD_NOW|RTLD_GLOBAL) + dlsym
 *     (gsel {s: (sum v) from: t where: (< a 100000) by: k})
 *
 * or linked in place of the reference's objects (Makefile:54-61 CORE_OBJECTS).  INTEGRATION.md shows both.
 *
 *   entry point            replaces (reference)                                  shape
 *   ---------------------  ----------------------------------------------------  -------
 *   rfx_select             ray_select            core/query.c:607-654            unary_f   (whole select dict)
 *   rfx_eq .. rfx_ge       ray_eq .. ray_ge      core/cmp.c:692-697              binary_f  -> B8 mask vector
 *   rfx_and, rfx_or        ray_and, ray_or       core/logic.c:262-264            vary_f    (over EVALUATED B8 masks: a loadfn
 *                                                                                           plugin is not a special form)
 *   rfx_where              ray_where             core/items.c:1366-1397          unary_f   -> ascending I64 row ids
 *   rfx_sum rfx_avg        ray_sum ray_avg       core/math.c:2388,2445-2526      unary_f   vector | MAPFILTER(val, ids)
 *   rfx_min rfx_max        ray_min ray_max       core/math.c:2428-2429           unary_f
 *   rfx_count rfx_first    ray_count ray_first   core/misc.c:43-60, core/items.c unary_f
 *   rfx_last rfx_dev       ray_last ray_dev      core/items.c:1112-1114, core/math.c:2628-2699   unary_f
 *   rfx_at                 at_ids via ray_at     core/rayforce.c:1100-1158       binary_f  (column, I64 ids) -> gathered column
 *   rfx_left_join          ray_left_join         core/join.c:158-198             vary_f    (key symbols, left table, right table)
 *   rfx_inner_join         ray_inner_join        core/join.c:200-298             vary_f
 *   rfx_add rfx_sub        ray_add ray_sub       core/math.c:2280-2345 (binop_map)   binary_f  vector (x) vector | atom -> vector
 *   rfx_mul rfx_div        ray_mul ray_fdiv (`div`)                                  binary_f  (i64 / f64, the reference's promotion)
 *   rfx_floordiv rfx_mod   ray_div (`/`: floor division, left operand's type) ray_mod (`%`)   binary_f  (core/math.c:1138-1364, 1449-1530)
 *   rfx_iasc rfx_idesc     ray_iasc ray_idesc    core/order.c:32-72              unary_f   I64 / TIMESTAMP / F64 / I32 / DATE / TIME / I16 / U8 / B8 vector -> I64 permutation
 *   rfx_asc rfx_desc       ray_asc ray_desc      core/order.c:74-244             unary_f   -> the sorted cells in the vector's own type, ATTR_ASC / ATTR_DESC
 *   rfx_rank               ray_rank              core/order.c:519-556            unary_f   -> the inverse of iasc
 *   rfx_xasc rfx_xdesc     ray_xasc ray_xdesc    core/order.c:246-420            binary_f  (table, column symbol | symbol vector) -> table
 *   rfx_asof_join          ray_asof_join         core/join.c:300-356             vary_f    (key symbols, the last one the asof column; left table, right table)
 *   rfx_bin rfx_binr       ray_bin ray_binr      core/items.c:1399-1644          binary_f  (I64 / TIMESTAMP vector, vector of the same type) -> I64 positions
 *   rfx_window_join rfx_window_join1  ray_window_join ray_window_join1  core/join.c:358-489  vary_f  (key symbols, windows, left table, right table, aggregates)
 *   rfx_distinct           ray_distinct          core/compose.c:839              unary_f   I64 / SYMBOL / TIMESTAMP vector -> its distinct cells, ATTR_DISTINCT
 *   rfx_in                 ray_in                core/items.c:736                binary_f  (x, y) two such vectors of one type -> B8, x[i] occurs in y
 *   rfx_find               ray_find              core/items.c:302                binary_f  (x, y) -> I64, the first row of x holding y[j], or null
 *   rfx_sect rfx_except    ray_sect ray_except   core/items.c:898-1019           binary_f  (x, y) I64 or SYMBOL pairs -> the cells of x in / not in y, in x's order
 *   rfx_union              ray_union             core/items.c:1022               binary_f  (x, y) -> distinct of x followed by y, ATTR_DISTINCT
 *   rfx_concat             ray_concat            core/compose.c:465-823          binary_f  (x, y) vectors of one type, a vector and an atom, two tables -> x's cells, then y's
 *   rfx_raze               ray_raze              core/compose.c:1096-1164        unary_f   LIST of vectors of one type -> their cells end to end
 *   rfx_row                ray_row               core/compose.c:1166-1169        unary_f   MAPGROUP(val, index) -> LIST of one I64 vector of row numbers per group
 *
 * Everything below runs on the MI355X through the flat ABI of rfx_hip.h.  There is NO CPU implementation behind these
 * entry points: queries whose shape the GPU path does not cover are handed back to the host's own ray_* function when
 * the library runs as a plugin (the host exports them, rayforce.syms), and return an error object otherwise.
 *
 * Data residency: columns are host objects.  The first query that touches a column uploads it to HBM (PCIe) and keeps
 * it in a residency cache keyed by (payload pointer, length, type); an UNPINNED copy is proven current at every use -- by the
 * soft-dirty bits of the payload's pages where the kernel tracks them (O(pages)), else by a checksum of the whole payload -- and
 * refreshed when the host wrote into it; later queries run HBM-resident.  rfx_pin (trusted until rfx_invalidate / rfx_unpin)
 * and rfx_cache_clear make that explicit.
 */
#ifndef RFX_OPS_H
#define RFX_OPS_H

#include "rfx_abi.h"

#ifdef __cplusplus
extern "C" {
#endif
#ifndef __HIPCC_RTC__
#pragma GCC visibility push(default) /* librfx.so is built with -fvisibility=hidden: what the headers under include/ declare is its WHOLE dynamic surface (plugins are
                                      * dlopen'ed RTLD_GLOBAL, core/dynlib.c:131 -- internals must not land in the host's namespace) */
#endif

/* ---- host binding ------------------------------------------------------------------------------------------------
 * The shim needs the host's constructors (vector, table, i64, f64, b8, drop_obj, clone_obj, eval, ray_err,
 * symbols_intern, str_from_symbol: all in the reference's dynamic export list, rayforce.syms).  As a plugin it finds
 * them with dlsym(RTLD_DEFAULT) on first use.  Without a host process (tests, bench, the GPU box) it falls back to the
 * minimal object allocator in rfx_host.c.  Returns 1 = reference host bound, 0 = standalone host, <0 = error. */
int rfx_host_bind(void);
/* GPU ordinal used by the operator layer (default 0 or $RFX_DEVICE).  Call before the first operator. */
int rfx_ops_set_device(int device);
/* SHARDS: the operator layer plans through rfx_exec.h over one context per shard.  Before the first operator: the devices to use
 * (ndevices = 0: $RFX_DEVICES = "0,1,2" | "all", else the one device above) and how many shards in all (0: $RFX_SHARDS, else one per
 * device; more shards than devices share devices round robin).  With more than one shard every column is split row-range over the
 * shards when it is uploaded (rfx_pin / first touch), rfx_select answers from all of them -- each shard's pass on its own host thread,
 * the partial states merged by a device kernel (same device) and ONE fused RCCL exchange (across devices) before rank / emit, as
 * ray_select merges its pool workers' partials (core/query.c:607-654, core/aggr.c:163-181,375, core/pool.c:369-424) -- and the
 * operators that need a column whole on one device return an error object. */
int rfx_ops_set_shards(const int *devices, int ndevices, int nshards);
int rfx_ops_shards(void);
/* one process per device instead: the operator layer's context joins an RCCL communicator of `world` processes (id from rfx_dist_unique_id on
 * rank 0, shipped by the host); from then on rfx_select over this process' row range of the table answers for the WHOLE table */
int rfx_ops_dist_init(int world, int rank, const void *id128);
int rfx_ops_dist_finalize(void);
struct rfx_exec;
struct rfx_exec *rfx_ops_exec(void); /* the operator layer's planner (NULL before the first operator): counters, transport */
const char *rfx_ops_last_error(void);

/* ---- the operator surface ---------------------------------------------------------------------------------------- */
rfx_obj_p rfx_select(rfx_obj_p dict);

rfx_obj_p rfx_eq(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_ne(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_lt(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_gt(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_le(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_ge(rfx_obj_p x, rfx_obj_p y);

rfx_obj_p rfx_add(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_sub(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_mul(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_div(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_floordiv(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_mod(rfx_obj_p x, rfx_obj_p y);

rfx_obj_p rfx_left_join(rfx_obj_p *x, int64_t n);  /* (keys symbol vector, left table, right table) */
rfx_obj_p rfx_inner_join(rfx_obj_p *x, int64_t n);

rfx_obj_p rfx_and(rfx_obj_p *x, int64_t n);
rfx_obj_p rfx_or(rfx_obj_p *x, int64_t n);
/* the same two as the SPECIAL FORMS the reference registers (FN_SPECIAL_FORM, core/env.c:224-225; logic_map evaluates its own arms,
 * core/logic.c:89-260): the arms arrive unevaluated.  Comparison trees over i64 / f64 vectors become one mask on the device; arms that are
 * B8 masks already take rfx_and / rfx_or; anything else is handed to the host's ray_and / ray_or.  These are the entry points to put in
 * place of ray_and / ray_or themselves (INTEGRATION.md sections 2 and 3). */
rfx_obj_p rfx_and_sf(rfx_obj_p *x, int64_t n);
rfx_obj_p rfx_or_sf(rfx_obj_p *x, int64_t n);
rfx_obj_p rfx_where(rfx_obj_p mask);
rfx_obj_p rfx_at(rfx_obj_p col, rfx_obj_p ids);

rfx_obj_p rfx_sum(rfx_obj_p x);
rfx_obj_p rfx_avg(rfx_obj_p x);
rfx_obj_p rfx_min(rfx_obj_p x);
rfx_obj_p rfx_max(rfx_obj_p x);
rfx_obj_p rfx_count(rfx_obj_p x);
rfx_obj_p rfx_first(rfx_obj_p x);
/* ray_last (core/items.c:1112-1114): a vector's last cell and a MAPFILTER pair's last collected cell, null or not; per group of a MAPGROUP pair (IDS / SHIFT
 * index, with or without filter ids) the last NON-NULL cell, null without one -- aggr_last's answer with one chunk (core/aggr.c:851-930), which is also its
 * answer whenever aggr_map does not split; with several executors and 16 384 selected rows or more the reference keeps the first chunk's value instead
 *  */
rfx_obj_p rfx_last(rfx_obj_p x);
/* ray_dev (core/math.c:2628-2699): an I64 / F64 vector or a MAPFILTER over one -> the population standard deviation of the non-null cells as F64 (two
 * passes: favg, then sqrt(sum (x - favg)^2 / l)); a MAPGROUP over I64 / TIMESTAMP / F64 values -> aggr_dev's per-group sqrt(max(0, sq/n - (s/n)^2))
 * (core/aggr.c:2250-2350,2864-2929; rfx_lastdev.hip); every other argument is the host's ray_dev */
rfx_obj_p rfx_dev(rfx_obj_p x);
/* ray_med (core/math.c:2529-2626): an I64 vector, a MAPFILTER over one, or a MAPGROUP (IDS / SHIFT index, with or without filter ids) over I64 /
 * TIMESTAMP / F64 values -> the exact median(s) as F64 (rfx_median.hip); every other argument is the host's ray_med */
rfx_obj_p rfx_med(rfx_obj_p x);
/* ray_iasc / ray_idesc / ray_asc / ray_desc / ray_rank (core/order.c:32-244,519-556) of an I64 / TIMESTAMP / F64 vector, or of an I32 / DATE /
 * TIME / I16 / U8 / B8 one (core/sort.c:183-263,481-559: by signed value, B8 / U8 by the unsigned byte; INT32_MIN is the null); ray_xasc / ray_xdesc
 * (core/order.c:246-420) of a table of 8-byte columns by one symbol or a symbol vector of I64 / TIMESTAMP / F64 columns: a stable radix sort on the
 * device (rfx_sort.hip).  Nulls first ascending, last descending; ties in ascending row order in both directions; asc / desc return the original
 * cells in the argument's type with ATTR_ASC / ATTR_DESC (| the argument's ATTR_DISTINCT); an argument carrying ATTR_ASC / ATTR_DESC is answered
 * from the attribute as the reference does (an I16 vector whose attribute asks asc / desc for a reverse is the host's: its ray_reverse has no I16
 * arm).  Every other shape (SYMBOL / C8 / LIST / DICT / ENUM keys, tables holding 1-2-4-byte columns, 1- and 2-byte keys over shards) is the
 * host's own verb. */
rfx_obj_p rfx_iasc(rfx_obj_p x);
rfx_obj_p rfx_idesc(rfx_obj_p x);
rfx_obj_p rfx_asc(rfx_obj_p x);
rfx_obj_p rfx_desc(rfx_obj_p x);
rfx_obj_p rfx_rank(rfx_obj_p x);
rfx_obj_p rfx_xasc(rfx_obj_p t, rfx_obj_p cols);
rfx_obj_p rfx_xdesc(rfx_obj_p t, rfx_obj_p cols);
/* 1: the last of those seven calls ran the device sort; 0: it was answered from an attribute / an empty argument, or handed to the host */
int rfx_last_sort_on_gpu(void);
/* vary_f: (asof-join [k1 .. kn t] left right) -- ray_asof_join, core/join.c:300-356: for every left row the right row of the same k1 .. kn tuple that
 * the reference's binary search by t over the tuple's rows (kept in ROW order; index_asof_join_obj, core/index.c:3194-3267) lands on -- on right
 * times that ascend inside every tuple, the last one at or before the left row's time -- assembled as a left join (all key columns, t included,
 * are the left table's own).  Right times that do not ascend are searched with the reference's very probe sequence, so the answers agree there too.
 * On the device (rfx_asof.hip): 1..8 equality keys that are 8-byte integer columns of one type in both tables (I64 / SYMBOL / TIMESTAMP), an asof
 * column of I64 / TIMESTAMP / I32 / DATE / TIME, every other column an 8-byte vector (the asof column is told by its NAME: its 4-byte vector under a
 * second column name is such another column).  A right-only column's unmatched rows are typed nulls (as for
 * rfx_left_join; the reference returns a LIST holding Null objects there).  Every other shape -- an F64 asof column, other key or column types,
 * more than 64 columns, sharded columns, a row-hash collision, scratch that does not fit -- and every argument error is the host's own verb.
 * binary_f: (bin x y) / (binr x y) -- ray_bin / ray_binr, core/items.c:1399-1644, of two I64 or two TIMESTAMP vectors: per cell of y the same search
 * over the whole of x by position -- bin: the last probe with x[mid] <= y, else -1; binr: the first probe with x[mid] >= y, else len x -- as an I64
 * vector.  Atoms on the right, 4-byte vectors and every other pair of types are the host's own verb. */
rfx_obj_p rfx_asof_join(rfx_obj_p *x, int64_t n);
rfx_obj_p rfx_bin(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_binr(rfx_obj_p x, rfx_obj_p y);
/* 1: the last of those three calls ran the device search; 0: it had no row to search for (an empty left table, an empty y), or went to the host */
int rfx_last_asof_on_gpu(void);
/* vary_f: (window-join [k1 .. kn t] windows left right {name: (agg col) ...}) / (window-join1 ...) -- ray_window_join / ray_window_join1,
 * core/join.c:358-489: `windows` is a LIST of two vectors, a lower and an upper bound of t per left row; every left row folds `agg` over the right
 * rows of its k1 .. kn tuple, in order of t, from the row the reference's search finds for the lower bound -- window-join: the last with t <= lo, so
 * the row prevailing at the window's start is inside; window-join1: the first with t >= lo -- to the last with t <= hi.  The result is the left
 * table's columns followed by one column per dict entry (count: I64, avg: F64, else the column's type); a left row without a group, or whose
 * window the reference's tests call empty, counts 0 and is null elsewhere.
 * On the device (rfx_window.hip): 1..8 equality keys that are 8-byte integer columns of one type in both tables (I64 / SYMBOL / TIMESTAMP), a
 * window column of TIME / DATE / I32 of one type in both tables, two 4-byte integer window vectors of the left table's length, aggregates of the
 * form (agg col) with agg one of sum, min, max, count, avg, first, last (the function object or its name) and col an I64 or F64 column of the
 * right table (at most 64 entries over 16 columns).  An empty left table is answered with empty typed columns.  Every other shape -- raw columns
 * ({bids: Bid}), med / dev, nested expressions, other value types, an 8-byte window column, parted tables, sharded columns, a row-hash collision,
 * scratch that does not fit -- and every argument error is the host's own verb. */
rfx_obj_p rfx_window_join(rfx_obj_p *x, int64_t n);
rfx_obj_p rfx_window_join1(rfx_obj_p *x, int64_t n);
/* 1: the last of those two calls ran on the device; 0: its left table was empty, or it went to the host */
int rfx_last_window_on_gpu(void);

/* The set verbs over plain I64 / SYMBOL / TIMESTAMP vectors (host vectors or device-column handles) on the device (rfx_set.hip), each on the ROUTE the
 * reference takes for the same cells (index_distinct_i64, index_in_i64_i64, index_find_i64: core/index.c:551-607,1291-1361,1507-1574):
 *   distinct / union: dense (max - min + 1 <= len or <= 2^20) the values ascending, else the keys in the slot order of the reference's linear-probing
 *     table -- the result carries x's type and ATTR_DISTINCT; in -> B8 of x's length; find -> I64 of y's length (I64(0) when x is empty);
 *     sect / except (I64 or SYMBOL pairs; except also a vector and an atom of its type) -> the kept cells of x, x's type, no attribute.
 * The host's own verb answers every other shape -- atoms elsewhere, ENUM / MAPLIST / parted / 1-2-4-byte / F64 / GUID / LIST operands, two types,
 * tables, sharded columns, scratch that does not fit -- every error the reference words itself, and every shape for which the reference's tables are
 * indexed outside themselves (a hash route over a negative key, `find`'s over a null, a range beyond 64 bits: DESIGN.md section 4); without a host
 * those are refused ("not covered ... no host function").  The reason is in rfx_ops_last_error(). */
rfx_obj_p rfx_distinct(rfx_obj_p x);
rfx_obj_p rfx_find(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_in(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_sect(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_except(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_union(rfx_obj_p x, rfx_obj_p y);
/* 1: the last of those six calls was answered by the device path (an empty operand included: no launch); 0: it went to the host or failed.
 * rfx_last_set_route: the route it took, RFX_SET_ROUTE_* of rfx_exec.h (1 dense, 2 hash, 3 disjoint scopes, 4 except's atom, 0 nothing to do) */
int rfx_last_set_on_gpu(void);
int rfx_last_set_route(void);
/* unary_f: I64[7] counters of those six verbs since load: {calls answered by the device path, calls handed to the host (or refused for want of one),
 * then the answered calls by route: nothing to look up, dense, hash, disjoint scopes, except's atom}; the argument is ignored.  Loadable like
 * rfx_stats, whose 17 cells stay what they were: what tells a host that the device answered. */
rfx_obj_p rfx_set_stats(rfx_obj_p ignored);

/* The bucket verbs as built-ins of their own (rfx_bucket.hip), every result a fresh host vector of the reference's result type:
 *   binary_f (xrank v n)  ray_xrank  core/order.c:598-649   v an I64 / TIMESTAMP / F64 vector (host vector or device-column handle), n an atom of type
 *       -I64 / -I32 / -I16 / -U8: I64 of v's length, cell i = (rank of v[i] under the stable ascending sort * n) / len; a v carrying ATTR_ASC /
 *       ATTR_DESC is answered from the attribute by the index formula alone; an empty v answers I64[0] without dividing.
 *   binary_f (xbar x y)   ray_xbar   core/math.c:1635-1782  every arm of ray_xbar_partial with at least one vector operand: x of I32 / I64 / F64 / DATE /
 *       TIME / TIMESTAMP, y an atom or vector of the types that arm lists (atom x with vector y included) -> I32 / I64 / F64 / DATE / TIME / TIMESTAMP
 *       by infer_xbar_type.  The function object behind "xbar" inside by: is still bucketed by rfx_select's planner as before.
 *   binary_f (within x r) ray_within core/items.c:848-872   an I64 vector against a 2-cell I64 vector -> B8
 *   unary_f  floor / ceil / round    core/math.c:2047-2117  F64 vectors -> F64, the reference's FLOORF64 / CEILF64 / ROUNDF64 with their (i64) casts
 *   unary_f  neg          ray_neg    core/order.c:445-497   I32 / I64 vectors -> I64, F64 -> F64
 * The host's own verb answers every other shape -- atoms alone, other vector types, n <= 0 or of another type (xrank's domain / type errors), (len - 1) * n
 * beyond 63 bits, vectors of unequal length, xrank over sharded columns or without room for its scratch -- and every error it words itself; without a
 * host those are refused with the reason, which is also in rfx_ops_last_error().  The element-wise verbs run over every shard's rows. */
rfx_obj_p rfx_xrank(rfx_obj_p v, rfx_obj_p n);
rfx_obj_p rfx_xbar(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_within(rfx_obj_p x, rfx_obj_p range);
rfx_obj_p rfx_floor(rfx_obj_p x);
rfx_obj_p rfx_ceil(rfx_obj_p x);
rfx_obj_p rfx_round(rfx_obj_p x);
rfx_obj_p rfx_neg(rfx_obj_p x);
/* 1: the last of those seven calls was answered by the device path (an empty vector included: no launch); 0: it went to the host or failed */
int rfx_last_bucket_on_gpu(void);

/* The row verbs as built-ins of their own (rfx_rows.hip): rows out of vectors and tables, every result fresh host vectors (a table: a fresh table of them)
 * with the reference's cells, type codes and attributes.  "A row type" below: I64 / SYMBOL / TIMESTAMP / F64 / I32 / DATE / TIME / B8.
 *   binary_f (filter x mask)  ray_filter   core/items.c:338-396    x a vector of a row type or a TABLE whose every column is one (host vectors or device-column
 *       handles); mask a B8 vector of the same length, a host vector or a device-column handle; any non-zero mask byte selects its row.  Runs over every
 *       shard's rows: the mask goes to a 1-bit selection and straight into the ordered compaction of all columns.
 *   binary_f (take from count) ray_take    core/items.c:398-734    from a vector or an atom of a row type, or a TABLE of such columns; count an -I64 / -I32 /
 *       -I16 atom (negative: from the end; cyclic beyond the length: j0 = (l - m % l) * (count < 0)) or an I64 vector [start amount] (a negative start
 *       counts from the end; clamped to the rows there are).
 *   unary_f  (reverse x)       ray_reverse core/compose.c:144-202  a vector of a row type; ATTR_ASC and ATTR_DESC change places, the other attributes stay.
 * The host's own verb answers everything else -- I16 / U8 / C8 / GUID / LIST / ENUM / MAPLIST / DICT, parted tables, a table without columns or with
 * columns of unequal length, 4-byte device-column handles; whatever the reference answers with an error of its own wording (a mask that is not B8,
 * lengths that differ, a negative range amount, a count of another type, reverse of a table); a count take from an empty vector or table (the reference
 * divides by its length), a count of INT64_MIN, a range whose start + amount leaves 63 bits; take and reverse over more than one shard; a filter naming
 * more than 63 columns when there is more than one shard; a result the device has no room for.  Without a host those are refused with the reason, which is also in rfx_ops_last_error(). */
rfx_obj_p rfx_filter(rfx_obj_p x, rfx_obj_p mask);
rfx_obj_p rfx_take(rfx_obj_p from, rfx_obj_p count);
rfx_obj_p rfx_reverse(rfx_obj_p x);
/* 1: the last of those three calls was answered by the device path (an empty result included: no launch); 0: it went to the host or failed */
int rfx_last_rows_on_gpu(void);

/* `as` as a built-in of its own (rfx_cast.hip):
 *   binary_f (as 'T x)  ray_cast_obj  core/compose.c:42-68, cast_obj core/rayforce.c:2312-2831   'T a symbol atom naming one of B8 U8 I16 I32 I64 F64 DATE
 *       TIME TIMESTAMP by its vector name or its atom name ('i32 answers as 'I32 over a vector); x a plain vector of one of those nine types, a host vector
 *       or an I64 / F64 / TIMESTAMP / B8 device-column handle.  One C cast per cell, nulls not carried (rfx_hip.h, rfx_hip_cast).  The same type answers a
 *       clone of x (its attributes with it), an empty x an empty vector of the target type, every other pair a fresh host vector of the target type,
 *       attribute byte 0.  Runs over every shard's rows.
 * The host's own verb answers everything else -- atoms, LIST / C8 / SYMBOL / GUID / ENUM vectors, tables and dicts, a type name that is no symbol atom or
 * names another type, B8 <-> U8 (the reference has no such arm: its type error), 4-byte / 2-byte / U8 device-column handles, a result the device has no
 * room for.  Without a host those are refused with the reason, which is also in rfx_ops_last_error(). */
rfx_obj_p rfx_as(rfx_obj_p type_name, rfx_obj_p x);
/* 1: the last rfx_as was answered by the device path (a clone and an empty vector included: no launch); 0: it went to the host or failed */
int rfx_last_cast_on_gpu(void);

/* The write side as built-ins of their own (rfx_concat.hip): a table grows by (concat t batch), per-partition answers are put back together by (raze (list
 * v1 v2 ...)).  "A concat type" below: B8 / U8 / I16 / I32 / DATE / TIME / I64 / SYMBOL / TIMESTAMP / F64.
 *   binary_f (concat x y)  ray_concat  core/compose.c:465-823    two vectors of one concat type; such a vector and an atom of its type, on either side; two
 *       TABLEs whose every column is such a vector and whose names are the same set: y's columns are taken in x's name order, the result carries x's names.
 *   unary_f  (raze l)      ray_raze    core/compose.c:1096-1164  a LIST of one or more vectors that all have one concat type, empties among them included.
 * Operands are host vectors or I64 / F64 / SYMBOL / TIMESTAMP / B8 device-column handles; every result is fresh host vectors of the operands' type, attribute
 * byte 0, each column ONE multi-span copy on the device (a table's columns RFX_MAX_COLS to a launch) read back.
 * THE RESULT INHERITS RESIDENCY: the device buffer of every I64 / SYMBOL / TIMESTAMP / F64 / B8 result column stays in the residency cache as the copy of
 * the fresh result vector (the cache holds its reference, counts the bytes against its budget and evicts it like any entry), so that an operator over the
 * answer uploads nothing.  I32 / DATE / TIME results are not adopted (the cache keeps their widened image), I16 / U8 are never resident.
 * RFX_CONCAT_ADOPT=0 in the environment turns adoption off.
 * The host's own verb answers everything else -- an atom with an atom; operands of different types (the reference answers a LIST); C8 / GUID / ENUM / LIST /
 * DICT / MAPLIST operands and parted columns; tables whose name sets differ or whose paired columns differ in type (the reference words those errors
 * itself); raze of something that is not a list, of an empty list, of elements that are not all vectors of one type; 4-byte, 2-byte and U8 device-column
 * handles; more than one shard or rank; a result the device has no room for.  Without a host those are refused with the reason, which is also in
 * rfx_ops_last_error(). */
rfx_obj_p rfx_concat(rfx_obj_p x, rfx_obj_p y);
rfx_obj_p rfx_raze(rfx_obj_p list);
/* 1: the last of those two calls was answered by the device path (an empty result included: no launch); 0: it went to the host or failed */
int rfx_last_concat_on_gpu(void);

/* The keyed write (rfx_upsert.hip): a batch merged into a table VALUE; the result is a new table, to be bound by the caller: (set t (upsert t 1 batch)).
 *   vary_f (upsert t keys batch)  ray_upsert  core/update.c:556-750  keys an -I64 atom, 1 .. 8: the first `keys` columns of t are the key.  Every batch row
 *       whose key tuple equals a row of t -- the FIRST such row of t as it was -- overwrites that row's value columns, the last such batch row winning;
 *       every other batch row is appended, in batch order, two rows with the same new key both.
 *   vary_f (insert t batch)       ray_insert  core/update.c:414-542  every batch row appended.
 * t: a TABLE whose every column is a plain vector of a concat type, its key columns I64 / SYMBOL / TIMESTAMP.  batch: a LIST of l <= p vectors of the
 * columns' own types and one length >= 1 (upsert: columns l .. p - 1 keep their matched rows and append their null; insert: l == p), a LIST of atoms (one
 * record), or a DICT with symbol keys / a TABLE in any name order (a column it misses is a null VECTOR: matched rows take the null too).  Operands are host
 * vectors or the device-column handles concat takes.  The result: a fresh table over a clone of t's names, every column a fresh host vector of its type,
 * attribute byte 0; its I64 / SYMBOL / TIMESTAMP / F64 / B8 columns stay resident exactly as concat's do (RFX_CONCAT_ADOPT=0 turns that off).
 * Handed to the host's own verb (without a host: refused, the reason in rfx_ops_last_error()): the quoted-symbol in-place form; keys > 8 and key columns
 * of other types; a null or a negative key on find's hash route, a key range beyond 64 bits, two key tuples under one row hash; an F64 batch cell for an
 * integer column and every other batch type that is not the column's; LIST / ENUM / MAPLIST / C8 / GUID columns and parted tables; DATE / TIME columns, U8
 * columns under upsert or one record, and a matched row for a B8 / I16 / I32 value column (the reference's set_idx turns those into LIST columns: known
 * once the index is); a column not provided
 * whose null(type) is no cell (U8 / I16 / I32 / DATE / TIME under a short LIST or a one-record DICT: the reference answers a LIST column); one record under
 * two or more keys (the reference does not find its row); a batch of no rows (insert: the reference's length error; upsert: it answers t's own vectors); insert's short LIST (a ragged table); 2^31 or more batch rows; more
 * than one shard or rank; a result the device has no room for; and every error the reference words itself -- arity, keys < 1, more batch columns than t
 * has, unequal lengths, unknown DICT names. */
rfx_obj_p rfx_upsert(rfx_obj_p *x, int64_t n);
rfx_obj_p rfx_insert(rfx_obj_p *x, int64_t n);
/* 1: the last of those two calls was answered by the device path; 0: it went to the host or failed */
int rfx_last_upsert_on_gpu(void);

/* The nested results of select ... by: (rfx_collect.hip): every group's rows and cells as a LIST of `groups` vectors, attribute byte 0, groups in the
 * index's own order, every vector in visiting order (AGGR_ITER, core/aggr.c:73-125: one thread, so the answer does not depend on the pool).
 *   rfx_row      ray_row (core/compose.c:1166-1169 -> aggr_row, core/aggr.c:3118-3136; FN_AGGR): a MAPGROUP (val, index) pair -> one I64 vector of row
 *                numbers per group; val's cells are never read.
 *   rfx_collect  aggr_collect (core/aggr.c:3021-3116), which the reference reaches through select / update only -- declared for the standalone host, the
 *                tests and rfx_select: the same pairs over a value column of type B8 U8 I16 I32 DATE TIME I64 SYMBOL TIMESTAMP F64 -> one vector of that
 *                type per group.
 * The index is INDEX_TYPE_IDS or INDEX_TYPE_SHIFT, with or without filter ids.  The device builds ONE buffer in group order plus the offsets (a stable
 * partition by group id, then a gather), both are read back once, the host cuts the vectors out with a memcpy each.  groups == 0 or no element: `groups`
 * empty vectors, no launch.
 * Handed to the host's own ray_row (rfx_collect, and both without a host: refused with the reason, also in rfx_ops_last_error()): parted / window
 * indexes; ENUM / GUID / LIST / C8 / parted value columns; a plain vector or a MAPFILTER pair; more than one shard ("collect over a sharded table");
 * 2^31 or more elements; a result the device has no room for; 4-byte and narrower device-column handles.
 * A malformed index is an error of ours, as for the grouped aggregates: wrong slot count, ids / filter length mismatch, an id outside [0, groups), a source
 * cell outside the SHIFT table, a filter id outside the column -- checked on the device before any of them is used as an index. */
rfx_obj_p rfx_row(rfx_obj_p x);
rfx_obj_p rfx_collect(rfx_obj_p x);
/* 1: the last of those two calls was answered by the device path (an empty answer included: no launch); 0: it went to the host or failed */
int rfx_last_collect_on_gpu(void);

/* ---- residency ---------------------------------------------------------------------------------------------------- */
/* unary_f: (update {col: mapping ... from: t [where: p] [by: k]}) -- ray_update, core/update.c:936-1106: a NEW table whose named columns
 * carry the mapping's values at the selected rows (value i at row ids[i]; under by: every group's aggregate at all of its selected
 * rows; unknown names become new columns, null elsewhere).  `from:` must be a table value; the in-place form on a quoted global and
 * everything the device path does not cover go to the host's ray_update. */
rfx_obj_p rfx_update(rfx_obj_p update_dict);
/* unary_f: the reference's 7-slot group index of an i64 key column (index_group_i64_scoped, core/index.c:2002-2092), built on the
 * device: what a link-time replacement of index_group hands to the FN_AGGR built-ins inside a MAPGROUP pair.  rfx_sum .. rfx_first
 * accept such pairs (val, index) -- with indexes built here or by the reference -- besides vectors and MAPFILTER pairs. */
rfx_obj_p rfx_group(rfx_obj_p keys);
/* Residency (round 6): a cached device copy HOLDS A REFERENCE to its host vector (clone_obj / drop_obj, rayforce.syms:25-26).  By the reference's
 * own rule -- in-place writes only with rc == 1: cow_obj core/rayforce.c:3003-3026, core/math.c:2248,2310, every writer of core/update.c --
 * its cells cannot change and its address cannot be reused while the copy lives, so a later use is validated by ONE pointer compare, pinned or not,
 * and an UNPATCHED reference never sees a stale answer.  Entries whose vector nobody else refers to any more are released at the next operator call. */
rfx_obj_p rfx_pin(rfx_obj_p table_or_column);   /* unary_f: upload NOW + exempt from LRU eviction; returns a clone of its argument */
rfx_obj_p rfx_unpin(rfx_obj_p table_or_column); /* unary_f: drop the device copies (and the cache's references) */
/* unary_f: drop every cached device copy overlapping this vector / this table's columns.  Never needed under validation by ownership; in
 * checksum mode (below) it is what a host that writes PINNED vectors in place calls afterwards */
rfx_obj_p rfx_invalidate(rfx_obj_p table_or_column);
/* How cached copies are proven current: 0 = by ownership (default), 1 = by a checksum of the full payload on every use of an unpinned entry,
 * keyed by (payload address, length, type) -- for a host that writes payloads in place without looking at reference counts (raw views over the
 * standalone host's vectors).  Also RFX_VALIDATE=checksum in the environment.  Switching drops the cached copies. */
int rfx_ops_set_validation(int mode);
/* Reproducible grouped f64 sums (opt-in; also RFX_DETERMINISTIC=1): rfx_select runs every (sum x) / (avg x) over f64 under by: as an INTEGER sum over x
 * scaled by a power of two and rounded once per cell -- the same bits whatever order the rows reach their group in (the reference is bit-stable for a fixed
 * pool size, core/pool.c:415-424; the default path's f64 atomics are not).  mode 1: ONE i64 limb -- a cell is rounded to a multiple of 2^(e + b - 62)
 * (2^e > max |x|, 2^b >= rows): absolute, so a group of values far below the column's largest loses relative precision; mode 2 (RFX_DETERMINISTIC=2): a
 * SECOND limb adds up what the first one's cells rounded away, scaled by 2^(62 - b) more -- 2^(e + 2b - 124) per cell, below an f64 sum's own rounding for
 * any data whose magnitudes span less than ~2^60; one more i64 sum per aggregate.  The images of a resident column are made once and cached with it (8 bytes
 * of HBM per row and limb); a column holding a NaN or an infinity keeps the default path.  DESIGN.md section 4.
 * The reproducible modes do not cover `dev`: rfx_dev / rfx_exec_group_dev keep their three f64 sums per group through the default path's atomics in
 * either mode (the scalar dev folds its block partials in a fixed order and is run-to-run stable without them). */
int rfx_ops_set_deterministic(int mode);
/* One process per device (rfx_ops_dist_init, or a transport on the planner): 1 = a grouped rfx_select returns only THIS rank's range of the groups
 * (rfx_exec_split(groups, ranks, rank) in the answer's order: the ranks' tables end to end are the answer) instead of the whole answer on every rank; also
 * RFX_RANK_SLICES=1.  Nothing changes in a process of its own. */
int rfx_ops_set_rank_slices(int on);
/* unary_f: I64[17] counters since load: {selects on the GPU, selects delegated to the host, joins on the GPU, joins delegated,
 * uploads, cache hits, stale entries refreshed, operator calls, group scopes sampled, sampled scopes retried exactly,
 * materialised B8 mask passes (RFX_STAT_MASK_PASSES: a fused `where:` tree runs none), uses validated by soft-dirty page bits,
 * uses that cost a full-payload checksum (0 under ownership), uses validated by ownership, entries released because the cache held the
 * last reference, fixed-point images of resident f64 columns made for the reproducible sums, such images found again}; the argument is ignored */
rfx_obj_p rfx_stats(rfx_obj_p ignored);
void rfx_cache_clear(void);
int64_t rfx_cache_bytes(void);
/* statistics of the most recent rfx_select: 1 = ran on the GPU path, 0 = delegated to the host's ray_select */
int rfx_last_select_on_gpu(void);

/* ---- standalone host (rfx_host.c): just enough object model to build queries without the reference ---------------- */
rfx_obj_p rfx_host_vector(int8_t type, int64_t len);
/* A DEVICE column handle for standalone hosts that keep their columns in HBM already: a vector header whose payload is the cells' device
 * address instead of the cells.  nptrs = 1: one allocation (shards on the same device take their row ranges of it); nptrs = shards: one
 * address per shard (rows rfx_exec_split(len, shards, s)).  Types: I64 / F64 / SYMBOL / TIMESTAMP / B8.  The memory is borrowed: the
 * operators never upload, cache, validate or free it; rfx_host_drop frees the header only. */
rfx_obj_p rfx_host_device_vector(int8_t type, int64_t len, const void *const *d_ptrs, int nptrs);
rfx_obj_p rfx_host_i64(int64_t v);
rfx_obj_p rfx_host_f64(double v);
rfx_obj_p rfx_host_symbol(const char *name);             /* symbol atom */
rfx_obj_p rfx_host_list(int64_t len);                    /* LIST of `len` null slots; fill with RFX_AS_LIST */
rfx_obj_p rfx_host_table(rfx_obj_p keys, rfx_obj_p vals); /* takes ownership of both */
rfx_obj_p rfx_host_dict(rfx_obj_p keys, rfx_obj_p vals);
rfx_obj_p rfx_host_fn(const char *name);                 /* function object for "sum" "<" "and" ... bound to rfx_* */
rfx_obj_p rfx_host_clone(rfx_obj_p o);
void rfx_host_drop(rfx_obj_p o);
int64_t rfx_host_intern(const char *s, int64_t len);
const char *rfx_host_symbol_name(int64_t id);
const char *rfx_host_error_text(rfx_obj_p err);          /* message of an error object made by the standalone host */

#ifndef __HIPCC_RTC__
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* RFX_OPS_H */
