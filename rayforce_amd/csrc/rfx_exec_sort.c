/* rfx_exec_sort.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The sorts behind iasc / idesc / asc / desc / rank / xasc / xdesc: which columns, in which order, through which permutation; the kernels of
 * rfx_sort.hip decide per column which of the digit passes move anything, and by the column's type which record form runs (8-byte keys: u64 key +
 * u32 row; keys of at most 32 bits: one packed u64), so the levels of a multi-column sort may mix widths.  rfx_exec_sort / _sort_values: one shard,
 * whole-column addresses; rfx_exec_sort_shards (at the end): per-shard pieces of 8-byte keys only, local sorts on the shards' threads, one merge on
 * shard 0 (rfx_merge.hip). */
static int sort_type_ok(int32_t t) {
    return t == RFX_I64 || t == RFX_F64 || t == RFX_I32 || t == RFX_I32_WIDE || t == RFX_I16 || t == RFX_U8 || t == RFX_B8;
}
#define SORT_TYPES_WHY "rfx_exec: sort keys are i64 / timestamp / f64 columns, or i32 / date / time (raw or widened), i16, u8 and b8 ones on one shard"
int rfx_exec_sort(rfx_exec_t *x, const void *const *d_cols, const int32_t *types, int ncols, int descending, int64_t n, int64_t *d_perm) {
    if (!x || !d_cols || !types || ncols < 1 || n < 0 || (n > 0 && !d_perm)) return RFX_EINVAL;
    int rc = exec_one_shard(x, "sort");
    if (rc != RFX_OK) return rc;
    for (int k = 0; k < ncols; k++)
        if (!sort_type_ok(types[k]) || (n > 0 && !d_cols[k])) {
            snprintf(x->err, sizeof(x->err), SORT_TYPES_WHY);
            return RFX_EINVAL;
        }
    if (n == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    /* the least significant column first; every level reads the running permutation and writes the next one (never in place) */
    void *other = NULL;
    if (ncols > 1 && (rc = rfx_hip_malloc(c, &other, (size_t)n * 8)) != RFX_OK) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: sort: %s", rfx_hip_last_error());
        return rc;
    }
    int64_t *buf[2] = {d_perm, (int64_t *)other};
    int at = (ncols - 1) & 1; /* so that the last level (k = 0) writes d_perm */
    const int64_t *in = NULL;
    for (int k = ncols - 1; k >= 0 && rc == RFX_OK; k--) {
        int32_t passes = 0;
        rc = rfx_hip_sort_index(c, d_cols[k], types[k], n, descending, in, buf[at], &passes);
        x->stat[RFX_XSTAT_SORTS]++;
        x->stat[RFX_XSTAT_SORT_PASSES] += passes;
        in = buf[at];
        at ^= 1;
    }
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: sort: %s", rfx_hip_last_error());
    if (other) {
        rfx_hip_ctx_sync(c);
        rfx_hip_free(c, other);
    }
    return rc;
}
int rfx_exec_sort_values(rfx_exec_t *x, const void *d_col, int32_t type, int descending, int64_t n, void *d_out, int64_t *d_perm) {
    if (!x || n < 0 || (n > 0 && (!d_col || !d_out))) return RFX_EINVAL;
    int rc = exec_one_shard(x, "sort");
    if (rc != RFX_OK) return rc;
    if (!sort_type_ok(type)) {
        snprintf(x->err, sizeof(x->err), SORT_TYPES_WHY);
        return RFX_EINVAL;
    }
    if (n == 0) return RFX_OK;
    int32_t passes = 0;
    rc = rfx_hip_sort_values(x->ctx[0], d_col, type, n, descending, d_out, d_perm, &passes);
    x->stat[RFX_XSTAT_SORTS]++;
    x->stat[RFX_XSTAT_SORT_PASSES] += passes;
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: sort: %s", rfx_hip_last_error());
    return rc;
}

/* ---- the same orders over row-range SHARDS: every shard sorts its piece (a sorted RUN), one stable multiway merge on shard 0 (rfx_merge.hip).
 * Shards are row ranges in row order and the local sorts are stable, so the merge's order (key tuple, run, place in run) is (key tuple, global row):
 * the unsharded answer bit for bit. */
_Static_assert(RFX_MAX_SHARDS <= RFX_MERGE_MAX_RUNS, "one run per shard");
typedef struct {
    rfx_exec_t *x;
    const rfx_qcol_t *cols;
    const int32_t *types;
    int ncols, desc, want_perm;
    int64_t n;
    void *block[RFX_MAX_SHARDS]; /* the run's arrays, on the shard's own context */
    rfx_merge_run_t run[RFX_MAX_SHARDS];
    int32_t sorts[RFX_MAX_SHARDS], passes[RFX_MAX_SHARDS];
} sort_shards_t;
static size_t sort_run_cells(int ncols) { return ncols == 1 ? 2 : (size_t)ncols + 2; }
static int sort_shard_local(void *arg, int s) {
    sort_shards_t *j = (sort_shards_t *)arg;
    rfx_ctx_t *c = j->x->ctx[s];
    int64_t r0, len;
    rfx_exec_split(j->n, j->x->nshards, s, &r0, &len);
    j->run[s].row0 = r0;
    j->run[s].len = len;
    if (len <= 0) return RFX_OK;
    for (int k = 0; k < j->ncols; k++)
        if (!j->cols[k].d[s]) return RFX_EINVAL;
    rfx_hip_ctx_bind_thread(c);
    /* one key: cells | rows.  Several: rows | the other permutation of the chain | the key columns gathered into the run's order */
    int rc = rfx_hip_malloc(c, &j->block[s], sort_run_cells(j->ncols) * (size_t)len * 8);
    if (rc != RFX_OK) return rc;
    int64_t *cell = (int64_t *)j->block[s];
    if (j->ncols == 1) {
        int32_t passes = 0;
        rc = rfx_hip_sort_values(c, j->cols[0].d[s], j->types[0], len, j->desc, cell, j->want_perm ? cell + len : NULL, &passes);
        j->sorts[s]++;
        j->passes[s] += passes;
        j->run[s].d_keys[0] = cell;
        j->run[s].d_rows = j->want_perm ? cell + len : NULL;
        return rc;
    }
    int64_t *buf[2] = {cell, cell + len};
    int at = (j->ncols - 1) & 1; /* so that the last level (k = 0) writes the run's rows */
    const int64_t *in = NULL;
    for (int k = j->ncols - 1; k >= 0 && rc == RFX_OK; k--) {
        int32_t passes = 0;
        rc = rfx_hip_sort_index(c, j->cols[k].d[s], j->types[k], len, j->desc, in, buf[at], &passes);
        j->sorts[s]++;
        j->passes[s] += passes;
        in = buf[at];
        at ^= 1;
    }
    const void *src[RFX_MAX_KEYS];
    void *dst[RFX_MAX_KEYS];
    for (int k = 0; k < j->ncols; k++) {
        src[k] = j->cols[k].d[s];
        dst[k] = cell + (size_t)(2 + k) * (size_t)len;
        j->run[s].d_keys[k] = dst[k];
    }
    j->run[s].d_rows = cell;
    if (rc == RFX_OK) rc = rfx_hip_gather_many(c, src, j->ncols, cell, len, dst);
    const int src_ = rfx_hip_ctx_sync(c); /* (shard 0's stream reads the run next) */
    return rc != RFX_OK ? rc : src_;
}
int rfx_exec_sort_shards(rfx_exec_t *x, const rfx_qcol_t *cols, const int32_t *types, int ncols, int descending, int64_t n, int64_t *d_perm, void *d_values) {
    if (!x || !cols || !types || ncols < 1 || n < 0 || (n > 0 && !d_perm && !d_values) || (d_values && ncols != 1)) return RFX_EINVAL;
    x->err[0] = 0;
    for (int k = 0; k < ncols; k++)
        if ((types[k] != RFX_I64 && types[k] != RFX_F64) || (n > 0 && !cols[k].d[0])) { /* (an I32-family column comes as its widened pieces, RFX_I64) */
            snprintf(x->err, sizeof(x->err), SORT_TYPES_WHY);
            return RFX_EINVAL;
        }
    if (x->has_tr || rfx_exec_ranks(x, NULL) > 1) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: sort over several ranks");
        return RFX_ELIMIT;
    }
    if (x->nshards == 1) { /* the one-shard path as it is: same kernels, same launches, same counters */
        if (d_values) return rfx_exec_sort_values(x, cols[0].d[0], types[0], descending, n, d_values, d_perm);
        const void *one[RFX_MAX_KEYS * 2];
        if (ncols > RFX_MAX_KEYS * 2) return RFX_ELIMIT;
        for (int k = 0; k < ncols; k++) one[k] = cols[k].d[0];
        return rfx_exec_sort(x, one, types, ncols, descending, n, d_perm);
    }
    if (ncols > RFX_MAX_KEYS) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: sort over shards by more than %d columns", RFX_MAX_KEYS);
        return RFX_ELIMIT;
    }
    if (n == 0) return RFX_OK;
    sort_shards_t j;
    memset(&j, 0, sizeof(j));
    j.x = x;
    j.cols = cols;
    j.types = types;
    j.ncols = ncols;
    j.desc = descending != 0;
    j.want_perm = d_perm != NULL;
    j.n = n;
    /* (a) the local sorts: every shard on its own thread (the radix sort waits for its histograms) */
    const int64_t t0 = now_ns();
    int rc = run_shards(x, sort_shard_local, &j);
    for (int s = 0; s < x->nshards; s++) {
        x->stat[RFX_XSTAT_SORTS] += j.sorts[s];
        x->stat[RFX_XSTAT_SORT_PASSES] += j.passes[s];
    }
    rfx_ctx_t *c0 = x->ctx[0];
    rfx_hip_ctx_bind_thread(c0);
    const int64_t t1 = now_ns();
    x->stat[RFX_XSTAT_NS_SORT_LOCAL] += t1 - t0;
    /* (b) runs on another device than shard 0's come over; runs on shard 0's device are read where they lie */
    void *copy[RFX_MAX_SHARDS] = {0};
    for (int s = 1; s < x->nshards && rc == RFX_OK; s++) {
        if (x->dev[s] == x->dev[0] || j.run[s].len <= 0) continue;
        const size_t len = (size_t)j.run[s].len, bytes = sort_run_cells(ncols) * len * 8;
        rc = rfx_hip_malloc(c0, &copy[s], bytes);
        if (rc == RFX_OK) rc = rfx_hip_d2d(c0, copy[s], j.block[s], bytes);
        const char *from = (const char *)j.block[s], *to = (const char *)copy[s];
        for (int k = 0; k < ncols; k++) j.run[s].d_keys[k] = to + ((const char *)j.run[s].d_keys[k] - from);
        if (j.run[s].d_rows) j.run[s].d_rows = (const int64_t *)(to + ((const char *)j.run[s].d_rows - from));
    }
    /* (c) the merge, on shard 0's context (it returns with the stream idle, so the copies above have landed and may go) */
    if (rc == RFX_OK) {
        rc = rfx_hip_merge_runs(c0, j.run, x->nshards, types, ncols, j.desc, x->merge_tile, d_perm, d_values);
        if (rc == RFX_OK) x->stat[RFX_XSTAT_SORT_MERGES]++;
    } else rfx_hip_ctx_sync(c0);
    if (rc != RFX_OK && !x->err[0]) snprintf(x->err, sizeof(x->err), "rfx_exec: sort: %s", rfx_hip_last_error());
    /* (d) every block back to the context it came from */
    for (int s = 0; s < x->nshards; s++) {
        if (copy[s]) rfx_hip_free(c0, copy[s]);
        if (!j.block[s]) continue;
        rfx_hip_ctx_bind_thread(x->ctx[s]);
        rfx_hip_free(x->ctx[s], j.block[s]);
    }
    rfx_hip_ctx_bind_thread(c0);
    x->stat[RFX_XSTAT_NS_SORT_MERGE] += now_ns() - t1;
    return rc;
}
