/* rfx_exec_window.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The window join's ranges and folds: the reference sorts the right table by (keys, time), keeps per key tuple its first and last row and searches
 * the window's two ends between them (index_window_join_obj, core/index.c:3269-3347; AGGR_ITER, core/aggr.c:133-160).  Here the sorted table is ONE
 * permutation -- the stable two-column sort by ("first row of my group", time) -- with the groups' boundaries found as the asof build finds them;
 * the kernels of rfx_window.hip do the rest.  One shard. */
int rfx_exec_window_ranges(rfx_exec_t *x, const void *const *dlk, const void *const *drk, int nk, const int64_t *d_lo, const int64_t *d_hi, const int64_t *d_rt,
                           int64_t nl, int64_t nr, int closed, int64_t *d_perm, int64_t *d_li, int64_t *d_ri, int64_t *stats, int *collision) {
    if (collision) *collision = 0;
    if (stats) stats[0] = stats[1] = 0;
    if (!x || !dlk || !drk || nk < 1 || nk > RFX_MAX_KEYS || nl < 0 || nr < 0 || (nl > 0 && (!d_lo || !d_hi || !d_li || !d_ri)) || (nr > 0 && (!d_rt || !d_perm)))
        return RFX_EINVAL;
    int rc = exec_one_shard(x, "window join");
    if (rc != RFX_OK) return rc;
    rfx_ctx_t *c = x->ctx[0];
    void *tmp[6];
    int ntmp = 0, quiet = 0;
    char err[sizeof(x->err)];
    err[0] = 0;
#define WT(ptr, bytes) do { ptr = NULL; if ((rc = rfx_hip_malloc(c, &ptr, (bytes))) != RFX_OK) goto out; tmp[ntmp++] = ptr; } while (0)
    void *g = NULL, *gs, *times = NULL, *seg = NULL, *ids, *dstats;
    if (nr > 0) {
        /* BUILD 1: g[r] = the first right row with right row r's key tuple; 2: the right rows by (g, time), stable */
        WT(g, (size_t)nr * 8);
        if ((rc = join_index_on(x, c, err, sizeof(err), drk, drk, nk, nr, nr, (int64_t *)g, collision)) != RFX_OK) { quiet = 1; goto out; }
        const void *cols[2] = {g, d_rt};
        const int32_t types[2] = {RFX_I64, RFX_I64};
        if ((rc = rfx_exec_sort(x, cols, types, 2, 0, nr, d_perm)) != RFX_OK) { snprintf(err, sizeof(err), "%s", x->err); quiet = 1; goto out; }
        /* BUILD 3: per group its run, addressed by its first row; the times in the sorted order */
        WT(gs, (size_t)nr * 8);
        WT(times, (size_t)nr * 8);
        WT(seg, (size_t)nr * 16);
        if ((rc = rfx_hip_gather(c, g, d_perm, nr, gs)) != RFX_OK || (rc = rfx_hip_gather(c, d_rt, d_perm, nr, times)) != RFX_OK ||
            (rc = rfx_hip_memset(c, seg, 0, (size_t)nr * 16)) != RFX_OK || (rc = rfx_hip_asof_runs(c, (const int64_t *)gs, nr, (int64_t *)seg)) != RFX_OK) goto out;
    }
    if (nl > 0) {
        /* PROBE 4: the group of every left row (a group's first right row, or null); 5: the two searches and the null tests */
        WT(ids, (size_t)nl * 8);
        WT(dstats, 16);
        if (nr == 0) rc = rfx_hip_fill_i64(c, (int64_t *)ids, nl, NULL_I64);
        else if ((rc = join_index_on(x, c, err, sizeof(err), dlk, drk, nk, nl, nr, (int64_t *)ids, collision)) != RFX_OK) { quiet = 1; goto out; }
        if (rc != RFX_OK || (rc = rfx_hip_memset(c, dstats, 0, 16)) != RFX_OK ||
            (rc = rfx_hip_window_ranges(c, d_lo, d_hi, nl, (const int64_t *)ids, nr, (const int64_t *)seg, (const int64_t *)times, closed != 0, d_li, d_ri,
                                        (uint64_t *)dstats)) != RFX_OK) goto out;
        int64_t st[2] = {0, 0};
        if ((rc = rfx_hip_d2h(c, st, dstats, 16)) != RFX_OK) goto out; /* (syncs) */
        if (stats) { stats[0] = st[0]; stats[1] = st[1]; }
        x->stat[RFX_XSTAT_SEARCHES] += 2 * nl;
    } else rc = rfx_hip_ctx_sync(c);
out:
    if (rc != RFX_OK && !quiet) snprintf(err, sizeof(err), "%s", rfx_hip_last_error());
    if (rc != RFX_OK) {
        rfx_hip_ctx_sync(c); /* (whatever was launched has read its scratch before it is freed) */
        snprintf(x->err, sizeof(x->err), "rfx_exec: window join: %.400s", err);
    }
    for (int i = 0; i < ntmp; i++) rfx_hip_free(c, tmp[i]);
    return rc;
#undef WT
}
int rfx_exec_window_fold(rfx_exec_t *x, const void *d_vals, int32_t type, const int64_t *d_perm, const int64_t *d_li, const int64_t *d_ri, int64_t nl,
                         int64_t nr, int64_t long_windows, void *const *d_outs) {
    if (!x || nl < 0 || nr < 0 || !d_outs || (nl > 0 && (!d_li || !d_ri)) || (nr > 0 && !d_vals) || (type != RFX_I64 && type != RFX_F64)) return RFX_EINVAL;
    int rc = exec_one_shard(x, "window join");
    if (rc != RFX_OK) return rc;
    if (nl == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    void *sorted = NULL;
    if (d_perm && nr > 0) {
        if ((rc = rfx_hip_malloc(c, &sorted, (size_t)nr * 8)) != RFX_OK || (rc = rfx_hip_gather(c, d_vals, d_perm, nr, sorted)) != RFX_OK) goto out;
        d_vals = sorted;
    }
    if ((rc = rfx_hip_window_fold(c, d_vals, type, nr, d_li, d_ri, nl, long_windows, d_outs)) != RFX_OK) goto out;
    rc = rfx_hip_ctx_sync(c);
out:
    if (rc != RFX_OK) {
        char err[400];
        snprintf(err, sizeof(err), "%.399s", rfx_hip_last_error());
        rfx_hip_ctx_sync(c);
        snprintf(x->err, sizeof(x->err), "rfx_exec: window fold: %s", err);
    }
    if (sorted) rfx_hip_free(c, sorted);
    return rc;
}
