/* rfx_exec_asof.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The asof join index and bin / binr: the reference keeps, per key tuple of the right table, the list of its rows in ascending row order
 * (index_asof_join_obj, core/index.c:3194-3267) and searches that list by time.  Here the lists are ONE permutation of the right rows -- a stable
 * sort by "first row of my group" -- with the groups' boundaries and the times laid out in that order; the kernels of rfx_asof.hip do the rest.
 * One shard. */
int rfx_exec_asof_index(rfx_exec_t *x, const void *const *dlk, const void *const *drk, int nk, const int64_t *d_lt, const int64_t *d_rt, int64_t nl,
                        int64_t nr, int64_t *d_ids, int *collision) {
    if (collision) *collision = 0;
    if (!x || !dlk || !drk || nk < 1 || nk > RFX_MAX_KEYS || nl < 0 || nr < 0 || (nl > 0 && (!d_ids || !d_lt)) || (nr > 0 && !d_rt)) return RFX_EINVAL;
    int rc = exec_one_shard(x, "asof join");
    if (rc != RFX_OK) return rc;
    if (nl == 0) return RFX_OK; /* (nothing to answer: no launch) */
    rfx_ctx_t *c = x->ctx[0];
    if (nr == 0) { /* no right row: no group for anybody */
        if ((rc = rfx_hip_fill_i64(c, d_ids, nl, NULL_I64)) != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: asof: %s", rfx_hip_last_error());
        else x->stat[RFX_XSTAT_ASOF_JOINS]++;
        return rc;
    }
    void *tmp[5];
    int ntmp = 0, quiet = 0;
    char err[sizeof(x->err)];
    err[0] = 0;
#define AT(ptr, bytes) do { ptr = NULL; if ((rc = rfx_hip_malloc(c, &ptr, (bytes))) != RFX_OK) goto out; tmp[ntmp++] = ptr; } while (0)
    void *g, *gs, *perm, *times, *seg;
    int64_t t0 = now_ns();
    /* BUILD 1: g[r] = the first right row with right row r's key tuple */
    AT(g, (size_t)nr * 8);
    if ((rc = join_index_on(x, c, err, sizeof(err), drk, drk, nk, nr, nr, (int64_t *)g, collision)) != RFX_OK) { quiet = 1; goto out; }
    /* BUILD 2: the right rows by group, stable: every group's rows adjacent and in ascending row order -- the reference's lists, end to end */
    AT(gs, (size_t)nr * 8);
    AT(perm, (size_t)nr * 8);
    if ((rc = rfx_exec_sort_values(x, g, RFX_I64, 0, nr, gs, (int64_t *)perm)) != RFX_OK) { snprintf(err, sizeof(err), "%s", x->err); quiet = 1; goto out; }
    /* BUILD 3: per group its run, addressed by its first row; the times in that order (one contiguous array per group) */
    AT(seg, (size_t)nr * 16);
    AT(times, (size_t)nr * 8);
    if ((rc = rfx_hip_memset(c, seg, 0, (size_t)nr * 16)) != RFX_OK) goto out; /* (a row that heads no group: the empty segment) */
    if ((rc = rfx_hip_asof_runs(c, (const int64_t *)gs, nr, (int64_t *)seg)) != RFX_OK || (rc = rfx_hip_gather(c, d_rt, (const int64_t *)perm, nr, times)) != RFX_OK ||
        (rc = rfx_hip_ctx_sync(c)) != RFX_OK) goto out;
    x->stat[RFX_XSTAT_NS_ASOF_BUILD] += now_ns() - t0;
    t0 = now_ns();
    /* PROBE 4: the group of every left row (a group's first right row, or null), left in d_ids; 5: the search rewrites d_ids in place */
    if ((rc = join_index_on(x, c, err, sizeof(err), dlk, drk, nk, nl, nr, d_ids, collision)) != RFX_OK) { quiet = 1; goto out; }
    if ((rc = rfx_hip_seg_search(c, d_lt, nl, d_ids, nr, (const int64_t *)seg, 0, (const int64_t *)times, (const int64_t *)perm, 0, NULL_I64, d_ids)) != RFX_OK ||
        (rc = rfx_hip_ctx_sync(c)) != RFX_OK) goto out;
    x->stat[RFX_XSTAT_NS_ASOF_PROBE] += now_ns() - t0;
    x->stat[RFX_XSTAT_ASOF_JOINS]++;
    x->stat[RFX_XSTAT_SEARCHES] += nl;
out:
    if (rc != RFX_OK && !quiet) snprintf(err, sizeof(err), "%s", rfx_hip_last_error());
    if (rc != RFX_OK) {
        rfx_hip_ctx_sync(c); /* (whatever was launched has read its scratch before it is freed) */
        snprintf(x->err, sizeof(x->err), "rfx_exec: asof: %.400s", err);
    }
    for (int i = 0; i < ntmp; i++) rfx_hip_free(c, tmp[i]);
    return rc;
#undef AT
}
int rfx_exec_bin(rfx_exec_t *x, const int64_t *d_x, int64_t nx, const int64_t *d_y, int64_t ny, int right, int64_t *d_out) {
    if (!x || nx < 0 || ny < 0 || (nx > 0 && !d_x) || (ny > 0 && (!d_y || !d_out))) return RFX_EINVAL;
    int rc = exec_one_shard(x, "bin");
    if (rc != RFX_OK) return rc;
    if (ny == 0) return RFX_OK;
    rc = rfx_hip_seg_search(x->ctx[0], d_y, ny, NULL, 0, NULL, nx, d_x, NULL, right != 0, right ? nx : -1, d_out);
    if (rc != RFX_OK) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: bin: %s", rfx_hip_last_error());
        return rc;
    }
    x->stat[RFX_XSTAT_BINS]++;
    x->stat[RFX_XSTAT_SEARCHES] += ny;
    return RFX_OK;
}
