/* rfx_exec_collect.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * row and collect (rfx_collect.hip): the stable partition of the elements by dense group id, then every column gathered through it, RFX_MAX_COLS columns
 * to a launch over the same permutation.  Both read across whole columns, so these run on one shard, one rank, as the sort does. */
void rfx_exec_group_partition_free(rfx_exec_t *x, rfx_partition_t *p) {
    if (!x || !p) return;
    if (p->d_offsets) rfx_hip_free(x->ctx[0], p->d_offsets);
    if (p->d_perm) rfx_hip_free(x->ctx[0], p->d_perm);
    memset(p, 0, sizeof(*p));
}
int rfx_exec_group_partition(rfx_exec_t *x, const int64_t *d_gid, int64_t m, int64_t groups, rfx_partition_t *out) {
    if (!x || !out || m < 0 || groups < 0 || (m > 0 && !d_gid)) return RFX_EINVAL;
    memset(out, 0, sizeof(*out));
    int rc = exec_one_shard(x, "collect");
    if (rc != RFX_OK) return rc;
    if (m >= 0x80000000LL || groups >= 0x80000000LL) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: collect: 2^31 or more elements or groups");
        return RFX_ELIMIT;
    }
    rfx_ctx_t *c = x->ctx[0];
    void *p = NULL;
    if ((rc = exec_fail(x, "collect", "offsets", rfx_hip_malloc(c, &p, (size_t)(groups + 1) * 8))) != RFX_OK) return rc;
    out->d_offsets = (int64_t *)p;
    if (m > 0) {
        p = NULL;
        if ((rc = exec_fail(x, "collect", "permutation", rfx_hip_malloc(c, &p, (size_t)m * 8))) != RFX_OK) {
            rfx_exec_group_partition_free(x, out);
            return rc;
        }
        out->d_perm = (int64_t *)p;
    }
    int32_t passes = 0;
    rc = exec_fail(x, "collect", "partition", rfx_hip_group_partition(c, d_gid, m, groups, out->d_offsets, out->d_perm, &passes));
    if (rc == RFX_OK) rc = exec_fail(x, "collect", "partition", rfx_hip_ctx_sync(c));
    if (rc != RFX_OK) {
        rfx_exec_group_partition_free(x, out);
        return rc;
    }
    out->m = m;
    out->groups = groups;
    x->stat[RFX_XSTAT_COLLECT_PARTITIONS]++;
    x->stat[RFX_XSTAT_COLLECT_PASSES] += passes;
    return RFX_OK;
}
int rfx_exec_group_collect(rfx_exec_t *x, const rfx_partition_t *part, const int64_t *d_rows, int64_t col_len, const void *const *d_cols, const int32_t *widths,
                           int ncols, void *const *d_outs, int want_rows, int64_t *d_rows_out) {
    if (!x || !part || ncols < 0 || col_len < 0 || (ncols > 0 && (!d_cols || !widths || !d_outs)) || (want_rows && !d_rows_out && part->m > 0)) return RFX_EINVAL;
    int rc = exec_one_shard(x, "collect");
    if (rc != RFX_OK) return rc;
    const int64_t m = part->m;
    const int total = ncols + (want_rows ? 1 : 0);
    if (total == 0) return RFX_EINVAL;
    x->stat[RFX_XSTAT_COLLECTS]++;
    if (m == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    if (!d_rows && m > col_len) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: collect: more elements than the columns hold");
        return RFX_EINVAL;
    }
    if (d_rows) { /* the filter's ids come from outside: one outside the columns is an error, not a read */
        int64_t bad = 0;
        if ((rc = exec_fail(x, "collect", "row ids", rfx_hip_ids_check(c, d_rows, m, col_len, &bad))) != RFX_OK) return rc;
        if (bad) {
            snprintf(x->err, sizeof(x->err), "rfx_exec: collect: a row id outside the columns");
            return RFX_EINVAL;
        }
    }
    rfx_collect_col_t cc[RFX_MAX_COLS];
    int np = 0;
    for (int k = 0; k < total && rc == RFX_OK; k++) {
        if (k < ncols) {
            if (!d_cols[k]) return RFX_EINVAL; /* (the identity is asked for by want_rows) */
            cc[np].d_col = d_cols[k];
            cc[np].d_out = d_outs[k];
            cc[np].width = widths[k];
        } else {
            cc[np].d_col = NULL;
            cc[np].d_out = d_rows_out;
            cc[np].width = 8;
        }
        cc[np]._pad = 0;
        np++;
        if (np == RFX_MAX_COLS || k == total - 1) {
            rc = exec_fail(x, "collect", "gather", rfx_hip_group_collect(c, cc, np, part->d_perm, d_rows, m, col_len));
            if (rc == RFX_OK) x->stat[RFX_XSTAT_COLLECT_LAUNCHES]++;
            np = 0;
        }
    }
    return rc;
}
