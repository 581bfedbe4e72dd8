/* rfx_exec_sort.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The sorts behind iasc / idesc / asc / desc / rank / xasc / xdesc: which columns, in which order, through which permutation; the kernels of
 * rfx_sort.hip decide per column which of the eight digit passes move anything.  One shard. */
static int sort_one_shard(rfx_exec_t *x) {
    if (x->nshards > 1 || x->has_tr) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: sort over a sharded table");
        return RFX_ELIMIT;
    }
    return RFX_OK;
}
int rfx_exec_sort(rfx_exec_t *x, const void *const *d_cols, const int32_t *types, int ncols, int descending, int64_t n, int64_t *d_perm) {
    if (!x || !d_cols || !types || ncols < 1 || n < 0 || (n > 0 && !d_perm)) return RFX_EINVAL;
    x->err[0] = 0;
    int rc = sort_one_shard(x);
    if (rc != RFX_OK) return rc;
    for (int k = 0; k < ncols; k++)
        if ((types[k] != RFX_I64 && types[k] != RFX_F64) || (n > 0 && !d_cols[k])) {
            snprintf(x->err, sizeof(x->err), "rfx_exec: sort keys are i64 / timestamp / f64 columns");
            return RFX_EINVAL;
        }
    if (n == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
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
    x->err[0] = 0;
    int rc = sort_one_shard(x);
    if (rc != RFX_OK) return rc;
    if (type != RFX_I64 && type != RFX_F64) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: sort keys are i64 / timestamp / f64 columns");
        return RFX_EINVAL;
    }
    if (n == 0) return RFX_OK;
    int32_t passes = 0;
    rfx_hip_ctx_bind_thread(x->ctx[0]);
    rc = rfx_hip_sort_values(x->ctx[0], d_col, type, n, descending, d_out, d_perm, &passes);
    x->stat[RFX_XSTAT_SORTS]++;
    x->stat[RFX_XSTAT_SORT_PASSES] += passes;
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: sort: %s", rfx_hip_last_error());
    return rc;
}
