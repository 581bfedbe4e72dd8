/* rfx_exec_median.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * `med`, scalar and under one by: column: which rows count (the query's where:, as preds or as the caller's mask) and in which group (the group-by's own
 * result, looked up from every row's key), then the kernels of rfx_median.hip.  One shard. */
static int med_one_shard(rfx_exec_t *x, const rfx_query_t *q) {
    if (x->nshards > 1) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: med runs on one shard");
        return RFX_ELIMIT;
    }
    if (q->cols && q->ncols < 0) return RFX_EINVAL;
    return RFX_OK;
}
int rfx_exec_median(rfx_exec_t *x, const rfx_query_t *q, const void *d_col, int32_t col_type, rfx_value_t *out) {
    if (!x || !q || !out || (q->nrows > 0 && !d_col)) return RFX_EINVAL;
    x->err[0] = 0;
    int rc = med_one_shard(x, q);
    if (rc != RFX_OK) return rc;
    if (col_type != RFX_I64) { /* (ray_med has no arm for f64 / timestamp vectors: err_type there) */
        snprintf(x->err, sizeof(x->err), "rfx_exec: scalar med of an i64 column only");
        return RFX_EINVAL;
    }
    rfx_hip_ctx_bind_thread(x->ctx[0]);
    rc = rfx_hip_median(x->ctx[0], q->preds, q->npred, q->logic, q->d_mask, (const int64_t *)d_col, q->nrows, out);
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: med: %s", rfx_hip_last_error());
    return rc;
}
/* Every selected row's group in `g` (rfx_exec_group_by of the same query, one key, one slice):
 *   dense keys  the slot -> group table of g's keys (range <= rows + groups), read inside the median's own passes (key column + table);
 *   sparse      the join index of the key column against g's keys (one probe per row -> a group index column, 8 B per row). */
int rfx_exec_group_median(rfx_exec_t *x, const rfx_query_t *q, const rfx_groups_t *g, const void *d_col, int32_t col_type, void *d_out) {
    if (!x || !q || !g || (g->groups > 0 && !d_out) || (q->nrows > 0 && !d_col)) return RFX_EINVAL;
    x->err[0] = 0;
    int rc = med_one_shard(x, q);
    if (rc != RFX_OK) return rc;
    if (q->nkeys != 1 || g->nkeys != 1 || g->nslices > 1 || (q->kxbar && q->kxbar[0] > 0) || !q->d_keys || !q->d_keys[0]) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: grouped med needs one plain key column and a one-slice result");
        return RFX_ELIMIT;
    }
    if (col_type != RFX_I64 && col_type != RFX_F64) return RFX_EINVAL;
    if (g->groups == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    rfx_med_rows_t rows;
    memset(&rows, 0, sizeof(rows));
    rows.preds = q->preds;
    rows.npred = q->npred;
    rows.logic = q->npred ? q->logic : RFX_AND;
    rows.d_mask = q->d_mask;
    void *scratch = NULL;
    int64_t kmin = 0, kmax = 0, cnt = 0;
    rc = rfx_hip_scope_i64(c, g->d_keys, NULL, 0, RFX_AND, g->groups, &kmin, &kmax, &cnt);
    const uint64_t range = (uint64_t)kmax - (uint64_t)kmin + 1;
    if (rc == RFX_OK && range != 0 && range <= (uint64_t)q->nrows + (uint64_t)g->groups) {
        rc = rfx_hip_malloc(c, &scratch, (size_t)range * 8);
        if (rc == RFX_OK) rc = rfx_hip_key_slot_table(c, g->d_keys, g->groups, kmin, (int64_t)range, (int64_t *)scratch);
        rows.d_key = (const int64_t *)q->d_keys[0];
        rows.d_table = (const int64_t *)scratch;
        rows.kmin = kmin;
        rows.range = (int64_t)range;
    } else if (rc == RFX_OK) {
        int collision = 0;
        const void *right[1] = {g->d_keys};
        rc = rfx_hip_malloc(c, &scratch, (size_t)(q->nrows ? q->nrows : 1) * 8);
        if (rc == RFX_OK) rc = rfx_exec_join_index(x, q->d_keys, right, 1, q->nrows, g->groups, (int64_t *)scratch, &collision);
        if (rc == RFX_OK && collision) rc = RFX_ESTATE;
        rows.d_gids = (const int64_t *)scratch;
    }
    if (rc == RFX_OK) rc = rfx_hip_group_median(c, &rows, d_col, col_type, q->nrows, g->groups, RFX_MED_GROUPED, (double *)d_out);
    if (rc != RFX_OK && !x->err[0]) snprintf(x->err, sizeof(x->err), "rfx_exec: grouped med: %s", rfx_hip_last_error());
    if (scratch) {
        rfx_hip_ctx_sync(c);
        rfx_hip_free(c, scratch);
    }
    return rc;
}
