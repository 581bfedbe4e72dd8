/* rfx_exec_upsert.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * upsert and insert (rfx_upsert.hip): index, plan, then per column copy + fill + place.  The index reads across whole columns and the place writes
 * anywhere in them, so these run on one shard, one rank, as concat does. */
int rfx_exec_upsert_index(rfx_exec_t *x, const void *const *d_table_keys, const void *const *d_batch_keys, int nkeys, int64_t n, int64_t m, int64_t *d_idx,
                          int *undefined) {
    if (undefined) *undefined = 0;
    if (!x || !d_table_keys || !d_batch_keys || nkeys < 1 || nkeys > RFX_MAX_KEYS || n < 0 || m < 0 || (m > 0 && !d_idx)) return RFX_EINVAL;
    int rc = exec_one_shard(x, "upsert");
    if (rc != RFX_OK || m == 0) return rc;
    rfx_ctx_t *c = x->ctx[0];
    const int64_t t0 = now_ns();
    if (n == 0) rc = exec_fail(x, "upsert", "index", rfx_hip_fill_i64(c, d_idx, m, INT64_MIN)); /* (a table of no rows: all nulls without a lookup) */
    else if (nkeys == 1) {
        int route = RFX_SET_ROUTE_NONE;
        rc = rfx_exec_member(x, (const int64_t *)d_table_keys[0], n, (const int64_t *)d_batch_keys[0], m, 1, d_idx, &route);
        if (rc == RFX_ESTATE && route == RFX_SET_ROUTE_UNDEFINED && undefined) *undefined = 1;
    } else {
        int collision = 0;
        rc = rfx_exec_join_index(x, d_batch_keys, d_table_keys, nkeys, m, n, d_idx, &collision);
        if (rc == RFX_ESTATE && collision && undefined) *undefined = 2;
    }
    if (rc == RFX_OK) rc = exec_fail(x, "upsert", "index", rfx_hip_ctx_sync(c));
    x->stat[RFX_XSTAT_NS_UPSERT_INDEX] += now_ns() - t0;
    return rc;
}
int rfx_exec_upsert_plan(rfx_exec_t *x, const int64_t *d_idx, int64_t m, int64_t n, int64_t *d_dest, int64_t *appended) {
    if (!x || !appended || m < 0 || n < 0) return RFX_EINVAL;
    *appended = 0;
    int rc = exec_one_shard(x, "upsert");
    if (rc != RFX_OK) return rc;
    const int64_t t0 = now_ns();
    rc = exec_fail(x, "upsert", "plan", rfx_hip_upsert_plan(x->ctx[0], d_idx, m, n, d_dest, appended)); /* (returns with the stream idle) */
    x->stat[RFX_XSTAT_NS_UPSERT_PLAN] += now_ns() - t0;
    return rc;
}
static int upsert_cols(rfx_exec_t *x, const rfx_upsert_xcol_t *cols, int ncols, const int64_t *d_dest, int64_t m, int64_t n, int64_t appended, int insert) {
    if (!x || !cols || ncols < 1 || m < 0 || n < 0 || appended < 0 || appended > m) return RFX_EINVAL;
    int rc = exec_one_shard(x, "upsert");
    if (rc != RFX_OK) {
        if (insert) snprintf(x->err, sizeof(x->err), "rfx_exec: insert over a sharded table");
        return rc;
    }
    for (int k = 0; k < ncols; k++)
        if (m > 0 && (cols[k].role == RFX_UPSERT_ABSENT) != (cols[k].d_batch == NULL)) return RFX_EINVAL;
    rfx_ctx_t *c = x->ctx[0];
    const int64_t t0 = now_ns(), stat_concats = x->stat[RFX_XSTAT_CONCATS], stat_spans = x->stat[RFX_XSTAT_CONCAT_SPANS], stat_cells = x->stat[RFX_XSTAT_CONCAT_CELLS];
    rfx_concat_col_t *cc = (rfx_concat_col_t *)calloc((size_t)ncols, sizeof(*cc));
    rfx_span_t *sp = (rfx_span_t *)calloc((size_t)ncols, sizeof(*sp));
    if (!cc || !sp) rc = RFX_ENOMEM;
    /* the table's n cells: the multi-span copy, one span per column */
    if (rc == RFX_OK && n > 0) {
        for (int k = 0; k < ncols; k++) {
            sp[k].d_ptr = cols[k].d_table;
            sp[k].cells = n;
            cc[k].spans = &sp[k];
            cc[k].nspans = 1;
            cc[k].width = cols[k].width;
            cc[k].d_out = cols[k].d_out;
        }
        rc = rfx_exec_concat_cols(x, cc, ncols);
        x->stat[RFX_XSTAT_CONCATS] = stat_concats; /* (the copy is this verb's, not a concat call) */
        x->stat[RFX_XSTAT_CONCAT_SPANS] = stat_spans;
        x->stat[RFX_XSTAT_CONCAT_CELLS] = stat_cells;
    }
    free(cc);
    free(sp);
    /* the appended cells of the columns the batch does not provide */
    for (int k = 0; k < ncols && rc == RFX_OK && appended > 0; k++)
        if (cols[k].role == RFX_UPSERT_ABSENT)
            rc = exec_fail(x, "upsert", "fill", rfx_hip_upsert_fill(c, (char *)cols[k].d_out + (size_t)n * (size_t)cols[k].width, cols[k].width, cols[k].null_bits, appended));
    /* the batch cells, RFX_MAX_COLS columns to a launch; with nothing appended the key columns have nothing to take */
    rfx_upsert_col_t pc[RFX_MAX_COLS];
    int np = 0;
    for (int k = 0; k < ncols && rc == RFX_OK && m > 0; k++) {
        if (cols[k].role != RFX_UPSERT_ABSENT && !(cols[k].role == RFX_UPSERT_KEY && appended == 0)) {
            pc[np].d_batch = cols[k].d_batch;
            pc[np].d_out = cols[k].d_out;
            pc[np].width = cols[k].width;
            pc[np].appends_only = cols[k].role == RFX_UPSERT_KEY;
            np++;
        }
        if (np == RFX_MAX_COLS || (k == ncols - 1 && np > 0)) {
            rc = exec_fail(x, "upsert", "place", rfx_hip_upsert_place(c, pc, np, d_dest, m, n, n + appended));
            np = 0;
        }
    }
    const int rs = rfx_hip_ctx_sync(c);
    if (rc == RFX_OK) rc = exec_fail(x, "upsert", "place", rs);
    x->stat[RFX_XSTAT_NS_UPSERT_PLACE] += now_ns() - t0;
    if (rc == RFX_OK && insert) x->stat[RFX_XSTAT_INSERTS]++;
    else if (rc == RFX_OK) {
        x->stat[RFX_XSTAT_UPSERTS]++;
        x->stat[RFX_XSTAT_UPSERT_MATCHED] += m - appended;
        x->stat[RFX_XSTAT_UPSERT_APPENDED] += appended;
    }
    return rc;
}
int rfx_exec_upsert_cols(rfx_exec_t *x, const rfx_upsert_xcol_t *cols, int ncols, const int64_t *d_dest, int64_t m, int64_t n, int64_t appended) {
    if (m > 0 && !d_dest) return RFX_EINVAL;
    return upsert_cols(x, cols, ncols, d_dest, m, n, appended, 0);
}
int rfx_exec_insert_cols(rfx_exec_t *x, const rfx_upsert_xcol_t *cols, int ncols, int64_t m, int64_t n) { return upsert_cols(x, cols, ncols, NULL, m, n, m, 1); }
