/* rfx_exec_concat.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * concat and raze (rfx_concat.hip): spans of cells laid end to end.  A span may lie anywhere in a column, so these read across whole columns and run on
 * one shard, one rank, as take and reverse do; a table's columns go RFX_MAX_COLS to a launch. */
static int concat_one_shard(rfx_exec_t *x) {
    x->err[0] = 0;
    if (x->nshards > 1 || x->has_tr) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: concat over a sharded column");
        return RFX_ELIMIT;
    }
    rfx_hip_ctx_bind_thread(x->ctx[0]);
    return RFX_OK;
}
int rfx_exec_concat_cols(rfx_exec_t *x, const rfx_concat_col_t *cols, int ncols) {
    if (!x || !cols || ncols < 1) return RFX_EINVAL;
    int rc = concat_one_shard(x);
    for (int k0 = 0; k0 < ncols && rc == RFX_OK; k0 += RFX_MAX_COLS) {
        const int nk = ncols - k0 < RFX_MAX_COLS ? ncols - k0 : RFX_MAX_COLS;
        if ((rc = rfx_hip_concat_cols(x->ctx[0], cols + k0, nk)) != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: concat: %s", rfx_hip_last_error());
    }
    if (rc == RFX_OK) {
        x->stat[RFX_XSTAT_CONCATS]++;
        for (int k = 0; k < ncols; k++) {
            x->stat[RFX_XSTAT_CONCAT_SPANS] += cols[k].nspans;
            for (int64_t s = 0; s < cols[k].nspans; s++) x->stat[RFX_XSTAT_CONCAT_CELLS] += cols[k].spans[s].cells;
        }
    }
    return rc;
}
int rfx_exec_concat(rfx_exec_t *x, const rfx_span_t *spans, int64_t nspans, int32_t kind, void *d_out) {
    const rfx_concat_col_t col = {spans, nspans, kind, d_out};
    return rfx_exec_concat_cols(x, &col, 1);
}
