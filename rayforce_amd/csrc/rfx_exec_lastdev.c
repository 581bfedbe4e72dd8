/* rfx_exec_lastdev.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * `last` under by: and `dev`, scalar and under by: (kernels: rfx_lastdev.hip).
 *
 * last under by: -- the reference's answer with ONE chunk (aggr_last_partial, core/aggr.c:851-895): per group the value at the highest selected row
 * whose cell is non-null, null when there is none.  (With several executors and 16 384 selected rows or more AGGR_COLLECT keeps the FIRST chunk
 * that has a value, core/aggr.c:909-930: an answer that depends on the thread count)  Planned as an i64 MAX: every LAST
 * aggregate reads a derived column  null(col[row]) ? null : row0 + row  made per shard, the group-by itself runs as for any MAX -- every kernel
 * family, the merge of the shards' tables -- and the result cells, which then hold rows, are replaced by the column's cells at those rows.  Two LAST
 * aggregates over different columns derive different rows.  Shards of ONE device (the gather reads every shard's piece); one process. */
static int group_by_last(rfx_exec_t *x, const rfx_query_t *q, rfx_groups_t *out) {
    const int S = x->nshards;
    x->err[0] = 0;
    memset(out, 0, sizeof(*out));
    if (world_is_multi(x)) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: last under by: over several processes is not covered");
        return RFX_ELIMIT;
    }
    for (int s = 1; s < S; s++)
        if (x->dev[s] != x->dev[0]) {
            snprintf(x->err, sizeof(x->err), "rfx_exec: last under by: runs on the shards of one device");
            return RFX_ELIMIT;
        }
    if (S > 1 && !q->cols) return RFX_EINVAL;
    const void *lcol[RFX_EXEC_MAX_AGGS];
    int32_t ltype[RFX_EXEC_MAX_AGGS];
    int which[RFX_EXEC_MAX_AGGS], nl = 0;
    for (int a = 0; a < q->nagg; a++) {
        const rfx_agg_t *g = &q->aggs[a];
        which[a] = -1;
        if (g->kind != RFX_AGG_LAST) continue;
        if (g->xop != RFX_X_NONE || g->nxnodes != 0 || (g->col_type != RFX_I64 && g->col_type != RFX_F64) || (!g->d_col && q->nrows > 0)) {
            snprintf(x->err, sizeof(x->err), "rfx_exec: aggregate %d: last takes a plain i64 / f64 column", a);
            return RFX_EINVAL;
        }
        int j = 0;
        for (; j < nl; j++)
            if (lcol[j] == g->d_col && ltype[j] == g->col_type) break;
        if (j == nl) {
            lcol[nl] = g->d_col;
            ltype[nl++] = g->col_type;
        }
        which[a] = j;
    }
    void *(*tmp)[RFX_MAX_SHARDS] = (void *(*)[RFX_MAX_SHARDS])calloc((size_t)nl, sizeof(*tmp));
    rfx_qcol_t *cols2 = (rfx_qcol_t *)calloc((size_t)(q->ncols > 0 ? q->ncols : 0) + (size_t)nl, sizeof(*cols2));
    rfx_agg_t *aggs2 = (rfx_agg_t *)calloc((size_t)q->nagg, sizeof(*aggs2));
    int rc = tmp && cols2 && aggs2 ? RFX_OK : RFX_ENOMEM, have = 0;
    int nc2 = q->cols && q->ncols > 0 ? q->ncols : 0;
    if (rc == RFX_OK && nc2) memcpy(cols2, q->cols, (size_t)nc2 * sizeof(*cols2));
    for (int j = 0; j < nl && rc == RFX_OK; j++) {
        for (int s = 0; s < S && rc == RFX_OK; s++) {
            int64_t r0, len;
            int bad = 0;
            rfx_exec_split(q->nrows, S, s, &r0, &len);
            const void *src = xlate(q, s, lcol[j], &bad);
            if (bad) { snprintf(x->err, sizeof(x->err), "rfx_exec: a column of the query has no per-shard address"); rc = RFX_EINVAL; break; }
            rfx_hip_ctx_bind_thread(x->ctx[s]);
            rc = rfx_hip_malloc(x->ctx[s], &tmp[j][s], (size_t)(len > 0 ? len : 1) * 8);
            if (rc == RFX_OK) rc = rfx_hip_last_rows(x->ctx[s], src, ltype[j], len, r0, (int64_t *)tmp[j][s]);
        }
        rfx_hip_ctx_bind_thread(x->ctx[0]);
        if (rc != RFX_OK) break;
        for (int s = 0; s < S; s++) cols2[nc2].d[s] = tmp[j][s];
        nc2++;
    }
    if (rc == RFX_OK) {
        memcpy(aggs2, q->aggs, (size_t)q->nagg * sizeof(*aggs2));
        for (int a = 0; a < q->nagg; a++)
            if (which[a] >= 0) {
                aggs2[a].kind = RFX_AGG_MAX;
                aggs2[a].d_col = tmp[which[a]][0];
                aggs2[a].col_type = RFX_I64;
            }
        rfx_query_t q2 = *q;
        q2.aggs = aggs2;
        q2.flags &= ~RFX_Q_SLICED; /* the rows are read back on shard 0: a whole result, as with FIRST */
        if (S > 1 || q->cols) {
            q2.cols = cols2;
            q2.ncols = nc2;
        }
        rc = group_by_query(x, &q2, out);
        have = rc == RFX_OK;
    }
    for (int a = 0; a < q->nagg && rc == RFX_OK && out->groups > 0; a++) {
        if (which[a] < 0) continue;
        const void *piece[RFX_MAX_SHARDS];
        int64_t r0[RFX_MAX_SHARDS], len[RFX_MAX_SHARDS];
        int bad = 0;
        for (int s = 0; s < S; s++) {
            rfx_exec_split(q->nrows, S, s, &r0[s], &len[s]);
            piece[s] = xlate(q, s, lcol[which[a]], &bad);
        }
        char *cells = (char *)out->d_results[a];
        rc = rfx_hip_last_gather(x->ctx[0], piece, r0, len, S, ltype[which[a]], (const int64_t *)cells, out->groups, cells);
        out->result_type[a] = ltype[which[a]];
        /* a small dense result is mirrored on the host (rfx_groups_t.h_block): the mirror follows */
        if (rc == RFX_OK && out->h_block && cells >= out->d_block && cells < out->d_block + out->block_bytes)
            rc = rfx_hip_d2h(x->ctx[0], (char *)out->h_block + (cells - out->d_block), cells, (size_t)out->groups * 8);
    }
    if (rc == RFX_OK && have) rc = rfx_hip_ctx_sync(x->ctx[0]);
    if (rc != RFX_OK && !x->err[0]) snprintf(x->err, sizeof(x->err), "rfx_exec: last under by: %s", rfx_hip_last_error());
    for (int j = 0; tmp && j < nl; j++)
        for (int s = 0; s < S; s++)
            if (tmp[j][s]) { /* (stream-ordered: the passes that read it are enqueued before the free) */
                rfx_hip_ctx_bind_thread(x->ctx[s]);
                rfx_hip_free(x->ctx[s], tmp[j][s]);
            }
    rfx_hip_ctx_bind_thread(x->ctx[0]);
    free(tmp);
    free(cols2);
    free(aggs2);
    if (rc != RFX_OK && have) rfx_exec_groups_free(x, out);
    return rc;
}
int rfx_exec_group_by(rfx_exec_t *x, const rfx_query_t *q, rfx_groups_t *out) {
    int nlast = 0;
    if (x && q && out && q->aggs && q->nagg > 0 && q->nagg <= RFX_EXEC_MAX_AGGS)
        for (int a = 0; a < q->nagg; a++) nlast += q->aggs[a].kind == RFX_AGG_LAST;
    if (!nlast) return group_by_query(x, q, out);
    if (q->nkeys < 1 || q->nkeys > RFX_MAX_KEYS || !q->d_keys || q->npred < 0 || q->npred > RFX_MAX_PREDS) return RFX_EINVAL;
    return group_by_last(x, q, out);
}

/* ---- dev: one shard (RFX_ELIMIT otherwise), as med ---- */
static int dev_one_shard(rfx_exec_t *x) {
    if (x->nshards > 1) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: dev runs on one shard");
        return RFX_ELIMIT;
    }
    return RFX_OK;
}
/* ray_dev's rule over the query's selection: the selected cells as a vector (where -> gather, what filter_collect makes of a MAPFILTER pair), then the two
 * passes of rfx_hip_dev; without a selection the column itself */
int rfx_exec_dev(rfx_exec_t *x, const rfx_query_t *q, const void *d_col, int32_t col_type, rfx_value_t *out) {
    if (!x || !q || !out || (q->nrows > 0 && !d_col) || q->npred < 0 || q->npred > RFX_MAX_PREDS || (q->d_mask && q->npred)) return RFX_EINVAL;
    x->err[0] = 0;
    int rc = dev_one_shard(x);
    if (rc != RFX_OK) return rc;
    if (col_type != RFX_I64 && col_type != RFX_F64) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: dev of an i64 / f64 column only");
        return RFX_EINVAL;
    }
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    void *ids = NULL, *vals = NULL;
    int64_t n = q->nrows;
    if ((q->npred || q->d_mask) && q->nrows > 0) {
        rc = rfx_hip_where_begin(c, q->preds, q->npred, q->npred ? q->logic : RFX_AND, q->d_mask, q->nrows, &n);
        if (rc == RFX_OK && n > 0) {
            rc = rfx_hip_malloc(c, &ids, (size_t)n * 8);
            if (rc == RFX_OK) rc = rfx_hip_malloc(c, &vals, (size_t)n * 8);
            if (rc == RFX_OK) rc = rfx_hip_where_emit(c, 0, (int64_t *)ids);
            if (rc == RFX_OK) rc = rfx_hip_gather(c, d_col, (const int64_t *)ids, n, vals);
            d_col = vals;
        }
    }
    if (rc == RFX_OK) rc = rfx_hip_dev(c, d_col, col_type, n, out);
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: dev: %s", rfx_hip_last_error());
    if (ids) rfx_hip_free(c, ids);
    if (vals) rfx_hip_free(c, vals);
    return rc;
}
/* aggr_dev's rule (core/aggr.c:2250-2350,2864-2929): per group sum (f64)x, sum (f64)x * (f64)x and the non-null count, kept by the grouped kernels as
 * hidden aggregates of the SAME query -- AVG x, AVG of the derived squares, SUM of the derived 0 / 1 column: the same keys, the same selection, the same
 * first-occurrence order as `g` -- then one finalise launch.  Scratch 16 B per row. */
int rfx_exec_group_dev(rfx_exec_t *x, const rfx_query_t *q, const rfx_groups_t *g, const void *d_col, int32_t col_type, void *d_out) {
    if (!x || !q || !g || (g->groups > 0 && !d_out) || (q->nrows > 0 && !d_col)) return RFX_EINVAL;
    x->err[0] = 0;
    int rc = dev_one_shard(x);
    if (rc != RFX_OK) return rc;
    if (col_type != RFX_I64 && col_type != RFX_F64) return RFX_EINVAL;
    if (g->groups == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    void *sq = NULL, *nn = NULL;
    rc = rfx_hip_malloc(c, &sq, (size_t)(q->nrows ? q->nrows : 1) * 8);
    if (rc == RFX_OK) rc = rfx_hip_malloc(c, &nn, (size_t)(q->nrows ? q->nrows : 1) * 8);
    if (rc == RFX_OK) rc = rfx_hip_dev_derive(c, d_col, col_type, q->nrows, (double *)sq, (int64_t *)nn);
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: grouped dev: %s", rfx_hip_last_error());
    rfx_groups_t *R = rc == RFX_OK ? (rfx_groups_t *)calloc(1, sizeof(*R)) : NULL;
    if (rc == RFX_OK && !R) rc = RFX_ENOMEM;
    if (rc == RFX_OK) {
        rfx_agg_t a3[3];
        memset(a3, 0, sizeof(a3));
        a3[0].kind = RFX_AGG_AVG;
        a3[0].d_col = d_col;
        a3[0].col_type = col_type;
        a3[1].kind = RFX_AGG_AVG;
        a3[1].d_col = sq;
        a3[1].col_type = RFX_F64;
        a3[2].kind = RFX_AGG_SUM;
        a3[2].d_col = nn;
        a3[2].col_type = RFX_I64;
        rfx_query_t q2 = *q;
        q2.aggs = a3;
        q2.nagg = 3;
        q2.flags &= ~(RFX_Q_SLICED | RFX_Q_WANT_FIRST | RFX_Q_PROBE_FIRST);
        rc = group_by_query(x, &q2, R);
        if (rc == RFX_OK) {
            if (R->groups != g->groups) {
                snprintf(x->err, sizeof(x->err), "rfx_exec: grouped dev: the groups are not those of the query's own result");
                rc = RFX_ESTATE;
            }
            if (rc == RFX_OK) rc = rfx_hip_dev_finalise(c, (const double *)R->d_results[0], (const double *)R->d_results[1], (const int64_t *)R->d_results[2], g->groups, (double *)d_out);
            if (rc == RFX_OK) rc = rfx_hip_ctx_sync(c);
            if (rc != RFX_OK && !x->err[0]) snprintf(x->err, sizeof(x->err), "rfx_exec: grouped dev: %s", rfx_hip_last_error());
            rfx_exec_groups_free(x, R);
        }
    }
    free(R);
    if (sq || nn) rfx_hip_ctx_sync(c);
    if (sq) rfx_hip_free(c, sq);
    if (nn) rfx_hip_free(c, nn);
    return rc;
}
