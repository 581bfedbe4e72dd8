/* rfx_exec_rows.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The row verbs (rfx_rows.hip): filter runs over every shard's rows as rfx_exec_where does -- the selection (a byte mask or the fused predicate tree) goes
 * straight into the ordered compaction of the columns, no mask and no ids in between, and the shards' pieces in shard order are the answer; take and
 * reverse read across the whole column and run on one shard only, as the sort does. */
#define ROWS_ALIGN 256 /* every column's piece starts a fresh 256-byte line of its shard's block */
typedef struct {
    rfx_exec_t *x;
    const rfx_query_t *q;
    shard_t *sh;
    const rfx_qcol_t *pieces;
    const int32_t *kinds;
    int ncols, form;
    rfx_rows_t *out;
} rows_t;
static int ph_filter(void *arg, int s) {
    rows_t *W = (rows_t *)arg;
    shard_t *h = &W->sh[s];
    rfx_ctx_t *c = W->x->ctx[s];
    rfx_rows_t *o = W->out;
    h->count = 0;
    if (h->nrows == 0) return RFX_OK; /* (a shard without rows; an empty table's mask has no address at all) */
    int rc = h->mask ? rfx_hip_where_begin(c, NULL, 0, RFX_AND, h->mask, h->nrows, &h->count)
                     : rfx_hip_where_begin(c, h->preds, W->q->npred, W->q->logic, NULL, h->nrows, &h->count);
    if (rc != RFX_OK || h->count == 0) return rc;
    size_t at = 0;
    for (int k = 0; k < W->ncols; k++) {
        o->col_off[(size_t)s * (size_t)W->ncols + (size_t)k] = at;
        at += ((size_t)h->count * (size_t)W->kinds[k] + ROWS_ALIGN - 1) & ~(size_t)(ROWS_ALIGN - 1);
    }
    void *blk = NULL;
    if ((rc = rfx_hip_malloc(c, &blk, at)) != RFX_OK) return rc;
    o->d_block[s] = blk;
    for (int k0 = 0; k0 < W->ncols && rc == RFX_OK; k0 += RFX_MAX_KEYS) { /* a wide table: several launches over the SAME bitmap and scanned offsets */
        const int nk = W->ncols - k0 < RFX_MAX_KEYS ? W->ncols - k0 : RFX_MAX_KEYS;
        const void *src[RFX_MAX_KEYS];
        void *dst[RFX_MAX_KEYS];
        for (int k = 0; k < nk; k++) {
            src[k] = W->pieces[k0 + k].d[s];
            dst[k] = (char *)blk + o->col_off[(size_t)s * (size_t)W->ncols + (size_t)(k0 + k)];
        }
        rc = rfx_hip_rows_compact(c, src, W->kinds + k0, nk, dst, W->form);
    }
    if (rc == RFX_OK && W->x->nshards > 1) rc = rfx_hip_ctx_sync(c); /* (the caller reads the pieces from shard 0's stream) */
    return rc;
}
int rfx_exec_filter(rfx_exec_t *x, const rfx_query_t *q, const rfx_qcol_t *pieces, const int32_t *kinds, int ncols, rfx_rows_t *out) {
    if (!x || !q || !out || !pieces || !kinds || ncols < 1 || q->npred < 0 || q->npred > RFX_MAX_PREDS || q->nrows < 0) return RFX_EINVAL;
    if ((q->d_mask != NULL) == (q->npred > 0) && q->nrows > 0) return RFX_EINVAL; /* either a mask or predicates */
    const int S = x->nshards;
    for (int k = 0; k < ncols; k++)
        if (kinds[k] != RFX_ROWS_8 && kinds[k] != RFX_ROWS_4W && kinds[k] != RFX_ROWS_1) return RFX_EINVAL;
    rfx_hip_ctx_bind_thread(x->ctx[0]);
    x->stat[RFX_XSTAT_QUERIES]++;
    x->err[0] = 0;
    memset(out, 0, sizeof(*out));
    out->nshards = S;
    out->ncols = ncols;
    out->col_off = (size_t *)calloc((size_t)S * (size_t)ncols, sizeof(size_t));
    shard_t *sh = (shard_t *)calloc((size_t)S, sizeof(shard_t));
    if (!sh || !out->col_off) {
        free(sh);
        free(out->col_off);
        memset(out, 0, sizeof(*out));
        return RFX_ENOMEM;
    }
    int rc = RFX_OK;
    for (int s = 0; s < S && rc == RFX_OK; s++) {
        rc = shard_view(q, S, s, 0, 0, &sh[s]);
        rfx_exec_split(q->nrows, S, s, &sh[s].row0, &sh[s].nrows);
        for (int k = 0; k < ncols && rc == RFX_OK; k++)
            if (sh[s].nrows > 0 && !pieces[k].d[s]) rc = RFX_EINVAL;
    }
    if (rc != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: a column of the query has no per-shard address");
    rows_t W = {x, q, sh, pieces, kinds, ncols, (q->flags & RFX_Q_ROWS_RING) ? RFX_ROWS_RING : ((q->flags & RFX_Q_ROWS_DIRECT) ? RFX_ROWS_DIRECT : RFX_ROWS_FORM_DEFAULT), out};
    if (rc == RFX_OK) rc = run_shards(x, ph_filter, &W);
    if (S > 1) rfx_hip_ctx_bind_thread(x->ctx[0]);
    for (int s = 0; s < S; s++) {
        out->count[s] = sh[s].count;
        out->total += sh[s].count;
        sh_release(x, &sh[s], s);
    }
    free(sh);
    if (rc != RFX_OK) {
        rfx_exec_rows_free(x, out);
        return rc;
    }
    x->stat[RFX_XSTAT_ROWS_FILTERS]++;
    x->stat[RFX_XSTAT_ROWS_IN] += q->nrows;
    x->stat[RFX_XSTAT_ROWS_OUT] += out->total;
    return RFX_OK;
}
void *rfx_exec_rows_piece(const rfx_rows_t *r, int shard, int col) {
    if (!r || !r->col_off || shard < 0 || shard >= r->nshards || col < 0 || col >= r->ncols || !r->d_block[shard]) return NULL;
    return (char *)r->d_block[shard] + r->col_off[(size_t)shard * (size_t)r->ncols + (size_t)col];
}
void rfx_exec_rows_free(rfx_exec_t *x, rfx_rows_t *r) {
    if (!x || !r) return;
    for (int s = 0; s < r->nshards && s < x->nshards; s++)
        if (r->d_block[s]) rfx_hip_free(x->ctx[s], r->d_block[s]);
    free(r->col_off);
    memset(r, 0, sizeof(*r));
}

int rfx_exec_take(rfx_exec_t *x, const void *const *d_cols, const int32_t *kinds, int ncols, int64_t l, int64_t j0, int64_t m, void *const *d_outs) {
    if (!x || !d_cols || !kinds || !d_outs || ncols < 1 || l < 0 || m < 0) return RFX_EINVAL;
    int rc = exec_one_shard(x, "take");
    for (int k = 0; k < ncols && rc == RFX_OK; k++)
        if ((rc = rfx_hip_rows_take(x->ctx[0], d_cols[k], kinds[k], l, j0, m, d_outs[k])) != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: take: %s", rfx_hip_last_error());
    if (rc == RFX_OK) {
        x->stat[RFX_XSTAT_ROWS_TAKES]++;
        x->stat[RFX_XSTAT_ROWS_IN] += l;
        x->stat[RFX_XSTAT_ROWS_OUT] += m;
    }
    return rc;
}
int rfx_exec_take_atom(rfx_exec_t *x, int32_t kind, uint64_t bits, int64_t m, void *d_out) {
    if (!x || m < 0) return RFX_EINVAL;
    int rc = exec_one_shard(x, "take");
    if (rc == RFX_OK && (rc = rfx_hip_rows_fill(x->ctx[0], kind, bits, m, d_out)) != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: take: %s", rfx_hip_last_error());
    if (rc == RFX_OK) {
        x->stat[RFX_XSTAT_ROWS_TAKES]++;
        x->stat[RFX_XSTAT_ROWS_IN] += 1;
        x->stat[RFX_XSTAT_ROWS_OUT] += m;
    }
    return rc;
}
int rfx_exec_reverse(rfx_exec_t *x, const void *d_col, int32_t kind, int64_t l, void *d_out) {
    if (!x || l < 0) return RFX_EINVAL;
    int rc = exec_one_shard(x, "reverse");
    if (rc == RFX_OK && (rc = rfx_hip_rows_reverse(x->ctx[0], d_col, kind, l, d_out)) != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: reverse: %s", rfx_hip_last_error());
    if (rc == RFX_OK) {
        x->stat[RFX_XSTAT_ROWS_REVERSES]++;
        x->stat[RFX_XSTAT_ROWS_IN] += l;
        x->stat[RFX_XSTAT_ROWS_OUT] += l;
    }
    return rc;
}
#undef ROWS_ALIGN
