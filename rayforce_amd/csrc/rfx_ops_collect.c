/* rfx_ops_collect.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * The nested results of select ... by: as built-ins: row (ray_row -> aggr_row, core/compose.c:1166-1169, core/aggr.c:3118-3136) and the collected column
 * (aggr_collect, core/aggr.c:3021-3116; reached by the reference through select / update only) over a lazy MAPGROUP (val, index) pair.  The index is the
 * 7-slot group index fold_mapgroup reads (rfx_ops_folds.c): IDS gives every element's group, SHIFT looks it up in the key table through the source column,
 * a filter's row ids stand between the elements and the rows.  The device makes ONE buffer of the rows / cells in group order and the groups' offsets
 * (rfx_collect.hip through rfx_exec_collect.c); both are read back once and the host cuts the `groups` vectors out of them, a memcpy each.
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c); a malformed index -- wrong slot count, ids / filter length mismatch, an id outside
 * [0, groups), a source cell outside the key table, a filter id outside the column -- is an error of ours, as in fold_mapgroup: the device checks every id
 * before it is used as an index. */
static int g_last_collect_gpu = 0;
int rfx_last_collect_on_gpu(void) { return g_last_collect_gpu; }

/* row: the host's own ray_row; collect: no such verb in the reference -- the reason, and nothing to delegate to */
static obj_p collect_host(int want_row, obj_p x, const char *why) {
    g_last_collect_gpu = 0;
    if (want_row) return hand_off(F_ROW, NULL, 0, 1, &x, 1, why);
    char b[512];
    snprintf(b, sizeof(b), "collect: not covered by the MI355X path (%.300s) and no host function to delegate to", why);
    return fail(b);
}
/* a LIST of `groups` vectors of `type` cut out of `cells` at `offsets` (NULL: every vector empty) */
static obj_p collect_lists(int type, int64_t groups, const int64_t *offsets, const char *cells, int width) {
    obj_p out = H.vector(RFX_TYPE_LIST, groups);
    for (int64_t g = 0; g < groups; g++) {
        const int64_t n = offsets ? offsets[g + 1] - offsets[g] : 0;
        obj_p v = H.vector((int8_t)type, n);
        v->attrs = 0;
        if (n) memcpy(RFX_AS_RAW(v), cells + (size_t)offsets[g] * (size_t)width, (size_t)n * (size_t)width);
        RFX_AS_LIST(out)[g] = v;
    }
    return out;
}
/* the group of every element of an index, on the device: *d_gid (n cells).  IDS: the id column itself; SHIFT: table[source[x] - shift] with x the
 * element's row -- a source cell outside the table (or a filter id outside the source column: gathered as the null) answers -1, which the partition's
 * check refuses */
static int collect_gids(obj_p *ix, int64_t n, const void *dfl, const void **d_gid) {
    obj_p gids = ix[2], source = ix[4];
    if (ix[0]->i64 == RFX_INDEX_TYPE_IDS) return transient(gids, d_gid);
    const void *dk = NULL, *dt = NULL;
    void *g = NULL, *o = NULL;
    int rc = resident(source, 0, &dk);
    if (rc == RFX_OK) rc = transient(gids, &dt);
    if (rc == RFX_OK && dfl) {
        if ((rc = op_scratch(&g, (size_t)n * 8)) == RFX_OK) rc = rfx_hip_gather_checked(g_ctx, dk, source->len, RFX_I64, (const int64_t *)dfl, n, g);
        dk = g;
    }
    if (rc == RFX_OK) rc = op_scratch(&o, (size_t)n * 8);
    if (rc == RFX_OK) rc = rfx_hip_group_ids_table(g_ctx, (const int64_t *)dk, n, ix[3]->i64, gids->len, (const int64_t *)dt, (int64_t *)o);
    *d_gid = o;
    return rc;
}
static obj_p collect_impl(obj_p x, int want_row) {
    const char *verb = want_row ? "row" : "collect";
    char msg[160];
    rfx_host_bind();
    g_last_collect_gpu = 0;
    if (!x) { snprintf(msg, sizeof(msg), "%s: null argument", verb); return fail(msg); }
    if (x->type == RFX_TYPE_MAPFILTER) return collect_host(want_row, x, "a MAPFILTER pair");
    if (x->type != RFX_TYPE_MAPGROUP) return collect_host(want_row, x, "not a MAPGROUP pair");
    obj_p val = RFX_AS_LIST(x)[0], index = RFX_AS_LIST(x)[1];
    if (!index || index->type != RFX_TYPE_LIST || index->len != 7) { snprintf(msg, sizeof(msg), "%s: malformed group index", verb); return fail(msg); }
    obj_p *ix = RFX_AS_LIST(index);
    const int64_t itype = ix[0]->i64, groups = ix[1]->i64;
    obj_p gids = ix[2], source = ix[4], filter = ix[5];
    if (itype != RFX_INDEX_TYPE_IDS && itype != RFX_INDEX_TYPE_SHIFT) return collect_host(want_row, x, "parted / window index");
    if (!gids || gids->type != RFX_TYPE_I64 || groups < 0) return collect_host(want_row, x, "group ids");
    if (itype == RFX_INDEX_TYPE_SHIFT && !(source && source->type > 0 && col_ctype(source) == RFX_I64)) return collect_host(want_row, x, "source column");
    const int width = want_row ? 8 : (val && val->type > 0 ? cell_width(val->type) : 0);
    const int type = want_row ? RFX_TYPE_I64 : (val ? val->type : 0);
    if (!want_row) { /* (row never reads the value's cells: any value passes) */
        if (!val) return fail("collect: null value column");
        if (IS_PARTED_TYPE(val->type)) return collect_host(0, x, "a parted value column");
        if (!width) return collect_host(0, x, "value column type");
        const char *why = device_handle_why(val, 0);
        if (why) return collect_host(0, x, why);
    }
    const int filtered = filter && filter->type == RFX_TYPE_I64;
    const int64_t n = filtered ? filter->len : (itype == RFX_INDEX_TYPE_IDS ? gids->len : source->len);
    if (itype == RFX_INDEX_TYPE_IDS && gids->len != n) { snprintf(msg, sizeof(msg), "%s: group ids / filter length mismatch", verb); return fail(msg); }
    if (!want_row && !filtered && val->len != n) return fail("length");
    if (groups == 0 || n == 0) {
        g_last_collect_gpu = 1; /* (answered here: no launch) */
        return collect_lists(type, groups, NULL, NULL, width);
    }
    if (n >= 0x80000000LL || groups >= 0x80000000LL) return collect_host(want_row, x, "2^31 or more elements or groups");
    if (itype == RFX_INDEX_TYPE_SHIFT && gids->len <= 0) return collect_host(want_row, x, "empty key table"); /* (before any device scratch is taken) */
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return collect_host(want_row, x, "collect over a sharded table");
    const void *dfl = NULL, *dgid = NULL, *dv = NULL;
    void *dout = NULL;
    rfx_partition_t part;
    memset(&part, 0, sizeof(part));
    obj_p res = NULL;
    int rc = RFX_OK;
    const char *at = "filter upload";
    if (filtered) rc = transient(filter, &dfl);
    if (rc == RFX_OK) at = "group ids", rc = collect_gids(ix, n, dfl, &dgid);
    if (rc == RFX_OK && !want_row) {
        at = "column upload";
        rc = native_cells(val, width, NULL, &dv); /* (a narrow column's upload lives for this call only) */
    }
    if (rc == RFX_OK) at = "result", rc = op_scratch(&dout, (size_t)n * (size_t)width);
    if (rc == RFX_ENOMEM) return collect_host(want_row, x, "no room on the device");
    if (rc != RFX_OK) return fail_hip(at);
    rc = rfx_exec_group_partition(g_x, (const int64_t *)dgid, n, groups, &part);
    if (rc == RFX_ENOMEM) return collect_host(want_row, x, "no room on the device");
    if (rc == RFX_EINVAL) { snprintf(msg, sizeof(msg), "%s: a group id outside [0, groups), or a source cell outside the key table", verb); return fail(msg); }
    if (rc != RFX_OK) return fail(rfx_exec_last_error(g_x)[0] ? rfx_exec_last_error(g_x) : rfx_hip_last_error());
    const void *cols[1] = {dv};
    const int32_t widths[1] = {width};
    void *outs[1] = {dout};
    /* (row reads no column: a filter's ids are bounded by the value column where the pair has one) */
    const int64_t col_len = want_row ? (val && val->type > 0 ? val->len : (INT64_MAX >> 4)) : val->len;
    rc = want_row ? rfx_exec_group_collect(g_x, &part, (const int64_t *)dfl, col_len, NULL, NULL, 0, NULL, 1, (int64_t *)dout)
                  : rfx_exec_group_collect(g_x, &part, (const int64_t *)dfl, col_len, cols, widths, 1, outs, 0, NULL);
    if (rc == RFX_EINVAL) { snprintf(msg, sizeof(msg), "%s: a filter id outside the column", verb); res = fail(msg); goto done; }
    if (rc != RFX_OK) { res = fail(rfx_exec_last_error(g_x)[0] ? rfx_exec_last_error(g_x) : rfx_hip_last_error()); goto done; }
    {
        int64_t *offsets = (int64_t *)malloc((size_t)(groups + 1) * 8);
        char *cells = (char *)malloc((size_t)n * (size_t)width);
        if (!offsets || !cells) res = fail("collect: out of host memory");
        else if (rfx_hip_d2h(g_ctx, offsets, part.d_offsets, (size_t)(groups + 1) * 8) != RFX_OK || rfx_hip_d2h_pipelined(g_ctx, cells, dout, (size_t)n * (size_t)width) != RFX_OK ||
                 rfx_hip_ctx_sync(g_ctx) != RFX_OK)
            res = fail_hip("collect read-back");
        else {
            res = collect_lists(type, groups, offsets, cells, width);
            g_last_collect_gpu = 1;
        }
        free(offsets);
        free(cells);
    }
done:
    rfx_hip_ctx_sync(g_ctx); /* (the partition's blocks go back to the pool: nothing may still read them) */
    rfx_exec_group_partition_free(g_x, &part);
    return res;
}
OP1(rfx_row, collect_impl(x, 1))
OP1(rfx_collect, collect_impl(x, 0))

/* ---- the nested columns of a grouped rfx_select (sel_mappings' nest[]): a bare column and (row column) under by: one plain key ----
 * The planner's group-by has run: R holds the groups' keys in the answer's own order.  The selected rows come from rfx_exec_where (the same query without
 * its aggregates), every selected row's group is the place of its key among R's keys (the join index of the selected keys against them: distinct keys, so
 * the first match is the only one) -- the SAME order the aggregates' columns come out in -- and one partition serves every nested column: all value columns
 * and the row numbers in launches of RFX_MAX_COLS over one permutation.  SEL_GO: M->lists[] filled; SEL_OUT: *why; SEL_DONE: *res is the error. */
static int sel_nested(sel_maps_t *M, const rfx_query_t *Q, const void *dkey, const rfx_groups_t *R, obj_p *res, const char **why) {
    const int64_t groups = R->groups, nrows = Q->nrows;
    const int filtered = Q->npred > 0 || Q->d_mask != NULL;
    int rc = RFX_OK, ret = SEL_GO, want_rows = 0, ncols = 0;
    rfx_ids_t ids;
    rfx_partition_t part;
    memset(&ids, 0, sizeof(ids));
    memset(&part, 0, sizeof(part));
    int64_t m = nrows;
    const int64_t *d_rows = NULL;
    int64_t *offsets = NULL;
    if (filtered) {
        rfx_query_t W = *Q;
        W.aggs = NULL;
        W.nagg = 0;
        W.nkeys = 0;
        W.d_keys = NULL;
        W.kxbar = NULL;
        W.flags = 0;
        W.key_scope = NULL;
        if (rfx_exec_where(g_x, &W, &ids) != RFX_OK) { *res = fail(rfx_exec_last_error(g_x)); return SEL_DONE; }
        m = ids.total;
        d_rows = ids.d_ids[0];
    }
    const void *cols[SEL_NEST];
    void *outs[SEL_NEST], *drows_out = NULL, *dksel = NULL, *dgid = NULL;
    int32_t widths[SEL_NEST];
    int at[SEL_NEST]; /* nested column c reads output at[c] (-1: the row numbers) */
    if (groups > 0 && m > 0) {
        const void *lk[1] = {dkey}, *rk[1] = {R->d_keys};
        if (filtered) {
            if ((rc = op_scratch(&dksel, (size_t)m * 8)) == RFX_OK) rc = rfx_hip_gather(g_ctx, dkey, d_rows, m, dksel);
            lk[0] = dksel;
        }
        int collision = 0;
        if (rc == RFX_OK) rc = op_scratch(&dgid, (size_t)m * 8);
        if (rc == RFX_OK && (rc = rfx_exec_join_index(g_x, lk, rk, 1, m, groups, (int64_t *)dgid, &collision)) != RFX_OK && rc != RFX_ENOMEM) {
            *res = fail(rfx_exec_last_error(g_x)[0] ? rfx_exec_last_error(g_x) : rfx_hip_last_error());
            ret = SEL_DONE;
            goto done;
        }
        if (rc == RFX_OK) rc = rfx_exec_group_partition(g_x, (const int64_t *)dgid, m, groups, &part);
        for (int c = 0; c < M->nnest && rc == RFX_OK; c++) {
            if (M->nest[c].row) {
                at[c] = -1;
                if (!want_rows) rc = op_scratch(&drows_out, (size_t)m * 8);
                want_rows = 1;
                continue;
            }
            obj_p v = M->nest[c].col;
            widths[ncols] = cell_width(v->type);
            if ((rc = native_cells(v, widths[ncols], NULL, &cols[ncols])) == RFX_OK) rc = op_scratch(&outs[ncols], (size_t)m * (size_t)widths[ncols]);
            at[c] = ncols++;
        }
        if (rc == RFX_OK) rc = rfx_exec_group_collect(g_x, &part, d_rows, nrows, cols, widths, ncols, outs, want_rows, (int64_t *)drows_out);
        if (rc == RFX_ENOMEM) { *why = "nested columns: device scratch not available"; ret = SEL_OUT; goto done; }
        if (rc != RFX_OK) { *res = fail(rfx_exec_last_error(g_x)[0] ? rfx_exec_last_error(g_x) : rfx_hip_last_error()); ret = SEL_DONE; goto done; }
        offsets = (int64_t *)malloc((size_t)(groups + 1) * 8);
        if (!offsets || rfx_hip_d2h(g_ctx, offsets, part.d_offsets, (size_t)(groups + 1) * 8) != RFX_OK) { *res = fail_hip("nested columns: offsets"); ret = SEL_DONE; goto done; }
    }
    for (int c = 0; c < M->nnest; c++) {
        const int type = M->nest[c].row ? RFX_TYPE_I64 : M->nest[c].col->type, width = M->nest[c].row ? 8 : cell_width(type);
        char *cells = NULL;
        if (offsets) {
            cells = (char *)malloc((size_t)m * (size_t)width);
            if (!cells || rfx_hip_d2h_pipelined(g_ctx, cells, at[c] < 0 ? drows_out : outs[at[c]], (size_t)m * (size_t)width) != RFX_OK || rfx_hip_ctx_sync(g_ctx) != RFX_OK) {
                free(cells);
                *res = fail_hip("nested columns: read-back");
                ret = SEL_DONE;
                goto done;
            }
        }
        M->lists[c] = collect_lists(type, groups, offsets, cells, width);
        free(cells);
    }
done:
    if (ret != SEL_GO)
        for (int c = 0; c < M->nnest; c++)
            if (M->lists[c]) { H.drop(M->lists[c]); M->lists[c] = NULL; }
    free(offsets);
    if (g_ctx) rfx_hip_ctx_sync(g_ctx); /* (the blocks below go back to the pool: nothing may still read them) */
    rfx_exec_group_partition_free(g_x, &part);
    if (filtered) rfx_exec_ids_free(g_x, &ids);
    return ret;
}
