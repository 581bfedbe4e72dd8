/* rfx_ops_rows.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * The row verbs as built-ins of their own: filter (ray_filter, core/items.c:338-396), take (ray_take, core/items.c:398-734), reverse (ray_reverse,
 * core/compose.c:144-202) on the device (rfx_rows.hip through rfx_exec_rows.c).
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c): a shape the device does not take is the
 * host's own verb when a host is bound, else an error object naming the reason (also in rfx_ops_last_error()).  Every result is fresh host vectors with
 * the reference's cells, type codes and attributes (a table: a fresh table of them over a clone of the names). */
static int g_last_rows_gpu = 0;
int rfx_last_rows_on_gpu(void) { return g_last_rows_gpu; }

static obj_p rows_host(int f, obj_p x, obj_p y, const char *why) {
    g_last_rows_gpu = 0;
    return hand_off_xy(f, NULL, x, y, why);
}
/* the cell kind of a row type (bytes of a result cell), 0: not a row type */
static int rows_kind(int type) {
    switch (type) {
        case RFX_TYPE_I64: case RFX_TYPE_SYMBOL: case RFX_TYPE_TIMESTAMP: case RFX_TYPE_F64: return RFX_ROWS_8;
        case RFX_TYPE_I32: case RFX_TYPE_DATE: case RFX_TYPE_TIME: return RFX_ROWS_4W; /* (the resident copy is the widened image) */
        case RFX_TYPE_B8: return RFX_ROWS_1;
        default: return 0;
    }
}
/* x as a list of columns: a vector of a row type is one column, a table its columns.  NULL: fine; else why the device does not take it */
typedef struct {
    obj_p names; /* a table's names (NULL: x is a vector) */
    obj_p *cols;
    obj_p one[1];
    int ncols;
    int64_t len;
} rows_src_t;
static const char *rows_source(obj_p x, rows_src_t *S) {
    memset(S, 0, sizeof(*S));
    if (x->type == RFX_TYPE_TABLE) {
        if (is_parted_table(x)) return "a parted table";
        obj_p cols = RFX_AS_LIST(x)[1];
        if (cols->type != RFX_TYPE_LIST || cols->len < 1) return "a table with no columns";
        S->names = RFX_AS_LIST(x)[0];
        S->cols = RFX_AS_LIST(cols);
        S->ncols = (int)cols->len;
    } else {
        S->one[0] = x;
        S->cols = S->one;
        S->ncols = 1;
    }
    for (int k = 0; k < S->ncols; k++) {
        obj_p c = S->cols[k];
        if (!c || c->type <= 0 || !rows_kind(c->type)) return S->names ? "a column that is not a vector of a row type" : "not a vector of a row type";
        const char *why = device_handle_why(c, 1);
        if (why) return why;
        if (k && c->len != S->len) return "columns of unequal length";
        S->len = c->len;
    }
    return NULL;
}
/* the answer's shell: per column a fresh vector of `len` cells (*vecs lists them; `slot` holds a lone vector's entry) -> the vector itself or the table */
static obj_p rows_result(const rows_src_t *S, int64_t len, obj_p *slot, obj_p **vecs) {
    if (!S->names) {
        *slot = H.vector(S->cols[0]->type, len);
        *vecs = slot;
        return *slot;
    }
    obj_p rv = H.vector(RFX_TYPE_LIST, S->ncols);
    for (int k = 0; k < S->ncols; k++) RFX_AS_LIST(rv)[k] = H.vector(S->cols[k]->type, len);
    *vecs = RFX_AS_LIST(rv);
    return H.table(H.clone(S->names), rv);
}
static size_t rows_align(size_t b) { return (b + 255) & ~(size_t)255; }

/* ---- filter ---- */
static obj_p filter_impl(obj_p x, obj_p mask) {
    rfx_host_bind();
    if (!x || !mask) return fail("filter: null argument");
    g_last_rows_gpu = 0;
    rows_src_t S;
    const char *why = rows_source(x, &S);
    if (why) return rows_host(F_FILTER, x, mask, why);
    if (mask->type != RFX_TYPE_B8) return rows_host(F_FILTER, x, mask, "a mask that is not a B8 vector");
    if (mask->len != S.len) return rows_host(F_FILTER, x, mask, "length"); /* (err_length is the host's to raise) */
    obj_p slot = NULL, *vecs = NULL;
    if (S.len == 0) { /* nothing to select from: no launch */
        g_last_rows_gpu = 1;
        return rows_result(&S, 0, &slot, &vecs);
    }
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    rfx_qcol_t *pieces = (rfx_qcol_t *)calloc((size_t)S.ncols, sizeof(rfx_qcol_t));
    int32_t *kinds = (int32_t *)calloc((size_t)S.ncols, sizeof(int32_t));
    if (!pieces || !kinds) {
        free(pieces);
        free(kinds);
        return fail("filter: out of host memory");
    }
    const void *dm = NULL;
    int rc = mask->mmod == RFX_MMOD_DEVICE ? resident(mask, 0, &dm) : (g_nshards > 1 ? transient_sharded(mask, &dm) : transient(mask, &dm));
    for (int k = 0; k < S.ncols && rc == RFX_OK; k++) {
        rc = col_pieces(S.cols[k], (const void **)pieces[k].d);
        if (rc == COL_PIECE_MISSING) rc = RFX_ELIMIT;
        kinds[k] = rows_kind(S.cols[k]->type);
    }
    rfx_rows_t R;
    memset(&R, 0, sizeof(R));
    int ran = 0;
    if (rc == RFX_OK) {
        rfx_query_t Q;
        memset(&Q, 0, sizeof(Q));
        Q.d_mask = (const int8_t *)dm;
        Q.logic = RFX_AND;
        Q.nrows = S.len;
        Q.cols = g_qcols;
        Q.ncols = g_nqcols;
        rc = rfx_exec_filter(g_x, &Q, pieces, kinds, S.ncols, &R);
        ran = 1;
    }
    qtmp_release();
    free(pieces);
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) {
        free(kinds);
        return rows_host(F_FILTER, x, mask, rc == RFX_ENOMEM ? "device memory" : (ran ? "a limit of the planner" : (g_nshards > 1 ? "more columns than a sharded call names" : "the call's device scratch list is full")));
    }
    if (rc != RFX_OK) {
        free(kinds);
        return ran && rfx_exec_last_error(g_x)[0] ? fail(rfx_exec_last_error(g_x)) : fail_hip("filter");
    }
    obj_p out = rows_result(&S, R.total, &slot, &vecs);
    for (int k = 0; k < S.ncols && rc == RFX_OK; k++) {
        size_t at = 0;
        for (int s = 0; s < R.nshards && rc == RFX_OK; s++) {
            if (!R.count[s]) continue;
            const size_t bytes = (size_t)R.count[s] * (size_t)kinds[k];
            if (g_nshards > 1) rfx_hip_ctx_bind_thread(g_ctxs[s]);
            rc = rfx_hip_d2h(g_ctxs[s], (char *)RFX_AS_RAW(vecs[k]) + at, rfx_exec_rows_piece(&R, s, k), bytes);
            at += bytes;
        }
    }
    if (g_nshards > 1) rfx_hip_ctx_bind_thread(g_ctx);
    rfx_exec_rows_free(g_x, &R);
    free(kinds);
    if (rc != RFX_OK) {
        H.drop(out);
        return fail_hip("filter result");
    }
    g_last_rows_gpu = 1;
    return out;
}

/* ---- take ---- */
static obj_p take_impl(obj_p from, obj_p count) {
    rfx_host_bind();
    if (!from || !count) return fail("take: null argument");
    g_last_rows_gpu = 0;
    int is_range = 0, neg = 0;
    int64_t start = 0, m = 0, cnt = 0;
    if (count->type == RFX_TYPE_I64 && count->len == 2 && count->mmod != RFX_MMOD_DEVICE) { /* [start amount] (core/items.c:405-411) */
        is_range = 1;
        start = RFX_AS_I64(count)[0];
        m = RFX_AS_I64(count)[1];
        if (m < 0) return rows_host(F_TAKE, from, count, "a negative range amount"); /* (err_length is the host's to raise) */
        int64_t end;
        if (__builtin_add_overflow(start, m, &end)) return rows_host(F_TAKE, from, count, "start + amount does not fit 63 bits");
    } else {
        switch (count->type) { /* (core/items.c:414-429) */
            case -RFX_TYPE_I64: cnt = count->i64; break;
            case -RFX_TYPE_I32: cnt = count->i32; break;
            case -RFX_TYPE_I16: cnt = count->i16; break;
            default: return rows_host(F_TAKE, from, count, "count type");
        }
        if (cnt == INT64_MIN) return rows_host(F_TAKE, from, count, "a count of INT64_MIN");
        neg = cnt < 0;
        m = neg ? -cnt : cnt;
    }
    if (from->type < 0) { /* an atom: m cells of it, whichever form the count has (core/items.c:456-462,514-520,546-553) */
        const int kind = rows_kind(-from->type);
        if (!kind) return rows_host(F_TAKE, from, count, "not an atom of a row type");
        if (m > (INT64_MAX >> 4)) return rows_host(F_TAKE, from, count, "device memory");
        obj_p out;
        if (m == 0) {
            g_last_rows_gpu = 1;
            return H.vector((int8_t)-from->type, 0);
        }
        if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
        if (g_nshards > 1) return rows_host(F_TAKE, from, count, "take over a sharded table");
        void *d = NULL;
        int at = OP_AT_SCRATCH, rc = op_scratch(&d, (size_t)m * (size_t)kind);
        if (rc == RFX_OK) at = OP_AT_PLANNER, rc = rfx_exec_take_atom(g_x, kind, atom_cell_bits(from, kind), m, d); /* (a cell kind is its bytes) */
        if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return rows_host(F_TAKE, from, count, op_limit_why(rc, at, "take over a sharded table"));
        if (rc != RFX_OK) return fail_hip("take");
        out = H.vector((int8_t)-from->type, m);
        if (rfx_hip_d2h(g_ctx, RFX_AS_RAW(out), d, (size_t)m * (size_t)kind) != RFX_OK) {
            H.drop(out);
            return fail_hip("take result");
        }
        g_last_rows_gpu = 1;
        return out;
    }
    rows_src_t S;
    const char *why = rows_source(from, &S);
    if (why) return rows_host(F_TAKE, from, count, why);
    const int64_t l = S.len;
    int64_t j0 = 0;
    if (is_range) { /* the clamps of core/items.c:437-445 */
        if (start < 0) start = l + start;
        if (start < 0) start = 0;
        if (start > l) start = l;
        int64_t end;
        if (__builtin_add_overflow(start, m, &end)) return rows_host(F_TAKE, from, count, "start + amount does not fit 63 bits");
        if (end > l) m = l - start;
        j0 = m ? start : 0;
    } else {
        if (l == 0) return rows_host(F_TAKE, from, count, S.names ? "take from an empty table" : "take from an empty vector"); /* (the reference divides by l) */
        j0 = neg ? (l - m % l) % l : 0; /* (l - m % l) * f, taken mod l as every index is */
    }
    obj_p slot = NULL, *vecs = NULL;
    if (m == 0) {
        g_last_rows_gpu = 1;
        return rows_result(&S, 0, &slot, &vecs);
    }
    if (m > (INT64_MAX >> 4)) return rows_host(F_TAKE, from, count, "device memory");
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return rows_host(F_TAKE, from, count, "take over a sharded table");
    const void **src = (const void **)calloc((size_t)S.ncols, sizeof(void *));
    void **dst = (void **)calloc((size_t)S.ncols, sizeof(void *));
    int32_t *kinds = (int32_t *)calloc((size_t)S.ncols, sizeof(int32_t));
    void *block = NULL;
    int rc = (src && dst && kinds) ? RFX_OK : RFX_ENOMEM;
    size_t total = 0;
    for (int k = 0; k < S.ncols && rc == RFX_OK; k++) {
        kinds[k] = rows_kind(S.cols[k]->type);
        rc = resident(S.cols[k], 0, &src[k]);
        dst[k] = (void *)total; /* (offsets first: the block is not there yet) */
        total += rows_align((size_t)m * (size_t)kinds[k]);
    }
    const int uploaded = rc == RFX_OK;
    int at = OP_AT_UPLOAD;
    if (rc == RFX_OK) at = OP_AT_SCRATCH, rc = rfx_hip_malloc(g_ctx, &block, total);
    if (rc == RFX_OK) {
        for (int k = 0; k < S.ncols; k++) dst[k] = (char *)block + (size_t)dst[k];
        at = OP_AT_PLANNER;
        rc = rfx_exec_take(g_x, src, kinds, S.ncols, l, j0, m, dst);
    }
    obj_p out = NULL;
    if (rc == RFX_OK) {
        out = rows_result(&S, m, &slot, &vecs);
        for (int k = 0; k < S.ncols && rc == RFX_OK; k++) rc = rfx_hip_d2h(g_ctx, RFX_AS_RAW(vecs[k]), dst[k], (size_t)m * (size_t)kinds[k]);
    }
    if (block) {
        rfx_hip_ctx_sync(g_ctx);
        rfx_hip_free(g_ctx, block);
    }
    free(src);
    free(dst);
    free(kinds);
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) {
        if (out) H.drop(out);
        return rows_host(F_TAKE, from, count, op_limit_why(rc, at, "take over a sharded table"));
    }
    if (rc != RFX_OK) {
        if (out) H.drop(out);
        return fail_hip(uploaded ? "take" : "column upload");
    }
    g_last_rows_gpu = 1;
    return out;
}

/* ---- reverse ---- */
static obj_p reverse_impl(obj_p x) {
    rfx_host_bind();
    if (!x) return fail("reverse: null argument");
    g_last_rows_gpu = 0;
    if (x->type == RFX_TYPE_TABLE) return rows_host(F_REVERSE, x, NULL, "a table");
    const int kind = x->type > 0 ? rows_kind(x->type) : 0;
    if (!kind) return rows_host(F_REVERSE, x, NULL, "not a vector of a row type");
    const char *why = device_handle_why(x, 1);
    if (why) return rows_host(F_REVERSE, x, NULL, why);
    const int64_t l = x->len;
    const uint8_t attrs = (uint8_t)((x->attrs & ~(ATTR_ASC_ | ATTR_DESC_)) | ((x->attrs & ATTR_ASC_) ? ATTR_DESC_ : 0) | ((x->attrs & ATTR_DESC_) ? ATTR_ASC_ : 0));
    if (l == 0) {
        obj_p o = H.vector(x->type, 0);
        o->attrs = attrs;
        g_last_rows_gpu = 1;
        return o;
    }
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return rows_host(F_REVERSE, x, NULL, "reverse over a sharded table");
    const void *dv = NULL;
    void *d = NULL;
    int at = OP_AT_UPLOAD, rc = resident(x, 0, &dv);
    if (rc == RFX_OK) at = OP_AT_SCRATCH, rc = op_scratch(&d, (size_t)l * (size_t)kind);
    if (rc == RFX_OK) at = OP_AT_PLANNER, rc = rfx_exec_reverse(g_x, dv, kind, l, d);
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return rows_host(F_REVERSE, x, NULL, op_limit_why(rc, at, "reverse over a sharded table"));
    if (rc != RFX_OK && at == OP_AT_UPLOAD) return fail_hip("column upload");
    if (rc != RFX_OK) return fail_hip("reverse");
    obj_p out = H.vector(x->type, l);
    if (rfx_hip_d2h(g_ctx, RFX_AS_RAW(out), d, (size_t)l * (size_t)kind) != RFX_OK) {
        H.drop(out);
        return fail_hip("reverse result");
    }
    out->attrs = attrs;
    g_last_rows_gpu = 1;
    return out;
}

OP2(rfx_filter, filter_impl(x, y))
OP2(rfx_take, take_impl(x, y))
OP1(rfx_reverse, reverse_impl(x))
