/* rfx_ops_concat.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * The write side as built-ins of their own: concat (ray_concat, core/compose.c:465-823) and raze (ray_raze, core/compose.c:1096-1164) of plain vectors and
 * of tables of them on the device (rfx_concat.hip through rfx_exec_concat.c): every result column is ONE multi-span copy, a table's columns
 * RFX_MAX_COLS to a launch.
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c): a shape the device does not take is the host's own verb when a host is bound, else an
 * error object naming the reason (also in rfx_ops_last_error()).  Every result is fresh host vectors of the operands' type, attribute byte 0, filled by
 * read-back (a table: a fresh table of them over a clone of x's names).
 * The result inherits residency (res_col_t, rfx_ops_cols.c). */
static int g_last_concat_gpu = 0;
int rfx_last_concat_on_gpu(void) { return g_last_concat_gpu; }

static obj_p concat_host(int f, obj_p x, obj_p y, const char *why) {
    g_last_concat_gpu = 0;
    return hand_off_xy(f, NULL, x, y, why);
}
/* one result column: `nparts` operands of one cell type laid end to end, each a vector of that type or (concat only) an atom of it */
typedef struct {
    int type;
    int64_t nparts;
    obj_p *parts;
} concat_col_t;
/* a part's cells on the device: a device handle's address, the resident copy (8-byte cells and B8: uploaded if need be), or -- staged -- the next cells of
 * the column's staging block `stage` (one block of the call's scratch per column, however many parts) */
static int concat_span(obj_p p, int width, char **stage, rfx_span_t *sp) {
    memset(sp, 0, sizeof(*sp));
    if (p->type < 0) {
        sp->cells = 1;
        sp->bits = atom_cell_bits(p, width);
        return RFX_OK;
    }
    sp->cells = p->len;
    return p->len ? native_cells(p, width, stage, &sp->d_ptr) : RFX_OK;
}
/* the columns' copies: outs[k] receives column k's fresh vector.  RFX_OK, or the failing step's code with *at saying which step (op_limit_why) */
static int concat_run(const concat_col_t *C, int ncols, obj_p *outs, int *at) {
    int rc = RFX_OK, any = 0;
    *at = OP_AT_PLANNER;
    for (int k = 0; k < ncols; k++) {
        int64_t total = 0;
        for (int64_t i = 0; i < C[k].nparts; i++)
            if (__builtin_add_overflow(total, C[k].parts[i]->type < 0 ? 1 : C[k].parts[i]->len, &total) || total > (INT64_MAX >> 5)) return RFX_ENOMEM;
        outs[k] = H.vector((int8_t)C[k].type, total);
        outs[k]->attrs = 0;
        any |= total > 0;
    }
    if (!any) return RFX_OK; /* nothing to copy: no launch */
    if (ensure_ctx() != RFX_OK) return RFX_EHIP;
    if (g_nshards > 1) return RFX_ELIMIT; /* (the planner would say so too: before anything is uploaded) */
    rfx_concat_col_t *cols = (rfx_concat_col_t *)calloc((size_t)ncols, sizeof(*cols));
    res_col_t *R = (res_col_t *)calloc((size_t)ncols, sizeof(*R));
    if (!cols || !R) {
        free(cols);
        free(R);
        return RFX_ENOMEM;
    }
    const int adopt = res_col_adopt_on();
    for (int k = 0; k < ncols && rc == RFX_OK; k++) {
        const int w = cell_width(C[k].type);
        rfx_span_t *sp = (rfx_span_t *)calloc((size_t)C[k].nparts, sizeof(*sp));
        cols[k].spans = sp;
        cols[k].nspans = C[k].nparts;
        cols[k].width = w;
        if (!sp) rc = RFX_ENOMEM;
        size_t staged = 0;
        for (int64_t i = 0; i < C[k].nparts; i++)
            if (cells_staged(C[k].parts[i])) staged += (size_t)C[k].parts[i]->len * (size_t)w;
        void *stage = NULL;
        *at = OP_AT_SCRATCH;
        if (rc == RFX_OK && staged) rc = op_scratch(&stage, staged);
        char *next = (char *)stage;
        if (rc == RFX_OK) *at = OP_AT_UPLOAD;
        for (int64_t i = 0; i < C[k].nparts && rc == RFX_OK; i++) rc = concat_span(C[k].parts[i], w, &next, &sp[i]);
        if (rc == RFX_OK && outs[k]->len) {
            *at = OP_AT_SCRATCH;
            rc = res_col_alloc(&R[k], outs[k], w, adopt);
            cols[k].d_out = R[k].d;
        }
    }
    if (rc == RFX_OK) *at = OP_AT_PLANNER, rc = rfx_exec_concat_cols(g_x, cols, ncols);
    if (rc == RFX_OK && (rc = res_cols_read(R, ncols)) != RFX_OK) *at = -1;
    res_cols_finish(R, ncols, rc, adopt);
    for (int k = 0; k < ncols; k++) free((void *)cols[k].spans);
    free(cols);
    free(R);
    return rc;
}
/* concat_run's outcome as the verb's answer: `res` (the vector, or the table over the columns) or the hand-off / the failure, the fresh vectors dropped */
static obj_p concat_finish(int f, obj_p x, obj_p y, int rc, int at, obj_p res) {
    if (rc == RFX_OK) {
        g_last_concat_gpu = 1;
        return res;
    }
    if (res) H.drop(res);
    obj_p a[2] = {x, y};
    return op_outcome(f, a, 2, rc, at, "concat over a sharded column", f == F_RAZE ? "raze" : "concat");
}

/* ---- concat ---- */
static obj_p concat_impl(obj_p x, obj_p y) {
    rfx_host_bind();
    if (!x || !y) return fail("concat: null argument");
    g_last_concat_gpu = 0;
    int rc, at;
    if (x->type == RFX_TYPE_TABLE && y->type == RFX_TYPE_TABLE) {
        if (is_parted_table(x) || is_parted_table(y)) return concat_host(F_CONCAT, x, y, "a parted table");
        obj_p xn = RFX_AS_LIST(x)[0], yn = RFX_AS_LIST(y)[0], xc = RFX_AS_LIST(x)[1], yc = RFX_AS_LIST(y)[1];
        if (xc->type != RFX_TYPE_LIST || yc->type != RFX_TYPE_LIST || xc->len < 1) return concat_host(F_CONCAT, x, y, "a table with no columns");
        if (xn->type != RFX_TYPE_SYMBOL || yn->type != RFX_TYPE_SYMBOL || xn->len != xc->len || yn->len != yc->len || xn->len != yn->len)
            return concat_host(F_CONCAT, x, y, "tables whose name sets differ"); /* (err_value is the host's to raise) */
        const int ncols = (int)xc->len;
        concat_col_t *C = (concat_col_t *)calloc((size_t)ncols, sizeof(*C));
        obj_p *pairs = (obj_p *)calloc((size_t)ncols * 2, sizeof(obj_p));
        const char *why = (C && pairs) ? NULL : "host memory";
        for (int k = 0; k < ncols && !why; k++) { /* y's columns in x's name order (ray_find over the names, core/compose.c:769) */
            int64_t j = 0;
            while (j < yn->len && RFX_AS_I64(yn)[j] != RFX_AS_I64(xn)[k]) j++;
            if (j == yn->len) { why = "tables whose name sets differ"; break; }
            obj_p a = RFX_AS_LIST(xc)[k], b = RFX_AS_LIST(yc)[j];
            if (!a || !b || a->type <= 0 || b->type <= 0) why = "a column that is not a vector of a concat type";
            else if (a->type != b->type) why = "paired columns of different types"; /* (err_type is the host's to raise) */
            else if ((why = cells_vec_why(a)) == NULL) why = cells_vec_why(b);
            pairs[2 * k] = a;
            pairs[2 * k + 1] = b;
            C[k].type = a ? a->type : 0;
            C[k].nparts = 2;
            C[k].parts = pairs + 2 * k;
        }
        for (int k = 0; k < ncols && !why; k++) /* (a name twice in x: as many names on both sides, yet not the same set) */
            for (int j = 0; j < k; j++)
                if (RFX_AS_I64(xn)[j] == RFX_AS_I64(xn)[k]) why = "tables whose name sets differ";
        if (why) {
            free(C);
            free(pairs);
            return concat_host(F_CONCAT, x, y, why);
        }
        obj_p rv = H.vector(RFX_TYPE_LIST, ncols);
        memset(RFX_AS_LIST(rv), 0, (size_t)ncols * sizeof(obj_p));
        rc = concat_run(C, ncols, RFX_AS_LIST(rv), &at);
        free(C);
        free(pairs);
        res_fill_empty(rv);
        return concat_finish(F_CONCAT, x, y, rc, at, H.table(H.clone(xn), rv));
    }
    if (x->type < 0 && y->type < 0) return concat_host(F_CONCAT, x, y, "an atom with an atom");
    const int tx = x->type < 0 ? -x->type : x->type, ty = y->type < 0 ? -y->type : y->type;
    if (x->type == RFX_TYPE_TABLE || y->type == RFX_TYPE_TABLE || x->type == RFX_TYPE_DICT || y->type == RFX_TYPE_DICT || x->type == RFX_TYPE_LIST ||
        y->type == RFX_TYPE_LIST)
        return concat_host(F_CONCAT, x, y, "a LIST, a DICT, or a table with something else");
    const char *why = x->type > 0 ? cells_vec_why(x) : (y->type > 0 ? cells_vec_why(y) : NULL);
    if (!why && tx != ty) why = "operands of different types"; /* (the reference answers a LIST) */
    if (!why && y->type > 0) why = cells_vec_why(y);
    if (why) return concat_host(F_CONCAT, x, y, why);
    obj_p parts[2] = {x, y}, out = NULL;
    const concat_col_t C = {tx, 2, parts};
    rc = concat_run(&C, 1, &out, &at);
    return concat_finish(F_CONCAT, x, y, rc, at, out);
}

/* ---- raze ---- */
static obj_p raze_impl(obj_p x) {
    rfx_host_bind();
    if (!x) return fail("raze: null argument");
    g_last_concat_gpu = 0;
    if (x->type != RFX_TYPE_LIST) return concat_host(F_RAZE, x, NULL, "not a list"); /* (the reference answers a clone) */
    if (x->len == 0) return concat_host(F_RAZE, x, NULL, "an empty list");            /* (... and its null object) */
    obj_p *v = RFX_AS_LIST(x);
    if (!v[0] || v[0]->type <= 0) return concat_host(F_RAZE, x, NULL, "elements that are not all vectors of one type");
    for (int64_t i = 1; i < x->len; i++)
        if (!v[i] || v[i]->type != v[0]->type) return concat_host(F_RAZE, x, NULL, "elements that are not all vectors of one type");
    for (int64_t i = 0; i < x->len; i++) {
        const char *why = cells_vec_why(v[i]);
        if (why) return concat_host(F_RAZE, x, NULL, why);
    }
    obj_p out = NULL;
    const concat_col_t C = {v[0]->type, x->len, v};
    int at;
    const int rc = concat_run(&C, 1, &out, &at);
    return concat_finish(F_RAZE, x, NULL, rc, at, out);
}

OP2(rfx_concat, concat_impl(x, y))
OP1(rfx_raze, raze_impl(x))
