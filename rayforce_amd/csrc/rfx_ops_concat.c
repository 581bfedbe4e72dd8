/* rfx_ops_concat.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * The write side as built-ins of their own: concat (ray_concat, core/compose.c:465-823) and raze (ray_raze, core/compose.c:1096-1164) of plain vectors and
 * of tables of them on the device (rfx_concat.hip through rfx_exec_concat.c): every result column is ONE multi-span copy, a table's columns
 * RFX_MAX_COLS to a launch.
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c): a shape the device does not take is the host's own verb when a host is bound, else an
 * error object naming the reason (also in rfx_ops_last_error()).  Every result is fresh host vectors of the operands' type, attribute byte 0, filled by
 * read-back (a table: a fresh table of them over a clone of x's names).
 * THE RESULT INHERITS RESIDENCY: the device buffer of every I64 / SYMBOL / TIMESTAMP / F64 / B8 result column is not freed but entered into the residency
 * cache as the copy of the fresh result vector (concat_adopt), in the form resident() keeps for that type, so that a later operator over the answer uploads
 * nothing.  I32 / DATE / TIME results are not adopted (the cache keeps their widened 8-byte image, which this copy does not make), I16 / U8 are never
 * resident.  RFX_CONCAT_ADOPT=0 turns adoption off. */
static int g_last_concat_gpu = 0;
int rfx_last_concat_on_gpu(void) { return g_last_concat_gpu; }

static obj_p concat_host(int f, obj_p x, obj_p y, const char *why) {
    g_last_concat_gpu = 0;
    return hand_off_xy(f, NULL, x, y, why);
}
/* bytes of one cell of a type concat and raze take (0: another type) */
static int concat_width(int type) { return type == RFX_TYPE_SYMBOL ? 8 : (int)cell_bytes(type); }
/* is the result of this type kept resident?  (the types whose cached copy is the cells as they are) */
static int concat_adopts(int type) {
    return type == RFX_TYPE_I64 || type == RFX_TYPE_SYMBOL || type == RFX_TYPE_TIMESTAMP || type == RFX_TYPE_F64 || type == RFX_TYPE_B8;
}
/* NULL: a vector the device takes; else why not */
static const char *concat_vec_why(obj_p v) {
    if (IS_PARTED_TYPE(v->type)) return "a parted column";
    const int w = concat_width(v->type);
    if (!w) return "not a vector of a concat type";
    if (v->mmod == RFX_MMOD_DEVICE && w != 8 && v->type != RFX_TYPE_B8) return "a device column that is not I64 / F64 / TIMESTAMP / B8";
    return NULL;
}
/* one result column: `nparts` operands of one cell type laid end to end, each a vector of that type or (concat only) an atom of it */
typedef struct {
    int type;
    int64_t nparts;
    obj_p *parts;
} concat_col_t;
/* does this part travel in the column's staging block?  (a host vector whose cells the cache would not keep as they are: U8, I16, I32 / DATE / TIME) */
static int concat_staged(obj_p p) { return p->type > 0 && p->len > 0 && p->mmod != RFX_MMOD_DEVICE && !concat_adopts(p->type); }
/* a part's cells on the device: a device handle's address, the resident copy (8-byte cells and B8: uploaded if need be), or -- staged -- the next cells of
 * the column's staging block `stage` (one block of the call's scratch per column, however many parts) */
static int concat_span(obj_p p, int width, char **stage, rfx_span_t *sp) {
    memset(sp, 0, sizeof(*sp));
    if (p->type < 0) {
        sp->cells = 1;
        sp->bits = width == 8 ? (uint64_t)p->i64 : (width == 4 ? (uint64_t)(uint32_t)p->i32 : (width == 2 ? (uint64_t)(uint16_t)p->i16 : (uint64_t)p->u8));
        return RFX_OK;
    }
    sp->cells = p->len;
    if (!p->len) return RFX_OK;
    if (!concat_staged(p)) return resident(p, 0, &sp->d_ptr);
    const size_t bytes = (size_t)p->len * (size_t)width;
    sp->d_ptr = *stage;
    *stage += bytes;
    g_stat[ST_UPLOADS]++;
    return rfx_hip_h2d_pipelined(g_ctx, (void *)sp->d_ptr, RFX_AS_RAW(p), bytes);
}
/* the device buffer of a result column becomes the cached copy of the fresh host vector it was read back into: what resident() would have made by an
 * upload, without one.  The cache holds its reference (or, in checksum mode, the payload's checksum) exactly as for an uploaded column; the scope fields
 * stay unset */
static void concat_adopt(obj_p out, void *dev, size_t bytes) {
    resident_t e;
    memset(&e, 0, sizeof(e));
    const int own = validate_mode() == 0;
    e.host = RFX_AS_RAW(out); e.len = out->len; e.type = out->type; e.dev = dev; e.bytes = bytes; e.dbytes = bytes; e.tick = ++g_tick; e.epoch = g_epoch;
    e.sum = own ? 0 : payload_sum(e.host, bytes);
    e.owner = own ? H.clone(out) : NULL;
    e.devs[0] = dev;
    res_append(&e);
}
static int concat_adopt_on(void) {
    const char *e = getenv("RFX_CONCAT_ADOPT");
    return !(e && atoi(e) == 0);
}
/* the columns' copies: outs[k] receives column k's fresh vector.  RFX_OK, or the failing step's code with *at saying which step (rows_limit_why) */
static int concat_run(const concat_col_t *C, int ncols, obj_p *outs, int *at) {
    int rc = RFX_OK, any = 0;
    *at = ROWS_AT_PLANNER;
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
    if (!cols) return RFX_ENOMEM;
    const int adopt = concat_adopt_on();
    for (int k = 0; k < ncols && rc == RFX_OK; k++) {
        const int w = concat_width(C[k].type);
        rfx_span_t *sp = (rfx_span_t *)calloc((size_t)C[k].nparts, sizeof(*sp));
        cols[k].spans = sp;
        cols[k].nspans = C[k].nparts;
        cols[k].width = w;
        if (!sp) rc = RFX_ENOMEM;
        size_t staged = 0;
        for (int64_t i = 0; i < C[k].nparts; i++)
            if (concat_staged(C[k].parts[i])) staged += (size_t)C[k].parts[i]->len * (size_t)w;
        void *stage = NULL;
        *at = ROWS_AT_SCRATCH;
        if (rc == RFX_OK && staged) rc = op_scratch(&stage, staged);
        char *next = (char *)stage;
        if (rc == RFX_OK) *at = ROWS_AT_UPLOAD;
        for (int64_t i = 0; i < C[k].nparts && rc == RFX_OK; i++) rc = concat_span(C[k].parts[i], w, &next, &sp[i]);
        if (rc == RFX_OK && outs[k]->len) {
            const size_t bytes = (size_t)outs[k]->len * (size_t)w;
            *at = ROWS_AT_SCRATCH;
            if (adopt && concat_adopts(C[k].type)) res_make_room(bytes);
            rc = rfx_hip_malloc(g_ctx, &cols[k].d_out, bytes);
        }
    }
    if (rc == RFX_OK) *at = ROWS_AT_PLANNER, rc = rfx_exec_concat_cols(g_x, cols, ncols);
    for (int k = 0; k < ncols && rc == RFX_OK; k++)
        if (cols[k].d_out && (rc = rfx_hip_d2h(g_ctx, RFX_AS_RAW(outs[k]), cols[k].d_out, (size_t)outs[k]->len * (size_t)cols[k].width)) != RFX_OK) *at = -1;
    if (rc != RFX_OK) rfx_hip_ctx_sync(g_ctx); /* (a kernel may still be writing the blocks that go back to the pool) */
    for (int k = 0; k < ncols; k++) {
        if (cols[k].d_out) {
            if (rc == RFX_OK && adopt && concat_adopts(C[k].type)) concat_adopt(outs[k], cols[k].d_out, (size_t)outs[k]->len * (size_t)cols[k].width);
            else rfx_hip_free(g_ctx, cols[k].d_out);
        }
        free((void *)cols[k].spans);
    }
    free(cols);
    return rc;
}
/* concat_run's outcome as the verb's answer: `res` (the vector, or the table over the columns) or the hand-off / the failure, the fresh vectors dropped */
static obj_p concat_finish(int f, obj_p x, obj_p y, int rc, int at, obj_p res) {
    if (rc == RFX_OK) {
        g_last_concat_gpu = 1;
        return res;
    }
    if (res) H.drop(res);
    if (rc == RFX_ELIMIT && g_nshards > 1) return concat_host(f, x, y, "concat over a sharded column");
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return concat_host(f, x, y, rows_limit_why(rc, at, "concat over a sharded column"));
    if (rc == RFX_EHIP && !g_ctx) return fail_hip("no usable MI355X");
    if (at == ROWS_AT_UPLOAD) return fail_hip("column upload");
    if (at == ROWS_AT_PLANNER && rfx_exec_last_error(g_x)[0]) return fail(rfx_exec_last_error(g_x));
    return fail_hip(f == F_RAZE ? "raze" : "concat");
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
            else if ((why = concat_vec_why(a)) == NULL) why = concat_vec_why(b);
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
        for (int k = 0; k < ncols; k++) /* (a run that stopped at a length leaves the later slots without a vector) */
            if (!RFX_AS_LIST(rv)[k]) RFX_AS_LIST(rv)[k] = H.vector(RFX_TYPE_I64, 0);
        return concat_finish(F_CONCAT, x, y, rc, at, H.table(H.clone(xn), rv));
    }
    if (x->type < 0 && y->type < 0) return concat_host(F_CONCAT, x, y, "an atom with an atom");
    const int tx = x->type < 0 ? -x->type : x->type, ty = y->type < 0 ? -y->type : y->type;
    if (x->type == RFX_TYPE_TABLE || y->type == RFX_TYPE_TABLE || x->type == RFX_TYPE_DICT || y->type == RFX_TYPE_DICT || x->type == RFX_TYPE_LIST ||
        y->type == RFX_TYPE_LIST)
        return concat_host(F_CONCAT, x, y, "a LIST, a DICT, or a table with something else");
    const char *why = x->type > 0 ? concat_vec_why(x) : (y->type > 0 ? concat_vec_why(y) : NULL);
    if (!why && tx != ty) why = "operands of different types"; /* (the reference answers a LIST) */
    if (!why && y->type > 0) why = concat_vec_why(y);
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
        const char *why = concat_vec_why(v[i]);
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
