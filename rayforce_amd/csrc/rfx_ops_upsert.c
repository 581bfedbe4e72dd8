/* rfx_ops_upsert.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * The keyed write: (upsert t keys batch) and (insert t batch) -- ray_upsert / ray_insert, core/update.c:414-750 -- over a table VALUE whose columns are
 * plain vectors of the concat types, on the device (rfx_upsert.hip through rfx_exec_upsert.c): one index (the set verbs' find for one key, the join index
 * for 2 .. 8), one plan (last writer wins, unmatched rows ranked in order), then per column the table's cells copied, the batch cells placed and the
 * column's null over what the batch does not provide.
 * The batch is a LIST of l <= p vectors of the columns' own types and one length, a LIST of l atoms (one record), or a DICT with symbol keys / a TABLE,
 * whose values are put into the table's column order first (__reorder_columns, :146-204): a column it misses is a null VECTOR there -- 0 for the 1-, 2- and
 * 4-byte types, the null for I64 / SYMBOL / TIMESTAMP / F64 (nullv, core/rayforce.c:104-148) -- which matched rows receive too, while a short LIST leaves
 * matched rows alone and appends null(type) ATOMS, which exist for B8 / I64 / SYMBOL / TIMESTAMP / F64 only (:85-102: another type's column becomes a LIST
 * in the reference -- the host's).  Matched rows are written by set_idx (core/rayforce.c:1399-1435), which knows I64 / SYMBOL / TIMESTAMP / F64 cells only: a
 * matched row turns a B8 / I16 / I32 value column into a LIST (the host's, decided once the index is known); DATE / TIME columns never stay vectors, U8
 * ones under insert's vector forms only.
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c).  Every result is a fresh table over a clone of t's names, every column a fresh host vector of
 * the column's type, attribute byte 0, filled by read-back; the result inherits residency exactly as concat's does (res_col_t, rfx_ops_cols.c). */
static int g_last_upsert_gpu = 0;
int rfx_last_upsert_on_gpu(void) { return g_last_upsert_gpu; }

static obj_p upsert_host(int f, obj_p *x, int64_t n, const char *why) {
    g_last_upsert_gpu = 0;
    return hand_off(f, NULL, 0, 0, x, n, why);
}
/* what nullv() fills a vector of this type with; *atom: null() of the type is a cell of it */
static uint64_t upsert_null_bits(int type, int *atom) {
    const int wide = type == RFX_TYPE_I64 || type == RFX_TYPE_SYMBOL || type == RFX_TYPE_TIMESTAMP;
    if (atom) *atom = wide || type == RFX_TYPE_F64 || type == RFX_TYPE_B8;
    return wide ? (uint64_t)RFX_NULL_I64 : (type == RFX_TYPE_F64 ? RFX_NULL_F64_BITS : 0);
}
static int64_t upsert_name_at(obj_p names, int64_t sym) {
    for (int64_t i = 0; i < names->len; i++)
        if (RFX_AS_I64(names)[i] == sym) return i;
    return -1;
}
/* one table column's share of the batch */
typedef struct {
    obj_p tcol; /* the table's vector */
    obj_p b;    /* the batch's vector (or atom: one record); NULL: not provided */
    int nulled; /* not provided by a DICT / TABLE: a null vector, matched rows included */
} upsert_col_t;
static size_t upsert_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

/* keys >= 1: upsert; keys == 0: insert.  x / n: the call as it came (for the hand-off) */
static obj_p upsert_run(int f, obj_p *x, int64_t nargs, obj_p tab, int64_t keys, obj_p batch) {
    const char *verb = keys ? "upsert" : "insert";
    if (tab->type == -RFX_TYPE_SYMBOL) return upsert_host(f, x, nargs, "a quoted symbol: the in-place form on a global");
    if (tab->type != RFX_TYPE_TABLE) return upsert_host(f, x, nargs, "not a table");
    obj_p names = RFX_AS_LIST(tab)[0], tcols = RFX_AS_LIST(tab)[1];
    if (!names || !tcols || names->type != RFX_TYPE_SYMBOL || tcols->type != RFX_TYPE_LIST || tcols->len < 1 || names->len != tcols->len)
        return upsert_host(f, x, nargs, "a table with no columns");
    if (is_parted_table(tab)) return upsert_host(f, x, nargs, "a parted table");
    const int64_t p = tcols->len;
    if (keys > p) return upsert_host(f, x, nargs, "more keys than the table has columns");
    int64_t n = -1;
    for (int64_t i = 0; i < p; i++) {
        obj_p c = RFX_AS_LIST(tcols)[i];
        if (!c || c->type <= 0) return upsert_host(f, x, nargs, "a column that is not a vector of a concat type");
        const char *why = cells_vec_why(c);
        if (why) return upsert_host(f, x, nargs, why);
        if (c->type == RFX_TYPE_DATE || c->type == RFX_TYPE_TIME) return upsert_host(f, x, nargs, "a DATE / TIME column: the reference answers a LIST column");
        if (c->type == RFX_TYPE_U8 && keys) return upsert_host(f, x, nargs, "a U8 column: the reference answers a LIST column");
        if (i < keys && !set_key_type(c)) return upsert_host(f, x, nargs, "a key column that is not I64 / SYMBOL / TIMESTAMP");
        if (n >= 0 && c->len != n) return upsert_host(f, x, nargs, "table columns of unequal lengths");
        n = c->len;
    }
    /* ---- the batch, in the table's column order ---- */
    obj_p bvals = batch;
    obj_p bnames = NULL;
    if (batch->type == RFX_TYPE_DICT || batch->type == RFX_TYPE_TABLE) {
        bnames = RFX_AS_LIST(batch)[0];
        bvals = RFX_AS_LIST(batch)[1];
        if (!bnames || bnames->type != RFX_TYPE_SYMBOL) return upsert_host(f, x, nargs, "a DICT whose keys are not symbols");
        if (!bvals || bvals->type != RFX_TYPE_LIST || bvals->len != bnames->len) return upsert_host(f, x, nargs, "a DICT whose values are not a LIST");
    } else if (batch->type != RFX_TYPE_LIST)
        return upsert_host(f, x, nargs, "a batch that is not a LIST, a DICT or a TABLE");
    const int64_t l = bvals->len;
    if (l < 1) return upsert_host(f, x, nargs, "an empty batch");
    if (l > p) return upsert_host(f, x, nargs, "more batch columns than the table has");
    for (int64_t i = 0; i < l; i++)
        if (!RFX_AS_LIST(bvals)[i]) return upsert_host(f, x, nargs, "a batch column that is not a vector or an atom of its column's type");
    const int single = RFX_AS_LIST(bvals)[0]->type < 0;
    upsert_col_t *C = (upsert_col_t *)calloc((size_t)p, sizeof(*C));
    if (!C) return fail("upsert: out of host memory");
    const char *why = NULL;
    for (int64_t i = 0; i < p; i++) C[i].tcol = RFX_AS_LIST(tcols)[i];
    if (bnames) {
        for (int64_t j = 0; j < l && !why; j++) {
            const int64_t i = upsert_name_at(names, RFX_AS_I64(bnames)[j]);
            if (i < 0) why = "a DICT name the table does not have";
            else if (C[i].b) why = "a name twice";
            else C[i].b = RFX_AS_LIST(bvals)[j];
        }
        for (int64_t i = 0; i < p && !why; i++) {
            C[i].nulled = !C[i].b;
            for (int64_t j = 0; j < i; j++)
                if (RFX_AS_I64(names)[j] == RFX_AS_I64(names)[i]) why = "a name twice";
        }
    } else {
        for (int64_t i = 0; i < l; i++) C[i].b = RFX_AS_LIST(bvals)[i];
        if (!keys && l < p) why = "a LIST of fewer columns than the table has: a ragged table";
    }
    if (!why && keys > l) why = "fewer batch columns than keys";
    if (!why && single && keys > 1) why = "one record under several keys: the reference does not find its row";
    for (int64_t i = 0; i < p && !why && single; i++)
        if (C[i].tcol->type == RFX_TYPE_U8) why = "one record for a U8 column: the reference's type error";
    int64_t m = single ? 1 : -1;
    for (int64_t i = 0; i < p && !why; i++) {
        obj_p b = C[i].b;
        const int t = C[i].tcol->type;
        if (!b) {
            int atom;
            upsert_null_bits(t, &atom);
            if (i < keys) why = "a key column the batch does not provide";
            else if (!atom && (single || !C[i].nulled)) why = "a column not provided whose null is not a cell of its type: the reference answers a LIST";
            continue;
        }
        if (single) {
            if (b->type != -t) why = b->type == -RFX_TYPE_F64 && (t == RFX_TYPE_I64 || t == RFX_TYPE_I32) ? "an F64 cell for an integer column" : "a batch cell that is not of its column's type";
        } else {
            if (b->type != t) why = b->type == RFX_TYPE_F64 && (t == RFX_TYPE_I64 || t == RFX_TYPE_I32) ? "an F64 cell for an integer column" : "a batch column that is not a vector or an atom of its column's type";
            else if ((why = cells_vec_why(b)) != NULL) continue;
            else if (m >= 0 && b->len != m) why = "batch columns of unequal lengths";
            else m = b->len;
        }
    }
    if (!why && m < 1) why = "a batch of no rows";
    if (!why && m >= 0x7FFFFFFFLL) why = "2^31 or more batch rows";
    if (why) {
        free(C);
        return upsert_host(f, x, nargs, why);
    }
    /* ---- the device ---- */
    if (ensure_ctx() != RFX_OK) {
        free(C);
        return fail_hip("no usable MI355X");
    }
    if (g_nshards > 1) {
        free(C);
        return upsert_host(f, x, nargs, keys ? "upsert over a sharded table" : "insert over a sharded table");
    }
    rfx_upsert_xcol_t *X = (rfx_upsert_xcol_t *)calloc((size_t)p, sizeof(*X));
    res_col_t *R = (res_col_t *)calloc((size_t)p, sizeof(*R));
    obj_p rv = NULL;
    int rc = X && R ? RFX_OK : RFX_ENOMEM, at = OP_AT_SCRATCH, undefined = 0, narrow = 0;
    /* one staging block: the host cells the cache would not keep as they are (U8, I16, I32 / DATE / TIME vectors), every part on a 16-byte boundary */
    size_t staged = 0;
    for (int64_t i = 0; i < p && rc == RFX_OK; i++) {
        const int w = cell_width(C[i].tcol->type);
        if (cells_staged(C[i].tcol)) staged += upsert_pad16((size_t)n * (size_t)w);
        if (C[i].b && !single && cells_staged(C[i].b)) staged += upsert_pad16((size_t)m * (size_t)w);
    }
    void *stage = NULL, *slots = NULL, *d_idx = NULL, *d_dest = NULL;
    if (rc == RFX_OK && staged) rc = op_scratch(&stage, staged);
    if (rc == RFX_OK && single) rc = op_scratch(&slots, (size_t)p * 16);
    char *next = (char *)stage;
    if (rc == RFX_OK) at = OP_AT_UPLOAD;
    uint64_t *hslots = single && rc == RFX_OK ? (uint64_t *)calloc((size_t)p * 2, 8) : NULL;
    if (single && rc == RFX_OK && !hslots) rc = RFX_ENOMEM;
    for (int64_t i = 0; i < p && rc == RFX_OK; i++) {
        const int t = C[i].tcol->type, w = cell_width(t);
        X[i].width = w;
        X[i].null_bits = upsert_null_bits(t, NULL);
        X[i].role = i < keys ? RFX_UPSERT_KEY : RFX_UPSERT_VALUE;
        if (n > 0 && (rc = native_cells(C[i].tcol, w, &next, &X[i].d_table)) != RFX_OK) break;
        next = (char *)stage + upsert_pad16((size_t)(next - (char *)stage));
        if (single) { /* the record's cell -- or the column's null -- in a 16-byte slot of its own */
            if (C[i].b) hslots[2 * i] = atom_cell_bits(C[i].b, w);
            else if (C[i].nulled && keys) hslots[2 * i] = X[i].null_bits;
            else X[i].role = RFX_UPSERT_ABSENT;
            if (X[i].role != RFX_UPSERT_ABSENT) X[i].d_batch = (char *)slots + 16 * i;
        } else if (C[i].b) {
            if ((rc = native_cells(C[i].b, w, &next, &X[i].d_batch)) != RFX_OK) break;
            next = (char *)stage + upsert_pad16((size_t)(next - (char *)stage));
        } else if (C[i].nulled && keys) { /* a null vector of the batch's length, as the reference makes one: matched rows take it too */
            void *dn = NULL;
            at = OP_AT_SCRATCH;
            if ((rc = op_scratch(&dn, (size_t)m * (size_t)w)) != RFX_OK) break;
            at = OP_AT_PLANNER;
            if ((rc = rfx_hip_upsert_fill(g_ctx, dn, w, X[i].null_bits, m)) != RFX_OK) break;
            at = OP_AT_UPLOAD;
            X[i].d_batch = dn;
        } else
            X[i].role = RFX_UPSERT_ABSENT;
    }
    if (rc == RFX_OK && single) rc = rfx_hip_h2d(g_ctx, slots, hslots, (size_t)p * 16);
    free(hslots);
    /* ---- index and plan ---- */
    int64_t a = m;
    if (rc == RFX_OK && keys) {
        at = OP_AT_SCRATCH;
        if ((rc = op_scratch(&d_idx, (size_t)m * 8)) == RFX_OK) rc = op_scratch(&d_dest, (size_t)m * 8);
        if (rc == RFX_OK) {
            const void *tk[RFX_MAX_KEYS], *bk[RFX_MAX_KEYS];
            for (int64_t i = 0; i < keys; i++) tk[i] = X[i].d_table, bk[i] = X[i].d_batch;
            at = OP_AT_PLANNER;
            rc = rfx_exec_upsert_index(g_x, tk, bk, (int)keys, n, m, (int64_t *)d_idx, &undefined);
            if (rc == RFX_OK) rc = rfx_exec_upsert_plan(g_x, (const int64_t *)d_idx, m, n, (int64_t *)d_dest, &a);
        }
        /* set_idx (core/rayforce.c:1399-1435) writes I64 / SYMBOL / TIMESTAMP / F64 cells only: a matched row turns any other value column into a LIST */
        for (int64_t i = keys; i < p && rc == RFX_OK && a < m; i++)
            if (X[i].role == RFX_UPSERT_VALUE && X[i].width != 8) narrow = 1, rc = RFX_ESTATE;
    }
    /* ---- the columns ---- */
    const int adopt = res_col_adopt_on();
    if (rc == RFX_OK) {
        rv = H.vector(RFX_TYPE_LIST, p);
        memset(RFX_AS_LIST(rv), 0, (size_t)p * sizeof(obj_p));
        for (int64_t i = 0; i < p && rc == RFX_OK; i++) {
            obj_p out = H.vector((int8_t)C[i].tcol->type, n + a);
            out->attrs = 0;
            RFX_AS_LIST(rv)[i] = out;
            at = OP_AT_SCRATCH;
            rc = res_col_alloc(&R[i], out, X[i].width, adopt);
            X[i].d_out = R[i].d;
        }
        if (rc == RFX_OK) {
            at = OP_AT_PLANNER;
            rc = keys ? rfx_exec_upsert_cols(g_x, X, (int)p, (const int64_t *)d_dest, m, n, a) : rfx_exec_insert_cols(g_x, X, (int)p, m, n);
        }
        if (rc == RFX_OK && (rc = res_cols_read(R, p)) != RFX_OK) at = -1;
        res_cols_finish(R, p, rc, adopt);
        res_fill_empty(rv);
    }
    free(X);
    free(R);
    free(C);
    if (rc == RFX_OK) {
        g_last_upsert_gpu = 1;
        return H.table(H.clone(names), rv);
    }
    if (rv) H.drop(rv);
    if (rc == RFX_ESTATE && narrow) return upsert_host(f, x, nargs, "a matched row for a 1-, 2- or 4-byte value column: the reference answers a LIST column");
    if (rc == RFX_ESTATE && undefined) return upsert_host(f, x, nargs, undefined == 2 ? "two key tuples share one row hash" : rfx_exec_last_error(g_x));
    return op_outcome(f, x, nargs, rc, at, keys ? "upsert over a sharded table" : "insert over a sharded table", verb);
}

static obj_p upsert_impl(obj_p *x, int64_t n) {
    rfx_host_bind();
    g_last_upsert_gpu = 0;
    if (!x || n != 3 || !x[0] || !x[1] || !x[2]) return x && n > 0 ? upsert_host(F_UPSERT, x, n, "not three arguments") : fail("upsert: null argument");
    if (x[1]->type != -RFX_TYPE_I64) return upsert_host(F_UPSERT, x, n, "keys is not an I64 atom");
    if (x[1]->i64 < 1) return upsert_host(F_UPSERT, x, n, "keys < 1");
    if (x[1]->i64 > RFX_MAX_KEYS) return upsert_host(F_UPSERT, x, n, "more than 8 keys");
    return upsert_run(F_UPSERT, x, n, x[0], x[1]->i64, x[2]);
}
static obj_p insert_impl(obj_p *x, int64_t n) {
    rfx_host_bind();
    g_last_upsert_gpu = 0;
    if (!x || n != 2 || !x[0] || !x[1]) return x && n > 0 ? upsert_host(F_INSERT, x, n, "not two arguments") : fail("insert: null argument");
    return upsert_run(F_INSERT, x, n, x[0], 0, x[1]);
}

OPN(rfx_upsert, upsert_impl(x, n))
OPN(rfx_insert, insert_impl(x, n))
