/* rfx_ops_asof.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * asof-join (ray_asof_join, core/join.c:300-356) and bin / binr (ray_bin / ray_binr, core/items.c:1552-1644) on the device: the index is the
 * planner's (rfx_exec_asof_index, rfx_exec_bin over rfx_asof.hip), the table is the left join's (left_join_assemble).  Every shape outside the
 * device path -- and every error the reference reports -- is the host's own verb, the reason in rfx_ops_last_error(). */
static int g_last_asof_gpu = 0, g_asof_handed = 0;
int rfx_last_asof_on_gpu(void) { return g_last_asof_gpu; }

static obj_p asof_host(obj_p *x, int64_t n, const char *why) {
    g_last_asof_gpu = 0;
    g_asof_handed = 1;
    return hand_off(F_AJ, NULL, 0, 0, x, n, why);
}
static int asof_time_type(obj_p c) { return c->type == RFX_TYPE_I64 || c->type == RFX_TYPE_TIMESTAMP || IS_I32_FAMILY(c->type); }
/* the key tuple of asof-join and of the window joins -- the equality keys' names and, last, the time column's -- looked up in both tables: why the device
 * does not take it, or NULL with the columns in lk / rk / *ltime / *rtime.  An asof column is an 8-byte or a 4-byte integer, a window column a 4-byte one */
static const char *join_key_tuple(obj_p ksyms, obj_p lt, obj_p rt, int window, obj_p *lk, obj_p *rk, obj_p *ltime, obj_p *rtime) {
    if (ksyms->len < 2) return "fewer than two key names";
    if (is_parted_table(lt) || is_parted_table(rt)) return "parted table";
    const int nk = (int)ksyms->len - 1; /* the equality keys; the last name is the time column */
    if (nk > RFX_MAX_KEYS) return "more than 8 equality keys";
    *ltime = table_col(lt, RFX_AS_I64(ksyms)[nk]);
    *rtime = table_col(rt, RFX_AS_I64(ksyms)[nk]);
    if (!*ltime || !*rtime) return window ? "window column missing from a table" : "asof column missing from a table";
    if ((*ltime)->type != (*rtime)->type) return window ? "window columns of different types" : "asof columns of different types";
    /* (an F64 asof column, an I64 / TIMESTAMP window column the reference reads through AS_I32: DESIGN.md, reference defects observed -- the host's) */
    if (window ? !IS_I32_FAMILY((*ltime)->type) : !asof_time_type(*ltime)) return window ? "window column type" : "asof column type";
    for (int i = 0; i < nk; i++) {
        lk[i] = table_col(lt, RFX_AS_I64(ksyms)[i]);
        rk[i] = table_col(rt, RFX_AS_I64(ksyms)[i]);
        if (!lk[i] || !rk[i] || lk[i]->type <= 0 || rk[i]->type <= 0 || col_ctype(lk[i]) != RFX_I64 || col_ctype(rk[i]) != RFX_I64 || lk[i]->type != rk[i]->type)
            return "equality key is not an 8-byte integer column of both tables";
    }
    return NULL;
}
static obj_p asof_impl(obj_p *x, int64_t n) {
    rfx_host_bind();
    g_last_asof_gpu = 0;
    /* the reference's own errors (arity, types, one key name, no such asof column, asof columns of two types) are the reference's to word */
    if (n != 3 || !x || !x[0] || !x[1] || !x[2]) return asof_host(x, n, "expected (keys, left table, right table)");
    if (x[0]->type != RFX_TYPE_SYMBOL || x[1]->type != RFX_TYPE_TABLE || x[2]->type != RFX_TYPE_TABLE) return asof_host(x, n, "expected (symbol vector, table, table)");
    obj_p ksyms = x[0], lt = x[1], rt = x[2], lk[RFX_MAX_KEYS], rk[RFX_MAX_KEYS], ltime = NULL, rtime = NULL;
    const char *why = join_key_tuple(ksyms, lt, rt, 0, lk, rk, &ltime, &rtime);
    if (why) return asof_host(x, n, why);
    obj_p lnames = RFX_AS_LIST(lt)[0], lcols = RFX_AS_LIST(lt)[1], rnames = RFX_AS_LIST(rt)[0], rcols = RFX_AS_LIST(rt)[1];
    const int64_t nl = lcols->len ? RFX_AS_LIST(lcols)[0]->len : 0, nr = rcols->len ? RFX_AS_LIST(rcols)[0]->len : 0;
    const int nk = (int)ksyms->len - 1; /* the equality keys; the last name is the asof column */
    /* every other column travels as 8 bytes.  The exemption is by NAME: only the column the asof symbol resolves to is never gathered (the result's
     * is the left table's own object); the same 4-byte vector under a second name -- (table [s t qt] (list S T T)) -- is a passenger like any other */
    const int64_t tsym = RFX_AS_I64(ksyms)[nk];
    for (int64_t i = 0; i < lcols->len; i++) {
        obj_p c = RFX_AS_LIST(lcols)[i];
        if (!(RFX_AS_I64(lnames)[i] == tsym && c == ltime) && !(c->type > 0 && col_ctype(c))) return asof_host(x, n, "non-8-byte column");
        if (c->len != nl) return asof_host(x, n, "columns of different lengths");
    }
    for (int64_t i = 0; i < rcols->len; i++) {
        obj_p rc = RFX_AS_LIST(rcols)[i], lc = table_col(lt, RFX_AS_I64(rnames)[i]);
        if (!(RFX_AS_I64(rnames)[i] == tsym && rc == rtime) && !(rc->type > 0 && col_ctype(rc))) return asof_host(x, n, "non-8-byte column");
        if (rc->len != nr) return asof_host(x, n, "columns of different lengths");
        if (lc && lc->type != rc->type) return fail("join: a column has different types in the two tables"); /* err_type, core/join.c:50-51 */
    }
    {
        int64_t names[64];
        if (join_column_names(ksyms, lt, rt, names) >= 64) return asof_host(x, n, "too many columns");
    }
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return asof_host(x, n, "asof join over a sharded table");
    const void *dlk[RFX_MAX_KEYS], *drk[RFX_MAX_KEYS], *dlt = NULL, *drt = NULL;
    for (int i = 0; i < nk; i++)
        if (resident(lk[i], 0, &dlk[i]) != RFX_OK || resident(rk[i], 0, &drk[i]) != RFX_OK) return fail_hip("column upload");
    /* (a 4-byte asof column is resident as its widened copy, rfx_hip_widen_i32: order and nulls survive) */
    if (resident(ltime, 0, &dlt) != RFX_OK || resident(rtime, 0, &drt) != RFX_OK) return fail_hip("column upload");
    void *ids = NULL;
    if (op_scratch(&ids, (size_t)nl * 8) != RFX_OK) return asof_host(x, n, "device memory");
    int collision = 0;
    const int rc = rfx_exec_asof_index(g_x, dlk, drk, nk, (const int64_t *)dlt, (const int64_t *)drt, nl, nr, (int64_t *)ids, &collision);
    if (rc != RFX_OK && collision) return asof_host(x, n, "row-hash collision between two key tuples");
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return asof_host(x, n, rc == RFX_ENOMEM ? "device memory" : "more rows than the device sort takes");
    if (rc != RFX_OK) return fail(rfx_exec_last_error(g_x));
    obj_p res = NULL;
    const int a = left_join_assemble(ksyms, lt, rt, ids, nl, &res);
    if (a == 0) return asof_host(x, n, "too many columns");
    if (a > 0) g_last_asof_gpu = nl > 0;
    return res;
}
rfx_obj_p rfx_asof_join(rfx_obj_p *x, int64_t n) {
    op_begin();
    g_asof_handed = 0;
    obj_p r = asof_impl(x, n);
    /* (an empty left table and the join's own type error are answered here without the device and without the host: neither counter) */
    if (g_last_asof_gpu) g_stat[ST_JOIN_GPU]++;
    else if (g_asof_handed) g_stat[ST_JOIN_DELEGATED]++;
    op_end();
    return r;
}

static obj_p bin_host(int f, obj_p x, obj_p y, const char *why) {
    g_last_asof_gpu = 0;
    return hand_off_xy(f, NULL, x, y, why);
}
static obj_p bin_impl(int right, obj_p x, obj_p y) {
    rfx_host_bind();
    const int f = right ? F_BINR : F_BIN;
    g_last_asof_gpu = 0;
    if (!x || !y) return fail("bin: null argument");
    /* (an atom on the right is one search of the host's own; 4-byte vectors and every other pair of types are the host's too) */
    if (x->type != y->type || (x->type != RFX_TYPE_I64 && x->type != RFX_TYPE_TIMESTAMP)) return bin_host(f, x, y, "operands are not two I64 or two TIMESTAMP vectors");
    const int64_t nx = x->len, ny = y->len;
    if (ny == 0) return H.vector(RFX_TYPE_I64, 0);
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return bin_host(f, x, y, "bin over a sharded table");
    const void *dx = NULL, *dy = NULL;
    void *dout = NULL;
    if (resident(x, 0, &dx) != RFX_OK || resident(y, 0, &dy) != RFX_OK) return fail_hip("column upload");
    if (op_scratch(&dout, (size_t)ny * 8) != RFX_OK) return bin_host(f, x, y, "device memory");
    if (rfx_exec_bin(g_x, (const int64_t *)dx, nx, (const int64_t *)dy, ny, right, (int64_t *)dout) != RFX_OK) return fail(rfx_exec_last_error(g_x));
    obj_p out = H.vector(RFX_TYPE_I64, ny);
    if (rfx_hip_d2h(g_ctx, RFX_AS_RAW(out), dout, (size_t)ny * 8) != RFX_OK) {
        H.drop(out);
        return fail_hip("bin result");
    }
    g_last_asof_gpu = 1;
    return out;
}
OP2(rfx_bin, bin_impl(0, x, y))
OP2(rfx_binr, bin_impl(1, x, y))
