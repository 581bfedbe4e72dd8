/* rfx_ops_window.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * window-join / window-join1 (ray_window_join / ray_window_join1, core/join.c:358-489) on the device: the windows are the planner's
 * (rfx_exec_window_ranges), every aggregate of one value column is one launch (rfx_exec_window_fold over rfx_window.hip).  The result is the left
 * table's own column objects followed by one new vector per dict entry.  Every shape outside the device path -- and every error the reference
 * reports -- is the host's own verb, the reason in rfx_ops_last_error(). */
static int g_last_window_gpu = 0, g_window_handed = 0;
int rfx_last_window_on_gpu(void) { return g_last_window_gpu; }

#define WJ_MAX_AGGS 64
#define WJ_MAX_COLS 16

static obj_p window_host(int closed, obj_p *x, int64_t n, const char *why) {
    g_last_window_gpu = 0;
    g_window_handed = 1;
    return hand_off(closed ? F_WJ1 : F_WJ, NULL, 0, 0, x, n, why);
}
/* (agg col): the aggregate as RFX_WAGG_*, by function object or by its name; -1: not one of the seven */
static int window_agg(obj_p head) {
    static const struct { int f; const char *name; int agg; } A[] = {{F_SUM, "sum", RFX_WAGG_SUM}, {F_MIN, "min", RFX_WAGG_MIN}, {F_MAX, "max", RFX_WAGG_MAX},
        {F_COUNT, "count", RFX_WAGG_COUNT}, {F_AVG, "avg", RFX_WAGG_AVG}, {F_FIRST, "first", RFX_WAGG_FIRST}, {F_LAST, "last", RFX_WAGG_LAST}};
    const int f = fn_id(head);
    const char *name = (head && head->type == -RFX_TYPE_SYMBOL) ? H.symname(head->i64) : NULL;
    for (size_t i = 0; i < sizeof(A) / sizeof(A[0]); i++)
        if (f == A[i].f || (name && strcmp(name, A[i].name) == 0)) return A[i].agg;
    return -1;
}
static obj_p window_impl(int closed, obj_p *x, int64_t n) {
    rfx_host_bind();
    g_last_window_gpu = 0;
    /* the reference's own errors (arity, argument types, no such window column, window columns of two types) are the reference's to word */
    if (n != 5 || !x || !x[0] || !x[1] || !x[2] || !x[3] || !x[4]) return window_host(closed, x, n, "expected (keys, windows, left table, right table, aggregates)");
    if (x[0]->type != RFX_TYPE_SYMBOL || x[1]->type != RFX_TYPE_LIST || x[2]->type != RFX_TYPE_TABLE || x[3]->type != RFX_TYPE_TABLE || x[4]->type != RFX_TYPE_DICT)
        return window_host(closed, x, n, "expected (symbol vector, list, table, table, dict)");
    obj_p ksyms = x[0], wins = x[1], lt = x[2], rt = x[3], dict = x[4], lk[RFX_MAX_KEYS], rk[RFX_MAX_KEYS], ltime = NULL, rtime = NULL;
    const char *bad = join_key_tuple(ksyms, lt, rt, 1, lk, rk, &ltime, &rtime); /* (rfx_ops_asof.c) */
    if (bad) return window_host(closed, x, n, bad);
    obj_p lnames = RFX_AS_LIST(lt)[0], lcols = RFX_AS_LIST(lt)[1], rcols = RFX_AS_LIST(rt)[1];
    const int64_t nl = lcols->len ? RFX_AS_LIST(lcols)[0]->len : 0, nr = rcols->len ? RFX_AS_LIST(rcols)[0]->len : 0;
    const int nk = (int)ksyms->len - 1; /* the equality keys; the last name is the window column */
    for (int64_t i = 0; i < lcols->len; i++)
        if (RFX_AS_LIST(lcols)[i]->type <= 0 || RFX_AS_LIST(lcols)[i]->len != nl) return window_host(closed, x, n, "columns of different lengths");
    for (int64_t i = 0; i < rcols->len; i++)
        if (RFX_AS_LIST(rcols)[i]->type <= 0 || RFX_AS_LIST(rcols)[i]->len != nr) return window_host(closed, x, n, "columns of different lengths");
    if (wins->len != 2) return window_host(closed, x, n, "windows are not a list of two vectors");
    obj_p wlo = RFX_AS_LIST(wins)[0], whi = RFX_AS_LIST(wins)[1];
    if (!wlo || !whi || !IS_I32_FAMILY(wlo->type) || !IS_I32_FAMILY(whi->type) || wlo->len != nl || whi->len != nl)
        return window_host(closed, x, n, "windows are not two 4-byte integer vectors of the left table's length");
    /* the aggregates: (agg col) over I64 / F64 columns of the right table, grouped by column */
    obj_p dkeys = RFX_AS_LIST(dict)[0], dvals = RFX_AS_LIST(dict)[1];
    if (!dkeys || !dvals || dkeys->type != RFX_TYPE_SYMBOL || dvals->type != RFX_TYPE_LIST || dkeys->len != dvals->len)
        return window_host(closed, x, n, "aggregates are not a dict of expressions by name");
    const int nagg = (int)dkeys->len;
    if (dkeys->len > WJ_MAX_AGGS) return window_host(closed, x, n, "more than 64 aggregates");
    int agg[WJ_MAX_AGGS], aggcol[WJ_MAX_AGGS], ncol = 0;
    obj_p vcol[WJ_MAX_COLS];
    for (int i = 0; i < nagg; i++) {
        obj_p e = RFX_AS_LIST(dvals)[i];
        if (!e || e->type != RFX_TYPE_LIST) return window_host(closed, x, n, "an aggregate is not of the form (agg column): a raw column or an atom");
        if (e->len != 2) return window_host(closed, x, n, "an aggregate is not of the form (agg column)");
        obj_p a = RFX_AS_LIST(e)[1];
        if ((agg[i] = window_agg(RFX_AS_LIST(e)[0])) < 0) return window_host(closed, x, n, "an aggregate other than sum, min, max, count, avg, first, last");
        if (!a || a->type != -RFX_TYPE_SYMBOL || (a->attrs & RFX_ATTR_QUOTED)) return window_host(closed, x, n, "an aggregate of an expression");
        obj_p c = table_col(rt, a->i64);
        if (!c) return window_host(closed, x, n, "an aggregate of a column the right table lacks");
        if (c->type != RFX_TYPE_I64 && c->type != RFX_TYPE_F64) return window_host(closed, x, n, "an aggregate of a column that is neither I64 nor F64");
        int k = 0;
        while (k < ncol && vcol[k] != c) k++;
        if (k == ncol) {
            if (ncol == WJ_MAX_COLS) return window_host(closed, x, n, "more than 16 aggregated columns");
            vcol[ncol++] = c;
        }
        aggcol[i] = k;
    }
    /* result: the left table's columns, then one vector per dict entry in dict order (count: I64, avg: F64, else the column's type) */
    obj_p names = H.vector(RFX_TYPE_SYMBOL, lnames->len + nagg), cols = H.vector(RFX_TYPE_LIST, lnames->len + nagg);
    for (int64_t i = 0; i < lnames->len; i++) {
        RFX_AS_I64(names)[i] = RFX_AS_I64(lnames)[i];
        RFX_AS_LIST(cols)[i] = H.clone(RFX_AS_LIST(lcols)[i]);
    }
    for (int i = 0; i < nagg; i++) {
        RFX_AS_I64(names)[lnames->len + i] = RFX_AS_I64(dkeys)[i];
        const int8_t t = agg[i] == RFX_WAGG_COUNT ? RFX_TYPE_I64 : agg[i] == RFX_WAGG_AVG ? RFX_TYPE_F64 : vcol[aggcol[i]]->type;
        RFX_AS_LIST(cols)[lnames->len + i] = H.vector(t, nl);
    }
    obj_p res = NULL;
    const char *why = NULL;
    void *dout[RFX_WAGG_N] = {0};
    /* an empty left table: empty typed columns, as the reference with one worker answers (with more its pool divides by zero) -- never the host's */
    if (nl == 0) return H.table(names, cols);
    if (ensure_ctx() != RFX_OK) { res = fail_hip("no usable MI355X"); goto drop; }
    if (g_nshards > 1) { why = "window join over a sharded table"; goto drop; }
    {
        const void *dlk[RFX_MAX_KEYS], *drk[RFX_MAX_KEYS], *dlo = NULL, *dhi = NULL, *drt = NULL, *dv = NULL;
        for (int i = 0; i < nk; i++)
            if (resident(lk[i], 0, &dlk[i]) != RFX_OK || resident(rk[i], 0, &drk[i]) != RFX_OK) { res = fail_hip("column upload"); goto drop; }
        /* (4-byte columns are resident as their widened copies, rfx_hip_widen_i32: order and nulls survive) */
        if (resident(wlo, 0, &dlo) != RFX_OK || resident(whi, 0, &dhi) != RFX_OK || resident(rtime, 0, &drt) != RFX_OK) { res = fail_hip("column upload"); goto drop; }
        void *perm = NULL, *li = NULL, *ri = NULL;
        if (op_scratch(&perm, (size_t)nr * 8) != RFX_OK || op_scratch(&li, (size_t)nl * 8) != RFX_OK || op_scratch(&ri, (size_t)nl * 8) != RFX_OK) { why = "device memory"; goto drop; }
        int collision = 0;
        int64_t stats[2];
        int rc = rfx_exec_window_ranges(g_x, dlk, drk, nk, (const int64_t *)dlo, (const int64_t *)dhi, (const int64_t *)drt, nl, nr, closed, (int64_t *)perm,
                                        (int64_t *)li, (int64_t *)ri, stats, &collision);
        if (rc != RFX_OK && collision) { why = "row-hash collision between two key tuples"; goto drop; }
        if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) { why = rc == RFX_ENOMEM ? "device memory" : "more rows than the device sort takes"; goto drop; }
        if (rc != RFX_OK) { res = fail(rfx_exec_last_error(g_x)); goto drop; }
        for (int k = 0; k < ncol; k++) {
            void *outs[RFX_WAGG_N] = {0};
            for (int i = 0; i < nagg; i++)
                if (aggcol[i] == k) {
                    if (!dout[agg[i]] && op_scratch(&dout[agg[i]], (size_t)nl * 8) != RFX_OK) { why = "device memory"; goto drop; }
                    outs[agg[i]] = dout[agg[i]];
                }
            if (resident(vcol[k], 0, &dv) != RFX_OK) { res = fail_hip("column upload"); goto drop; }
            rc = rfx_exec_window_fold(g_x, dv, col_ctype(vcol[k]), (const int64_t *)perm, (const int64_t *)li, (const int64_t *)ri, nl, nr, stats[0], outs);
            if (rc == RFX_ENOMEM) { why = "device memory"; goto drop; }
            if (rc != RFX_OK) { res = fail(rfx_exec_last_error(g_x)); goto drop; }
            for (int i = 0; i < nagg; i++)
                if (aggcol[i] == k && rfx_hip_d2h(g_ctx, RFX_AS_RAW(RFX_AS_LIST(cols)[lnames->len + i]), outs[agg[i]], (size_t)nl * 8) != RFX_OK) {
                    res = fail_hip("window join result");
                    goto drop;
                }
        }
    }
    g_last_window_gpu = 1;
    return H.table(names, cols);
drop:
    H.drop(names);
    H.drop(cols);
    return why ? window_host(closed, x, n, why) : res;
}
static obj_p window_door(int closed, obj_p *x, int64_t n) {
    op_begin();
    g_window_handed = 0;
    obj_p r = window_impl(closed, x, n);
    /* (an empty left table is answered here without the device and without the host: neither counter) */
    if (g_last_window_gpu) g_stat[ST_JOIN_GPU]++;
    else if (g_window_handed) g_stat[ST_JOIN_DELEGATED]++;
    op_end();
    return r;
}
rfx_obj_p rfx_window_join(rfx_obj_p *x, int64_t n) { return window_door(0, x, n); }
rfx_obj_p rfx_window_join1(rfx_obj_p *x, int64_t n) { return window_door(1, x, n); }
