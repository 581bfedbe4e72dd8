/* rfx_ops_sort.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * iasc / idesc / asc / desc / rank / xasc / xdesc (core/order.c:32-556, core/sort.c:430-479,691-740) over I64 / TIMESTAMP / F64 keys on the device
 * (rfx_sort.hip through rfx_exec_sort).  The five vector verbs also take I32 / DATE / TIME (the resident widened copy, RFX_I32_WIDE), B8 (the
 * resident 1-byte copy; B8 device-column handles too) and I16 / U8 (raw cells uploaded for the call only) -- the sort's packed-record path; asc /
 * desc answer cells of x's own width.  Every other shape -- SYMBOL keys (the reference picks id order or string order), C8, LIST / DICT / ENUM,
 * tables holding a column that is not an 8-byte vector, 4-byte xrank keys -- is the host's own verb, the reason in rfx_ops_last_error().
 * Over shards (RFX_SHARDS=k, RFX_DEVICES=all) the key columns' pieces go through rfx_exec_sort_shards: every shard sorts its rows, one stable multiway
 * merge on shard 0 (rfx_merge.hip) -- the unsharded answer bit for bit; `rank` inverts the merged permutation there, xasc / xdesc lay every batch of
 * columns end to end on shard 0's device from their pieces before the gather.  Everything decided before the device is touched is the same.
 * An I32-family vector goes over shards as its widened pieces under RFX_I64 (order and nulls survive the widening); asc / desc narrow the merged
 * 8-byte cells on shard 0 with rfx_hip_rows_take's RFX_ROWS_4W form before they leave.  I16 / U8 / B8 keys over shards are the host's verb. */
#define ATTR_DISTINCT_ 1
#define ATTR_ASC_ 2
#define ATTR_DESC_ 4
enum { SORT_IASC, SORT_IDESC, SORT_ASC, SORT_DESC, SORT_RANK };
static int g_last_sort_gpu = 0;
int rfx_last_sort_on_gpu(void) { return g_last_sort_gpu; }

static obj_p sort_host(int f, obj_p x, obj_p y, const char *why) { /* (the shared hand_off, rfx_ops_plan.c) */
    g_last_sort_gpu = 0;
    return hand_off_xy(f, NULL, x, y, why);
}
/* a resident column as the planner's per-shard pieces (a missing piece fails like an upload) */
static int sort_pieces(obj_p c, rfx_qcol_t *q) {
    memset(q, 0, sizeof(*q));
    return col_pieces(c, (const void **)q->d);
}
/* the pieces of a resident column laid end to end at d_whole on shard 0's device (n cells of 8 bytes) */
static int sort_whole(obj_p c, int64_t n, void *d_whole) {
    rfx_qcol_t q;
    int rc = sort_pieces(c, &q);
    for (int s = 0; s < g_nshards && rc == RFX_OK; s++) {
        int64_t r0, len;
        rfx_exec_split(n, g_nshards, s, &r0, &len);
        if (len > 0) rc = rfx_hip_d2d(g_ctx, (char *)d_whole + (size_t)r0 * 8, q.d[s], (size_t)len * 8);
    }
    return rc;
}
#define SORT_LIMIT_WHY (g_nshards > 1 ? "a limit of the sort over shards" : "more rows than the device sort takes")
static int sort_key_type(obj_p c) { return c->type == RFX_TYPE_I64 || c->type == RFX_TYPE_TIMESTAMP || c->type == RFX_TYPE_F64; }
/* 0..n-1 (attrs ASC | DISTINCT) or n-1..0 (DESC | DISTINCT): the order of a vector whose attribute says it is sorted already */
static obj_p sort_iota(int64_t n, int down) {
    obj_p o = H.vector(RFX_TYPE_I64, n);
    for (int64_t i = 0; i < n; i++) RFX_AS_I64(o)[i] = down ? n - 1 - i : i;
    o->attrs = (uint8_t)((down ? ATTR_DESC_ : ATTR_ASC_) | ATTR_DISTINCT_);
    return o;
}
static obj_p sort_reversed(obj_p x) { /* ray_reverse (core/compose.c:144-202): ATTR_ASC and ATTR_DESC change places, the other attributes stay */
    obj_p o = H.vector(x->type, x->len);
    const size_t w = cell_bytes(x->type);
    const char *src = (const char *)RFX_AS_RAW(x);
    char *dst = (char *)RFX_AS_RAW(o);
    for (int64_t i = 0; i < x->len; i++) memcpy(dst + (size_t)i * w, src + (size_t)(x->len - 1 - i) * w, w);
    o->attrs = (uint8_t)((x->attrs & ~(ATTR_ASC_ | ATTR_DESC_)) | ((x->attrs & ATTR_ASC_) ? ATTR_DESC_ : 0) | ((x->attrs & ATTR_DESC_) ? ATTR_ASC_ : 0));
    return o;
}
static obj_p sort_unary(int kind, int f, obj_p x) {
    rfx_host_bind();
    if (!x) return fail("sort: null argument");
    const size_t w = x->type > 0 ? cell_bytes(x->type) : 0; /* (SYMBOL, C8, LIST ...: 0) */
    if (!w) return sort_host(f, x, NULL, "key type");
    const int wide = w == 8, i32 = IS_I32_FAMILY(x->type);
    if (x->mmod == RFX_MMOD_DEVICE && !wide && x->type != RFX_TYPE_B8) return sort_host(f, x, NULL, "a device column that is not I64 / F64 / TIMESTAMP / B8");
    const int64_t n = x->len;
    const int desc = kind == SORT_IDESC || kind == SORT_DESC, values = kind == SORT_ASC || kind == SORT_DESC;
    const int sorted_up = x->attrs & ATTR_ASC_, sorted_down = x->attrs & ATTR_DESC_;
    const uint8_t out_attrs = values ? (uint8_t)((desc ? ATTR_DESC_ : ATTR_ASC_) | (x->attrs & ATTR_DISTINCT_)) : 0;
    g_last_sort_gpu = 0;
    /* the attribute is trusted, not the data (core/sort.c:430-451,691-712; core/order.c:79-83,165-169,524-538) */
    if (values) {
        if (desc ? sorted_down : sorted_up) return H.clone(x);
        if (desc ? sorted_up : sorted_down) {
            if (x->type == RFX_TYPE_I16) return sort_host(f, x, NULL, "the reference's reverse has no I16 arm"); /* (its err_type, core/compose.c:195-196) */
            return sort_reversed(x);
        }
    } else if (kind == SORT_RANK) {
        if (sorted_up) return sort_iota(n, 0); /* (ray_til: attrs ASC | DISTINCT) */
        if (sorted_down) {
            obj_p o = sort_iota(n, 1);
            o->attrs = 0;
            return o;
        }
    }
    if (n == 0) {
        obj_p o = H.vector(values ? x->type : RFX_TYPE_I64, 0);
        o->attrs = out_attrs;
        return o;
    }
    if (!values && kind != SORT_RANK) {
        if (desc ? sorted_down : sorted_up) return sort_iota(n, 0);
        if (desc ? sorted_up : sorted_down) return sort_iota(n, 1);
    }
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1 && !wide && !i32) return sort_host(f, x, NULL, "1- and 2-byte keys over shards");
    const void *dv = NULL;
    void *d0 = NULL, *d1 = NULL;
    rfx_qcol_t q;
    int rc = RFX_OK;
    int32_t type; /* as the planner takes it */
    if (x->type == RFX_TYPE_I16 || x->type == RFX_TYPE_U8) { /* (the residency cache keeps 8-byte, widened 4-byte and B8 columns: raw cells for this call only) */
        const void *raw[RFX_MAX_SHARDS]; /* (one shard here: narrow keys over shards went to the host above) */
        rc = raw_pieces(x, w, raw);
        if (rc != RFX_OK && raw[0]) return fail_hip("column upload"); /* (a failed copy; scratch that does not fit is the host's verb below) */
        dv = raw[0];
        type = x->type == RFX_TYPE_I16 ? RFX_I16 : RFX_U8;
    } else {
        if (g_nshards > 1) {
            if (sort_pieces(x, &q) != RFX_OK) return fail_hip("column upload");
        } else if (resident(x, 0, &dv) != RFX_OK) return fail_hip("column upload");
        /* (the resident copy of a 4-byte column is its widened image; over shards its pieces sort and merge as the 8-byte integers they are) */
        type = i32 ? (g_nshards > 1 ? RFX_I64 : RFX_I32_WIDE) : x->type == RFX_TYPE_B8 ? RFX_B8 : col_ctype(x);
    }
    const size_t ow = values ? w : 8; /* bytes of one cell of the answer */
    if (rc == RFX_OK) rc = op_scratch(&d0, (size_t)n * 8);
    if (rc == RFX_OK && (kind == SORT_RANK || (values && i32 && g_nshards > 1))) rc = op_scratch(&d1, (size_t)n * 8);
    const void *d_res = d0;
    if (rc == RFX_OK) {
        const void *cols[1] = {dv};
        const int32_t types[1] = {type};
        if (g_nshards > 1) rc = rfx_exec_sort_shards(g_x, &q, types, 1, desc, n, values ? NULL : (int64_t *)d0, values ? d0 : NULL); /* (the outputs on shard 0) */
        else if (values) rc = rfx_exec_sort_values(g_x, dv, types[0], desc, n, d0, NULL);
        else rc = rfx_exec_sort(g_x, cols, types, 1, desc, n, (int64_t *)d0);
        if (rc == RFX_OK && kind == SORT_RANK) rc = rfx_hip_inverse_perm(g_ctx, (const int64_t *)d0, n, (int64_t *)d1), d_res = d1;
        else if (rc == RFX_OK && d1) rc = rfx_hip_rows_take(g_ctx, d0, RFX_ROWS_4W, n, 0, n, d1), d_res = d1; /* (the merged 8-byte cells -> 4-byte cells) */
    }
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return sort_host(f, x, NULL, rc == RFX_ENOMEM ? "device memory" : SORT_LIMIT_WHY);
    if (rc != RFX_OK) return fail_hip("sort");
    obj_p out = H.vector(values ? x->type : RFX_TYPE_I64, n);
    if (rfx_hip_d2h(g_ctx, RFX_AS_RAW(out), d_res, (size_t)n * ow) != RFX_OK) {
        H.drop(out);
        return fail_hip("sort result");
    }
    out->attrs = out_attrs;
    g_last_sort_gpu = 1;
    return out;
}
static obj_p sort_table(int desc, int f, obj_p t, obj_p y) {
    rfx_host_bind();
    if (!t || !y) return fail("sort: null argument");
    g_last_sort_gpu = 0;
    if (t->type != RFX_TYPE_TABLE) return sort_host(f, t, y, "not a table");
    if ((y->type == RFX_TYPE_SYMBOL || y->type == RFX_TYPE_I64) && y->len == 0) return H.clone(t); /* an empty symbol vector or [] */
    if (y->type != -RFX_TYPE_SYMBOL && y->type != RFX_TYPE_SYMBOL) return sort_host(f, t, y, "sort columns are not symbols");
    if (is_parted_table(t)) return sort_host(f, t, y, "parted table");
    obj_p names = RFX_AS_LIST(t)[0], cols = RFX_AS_LIST(t)[1];
    const int ncol = (int)cols->len, nk = y->type < 0 ? 1 : (int)y->len;
    if (ncol < 1 || ncol > 64 || nk > 16) return sort_host(f, t, y, "too many columns");
    const int64_t n = RFX_AS_LIST(cols)[0]->len;
    for (int i = 0; i < ncol; i++) {
        obj_p c = RFX_AS_LIST(cols)[i];
        if (!(c->type > 0 && col_ctype(c)) || c->len != n) return sort_host(f, t, y, "a column that is not an 8-byte vector");
    }
    obj_p kc[16];
    for (int k = 0; k < nk; k++) {
        kc[k] = table_col(t, y->type < 0 ? y->i64 : RFX_AS_I64(y)[k]);
        if (!kc[k]) return sort_host(f, t, y, "no such column");
        if (!sort_key_type(kc[k])) return sort_host(f, t, y, "key type");
    }
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1 && nk > RFX_MAX_KEYS) return sort_host(f, t, y, "more sort columns than a sort over shards takes");
    const void *dperm = NULL;
    obj_p hperm = NULL;
    int on_gpu = 0;
    if (n > 0 && y->type < 0 && (kc[0]->attrs & (ATTR_ASC_ | ATTR_DESC_))) { /* (one symbol: ray_iasc / ray_idesc of the column itself, attribute and all) */
        const int up = (kc[0]->attrs & ATTR_ASC_) != 0;
        hperm = sort_iota(n, desc ? up : !up);
        if (transient(hperm, &dperm) != RFX_OK) {
            H.drop(hperm);
            return fail_hip("upload");
        }
    } else if (n > 0) {
        const void *dk[16];
        rfx_qcol_t qk[RFX_MAX_KEYS];
        int32_t types[16];
        void *d = NULL;
        for (int k = 0; k < nk; k++) {
            if ((g_nshards > 1 ? sort_pieces(kc[k], &qk[k]) : resident(kc[k], 0, &dk[k])) != RFX_OK) return fail_hip("column upload");
            types[k] = col_ctype(kc[k]);
        }
        int rc = op_scratch(&d, (size_t)n * 8);
        if (rc == RFX_OK) rc = g_nshards > 1 ? rfx_exec_sort_shards(g_x, qk, types, nk, desc, n, (int64_t *)d, NULL) : rfx_exec_sort(g_x, dk, types, nk, desc, n, (int64_t *)d);
        if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return sort_host(f, t, y, rc == RFX_ENOMEM ? "device memory" : SORT_LIMIT_WHY);
        if (rc != RFX_OK) return fail_hip("sort");
        dperm = d;
        on_gpu = 1;
    }
    /* every column by the final permutation, RFX_MAX_KEYS columns per launch; over shards every batch's columns are first laid end to end on shard 0's
     * device from their pieces (the second half of the batch's block) */
    const int cat = g_nshards > 1;
    obj_p rv = H.vector(RFX_TYPE_LIST, ncol);
    for (int i = 0; i < ncol; i++) RFX_AS_LIST(rv)[i] = NULL;
    int ok = 1;
    for (int c0 = 0; c0 < ncol && ok && n > 0; c0 += RFX_MAX_KEYS) {
        const int m = ncol - c0 < RFX_MAX_KEYS ? ncol - c0 : RFX_MAX_KEYS;
        const void *src[RFX_MAX_KEYS];
        void *dst[RFX_MAX_KEYS];
        void *block = NULL;
        const int brc = rfx_hip_malloc(g_ctx, &block, (size_t)m * (size_t)n * 8 * (size_t)(cat ? 2 : 1));
        if (cat && brc == RFX_ENOMEM) { /* (the whole copies double the batch's block on shard 0: no room is the host's verb, as for the sort's own scratch) */
            if (hperm) H.drop(hperm);
            for (int i = 0; i < ncol; i++)
                if (!RFX_AS_LIST(rv)[i]) RFX_AS_LIST(rv)[i] = H.vector(RFX_AS_LIST(cols)[i]->type, 0);
            H.drop(rv);
            return sort_host(f, t, y, "device memory");
        }
        ok = brc == RFX_OK;
        for (int j = 0; j < m && ok; j++) {
            dst[j] = (char *)block + (size_t)j * (size_t)n * 8;
            if (cat) {
                void *whole = (char *)block + (size_t)(m + j) * (size_t)n * 8;
                ok = sort_whole(RFX_AS_LIST(cols)[c0 + j], n, whole) == RFX_OK;
                src[j] = whole;
            } else ok = resident(RFX_AS_LIST(cols)[c0 + j], 0, &src[j]) == RFX_OK;
        }
        ok = ok && rfx_hip_gather_many(g_ctx, src, m, (const int64_t *)dperm, n, dst) == RFX_OK;
        for (int j = 0; j < m && ok; j++) {
            obj_p o = H.vector(RFX_AS_LIST(cols)[c0 + j]->type, n);
            RFX_AS_LIST(rv)[c0 + j] = o;
            ok = rfx_hip_d2h(g_ctx, RFX_AS_RAW(o), dst[j], (size_t)n * 8) == RFX_OK;
        }
        if (block) {
            rfx_hip_ctx_sync(g_ctx);
            rfx_hip_free(g_ctx, block);
        }
    }
    if (hperm) H.drop(hperm);
    for (int i = 0; i < ncol; i++)
        if (!RFX_AS_LIST(rv)[i]) RFX_AS_LIST(rv)[i] = H.vector(RFX_AS_LIST(cols)[i]->type, 0); /* (an empty table, or the cells a failure left) */
    if (!ok) {
        H.drop(rv);
        return fail_hip("sort: gather");
    }
    g_last_sort_gpu = on_gpu;
    return H.table(H.clone(names), rv);
}
OP1(rfx_iasc, sort_unary(SORT_IASC, F_IASC, x))
OP1(rfx_idesc, sort_unary(SORT_IDESC, F_IDESC, x))
OP1(rfx_asc, sort_unary(SORT_ASC, F_ASC, x))
OP1(rfx_desc, sort_unary(SORT_DESC, F_DESC, x))
OP1(rfx_rank, sort_unary(SORT_RANK, F_RANK, x))
OP2(rfx_xasc, sort_table(0, F_XASC, x, y))
OP2(rfx_xdesc, sort_table(1, F_XDESC, x, y))
