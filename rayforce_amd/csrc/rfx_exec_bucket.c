/* rfx_exec_bucket.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The bucket verbs: xrank (a sort + the fused scatter, or the attribute's formula alone; one shard), and the element-wise maps xbar / floor / ceil /
 * round / neg / within, which run over every shard's rows (rfx_exec_split) like the arithmetic verbs: no shard reads another's cells. */
int rfx_exec_xrank(rfx_exec_t *x, const void *d_col, int32_t type, int attrs, int64_t n, int64_t nb, int64_t *d_out) {
    if (!x || n < 0 || nb <= 0 || (n > 0 && !d_out)) return RFX_EINVAL;
    x->err[0] = 0;
    if (x->nshards > 1 || x->has_tr) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: xrank over a sharded table");
        return RFX_ELIMIT;
    }
    if (n == 0) return RFX_OK; /* (nothing is divided) */
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    int rc;
    if (attrs & (RFX_XRANK_ASC | RFX_XRANK_DESC)) { /* the attribute is trusted, not the data: ascending wins when both are set (core/order.c:627-636) */
        rc = rfx_hip_xrank_sorted(c, n, nb, !(attrs & RFX_XRANK_ASC), d_out);
        if (rc == RFX_OK) { x->stat[RFX_XSTAT_XRANKS]++; x->stat[RFX_XSTAT_XRANK_SORTED]++; }
        else snprintf(x->err, sizeof(x->err), "rfx_exec: xrank: %s", rfx_hip_last_error());
        return rc;
    }
    if (!d_col) return RFX_EINVAL;
    void *perm = NULL;
    if ((rc = rfx_hip_malloc(c, &perm, (size_t)n * 8)) != RFX_OK) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: xrank: %s", rfx_hip_last_error());
        return rc;
    }
    const void *cols[1] = {d_col};
    rc = rfx_exec_sort(x, cols, &type, 1, 0, n, (int64_t *)perm);
    if (rc == RFX_OK && (rc = rfx_hip_xrank(c, (const int64_t *)perm, n, nb, d_out)) != RFX_OK) snprintf(x->err, sizeof(x->err), "rfx_exec: xrank: %s", rfx_hip_last_error());
    if (rc == RFX_OK) x->stat[RFX_XSTAT_XRANKS]++;
    rfx_hip_ctx_sync(c); /* (the permutation goes back to the pool: the scatter must have read it) */
    rfx_hip_free(c, perm);
    return rc;
}

/* ray_xbar_partial's arms by (|x type|, |y type|), the reference's type codes (core/rayforce.h:51-60): the operands' storage, the middle type the formula
 * runs in, the result's type code (infer_xbar_type, core/math.c:225-249) and width */
enum { XT_I32 = 4, XT_I64 = 5, XT_DATE = 7, XT_TIME = 8, XT_TIMESTAMP = 9, XT_F64 = 10 };
static int32_t xbar_storage(int t) { return (t == XT_I32 || t == XT_DATE || t == XT_TIME) ? RFX_I32 : (t == XT_F64 ? RFX_F64 : RFX_I64); }
int rfx_exec_xbar_plan(int x_type, int y_type, rfx_xbar_desc_t *desc, int *out_type) {
    if (!desc || !out_type) return RFX_EINVAL;
    int mid = 0, ot = 0, y_time = 0;
    const int yi = y_type == XT_I32 || y_type == XT_I64;
    switch (x_type) {
        case XT_I32:
            if (y_type == XT_I32) { mid = RFX_I32; ot = XT_I32; }
            else if (y_type == XT_I64) { mid = RFX_I64; ot = XT_I64; }
            else if (y_type == XT_F64) { mid = RFX_F64; ot = XT_F64; }
            break;
        case XT_I64:
            if (yi) { mid = RFX_I64; ot = XT_I64; }
            else if (y_type == XT_F64) { mid = RFX_F64; ot = XT_F64; }
            break;
        case XT_F64:
            if (yi || y_type == XT_F64) { mid = RFX_F64; ot = XT_F64; }
            break;
        case XT_DATE:
            if (yi) { mid = y_type == XT_I32 ? RFX_I32 : RFX_I64; ot = XT_DATE; }
            break;
        case XT_TIME:
            if (y_type == XT_I32 || y_type == XT_TIME) { mid = RFX_I32; ot = XT_TIME; }
            else if (y_type == XT_I64) { mid = RFX_I64; ot = XT_TIME; }
            break;
        case XT_TIMESTAMP:
            if (yi) { mid = RFX_I64; ot = XT_TIMESTAMP; }
            else if (y_type == XT_TIME) { mid = RFX_I64; ot = XT_TIMESTAMP; y_time = 1; }
            break;
        default: break;
    }
    if (!ot) return RFX_EINVAL;
    desc->x_type = xbar_storage(x_type);
    desc->y_type = xbar_storage(y_type);
    desc->mid = mid;
    desc->y_time = y_time;
    desc->out_bytes = xbar_storage(ot) == RFX_I32 ? 4 : 8;
    *out_type = ot;
    return RFX_OK;
}

/* one element-wise map over shard `shard`'s n rows (shard >= 0: the operator layer's piece), or over every shard's rows of an n-row column (shard < 0) */
typedef int (*bucket_piece_fn)(rfx_exec_t *x, const void *arg, int s, int64_t n);
static int bucket_map(rfx_exec_t *x, bucket_piece_fn fn, const void *arg, int64_t n, int shard, const char *what) {
    if (!x || n < 0 || shard >= x->nshards) return RFX_EINVAL;
    x->err[0] = 0;
    int rc = RFX_OK;
    if (shard >= 0) rc = fn(x, arg, shard, n);
    else {
        for (int s = 0; s < x->nshards && rc == RFX_OK; s++) {
            int64_t r0, len;
            rfx_exec_split(n, x->nshards, s, &r0, &len);
            if (len <= 0) continue;
            if (x->nshards > 1) rfx_hip_ctx_bind_thread(x->ctx[s]);
            rc = fn(x, arg, s, len);
        }
        if (x->nshards > 1) {
            for (int s = 0; s < x->nshards; s++) { /* everything enqueued, then one wait per shard */
                rfx_hip_ctx_bind_thread(x->ctx[s]);
                const int src = rfx_hip_ctx_sync(x->ctx[s]);
                if (rc == RFX_OK) rc = src;
            }
            rfx_hip_ctx_bind_thread(x->ctx[0]);
        }
    }
    if (rc == RFX_OK) x->stat[RFX_XSTAT_BUCKET_MAPS]++;
    else snprintf(x->err, sizeof(x->err), "rfx_exec: %s: %s", what, rfx_hip_last_error());
    return rc;
}
#define PIECE(a, s) ((a) ? (a)[s] : NULL)
typedef struct { const rfx_xbar_desc_t *d; const void *const *xs, *const *ys; void *const *outs; } xbar_job_t;
static int xbar_piece(rfx_exec_t *x, const void *arg, int s, int64_t n) {
    const xbar_job_t *j = (const xbar_job_t *)arg;
    rfx_xbar_desc_t d = *j->d;
    d.d_x = PIECE(j->xs, s);
    d.d_y = PIECE(j->ys, s);
    return rfx_hip_xbar(x->ctx[s], &d, n, j->outs[s]);
}
int rfx_exec_xbar(rfx_exec_t *x, const rfx_xbar_desc_t *desc, const void *const *d_xs, const void *const *d_ys, int64_t n, void *const *d_outs, int shard) {
    if (!desc || !d_outs || (!d_xs && !d_ys)) return RFX_EINVAL;
    const xbar_job_t j = {desc, d_xs, d_ys, d_outs};
    return bucket_map(x, xbar_piece, &j, n, shard, "xbar");
}
typedef struct { int op; int32_t type; int64_t lo, hi; const void *const *ins; void *const *outs; } unary_job_t;
static int round_piece(rfx_exec_t *x, const void *arg, int s, int64_t n) {
    const unary_job_t *j = (const unary_job_t *)arg;
    return rfx_hip_round_f64(x->ctx[s], j->op, (const double *)j->ins[s], n, (double *)j->outs[s]);
}
static int neg_piece(rfx_exec_t *x, const void *arg, int s, int64_t n) {
    const unary_job_t *j = (const unary_job_t *)arg;
    return rfx_hip_neg(x->ctx[s], j->type, j->ins[s], n, j->outs[s]);
}
static int within_piece(rfx_exec_t *x, const void *arg, int s, int64_t n) {
    const unary_job_t *j = (const unary_job_t *)arg;
    return rfx_hip_within_i64(x->ctx[s], (const int64_t *)j->ins[s], j->lo, j->hi, n, (int8_t *)j->outs[s]);
}
int rfx_exec_round(rfx_exec_t *x, int op, const void *const *d_ins, int64_t n, void *const *d_outs, int shard) {
    if (!d_ins || !d_outs) return RFX_EINVAL;
    const unary_job_t j = {op, RFX_F64, 0, 0, d_ins, d_outs};
    return bucket_map(x, round_piece, &j, n, shard, op == RFX_ROUND_FLOOR ? "floor" : (op == RFX_ROUND_CEIL ? "ceil" : "round"));
}
int rfx_exec_neg(rfx_exec_t *x, int32_t type, const void *const *d_ins, int64_t n, void *const *d_outs, int shard) {
    if (!d_ins || !d_outs) return RFX_EINVAL;
    const unary_job_t j = {0, type, 0, 0, d_ins, d_outs};
    return bucket_map(x, neg_piece, &j, n, shard, "neg");
}
int rfx_exec_within(rfx_exec_t *x, const void *const *d_cols, int64_t lo, int64_t hi, int64_t n, void *const *d_masks, int shard) {
    if (!d_cols || !d_masks) return RFX_EINVAL;
    const unary_job_t j = {0, RFX_I64, lo, hi, d_cols, d_masks};
    return bucket_map(x, within_piece, &j, n, shard, "within");
}
#undef PIECE
