/* rfx_ops_bucket.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * The bucket verbs as built-ins of their own: xrank (ray_xrank, core/order.c:598-649), xbar (ray_xbar, core/math.c:1635-1782,2442), within (ray_within,
 * core/items.c:848-872), floor / ceil / round (core/math.c:2047-2117,2430-2432), neg (ray_neg, core/order.c:445-497) on the device (rfx_bucket.hip through
 * rfx_exec_bucket.c).
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c): a shape the device does not take is the host's own verb when a host is bound, else an error object
 * naming the reason (also in rfx_ops_last_error()).  Every result is a fresh host vector with the reference's result type; nothing is written in place. */
static int g_last_bucket_gpu = 0;
int rfx_last_bucket_on_gpu(void) { return g_last_bucket_gpu; }

static obj_p bucket_host(int f, obj_p x, obj_p y, const char *why) {
    g_last_bucket_gpu = 0;
    return hand_off_xy(f, NULL, x, y, why);
}
static int bucket_is_device(obj_p v) { return v->mmod == RFX_MMOD_DEVICE; }

/* ---- xrank ---- */
static obj_p xrank_impl(obj_p v, obj_p nobj) {
    rfx_host_bind();
    if (!v || !nobj) return fail("xrank: null argument");
    g_last_bucket_gpu = 0;
    int64_t nb;
    switch (nobj->type) { /* (core/order.c:602-617) */
        case -RFX_TYPE_I64: nb = nobj->i64; break;
        case -RFX_TYPE_I32: nb = nobj->i32; break;
        case -RFX_TYPE_I16: nb = nobj->i16; break;
        case -RFX_TYPE_U8: nb = nobj->u8; break;
        default: return bucket_host(F_XRANK, v, nobj, "bucket count type");
    }
    if (nb <= 0) return bucket_host(F_XRANK, v, nobj, "domain"); /* (err_domain is the host's to raise) */
    if (!(v->type > 0 && sort_key_type(v))) return bucket_host(F_XRANK, v, nobj, "key type");
    const int64_t n = v->len;
    if (n == 0) { /* nothing is divided */
        g_last_bucket_gpu = 1;
        return H.vector(RFX_TYPE_I64, 0);
    }
    if ((unsigned __int128)(n - 1) * (unsigned __int128)nb >= ((unsigned __int128)1 << 63)) return bucket_host(F_XRANK, v, nobj, "(len - 1) * n does not fit 63 bits");
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return bucket_host(F_XRANK, v, nobj, "xrank over a sharded table");
    const int attrs = v->attrs & (ATTR_ASC_ | ATTR_DESC_);
    const void *dv = NULL;
    void *d0 = NULL;
    if (!attrs && resident(v, 0, &dv) != RFX_OK) return fail_hip("column upload");
    int rc = op_scratch(&d0, (size_t)n * 8);
    if (rc == RFX_OK) rc = rfx_exec_xrank(g_x, dv, col_ctype(v), attrs, n, nb, (int64_t *)d0);
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return bucket_host(F_XRANK, v, nobj, rc == RFX_ENOMEM ? "device memory" : "more rows than the device sort takes");
    if (rc != RFX_OK) return fail_hip("xrank");
    obj_p out = H.vector(RFX_TYPE_I64, n);
    if (rfx_hip_d2h(g_ctx, RFX_AS_RAW(out), d0, (size_t)n * 8) != RFX_OK) {
        H.drop(out);
        return fail_hip("xrank result");
    }
    g_last_bucket_gpu = 1;
    return out;
}

/* ---- the element-wise verbs: every shard maps its rows (map_shards), its piece of the result lands in the host vector at the piece's offset ---- */
typedef struct {
    int verb; /* 0 xbar, 1 floor / ceil / round, 2 neg, 3 within */
    rfx_xbar_desc_t d;
    int op;
    int32_t type;
    int64_t lo, hi;
    const void *xs[RFX_MAX_SHARDS], *ys[RFX_MAX_SHARDS];
    int has_x, has_y;
} bucket_arg_t;
static int bucket_piece(void *arg, int s, int64_t r0, int64_t n, void *d_out) {
    bucket_arg_t *A = (bucket_arg_t *)arg;
    (void)r0; /* (the operands' pieces are addressed per shard already) */
    void *outs[RFX_MAX_SHARDS] = {0};
    outs[s] = d_out;
    switch (A->verb) {
        case 0: return rfx_exec_xbar(g_x, &A->d, A->has_x ? A->xs : NULL, A->has_y ? A->ys : NULL, n, outs, s);
        case 1: return rfx_exec_round(g_x, A->op, A->xs, n, outs, s);
        case 3: return rfx_exec_within(g_x, A->xs, A->lo, A->hi, n, outs, s);
        default: break;
    }
    return rfx_exec_neg(g_x, A->type, A->xs, n, outs, s);
}
static obj_p bucket_run(bucket_arg_t *A, int8_t out_type, size_t esz, int64_t n, const char *what) {
    obj_p out = H.vector(out_type, n);
    if (n > 0 && map_shards(out, esz, bucket_piece, A) != RFX_OK) {
        H.drop(out);
        char b[300];
        snprintf(b, sizeof(b), "%s: %s", what, rfx_exec_last_error(g_x));
        return fail_hip(b);
    }
    g_last_bucket_gpu = 1;
    return out;
}
/* the shards' pieces of a vector operand (uploaded if need be); a piece that is missing goes to the planner as the NULL it is */
static int bucket_operand(obj_p v, const void **pieces) {
    const int rc = col_pieces(v, pieces);
    return rc == COL_PIECE_MISSING ? RFX_OK : rc;
}

/* an atom operand's cell: 4 bytes of an I32 / DATE / TIME atom, else the union's 8 */
static uint64_t bucket_atom_bits(obj_p a) { return atom_cell_bits(a, IS_I32_FAMILY(-a->type) ? 4 : 8); }
static obj_p xbar_impl(obj_p x, obj_p y) {
    rfx_host_bind();
    if (!x || !y) return fail("xbar: null argument");
    g_last_bucket_gpu = 0;
    const int xv = x->type > 0, yv = y->type > 0;
    if (!xv && !yv) return bucket_host(F_XBAR, x, y, "atom and atom");
    bucket_arg_t A;
    memset(&A, 0, sizeof(A));
    int ot = 0;
    if (rfx_exec_xbar_plan(xv ? x->type : -x->type, yv ? y->type : -y->type, &A.d, &ot) != RFX_OK) return bucket_host(F_XBAR, x, y, "operand types");
    if (xv && yv && x->len != y->len) return bucket_host(F_XBAR, x, y, "length"); /* (err_length is the host's to raise) */
    const char *why = xv ? device_handle_why(x, 1) : NULL;
    if (!why && yv) why = device_handle_why(y, 1);
    if (why) return bucket_host(F_XBAR, x, y, why);
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    A.verb = 0;
    A.has_x = xv;
    A.has_y = yv;
    if (xv) {
        if (bucket_operand(x, A.xs) != RFX_OK) return fail_hip("column upload");
        if (A.d.x_type == RFX_I32) A.d.widened |= 1;
    } else A.d.x_atom = bucket_atom_bits(x);
    if (yv) {
        if (bucket_operand(y, A.ys) != RFX_OK) return fail_hip("column upload");
        if (A.d.y_type == RFX_I32) A.d.widened |= 2;
    } else A.d.y_atom = bucket_atom_bits(y);
    return bucket_run(&A, (int8_t)ot, (size_t)A.d.out_bytes, xv ? x->len : y->len, "xbar");
}

static obj_p round_impl(int op, int f, obj_p x) {
    rfx_host_bind();
    if (!x) return fail("round: null argument");
    g_last_bucket_gpu = 0;
    if (x->type != RFX_TYPE_F64) return bucket_host(f, x, NULL, x->type < 0 ? "an atom" : "not an F64 vector"); /* (the integer and temporal arms are clone_obj) */
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    bucket_arg_t A;
    memset(&A, 0, sizeof(A));
    A.verb = 1;
    A.op = op;
    if (bucket_operand(x, A.xs) != RFX_OK) return fail_hip("column upload");
    return bucket_run(&A, RFX_TYPE_F64, 8, x->len, VERB[f].host + 4);
}
static obj_p neg_impl(obj_p x) {
    rfx_host_bind();
    if (!x) return fail("neg: null argument");
    g_last_bucket_gpu = 0;
    if (x->type != RFX_TYPE_I32 && x->type != RFX_TYPE_I64 && x->type != RFX_TYPE_F64) return bucket_host(F_NEG, x, NULL, x->type < 0 ? "an atom" : "not an I32 / I64 / F64 vector");
    const char *why = device_handle_why(x, 1);
    if (why) return bucket_host(F_NEG, x, NULL, why);
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    bucket_arg_t A;
    memset(&A, 0, sizeof(A));
    A.verb = 2;
    A.type = x->type == RFX_TYPE_I32 ? RFX_I32_WIDE : col_ctype(x); /* (the resident copy of a 4-byte column is its widened image, as for xbar) */
    if (bucket_operand(x, A.xs) != RFX_OK) return fail_hip("column upload");
    return bucket_run(&A, x->type == RFX_TYPE_F64 ? RFX_TYPE_F64 : RFX_TYPE_I64, 8, x->len, "neg"); /* (I32 and I64 both answer I64, core/order.c:474-485) */
}
static obj_p within_impl(obj_p x, obj_p y) {
    rfx_host_bind();
    if (!x || !y) return fail("within: null argument");
    g_last_bucket_gpu = 0;
    /* all the reference itself answers over a vector: I64 cells against a 2-cell I64 vector; everything else raises the host's own type error */
    if (!(x->type == RFX_TYPE_I64 && y->type == RFX_TYPE_I64 && y->len == 2 && !bucket_is_device(y))) return bucket_host(F_WITHIN, x, y, "not an I64 vector against a 2-cell I64 vector");
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    bucket_arg_t A;
    memset(&A, 0, sizeof(A));
    A.verb = 3;
    A.lo = RFX_AS_I64(y)[0];
    A.hi = RFX_AS_I64(y)[1];
    if (bucket_operand(x, A.xs) != RFX_OK) return fail_hip("column upload");
    return bucket_run(&A, RFX_TYPE_B8, 1, x->len, "within");
}

OP2(rfx_xrank, xrank_impl(x, y))
OP2(rfx_xbar, xbar_impl(x, y))
OP2(rfx_within, within_impl(x, y))
OP1(rfx_floor, round_impl(RFX_ROUND_FLOOR, F_FLOOR, x))
OP1(rfx_ceil, round_impl(RFX_ROUND_CEIL, F_CEIL, x))
OP1(rfx_round, round_impl(RFX_ROUND_ROUND, F_ROUND, x))
OP1(rfx_neg, neg_impl(x))
