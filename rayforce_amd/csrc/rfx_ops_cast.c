/* rfx_ops_cast.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * `as` as a built-in of its own (ray_cast_obj, core/compose.c:42-68 -> cast_obj, core/rayforce.c:2312-2831): a vector of one of the nine numeric and
 * temporal types cast to another of them on the device (rfx_cast.hip through rfx_exec_cast.c).
 * The hand-off is the shared one (hand_off, rfx_ops_plan.c): a shape the device does not
 * take is the host's own verb when a host is bound, else an error object naming the reason (also in rfx_ops_last_error()).  A converted result is a
 * fresh host vector of the target type, attribute byte 0; the same type is a clone of the argument, as the reference answers it. */
static int g_last_cast_gpu = 0;
int rfx_last_cast_on_gpu(void) { return g_last_cast_gpu; }

static obj_p cast_host(obj_p t, obj_p x, const char *why) {
    g_last_cast_gpu = 0;
    return hand_off_xy(F_AS, "as", t, x, why); /* (the host's symbol is ray_cast_obj: the verb's own name is passed in) */
}
/* the nine types by either spelling of their names (the atom's 'i32 is flipped to the vector's 'I32 when the source is a vector, core/compose.c:53-65);
 * 0: another name */
static int cast_type_of(int64_t sym) {
    static const struct { const char *atom, *vec; int type; } T[] = {
        {"b8", "B8", RFX_TYPE_B8}, {"u8", "U8", RFX_TYPE_U8}, {"i16", "I16", RFX_TYPE_I16}, {"i32", "I32", RFX_TYPE_I32}, {"i64", "I64", RFX_TYPE_I64},
        {"f64", "F64", RFX_TYPE_F64}, {"date", "DATE", RFX_TYPE_DATE}, {"time", "TIME", RFX_TYPE_TIME}, {"timestamp", "TIMESTAMP", RFX_TYPE_TIMESTAMP}};
    const char *s = H.symname(sym);
    if (!s) return 0;
    for (size_t i = 0; i < sizeof(T) / sizeof(T[0]); i++)
        if (strcmp(s, T[i].atom) == 0 || strcmp(s, T[i].vec) == 0) return T[i].type;
    return 0;
}
typedef struct {
    int32_t src_type, dst_type;
    const void *xs[RFX_MAX_SHARDS];
} cast_arg_t;
static int cast_piece(void *arg, int s, int64_t r0, int64_t n, void *d_out) {
    cast_arg_t *A = (cast_arg_t *)arg;
    (void)r0; /* (the source's pieces are addressed per shard already) */
    void *outs[RFX_MAX_SHARDS] = {0};
    outs[s] = d_out;
    return rfx_exec_cast(g_x, A->src_type, A->dst_type, A->xs, n, outs, s);
}
static obj_p cast_impl(obj_p t, obj_p x) {
    rfx_host_bind();
    if (!t || !x) return fail("as: null argument");
    g_last_cast_gpu = 0;
    if (t->type != -RFX_TYPE_SYMBOL) return cast_host(t, x, "the type name is not a symbol atom"); /* (err_type is the host's to raise) */
    const int dst = cast_type_of(t->i64);
    if (!dst) return cast_host(t, x, "a type name outside the nine numeric and temporal types");
    if (x->type < 0) return cast_host(t, x, "an atom");
    const size_t ssz = cell_bytes(x->type), dsz = cell_bytes(dst);
    if (!ssz) return cast_host(t, x, "not a vector of the nine numeric and temporal types");
    const int device = x->mmod == RFX_MMOD_DEVICE;
    const char *why = device_handle_why(x, 0);
    if (why) return cast_host(t, x, why);
    if (x->type == dst) { /* clone_obj: the same object, attributes kept; nothing runs */
        g_last_cast_gpu = 1;
        return H.clone(x);
    }
    const int64_t n = x->len;
    if (n == 0) { /* (before the arms are looked at, core/rayforce.c:2324-2325) */
        g_last_cast_gpu = 1;
        return H.vector((int8_t)dst, 0);
    }
    if (!rfx_hip_cast_arm(x->type, dst)) return cast_host(t, x, "the reference has no cast between B8 and U8 vectors"); /* (its err_type) */
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    cast_arg_t A;
    memset(&A, 0, sizeof(A));
    A.src_type = x->type;
    A.dst_type = dst;
    int rc;
    if (x->type == RFX_TYPE_U8 || x->type == RFX_TYPE_I16) rc = raw_pieces(x, ssz, A.xs);
    else {
        rc = col_pieces(x, A.xs);
        if (rc == COL_PIECE_MISSING) rc = RFX_ELIMIT;
        if (!device && IS_I32_FAMILY(x->type)) A.src_type |= RFX_CAST_WIDENED; /* (the resident copy of a 4-byte column is its widened image) */
    }
    if (rc != RFX_OK) {
        if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return cast_host(t, x, rc == RFX_ENOMEM ? "device memory" : "a column the residency cache does not take");
        return fail_hip("column upload");
    }
    obj_p out = H.vector((int8_t)dst, n);
    rc = map_shards(out, dsz, cast_piece, &A);
    if (rc != RFX_OK) {
        H.drop(out);
        if (rc == RFX_ENOMEM) return cast_host(t, x, "device memory");
        char b[300];
        snprintf(b, sizeof(b), "as: %s", rfx_exec_last_error(g_x));
        return fail_hip(b);
    }
    out->attrs = 0;
    g_last_cast_gpu = 1;
    return out;
}
OP2(rfx_as, cast_impl(x, y))
