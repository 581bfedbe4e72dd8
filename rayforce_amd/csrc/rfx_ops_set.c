/* rfx_ops_set.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * distinct (ray_distinct, core/compose.c:839), find (ray_find, core/items.c:302), in (ray_in, :736), sect (:898), except (:916) and union (:1022)
 * over plain I64 / SYMBOL / TIMESTAMP vectors on the device: the planner's rfx_exec_distinct / rfx_exec_member / rfx_exec_set_filter over
 * rfx_set.hip.  Every shape outside the device path -- atoms (but except's), ENUM / MAPLIST / parted operands, 1/2/4-byte, F64, GUID and LIST
 * operands, mixed types, tables, sharded columns -- every shape the reference's own tables cannot answer and every error the
 * reference words itself is the host's own verb, the reason in rfx_ops_last_error(). */
enum { SET_DISTINCT, SET_FIND, SET_IN, SET_SECT, SET_EXCEPT, SET_UNION };
enum { SST_GPU, SST_DELEGATED, SST_ROUTE0, SST_N = SST_ROUTE0 + RFX_SET_ROUTE_ATOM + 1 }; /* see rfx_set_stats */
static int g_last_set_gpu = 0, g_last_set_route = 0;
static int64_t g_set_stat[SST_N];
int rfx_last_set_on_gpu(void) { return g_last_set_gpu; }
int rfx_last_set_route(void) { return g_last_set_route; }

static obj_p set_host(int f, obj_p x, obj_p y, const char *why) {
    g_last_set_gpu = 0;
    g_last_set_route = RFX_SET_ROUTE_NONE;
    g_set_stat[SST_DELEGATED]++;
    return hand_off_xy(f, NULL, x, y, why);
}
static int set_key_type(obj_p c) { return c->type == RFX_TYPE_I64 || c->type == RFX_TYPE_SYMBOL || c->type == RFX_TYPE_TIMESTAMP; }
/* the planner's verdict on a call: the host's verb for a shape the reference cannot answer, for scratch that does not fit and for shards */
static obj_p set_declined(int f, obj_p x, obj_p y, int rc, int route) {
    if (rc == RFX_ESTATE && route == RFX_SET_ROUTE_UNDEFINED) return set_host(f, x, y, rfx_exec_last_error(g_x));
    if (rc == RFX_ENOMEM) return set_host(f, x, y, "device memory");
    if (rc == RFX_ELIMIT) return set_host(f, x, y, rfx_exec_last_error(g_x));
    return fail(rfx_exec_last_error(g_x));
}
static obj_p set_result(int8_t type, int64_t n, const void *d, size_t esz, uint8_t attrs, int route) {
    obj_p out = H.vector(type, n);
    if (n > 0 && rfx_hip_d2h(g_ctx, RFX_AS_RAW(out), d, (size_t)n * esz) != RFX_OK) {
        H.drop(out);
        return fail_hip("set verb result");
    }
    out->attrs = attrs;
    g_last_set_gpu = 1;
    g_last_set_route = route;
    g_set_stat[SST_GPU]++;
    if (route >= 0 && route <= RFX_SET_ROUTE_ATOM) g_set_stat[SST_ROUTE0 + route]++;
    return out;
}
static obj_p set_impl(int verb, int f, obj_p x, obj_p y) {
    rfx_host_bind();
    g_last_set_gpu = 0;
    g_last_set_route = RFX_SET_ROUTE_NONE;
    const int binary = verb != SET_DISTINCT;
    if (!x || (binary && !y)) return fail("set verb: null argument");
    if (!(x->type > 0 && set_key_type(x))) return set_host(f, x, binary ? y : NULL, "the first operand is not a plain I64, SYMBOL or TIMESTAMP vector");
    const int atom = verb == SET_EXCEPT && y->type == -x->type;
    if (binary && !atom && (y->type != x->type)) return set_host(f, x, y, "the operands are not two vectors of one 8-byte integer type");
    if ((verb == SET_SECT || verb == SET_EXCEPT) && x->type == RFX_TYPE_TIMESTAMP) return set_host(f, x, y, "sect / except take I64 or SYMBOL pairs");
    const int64_t nx = x->len, ny = binary && !atom ? y->len : 0;
    if (ensure_ctx() != RFX_OK) return fail_hip("no usable MI355X");
    if (g_nshards > 1) return set_host(f, x, binary ? y : NULL, "set verb over a sharded column");
    const void *dx = NULL, *dy = NULL;
    if (nx > 0 && resident(x, 0, &dx) != RFX_OK) return fail_hip("column upload");
    if (ny > 0 && resident(y, 0, &dy) != RFX_OK) return fail_hip("column upload");
    void *dout = NULL;
    int64_t nout = 0;
    int rc, route = RFX_SET_ROUTE_NONE;
    switch (verb) {
    case SET_DISTINCT:
    case SET_UNION:
        if (op_scratch(&dout, (size_t)(nx + ny) * 8) != RFX_OK) return set_host(f, x, binary ? y : NULL, "device memory");
        rc = rfx_exec_distinct(g_x, (const int64_t *)dx, nx, (const int64_t *)dy, ny, (int64_t *)dout, &nout, &route);
        if (rc != RFX_OK) return set_declined(f, x, binary ? y : NULL, rc, route);
        return set_result(x->type, nout, dout, 8, ATTR_DISTINCT_, route);
    case SET_IN:
        if (op_scratch(&dout, (size_t)nx) != RFX_OK) return set_host(f, x, y, "device memory");
        rc = rfx_exec_member(g_x, (const int64_t *)dx, nx, (const int64_t *)dy, ny, 0, dout, &route);
        if (rc != RFX_OK) return set_declined(f, x, y, rc, route);
        return set_result(RFX_TYPE_B8, nx, dout, 1, 0, route);
    case SET_FIND:
        if (op_scratch(&dout, (size_t)ny * 8) != RFX_OK) return set_host(f, x, y, "device memory");
        rc = rfx_exec_member(g_x, (const int64_t *)dx, nx, (const int64_t *)dy, ny, 1, dout, &route);
        if (rc != RFX_OK) return set_declined(f, x, y, rc, route);
        return set_result(RFX_TYPE_I64, nx == 0 ? 0 : ny, dout, 8, 0, route); /* (an empty x: I64(0), core/index.c:1512) */
    default:
        if (op_scratch(&dout, (size_t)nx * 8) != RFX_OK) return set_host(f, x, y, "device memory");
        rc = rfx_exec_set_filter(g_x, (const int64_t *)dx, nx, (const int64_t *)dy, ny, atom, atom ? y->i64 : 0, verb == SET_SECT, (int64_t *)dout, &nout, &route);
        if (rc != RFX_OK) return set_declined(f, x, y, rc, route);
        return set_result(x->type, nout, dout, 8, 0, route);
    }
}
OP1(rfx_distinct, set_impl(SET_DISTINCT, F_DISTINCT, x, NULL))
OP2(rfx_find, set_impl(SET_FIND, F_FIND, x, y))
OP2(rfx_in, set_impl(SET_IN, F_IN, x, y))
OP2(rfx_sect, set_impl(SET_SECT, F_SECT, x, y))
OP2(rfx_except, set_impl(SET_EXCEPT, F_EXCEPT, x, y))
OP2(rfx_union, set_impl(SET_UNION, F_UNION, x, y))
/* (rfx_set_stats 0): the set verbs' counters since load as an I64 vector -- [calls answered by the device path, calls handed to the host's ray_*
 * (or refused for want of one), then the answered ones by route: nothing to look up, dense, hash, disjoint scopes, except's atom].  What a
 * drop-in test asserts to know that a set verb's answer came from the device (rfx_stats keeps its 17 cells). */
rfx_obj_p rfx_set_stats(rfx_obj_p x) {
    (void)x;
    rfx_host_bind();
    op_begin();
    obj_p out = H.vector(RFX_TYPE_I64, SST_N);
    for (int i = 0; i < SST_N; i++) RFX_AS_I64(out)[i] = g_set_stat[i];
    op_end();
    return out;
}
