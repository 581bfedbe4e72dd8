/* rfx_ops_cols.c -- part of the operator layer's ONE translation unit (rfx_ops.c #includes it -- the Makefile does not compile it on its own).
 * What the column-moving verbs share (rows, cast, bucket, concat / raze, upsert / insert, row / collect): a type's cell, an atom's cell, which device
 * handles a verb takes, a column's cells on the device in their own width, the life of a result column, and a failed call's way to the host. */
/* bytes of one cell of a type the column verbs take (0: another type) */
static int cell_width(int type) { return type == RFX_TYPE_SYMBOL ? 8 : (int)cell_bytes(type); }
/* an atom's cell in the low `width` bytes (an f64 atom's bits share the union) */
static uint64_t atom_cell_bits(obj_p a, int width) {
    return width == 8 ? (uint64_t)a->i64 : (width == 4 ? (uint64_t)(uint32_t)a->i32 : (width == 2 ? (uint64_t)(uint16_t)a->i16 : (uint64_t)a->u8));
}
/* NULL: not a device handle, or one the verb takes; else why not.  narrow_ok: the verb reads the cells as they are, and only I32 / DATE / TIME -- whose
 * resident form would be the widened image, which a handle is not -- are refused */
static const char *device_handle_why(obj_p v, int narrow_ok) {
    if (v->mmod != RFX_MMOD_DEVICE) return NULL;
    if (narrow_ok) return IS_I32_FAMILY(v->type) ? "a 4-byte device column" : NULL;
    return cell_width(v->type) != 8 && v->type != RFX_TYPE_B8 ? "a device column that is not I64 / F64 / TIMESTAMP / B8" : NULL;
}
/* NULL: a vector the write verbs (concat / raze, upsert / insert) take; else why not */
static const char *cells_vec_why(obj_p v) {
    if (IS_PARTED_TYPE(v->type)) return "a parted column";
    if (!cell_width(v->type)) return "not a vector of a concat type";
    return device_handle_why(v, 0);
}
/* a column's cells on the device, in the column's own width: the resident copy of an 8-byte or B8 column (and of a device handle), else -- U8, I16,
 * I32 / DATE / TIME, of which the cache keeps no such copy -- an upload: into the next cells of the caller's staging block `*stage`, or, without one,
 * into a block of the call's scratch */
static int native_cells(obj_p v, int width, char **stage, const void **d) {
    if (width == 8 || v->type == RFX_TYPE_B8 || v->mmod == RFX_MMOD_DEVICE) return resident(v, 0, d);
    const size_t bytes = (size_t)v->len * (size_t)width;
    void *st = NULL;
    int rc = RFX_OK;
    if (stage) st = *stage, *stage += bytes;
    else rc = op_scratch(&st, bytes);
    g_stat[ST_UPLOADS]++;
    *d = st;
    return rc == RFX_OK ? rfx_hip_h2d_pipelined(g_ctx, st, RFX_AS_RAW(v), bytes) : rc;
}

/* ---- a result column: the fresh host vector, its device buffer, the buffer's bytes ----
 * THE RESULT INHERITS RESIDENCY: the buffer of an I64 / SYMBOL / TIMESTAMP / F64 / B8 column is not freed but entered into the residency cache as the copy
 * of the fresh vector (res_col_adopt), in the form resident() keeps for that type, so that a later operator over the answer uploads nothing.  I32 / DATE /
 * TIME results are not adopted (the cache keeps their widened 8-byte image, which these copies do not make), I16 / U8 are never resident.
 * RFX_CONCAT_ADOPT=0 turns adoption off. */
typedef struct { obj_p out; void *d; size_t bytes; } res_col_t;
static int res_col_adopts(int type) {
    return type == RFX_TYPE_I64 || type == RFX_TYPE_SYMBOL || type == RFX_TYPE_TIMESTAMP || type == RFX_TYPE_F64 || type == RFX_TYPE_B8;
}
static int res_col_adopt_on(void) {
    const char *e = getenv("RFX_CONCAT_ADOPT");
    return !(e && atoi(e) == 0);
}
/* does this vector travel in a staging block?  (a host vector whose cells the cache would not keep as they are: U8, I16, I32 / DATE / TIME) */
static int cells_staged(obj_p p) { return p->type > 0 && p->len > 0 && p->mmod != RFX_MMOD_DEVICE && !res_col_adopts(p->type); }
/* the buffer becomes the cached copy of the vector it was read back into: what resident() would have made by an upload, without one.  The cache holds
 * its reference (or, in checksum mode, the payload's checksum) exactly as for an uploaded column; the scope fields stay unset */
static void res_col_adopt(const res_col_t *r) {
    resident_t e;
    memset(&e, 0, sizeof(e));
    const int own = validate_mode() == 0;
    e.host = RFX_AS_RAW(r->out); e.len = r->out->len; e.type = r->out->type; e.dev = r->d; e.bytes = r->bytes; e.dbytes = r->bytes; e.tick = ++g_tick; e.epoch = g_epoch;
    e.sum = own ? 0 : payload_sum(e.host, r->bytes);
    e.owner = own ? H.clone(r->out) : NULL;
    e.devs[0] = r->d;
    res_append(&e);
}
/* the buffer of `out` (a vector with cells): room in the cache first where the column will be adopted */
static int res_col_alloc(res_col_t *r, obj_p out, int width, int adopt) {
    r->out = out;
    r->bytes = (size_t)out->len * (size_t)width;
    if (adopt && res_col_adopts(out->type)) res_make_room(r->bytes);
    return rfx_hip_malloc(g_ctx, &r->d, r->bytes);
}
static int res_cols_read(const res_col_t *r, int64_t n) {
    int rc = RFX_OK;
    for (int64_t k = 0; k < n && rc == RFX_OK; k++)
        if (r[k].d) rc = rfx_hip_d2h(g_ctx, RFX_AS_RAW(r[k].out), r[k].d, r[k].bytes);
    return rc;
}
/* the end of the buffers, whatever `rc` the call came to: adopted, or back to the pool */
static void res_cols_finish(const res_col_t *r, int64_t n, int rc, int adopt) {
    if (rc != RFX_OK) rfx_hip_ctx_sync(g_ctx); /* (a kernel may still be writing the blocks that go back to the pool) */
    for (int64_t k = 0; k < n; k++) {
        if (!r[k].d) continue;
        if (rc == RFX_OK && adopt && res_col_adopts(r[k].out->type)) res_col_adopt(&r[k]);
        else rfx_hip_free(g_ctx, r[k].d);
    }
}
/* a run that stopped early leaves the later slots of the answer's column list without a vector */
static void res_fill_empty(obj_p list) {
    for (int64_t k = 0; k < list->len; k++)
        if (!RFX_AS_LIST(list)[k]) RFX_AS_LIST(list)[k] = H.vector(RFX_TYPE_I64, 0);
}

/* ---- a failed call ----
 * why a call goes to the host after RFX_ENOMEM / RFX_ELIMIT, by the step that answered it: the call's scratch list, a column's upload, the planner */
enum { OP_AT_SCRATCH, OP_AT_UPLOAD, OP_AT_PLANNER };
static const char *op_limit_why(int rc, int at, const char *sharded) {
    if (rc == RFX_ENOMEM) return "device memory";
    if (at == OP_AT_SCRATCH) return "the call's device scratch list is full";
    if (at == OP_AT_UPLOAD) return "a column the residency cache does not take";
    return strstr(rfx_exec_last_error(g_x), "sharded") ? sharded : "a limit of the planner";
}
/* (rc != RFX_OK, at) as the verb's answer: the hand-off with its reason (x, n: the call as it came), or the failure */
static obj_p op_outcome(int f, obj_p *x, int64_t n, int rc, int at, const char *sharded, const char *verb) {
    const int arity = VERB[f].type == RFX_TYPE_UNARY ? 1 : (VERB[f].type == RFX_TYPE_BINARY ? 2 : 0);
    if (rc == RFX_ELIMIT && g_nshards > 1) return hand_off(f, NULL, 0, arity, x, n, sharded);
    if (rc == RFX_ENOMEM || rc == RFX_ELIMIT) return hand_off(f, NULL, 0, arity, x, n, op_limit_why(rc, at, sharded));
    if (rc == RFX_EHIP && !g_ctx) return fail_hip("no usable MI355X");
    if (at == OP_AT_UPLOAD) return fail_hip("column upload");
    if (at == OP_AT_PLANNER && rfx_exec_last_error(g_x)[0]) return fail(rfx_exec_last_error(g_x));
    return fail_hip(verb);
}
