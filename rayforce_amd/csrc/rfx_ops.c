/*
 * rfx_ops.c -- the drop-in operator layer (host code stays in C, as in the reference): obj_p-shaped entry points that
 * plan a RayforceDB select / where / by query onto the flat HIP ABI (rfx_hip.h).
 *
 *   rfx_select walks the select dictionary the way ray_select does (core/query.c:243-654): `from:` is evaluated through
 *   the host's eval, `where:` is an expression LIST whose head is a function object (the parser already substituted the
 *   built-in for the symbol, core/parse.c:771-772), `by:` is a column symbol, every other key is an output mapping
 *   `(aggr col)`.  Supported shapes run as <= 4 kernel launches on HBM-resident columns; anything else goes back to
 *   the host's own ray_select (plugin mode) -- never to a CPU re-implementation of ours.
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <pthread.h>
#include <stdlib.h>
#include <unistd.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <string.h>
#include <math.h>
#include <time.h>
#include "rfx_abi.h"
#include "rfx_hip.h"
#include "rfx_exec.h"
#include "rfx_ops.h"

typedef rfx_obj_p obj_p;

/* rfx_host.c */
obj_p rfx_host_null(void);
obj_p rfx_host_b8(int8_t v);
obj_p rfx_host_err(const char *msg);
obj_p rfx_host_eval(obj_p o);
void rfx_host_trim(void);

/* ------------------------------------------------------------------------------------------------ the verb table */
/* ONE row per built-in: V(id, the host's symbol, our entry point or NULL, the name the standalone host binds it to or NULL, the function object's type,
 * its attribute).  The F_* ids, the host's functions (H.f, bound by symbol), our entry points (fn_id recognises both inside parsed expressions) and
 * rfx_host_fn's lookup are all generated from it: a new verb is one new row and its implementation.  Row order is id order.
 * Three runs are addressed by range or by offset and must stay as they are (the _Static_asserts below):
 *   F_SUM .. F_FIRST  the aggregates rfx_select and rfx_update map: they test that id RANGE (rfx_select also takes, by name, F_LAST, F_MED and F_DEV);
 *   F_EQ .. F_GE      cmp_impl calls the host's H.f[F_EQ + op], op = RFX_EQ .. RFX_GE;
 *   F_ADD .. F_MOD    build_xnodes maps an operator to RFX_X_ADD + (f - F_ADD).
 * The ids after F_BINR lie outside the aggregates' range: window_agg (rfx_ops_window.c) recognises F_LAST and refuses F_DEV; F_DISTINCT .. F_UNION (and
 * F_IN as a verb of its own) are the set verbs of rfx_ops_set.c, which no reader of fn_id maps -- inside where: F_IN stays the comparison list of
 * rfx_ops_plan.c and nothing else.  `not` is recognised inside where: only; xbar inside `by:` is recognised by its function object and
 * bucketed by the planner, called as a verb it is rfx_xbar.  "div" is the reference's ray_fdiv (our rfx_div), "/" its ray_div (our rfx_floordiv).
 * rfx_select's take: stays the host's H.f[F_TAKE]. */
#define RFX_VERBS(V)                                                                                  \
    /* F_SUM .. F_FIRST: one run, addressed as a range */                                             \
    V(F_SUM, "ray_sum", rfx_sum, "sum", RFX_TYPE_UNARY, RFX_FN_AGGR)                                  \
    V(F_AVG, "ray_avg", rfx_avg, "avg", RFX_TYPE_UNARY, RFX_FN_AGGR)                                  \
    V(F_MIN, "ray_min", rfx_min, "min", RFX_TYPE_UNARY, RFX_FN_AGGR)                                  \
    V(F_MAX, "ray_max", rfx_max, "max", RFX_TYPE_UNARY, RFX_FN_AGGR)                                  \
    V(F_COUNT, "ray_count", rfx_count, "count", RFX_TYPE_UNARY, RFX_FN_AGGR)                          \
    V(F_FIRST, "ray_first", rfx_first, "first", RFX_TYPE_UNARY, RFX_FN_AGGR)                          \
    /* F_EQ .. F_GE: one run, addressed as F_EQ + RFX_EQ .. RFX_GE */                                 \
    V(F_EQ, "ray_eq", rfx_eq, "==", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                   \
    V(F_NE, "ray_ne", rfx_ne, "!=", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                   \
    V(F_LT, "ray_lt", rfx_lt, "<", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                    \
    V(F_GT, "ray_gt", rfx_gt, ">", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                    \
    V(F_LE, "ray_le", rfx_le, "<=", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                   \
    V(F_GE, "ray_ge", rfx_ge, ">=", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                   \
    V(F_AND, "ray_and", rfx_and, "and", RFX_TYPE_VARY, RFX_FN_SPECIAL_FORM)                           \
    V(F_OR, "ray_or", rfx_or, "or", RFX_TYPE_VARY, RFX_FN_SPECIAL_FORM)                               \
    V(F_SELECT, "ray_select", rfx_select, "select", RFX_TYPE_UNARY, RFX_FN_NONE)                      \
    /* F_ADD .. F_MOD: one run, addressed as RFX_X_ADD + (f - F_ADD) */                               \
    V(F_ADD, "ray_add", rfx_add, "+", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                 \
    V(F_SUB, "ray_sub", rfx_sub, "-", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                 \
    V(F_MUL, "ray_mul", rfx_mul, "*", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                 \
    V(F_FDIV, "ray_fdiv", rfx_div, "div", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                             \
    V(F_DIV, "ray_div", rfx_floordiv, "/", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                            \
    V(F_MOD, "ray_mod", rfx_mod, "%", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                                 \
    V(F_XBAR, "ray_xbar", rfx_xbar, "xbar", RFX_TYPE_BINARY, RFX_FN_ATOMIC)                           \
    V(F_LJ, "ray_left_join", rfx_left_join, NULL, RFX_TYPE_VARY, RFX_FN_NONE)                         \
    V(F_IJ, "ray_inner_join", rfx_inner_join, NULL, RFX_TYPE_VARY, RFX_FN_NONE)                       \
    V(F_UPDATE, "ray_update", rfx_update, "update", RFX_TYPE_UNARY, RFX_FN_NONE)                      \
    V(F_TAKE, "ray_take", rfx_take, "take", RFX_TYPE_BINARY, RFX_FN_NONE)                             \
    V(F_IN, "ray_in", rfx_in, "in", RFX_TYPE_BINARY, RFX_FN_NONE)                                     \
    V(F_WITHIN, "ray_within", rfx_within, NULL, RFX_TYPE_BINARY, RFX_FN_NONE)                         \
    V(F_NOT, "ray_not", NULL, NULL, RFX_TYPE_UNARY, RFX_FN_NONE)                                      \
    V(F_MED, "ray_med", rfx_med, "med", RFX_TYPE_UNARY, RFX_FN_AGGR)                                  \
    V(F_IASC, "ray_iasc", rfx_iasc, "iasc", RFX_TYPE_UNARY, RFX_FN_NONE)                              \
    V(F_IDESC, "ray_idesc", rfx_idesc, "idesc", RFX_TYPE_UNARY, RFX_FN_NONE)                          \
    V(F_ASC, "ray_asc", rfx_asc, "asc", RFX_TYPE_UNARY, RFX_FN_NONE)                                  \
    V(F_DESC, "ray_desc", rfx_desc, "desc", RFX_TYPE_UNARY, RFX_FN_NONE)                              \
    V(F_RANK, "ray_rank", rfx_rank, "rank", RFX_TYPE_UNARY, RFX_FN_NONE)                              \
    V(F_XASC, "ray_xasc", rfx_xasc, "xasc", RFX_TYPE_BINARY, RFX_FN_NONE)                             \
    V(F_XDESC, "ray_xdesc", rfx_xdesc, "xdesc", RFX_TYPE_BINARY, RFX_FN_NONE)                         \
    V(F_AJ, "ray_asof_join", rfx_asof_join, "asof-join", RFX_TYPE_VARY, RFX_FN_NONE)                  \
    V(F_BIN, "ray_bin", rfx_bin, "bin", RFX_TYPE_BINARY, RFX_FN_NONE)                                 \
    V(F_BINR, "ray_binr", rfx_binr, "binr", RFX_TYPE_BINARY, RFX_FN_NONE)                             \
    V(F_WJ, "ray_window_join", rfx_window_join, "window-join", RFX_TYPE_VARY, RFX_FN_NONE)            \
    V(F_WJ1, "ray_window_join1", rfx_window_join1, "window-join1", RFX_TYPE_VARY, RFX_FN_NONE)        \
    V(F_LAST, "ray_last", rfx_last, "last", RFX_TYPE_UNARY, RFX_FN_AGGR)                              \
    V(F_DISTINCT, "ray_distinct", rfx_distinct, "distinct", RFX_TYPE_UNARY, RFX_FN_NONE)              \
    V(F_FIND, "ray_find", rfx_find, "find", RFX_TYPE_BINARY, RFX_FN_NONE)                             \
    V(F_SECT, "ray_sect", rfx_sect, "sect", RFX_TYPE_BINARY, RFX_FN_NONE)                             \
    V(F_EXCEPT, "ray_except", rfx_except, "except", RFX_TYPE_BINARY, RFX_FN_NONE)                     \
    V(F_UNION, "ray_union", rfx_union, "union", RFX_TYPE_BINARY, RFX_FN_NONE)                         \
    V(F_DEV, "ray_dev", rfx_dev, "dev", RFX_TYPE_UNARY, RFX_FN_AGGR)                                  \
    V(F_XRANK, "ray_xrank", rfx_xrank, "xrank", RFX_TYPE_BINARY, RFX_FN_NONE)                         \
    V(F_FLOOR, "ray_floor", rfx_floor, "floor", RFX_TYPE_UNARY, RFX_FN_ATOMIC)                        \
    V(F_CEIL, "ray_ceil", rfx_ceil, "ceil", RFX_TYPE_UNARY, RFX_FN_ATOMIC)                            \
    V(F_ROUND, "ray_round", rfx_round, "round", RFX_TYPE_UNARY, RFX_FN_ATOMIC)                        \
    V(F_NEG, "ray_neg", rfx_neg, "neg", RFX_TYPE_UNARY, RFX_FN_ATOMIC)                                \
    V(F_FILTER, "ray_filter", rfx_filter, "filter", RFX_TYPE_BINARY, RFX_FN_NONE)                     \
    V(F_REVERSE, "ray_reverse", rfx_reverse, "reverse", RFX_TYPE_UNARY, RFX_FN_NONE)                  \
    V(F_AS, "ray_cast_obj", rfx_as, "as", RFX_TYPE_BINARY, RFX_FN_NONE)                               \
    V(F_CONCAT, "ray_concat", rfx_concat, "concat", RFX_TYPE_BINARY, RFX_FN_NONE)                     \
    V(F_RAZE, "ray_raze", rfx_raze, "raze", RFX_TYPE_UNARY, RFX_FN_NONE)                              \
    V(F_UPSERT, "ray_upsert", rfx_upsert, "upsert", RFX_TYPE_VARY, RFX_FN_NONE)                       \
    V(F_INSERT, "ray_insert", rfx_insert, "insert", RFX_TYPE_VARY, RFX_FN_NONE)                       \
    V(F_ROW, "ray_row", rfx_row, "row", RFX_TYPE_UNARY, RFX_FN_AGGR)
#define V(id, host, ours, name, type, attrs) id,
enum { RFX_VERBS(V) F_N };
#undef V
#define V(id, host, ours, name, type, attrs) [id] = {host, (void *)(ours), name, type, attrs},
static const struct { const char *host; void *ours; const char *name; int type, attrs; } VERB[F_N] = {RFX_VERBS(V)};
#undef V
_Static_assert(F_SUM == 0 && F_AVG == F_SUM + 1 && F_MIN == F_SUM + 2 && F_MAX == F_SUM + 3 && F_COUNT == F_SUM + 4 && F_FIRST == F_SUM + 5, "F_SUM .. F_FIRST: the aggregates' id range");
_Static_assert(F_NE == F_EQ + RFX_NE && F_LT == F_EQ + RFX_LT && F_GT == F_EQ + RFX_GT && F_LE == F_EQ + RFX_LE && F_GE == F_EQ + RFX_GE && RFX_EQ == 0, "F_EQ .. F_GE follow RFX_EQ .. RFX_GE");
_Static_assert(F_SUB - F_ADD == RFX_X_SUB - RFX_X_ADD && F_MUL - F_ADD == RFX_X_MUL - RFX_X_ADD && F_FDIV - F_ADD == RFX_X_FDIV - RFX_X_ADD && F_DIV - F_ADD == RFX_X_DIV - RFX_X_ADD && F_MOD - F_ADD == RFX_X_MOD - RFX_X_ADD, "F_ADD .. F_MOD follow RFX_X_ADD .. RFX_X_MOD");
/* ------------------------------------------------------------------------------------------------ host binding */
static struct {
    int bound; /* 0 = not yet, 1 = reference host, 2 = standalone */
    obj_p (*vector)(int8_t, int64_t);
    obj_p (*table)(obj_p, obj_p);
    obj_p (*i64)(int64_t);
    obj_p (*f64)(double);
    void (*drop)(obj_p);
    obj_p (*clone)(obj_p);
    obj_p (*eval)(obj_p);
    obj_p (*err)(const char *);
    int64_t (*intern)(const char *, int64_t);
    const char *(*symname)(int64_t);
    obj_p null_obj;
    /* the host's own built-ins by verb id (all NULL without a host), for recognising function objects inside parsed expressions and for delegation */
    void *f[F_N];
} H;
static void *g_host_where, *g_host_at, *g_host_group; /* the host's built-ins behind rfx_where / rfx_at / rfx_group (NULL without a host) */
static char g_err[640];
static int g_last_gpu = 0;

const char *rfx_ops_last_error(void) { return g_err; }
int rfx_last_select_on_gpu(void) { return g_last_gpu; }

int rfx_host_bind(void) {
    if (H.bound) return H.bound == 1;
    void *v = dlsym(RTLD_DEFAULT, "vector"), *t = dlsym(RTLD_DEFAULT, "table"), *e = dlsym(RTLD_DEFAULT, "eval");
    void *rs = dlsym(RTLD_DEFAULT, "ray_select"), *nu = dlsym(RTLD_DEFAULT, "__NULL_OBJ");
    if (v && t && e && rs && nu && !getenv("RFX_FORCE_STANDALONE")) {
        H.vector = (obj_p(*)(int8_t, int64_t))v;
        H.table = (obj_p(*)(obj_p, obj_p))t;
        H.eval = (obj_p(*)(obj_p))e;
        H.i64 = (obj_p(*)(int64_t))dlsym(RTLD_DEFAULT, "i64");
        H.f64 = (obj_p(*)(double))dlsym(RTLD_DEFAULT, "f64");
        H.drop = (void (*)(obj_p))dlsym(RTLD_DEFAULT, "drop_obj");
        H.clone = (obj_p(*)(obj_p))dlsym(RTLD_DEFAULT, "clone_obj");
        H.err = (obj_p(*)(const char *))dlsym(RTLD_DEFAULT, "ray_err");
        H.intern = (int64_t(*)(const char *, int64_t))dlsym(RTLD_DEFAULT, "symbols_intern");
        H.symname = (const char *(*)(int64_t))dlsym(RTLD_DEFAULT, "str_from_symbol");
        H.null_obj = (obj_p)nu;
        for (int i = 0; i < F_N; i++) H.f[i] = dlsym(RTLD_DEFAULT, VERB[i].host);
        g_host_where = dlsym(RTLD_DEFAULT, "ray_where"); /* (not in H.f: never recognised inside a query, only handed back to -- refused1x) */
        g_host_at = dlsym(RTLD_DEFAULT, "ray_at");
        g_host_group = dlsym(RTLD_DEFAULT, "ray_group");
        if (H.i64 && H.f64 && H.drop && H.clone && H.err && H.intern && H.symname) {
            H.bound = 1;
            return 1;
        }
    }
    H.vector = rfx_host_vector;
    H.table = rfx_host_table;
    H.i64 = rfx_host_i64;
    H.f64 = rfx_host_f64;
    H.drop = rfx_host_drop;
    H.clone = rfx_host_clone;
    H.eval = rfx_host_eval;
    H.err = rfx_host_err;
    H.intern = rfx_host_intern;
    H.symname = rfx_host_symbol_name;
    H.null_obj = rfx_host_null();
    memset(H.f, 0, sizeof(H.f));
    H.bound = 2;
    return 0;
}

obj_p rfx_host_fn(const char *name) {
    rfx_host_bind();
    for (int f = 0; f < F_N; f++)
        if (VERB[f].name && strcmp(VERB[f].name, name) == 0) {
            obj_p o = rfx_host_i64((int64_t)(intptr_t)VERB[f].ours);
            o->type = (int8_t)VERB[f].type; /* function objects carry the POSITIVE type code (core/env.c:66-74) */
            o->attrs = (uint8_t)VERB[f].attrs;
            return o;
        }
    return NULL;
}

static obj_p fail(const char *msg) {
    rfx_host_bind();
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return H.err(msg);
}
static obj_p fail_hip(const char *what) {
    char b[600];
    snprintf(b, sizeof(b), "%s: %s", what, rfx_hip_last_error());
    return fail(b);
}
static int g_refused_sharded;
static obj_p fail_ctx(void) {
    if (g_refused_sharded) return fail("this operator (or this shape of its arguments) needs its columns whole on one device: with RFX_SHARDS / RFX_DEVICES it is the host's own built-in -- joins, update, at over unordered ids, group over sparse keys, filtered MAPGROUP pairs");
    return fail_hip("no usable MI355X");
}
/* ... unless there is a host beside us: then the operator is simply the host's own again (the shards hold row ranges; RFX_SHARDS /
 * RFX_DEVICES is about rfx_select).  Defined below, once HOST_CALL is. */
static obj_p refused1(int f, obj_p x);
__attribute__((unused)) static obj_p refused2(int f, obj_p x, obj_p y);
static obj_p refusedn(int f, obj_p *x, int64_t n);

/* which built-in does this function object denote? -1 if none */
static int fn_id(obj_p o) {
    if (!o || (o->type != RFX_TYPE_UNARY && o->type != RFX_TYPE_BINARY && o->type != RFX_TYPE_VARY)) return -1;
    void *p = (void *)(intptr_t)o->i64;
    for (int i = 0; i < F_N; i++)
        if ((VERB[i].ours && p == VERB[i].ours) || (H.f[i] && p == H.f[i])) return i;
    return -1;
}

/* The operator layer by concern (round 5: one 3 100-line file before).  ONE translation unit -- the pieces share the lock, the residency cache and the
 * per-call scratch lists as file statics -- read in this order: */
#include "rfx_ops_residency.c"
#include "rfx_ops_repro.c"
#include "rfx_ops_plan.c"
#include "rfx_ops_select.c"
#include "rfx_ops_update.c"
#include "rfx_ops_operators.c"
#include "rfx_ops_cols.c"
#include "rfx_ops_join.c"
#include "rfx_ops_folds.c"
#include "rfx_ops_verbs.c"
#include "rfx_ops_sort.c"
#include "rfx_ops_asof.c"
#include "rfx_ops_window.c"
#include "rfx_ops_set.c"
#include "rfx_ops_bucket.c"
#include "rfx_ops_rows.c"
#include "rfx_ops_cast.c"
#include "rfx_ops_concat.c"
#include "rfx_ops_upsert.c"
#include "rfx_ops_collect.c"
