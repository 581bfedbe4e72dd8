/* rfx_exec_set.c -- part of the planner's ONE translation unit (rfx_exec.c #includes it -- the Makefile does not compile it on its own).
 * The set verbs over 8-byte keys: distinct / union (index_distinct_i64, core/index.c:551-607), in (index_in_i64_i64, :1291-1361), find
 * (index_find_i64, :1507-1574), sect / except (core/items.c:898-948).  The ROUTE of every call is the reference's, decided from the key scopes
 * exactly as it decides; the kernels are rfx_set.hip's.  Where the reference's own indexing would leave its tables -- ht_oa_tab_next / _get start at
 * (i64)key % size, negative for a negative key; a range that does not fit 64 bits -- there is no answer to reproduce: the call is declined with
 * *route = RFX_SET_ROUTE_UNDEFINED, RFX_ESTATE and the reason in rfx_exec_last_error(), and the operator layer hands it to the host.  One shard. */
#define SET_MAX_RANGE ((int64_t)1 << 20) /* MAX_RANGE, core/index.c:36 */
typedef __int128 set_i128;

static int set_one_shard(rfx_exec_t *x, const char *what) {
    if (x->nshards > 1 || x->has_tr) {
        snprintf(x->err, sizeof(x->err), "rfx_exec: %s over a sharded column", what);
        return RFX_ELIMIT;
    }
    return RFX_OK;
}
static int set_undefined(rfx_exec_t *x, const char *what, const char *why, int *route) {
    if (route) *route = RFX_SET_ROUTE_UNDEFINED;
    snprintf(x->err, sizeof(x->err), "rfx_exec: %s: undefined in the reference (%s)", what, why);
    return RFX_ESTATE;
}
/* ops_is_prime / ops_next_prime (core/ops.c:66-88) and optimal_hash_table_size (core/hash.c:35-38): P = the first prime >= ceil(len / 0.75) */
static int set_is_prime(int64_t v) {
    if (v <= 1) return 0;
    if (v <= 3) return 1;
    if (v % 2 == 0 || v % 3 == 0) return 0;
    for (int64_t i = 5; i * i <= v; i += 6)
        if (v % i == 0 || v % (i + 2) == 0) return 0;
    return 1;
}
int64_t rfx_set_table_cells(int64_t len) {
    const double want = (double)len / 0.75;
    int64_t p = (int64_t)want;
    if ((double)p < want) p++;
    while (!set_is_prime(p)) p++;
    return p;
}
static int64_t set_capacity(int64_t cells) { /* this library's own table: a power of two, at most half full */
    int64_t cap = 64;
    while (cap < 2 * cells) cap <<= 1;
    return cap;
}
/* scratch of one call */
typedef struct set_tmp {
    rfx_ctx_t *c;
    void *p[8];
    int n;
} set_tmp_t;
static int set_alloc(set_tmp_t *t, void **out, size_t bytes) {
    *out = NULL;
    if (t->n >= 8) return RFX_ELIMIT;
    int rc = rfx_hip_malloc(t->c, out, bytes ? bytes : 8);
    if (rc == RFX_OK) t->p[t->n++] = *out;
    return rc;
}
static void set_release(set_tmp_t *t) {
    rfx_hip_ctx_sync(t->c); /* (whatever was launched has read its scratch before it is freed) */
    for (int i = 0; i < t->n; i++) rfx_hip_free(t->c, t->p[i]);
    t->n = 0;
}
static int set_fail(rfx_exec_t *x, const char *what, int rc) {
    snprintf(x->err, sizeof(x->err), "rfx_exec: %s: %.400s", what, rfx_hip_last_error());
    return rc;
}

int rfx_exec_distinct(rfx_exec_t *x, const int64_t *d_a, int64_t na, const int64_t *d_b, int64_t nb, int64_t *d_out, int64_t *nout, int *route) {
    if (route) *route = RFX_SET_ROUTE_NONE;
    if (nout) *nout = 0;
    if (!x || !nout || na < 0 || nb < 0 || (na > 0 && !d_a) || (nb > 0 && !d_b) || (na + nb > 0 && !d_out)) return RFX_EINVAL;
    x->err[0] = 0;
    const char *what = nb > 0 ? "union" : "distinct";
    int rc = set_one_shard(x, what);
    if (rc != RFX_OK) return rc;
    const int64_t len = na + nb;
    if (len == 0) return RFX_OK; /* (range 0 <= len 0: the dense route over no cell, no launch) */
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    int64_t t0 = now_ns();
    int64_t sc[4];
    if ((rc = rfx_hip_set_scope(c, d_a, na, d_b, nb, sc)) != RFX_OK) return set_fail(x, what, rc);
    const set_i128 range = (set_i128)sc[1] - (set_i128)sc[0] + 1;
    if (range > (set_i128)INF_I64) return set_undefined(x, what, "max - min + 1 does not fit 64 bits", route);
    set_tmp_t t = {c, {0}, 0};
    void *bits = NULL, *scan = NULL;
    int r = RFX_SET_ROUTE_NONE;
    if (range <= (set_i128)len || range <= (set_i128)SET_MAX_RANGE) {
        /* DENSE: mark [min, max], the marked values ascending */
        r = RFX_SET_ROUTE_DENSE;
        const int64_t rg = (int64_t)range, words = (rg + 63) / 64;
        if ((rc = set_alloc(&t, &bits, (size_t)words * 8)) != RFX_OK || (rc = set_alloc(&t, &scan, (size_t)(rg / 16384 + 2) * 8)) != RFX_OK ||
            (rc = rfx_hip_memset(c, bits, 0, (size_t)words * 8)) != RFX_OK || (rc = rfx_hip_set_mark(c, d_a, na, d_b, nb, sc[0], rg, (uint64_t *)bits)) != RFX_OK)
            goto out;
        rfx_hip_ctx_sync(c); /* (the build half ends with the stream idle: the two counters add up to the call) */
        x->stat[RFX_XSTAT_NS_SET_BUILD] += now_ns() - t0;
        t0 = now_ns();
        rc = rfx_hip_set_compact(c, (const uint64_t *)bits, rg, RFX_SET_EMIT_OFFSET, sc[0], NULL, NULL, 0, NULL, (int64_t *)scan, len, d_out, nout);
        if (rc == RFX_OK) rc = rfx_hip_ctx_sync(c); /* (the emit kernel is launched behind the count: the probe half ends with the stream idle too) */
        x->stat[RFX_XSTAT_NS_SET_PROBE] += now_ns() - t0;
    } else {
        /* HASH: the reference's linear-probing table of P cells, the keys in slot order */
        if (sc[2] < 0) return set_undefined(x, what, "hash route over a negative key: (i64)key % size indexes before the table", route);
        r = RFX_SET_ROUTE_HASH;
        const int64_t P = rfx_set_table_cells(len), cap = set_capacity(len), words = (P + 63) / 64;
        void *keys, *first, *cells;
        if ((rc = set_alloc(&t, &keys, (size_t)cap * 8)) != RFX_OK || (rc = set_alloc(&t, &first, (size_t)cap * 8)) != RFX_OK ||
            (rc = set_alloc(&t, &cells, (size_t)P * 8)) != RFX_OK || (rc = set_alloc(&t, &bits, (size_t)words * 8)) != RFX_OK ||
            (rc = set_alloc(&t, &scan, (size_t)(P / 16384 + 2) * 8)) != RFX_OK)
            goto out;
        if ((rc = rfx_hip_fill_i64(c, (int64_t *)keys, cap, NULL_I64)) != RFX_OK || (rc = rfx_hip_fill_i64(c, (int64_t *)first, cap, INF_I64)) != RFX_OK ||
            (rc = rfx_hip_fill_i64(c, (int64_t *)cells, P, INF_I64)) != RFX_OK ||
            (rc = rfx_hip_set_hash_build(c, d_a, na, d_b, nb, (int64_t *)keys, (int64_t *)first, cap)) != RFX_OK ||
            (rc = rfx_hip_set_priority_insert(c, (const int64_t *)keys, (const int64_t *)first, cap, P, (int64_t *)cells)) != RFX_OK)
            goto out;
        rfx_hip_ctx_sync(c); /* (the build half ends with the stream idle: the two counters add up to the call) */
        x->stat[RFX_XSTAT_NS_SET_BUILD] += now_ns() - t0;
        t0 = now_ns();
        if ((rc = rfx_hip_set_cells_flags(c, (const int64_t *)cells, P, (uint64_t *)bits)) != RFX_OK) goto out;
        rc = rfx_hip_set_compact(c, (const uint64_t *)bits, P, RFX_SET_EMIT_ROWKEY, 0, (const int64_t *)cells, d_a, na, d_b, (int64_t *)scan, len, d_out, nout);
        if (rc == RFX_OK) rc = rfx_hip_ctx_sync(c);
        x->stat[RFX_XSTAT_NS_SET_PROBE] += now_ns() - t0;
    }
out:
    if (rc != RFX_OK) set_fail(x, what, rc);
    else {
        x->stat[RFX_XSTAT_SET_DISTINCTS]++;
        if (route) *route = r;
    }
    set_release(&t);
    return rc;
}

/* The lookup structure of in / find / sect / except: `set` (ns cells) is what is looked INTO, `q` (nq > 0 cells) what is looked up. */
static int set_lookup_build(rfx_exec_t *x, rfx_ctx_t *c, set_tmp_t *t, const char *what, const int64_t *d_set, int64_t ns, const int64_t *d_q, int64_t nq, int want_first,
                            rfx_set_lookup_t *L, int *route) {
    int rc;
    memset(L, 0, sizeof(*L));
    L->kind = want_first ? RFX_SET_DENSE_FIRST : RFX_SET_BITS; /* range 0: nobody is found */
    *route = RFX_SET_ROUTE_DISJOINT;
    if (ns == 0) return RFX_OK; /* (an empty scope is {null, null}: the intersection is empty or the one null cell, the set holds nothing either way) */
    int64_t ss[4], sq[4];
    if ((rc = rfx_hip_set_scope(c, d_set, ns, NULL, 0, ss)) != RFX_OK || (rc = rfx_hip_set_scope(c, d_q, nq, NULL, 0, sq)) != RFX_OK) return set_fail(x, what, rc);
    const int64_t mn = ss[0] > sq[0] ? ss[0] : sq[0], mx = ss[1] < sq[1] ? ss[1] : sq[1];
    if (mn > mx) return RFX_OK;
    const set_i128 range = (set_i128)mx - (set_i128)mn + 1;
    if (want_first && range > (set_i128)INF_I64) return set_undefined(x, what, "max - min + 1 does not fit 64 bits", route);
    if (range <= (set_i128)SET_MAX_RANGE) {
        const int64_t rg = (int64_t)range;
        void *tab;
        *route = RFX_SET_ROUTE_DENSE;
        L->kmin = mn;
        L->range = rg;
        if (want_first) {
            if ((rc = set_alloc(t, &tab, (size_t)rg * 8)) != RFX_OK || (rc = rfx_hip_fill_i64(c, (int64_t *)tab, rg, INF_I64)) != RFX_OK ||
                (rc = rfx_hip_set_first_dense(c, d_set, ns, mn, rg, (int64_t *)tab)) != RFX_OK)
                return set_fail(x, what, rc);
            L->d_first = (const int64_t *)tab;
        } else {
            const size_t bytes = (size_t)((rg + 63) / 64) * 8;
            if ((rc = set_alloc(t, &tab, bytes)) != RFX_OK || (rc = rfx_hip_memset(c, tab, 0, bytes)) != RFX_OK ||
                (rc = rfx_hip_set_mark(c, d_set, ns, NULL, 0, mn, rg, (uint64_t *)tab)) != RFX_OK)
                return set_fail(x, what, rc);
            L->d_bits = (const uint64_t *)tab;
        }
        return RFX_OK;
    }
    /* HASH.  `in` steps over nulls on both sides (a null is a member when the set holds one); `find` inserts and looks up every cell, nulls too */
    if (ss[2] < 0 || sq[2] < 0) return set_undefined(x, what, "hash route over a negative key: (i64)key % size indexes before the table", route);
    if (want_first && (ss[3] > 0 || sq[3] > 0)) return set_undefined(x, what, "hash route over a null: INT64_MIN % size indexes before the table", route);
    *route = RFX_SET_ROUTE_HASH;
    const int64_t cap = set_capacity(ns);
    void *keys, *first = NULL;
    if ((rc = set_alloc(t, &keys, (size_t)cap * 8)) != RFX_OK || (rc = rfx_hip_fill_i64(c, (int64_t *)keys, cap, NULL_I64)) != RFX_OK) return set_fail(x, what, rc);
    if (want_first && ((rc = set_alloc(t, &first, (size_t)cap * 8)) != RFX_OK || (rc = rfx_hip_fill_i64(c, (int64_t *)first, cap, INF_I64)) != RFX_OK))
        return set_fail(x, what, rc);
    if ((rc = rfx_hip_set_hash_build(c, d_set, ns, NULL, 0, (int64_t *)keys, (int64_t *)first, cap)) != RFX_OK) return set_fail(x, what, rc);
    L->kind = RFX_SET_HASH;
    L->null_hit = ss[3] > 0;
    L->d_keys = (const int64_t *)keys;
    L->d_first = (const int64_t *)first;
    L->capacity = cap;
    return RFX_OK;
}

int rfx_exec_member(rfx_exec_t *x, const int64_t *d_x, int64_t nx, const int64_t *d_y, int64_t ny, int want_first, void *d_out, int *route) {
    if (route) *route = RFX_SET_ROUTE_NONE;
    if (!x || nx < 0 || ny < 0 || (nx > 0 && !d_x) || (ny > 0 && !d_y)) return RFX_EINVAL;
    x->err[0] = 0;
    const char *what = want_first ? "find" : "in";
    int rc = set_one_shard(x, what);
    if (rc != RFX_OK) return rc;
    /* in x y: every cell of x is looked up in y; find x y: every cell of y is looked up in x */
    const int64_t *d_set = want_first ? d_x : d_y, *d_q = want_first ? d_y : d_x;
    const int64_t ns = want_first ? nx : ny, nq = want_first ? ny : nx;
    if (nq == 0 || (want_first && nx == 0)) return RFX_OK; /* (nothing to write; find over an empty x answers I64(0) whatever y holds, core/index.c:1512) */
    if (!d_out) return RFX_EINVAL;
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    set_tmp_t t = {c, {0}, 0};
    rfx_set_lookup_t L;
    int r = RFX_SET_ROUTE_NONE;
    int64_t t0 = now_ns();
    if ((rc = set_lookup_build(x, c, &t, what, d_set, ns, d_q, nq, want_first, &L, &r)) == RFX_OK) {
        rfx_hip_ctx_sync(c); /* (the build half ends with the stream idle: the two counters add up to the call) */
        x->stat[RFX_XSTAT_NS_SET_BUILD] += now_ns() - t0;
        t0 = now_ns();
        if ((rc = rfx_hip_set_probe(c, &L, d_q, nq, want_first ? RFX_SET_OUT_FIRST : RFX_SET_OUT_B8, d_out)) != RFX_OK || (rc = rfx_hip_ctx_sync(c)) != RFX_OK)
            set_fail(x, what, rc);
        x->stat[RFX_XSTAT_NS_SET_PROBE] += now_ns() - t0;
    }
    if (rc == RFX_OK) x->stat[RFX_XSTAT_SET_MEMBERS]++;
    if (route && (rc == RFX_OK || r == RFX_SET_ROUTE_UNDEFINED)) *route = r;
    set_release(&t);
    return rc;
}

int rfx_exec_set_filter(rfx_exec_t *x, const int64_t *d_x, int64_t nx, const int64_t *d_y, int64_t ny, int y_is_atom, int64_t atom, int keep_members, int64_t *d_out,
                        int64_t *nout, int *route) {
    if (route) *route = RFX_SET_ROUTE_NONE;
    if (nout) *nout = 0;
    if (!x || !nout || nx < 0 || ny < 0 || (nx > 0 && (!d_x || !d_out)) || (!y_is_atom && ny > 0 && !d_y)) return RFX_EINVAL;
    x->err[0] = 0;
    const char *what = keep_members ? "sect" : "except";
    int rc = set_one_shard(x, what);
    if (rc != RFX_OK) return rc;
    if (nx == 0) return RFX_OK;
    rfx_ctx_t *c = x->ctx[0];
    rfx_hip_ctx_bind_thread(c);
    set_tmp_t t = {c, {0}, 0};
    rfx_set_lookup_t L;
    int r = RFX_SET_ROUTE_ATOM;
    void *flags, *scan;
    int64_t t0 = now_ns();
    if (y_is_atom) {
        memset(&L, 0, sizeof(L));
        L.kind = RFX_SET_ATOM;
        L.atom = atom;
    } else if ((rc = set_lookup_build(x, c, &t, what, d_y, ny, d_x, nx, 0, &L, &r)) != RFX_OK)
        goto out;
    rfx_hip_ctx_sync(c); /* (the build half ends with the stream idle: the two counters add up to the call) */
    x->stat[RFX_XSTAT_NS_SET_BUILD] += now_ns() - t0;
    t0 = now_ns();
    /* probe + ordered compaction of the VALUES: one bit per cell of x, then x's own cells at the set bits -- no B8 vector, no id vector, no gather */
    if ((rc = set_alloc(&t, &flags, (size_t)((nx + 63) / 64) * 8)) != RFX_OK || (rc = set_alloc(&t, &scan, (size_t)(nx / 16384 + 2) * 8)) != RFX_OK ||
        (rc = rfx_hip_set_probe(c, &L, d_x, nx, keep_members ? RFX_SET_OUT_FLAGS : RFX_SET_OUT_NOT_FLAGS, flags)) != RFX_OK ||
        (rc = rfx_hip_set_compact(c, (const uint64_t *)flags, nx, RFX_SET_EMIT_SRC, 0, d_x, NULL, 0, NULL, (int64_t *)scan, nx, d_out, nout)) != RFX_OK ||
        (rc = rfx_hip_ctx_sync(c)) != RFX_OK)
        set_fail(x, what, rc);
    x->stat[RFX_XSTAT_NS_SET_PROBE] += now_ns() - t0;
out:
    if (rc == RFX_OK) x->stat[RFX_XSTAT_SET_FILTERS]++;
    if (route && (rc == RFX_OK || r == RFX_SET_ROUTE_UNDEFINED)) *route = r;
    set_release(&t);
    return rc;
}
