// rfx_bucket.hip -- the bucket verbs as columns of their own: xrank (ray_xrank, core/order.c:598-649), xbar (ray_xbar_partial, core/math.c:1635-1782),
// floor / ceil / round (core/math.c:2047-2117), neg (ray_neg, core/order.c:445-497), within (ray_within, core/items.c:848-872).
// Streaming and scatter kernels: a lane owns four consecutive cells per step (16-byte loads and stores at either element width), no LDS.
// The cell rules live in rfx_common.hpp (rfx_xbar_*, rfx_floor_f64_bits ...): the by: path buckets its keys with the same functions.
#include "rfx_cells.hpp"

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// four consecutive cells from row r (a multiple of 4) as raw bits; 4-byte cells sign-extended
__device__ __forceinline__ void bk_ld4(const void *p, bool wide, i64 r, u64 v[4]) {
    if (wide) {
        const rfx_v2q a = __builtin_nontemporal_load((const rfx_v2q *)((const u64 *)p + r)), b = __builtin_nontemporal_load((const rfx_v2q *)((const u64 *)p + r + 2));
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
        const v4u a = __builtin_nontemporal_load((const v4u *)((const unsigned *)p + r));
        v[0] = (u64)(i64)(int)a.x; v[1] = (u64)(i64)(int)a.y; v[2] = (u64)(i64)(int)a.z; v[3] = (u64)(i64)(int)a.w;
    }
}
__device__ __forceinline__ u64 bk_ld1(const void *p, bool wide, i64 r) { return wide ? ((const u64 *)p)[r] : (u64)(i64)((const int *)p)[r]; }
__device__ __forceinline__ void bk_st4(void *p, bool wide, i64 r, const u64 v[4]) {
    if (wide) {
        rfx_v2q a, b;
        a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
        __builtin_nontemporal_store(a, (rfx_v2q *)((u64 *)p + r));
        __builtin_nontemporal_store(b, (rfx_v2q *)((u64 *)p + r + 2));
    } else {
        v4u a;
        a.x = (unsigned)v[0]; a.y = (unsigned)v[1]; a.z = (unsigned)v[2]; a.w = (unsigned)v[3];
        __builtin_nontemporal_store(a, (v4u *)((unsigned *)p + r));
    }
}
__device__ __forceinline__ void bk_st1(void *p, bool wide, i64 r, u64 v) {
    if (wide) ((u64 *)p)[r] = v;
    else ((unsigned *)p)[r] = (unsigned)v;
}

// every map below: quads of four cells grid-strided, then the 0..3 cells left over
template <class Op>
__global__ __launch_bounds__(RFX_BLOCK) void k_bucket_map(const Op op, i64 n) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK, n4 = n / 4;
    for (i64 g = tid; g < n4; g += nt) {
        u64 o[4];
        op.quad(g * 4, o);
        bk_st4(op.out, op.out_wide, g * 4, o);
    }
    for (i64 r = n4 * 4 + tid; r < n; r += nt) bk_st1(op.out, op.out_wide, r, op.cell(r));
}
template <class Op>
static int bucket_launch(rfx_ctx *c, const Op &op, i64 n) {
    i64 blocks = (n / 4 + RFX_BLOCK - 1) / RFX_BLOCK;
    int grid = rfx_grid(c);
    if (blocks < 1) blocks = 1;
    if (blocks < grid) grid = (int)blocks;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL((k_bucket_map<Op>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, op, n);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
static inline bool bk_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

// a 4-byte cell read from its widened 8-byte image (rfx_hip_widen_i32): the null's promotion undone, every other cell is its sign extension already
__device__ __forceinline__ u64 unwiden(u64 v, bool fix) { return fix && (i64)v == RFX_NULL_I64_D ? (u64)(i64)RFX_NULL_I32_D : v; }

// ---- xbar ----
struct XbarOp {
    const void *x, *y; // NULL: the atom, already promoted to `mid` (xm / ym)
    void *out;
    u64 xm, ym, yr; // yr: 1 / ym of an f64-middle atom y, flushed
    int x_type, y_type, mid, y_time;
    bool out_wide, xw, yw, xfix, yfix; // xw / yw: 8-byte cells; xfix / yfix: a 4-byte operand widened (its null is NULL_I64 there)
    // an operand's cell in the middle type: i32_to_i64 / i32_to_f64 / i64_to_f64 (null -> null), time_to_timestamp (null -> null, else x 10^6)
    __device__ __forceinline__ u64 to_mid(u64 v, int type, int time) const {
        if (mid == RFX_F64) {
            if (type == RFX_F64) return v;
            if (type == RFX_I32) return (int)v == RFX_NULL_I32_D ? RFX_NAN_BITS : rfx_as_u64((double)(int)v);
            return rfx_i64_to_f64_bits(v);
        }
        if (mid == RFX_I64 && type == RFX_I32) return (int)v == RFX_NULL_I32_D ? (u64)RFX_NULL_I64_D : (time ? (u64)((i64)(int)v * 1000000) : v);
        return v;
    }
    __device__ __forceinline__ u64 apply(u64 a, u64 b) const {
        if (mid == RFX_F64) return rfx_xbar_f64_bits(a, b, yr, y == nullptr);
        if (mid == RFX_I32) return (u64)(i64)rfx_xbar_i32((int)a, (int)b);
        const i64 r = rfx_xbar_i64((i64)a, (i64)b);
        if (out_wide) return (u64)r;
        return r == RFX_NULL_I64_D ? (u64)(i64)RFX_NULL_I32_D : (u64)r; // i64_to_date / i64_to_time: the store truncates
    }
    __device__ __forceinline__ u64 cell(i64 r) const {
        const u64 a = x ? to_mid(unwiden(bk_ld1(x, xw, r), xfix), x_type, 0) : xm;
        const u64 b = y ? to_mid(unwiden(bk_ld1(y, yw, r), yfix), y_type, y_time) : ym;
        return apply(a, b);
    }
    __device__ __forceinline__ void quad(i64 r, u64 o[4]) const {
        u64 a[4] = {xm, xm, xm, xm}, b[4] = {ym, ym, ym, ym};
        if (x) bk_ld4(x, xw, r, a);
        if (y) bk_ld4(y, yw, r, b);
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = apply(x ? to_mid(unwiden(a[j], xfix), x_type, 0) : a[j], y ? to_mid(unwiden(b[j], yfix), y_type, y_time) : b[j]);
    }
};
static bool bk_type_ok(int t) { return t == RFX_I32 || t == RFX_I64 || t == RFX_F64; }
static u64 bk_host_mid(u64 v, int type, int mid, int time) { // XbarOp::to_mid for an atom, once
    if (mid == RFX_F64) {
        double d;
        if (type == RFX_F64) return v;
        if (type == RFX_I32) { if ((int32_t)v == INT32_MIN) return RFX_NAN_BITS; d = (double)(int32_t)v; }
        else { if ((i64)v == RFX_NULL_I64_D) return RFX_NAN_BITS; d = (double)(i64)v; }
        u64 b;
        memcpy(&b, &d, 8);
        return b;
    }
    if (type == RFX_I32) {
        if (mid == RFX_I64) return (int32_t)v == INT32_MIN ? (u64)RFX_NULL_I64_D : (u64)((i64)(int32_t)v * (time ? 1000000 : 1));
        return (u64)(i64)(int32_t)v;
    }
    return v;
}
extern "C" int rfx_hip_xbar(rfx_ctx_t *ctx, const rfx_xbar_desc_t *d, int64_t n, void *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && d && n >= 0, RFX_EINVAL, "bad argument");
    RFX_REQUIRE(bk_type_ok(d->x_type) && bk_type_ok(d->y_type) && bk_type_ok(d->mid) && (d->out_bytes == 4 || d->out_bytes == 8), RFX_EINVAL, "bad descriptor");
    // the middle type holds both operands (a narrower middle than an operand is no arm of the reference); f64 and i32 results keep their width
    RFX_REQUIRE(d->mid == RFX_F64 || (d->x_type != RFX_F64 && d->y_type != RFX_F64), RFX_EINVAL, "an f64 operand needs the f64 middle type");
    RFX_REQUIRE(d->mid != RFX_I32 || (d->x_type == RFX_I32 && d->y_type == RFX_I32), RFX_EINVAL, "the i32 middle type takes 4-byte operands");
    RFX_REQUIRE((d->mid == RFX_I32) == (d->out_bytes == 4) || (d->mid == RFX_I64 && d->out_bytes == 4), RFX_EINVAL, "output width does not fit the middle type");
    RFX_REQUIRE(!d->y_time || (d->mid == RFX_I64 && d->y_type == RFX_I32), RFX_EINVAL, "y_time is a 4-byte y under the i64 middle type");
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d->d_x || d->d_y, RFX_EINVAL, "at least one operand is a column");
    RFX_REQUIRE(d_out && bk_aligned(d_out) && bk_aligned(d->d_x) && bk_aligned(d->d_y), RFX_EINVAL, "16-byte aligned device buffers expected");
    XbarOp op;
    op.x = d->d_x;
    op.y = d->d_y;
    op.out = d_out;
    op.x_type = d->x_type;
    op.y_type = d->y_type;
    op.mid = d->mid;
    op.y_time = d->y_time;
    op.out_wide = d->out_bytes == 8;
    op.xfix = d->x_type == RFX_I32 && (d->widened & 1);
    op.yfix = d->y_type == RFX_I32 && (d->widened & 2);
    op.xw = d->x_type != RFX_I32 || op.xfix;
    op.yw = d->y_type != RFX_I32 || op.yfix;
    op.xm = bk_host_mid(d->x_atom, d->x_type, d->mid, 0); // an atom is promoted once, here
    op.ym = bk_host_mid(d->y_atom, d->y_type, d->mid, d->y_time);
    op.yr = 0;
    if (d->mid == RFX_F64 && !d->d_y) { // the atom divisor's reciprocal, hoisted: what the reference's build multiplies by
        const u64 yb = rfx_ftz_bits(op.ym);
        double y, r;
        memcpy(&y, &yb, 8);
        r = 1.0 / y;
        memcpy(&op.yr, &r, 8);
        op.yr = rfx_ftz_bits(op.yr);
    }
    return bucket_launch(c, op, (i64)n);
}

// ---- floor / ceil / round ----
struct RoundOp {
    const void *in;
    void *out;
    int op;
    bool out_wide;
    __device__ __forceinline__ u64 one(u64 b) const { return op == RFX_ROUND_FLOOR ? rfx_floor_f64_bits(b) : (op == RFX_ROUND_CEIL ? rfx_ceil_f64_bits(b) : rfx_round_f64_bits(b)); }
    __device__ __forceinline__ u64 cell(i64 r) const { return one(bk_ld1(in, true, r)); }
    __device__ __forceinline__ void quad(i64 r, u64 o[4]) const {
        u64 a[4];
        bk_ld4(in, true, r, a);
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = one(a[j]);
    }
};
extern "C" int rfx_hip_round_f64(rfx_ctx_t *ctx, int op, const double *d_in, int64_t n, double *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && n >= 0 && op >= RFX_ROUND_FLOOR && op <= RFX_ROUND_ROUND, RFX_EINVAL, "bad argument");
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_in && d_out && bk_aligned(d_in) && bk_aligned(d_out), RFX_EINVAL, "16-byte aligned device buffers expected");
    RoundOp o;
    o.in = d_in;
    o.out = d_out;
    o.op = op;
    o.out_wide = true;
    return bucket_launch(c, o, (i64)n);
}

// ---- neg ----
struct NegOp {
    const void *in;
    void *out;
    int type;
    bool out_wide, in_wide, fix; // in_wide: 8-byte cells; fix: 4-byte cells widened (RFX_I32_WIDE)
    __device__ __forceinline__ u64 one(u64 b) const { return type == RFX_F64 ? b ^ 0x8000000000000000ULL : 0 - unwiden(b, fix); } // (a 4-byte cell arrives sign-extended)
    __device__ __forceinline__ u64 cell(i64 r) const { return one(bk_ld1(in, in_wide, r)); }
    __device__ __forceinline__ void quad(i64 r, u64 o[4]) const {
        u64 a[4];
        bk_ld4(in, in_wide, r, a);
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = one(a[j]);
    }
};
extern "C" int rfx_hip_neg(rfx_ctx_t *ctx, int32_t type, const void *d_in, int64_t n, void *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && n >= 0 && (bk_type_ok(type) || type == RFX_I32_WIDE), RFX_EINVAL, "bad argument");
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_in && d_out && bk_aligned(d_in) && bk_aligned(d_out), RFX_EINVAL, "16-byte aligned device buffers expected");
    RFX_REQUIRE(type != RFX_I32 || d_in != d_out, RFX_EINVAL, "a 4-byte input widens: not in place");
    NegOp o;
    o.in = d_in;
    o.out = d_out;
    o.fix = type == RFX_I32_WIDE;
    o.type = o.fix ? RFX_I32 : type;
    o.in_wide = type != RFX_I32;
    o.out_wide = true;
    return bucket_launch(c, o, (i64)n);
}

// ---- xrank ----
// (r * nb) / n for consecutive r without a division per cell: the quotient and remainder of one r, then +1 in r is + nb / n, + nb % n with a carry.
struct QR { u64 q, rem; };
__device__ __forceinline__ QR qr_at(u64 r, u64 nb, u64 n) { const u64 p = r * nb; QR t; t.q = p / n; t.rem = p - t.q * n; return t; }
__device__ __forceinline__ void qr_up(QR &t, u64 dq, u64 dr, u64 n) { t.q += dq; t.rem += dr; if (t.rem >= n) { t.rem -= n; t.q += 1; } }
__device__ __forceinline__ void qr_down(QR &t, u64 dq, u64 dr, u64 n) { t.q -= dq; if (t.rem < dr) { t.rem += n; t.q -= 1; } t.rem -= dr; }

// d_out[perm[r]] = (r * nb) / n: a lane takes eight consecutive ranks per step (four 16-byte loads in flight, one division), scattered 8-byte stores
#define XR_CELLS 8
__global__ __launch_bounds__(RFX_BLOCK) void k_xrank(const u64 *__restrict__ perm, i64 n, u64 nb, u64 dq, u64 dr, u64 *__restrict__ out) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK, ng = n / XR_CELLS;
    for (i64 g = tid; g < ng; g += nt) {
        const i64 r0 = g * XR_CELLS;
        u64 p[XR_CELLS];
#pragma unroll
        for (int j = 0; j < XR_CELLS; j += 2) {
            const u64x2 t = rfx_ld2(perm + r0 + j);
            p[j] = t.x;
            p[j + 1] = t.y;
        }
        QR t = qr_at((u64)r0, nb, (u64)n);
#pragma unroll
        for (int j = 0; j < XR_CELLS; j++) {
            if (p[j] < (u64)n) out[p[j]] = t.q;
            qr_up(t, dq, dr, (u64)n);
        }
    }
    for (i64 r = ng * XR_CELLS + tid; r < n; r += nt) {
        const u64 p = perm[r];
        if (p < (u64)n) out[p] = qr_at((u64)r, nb, (u64)n).q;
    }
}
// the sorted short-cuts: d_out[i] = (idx * nb) / n, idx = i or n - 1 - i; four cells per lane and step, 16-byte stores
__global__ __launch_bounds__(RFX_BLOCK) void k_xrank_sorted(i64 n, u64 nb, u64 dq, u64 dr, int desc, u64 *__restrict__ out) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK, n4 = n / 4;
    for (i64 g = tid; g < n4; g += nt) {
        const i64 i0 = g * 4;
        QR t = qr_at((u64)(desc ? n - 1 - i0 : i0), nb, (u64)n);
        u64 o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            o[j] = t.q;
            if (j < 3) { if (desc) qr_down(t, dq, dr, (u64)n); else qr_up(t, dq, dr, (u64)n); }
        }
        bk_st4(out, true, i0, o);
    }
    for (i64 i = n4 * 4 + tid; i < n; i += nt) out[i] = qr_at((u64)(desc ? n - 1 - i : i), nb, (u64)n).q;
}
static int xrank_check(rfx_ctx *c, int64_t n, int64_t nb) {
    RFX_REQUIRE(c && n >= 0 && nb > 0, RFX_EINVAL, "bad argument");
    RFX_REQUIRE(n <= 1 || (unsigned __int128)(n - 1) * (unsigned __int128)nb < ((unsigned __int128)1 << 63), RFX_ELIMIT, "(n - 1) * nb does not fit 63 bits");
    return RFX_OK;
}
static int xrank_grid(rfx_ctx *c, i64 n, int cells) {
    i64 blocks = (n / cells + RFX_BLOCK - 1) / RFX_BLOCK;
    int grid = rfx_grid(c);
    if (blocks < 1) blocks = 1;
    return blocks < grid ? (int)blocks : grid;
}
extern "C" int rfx_hip_xrank(rfx_ctx_t *ctx, const int64_t *d_perm, int64_t n, int64_t nb, int64_t *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    int rc = xrank_check(c, n, nb);
    if (rc != RFX_OK) return rc;
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_perm && d_out && d_perm != d_out && bk_aligned(d_perm), RFX_EINVAL, "a 16-byte aligned permutation and an output of its own expected");
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_xrank, dim3(xrank_grid(c, n, XR_CELLS)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_perm, (i64)n, (u64)nb, (u64)nb / (u64)n, (u64)nb % (u64)n, (u64 *)d_out);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_xrank_sorted(rfx_ctx_t *ctx, int64_t n, int64_t nb, int descending, int64_t *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    int rc = xrank_check(c, n, nb);
    if (rc != RFX_OK) return rc;
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_out && bk_aligned(d_out), RFX_EINVAL, "a 16-byte aligned output expected");
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_xrank_sorted, dim3(xrank_grid(c, n, 4)), dim3(RFX_BLOCK), 0, c->stream, (i64)n, (u64)nb, (u64)nb / (u64)n, (u64)nb % (u64)n, descending != 0, (u64 *)d_out);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

// ---- within ----
// k_cmp_mask's scheme: a wave owns 512 consecutive rows per step, lane l rows 2l, 2l + 1 of each 128-row group; the bytes leave transposed
__global__ __launch_bounds__(RFX_BLOCK) void k_within_i64(const u64 *__restrict__ col, i64 n, i64 lo, i64 hi, int8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 wave_id = (i64)blockIdx.x * (RFX_BLOCK / RFX_WAVE) + (threadIdx.x >> 6), nwaves = (i64)gridDim.x * (RFX_BLOCK / RFX_WAVE), nfull = n / 512;
    for (i64 q = wave_id; q < nfull; q += nwaves) {
        const i64 base = q * 512 + lane * 2;
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64x2 t = rfx_ld2(col + base + j * 128);
            m |= (unsigned)((i64)t.x >= lo && (i64)t.x <= hi) << (2 * j);
            m |= (unsigned)((i64)t.y >= lo && (i64)t.y <= hi) << (2 * j + 1);
        }
        rfx_mask_store512(m, lane, out + q * 512);
    }
    if (blockIdx.x == 0)
        for (i64 r = nfull * 512 + threadIdx.x; r < n; r += RFX_BLOCK) out[r] = (int8_t)((i64)col[r] >= lo && (i64)col[r] <= hi);
}
extern "C" int rfx_hip_within_i64(rfx_ctx_t *ctx, const int64_t *d_col, int64_t lo, int64_t hi, int64_t n, int8_t *d_mask) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && n >= 0, RFX_EINVAL, "bad argument");
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_col && d_mask && bk_aligned(d_col) && ((uintptr_t)d_mask & 7) == 0, RFX_EINVAL, "a 16-byte aligned column and an 8-byte aligned mask expected");
    i64 blocks = (n / 512 + 3) / 4;
    int grid = c->num_cus * 8;
    if (blocks < 1) blocks = 1;
    if (blocks < grid) grid = (int)blocks;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_within_i64, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, (i64)n, (i64)lo, (i64)hi, d_mask);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
