// rfx_lastdev.hip -- the small kernels behind `last` under by: and behind `dev` (scalar: ray_dev, core/math.c:2628-2699; grouped: aggr_dev,
// core/aggr.c:2250-2350,2864-2929).
//
// last under by: is a MAX in disguise.  The answer of a group is the value at its highest selected row whose cell is non-null (the reference's
// one-chunk answer: aggr_last_partial keeps the last non-null value of every group, core/aggr.c:851-895), so the planner (rfx_exec_lastdev.c)
//   k_last_rows     derives, per shard, the i64 column  null(col[i]) ? null : row0 + i,
//   (every grouped kernel family then runs an ordinary i64 MAX over it: LDS and device atomics, value planes, the shard merge -- unchanged)
//   k_last_gather   reads the column at the rows that MAX found, out of the shard that owns each row; a null accumulator emits the typed null.
//
// dev under by: keeps the reference's three sums per group -- sum (f64)x, sum (f64)x * (f64)x, the non-null count -- as ordinary null-skipping
// accumulators of the grouped kernels (two AVGs and an i64 SUM), fed by
//   k_dev_derive    sq[i] = null ? NaN : (f64)x * (f64)x,  nn[i] = null ? 0 : 1,
//   k_dev_finalise  n == 0 -> null, n == 1 -> 0.0, else mean = s/n, var = sq/n - mean * mean, var < 0 ? 0 : sqrt(var) -- that formula and not
//                   Welford's, so the answer cancels where the reference's does.  (-ffp-contract=off for every file of the library: not fused.)
//
// scalar dev is ray_dev's two passes over the column: l = non-null count and the sum (k_dev_sum; i64: the wrapping integer sum), favg = sum / l,
// then sum (x - favg)^2 (k_dev_sqsub); per-workgroup partials are folded on the host in block order, so a call is run-to-run deterministic.
#include "rfx_common.hpp"
#include <math.h>
#include <stdlib.h>

#define LD_MAX_SHARDS 16

__device__ __forceinline__ bool ld_is_null(u64 x, int f64) { return f64 ? rfx_isnan_bits(x) : (i64)x == RFX_NULL_I64_D; }

__global__ __launch_bounds__(RFX_BLOCK) void k_last_rows(const u64 *__restrict__ col, int f64, i64 n, i64 row0, i64 *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) out[i] = ld_is_null(col[i], f64) ? RFX_NULL_I64_D : row0 + i;
}

struct LastPieces {
    int n;
    const u64 *base[LD_MAX_SHARDS];
    i64 row0[LD_MAX_SHARDS], len[LD_MAX_SHARDS];
};
// (rows == out is allowed: every thread reads its own cell before it writes it)
__global__ __launch_bounds__(RFX_BLOCK) void k_last_gather(const LastPieces P, const i64 *rows, i64 g, int f64, u64 *out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < g; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 r = rows[i];
        u64 v = f64 ? RFX_NAN_BITS : (u64)RFX_NULL_I64_D;
        for (int s = 0; s < P.n; s++)
            if (r >= P.row0[s] && r - P.row0[s] < P.len[s]) v = P.base[s][r - P.row0[s]]; // (a null row is below every row0: no piece owns it)
        out[i] = v;
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_dev_derive(const u64 *__restrict__ col, int f64, i64 n, double *__restrict__ sq, i64 *__restrict__ nn) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const u64 x = col[i];
        const bool null = ld_is_null(x, f64);
        const double d = f64 ? rfx_as_f64(x) : (double)(i64)x;
        sq[i] = null ? rfx_as_f64(RFX_NAN_BITS) : d * d;
        nn[i] = null ? 0 : 1;
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_dev_finalise(const double *__restrict__ mean, const double *__restrict__ meansq, const i64 *__restrict__ cnt, i64 g,
                                                            double *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < g; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 n = cnt[i];
        double r;
        if (n <= 0) r = rfx_as_f64(RFX_NAN_BITS);
        else if (n == 1) r = 0.0;
        else {
            const double m = mean[i];
            const double var = meansq[i] - m * m;
            r = var < 0 ? 0.0 : sqrt(var);
        }
        out[i] = r;
    }
}

// ---- scalar dev: block partials {integer sum bits | f64 sum bits, count} and {sum of squared differences} ----
__device__ __forceinline__ double ld_block_sum_f64(double v, double *lds) {
    for (int s = 32; s >= 1; s >>= 1) v += rfx_as_f64(rfx_shfl_xor_u64(rfx_as_u64(v), s));
    if (threadIdx.x % RFX_WAVE == 0) lds[threadIdx.x / RFX_WAVE] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < RFX_BLOCK / RFX_WAVE; w++) r += lds[w];
    __syncthreads();
    return r; // (thread 0 only)
}
__device__ __forceinline__ u64 ld_block_sum_u64(u64 v, u64 *lds) {
    for (int s = 32; s >= 1; s >>= 1) v += rfx_shfl_xor_u64(v, s);
    if (threadIdx.x % RFX_WAVE == 0) lds[threadIdx.x / RFX_WAVE] = v;
    __syncthreads();
    u64 r = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < RFX_BLOCK / RFX_WAVE; w++) r += lds[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(RFX_BLOCK) void k_dev_sum(const u64 *__restrict__ col, int f64, i64 n, u64 *__restrict__ part /* [grid][2] */) {
    __shared__ u64 lds[RFX_BLOCK / RFX_WAVE];
    u64 isum = 0, cnt = 0;
    double fsum = 0.0;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const u64 x = col[i];
        const bool ok = !ld_is_null(x, f64);
        cnt += ok;
        if (f64) fsum += ok ? rfx_as_f64(x) : 0.0;
        else isum += ok ? x : 0ULL;
    }
    const u64 c = ld_block_sum_u64(cnt, lds);
    u64 s;
    if (f64) s = rfx_as_u64(ld_block_sum_f64(fsum, (double *)lds));
    else s = ld_block_sum_u64(isum, lds);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s;
        part[2 * (size_t)blockIdx.x + 1] = c;
    }
}
__global__ __launch_bounds__(RFX_BLOCK) void k_dev_sqsub(const u64 *__restrict__ col, int f64, i64 n, double favg, double *__restrict__ part /* [grid] */) {
    __shared__ double lds[RFX_BLOCK / RFX_WAVE];
    double acc = 0.0;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const u64 x = col[i];
        const double t = (f64 ? rfx_as_f64(x) : (double)(i64)x) - favg;
        acc += ld_is_null(x, f64) ? 0.0 : t * t;
    }
    const double r = ld_block_sum_f64(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

static inline unsigned ld_grid(const rfx_ctx *c, i64 n) {
    const i64 want = (n + RFX_BLOCK - 1) / RFX_BLOCK;
    const i64 cap = (i64)c->num_cus * 16;
    return (unsigned)(want < 1 ? 1 : (want < cap ? want : cap));
}

extern "C" int rfx_hip_last_rows(rfx_ctx_t *c, const void *d_col, int32_t col_type, int64_t nrows, int64_t row0, int64_t *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(col_type == RFX_I64 || col_type == RFX_F64, RFX_EINVAL, "column type must be i64 or f64");
    if (nrows <= 0) return RFX_OK;
    RFX_REQUIRE(d_col && d_out, RFX_EINVAL, "device buffers expected");
    // d_out is usually a pooled block that held another query's derived rows a moment ago: what a scope pass remembered about a value column at this
    // address (the one-pass partitions, the scope histogram: matched by pointer, size and predicates) must not outlive the rewrite
    c->ck_valid = 0;
    c->pc_valid = 0;
    hipLaunchKernelGGL(k_last_rows, dim3(ld_grid(c, nrows)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, (int)(col_type == RFX_F64), (i64)nrows, (i64)row0, (i64 *)d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_last_gather(rfx_ctx_t *c, const void *const *d_pieces, const int64_t *row0, const int64_t *len, int npieces, int32_t col_type,
                                   const int64_t *d_rows, int64_t groups, void *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(col_type == RFX_I64 || col_type == RFX_F64, RFX_EINVAL, "column type must be i64 or f64");
    RFX_REQUIRE(npieces >= 0 && npieces <= LD_MAX_SHARDS && (npieces == 0 || (d_pieces && row0 && len)), RFX_ELIMIT, "0..16 pieces of the column");
    if (groups <= 0) return RFX_OK;
    RFX_REQUIRE(d_rows && d_out, RFX_EINVAL, "device buffers expected");
    LastPieces P;
    memset(&P, 0, sizeof(P));
    for (int s = 0; s < npieces; s++) {
        if (len[s] <= 0) continue;
        RFX_REQUIRE(d_pieces[s] && row0[s] >= 0, RFX_EINVAL, "a piece with rows needs an address and a first row");
        P.base[P.n] = (const u64 *)d_pieces[s];
        P.row0[P.n] = row0[s];
        P.len[P.n++] = len[s];
    }
    hipLaunchKernelGGL(k_last_gather, dim3(ld_grid(c, groups)), dim3(RFX_BLOCK), 0, c->stream, P, (const i64 *)d_rows, (i64)groups, (int)(col_type == RFX_F64), (u64 *)d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_dev_derive(rfx_ctx_t *c, const void *d_col, int32_t col_type, int64_t nrows, double *d_sq, int64_t *d_nn) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(col_type == RFX_I64 || col_type == RFX_F64, RFX_EINVAL, "column type must be i64 or f64");
    if (nrows <= 0) return RFX_OK;
    RFX_REQUIRE(d_col && d_sq && d_nn, RFX_EINVAL, "device buffers expected");
    hipLaunchKernelGGL(k_dev_derive, dim3(ld_grid(c, nrows)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, (int)(col_type == RFX_F64), (i64)nrows, d_sq, (i64 *)d_nn);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_dev_finalise(rfx_ctx_t *c, const double *d_mean, const double *d_meansq, const int64_t *d_cnt, int64_t groups, double *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    if (groups <= 0) return RFX_OK;
    RFX_REQUIRE(d_mean && d_meansq && d_cnt && d_out, RFX_EINVAL, "device buffers expected");
    hipLaunchKernelGGL(k_dev_finalise, dim3(ld_grid(c, groups)), dim3(RFX_BLOCK), 0, c->stream, d_mean, d_meansq, (const i64 *)d_cnt, (i64)groups, d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

// ray_dev over a plain column of nrows cells (syncs)
extern "C" int rfx_hip_dev(rfx_ctx_t *c, const void *d_col, int32_t col_type, int64_t nrows, rfx_value_t *out) {
    RFX_REQUIRE(c && out, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(col_type == RFX_I64 || col_type == RFX_F64, RFX_EINVAL, "column type must be i64 or f64");
    RFX_REQUIRE(nrows <= 0 || d_col, RFX_EINVAL, "device column expected");
    memset(out, 0, sizeof(*out));
    out->type = RFX_F64;
    out->is_null = 1;
    out->i = (int64_t)RFX_NAN_BITS;
    if (nrows <= 0) return RFX_OK;
    const int f64 = col_type == RFX_F64;
    const unsigned grid = ld_grid(c, nrows);
    int rc = rfx_ws_reserve(c, (size_t)grid * 16);
    if (rc != RFX_OK) return rc;
    u64 *h = (u64 *)malloc((size_t)grid * 16);
    RFX_REQUIRE(h, RFX_ENOMEM, "host staging");
    hipLaunchKernelGGL(k_dev_sum, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, f64, (i64)nrows, (u64 *)c->d_ws);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, c->d_ws, (size_t)grid * 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        free(h);
        rfx_set_error("rfx_hip_dev: sum pass: %s", hipGetErrorString(e));
        return RFX_EHIP;
    }
    u64 isum = 0;
    i64 l = 0;
    double fsum = 0.0;
    for (unsigned b = 0; b < grid; b++) {
        double d;
        memcpy(&d, &h[2 * b], 8);
        fsum += d;
        isum += h[2 * b];
        l += (i64)h[2 * b + 1];
    }
    if (l <= 1) {
        free(h);
        if (l == 1) {
            out->is_null = 0;
            out->f = 0.0;
        }
        return RFX_OK;
    }
    const double favg = (f64 ? fsum : (double)(i64)isum) / (double)l;
    hipLaunchKernelGGL(k_dev_sqsub, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, f64, (i64)nrows, favg, (double *)c->d_ws);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, c->d_ws, (size_t)grid * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        free(h);
        rfx_set_error("rfx_hip_dev: squares pass: %s", hipGetErrorString(e));
        return RFX_EHIP;
    }
    double sq = 0.0;
    for (unsigned b = 0; b < grid; b++) {
        double d;
        memcpy(&d, &h[b], 8);
        sq += d;
    }
    free(h);
    out->f = sqrt(sq / (double)l);
    out->is_null = out->f != out->f;
    return RFX_OK;
}
