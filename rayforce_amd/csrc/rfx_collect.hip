// rfx_collect.hip -- `row` and the collected column of select ... by: (aggr_row / aggr_collect, core/aggr.c:3021-3136): every group's rows and cells.
// The reference appends cell by cell to one vector per group on one thread; here the answer is ONE buffer in group order plus the groups' offsets:
//   the check      every id that comes from outside and is about to index something is counted against its bound first (k_col_check): a bad one ends
//                  the call before any kernel uses it.
//   the partition  perm = the positions 0 .. m-1 ordered by (group id, position): the packed radix sort of rfx_sort.hip over gid << 32 | position (the
//                  widened 32-bit key form: a dense id in [0, 2^31) keeps its order under that key, and every digit the ids agree on is skipped).  The
//                  sort also leaves the sorted ids as 4-byte cells decoded from the keys, so the offsets are read off the run boundaries with two
//                  coalesced reads per position (k_col_offsets) -- no histogram, no atomics, nothing that depends on which wave ran first.
//   the collect    out_c[j] = col_c[src(j)], src(j) = rows ? rows[perm[j]] : perm[j], for up to RFX_MAX_COLS columns in one launch: a workgroup stages
//                  the sources of its 2048 cells in LDS (perm by 16-byte loads, rows through it), then every column gathers its cells in its own width
//                  and leaves them in whole 16-byte stores -- the groups of cells are cut at the OUTPUT's 16-byte boundaries, so a base that is only
//                  cell-aligned costs single-cell stores at the two ends of the column and nowhere else.  A column without cells is the identity (`row`).
#include "rfx_cells.hpp"

#define COL_STEPS 8
#define COL_TILE (RFX_BLOCK * COL_STEPS) /* cells per workgroup: 2048 (16 KB of staged sources) */

// ---- how many ids lie outside [0, bound): per-wave ballots, one integer add per workgroup ----
__global__ __launch_bounds__(RFX_BLOCK) void k_col_check(const i64 *__restrict__ ids, i64 m, i64 bound, unsigned long long *__restrict__ bad) {
    __shared__ unsigned int wsum[RFX_BLOCK / RFX_WAVE];
    unsigned int cnt = 0; // (wave-uniform)
    const i64 nt = (i64)gridDim.x * RFX_BLOCK;
    for (i64 i0 = blockIdx.x * (i64)RFX_BLOCK; i0 < m; i0 += nt) {
        const i64 i = i0 + threadIdx.x;
        cnt += (unsigned int)__popcll(__ballot(i < m && (u64)ids[i] >= (u64)bound));
    }
    if ((threadIdx.x & (RFX_WAVE - 1)) == 0) wsum[threadIdx.x / RFX_WAVE] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < RFX_BLOCK / RFX_WAVE; w++) t += wsum[w];
        if (t) atomicAdd(bad, t);
    }
}

// ---- offsets off the run boundaries: sorted[] ascending in [0, groups); position j opens every group in (sorted[j - 1], sorted[j]], j == m the rest ----
__global__ __launch_bounds__(RFX_BLOCK) void k_col_offsets(const int *__restrict__ sorted, i64 m, i64 groups, i64 *__restrict__ offsets) {
    const i64 nt = (i64)gridDim.x * RFX_BLOCK;
    for (i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; j <= m; j += nt) {
        const i64 prev = j > 0 ? (i64)sorted[j - 1] : -1;
        i64 g = j < m ? (i64)sorted[j] : groups;
        if (g > groups) g = groups; // (checked ids never get here; never a write beyond offsets[groups])
        for (i64 q = prev < -1 ? 0 : prev + 1; q <= g; q++) offsets[q] = j; // (more than one turn only past a group without rows)
    }
}

struct col_cols {
    const unsigned char *col[RFX_MAX_COLS];
    unsigned char *out[RFX_MAX_COLS];
    int width[RFX_MAX_COLS];
    int ncols;
};

template <int WID> __device__ __forceinline__ u64 col_get(const unsigned char *__restrict__ in, i64 s) {
    if (s < 0) return 0ULL;
    if (!in) return (u64)s;
    return rfx_cell_get<WID>(in, s);
}
// one column over the workgroup's tile [base, base + COL_TILE): the cells in groups of R = 16 / WID that start at the output's 16-byte boundaries -- group k
// holds the cells [base - a + k R, + R), a = the cells between the boundary below the output's base and the base.  A whole group inside the tile and the
// column is one 16-byte store; the pieces at the tile's edges (the neighbouring tile writes the other piece) and at the column's ends go cell by cell.
template <int WID>
__device__ __forceinline__ void col_gather_col(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, const i64 *sl, i64 base, i64 m) {
    constexpr int R = 16 / WID, NGRP = COL_TILE / R + 1;
    const int a = (int)(((uintptr_t)out & 15) / WID);
    const i64 end = base + COL_TILE < m ? base + COL_TILE : m;
    for (int k = threadIdx.x; k < NGRP; k += RFX_BLOCK) {
        const i64 j0 = base - a + (i64)k * R;
        if (j0 >= end) break;
        if (j0 >= base && j0 + R <= end) {
            u64 w[2] = {0ULL, 0ULL};
#pragma unroll
            for (int i = 0; i < R; i++) {
                const u64 v = col_get<WID>(in, sl[j0 - base + i]);
                if (WID == 8) w[i] = v;
                else w[(i * WID) / 8] |= v << (((i * WID) & 7) * 8);
            }
            rfx_v2q o;
            o.x = w[0]; o.y = w[1];
            *(rfx_v2q *)(out + j0 * WID) = o;
        } else {
            for (int i = 0; i < R; i++) {
                const i64 j = j0 + i;
                if (j >= base && j < end) rfx_cell_put<WID>(out, j, col_get<WID>(in, sl[j - base]));
            }
        }
    }
}
__global__ __launch_bounds__(RFX_BLOCK) void k_col_gather(const col_cols C, const i64 *__restrict__ perm, const i64 *__restrict__ rows, i64 m, i64 col_len) {
    __shared__ __attribute__((aligned(16))) i64 sl[COL_TILE];
    const i64 base = (i64)blockIdx.x * COL_TILE;
    for (int g = threadIdx.x; g < COL_TILE / 2; g += RFX_BLOCK) { // perm: two cells per 16-byte load (perm is 16-byte aligned, base even)
        const i64 j0 = base + (i64)g * 2;
        i64 s0 = -1, s1 = -1;
        if (j0 + 2 <= m) {
            const rfx_v2q v = *(const rfx_v2q *)(perm + j0);
            s0 = (i64)v.x;
            s1 = (i64)v.y;
        } else if (j0 < m) s0 = perm[j0];
        if (rows) { // (a position of the partition is below m; anything else reads nothing)
            s0 = (u64)s0 < (u64)m ? rows[s0] : -1;
            s1 = (u64)s1 < (u64)m ? rows[s1] : -1;
        }
        sl[g * 2] = (u64)s0 < (u64)col_len ? s0 : -1;
        sl[g * 2 + 1] = (u64)s1 < (u64)col_len ? s1 : -1;
    }
    __syncthreads();
    for (int k = 0; k < C.ncols; k++) {
        switch (C.width[k]) {
            case 8: col_gather_col<8>(C.col[k], C.out[k], sl, base, m); break;
            case 4: col_gather_col<4>(C.col[k], C.out[k], sl, base, m); break;
            case 2: col_gather_col<2>(C.col[k], C.out[k], sl, base, m); break;
            default: col_gather_col<1>(C.col[k], C.out[k], sl, base, m); break;
        }
    }
}

extern "C" int rfx_hip_ids_check(rfx_ctx_t *ctx, const int64_t *d_ids, int64_t m, int64_t bound, int64_t *bad) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && bad, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(m >= 0, RFX_EINVAL, "negative length");
    *bad = 0;
    if (m == 0) return RFX_OK;
    RFX_REQUIRE(d_ids && ((uintptr_t)d_ids & 7) == 0, RFX_EINVAL, "NULL ids, or ones that are not 8-byte aligned");
    if (bound <= 0) { // (nothing is inside an empty range: no pass needed)
        *bad = m;
        return RFX_OK;
    }
    void *d_bad = NULL;
    int rc = rfx_hip_malloc(ctx, &d_bad, 8);
    if (rc != RFX_OK) return rc;
    unsigned long long h = 0;
    hipError_t e = hipMemsetAsync(d_bad, 0, 8, c->stream);
    RFX_KERNEL_BEGIN(c);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_col_check, dim3(rfx_stream_grid(c, m)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_ids, (i64)m, (i64)bound, (unsigned long long *)d_bad);
        e = hipGetLastError();
    }
    RFX_KERNEL_END(c);
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_bad, 8, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream); // (the scratch goes back idle, whatever happened)
    if (e == hipSuccess) e = es;
    rfx_hip_free(ctx, d_bad);
    RFX_HIP_CHECK(e);
    *bad = (int64_t)h;
    return RFX_OK;
}

extern "C" int rfx_hip_group_partition(rfx_ctx_t *ctx, const int64_t *d_gid, int64_t m, int64_t groups, int64_t *d_offsets, int64_t *d_perm, int32_t *passes) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && d_offsets, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(m >= 0 && groups >= 0, RFX_EINVAL, "negative length");
    RFX_REQUIRE(m < 0x80000000LL, RFX_ELIMIT, "2^31 or more elements");
    RFX_REQUIRE(groups < 0x80000000LL, RFX_ELIMIT, "2^31 or more groups");
    if (passes) *passes = 0;
    if (m == 0) return rfx_hip_fill_i64(ctx, d_offsets, groups + 1, 0);
    RFX_REQUIRE(d_gid && d_perm, RFX_EINVAL, "NULL ids or permutation");
    int64_t bad = 0;
    int rc = rfx_hip_ids_check(ctx, d_gid, m, groups, &bad);
    if (rc != RFX_OK) return rc;
    RFX_REQUIRE(bad == 0, RFX_EINVAL, "a group id outside [0, groups)");
    void *d_sorted = NULL;
    rc = rfx_hip_malloc(ctx, &d_sorted, (size_t)m * 4);
    if (rc != RFX_OK) return rc;
    rc = rfx_hip_sort_values(ctx, d_gid, RFX_I32_WIDE, m, 0, d_sorted, d_perm, passes); // (returns with the stream idle)
    if (rc != RFX_OK) {
        rfx_hip_free(ctx, d_sorted);
        return rc;
    }
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_col_offsets, dim3(rfx_stream_grid(c, m + 1)), dim3(RFX_BLOCK), 0, c->stream, (const int *)d_sorted, (i64)m, (i64)groups, (i64 *)d_offsets);
    RFX_KERNEL_END(c);
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    rfx_hip_free(ctx, d_sorted);
    RFX_HIP_CHECK(e);
    return RFX_OK;
}

extern "C" int rfx_hip_group_collect(rfx_ctx_t *ctx, const rfx_collect_col_t *cols, int ncols, const int64_t *d_perm, const int64_t *d_rows, int64_t m,
                                     int64_t col_len) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && cols, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(ncols >= 1 && ncols <= RFX_MAX_COLS, RFX_EINVAL, "1 .. RFX_MAX_COLS columns per launch");
    RFX_REQUIRE(m >= 0 && col_len >= 0, RFX_EINVAL, "negative length");
    if (m == 0) return RFX_OK;
    RFX_REQUIRE(m < 0x80000000LL, RFX_ELIMIT, "2^31 or more elements");
    RFX_REQUIRE(d_perm && ((uintptr_t)d_perm & 15) == 0, RFX_EINVAL, "NULL permutation, or one that is not 16-byte aligned");
    RFX_REQUIRE(((uintptr_t)d_rows & 7) == 0, RFX_EINVAL, "row ids that are not 8-byte aligned");
    col_cols C;
    memset(&C, 0, sizeof(C));
    for (int k = 0; k < ncols; k++) {
        const int w = cols[k].width;
        RFX_REQUIRE(rfx_width_ok(w), RFX_EINVAL, "a cell width that is not 1, 2, 4 or 8 bytes");
        RFX_REQUIRE(cols[k].d_col || w == 8, RFX_EINVAL, "the identity column has 8-byte cells");
        RFX_REQUIRE(((uintptr_t)cols[k].d_col & (uintptr_t)(w - 1)) == 0, RFX_EINVAL, "a column that is not cell-aligned");
        RFX_REQUIRE(cols[k].d_out && ((uintptr_t)cols[k].d_out & (uintptr_t)(w - 1)) == 0, RFX_EINVAL, "NULL result, or one that is not cell-aligned");
        C.col[k] = (const unsigned char *)cols[k].d_col;
        C.out[k] = (unsigned char *)cols[k].d_out;
        C.width[k] = w;
    }
    C.ncols = ncols;
    rfx_ctx_device_written(c);
    const i64 nblk = (m + COL_TILE - 1) / COL_TILE; // < 2^20
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_col_gather, dim3((unsigned)nblk), dim3(RFX_BLOCK), 0, c->stream, C, (const i64 *)d_perm, (const i64 *)d_rows, (i64)m, (i64)col_len);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
