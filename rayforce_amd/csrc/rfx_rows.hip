// rfx_rows.hip -- the row verbs: filter (ray_filter, core/items.c:338-396), take (ray_take, core/items.c:398-734), reverse (ray_reverse,
// core/compose.c:144-202) -- rows out of columns, cell for cell.
//   compact   after rfx_hip_where_begin (rfx_where.hip: 1 bit per row in the pair-split 128 layout + the scanned per-512-row offsets in the context):
//             the ordered compaction of 1 .. RFX_MAX_KEYS columns in one launch, the bitmap read once.  A wave owns a CONTIGUOUS run of chunks, so a
//             contiguous run of every output.  Two write-outs: DIRECT -- the masked stores of k_compact_cols; RING -- k_emit_ids_wc's wave-private LDS
//             ring, one per column: selected cells leave as whole, aligned 64-cell lines (a short first flush reaches alignment, the last one drains).
//             Wave-private: no workgroup barrier, a wave that runs out of chunks just ends.
//   take      out[i] = col[(j0 + i) mod l]: without a wrap a streaming copy (16-byte loads and stores); else a thread owns a contiguous run of output
//             cells (whole 16-byte stores), takes ONE 64-bit remainder at the run's first cell and wraps by compare-and-subtract.
//   reverse   the same run kernel walking the column downwards;  fill: an atom's cell m times.
// Cell kinds (rfx_hip.h): RFX_ROWS_8, RFX_ROWS_4W (widened 8-byte cells in, 4-byte cells out: the null's promotion undone), RFX_ROWS_1.
#include "rfx_cells.hpp"

#define ROWS_CHUNK 512 /* rows per chunk of the selection: 4 groups of 128 = 8 bitmap words (RFX_CHUNK of rfx_where.hip) */
#define ROWS_RING 256  /* cells per ring: at most 63 left over + 128 of one group */
// Which write-out ships: the ring only where it beat the direct form by more than the spread of two runs of one build (1e8 rows, I64 columns; measured at
// 1, 4 and 8 columns and 1 %, 10 %, 50 % selected -- DESIGN.md section 3, "Row verbs"): one column up to 10 % selected (at 50 % the two tie), two to four
// columns always.  At eight columns the direct form won at every selectivity (the ring's 64 KB of LDS per workgroup); five to seven are not measured: direct.
static int rows_shipped_form(int ncols, long long nrows, long long count) {
    if (ncols == 1) return count <= nrows / 10 ? RFX_ROWS_RING : RFX_ROWS_DIRECT;
    return ncols <= 4 ? RFX_ROWS_RING : RFX_ROWS_DIRECT;
}

typedef unsigned v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u64 rows_lanemask_lt() {
    const unsigned l = threadIdx.x & 63;
    return (l == 0) ? 0ULL : (~0ULL >> (64 - l));
}
// a widened 4-byte cell back in 32 bits (rfx_hip_widen_i32: NULL_I32 -> NULL_I64, every other cell its sign extension)
__device__ __forceinline__ u64 rows_narrow(u64 v) { return (i64)v == RFX_NULL_I64_D ? 0x80000000ULL : (v & 0xFFFFFFFFULL); }
// the cell at `row` in its OUTPUT form (the low `kind` bytes)
__device__ __forceinline__ u64 rows_ld(const void *col, int kind, i64 row) {
    if (kind == RFX_ROWS_1) return ((const unsigned char *)col)[row];
    const u64 v = ((const u64 *)col)[row];
    return kind == RFX_ROWS_4W ? rows_narrow(v) : v;
}
__device__ __forceinline__ void rows_st(void *out, int kind, i64 r, u64 v) {
    if (kind == RFX_ROWS_8) ((u64 *)out)[r] = v;
    else if (kind == RFX_ROWS_4W) ((unsigned *)out)[r] = (unsigned)v;
    else ((unsigned char *)out)[r] = (unsigned char)v;
}
// rows `row` (even) and row + 1: one 16-byte load for the 8-byte kinds when both rows exist
__device__ __forceinline__ void rows_ld_pair(const void *col, int kind, i64 row, bool pair_ok, u64 &x, u64 &y) {
    y = 0;
    if (kind == RFX_ROWS_1) {
        x = ((const unsigned char *)col)[row];
        if (pair_ok) y = ((const unsigned char *)col)[row + 1];
        return;
    }
    if (pair_ok) {
        const u64x2 t = rfx_ld2((const u64 *)col + row);
        x = t.x;
        y = t.y;
    } else x = ((const u64 *)col)[row];
    if (kind == RFX_ROWS_4W) {
        x = rows_narrow(x);
        y = rows_narrow(y);
    }
}

// ---------------- ordered compaction ----------------
struct RowsArgs {
    const void *src[RFX_MAX_KEYS];
    void *dst[RFX_MAX_KEYS];
    unsigned kinds; // 4 bits per column: its cell kind
};
#define ROWS_KIND(A, c) ((int)(((A).kinds >> (4 * (c))) & 15u))

// `count` = cells of every output (the selection's size): no store lands beyond it, whatever the bitmap and the offsets say; no row >= nrows is read.
template <int NCOL, bool RING>
__global__ __launch_bounds__(RFX_BLOCK) void k_rows_compact(const u64 *__restrict__ bitmap, const i64 *__restrict__ chunk_off, i64 nrows, i64 count,
                                                          const RowsArgs A) {
    __shared__ u64 ring[RING ? RFX_BLOCK / RFX_WAVE : 1][RING ? NCOL : 1][RING ? ROWS_RING : 1];
    const int lane = threadIdx.x & 63;
    u64(*R)[RING ? ROWS_RING : 1] = ring[RING ? (threadIdx.x >> 6) : 0];
    const i64 wave_id = (i64)blockIdx.x * (RFX_BLOCK / RFX_WAVE) + (threadIdx.x >> 6);
    const i64 nwaves = (i64)gridDim.x * (RFX_BLOCK / RFX_WAVE);
    const i64 nchunks = (nrows + ROWS_CHUNK - 1) / ROWS_CHUNK;
    const i64 per = (nchunks + nwaves - 1) / nwaves;
    const i64 q0 = wave_id * per, q1 = (q0 + per < nchunks) ? q0 + per : nchunks;
    if (q0 >= q1) return;
    const u64 below = rows_lanemask_lt();
    i64 gpos = chunk_off[q0]; // output index of the next cell of this wave's run (RING: of the ring's head)
    unsigned head = 0, fill = 0;
    u64 nxt[8]; // the next chunk's bitmap words, fetched while the current chunk is compacted
#pragma unroll
    for (int i = 0; i < 8; i++) nxt[i] = bitmap[q0 * 8 + i];
    for (i64 q = q0; q < q1; q++) {
        u64 w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = nxt[i];
        if (q + 1 < q1) {
#pragma unroll
            for (int i = 0; i < 8; i++) nxt[i] = bitmap[(q + 1) * 8 + i];
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const u64 w0 = w[2 * g], w1 = w[2 * g + 1];
            if ((w0 | w1) == 0) continue; // (wave-uniform)
            const i64 row = q * ROWS_CHUNK + g * 128 + lane * 2;
            const unsigned s0 = ((unsigned)(w0 >> lane) & 1u) & (unsigned)(row < nrows), s1 = ((unsigned)(w1 >> lane) & 1u) & (unsigned)(row + 1 < nrows);
            const unsigned rank = (unsigned)(__popcll(w0 & below) + __popcll(w1 & below));
            const unsigned added = (unsigned)(__popcll(w0) + __popcll(w1));
            if (s0 | s1) { // a lane fetches its row pair only when one of the two rows is selected
                const bool pair_ok = row + 1 < nrows;
                u64 x[NCOL], y[NCOL]; // every column's pair in flight before the first store: a store between two loads would order them
#pragma unroll
                for (int c = 0; c < NCOL; c++) rows_ld_pair(A.src[c], ROWS_KIND(A, c), row, pair_ok, x[c], y[c]);
#pragma unroll
                for (int c = 0; c < NCOL; c++) {
                    if constexpr (RING) {
                        const unsigned r = head + fill + rank;
                        if (s0) R[c][r & (ROWS_RING - 1)] = x[c];
                        if (s1) R[c][(r + s0) & (ROWS_RING - 1)] = y[c];
                    } else {
                        const int kind = ROWS_KIND(A, c);
                        const i64 r = gpos + rank;
                        if (s0 && r < count) rows_st(A.dst[c], kind, r, x[c]);
                        if (s1 && r + s0 < count) rows_st(A.dst[c], kind, r + s0, y[c]);
                    }
                }
            }
            if constexpr (RING) {
                fill += added;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the wave's ring writes have landed before other lanes read them
                while (fill >= 64) {
                    const unsigned k = 64 - (unsigned)(gpos & 63); // a short first flush, then whole aligned 64-cell lines
#pragma unroll
                    for (int c = 0; c < NCOL; c++)
                        if ((unsigned)lane < k && gpos + lane < count) rows_st(A.dst[c], ROWS_KIND(A, c), gpos + lane, R[c][(head + lane) & (ROWS_RING - 1)]);
                    gpos += k;
                    head += k;
                    fill -= k;
                }
                asm volatile("" ::: "memory");
            } else gpos += added;
        }
    }
    if constexpr (RING) {
#pragma unroll
        for (int c = 0; c < NCOL; c++)
            if ((unsigned)lane < fill && gpos + lane < count) rows_st(A.dst[c], ROWS_KIND(A, c), gpos + lane, R[c][(head + lane) & (ROWS_RING - 1)]);
    }
}

static inline bool rows_kind_ok(int kind) { return kind == RFX_ROWS_8 || kind == RFX_ROWS_4W || kind == RFX_ROWS_1; }
static inline bool rows_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int rfx_hip_rows_compact(rfx_ctx_t *c, const void *const *d_cols, const int32_t *kinds, int ncols, void *const *d_outs, int form) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(c->where_n >= 0, RFX_ESTATE, "rows_compact without a successful where_begin");
    RFX_REQUIRE(ncols >= 1 && ncols <= RFX_MAX_KEYS && d_cols && kinds && d_outs, RFX_EINVAL, "1..RFX_MAX_KEYS columns");
    RFX_REQUIRE(form == RFX_ROWS_FORM_DEFAULT || form == RFX_ROWS_DIRECT || form == RFX_ROWS_RING, RFX_EINVAL, "unknown write-out form");
    if (c->where_count == 0) return RFX_OK;
    RowsArgs A;
    memset(&A, 0, sizeof(A));
    for (int k = 0; k < ncols; k++) {
        RFX_REQUIRE(rows_kind_ok(kinds[k]), RFX_EINVAL, "unknown cell kind");
        RFX_REQUIRE(d_cols[k] && d_outs[k], RFX_EINVAL, "NULL column");
        RFX_REQUIRE(kinds[k] == RFX_ROWS_1 || rows_aligned16(d_cols[k]), RFX_EINVAL, "8-byte columns must be 16-byte aligned");
        A.src[k] = d_cols[k];
        A.dst[k] = d_outs[k];
        A.kinds |= (unsigned)kinds[k] << (4 * k);
    }
    const i64 nrows = c->where_n, count = c->where_count;
    if (form == RFX_ROWS_FORM_DEFAULT) form = rows_shipped_form(ncols, nrows, count);
    const i64 nchunks = (nrows + ROWS_CHUNK - 1) / ROWS_CHUNK;
    int grid = c->num_cus * 16;
    if ((i64)grid * 4 > nchunks) grid = (int)((nchunks + 3) / 4);
    const u64 *bm = (const u64 *)c->d_bitmap;
    const i64 *off = (const i64 *)c->d_blksum;
    RFX_KERNEL_BEGIN(c);
#define RC(N)                                                                                                                                         \
    case N:                                                                                                                                           \
        if (form == RFX_ROWS_RING) hipLaunchKernelGGL((k_rows_compact<N, true>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, bm, off, nrows, count, A); \
        else hipLaunchKernelGGL((k_rows_compact<N, false>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, bm, off, nrows, count, A);                     \
        break;
    switch (ncols) {
        RC(1) RC(2) RC(3) RC(4) RC(5) RC(6) RC(7) RC(8)
        default: break;
    }
#undef RC
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

// ---------------- take / reverse / fill ----------------
// n16 whole 16-byte vectors, then the bytes [16 * n16, nbytes)
__global__ __launch_bounds__(RFX_BLOCK) void k_rows_copy16(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst, i64 n16, i64 nbytes) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK;
    for (i64 g = tid; g < n16; g += nt) __builtin_nontemporal_store(__builtin_nontemporal_load((const rfx_v2q *)src + g), (rfx_v2q *)dst + g);
    for (i64 b = n16 * 16 + tid; b < nbytes; b += nt) dst[b] = src[b];
}
// widened cells -> 4-byte cells, four per thread and step
__global__ __launch_bounds__(RFX_BLOCK) void k_rows_narrow16(const u64 *__restrict__ src, unsigned *__restrict__ dst, i64 m) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK, m4 = m / 4;
    for (i64 g = tid; g < m4; g += nt) {
        const rfx_v2q a = __builtin_nontemporal_load((const rfx_v2q *)(src + 4 * g)), b = __builtin_nontemporal_load((const rfx_v2q *)(src + 4 * g + 2));
        v4u o;
        o.x = (unsigned)rows_narrow(a.x); o.y = (unsigned)rows_narrow(a.y); o.z = (unsigned)rows_narrow(b.x); o.w = (unsigned)rows_narrow(b.y);
        __builtin_nontemporal_store(o, (v4u *)(dst + 4 * g));
    }
    for (i64 r = m4 * 4 + tid; r < m; r += nt) dst[r] = (unsigned)rows_narrow(src[r]);
}
// A thread owns ROWS_RUN(KIND) consecutive OUTPUT cells (64 / 32 / 16 bytes: whole 16-byte stores): cell i = col[(j0 + i) mod l], or col[l - 1 - i]
// (REV; m <= l then).  One remainder per run; within it the column index steps by one and wraps by compare-and-subtract.
#define ROWS_RUN(KIND) ((KIND) == RFX_ROWS_1 ? 16 : 8)
template <int KIND, bool REV>
__global__ __launch_bounds__(RFX_BLOCK) void k_rows_run(const void *__restrict__ col, i64 l, i64 j0, i64 m, void *__restrict__ out) {
    constexpr int RUN = ROWS_RUN(KIND);
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK;
    const i64 nruns = (m + RUN - 1) / RUN;
    for (i64 t = tid; t < nruns; t += nt) {
        const i64 i0 = t * RUN;
        i64 j = REV ? l - 1 - i0 : (i64)(((u64)j0 + (u64)i0) % (u64)l);
        u64 v[RUN];
#pragma unroll
        for (int k = 0; k < RUN; k++) {
            v[k] = 0;
            if (i0 + k < m) {
                v[k] = rows_ld(col, KIND, j);
                if (REV) j--;
                else {
                    j++;
                    if (j >= l) j -= l;
                }
            }
        }
        if (i0 + RUN <= m) {
            if (KIND == RFX_ROWS_8) {
#pragma unroll
                for (int k = 0; k < RUN; k += 2) {
                    rfx_v2q o;
                    o.x = v[k]; o.y = v[k + 1];
                    __builtin_nontemporal_store(o, (rfx_v2q *)((u64 *)out + i0 + k));
                }
            } else if (KIND == RFX_ROWS_4W) {
#pragma unroll
                for (int k = 0; k < RUN; k += 4) {
                    v4u o;
                    o.x = (unsigned)v[k]; o.y = (unsigned)v[k + 1]; o.z = (unsigned)v[k + 2]; o.w = (unsigned)v[k + 3];
                    __builtin_nontemporal_store(o, (v4u *)((unsigned *)out + i0 + k));
                }
            } else {
                unsigned p[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < RUN; k++) p[k >> 2] |= (unsigned)(v[k] & 0xFF) << (8 * (k & 3));
                v4u o;
                o.x = p[0]; o.y = p[1]; o.z = p[2]; o.w = p[3];
                __builtin_nontemporal_store(o, (v4u *)((unsigned char *)out + i0));
            }
        } else {
#pragma unroll
            for (int k = 0; k < RUN; k++)
                if (i0 + k < m) rows_st(out, KIND, i0 + k, v[k]);
        }
    }
}
__global__ __launch_bounds__(RFX_BLOCK) void k_rows_fill(u64 pattern, unsigned char *__restrict__ dst, i64 n16, i64 nbytes) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK;
    rfx_v2q o;
    o.x = pattern; o.y = pattern;
    for (i64 g = tid; g < n16; g += nt) __builtin_nontemporal_store(o, (rfx_v2q *)dst + g);
    for (i64 b = n16 * 16 + tid; b < nbytes; b += nt) dst[b] = (unsigned char)(pattern >> (8 * (b & 7)));
}

template <bool REV>
static void rows_run_launch(rfx_ctx *c, int kind, const void *d_col, i64 l, i64 j0, i64 m, void *d_out) {
    const int grid = rfx_stream_grid(c, (m + ROWS_RUN(kind) - 1) / ROWS_RUN(kind));
    if (kind == RFX_ROWS_8) hipLaunchKernelGGL((k_rows_run<RFX_ROWS_8, REV>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, d_col, l, j0, m, d_out);
    else if (kind == RFX_ROWS_4W) hipLaunchKernelGGL((k_rows_run<RFX_ROWS_4W, REV>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, d_col, l, j0, m, d_out);
    else hipLaunchKernelGGL((k_rows_run<RFX_ROWS_1, REV>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, d_col, l, j0, m, d_out);
}

extern "C" int rfx_hip_rows_take(rfx_ctx_t *c, const void *d_col, int32_t kind, int64_t l, int64_t j0, int64_t m, void *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(rows_kind_ok(kind), RFX_EINVAL, "unknown cell kind");
    RFX_REQUIRE(l >= 0 && m >= 0, RFX_EINVAL, "negative length");
    if (m == 0) return RFX_OK;
    RFX_REQUIRE(l > 0 && j0 >= 0 && j0 < l, RFX_EINVAL, "take from an empty column, or a start outside it");
    RFX_REQUIRE(d_col && d_out && rows_aligned16(d_out), RFX_EINVAL, "NULL column, or a result that is not 16-byte aligned");
    RFX_REQUIRE((size_t)m <= (SIZE_MAX >> 4), RFX_ELIMIT, "count");
    const size_t in_bytes = kind == RFX_ROWS_1 ? 1 : 8;
    const unsigned char *src = (const unsigned char *)d_col + (size_t)j0 * in_bytes;
    RFX_KERNEL_BEGIN(c);
    if (m <= l - j0 && rows_aligned16(src)) { // head, tail, range: a streaming copy
        if (kind == RFX_ROWS_4W) hipLaunchKernelGGL(k_rows_narrow16, dim3(rfx_stream_grid(c, m / 4)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)src, (unsigned *)d_out, (i64)m);
        else {
            const i64 nbytes = (i64)m * (i64)in_bytes;
            hipLaunchKernelGGL(k_rows_copy16, dim3(rfx_stream_grid(c, nbytes / 16)), dim3(RFX_BLOCK), 0, c->stream, src, (unsigned char *)d_out, nbytes / 16, nbytes);
        }
    } else rows_run_launch<false>(c, kind, d_col, (i64)l, (i64)j0, (i64)m, d_out); // (a range from an odd cell: the run kernel never wraps there)
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_rows_reverse(rfx_ctx_t *c, const void *d_col, int32_t kind, int64_t l, void *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(rows_kind_ok(kind), RFX_EINVAL, "unknown cell kind");
    RFX_REQUIRE(l >= 0, RFX_EINVAL, "negative length");
    if (l == 0) return RFX_OK;
    RFX_REQUIRE(d_col && d_out && rows_aligned16(d_out), RFX_EINVAL, "NULL column, or a result that is not 16-byte aligned");
    RFX_KERNEL_BEGIN(c);
    rows_run_launch<true>(c, kind, d_col, (i64)l, 0, (i64)l, d_out);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_rows_fill(rfx_ctx_t *c, int32_t kind, uint64_t bits, int64_t m, void *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(rows_kind_ok(kind), RFX_EINVAL, "unknown cell kind");
    RFX_REQUIRE(m >= 0, RFX_EINVAL, "negative length");
    if (m == 0) return RFX_OK;
    RFX_REQUIRE(d_out && rows_aligned16(d_out), RFX_EINVAL, "NULL result, or one that is not 16-byte aligned");
    RFX_REQUIRE((size_t)m <= (SIZE_MAX >> 4), RFX_ELIMIT, "count");
    const u64 pattern = kind == RFX_ROWS_8 ? bits : (kind == RFX_ROWS_4W ? (bits & 0xFFFFFFFFULL) * 0x100000001ULL : (bits & 0xFFULL) * 0x0101010101010101ULL);
    const i64 nbytes = (i64)m * kind;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_rows_fill, dim3(rfx_stream_grid(c, nbytes / 16)), dim3(RFX_BLOCK), 0, c->stream, pattern, (unsigned char *)d_out, nbytes / 16, nbytes);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
