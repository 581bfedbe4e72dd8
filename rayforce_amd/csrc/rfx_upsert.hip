// rfx_upsert.hip -- upsert (ray_upsert, core/update.c:556-750) and insert of a keyed batch once the index is known: idx[j] = the table row batch row j
// matched, or none.  The reference walks every column cell by cell (at_idx / push_obj / set_idx); here:
//   the plan    dest[j] = idx[j] when j is the LAST batch row that matched that row, -1 when a later one did, n + rank(j) when j matched none, rank the
//               exclusive count of unmatched rows before j.  Last writer wins over an UNINITIALISED scratch W of n 4-byte cells, touched at matched rows
//               only: k_up_clear stores -1 at W[idx[j]], k_up_max atomicMax(W[idx[j]], j) (and counts its block's unmatched rows), k_up_dest compares
//               W[idx[j]] == j inside the ordered scan that writes dest.  Integer max commutes: the outcome does not depend on the order of the atomics.
//   the place   out_c[dest[j]] = batch_c[j] for up to RFX_MAX_COLS columns in one launch: a workgroup stages its 2048 cells of dest in LDS (one 16-byte
//               load per lane and access), then reads every column once, 16 bytes per lane, and stores cell by cell -- the appended cells at consecutive
//               addresses, the matched ones a scatter.  No atomics: the plan leaves every destination at most once.
//   the fill    the appended cells of a column the batch does not provide = the column's null.
#include "rfx_cells.hpp"

#define UP_STEPS 8
#define UP_TILE (RFX_BLOCK * UP_STEPS) /* batch rows per workgroup: 2048 */

// a matched row?  (the null, a negative and a row past the table are "none": the unsigned compare takes all three)
__device__ __forceinline__ bool up_hit(i64 r, i64 n) { return (u64)r < (u64)n; }

__global__ __launch_bounds__(RFX_BLOCK) void k_up_clear(const i64 *__restrict__ idx, i64 m, i64 n, int *__restrict__ W) {
    const i64 nt = (i64)gridDim.x * RFX_BLOCK;
    for (i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; j < m; j += nt) {
        const i64 r = idx[j];
        if (up_hit(r, n)) W[r] = -1;
    }
}

// workgroup b owns batch rows [b * UP_TILE, (b + 1) * UP_TILE): the winners' max, and blk[b] = its unmatched rows
__global__ __launch_bounds__(RFX_BLOCK) void k_up_max(const i64 *__restrict__ idx, i64 m, i64 n, int *__restrict__ W, i64 *__restrict__ blk) {
    __shared__ int wsum[RFX_BLOCK / RFX_WAVE];
    const i64 base = (i64)blockIdx.x * UP_TILE;
    int cnt = 0; // (wave-uniform)
#pragma unroll
    for (int s = 0; s < UP_STEPS; s++) {
        const i64 j = base + (i64)s * RFX_BLOCK + threadIdx.x;
        bool miss = false;
        if (j < m) {
            const i64 r = idx[j];
            if (up_hit(r, n)) atomicMax(&W[r], (int)j);
            else miss = true;
        }
        cnt += __popcll(__ballot(miss));
    }
    if ((threadIdx.x & (RFX_WAVE - 1)) == 0) wsum[threadIdx.x / RFX_WAVE] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 t = 0;
        for (int w = 0; w < RFX_BLOCK / RFX_WAVE; w++) t += wsum[w];
        blk[blockIdx.x] = t;
    }
}

// ONE workgroup: blk[0 .. nblk) becomes its exclusive prefix, blk[nblk] the total
__global__ __launch_bounds__(RFX_BLOCK) void k_up_scan(i64 *__restrict__ blk, i64 nblk) {
    __shared__ i64 part[RFX_BLOCK];
    const i64 per = (nblk + RFX_BLOCK - 1) / RFX_BLOCK;
    const i64 b0 = (i64)threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    i64 t = 0;
    for (i64 b = b0; b < b1; b++) t += blk[b];
    part[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 run = 0;
        for (int i = 0; i < RFX_BLOCK; i++) {
            const i64 v = part[i];
            part[i] = run;
            run += v;
        }
        blk[nblk] = run;
    }
    __syncthreads();
    i64 run = part[threadIdx.x];
    for (i64 b = b0; b < b1; b++) {
        const i64 v = blk[b];
        blk[b] = run;
        run += v;
    }
}

// the ordered scan: wave w of workgroup b owns rows b * UP_TILE + w * 512 + s * 64 + lane, s = 0 .. 7 -- ballots in row order
__global__ __launch_bounds__(RFX_BLOCK) void k_up_dest(const i64 *__restrict__ idx, i64 m, i64 n, const int *__restrict__ W, const i64 *__restrict__ blk,
                                                       i64 *__restrict__ dest) {
    __shared__ int wsum[RFX_BLOCK / RFX_WAVE];
    const int lane = threadIdx.x & (RFX_WAVE - 1), wave = threadIdx.x / RFX_WAVE;
    const i64 base = (i64)blockIdx.x * UP_TILE + (i64)wave * (RFX_WAVE * UP_STEPS) + lane;
    i64 r[UP_STEPS];
    u64 miss[UP_STEPS]; // (wave-uniform ballots)
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < UP_STEPS; s++) {
        const i64 j = base + (i64)s * RFX_WAVE;
        r[s] = j < m ? idx[j] : 0;
        miss[s] = __ballot(j < m && !up_hit(r[s], n));
        cnt += __popcll(miss[s]);
    }
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    i64 run = blk[blockIdx.x];
    for (int w = 0; w < wave; w++) run += wsum[w];
    const u64 below = lane ? (~0ULL >> (RFX_WAVE - lane)) : 0ULL;
#pragma unroll
    for (int s = 0; s < UP_STEPS; s++) {
        const i64 j = base + (i64)s * RFX_WAVE;
        if (j < m) {
            i64 d;
            if (up_hit(r[s], n)) d = W[r[s]] == (int)j ? r[s] : -1;
            else d = n + run + __popcll(miss[s] & below);
            dest[j] = d;
        }
        run += __popcll(miss[s]);
    }
}

struct up_cols {
    const unsigned char *batch[RFX_MAX_COLS];
    unsigned char *out[RFX_MAX_COLS];
    int width[RFX_MAX_COLS];
    int appends_only[RFX_MAX_COLS];
    int ncols;
};

// one column over the workgroup's tile: access g covers rows base + g * R .. + R - 1, R = 16 / WID cells of one 16-byte load
template <int WID>
__device__ __forceinline__ void up_place_col(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, bool ao, const i64 *dl, i64 base, i64 m, i64 n,
                                             i64 total) {
    constexpr int R = 16 / WID, NACC = UP_TILE / R; // accesses per tile: 1024, 512, 256, 128
    for (int g = threadIdx.x; g < NACC; g += RFX_BLOCK) {
        const i64 j0 = base + (i64)g * R;
        if (j0 >= m) break;
        if (j0 + R <= m) {
            const rfx_v2q v = __builtin_nontemporal_load((const rfx_v2q *)(in + j0 * WID));
#pragma unroll
            for (int i = 0; i < R; i++) {
                const i64 d = dl[g * R + i];
                const u64 word = (i * WID) / 8 ? v.y : v.x;
                const u64 cell = WID == 8 ? word : (word >> (((i * WID) & 7) * 8));
                if (d >= (ao ? n : 0) && d < total) rfx_cell_put<WID>(out, d, cell);
            }
        } else { // the batch's last cells: one by one, nothing read past cell m - 1
            for (int i = 0; i < R && j0 + i < m; i++) {
                const i64 d = dl[g * R + i];
                if (d >= (ao ? n : 0) && d < total) rfx_cell_put<WID>(out, d, rfx_cell_get<WID>(in, j0 + i));
            }
        }
    }
}
__global__ __launch_bounds__(RFX_BLOCK) void k_up_place(const up_cols C, const i64 *__restrict__ dest, i64 m, i64 n, i64 total) {
    __shared__ __attribute__((aligned(16))) i64 dl[UP_TILE];
    const i64 base = (i64)blockIdx.x * UP_TILE;
    for (int g = threadIdx.x; g < UP_TILE / 2; g += RFX_BLOCK) { // dest: two cells per 16-byte load (dest is 16-byte aligned, base even)
        const i64 j0 = base + (i64)g * 2;
        i64 d0 = -1, d1 = -1;
        if (!dest) { // insert: every row is appended, in order
            d0 = j0 < m ? n + j0 : -1;
            d1 = j0 + 1 < m ? n + j0 + 1 : -1;
        } else if (j0 + 2 <= m) {
            const rfx_v2q v = __builtin_nontemporal_load((const rfx_v2q *)(dest + j0));
            d0 = (i64)v.x;
            d1 = (i64)v.y;
        } else if (j0 < m) d0 = dest[j0];
        dl[g * 2] = d0;
        dl[g * 2 + 1] = d1;
    }
    __syncthreads();
    for (int k = 0; k < C.ncols; k++) {
        const bool ao = C.appends_only[k] != 0;
        switch (C.width[k]) {
            case 8: up_place_col<8>(C.batch[k], C.out[k], ao, dl, base, m, n, total); break;
            case 4: up_place_col<4>(C.batch[k], C.out[k], ao, dl, base, m, n, total); break;
            case 2: up_place_col<2>(C.batch[k], C.out[k], ao, dl, base, m, n, total); break;
            default: up_place_col<1>(C.batch[k], C.out[k], ao, dl, base, m, n, total); break;
        }
    }
}

// `pattern` repeats the cell through 8 bytes; head (to the first 16-byte boundary) and nbytes are multiples of the cell, so the phase holds
__global__ __launch_bounds__(RFX_BLOCK) void k_up_fill(u64 pattern, unsigned char *__restrict__ dst, i64 head, i64 n16, i64 nbytes) {
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK;
    rfx_v2q o;
    o.x = pattern; o.y = pattern;
    for (i64 g = tid; g < n16; g += nt) __builtin_nontemporal_store(o, (rfx_v2q *)(dst + head) + g);
    for (i64 b = tid; b < head; b += nt) dst[b] = (unsigned char)(pattern >> (8 * (b & 7)));
    for (i64 b = head + n16 * 16 + tid; b < nbytes; b += nt) dst[b] = (unsigned char)(pattern >> (8 * ((b - head) & 7)));
}

extern "C" int rfx_hip_upsert_plan(rfx_ctx_t *c, const int64_t *d_idx, int64_t m, int64_t n, int64_t *d_dest, int64_t *appended) {
    RFX_REQUIRE(c && appended, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(m >= 0 && n >= 0, RFX_EINVAL, "negative length");
    *appended = 0;
    if (m == 0) return RFX_OK;
    RFX_REQUIRE(d_idx && d_dest, RFX_EINVAL, "NULL index or destination");
    RFX_REQUIRE(m < 0x80000000LL, RFX_ELIMIT, "2^31 or more batch rows");
    RFX_REQUIRE(n < (1LL << 61), RFX_ELIMIT, "table rows");
    const i64 nblk = (m + UP_TILE - 1) / UP_TILE; // < 2^20
    void *d_w = NULL, *d_blk = NULL;
    int rc = rfx_hip_malloc(c, &d_blk, (size_t)(nblk + 1) * 8);
    if (rc == RFX_OK && n > 0) rc = rfx_hip_malloc(c, &d_w, (size_t)n * 4);
    if (rc != RFX_OK) {
        if (d_blk) rfx_hip_free(c, d_blk);
        return rc;
    }
    RFX_KERNEL_BEGIN(c);
    if (n > 0) hipLaunchKernelGGL(k_up_clear, dim3(rfx_stream_grid(c, m)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_idx, (i64)m, (i64)n, (int *)d_w);
    hipLaunchKernelGGL(k_up_max, dim3((unsigned)nblk), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_idx, (i64)m, (i64)n, (int *)d_w, (i64 *)d_blk);
    hipLaunchKernelGGL(k_up_scan, dim3(1), dim3(RFX_BLOCK), 0, c->stream, (i64 *)d_blk, nblk);
    hipLaunchKernelGGL(k_up_dest, dim3((unsigned)nblk), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_idx, (i64)m, (i64)n, (const int *)d_w, (const i64 *)d_blk,
                       (i64 *)d_dest);
    RFX_KERNEL_END(c);
    hipError_t e = hipGetLastError();
    i64 a = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&a, (const i64 *)d_blk + nblk, 8, hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream); // (the scratch goes back idle, whatever happened)
    if (e == hipSuccess) e = es;
    if (d_w) rfx_hip_free(c, d_w);
    rfx_hip_free(c, d_blk);
    RFX_HIP_CHECK(e);
    RFX_REQUIRE(a >= 0 && a <= m, RFX_EHIP, "an append count outside 0 .. m");
    *appended = a;
    return RFX_OK;
}

extern "C" int rfx_hip_upsert_place(rfx_ctx_t *c, const rfx_upsert_col_t *cols, int ncols, const int64_t *d_dest, int64_t m, int64_t n, int64_t total) {
    RFX_REQUIRE(c && cols, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(ncols >= 1 && ncols <= RFX_MAX_COLS, RFX_EINVAL, "1 .. RFX_MAX_COLS columns per launch");
    RFX_REQUIRE(m >= 0 && n >= 0 && total >= n && total - n <= m, RFX_EINVAL, "lengths that do not fit: total is n + at most m appended rows");
    if (m == 0) return RFX_OK;
    RFX_REQUIRE(m < 0x80000000LL, RFX_ELIMIT, "2^31 or more batch rows");
    RFX_REQUIRE(((uintptr_t)d_dest & 15) == 0, RFX_EINVAL, "destinations that are not 16-byte aligned");
    RFX_REQUIRE(d_dest || total - n == m, RFX_EINVAL, "no destinations, yet not every row appended");
    up_cols C;
    memset(&C, 0, sizeof(C));
    for (int k = 0; k < ncols; k++) {
        RFX_REQUIRE(rfx_width_ok(cols[k].width), RFX_EINVAL, "a cell width that is not 1, 2, 4 or 8 bytes");
        RFX_REQUIRE(cols[k].d_batch && ((uintptr_t)cols[k].d_batch & 15) == 0, RFX_EINVAL, "NULL batch cells, or ones that are not 16-byte aligned");
        RFX_REQUIRE(cols[k].d_out && ((uintptr_t)cols[k].d_out & (uintptr_t)(cols[k].width - 1)) == 0, RFX_EINVAL, "NULL result, or one that is not cell-aligned");
        C.batch[k] = (const unsigned char *)cols[k].d_batch;
        C.out[k] = (unsigned char *)cols[k].d_out;
        C.width[k] = cols[k].width;
        C.appends_only[k] = cols[k].appends_only != 0;
    }
    C.ncols = ncols;
    rfx_ctx_device_written(c);
    const i64 nblk = (m + UP_TILE - 1) / UP_TILE;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_up_place, dim3((unsigned)nblk), dim3(RFX_BLOCK), 0, c->stream, C, (const i64 *)d_dest, (i64)m, (i64)n, (i64)total);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_upsert_fill(rfx_ctx_t *c, void *d_dst, int32_t width, uint64_t bits, int64_t cells) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(rfx_width_ok(width), RFX_EINVAL, "a cell width that is not 1, 2, 4 or 8 bytes");
    RFX_REQUIRE(cells >= 0 && cells <= (INT64_MAX >> 5), RFX_EINVAL, "cell count");
    if (cells == 0) return RFX_OK;
    RFX_REQUIRE(d_dst && ((uintptr_t)d_dst & (uintptr_t)(width - 1)) == 0, RFX_EINVAL, "NULL destination, or one that is not cell-aligned");
    const u64 pattern = width == 8 ? bits : (width == 4 ? (bits & 0xFFFFFFFFULL) * 0x100000001ULL
                                                        : (width == 2 ? (bits & 0xFFFFULL) * 0x0001000100010001ULL : (bits & 0xFFULL) * 0x0101010101010101ULL));
    const i64 nbytes = cells * width;
    i64 head = (i64)((16 - ((uintptr_t)d_dst & 15)) & 15);
    if (head > nbytes) head = nbytes;
    const i64 n16 = (nbytes - head) / 16;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_up_fill, dim3(rfx_stream_grid(c, n16 + 32)), dim3(RFX_BLOCK), 0, c->stream, pattern, (unsigned char *)d_dst, head, n16, nbytes);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
