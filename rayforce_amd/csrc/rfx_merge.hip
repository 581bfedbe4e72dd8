// rfx_merge.hip -- stable multiway merge of k <= RFX_MERGE_MAX_RUNS sorted runs: the second half of a sort over row-range shards (every shard's piece
// sorted by rfx_sort.hip, the runs merged here).  gfx950 / wave64.
//
// Order: (sort-key tuple, run, place in run).  The tuple is sort_key() of rfx_sort_key.hpp -- the radix sort's own function -- over the raw cells of
// 1 .. RFX_MAX_KEYS key columns that lie in each run's sorted order; nothing is decoded and no key is ever moved: the kernels write rows and / or cells only.
//
// Launches (no workgroup ever waits on another inside a launch):
//   k_merge_splitters  every T-th record of every run (places T, 2T, .. < len) is a splitter.  16 lanes per splitter, lane b searches run b: the number of
//                      run b's records that come before the splitter -- an UPPER bound for b before the splitter's own run, a LOWER bound for b after
//                      it (equal keys: earlier runs first -- the stability), its own place for its own run.  The 16 co-ranks are stored and their sum
//                      (a shuffle reduction) is the splitter's global place.
//   rfx_hip_sort_index over the places (distinct by construction): the splitters in global order
//   k_merge_segments   one workgroup per gap between consecutive splitters: run b contributes its records [lo_b, hi_b) -- the two splitters' co-ranks,
//                      at most T records each -- and the gap starts at output place sum(lo_b): exact, no scan, no look-back.  A record's place inside
//                      the gap = its index in its own slice + its co-ranks in the other slices (k - 1 searches of <= log2 T + 1 steps over cache-hot
//                      cells), computed once.  A gap of at most MERGE_WINDOW records stages its cells in LDS and writes them out contiguously; a wider one
//                      (the mean gap is T records whatever the data, but gap sizes spread: at T = 2048 about every third record lies in one) writes
//                      them straight to their places inside the gap's own range.  The worst case -- every gap holding a tile of every run, k * T
//                      records -- is what tools/bench_sort.py's "interleaved runs" case measures.
//   k_merge_copy       instead of all of the above when exactly one run holds records: a copy with row0 added.
// Every search runs inside [0, len_b) resp. [lo_b, hi_b) with 0 <= lo_b <= hi_b <= len_b enforced, a record's place inside its gap is below the gap's size by
// construction and every store is checked against n: unsorted input gives a wrong answer, never an access outside a run or an output.
#include "rfx_common.hpp"
#include "rfx_sort_key.hpp"

#define MERGE_TILE 1024   /* the shipped T */
#define MERGE_TILE_MIN 512
#define MERGE_TILE_MAX 2048
#define MERGE_WINDOW 2048 /* cells staged per output and write-out step: 16 KB of LDS per output */
#define MERGE_THREADS 256
#define MERGE_K RFX_MERGE_MAX_RUNS

struct MergeRun {
    const u64 *keys[RFX_MAX_KEYS];
    const i64 *rows;
    i64 len, row0;
    i64 sp0; // index of the run's first splitter among all splitters
};
struct MergeArgs { // one copy in device memory per call: indexed by run inside the kernels
    MergeRun run[MERGE_K];
    i64 n, nsplit;
    int k, nk, desc, tile;
    int f64[RFX_MAX_KEYS];
};

// the sort-key tuple of record p of a run
__device__ __forceinline__ void merge_load(const MergeArgs *__restrict__ A, const MergeRun *__restrict__ R, i64 p, u64 (&ka)[RFX_MAX_KEYS]) {
#pragma unroll
    for (int c = 0; c < RFX_MAX_KEYS; c++) ka[c] = c < A->nk ? sort_key(R->keys[c][p], A->f64[c], A->desc) : 0ULL;
}
// how many records of run b's [lo, hi) come before the record with tuple ka: those below it, and (with_equal) those equal to it as well
__device__ __forceinline__ i64 merge_corank(const MergeArgs *__restrict__ A, const MergeRun *__restrict__ B, i64 lo, i64 hi, const u64 (&ka)[RFX_MAX_KEYS], bool with_equal) {
    const u64 *__restrict__ lead = B->keys[0]; // (one dependent load per step, not two)
    const int nk = A->nk, desc = A->desc, f0 = A->f64[0];
    while (lo < hi) {
        const i64 m = lo + ((hi - lo) >> 1);
        bool less = false, eq = true; // of B[m] against ka
#pragma unroll
        for (int c = 0; c < RFX_MAX_KEYS; c++) {
            if (c < nk && eq) {
                const u64 kb = c == 0 ? sort_key(lead[m], f0, desc) : sort_key(B->keys[c][m], A->f64[c], desc);
                if (kb != ka[c]) {
                    less = kb < ka[c];
                    eq = false;
                }
            }
        }
        if (less || (eq && with_equal)) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(MERGE_THREADS) void k_merge_splitters(const MergeArgs *__restrict__ A, i64 *__restrict__ corank, i64 *__restrict__ place) {
    const int k = A->k, b = threadIdx.x & 15;
    const i64 T = A->tile;
    for (i64 s = (blockIdx.x * (i64)MERGE_THREADS + threadIdx.x) >> 4; s < A->nsplit; s += ((i64)gridDim.x * MERGE_THREADS) >> 4) {
        int a = 0; // the splitter's run: the last one whose first splitter is at or before s
        for (int r = 1; r < k; r++)
            if (A->run[r].sp0 <= s) a = r;
        const i64 p = (s - A->run[a].sp0 + 1) * T;
        i64 cr = 0;
        if (b < k && p < A->run[a].len) { // (p < len by the host's count of splitters; never a read outside the run)
            if (b == a) cr = p;
            else if (A->run[b].len > 0) {
                u64 ka[RFX_MAX_KEYS];
                merge_load(A, &A->run[a], p, ka);
                cr = merge_corank(A, &A->run[b], 0, A->run[b].len, ka, b < a);
            }
        }
        if (b < k) corank[s * k + b] = cr;
        i64 sum = cr;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) sum += (i64)rfx_shfl_xor_u64((u64)sum, o);
        if (b == 0) place[s] = sum;
    }
}

__global__ __launch_bounds__(MERGE_THREADS) void k_merge_segments(const MergeArgs *__restrict__ A, const i64 *__restrict__ corank, const i64 *__restrict__ order,
                                                                  i64 *__restrict__ perm_out, u64 *__restrict__ vals_out) {
    extern __shared__ __attribute__((aligned(16))) u64 stage[]; // [MERGE_WINDOW] rows, then [MERGE_WINDOW] cells -- each only when wanted
    __shared__ i64 s_lo[MERGE_K];
    __shared__ int s_off[MERGE_K + 1];
    __shared__ i64 s_base;
    const int k = A->k, t = threadIdx.x;
    const i64 seg = blockIdx.x, ns = A->nsplit;
    if (t < k) {
        const i64 len = A->run[t].len;
        i64 lo = 0, hi = len;
        if (seg > 0) {
            const i64 sid = order[seg - 1];
            lo = ((u64)sid < (u64)ns) ? corank[sid * k + t] : 0;
        }
        if (seg < ns) {
            const i64 sid = order[seg];
            hi = ((u64)sid < (u64)ns) ? corank[sid * k + t] : len;
        }
        lo = lo < 0 ? 0 : (lo > len ? len : lo);
        hi = hi < lo ? lo : (hi > len ? len : hi);
        if (hi - lo > A->tile) hi = lo + A->tile; // (sorted runs never get here: no splitter of run t lies inside the gap)
        s_lo[t] = lo;
        s_off[t + 1] = (int)(hi - lo);
    }
    __syncthreads();
    if (t == 0) {
        i64 base = 0;
        int off = 0;
        s_off[0] = 0;
        for (int b = 0; b < k; b++) {
            base += s_lo[b];
            off += s_off[b + 1];
            s_off[b + 1] = off;
        }
        s_base = base;
    }
    __syncthreads();
    const int S = s_off[k];
    const i64 base = s_base, n = A->n;
    u64 *st_rows = stage, *st_vals = stage + (perm_out ? MERGE_WINDOW : 0);
    const bool direct = S > MERGE_WINDOW; // a gap beyond the staging window writes its cells where they go: every place is computed ONCE either way
    for (int e = t; e < S; e += MERGE_THREADS) {
        int a = 0;
        for (int r = 1; r < k; r++)
            if (s_off[r] <= e) a = r;
        const int own = e - s_off[a];
        const MergeRun *Ra = &A->run[a];
        const i64 p = s_lo[a] + own;
        u64 ka[RFX_MAX_KEYS];
        merge_load(A, Ra, p, ka);
        int at = own;
        for (int b = 0; b < k; b++) {
            const int cnt = s_off[b + 1] - s_off[b];
            if (b == a || cnt == 0) continue;
            const i64 lo = s_lo[b];
            at += (int)(merge_corank(A, &A->run[b], lo, lo + cnt, ka, b < a) - lo);
        }
        // (0 <= at < S: own < its slice's size, every co-rank at most its slice's size)
        if (direct) {
            const i64 o = base + at;
            if (at >= 0 && at < S && o < n) { // (never a write beyond the outputs)
                if (perm_out) perm_out[o] = Ra->row0 + Ra->rows[p];
                if (vals_out) vals_out[o] = Ra->keys[0][p];
            }
        } else if (at >= 0 && at < MERGE_WINDOW) {
            if (perm_out) st_rows[at] = (u64)(Ra->row0 + Ra->rows[p]);
            if (vals_out) st_vals[at] = Ra->keys[0][p];
        }
    }
    if (direct) return; // (uniform over the workgroup)
    __syncthreads();
    for (int j = t; j < S; j += MERGE_THREADS) {
        const i64 o = base + j;
        if (o >= n) break; // (never a write beyond the outputs)
        if (perm_out) perm_out[o] = (i64)st_rows[j];
        if (vals_out) vals_out[o] = st_vals[j];
    }
}

// exactly one run holds records: its order is the answer -- a copy with row0 added, no splitters, no searches
__global__ __launch_bounds__(RFX_BLOCK) void k_merge_copy(const u64 *__restrict__ cells, const i64 *__restrict__ rows, i64 row0, i64 n, i64 *__restrict__ perm_out,
                                                          u64 *__restrict__ vals_out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        if (perm_out) perm_out[i] = row0 + rows[i];
        if (vals_out) vals_out[i] = cells[i];
    }
}

extern "C" int rfx_hip_merge_tile(void) { return MERGE_TILE; }

extern "C" int rfx_hip_merge_runs(rfx_ctx_t *ctx, const rfx_merge_run_t *runs, int nruns, const int32_t *types, int nkeys, int descending, int tile,
                                  int64_t *d_perm_out, void *d_values_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && runs && types, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(nruns >= 1 && nruns <= MERGE_K, RFX_EINVAL, "1 .. RFX_MERGE_MAX_RUNS runs");
    RFX_REQUIRE(nkeys >= 1 && nkeys <= RFX_MAX_KEYS, RFX_EINVAL, "1 .. RFX_MAX_KEYS key columns");
    RFX_REQUIRE(tile == 0 || (tile >= MERGE_TILE_MIN && tile <= MERGE_TILE_MAX), RFX_EINVAL, "tile: 0 or 512 .. 2048");
    RFX_REQUIRE(!d_values_out || nkeys == 1, RFX_EINVAL, "merged cells are those of ONE key column");
    MergeArgs H;
    memset(&H, 0, sizeof(H));
    H.k = nruns;
    H.nk = nkeys;
    H.desc = descending != 0;
    H.tile = tile ? tile : MERGE_TILE;
    for (int j = 0; j < nkeys; j++) {
        RFX_REQUIRE(types[j] == RFX_I64 || types[j] == RFX_F64, RFX_EINVAL, "key type must be i64 (timestamp) or f64");
        H.f64[j] = types[j] == RFX_F64;
    }
    for (int r = 0; r < nruns; r++) {
        RFX_REQUIRE(runs[r].len >= 0, RFX_EINVAL, "negative run length");
        H.run[r].len = runs[r].len;
        H.run[r].row0 = runs[r].row0;
        H.run[r].rows = (const i64 *)runs[r].d_rows;
        H.run[r].sp0 = H.nsplit;
        for (int j = 0; j < nkeys; j++) {
            RFX_REQUIRE(runs[r].len == 0 || runs[r].d_keys[j], RFX_EINVAL, "NULL key column");
            H.run[r].keys[j] = (const u64 *)runs[r].d_keys[j];
        }
        RFX_REQUIRE(runs[r].len == 0 || !d_perm_out || runs[r].d_rows, RFX_EINVAL, "NULL rows of a run");
        if (runs[r].len > 0) H.nsplit += (runs[r].len - 1) / H.tile;
        H.n += runs[r].len;
    }
    if (H.n == 0) return RFX_OK;
    RFX_REQUIRE(d_perm_out || d_values_out, RFX_EINVAL, "NULL outputs");
    int nonempty = 0, only = 0;
    for (int r = 0; r < nruns; r++)
        if (runs[r].len > 0) nonempty++, only = r;
    if (nonempty == 1) {
        const i64 want = (H.n + RFX_BLOCK - 1) / RFX_BLOCK, cap = (i64)rfx_grid(c) * 4;
        RFX_KERNEL_BEGIN(c);
        hipLaunchKernelGGL(k_merge_copy, dim3((unsigned)(want < cap ? want : cap)), dim3(RFX_BLOCK), 0, c->stream, H.run[only].keys[0], H.run[only].rows, H.run[only].row0,
                           H.n, (i64 *)d_perm_out, (u64 *)d_values_out);
        RFX_KERNEL_END(c);
        RFX_HIP_CHECK(hipGetLastError());
        RFX_HIP_CHECK(hipStreamSynchronize(c->stream)); // (as the merge: returns with the outputs written)
        return RFX_OK;
    }
    RFX_REQUIRE(H.nsplit < (1LL << 24) - 1, RFX_ELIMIT, "2^24 gaps or more (one workgroup per gap, 2^32 threads per launch)");
    const i64 ns = H.nsplit;
    // scratch: the arguments | co-ranks [ns][k] | places [ns] | the splitters in place order [ns]
    const size_t ab = (sizeof(MergeArgs) + 255) & ~(size_t)255, cb = (((size_t)ns * nruns * 8) + 255) & ~(size_t)255, pb = (((size_t)ns * 8) + 255) & ~(size_t)255;
    void *scratch = NULL;
    int rc = rfx_hip_malloc(ctx, &scratch, ab + cb + 2 * pb);
    if (rc != RFX_OK) return rc;
    char *sp = (char *)scratch;
    const MergeArgs *dA = (const MergeArgs *)sp;
    i64 *corank = (i64 *)(sp + ab), *place = (i64 *)(sp + ab + cb), *order = (i64 *)(sp + ab + cb + pb);
    hipError_t e = hipMemcpyAsync(sp, &H, sizeof(H), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (H leaves with this frame)
    if (e == hipSuccess && ns > 0) {
        const i64 want = (ns * 16 + MERGE_THREADS - 1) / MERGE_THREADS, cap = (i64)rfx_grid(c) * 8;
        RFX_KERNEL_BEGIN(c);
        hipLaunchKernelGGL(k_merge_splitters, dim3((unsigned)(want < cap ? want : cap)), dim3(MERGE_THREADS), 0, c->stream, dA, corank, place);
        e = hipGetLastError();
        RFX_KERNEL_END(c);
        if (e == hipSuccess) {
            rc = rfx_hip_sort_index(ctx, place, RFX_I64, ns, 0, NULL, (int64_t *)order, NULL);
            if (rc != RFX_OK) {
                (void)hipStreamSynchronize(c->stream);
                rfx_hip_free(ctx, scratch);
                return rc;
            }
        }
    }
    RFX_KERNEL_BEGIN(c);
    if (e == hipSuccess) {
        const size_t lds = (size_t)MERGE_WINDOW * 8 * ((d_perm_out ? 1 : 0) + (d_values_out ? 1 : 0));
        hipLaunchKernelGGL(k_merge_segments, dim3((unsigned)(ns + 1)), dim3(MERGE_THREADS), lds, c->stream, dA, (const i64 *)corank, (const i64 *)order,
                           (i64 *)d_perm_out, (u64 *)d_values_out);
        e = hipGetLastError();
    }
    RFX_KERNEL_END(c);
    const hipError_t es = hipStreamSynchronize(c->stream); // (the scratch goes back to the context's pool: nothing may still read it)
    rfx_hip_free(ctx, scratch);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        rfx_set_error("rfx_merge: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RFX_ENOMEM : RFX_EHIP;
    }
    return RFX_OK;
}
