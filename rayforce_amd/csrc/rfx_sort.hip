// rfx_sort.hip -- stable LSD radix sort of (key, row) pairs: the permutation behind iasc / idesc / rank / xasc / xdesc and the sorted
// cells behind asc / desc.  gfx950 / wave64.
//
// Sort key: sort_key() of rfx_sort_key.hpp, shared with the merge of sorted runs (rfx_merge.hip).
//
// Launches (no workgroup ever waits on another inside a launch):
//   k_sort_keys     the column read once (through perm_in when given) -> the keys, and all eight 8-bit digit histograms (LDS counters per
//                   workgroup, merged with integer atomics).  The host reads the 16 KB of histograms back: a digit with one occupied bin moves
//                   nothing and its pass is skipped.
//   per executed digit:
//   k_sort_count    per tile of SORT_TILE (8192) rows the 256 digit counts -> counts[digit][tile]
//   k_sort_scan     one workgroup per digit: counts[digit][*] -> exclusive offsets, starting at the digit's base (from the global histogram)
//   k_sort_scatter  every row's place = its tile's offset for its digit + its stable rank inside the tile: waves take consecutive runs of the
//                   tile, a wave takes 64 consecutive rows per step; equal digits of one step are found with 8 ballots (rank = lower lanes of
//                   the match), steps and waves accumulate in per-wave LDS counters -- wave order = step order = row order.
// Records are a u64 key and a u32 row (rows < 2^32), in two ping-pong pairs; the first pass reads rows as 0..n-1 and the last one writes the
// caller's outputs: the i64 permutation (looked up in perm_in when given) and / or the sorted cells decoded from the keys (a NaN takes its
// own bits from the column through its row).
#include "rfx_common.hpp"
#include "rfx_sort_key.hpp"

#define SORT_THREADS 1024
#define SORT_WAVES (SORT_THREADS / RFX_WAVE)
#define SORT_ITEMS 8
#define SORT_TILE (SORT_THREADS * SORT_ITEMS) /* 8192 rows: 1 KB of counts per 96 KB of records (16 rows per thread spill registers) */
#define SORT_SMALL_ITEMS 2
#define SORT_SMALL_TILE (SORT_THREADS * SORT_SMALL_ITEMS)
#define SORT_SMALL_ROWS ((i64)1 << 23) /* below: the small tile, so that a few million rows still fill the device */
#define SORT_MAX_ROWS ((i64)0xFFFFFFFFLL)

// ---- keys + the eight digit histograms ----
__global__ __launch_bounds__(RFX_BLOCK) void k_sort_keys(const u64 *__restrict__ col, const i64 *__restrict__ perm_in, i64 n, int f64, int desc,
                                                         u64 *__restrict__ keys, unsigned long long *__restrict__ hist) {
    __shared__ unsigned int lh[8 * 256];
    for (int i = threadIdx.x; i < 8 * 256; i += RFX_BLOCK) lh[i] = 0;
    __syncthreads();
    // (a workgroup's share of at most 2^32 rows fits the 32-bit LDS counters)
    const int lane = threadIdx.x & 63;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        u64 x;
        if (perm_in) {
            const i64 r = perm_in[i];
            x = ((u64)r < (u64)n) ? col[r] : (f64 ? RFX_NAN_BITS : (u64)RFX_NULL_I64_D); // (never a read beyond the column)
        } else x = col[i];
        const u64 k = sort_key(x, f64, desc);
        keys[i] = k;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            // a digit the whole wave agrees on (the constant high bytes of narrow keys) is one add, not 64 colliding ones
            const int dg = (int)((k >> (8 * d)) & 255), first = __builtin_amdgcn_readfirstlane(dg);
            const u64 active = __ballot(1);
            if (__ballot(dg == first) == active) {
                if (lane == __ffsll((long long)active) - 1) atomicAdd(&lh[d * 256 + first], (unsigned int)__popcll(active));
            } else atomicAdd(&lh[d * 256 + dg], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256; i += RFX_BLOCK)
        if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

// ---- per-tile digit counts ----
template <int ITEMS>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_count(const u64 *__restrict__ keys, i64 n, int shift, i64 tiles, unsigned int *__restrict__ counts) {
    __shared__ unsigned int lh[256];
    const i64 tile = blockIdx.x;
    if (threadIdx.x < 256) lh[threadIdx.x] = 0;
    __syncthreads();
    const i64 base = tile * (i64)(SORT_THREADS * ITEMS);
#pragma unroll
    for (int s = 0; s < ITEMS; s++) {
        const i64 i = base + (i64)s * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&lh[(int)((keys[i] >> shift) & 255)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256) counts[(i64)threadIdx.x * tiles + tile] = lh[threadIdx.x];
}

// ---- counts[digit][0..tiles) -> exclusive offsets from the digit's base; one workgroup per digit ----
__global__ __launch_bounds__(RFX_BLOCK) void k_sort_scan(unsigned int *__restrict__ counts, i64 tiles, const unsigned long long *__restrict__ hist) {
    __shared__ unsigned long long red[RFX_BLOCK];
    __shared__ unsigned int wsum[RFX_BLOCK / RFX_WAVE];
    const int d = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    red[t] = (t < d) ? hist[t] : 0ULL; // rows whose digit is smaller: where this digit's run starts
    __syncthreads();
    for (int s = RFX_BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    unsigned int carry = (unsigned int)red[0];
    unsigned int *row = counts + (i64)d * tiles;
    for (i64 c0 = 0; c0 < tiles; c0 += RFX_BLOCK) {
        const i64 i = c0 + t;
        const unsigned int v = (i < tiles) ? row[i] : 0u;
        unsigned int x = v; // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        unsigned int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < RFX_BLOCK / RFX_WAVE; k++) {
            const unsigned int s = wsum[k];
            if (k < w) before += s;
            total += s;
        }
        if (i < tiles) row[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
}

struct SortPass {
    const u64 *keys_in;
    const unsigned int *rows_in; // NULL: row i is i (the first executed pass)
    u64 *keys_out;               // ping-pong outputs (NULL in the last pass)
    unsigned int *rows_out;
    i64 *perm_out;               // last pass: the i64 permutation (NULL: not wanted) ...
    const i64 *perm_in;          // ... read through the caller's incoming permutation when given
    u64 *vals_out;               // last pass: the sorted cells (NULL: not wanted)
    const u64 *col;              // the column (a NaN's own bits)
    const unsigned int *offsets; // [256][tiles]
    i64 n, tiles;
    int shift, f64, desc, _pad;
};

template <int ITEMS>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const SortPass P) {
    __shared__ unsigned int cnt[SORT_WAVES][256]; // phase 1: the wave's running digit counts; phase 2: where the wave's first row of a digit goes
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const i64 tile = blockIdx.x;
    for (int i = t; i < SORT_WAVES * 256; i += SORT_THREADS) (&cnt[0][0])[i] = 0;
    __syncthreads();
    volatile unsigned int *mine = cnt[w];
    const i64 base = tile * (i64)(SORT_THREADS * ITEMS) + (i64)w * (64 * ITEMS);
    const u64 lt = (1ULL << lane) - 1ULL;
    u64 key[ITEMS];
    unsigned int rank[ITEMS];
#pragma unroll
    for (int s = 0; s < ITEMS; s++) {
        const i64 i = base + (i64)s * 64 + lane;
        const bool valid = i < P.n;
        key[s] = valid ? P.keys_in[i] : 0ULL;
        const int d = (int)((key[s] >> P.shift) & 255);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1;
            const u64 m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        unsigned int before = 0;
        if (valid) before = mine[d];
        __builtin_amdgcn_wave_barrier();
        if (valid && (peers & lt) == 0ULL) mine[d] = before + (unsigned int)__popcll(peers); // (the lowest lane of each match)
        __builtin_amdgcn_wave_barrier();
        rank[s] = before + (unsigned int)__popcll(peers & lt);
    }
    __syncthreads();
    if (t < 256) { // digit t: the tile's offset, then wave after wave
        unsigned int at = P.offsets[(i64)t * P.tiles + tile];
#pragma unroll
        for (int k = 0; k < SORT_WAVES; k++) {
            const unsigned int c = cnt[k][t];
            cnt[k][t] = at;
            at += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < ITEMS; s++) {
        const i64 i = base + (i64)s * 64 + lane;
        if (i >= P.n) continue;
        const u64 k = key[s];
        const i64 pos = (i64)(cnt[w][(int)((k >> P.shift) & 255)] + rank[s]);
        if (pos >= P.n) continue; // (cannot happen with consistent counts; never a write beyond the buffers)
        const unsigned int r = P.rows_in ? P.rows_in[i] : (unsigned int)i;
        if (P.keys_out) {
            P.keys_out[pos] = k;
            P.rows_out[pos] = r;
        }
        if (P.perm_out) P.perm_out[pos] = P.perm_in ? P.perm_in[r] : (i64)r;
        if (P.vals_out) {
            const u64 u = P.desc ? ~k : k;
            u64 x;
            if (!P.f64) x = u ^ 0x8000000000000000ULL;
            else if (u == 0ULL) x = P.col[r]; // a NaN: its own sign and payload
            else x = (u & 0x8000000000000000ULL) ? (u & 0x7FFFFFFFFFFFFFFFULL) : ~u;
            P.vals_out[pos] = x;
        }
    }
}

// no pass ran (every key equal, or fewer than two rows): the order is the incoming one
__global__ __launch_bounds__(RFX_BLOCK) void k_sort_identity(const u64 *__restrict__ col, const i64 *__restrict__ perm_in, i64 n, i64 *__restrict__ perm_out,
                                                             u64 *__restrict__ vals_out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        if (perm_out) perm_out[i] = perm_in ? perm_in[i] : i;
        if (vals_out) vals_out[i] = col[i];
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_inverse_perm(const i64 *__restrict__ perm, i64 n, i64 *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 p = perm[i];
        if ((u64)p < (u64)n) out[p] = i; // (a permutation of ours hits every cell once; anything else never writes outside)
    }
}

static int sort_grid(const rfx_ctx *c, i64 n) {
    const i64 want = (n + RFX_BLOCK - 1) / RFX_BLOCK, cap = (i64)rfx_grid(c) * 4;
    return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

static int sort_run(rfx_ctx *c, const void *d_col, int32_t type, i64 n, int desc, const i64 *d_perm_in, i64 *d_perm_out, u64 *d_vals_out, int32_t *passes) {
    RFX_REQUIRE(c, RFX_EINVAL, "NULL context");
    RFX_REQUIRE(type == RFX_I64 || type == RFX_F64, RFX_EINVAL, "key type must be i64 (timestamp) or f64");
    RFX_REQUIRE(n >= 0, RFX_EINVAL, "negative size");
    RFX_REQUIRE(n == 0 || (d_col && (d_perm_out || d_vals_out)), RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(n <= SORT_MAX_ROWS, RFX_ELIMIT, "more than 2^32 - 1 rows (rows travel as 4 bytes)");
    if (passes) *passes = 0;
    if (n == 0) return RFX_OK;
    const int f64 = type == RFX_F64;
    const int items = n < SORT_SMALL_ROWS ? SORT_SMALL_ITEMS : SORT_ITEMS;
    const i64 tile = (i64)SORT_THREADS * items, tiles = (n + tile - 1) / tile;
    // scratch: keys A | keys B | rows A | rows B | counts [256][tiles] | histograms [8][256]   (every part 16-byte aligned)
    const size_t kb = (((size_t)n * 8) + 15) & ~(size_t)15, rb = (((size_t)n * 4) + 15) & ~(size_t)15, cb = (size_t)tiles * 256 * 4, hb = 8 * 256 * 8;
    void *scratch = NULL;
    int rc = rfx_hip_malloc((rfx_ctx_t *)c, &scratch, 2 * kb + 2 * rb + cb + hb);
    if (rc != RFX_OK) return rc;
    char *sp = (char *)scratch;
    u64 *keys[2] = {(u64 *)sp, (u64 *)(sp + kb)};
    unsigned int *rows[2] = {(unsigned int *)(sp + 2 * kb), (unsigned int *)(sp + 2 * kb + rb)};
    unsigned int *counts = (unsigned int *)(sp + 2 * kb + 2 * rb);
    unsigned long long *hist = (unsigned long long *)(sp + 2 * kb + 2 * rb + cb);
    unsigned long long h[8 * 256];
    hipError_t e = hipMemsetAsync(hist, 0, hb, c->stream);
    RFX_KERNEL_BEGIN(c);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_sort_keys, dim3(sort_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, d_perm_in, n, f64, desc, keys[0], hist);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, hist, hb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int todo[8], ntodo = 0;
    if (e == hipSuccess) {
        for (int d = 0; d < 8; d++) {
            int one = 0;
            for (int b = 0; b < 256 && !one; b++) one = h[d * 256 + b] == (unsigned long long)n;
            if (!one) todo[ntodo++] = d;
        }
    }
    int cur = 0, have_rows = 0;
    for (int p = 0; p < ntodo && e == hipSuccess; p++) {
        const int last = p == ntodo - 1;
        SortPass P;
        memset(&P, 0, sizeof(P));
        P.keys_in = keys[cur];
        P.rows_in = have_rows ? rows[cur] : NULL;
        if (!last) {
            P.keys_out = keys[cur ^ 1];
            P.rows_out = rows[cur ^ 1];
        } else {
            P.perm_out = d_perm_out;
            P.perm_in = d_perm_in;
            P.vals_out = d_vals_out;
            P.col = (const u64 *)d_col;
        }
        P.offsets = counts;
        P.n = n;
        P.tiles = tiles;
        P.shift = 8 * todo[p];
        P.f64 = f64;
        P.desc = desc;
        if (items == SORT_ITEMS) {
            hipLaunchKernelGGL((k_sort_count<SORT_ITEMS>), dim3((unsigned)tiles), dim3(SORT_THREADS), 0, c->stream, (const u64 *)keys[cur], n, P.shift, tiles, counts);
            hipLaunchKernelGGL(k_sort_scan, dim3(256), dim3(RFX_BLOCK), 0, c->stream, counts, tiles, (const unsigned long long *)(hist + 256 * todo[p]));
            hipLaunchKernelGGL((k_sort_scatter<SORT_ITEMS>), dim3((unsigned)tiles), dim3(SORT_THREADS), 0, c->stream, P);
        } else {
            hipLaunchKernelGGL((k_sort_count<SORT_SMALL_ITEMS>), dim3((unsigned)tiles), dim3(SORT_THREADS), 0, c->stream, (const u64 *)keys[cur], n, P.shift, tiles, counts);
            hipLaunchKernelGGL(k_sort_scan, dim3(256), dim3(RFX_BLOCK), 0, c->stream, counts, tiles, (const unsigned long long *)(hist + 256 * todo[p]));
            hipLaunchKernelGGL((k_sort_scatter<SORT_SMALL_ITEMS>), dim3((unsigned)tiles), dim3(SORT_THREADS), 0, c->stream, P);
        }
        e = hipGetLastError();
        cur ^= 1;
        have_rows = 1;
    }
    if (e == hipSuccess && ntodo == 0) {
        hipLaunchKernelGGL(k_sort_identity, dim3(sort_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, d_perm_in, n, d_perm_out, d_vals_out);
        e = hipGetLastError();
    }
    RFX_KERNEL_END(c);
    const hipError_t es = hipStreamSynchronize(c->stream); // (the scratch goes back to the context's pool: nothing may still read it)
    rfx_hip_free((rfx_ctx_t *)c, scratch);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        rfx_set_error("rfx_sort: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RFX_ENOMEM : RFX_EHIP;
    }
    if (passes) *passes = ntodo;
    return RFX_OK;
}

extern "C" int rfx_hip_sort_index(rfx_ctx_t *ctx, const void *d_col, int32_t type, int64_t n, int descending, const int64_t *d_perm_in, int64_t *d_perm_out,
                                  int32_t *passes) {
    RFX_REQUIRE(n == 0 || d_perm_out, RFX_EINVAL, "NULL output");
    return sort_run((rfx_ctx *)ctx, d_col, type, (i64)n, descending != 0, (const i64 *)d_perm_in, (i64 *)d_perm_out, NULL, passes);
}
extern "C" int rfx_hip_sort_values(rfx_ctx_t *ctx, const void *d_col, int32_t type, int64_t n, int descending, void *d_out, int64_t *d_perm_out, int32_t *passes) {
    RFX_REQUIRE(n == 0 || d_out, RFX_EINVAL, "NULL output");
    RFX_REQUIRE(n == 0 || d_out != d_col, RFX_EINVAL, "the output may not be the column itself");
    return sort_run((rfx_ctx *)ctx, d_col, type, (i64)n, descending != 0, NULL, (i64 *)d_perm_out, (u64 *)d_out, passes);
}
extern "C" int rfx_hip_inverse_perm(rfx_ctx_t *ctx, const int64_t *d_perm, int64_t n, int64_t *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && n >= 0 && (n == 0 || (d_perm && d_out && d_perm != d_out)), RFX_EINVAL, "bad argument");
    if (n == 0) return RFX_OK;
    hipLaunchKernelGGL(k_inverse_perm, dim3(sort_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_perm, (i64)n, (i64 *)d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
