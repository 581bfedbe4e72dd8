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
//
// Keys of at most 32 bits (B8 / U8, I16, I32 / DATE / TIME as raw cells or as the widened 8-byte image; sort_key32() of rfx_sort_key.hpp) travel as
// ONE u64 record, key << 32 | row, in one ping-pong pair: k_sort_keys32 builds the records and only the 1, 2 or 4 histograms the key's width has,
// a pass streams 8 B per row in and out instead of 12, and the last pass decodes the sorted cells in the column's own width from the key alone.
// The digit of a pass sits at bit 32 + 8 d of the record, so k_sort_count and k_sort_scan run as they are; k_sort_scatter is one template over the
// record form.
#include "rfx_cells.hpp"
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

// ---- packed records + the histograms of a key of at most 32 bits ----
typedef unsigned v4u __attribute__((ext_vector_type(4)));
// one cell's digits into the workgroup's histograms; a digit the whole wave agrees on is one add, as above
template <int NDIG> __device__ __forceinline__ void sort_hist32(unsigned int *lh, unsigned int k, int lane) {
#pragma unroll
    for (int d = 0; d < NDIG; d++) {
        const int dg = (int)((k >> (8 * d)) & 255), first = __builtin_amdgcn_readfirstlane(dg);
        const u64 active = __ballot(1);
        if (__ballot(dg == first) == active) {
            if (lane == __ffsll((long long)active) - 1) atomicAdd(&lh[d * 256 + first], (unsigned int)__popcll(active));
        } else atomicAdd(&lh[d * 256 + dg], 1u);
    }
}
template <int CLS> __device__ __forceinline__ u64 sort_ld32(const void *p, i64 r) {
    if (CLS == SK_U8) return ((const unsigned char *)p)[r];
    if (CLS == SK_I16) return ((const unsigned short *)p)[r];
    if (CLS == SK_I32) return ((const unsigned int *)p)[r];
    return ((const u64 *)p)[r];
}
// cell j of a lane's 16 bytes
template <int CLS> __device__ __forceinline__ u64 sort_pick32(const unsigned int *w, int j) {
    if (CLS == SK_U8) return (w[j / 4] >> (8 * (j % 4))) & 0xFFu;
    if (CLS == SK_I16) return (w[j / 2] >> (16 * (j % 2))) & 0xFFFFu;
    if (CLS == SK_I32) return w[j];
    return ((u64)w[2 * j + 1] << 32) | w[2 * j];
}
// The column read once.  Without perm_in and with a 16-byte aligned column (vec) a lane takes whole 16-byte accesses: 16, 8, 4 or 2 cells in, as
// many records out in 16-byte stores; the cells after the last whole run, and every cell read through perm_in, go one by one.
template <int CLS>
__global__ __launch_bounds__(RFX_BLOCK) void k_sort_keys32(const void *__restrict__ col, const i64 *__restrict__ perm_in, i64 n, int desc, int vec,
                                                           u64 *__restrict__ recs, unsigned long long *__restrict__ hist) {
    constexpr int NDIG = sort_key32_bytes(CLS), R = 16 / sort_src32_bytes(CLS);
    __shared__ unsigned int lh[NDIG * 256];
    for (int i = threadIdx.x; i < NDIG * 256; i += RFX_BLOCK) lh[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK, nr = (vec && !perm_in) ? n / R : 0;
    for (i64 g = tid; g < nr; g += nt) {
        const v4u t = __builtin_nontemporal_load((const v4u *)col + g);
        const unsigned int w[4] = {t.x, t.y, t.z, t.w};
        v4u *out = (v4u *)recs + g * (R / 2);
#pragma unroll
        for (int j = 0; j < R; j += 2) {
            const unsigned int k0 = sort_key32(sort_pick32<CLS>(w, j), CLS, desc), k1 = sort_key32(sort_pick32<CLS>(w, j + 1), CLS, desc);
            sort_hist32<NDIG>(lh, k0, lane);
            sort_hist32<NDIG>(lh, k1, lane);
            v4u o;
            o.x = (unsigned int)(g * R + j); o.y = k0; o.z = (unsigned int)(g * R + j + 1); o.w = k1; // (little-endian: row below key)
            out[j / 2] = o;
        }
    }
    for (i64 i = nr * R + tid; i < n; i += nt) {
        u64 x;
        if (perm_in) {
            const i64 r = perm_in[i];
            x = ((u64)r < (u64)n) ? sort_ld32<CLS>(col, r) : (CLS == SK_I32W ? (u64)RFX_NULL_I64_D : 0ULL); // (never a read beyond the column)
        } else x = sort_ld32<CLS>(col, i);
        const unsigned int k = sort_key32(x, CLS, desc);
        recs[i] = ((u64)k << 32) | (u64)(unsigned int)i;
        sort_hist32<NDIG>(lh, k, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NDIG * 256; i += RFX_BLOCK)
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
    u64 *vals_out;               // last pass: the sorted cells (NULL: not wanted); packed records: cells of the column's own width
    const u64 *col;              // the column (a NaN's own bits)
    const unsigned int *offsets; // [256][tiles]
    i64 n, tiles;
    int shift, f64, desc, cls; // shift: of the digit inside keys_in's u64 (packed: 32 + 8 d); cls: the packed key's source class (SK_*)
};

// PACKED: keys_in / keys_out hold key << 32 | row records (rows_in / rows_out unused)
template <int ITEMS, int PACKED>
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
        if (PACKED) {
            const unsigned int r = (unsigned int)k;
            if (P.keys_out) P.keys_out[pos] = k;
            if (P.perm_out) P.perm_out[pos] = P.perm_in ? P.perm_in[r] : (i64)r;
            if (P.vals_out) {
                const unsigned int x = sort_cell32((unsigned int)(k >> 32), P.cls, P.desc);
                if (P.cls == SK_U8) ((unsigned char *)P.vals_out)[pos] = (unsigned char)x;
                else if (P.cls == SK_I16) ((unsigned short *)P.vals_out)[pos] = (unsigned short)x;
                else ((unsigned int *)P.vals_out)[pos] = x;
            }
            continue;
        }
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

// the same for a key of at most 32 bits: the cells leave in the column's own width (the widened image narrowed)
template <int CLS>
__global__ __launch_bounds__(RFX_BLOCK) void k_sort_identity32(const void *__restrict__ col, const i64 *__restrict__ perm_in, i64 n, i64 *__restrict__ perm_out,
                                                               void *__restrict__ vals_out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        if (perm_out) perm_out[i] = perm_in ? perm_in[i] : i;
        if (vals_out) {
            const unsigned int x = sort_cell32(sort_key32(sort_ld32<CLS>(col, i), CLS, 0), CLS, 0);
            if (CLS == SK_U8) ((unsigned char *)vals_out)[i] = (unsigned char)x;
            else if (CLS == SK_I16) ((unsigned short *)vals_out)[i] = (unsigned short)x;
            else ((unsigned int *)vals_out)[i] = x;
        }
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_inverse_perm(const i64 *__restrict__ perm, i64 n, i64 *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 p = perm[i];
        if ((u64)p < (u64)n) out[p] = i; // (a permutation of ours hits every cell once; anything else never writes outside)
    }
}

// one digit pass of either record form: the tile counts, their scan from the digit's histogram, the scatter
template <int PACKED>
static void sort_launch_pass(rfx_ctx *c, int items, const SortPass &P, unsigned int *counts, const unsigned long long *digit_hist) {
    const dim3 grid((unsigned)P.tiles), block(SORT_THREADS);
    if (items == SORT_ITEMS) hipLaunchKernelGGL((k_sort_count<SORT_ITEMS>), grid, block, 0, c->stream, P.keys_in, P.n, P.shift, P.tiles, counts);
    else hipLaunchKernelGGL((k_sort_count<SORT_SMALL_ITEMS>), grid, block, 0, c->stream, P.keys_in, P.n, P.shift, P.tiles, counts);
    hipLaunchKernelGGL(k_sort_scan, dim3(256), dim3(RFX_BLOCK), 0, c->stream, counts, P.tiles, digit_hist);
    if (items == SORT_ITEMS) hipLaunchKernelGGL((k_sort_scatter<SORT_ITEMS, PACKED>), grid, block, 0, c->stream, P);
    else hipLaunchKernelGGL((k_sort_scatter<SORT_SMALL_ITEMS, PACKED>), grid, block, 0, c->stream, P);
}
// the source class of a key of at most 32 bits (-1: another type)
static int sort_class32(int32_t type) {
    switch (type) {
        case RFX_B8: case RFX_U8: return SK_U8;
        case RFX_I16: return SK_I16;
        case RFX_I32: return SK_I32;
        case RFX_I32_WIDE: return SK_I32W;
        default: return -1;
    }
}
template <int CLS>
static void sort_launch_keys32(rfx_ctx *c, const void *d_col, const i64 *d_perm_in, i64 n, int desc, u64 *recs, unsigned long long *hist) {
    const int vec = ((uintptr_t)d_col & 15) == 0;
    const i64 per = (vec && !d_perm_in) ? 16 / sort_src32_bytes(CLS) : 1;
    hipLaunchKernelGGL((k_sort_keys32<CLS>), dim3(rfx_stream_grid(c, (n + per - 1) / per)), dim3(RFX_BLOCK), 0, c->stream, d_col, d_perm_in, n, desc, vec, recs, hist);
}
template <int CLS>
static void sort_launch_identity32(rfx_ctx *c, const void *d_col, const i64 *d_perm_in, i64 n, i64 *d_perm_out, void *d_vals_out) {
    hipLaunchKernelGGL((k_sort_identity32<CLS>), dim3(rfx_stream_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, d_col, d_perm_in, n, d_perm_out, d_vals_out);
}
#define SORT_BY_CLASS32(cls, fn, ...)                         \
    do {                                                      \
        if ((cls) == SK_U8) fn<SK_U8>(__VA_ARGS__);           \
        else if ((cls) == SK_I16) fn<SK_I16>(__VA_ARGS__);    \
        else if ((cls) == SK_I32) fn<SK_I32>(__VA_ARGS__);    \
        else fn<SK_I32W>(__VA_ARGS__);                        \
    } while (0)

// keys of at most 32 bits: one pair of n packed records, the histograms and passes the key's width has
static int sort_run32(rfx_ctx *c, const void *d_col, int cls, i64 n, int desc, const i64 *d_perm_in, i64 *d_perm_out, void *d_vals_out, int32_t *passes) {
    const int ndig = sort_key32_bytes(cls);
    const int items = n < SORT_SMALL_ROWS ? SORT_SMALL_ITEMS : SORT_ITEMS;
    const i64 tile = (i64)SORT_THREADS * items, tiles = (n + tile - 1) / tile;
    // scratch: records A | records B | counts [256][tiles] | histograms [ndig][256]   (every part 16-byte aligned)
    const size_t kb = (((size_t)n * 8) + 15) & ~(size_t)15, cb = (size_t)tiles * 256 * 4, hb = (size_t)ndig * 256 * 8;
    void *scratch = NULL;
    int rc = rfx_hip_malloc((rfx_ctx_t *)c, &scratch, 2 * kb + cb + hb);
    if (rc != RFX_OK) return rc;
    char *sp = (char *)scratch;
    u64 *recs[2] = {(u64 *)sp, (u64 *)(sp + kb)};
    unsigned int *counts = (unsigned int *)(sp + 2 * kb);
    unsigned long long *hist = (unsigned long long *)(sp + 2 * kb + cb);
    unsigned long long h[4 * 256];
    hipError_t e = hipMemsetAsync(hist, 0, hb, c->stream);
    RFX_KERNEL_BEGIN(c);
    if (e == hipSuccess) {
        SORT_BY_CLASS32(cls, sort_launch_keys32, c, d_col, d_perm_in, n, desc, recs[0], hist);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, hist, hb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int todo[4], ntodo = 0;
    if (e == hipSuccess) {
        for (int d = 0; d < ndig; d++) {
            int one = 0;
            for (int b = 0; b < 256 && !one; b++) one = h[d * 256 + b] == (unsigned long long)n;
            if (!one) todo[ntodo++] = d;
        }
    }
    int cur = 0;
    for (int p = 0; p < ntodo && e == hipSuccess; p++) {
        const int last = p == ntodo - 1;
        SortPass P;
        memset(&P, 0, sizeof(P));
        P.keys_in = recs[cur];
        if (!last) P.keys_out = recs[cur ^ 1];
        else {
            P.perm_out = d_perm_out;
            P.perm_in = d_perm_in;
            P.vals_out = (u64 *)d_vals_out;
        }
        P.offsets = counts;
        P.n = n;
        P.tiles = tiles;
        P.shift = 32 + 8 * todo[p];
        P.desc = desc;
        P.cls = cls;
        sort_launch_pass<1>(c, items, P, counts, hist + 256 * todo[p]);
        e = hipGetLastError();
        cur ^= 1;
    }
    if (e == hipSuccess && ntodo == 0) {
        SORT_BY_CLASS32(cls, sort_launch_identity32, c, d_col, d_perm_in, n, d_perm_out, d_vals_out);
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

static int sort_run(rfx_ctx *c, const void *d_col, int32_t type, i64 n, int desc, const i64 *d_perm_in, i64 *d_perm_out, u64 *d_vals_out, int32_t *passes) {
    RFX_REQUIRE(c, RFX_EINVAL, "NULL context");
    const int cls32 = sort_class32(type);
    RFX_REQUIRE(type == RFX_I64 || type == RFX_F64 || cls32 >= 0, RFX_EINVAL, "key type must be i64 (timestamp), f64, i32 (date, time; raw or widened), i16, u8 or b8");
    RFX_REQUIRE(n >= 0, RFX_EINVAL, "negative size");
    RFX_REQUIRE(n == 0 || (d_col && (d_perm_out || d_vals_out)), RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(n <= SORT_MAX_ROWS, RFX_ELIMIT, "more than 2^32 - 1 rows (rows travel as 4 bytes)");
    if (passes) *passes = 0;
    if (n == 0) return RFX_OK;
    if (cls32 >= 0) return sort_run32(c, d_col, cls32, n, desc, d_perm_in, d_perm_out, d_vals_out, passes);
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
        hipLaunchKernelGGL(k_sort_keys, dim3(rfx_stream_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, d_perm_in, n, f64, desc, keys[0], hist);
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
        sort_launch_pass<0>(c, items, P, counts, hist + 256 * todo[p]);
        e = hipGetLastError();
        cur ^= 1;
        have_rows = 1;
    }
    if (e == hipSuccess && ntodo == 0) {
        hipLaunchKernelGGL(k_sort_identity, dim3(rfx_stream_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_col, d_perm_in, n, d_perm_out, d_vals_out);
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
    hipLaunchKernelGGL(k_inverse_perm, dim3(rfx_stream_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_perm, (i64)n, (i64 *)d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
