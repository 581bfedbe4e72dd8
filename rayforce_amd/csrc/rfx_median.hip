// rfx_median.hip -- exact medians on the device: `med` scalar (ray_med, core/math.c:2529-2626) and grouped (aggr_med, core/aggr.c:2136-2247).
//
// A median is an order statistic: the values of ranks (l-1)/2 and l/2 among a group's l selected rows (nulls included), then a fixed
// formula -- so the answer is bit-exact, whatever order the rows arrive in.  The ranks are taken over the reference's sort keys
// (core/sort.c:266-311): i64 x -> x ^ 2^63 (NULL_I64 first); f64 NaN -> 0, negative -> ~bits, else bits | 2^63 (-0.0 before +0.0).
//
// Passes (every one applies the where: -- rfx_pred_t through the common predicate code, or the caller's B8 mask -- and the row's group
// lookup, so no per-row selection or index column is ever written):
//   1. k_med_count     rows per group (LDS-private counters when the groups fit, global atomics otherwise)
//   2. k_scan_*        exclusive scan of the counts -> every group's segment [off[g], off[g+1])
//   3. k_med_scatter   every selected row's sort key into its group's segment (order inside a segment is free); few groups reserve a
//                      block's share of a segment with ONE global atomic per group and fill it through LDS cursors
//   4. k_med_classify  every group into one of three size classes:
//        tiny   (<= 64 rows)            k_med_tiny:   one wave per segment, every lane ranks its key by counting over the segment
//        medium (<= MED_LDS rows)       k_med_lds:    one workgroup per segment, bitonic sort in LDS, the two ranks read off
//        large                          k_med_hist / k_med_pick: MSB-first radix select, 8 digits of 8 bits; every segment is cut into
//                                       chunks of MED_CHUNK keys (many workgroups per segment, all large segments in one launch), the
//                                       chunks' LDS histograms merged into the segment's global one, one pick step per digit
//   5. every class writes its groups' answers itself (med_finish: the grouped or the scalar rule of the value type).
// Scratch (rfx_hip_malloc, freed before return): 8 B per selected row (the keys) + 24 B per group (offsets, cursors, class lists) + per
// large segment 4 KB of histogram and state.
// Stores are plain vector stores and atomics.
#include "rfx_scalar_kernel.hpp"
#include "rfx_cells.hpp"

#define MED_TINY 64
#define MED_LDS 8192                        // medium class: keys of one segment in LDS (64 KB)
#define MED_CHUNK 65536                     // large class: keys one workgroup histograms per digit
#define MED_GLDS 2048                       // up to this many groups the count / scatter passes keep per-group counters in LDS
#define MED_ROWS_PER_BLOCK (RFX_BLOCK * 32) // scatter with LDS cursors: rows one workgroup reserves space for at once

struct MedArgs {
    Plan P;
    const signed char *mask;
    const i64 *gids;  // per-row group index ...
    const i64 *key;   // ... or the key, looked up through table[key - kmin]
    const i64 *table;
    i64 kmin, range;
    const u64 *val;
    int f64, rule;
    i64 nrows, groups;
};

__device__ __host__ __forceinline__ u64 med_key(u64 x, int f64) {
    if (!f64) return x ^ 0x8000000000000000ULL;
    if ((x & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL) return 0ULL; // NaN (either sign)
    return (x & 0x8000000000000000ULL) ? ~x : (x | 0x8000000000000000ULL);
}
__device__ __host__ __forceinline__ u64 med_unkey(u64 k, int f64) {
    if (!f64) return k ^ 0x8000000000000000ULL;
    if (k == 0ULL) return RFX_NAN_BITS;
    return (k & 0x8000000000000000ULL) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k;
}
// a subnormal as the zero of its sign: the reference's release build (-funsafe-math-optimizations) runs with the x86 FTZ / DAZ modes,
// so its f64 arithmetic reads and writes subnormals as zeros
__device__ __forceinline__ double med_flush(double x) {
    const u64 b = rfx_as_u64(x);
    return (b & 0x7FF0000000000000ULL) ? x : rfx_as_f64(b & 0x8000000000000000ULL);
}
// the reference's formulas over l values: grouped (aggr_med_partial) converts both i64 halves to f64 before adding; scalar ray_med adds
// them as i64 first (wrapping), then converts
__device__ __forceinline__ double med_finish(u64 klo, u64 khi, i64 len, int f64, int rule) {
    if (len <= 0) return rfx_as_f64(RFX_NAN_BITS);
    const u64 lo = med_unkey(klo, f64), hi = med_unkey(khi, f64);
    if (len & 1) return f64 ? rfx_as_f64(hi) : (double)(i64)hi;
    if (f64) return med_flush(med_flush(med_flush(rfx_as_f64(lo)) + med_flush(rfx_as_f64(hi))) / 2.0);
    if (rule == RFX_MED_SCALAR) return (double)(i64)(lo + hi) / 2.0;
    return ((double)(i64)lo + (double)(i64)hi) / 2.0;
}

// the group of row r, or -1: not selected / no group
__device__ __forceinline__ i64 med_group(const MedArgs &A, const PredSet<RFX_MAX_PREDS> &S, i64 r) {
    if (A.mask && !A.mask[r]) return -1;
    if (A.P.npred) {
        u64 v[RFX_MAX_COLS][1];
#pragma unroll
        for (int c = 0; c < RFX_MAX_COLS; c++) v[c][0] = c < A.P.ncols ? A.P.cols[c][r] : 0ULL;
        bool valid[1] = {true}, sel[1];
        eval_sel<RFX_MAX_COLS, 1, RFX_MAX_PREDS>(S, v, valid, sel);
        if (!sel[0]) return -1;
    }
    i64 g = 0;
    if (A.gids) g = A.gids[r];
    else if (A.key) {
        const u64 s = (u64)A.key[r] - (u64)A.kmin;
        if (s >= (u64)A.range) return -1;
        g = A.table[s];
    }
    return ((u64)g < (u64)A.groups) ? g : -1;
}

// (scalar rule: the nulls among the selected values are counted too, into *nulls)
__global__ __launch_bounds__(RFX_BLOCK) void k_med_count(const MedArgs A, unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ nulls) {
    __shared__ unsigned int lc[MED_GLDS];
    __shared__ unsigned int ln;
    if (threadIdx.x == 0) ln = 0;
    PredSet<RFX_MAX_PREDS> S;
    predset_load<RFX_MAX_PREDS>(A.P, S);
    const bool lds = A.groups <= MED_GLDS;
    if (lds)
        for (int i = threadIdx.x; i < A.groups; i += RFX_BLOCK) lc[i] = 0;
    __syncthreads();
    for (i64 r = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; r < A.nrows; r += (i64)gridDim.x * RFX_BLOCK) {
        const i64 g = med_group(A, S, r);
        if (g < 0) continue;
        if (lds) atomicAdd(&lc[g], 1u);
        else atomicAdd(&cnt[g], 1ULL);
        if (A.rule == RFX_MED_SCALAR && A.val[r] == (u64)RFX_NULL_I64_D) atomicAdd(&ln, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && ln) atomicAdd(nulls, (unsigned long long)ln);
    if (lds) {
        for (int i = threadIdx.x; i < A.groups; i += RFX_BLOCK)
            if (lc[i]) atomicAdd(&cnt[i], (unsigned long long)lc[i]);
    }
}

// ---- exclusive scan of n counts in place, off[n] = total.  Tiles of RFX_BLOCK * 8; the tiles' totals scanned by one workgroup ----
#define SCAN_EPT 8
#define SCAN_TILE (RFX_BLOCK * SCAN_EPT)
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64 *tot) {
    __shared__ u64 s[RFX_BLOCK];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < RFX_BLOCK; d <<= 1) {
        const u64 a = threadIdx.x >= (unsigned)d ? s[threadIdx.x - d] : 0ULL;
        __syncthreads();
        s[threadIdx.x] += a;
        __syncthreads();
    }
    const u64 incl = s[threadIdx.x];
    *tot = s[RFX_BLOCK - 1];
    __syncthreads();
    return incl - v;
}
__global__ __launch_bounds__(RFX_BLOCK) void k_scan_tiles(u64 *__restrict__ a, i64 n, u64 *__restrict__ tile_sum) {
    const i64 base = blockIdx.x * (i64)SCAN_TILE + threadIdx.x * (i64)SCAN_EPT;
    u64 v[SCAN_EPT], t = 0;
#pragma unroll
    for (int e = 0; e < SCAN_EPT; e++) {
        v[e] = base + e < n ? a[base + e] : 0ULL;
        t += v[e];
    }
    u64 tot;
    u64 p = block_excl_scan(t, &tot);
#pragma unroll
    for (int e = 0; e < SCAN_EPT; e++) {
        if (base + e < n) a[base + e] = p;
        p += v[e];
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(RFX_BLOCK) void k_scan_top(u64 *__restrict__ tile_sum, i64 ntiles, u64 *__restrict__ total) {
    u64 carry = 0;
    for (i64 b = 0; b < ntiles; b += RFX_BLOCK) {
        const i64 i = b + threadIdx.x;
        const u64 v = i < ntiles ? tile_sum[i] : 0ULL;
        u64 tot;
        const u64 p = block_excl_scan(v, &tot);
        if (i < ntiles) tile_sum[i] = carry + p;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(RFX_BLOCK) void k_scan_add(u64 *__restrict__ a, i64 n, const u64 *__restrict__ tile_sum) {
    const i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x;
    if (i < n) a[i] += tile_sum[i / SCAN_TILE];
}

// ---- scatter: keys[cur[g]++] = key(value) ----
__global__ __launch_bounds__(RFX_BLOCK) void k_med_scatter(const MedArgs A, unsigned long long *__restrict__ cur, u64 *__restrict__ keys) {
    PredSet<RFX_MAX_PREDS> S;
    predset_load<RFX_MAX_PREDS>(A.P, S);
    for (i64 r = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; r < A.nrows; r += (i64)gridDim.x * RFX_BLOCK) {
        const i64 g = med_group(A, S, r);
        if (g < 0) continue;
        const u64 at = atomicAdd(&cur[g], 1ULL);
        keys[at] = med_key(A.val[r], A.f64);
    }
}
// few groups: a block's rows [c * MED_ROWS_PER_BLOCK, ...) counted per group in LDS, one global reservation per group, then filled
__global__ __launch_bounds__(RFX_BLOCK) void k_med_scatter_lds(const MedArgs A, unsigned long long *__restrict__ cur, u64 *__restrict__ keys) {
    __shared__ unsigned int lc[MED_GLDS];
    __shared__ unsigned long long lb[MED_GLDS];
    PredSet<RFX_MAX_PREDS> S;
    predset_load<RFX_MAX_PREDS>(A.P, S);
    const i64 nchunks = (A.nrows + MED_ROWS_PER_BLOCK - 1) / MED_ROWS_PER_BLOCK;
    for (i64 c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const i64 r0 = c * MED_ROWS_PER_BLOCK, r1 = r0 + MED_ROWS_PER_BLOCK < A.nrows ? r0 + MED_ROWS_PER_BLOCK : A.nrows;
        for (int i = threadIdx.x; i < A.groups; i += RFX_BLOCK) lc[i] = 0;
        __syncthreads();
        for (i64 r = r0 + threadIdx.x; r < r1; r += RFX_BLOCK) {
            const i64 g = med_group(A, S, r);
            if (g >= 0) atomicAdd(&lc[g], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < A.groups; i += RFX_BLOCK) {
            lb[i] = lc[i] ? atomicAdd(&cur[i], (unsigned long long)lc[i]) : 0ULL;
            lc[i] = 0;
        }
        __syncthreads();
        for (i64 r = r0 + threadIdx.x; r < r1; r += RFX_BLOCK) {
            const i64 g = med_group(A, S, r);
            if (g < 0) continue;
            const u64 at = lb[g] + atomicAdd(&lc[g], 1u);
            keys[at] = med_key(A.val[r], A.f64);
        }
        __syncthreads();
    }
}

// ---- size classes: tiny ids from the front of `cls`, medium ids from its back; large ids and lengths into their own lists ----
__device__ __forceinline__ i64 wave_append(bool p, unsigned long long *ctr) {
    const u64 m = __ballot(p);
    if (!m) return -1;
    const int lane = __lane_id();
    const int leader = __ffsll((long long)m) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    return p ? (i64)(base + __popcll(m & ((1ULL << lane) - 1ULL))) : -1;
}
__global__ __launch_bounds__(RFX_BLOCK) void k_med_classify(const u64 *__restrict__ off, i64 groups, unsigned long long *__restrict__ ctr, i64 *__restrict__ cls,
                                                            i64 *__restrict__ large, i64 large_cap) {
    const i64 g0 = blockIdx.x * (i64)RFX_BLOCK;
    const i64 g = g0 + threadIdx.x;
    const i64 len = g < groups ? (i64)(off[g + 1] - off[g]) : 0;
    const bool in = g < groups;
    const i64 t = wave_append(in && len <= MED_TINY, &ctr[0]);
    const i64 m = wave_append(in && len > MED_TINY && len <= MED_LDS, &ctr[1]);
    const i64 l = wave_append(in && len > MED_LDS, &ctr[2]);
    if (t >= 0) cls[t] = g;
    if (m >= 0) cls[groups - 1 - m] = g;
    if (l >= 0 && l < large_cap) {
        large[l] = g;
        large[large_cap + l] = len;
    }
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}
// tiny: one wave per segment; lane i holds key i, its rank = keys below it + equal keys at lower positions
// (the grid is capped: every wave walks segments w, w + waves in the grid, ...)
// l = the segment's length, or with the scalar rule its non-null count (ray_med's l = ray_cnt(x), core/math.c:2530); the ranks
// (l-1)/2 and l/2 are taken in the WHOLE sorted segment, nulls first
__device__ __forceinline__ i64 med_len(i64 len, const unsigned long long *nulls) { return nulls ? len - (i64)*nulls : len; }
__global__ __launch_bounds__(RFX_BLOCK) void k_med_tiny(const u64 *__restrict__ off, const u64 *__restrict__ keys, const i64 *__restrict__ cls, i64 n, int f64,
                                                        int rule, const unsigned long long *__restrict__ nulls, double *__restrict__ out) {
    const int lane = threadIdx.x % RFX_WAVE;
    for (i64 w = blockIdx.x * (i64)(RFX_BLOCK / RFX_WAVE) + threadIdx.x / RFX_WAVE; w < n; w += (i64)gridDim.x * (RFX_BLOCK / RFX_WAVE)) {
        const i64 g = cls[w];
        const u64 o = off[g];
        const int len = (int)(off[g + 1] - o);
        const int l = (int)med_len(len, nulls);
        const u64 k = lane < len ? keys[o + lane] : ~0ULL;
        int rank = 0;
        for (int j = 0; j < len; j++) {
            const u64 kj = shfl_u64(k, j);
            rank += (kj < k) || (kj == k && j < lane);
        }
        const int rlo = (l - 1) / 2, rhi = l / 2;
        const u64 mlo = __ballot(lane < len && rank == rlo), mhi = __ballot(lane < len && rank == rhi);
        const u64 klo = mlo ? shfl_u64(k, __ffsll((long long)mlo) - 1) : 0ULL, khi = mhi ? shfl_u64(k, __ffsll((long long)mhi) - 1) : 0ULL;
        if (lane == 0) out[g] = med_finish(klo, khi, l, f64, rule);
    }
}
// medium: one workgroup per segment, bitonic sort of the segment (padded to a power of two with ~0) in LDS
__global__ __launch_bounds__(RFX_BLOCK) void k_med_lds(const u64 *__restrict__ off, const u64 *__restrict__ keys, const i64 *__restrict__ cls, i64 groups,
                                                       i64 nm, int f64, int rule, const unsigned long long *__restrict__ nulls, double *__restrict__ out) {
    __shared__ u64 s[MED_LDS];
    for (i64 seg = blockIdx.x; seg < nm; seg += gridDim.x) { // (the grid is capped: every workgroup walks segments seg, seg + gridDim.x, ...)
        const i64 g = cls[groups - 1 - seg];
        const u64 o = off[g];
        const int len = (int)(off[g + 1] - o);
        int n2 = 1;
        while (n2 < len) n2 <<= 1;
        for (int i = threadIdx.x; i < n2; i += RFX_BLOCK) s[i] = i < len ? keys[o + i] : ~0ULL;
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = threadIdx.x; t < n2 / 2; t += RFX_BLOCK) {
                    const int i = 2 * t - (t & (j - 1)); // the lower index of this thread's pair
                    const int p = i + j;
                    const bool up = (i & k) == 0;
                    const u64 a = s[i], b = s[p];
                    if ((a > b) == up) {
                        s[i] = b;
                        s[p] = a;
                    }
                }
                __syncthreads();
            }
        }
        const i64 l = med_len(len, nulls);
        if (threadIdx.x == 0) out[g] = l > 0 ? med_finish(s[(l - 1) / 2], s[l / 2], l, f64, rule) : rfx_as_f64(RFX_NAN_BITS);
        __syncthreads(); // (s is refilled for the next segment)
    }
}

// large: per segment j  st[j] = {group, prefix lo, prefix hi, rank left lo, rank left hi},  hist[j][2][256]
struct MedLarge {
    u64 plo, phi;
    i64 klo, khi;
};
__global__ __launch_bounds__(RFX_BLOCK) void k_med_large_init(const u64 *__restrict__ off, const i64 *__restrict__ large, i64 nl, const unsigned long long *__restrict__ nulls,
                                                             MedLarge *__restrict__ st) {
    const i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x;
    if (j >= nl) return;
    const i64 g = large[j];
    i64 len = med_len((i64)(off[g + 1] - off[g]), nulls);
    if (len <= 0) len = 1; // (no value counts: the ranks are never read, k_med_large_out answers null)
    st[j].plo = 0;
    st[j].phi = 0;
    st[j].klo = (len - 1) / 2;
    st[j].khi = len / 2;
}
// one workgroup per (segment, chunk) of the chunk table: the digit at `shift` of every key whose higher digits equal a prefix
__global__ __launch_bounds__(RFX_BLOCK) void k_med_hist(const u64 *__restrict__ off, const u64 *__restrict__ keys, const i64 *__restrict__ large,
                                                        const i64 *__restrict__ chunk_seg, const i64 *__restrict__ chunk_at, const MedLarge *__restrict__ st,
                                                        unsigned long long *__restrict__ hist, int shift) {
    __shared__ unsigned int h[2][256];
    const i64 j = chunk_seg[blockIdx.x];
    const i64 g = large[j];
    const u64 o = off[g], len = off[g + 1] - o;
    const u64 a = (u64)chunk_at[blockIdx.x], b = a + MED_CHUNK < len ? a + MED_CHUNK : len;
    for (int i = threadIdx.x; i < 512; i += RFX_BLOCK) h[i >> 8][i & 255] = 0;
    __syncthreads();
    const MedLarge m = st[j];
    const int hs = shift + 8;
    const u64 hlo = hs >= 64 ? 0ULL : m.plo >> hs, hhi = hs >= 64 ? 0ULL : m.phi >> hs;
    const bool two = hlo != hhi;
    for (u64 i = a + threadIdx.x; i < b; i += RFX_BLOCK) {
        const u64 k = keys[o + i];
        const u64 hk = hs >= 64 ? 0ULL : k >> hs;
        const unsigned d = (unsigned)(k >> shift) & 255u;
        if (hk == hlo) atomicAdd(&h[0][d], 1u);
        if (two && hk == hhi) atomicAdd(&h[1][d], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += RFX_BLOCK) {
        const unsigned v = h[i >> 8][i & 255];
        if (v) atomicAdd(&hist[j * 512 + i], (unsigned long long)v);
    }
}
// one wave per segment: the digit that holds each remaining rank; the histogram cleared for the next digit
__device__ __forceinline__ void med_pick_one(const unsigned long long *h, i64 &k, u64 &prefix, int shift) {
    i64 cum = 0;
    for (int d = 0; d < 256; d++) {
        const i64 c = (i64)h[d];
        if (cum + c > k) {
            prefix |= (u64)d << shift;
            k -= cum;
            return;
        }
        cum += c;
    }
}
__global__ __launch_bounds__(RFX_BLOCK) void k_med_pick(MedLarge *__restrict__ st, i64 nl, unsigned long long *__restrict__ hist, int shift) {
    const i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x;
    if (j >= nl) return;
    MedLarge m = st[j];
    const int hs = shift + 8;
    const bool two = (hs >= 64 ? 0ULL : m.plo >> hs) != (hs >= 64 ? 0ULL : m.phi >> hs);
    unsigned long long *h = hist + j * 512;
    med_pick_one(h, m.klo, m.plo, shift);
    med_pick_one(two ? h + 256 : h, m.khi, m.phi, shift);
    st[j] = m;
    for (int i = 0; i < 512; i++) h[i] = 0ULL;
}
__global__ __launch_bounds__(RFX_BLOCK) void k_med_large_out(const u64 *__restrict__ off, const i64 *__restrict__ large, i64 nl, const MedLarge *__restrict__ st,
                                                             int f64, int rule, const unsigned long long *__restrict__ nulls, double *__restrict__ out) {
    const i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x;
    if (j >= nl) return;
    const i64 g = large[j];
    out[g] = med_finish(st[j].plo, st[j].phi, med_len((i64)(off[g + 1] - off[g]), nulls), f64, rule);
}

static inline unsigned blocks_of(i64 n, i64 per) { return (unsigned)((n + per - 1) / per); }
static inline unsigned capped(i64 blocks, i64 cap) { return (unsigned)(blocks < cap ? blocks : cap); }

extern "C" int rfx_hip_group_median(rfx_ctx_t *ctx, const rfx_med_rows_t *rows, const void *d_val, int32_t val_type, int64_t nrows, int64_t groups, int32_t rule,
                                    double *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && rows, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(val_type == RFX_I64 || val_type == RFX_F64, RFX_EINVAL, "value type must be i64 or f64");
    RFX_REQUIRE(rule == RFX_MED_GROUPED || (rule == RFX_MED_SCALAR && val_type == RFX_I64), RFX_EINVAL, "bad median rule");
    RFX_REQUIRE(nrows >= 0 && groups >= 0, RFX_EINVAL, "negative size");
    if (groups == 0) return RFX_OK;
    RFX_REQUIRE(d_out && (nrows == 0 || d_val), RFX_EINVAL, "NULL column");
    RFX_REQUIRE(!(rows->d_gids && rows->d_key), RFX_EINVAL, "group ids and a key table are exclusive");
    RFX_REQUIRE(!rows->d_key || (rows->d_table && rows->range > 0), RFX_EINVAL, "key without a slot table");
    RFX_REQUIRE(rows->d_gids || rows->d_key || groups == 1, RFX_EINVAL, "several groups without a group lookup");
    MedArgs A;
    memset(&A, 0, sizeof(A));
    int rc = rfx_plan_build(&A.P, rows->preds, rows->npred, rows->npred ? rows->logic : RFX_AND, NULL, 0, NULL, NULL, nrows, 0);
    if (rc != RFX_OK) return rc;
    A.mask = (const signed char *)rows->d_mask;
    A.gids = (const i64 *)rows->d_gids;
    A.key = (const i64 *)rows->d_key;
    A.table = (const i64 *)rows->d_table;
    A.kmin = rows->kmin;
    A.range = rows->range;
    A.val = (const u64 *)d_val;
    A.f64 = val_type == RFX_F64;
    A.rule = rule;
    A.nrows = nrows;
    A.groups = groups;

    // scratch: off (groups + 1) | cur (groups) | cls (groups) | tile sums | 4 counters
    const i64 ntiles = (groups + 1 + SCAN_TILE - 1) / SCAN_TILE;
    void *blk = NULL, *dkeys = NULL, *dlarge = NULL;
    const size_t bytes = (size_t)(3 * groups + 1 + ntiles + 5) * 8;
    rc = rfx_hip_malloc(ctx, &blk, bytes);
    if (rc != RFX_OK) return rc;
    u64 *off = (u64 *)blk, *cur = off + groups + 1, *tiles = cur + groups + groups, *ctr = tiles + ntiles;
    i64 *cls = (i64 *)(cur + groups);
    u64 h[4];
    i64 total = 0, nt = 0, nm = 0, nl = 0;
    rc = rfx_hip_memset(ctx, blk, 0, bytes);
    if (rc == RFX_OK) {
        hipLaunchKernelGGL(k_med_count, dim3(rfx_stream_grid(c, nrows)), dim3(RFX_BLOCK), 0, c->stream, A, (unsigned long long *)off, (unsigned long long *)(ctr + 4));
        hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(RFX_BLOCK), 0, c->stream, off, (i64)(groups + 1), tiles);
        hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(RFX_BLOCK), 0, c->stream, tiles, ntiles, ctr + 3);
        hipLaunchKernelGGL(k_scan_add, dim3(blocks_of(groups + 1, RFX_BLOCK)), dim3(RFX_BLOCK), 0, c->stream, off, (i64)(groups + 1), (const u64 *)tiles);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cur, off, (size_t)groups * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess) {
            rfx_set_error("rfx_hip_group_median: count / scan: %s", hipGetErrorString(e));
            rc = RFX_EHIP;
        }
    }
    if (rc == RFX_OK) rc = rfx_hip_d2h(ctx, &h[0], off + groups, 8);
    total = (i64)h[0];
    if (rc == RFX_OK) rc = rfx_hip_malloc(ctx, &dkeys, (size_t)(total ? total : 1) * 8);
    if (rc == RFX_OK) {
        if (groups <= MED_GLDS) {
            const i64 chunks = (nrows + MED_ROWS_PER_BLOCK - 1) / MED_ROWS_PER_BLOCK;
            int grid = rfx_grid(c) * 4;
            if (chunks < grid) grid = (int)chunks;
            hipLaunchKernelGGL(k_med_scatter_lds, dim3(grid < 1 ? 1 : grid), dim3(RFX_BLOCK), 0, c->stream, A, (unsigned long long *)cur, (u64 *)dkeys);
        } else hipLaunchKernelGGL(k_med_scatter, dim3(rfx_stream_grid(c, nrows)), dim3(RFX_BLOCK), 0, c->stream, A, (unsigned long long *)cur, (u64 *)dkeys);
        const i64 large_cap = total / MED_LDS + 1;
        rc = rfx_hip_malloc(ctx, &dlarge, (size_t)large_cap * 16);
        if (rc == RFX_OK) {
            hipLaunchKernelGGL(k_med_classify, dim3(blocks_of(groups, RFX_BLOCK)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)off, (i64)groups,
                               (unsigned long long *)ctr, cls, (i64 *)dlarge, large_cap);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) {
                rfx_set_error("rfx_hip_group_median: scatter: %s", hipGetErrorString(e));
                rc = RFX_EHIP;
            }
        }
    }
    if (rc == RFX_OK) rc = rfx_hip_d2h(ctx, h, ctr, 3 * 8);
    nt = (i64)h[0];
    nm = (i64)h[1];
    nl = (i64)h[2];
    const u64 *koff = off;
    const unsigned long long *nulls = rule == RFX_MED_SCALAR ? (const unsigned long long *)(ctr + 4) : NULL; // (ranks by the non-null count)
    const u64 *kk = (const u64 *)dkeys;
    if (rc == RFX_OK && nt > 0)
        hipLaunchKernelGGL(k_med_tiny, dim3(capped(blocks_of(nt, RFX_BLOCK / RFX_WAVE), rfx_grid(c) * 8)), dim3(RFX_BLOCK), 0, c->stream, koff, kk, (const i64 *)cls, nt,
                           A.f64, rule, nulls, d_out);
    if (rc == RFX_OK && nm > 0)
        hipLaunchKernelGGL(k_med_lds, dim3(capped(nm, rfx_grid(c) * 4)), dim3(RFX_BLOCK), 0, c->stream, koff, kk, (const i64 *)cls, (i64)groups, nm, A.f64, rule,
                           nulls, d_out);
    const i64 large_cap = total / MED_LDS + 1;
    if (rc == RFX_OK && nl > large_cap) {
        rfx_set_error("rfx_hip_group_median: %lld large segments, room for %lld", (long long)nl, (long long)large_cap);
        rc = RFX_ESTATE;
    }
    if (rc == RFX_OK && nl > 0) {
        // the chunk table of the large segments: (segment, first key) per workgroup of a digit pass (large segments are few: < rows / MED_LDS)
        i64 *hl = (i64 *)malloc((size_t)large_cap * 16), *hoff = hl ? hl + large_cap : NULL;
        void *dst = NULL, *dhist = NULL, *dchunks = NULL;
        i64 nch = 0;
        rc = hl ? rfx_hip_d2h(ctx, hl, dlarge, (size_t)large_cap * 16) : RFX_ENOMEM;
        for (i64 j = 0; j < nl && rc == RFX_OK; j++) nch += (hoff[j] + MED_CHUNK - 1) / MED_CHUNK;
        i64 *ht = rc == RFX_OK ? (i64 *)malloc((size_t)nch * 16) : NULL;
        if (rc == RFX_OK && !ht) rc = RFX_ENOMEM;
        if (rc == RFX_OK) {
            i64 q = 0;
            for (i64 j = 0; j < nl; j++)
                for (i64 a = 0; a < hoff[j]; a += MED_CHUNK, q++) {
                    ht[q] = j;
                    ht[nch + q] = a;
                }
            rc = rfx_hip_malloc(ctx, &dchunks, (size_t)nch * 16);
        }
        if (rc == RFX_OK) rc = rfx_hip_h2d(ctx, dchunks, ht, (size_t)nch * 16);
        if (rc == RFX_OK) rc = rfx_hip_malloc(ctx, &dst, (size_t)nl * sizeof(MedLarge));
        if (rc == RFX_OK) rc = rfx_hip_malloc(ctx, &dhist, (size_t)nl * 512 * 8);
        if (rc == RFX_OK) rc = rfx_hip_memset(ctx, dhist, 0, (size_t)nl * 512 * 8);
        if (rc == RFX_OK) {
            const i64 *cs = (const i64 *)dchunks, *ca = cs + nch;
            hipLaunchKernelGGL(k_med_large_init, dim3(blocks_of(nl, RFX_BLOCK)), dim3(RFX_BLOCK), 0, c->stream, koff, (const i64 *)dlarge, nl, nulls, (MedLarge *)dst);
            for (int shift = 56; shift >= 0; shift -= 8) {
                hipLaunchKernelGGL(k_med_hist, dim3((unsigned)nch), dim3(RFX_BLOCK), 0, c->stream, koff, kk, (const i64 *)dlarge, cs, ca, (const MedLarge *)dst,
                                   (unsigned long long *)dhist, shift);
                hipLaunchKernelGGL(k_med_pick, dim3(blocks_of(nl, RFX_BLOCK)), dim3(RFX_BLOCK), 0, c->stream, (MedLarge *)dst, nl, (unsigned long long *)dhist, shift);
            }
            hipLaunchKernelGGL(k_med_large_out, dim3(blocks_of(nl, RFX_BLOCK)), dim3(RFX_BLOCK), 0, c->stream, koff, (const i64 *)dlarge, nl, (const MedLarge *)dst,
                               A.f64, rule, nulls, d_out);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) {
                rfx_set_error("rfx_hip_group_median: radix select: %s", hipGetErrorString(e));
                rc = RFX_EHIP;
            }
        }
        const int src = rfx_hip_ctx_sync(ctx); // (the chunk table and the histograms are freed below)
        if (rc == RFX_OK) rc = src;
        if (dst) rfx_hip_free(ctx, dst);
        if (dhist) rfx_hip_free(ctx, dhist);
        if (dchunks) rfx_hip_free(ctx, dchunks);
        free(hl);
        free(ht);
    }
    if (rc == RFX_OK) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            rfx_set_error("rfx_hip_group_median: select: %s", hipGetErrorString(e));
            rc = RFX_EHIP;
        }
    }
    const int src = rfx_hip_ctx_sync(ctx); // the scratch below is still read by the select kernels until here
    if (rc == RFX_OK) rc = src;
    if (dlarge) rfx_hip_free(ctx, dlarge);
    if (dkeys) rfx_hip_free(ctx, dkeys);
    rfx_hip_free(ctx, blk);
    return rc;
}

extern "C" int rfx_hip_median(rfx_ctx_t *ctx, const rfx_pred_t *preds, int npred, int logic, const int8_t *d_mask, const int64_t *d_val, int64_t nrows,
                              rfx_value_t *out) {
    RFX_REQUIRE(ctx && out, RFX_EINVAL, "NULL argument");
    rfx_med_rows_t rows;
    memset(&rows, 0, sizeof(rows));
    rows.preds = preds;
    rows.npred = npred;
    rows.logic = logic;
    rows.d_mask = d_mask;
    void *d = NULL;
    int rc = rfx_hip_malloc(ctx, &d, 8);
    if (rc != RFX_OK) return rc;
    double v = 0.0;
    rc = rfx_hip_group_median(ctx, &rows, d_val, RFX_I64, nrows, 1, RFX_MED_SCALAR, (double *)d);
    if (rc == RFX_OK) rc = rfx_hip_d2h(ctx, &v, d, 8);
    rfx_hip_free(ctx, d);
    if (rc != RFX_OK) return rc;
    out->type = RFX_F64;
    out->f = v;
    out->is_null = v != v;
    return RFX_OK;
}

// the sort keys of n values (tests: the device's order against the host restatement)
__global__ __launch_bounds__(RFX_BLOCK) void k_med_keys(const u64 *__restrict__ v, i64 n, int f64, u64 *__restrict__ out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) out[i] = med_key(v[i], f64);
}
extern "C" int rfx_hip_median_keys(rfx_ctx_t *ctx, const void *d_val, int32_t val_type, int64_t n, uint64_t *d_out) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && (n == 0 || (d_val && d_out)), RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(val_type == RFX_I64 || val_type == RFX_F64, RFX_EINVAL, "value type must be i64 or f64");
    if (n <= 0) return RFX_OK;
    hipLaunchKernelGGL(k_med_keys, dim3(rfx_stream_grid(c, n)), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_val, (i64)n, val_type == RFX_F64, (u64 *)d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

__global__ __launch_bounds__(RFX_BLOCK) void k_fill_null(i64 *__restrict__ p, i64 n) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) p[i] = RFX_NULL_I64_D;
}
// the slot table of a dense result's keys: d_table[d_keys[g] - kmin] = g (every other cell null) -- the INDEX_TYPE_SHIFT payload of
// index_group_i64_scoped (core/index.c:2037-2062), built from the groups rather than from the rows
__global__ __launch_bounds__(RFX_BLOCK) void k_key_slots(const i64 *__restrict__ keys, i64 groups, i64 kmin, i64 range, i64 *__restrict__ table) {
    const i64 g = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x;
    if (g >= groups) return;
    const u64 s = (u64)keys[g] - (u64)kmin;
    if (s < (u64)range) table[s] = g;
}
extern "C" int rfx_hip_key_slot_table(rfx_ctx_t *ctx, const int64_t *d_keys, int64_t groups, int64_t kmin, int64_t range, int64_t *d_table) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && range > 0 && d_table && (groups == 0 || d_keys), RFX_EINVAL, "bad argument");
    hipLaunchKernelGGL(k_fill_null, dim3(rfx_stream_grid(c, range)), dim3(RFX_BLOCK), 0, c->stream, (i64 *)d_table, (i64)range);
    if (groups > 0) hipLaunchKernelGGL(k_key_slots, dim3(blocks_of(groups, RFX_BLOCK)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_keys, (i64)groups, (i64)kmin, (i64)range, (i64 *)d_table);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
