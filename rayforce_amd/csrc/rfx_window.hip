// rfx_window.hip -- window-join / window-join1: per left row the window's rows of its key group, then every aggregate of a value column.
//
// Reference: __window_join (core/join.c:358-489) sorts the right table by (keys, time) -- jtab --, keeps per key tuple its first and last row
// [fi, ti] of jtab (index_window_join_obj, core/index.c:3269-3347), and every aggregate's INDEX_TYPE_WINDOW arm (AGGR_ITER, core/aggr.c:133-160;
// aggr_avg_partial, core/aggr.c:1545-1578) runs two binary searches over jtab's time cells T[fi .. ti] (core/aggr.c:39-71, both starting from
// idx = 0, so "nothing qualified" is fi) and folds rows li .. ri in order:
//     ri = last position with T <= hi;   li = last position with T <= lo (window-join)  |  first position with T >= lo (window-join1)
//     null row when there is no group, T[li] > hi, or (window-join1) T[ri] < lo
// T is read as 32-bit cells there; here the times and the window bounds are the widened cells (NULL_I32 -> NULL_I64, else sign-extended), an
// order isomorphism, so the 64-bit comparisons below answer what the 32-bit ones answer.
//
//   k_window_ranges   one left row per lane: its group's segment, the two searches, the null tests -> (li, ri) as positions of the sorted right
//                     table, (-1, -2) for a null row; per wave the number of windows longer than RFX_WINDOW_LANE_MAX and the longest one
//   k_window_fold     one launch per value column, every aggregate at once.  A wave owns `rpw` consecutive left rows: a lane folds its own row
//                     when the window has at most RFX_WINDOW_LANE_MAX cells; the longer windows are folded one after the other by the whole
//                     wave -- 16-byte loads, four cells per lane and step -- and reduced with wave shuffles.
//
// Order of addition: I64 sums wrap, so any order gives the reference's bits (unless a PARTIAL sum of the reference's order happens to equal
// NULL_I64, which it then keeps: not replayed).  F64 sums -- and the f64 sum behind avg, of I64 columns too: the reference adds (f64)cell in row
// order (core/aggr.c:1569-1574), so past 2^53 its chain rounds -- are a tree here and a chain there: equal when the additions are exact, else within
// rounding.  min / max compare values, so +0.0 against -0.0 may pick the other zero than the reference's chain does.
#include "rfx_common.hpp"

#define RFX_WINDOW_LANE_MAX 16

template <int CLOSED>
__global__ __launch_bounds__(RFX_BLOCK) void k_window_ranges(const i64 *__restrict__ lo, const i64 *__restrict__ hi, i64 n, const i64 *__restrict__ group,
                                                             i64 ngroups, const i64 *__restrict__ seg, const i64 *__restrict__ t, i64 *__restrict__ li_out,
                                                             i64 *__restrict__ ri_out, u64 *__restrict__ stats) {
    // (whole waves walk the loop together: the ballot below wants every lane of a wave present)
    const i64 nround = (n + RFX_WAVE - 1) / RFX_WAVE * RFX_WAVE;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < nround; i += (i64)gridDim.x * RFX_BLOCK) {
        i64 li = -1, ri = -2;
        if (i < n) {
            const i64 g = group[i];
            if ((u64)g < (u64)ngroups) { // (a null id is negative: no group)
                const i64 fi = seg[2 * g], len = seg[2 * g + 1] - fi;
                if (len > 0) {
                    const i64 kl = lo[i], kr = hi[i];
                    const i64 *__restrict__ ts = t + fi;
                    i64 left = 0, right = len - 1, r = 0, l = 0;
                    while (left <= right) { // indexr_bin_i32_(kr, ...)
                        const i64 mid = left + ((right - left) >> 1);
                        if (ts[mid] <= kr) { r = mid; left = mid + 1; }
                        else right = mid - 1;
                    }
                    left = 0, right = len - 1;
                    while (left <= right) {
                        const i64 mid = left + ((right - left) >> 1);
                        if (CLOSED) { // indexl_bin_i32_(kl, ...)
                            if (ts[mid] < kl) left = mid + 1;
                            else { l = mid; right = mid - 1; }
                        } else { // indexr_bin_i32_(kl, ...)
                            if (ts[mid] <= kl) { l = mid; left = mid + 1; }
                            else right = mid - 1;
                        }
                    }
                    if (!(ts[l] > kr || (CLOSED && ts[r] < kl))) { li = fi + l; ri = fi + r; }
                }
            }
            li_out[i] = li;
            ri_out[i] = ri;
        }
        const i64 len = li < 0 ? 0 : ri - li + 1;
        const u64 nlong = (u64)__popcll(__ballot(len > RFX_WINDOW_LANE_MAX));
        u64 mx = (u64)(len > 0 ? len : 0);
        for (int m = 32; m; m >>= 1) { const u64 o = rfx_shfl_xor_u64(mx, m); mx = o > mx ? o : mx; }
        if ((threadIdx.x & (RFX_WAVE - 1)) == 0 && mx) {
            if (nlong) atomicAdd((unsigned long long *)&stats[0], (unsigned long long)nlong);
            atomicMax((unsigned long long *)&stats[1], (unsigned long long)mx);
        }
    }
}

__device__ __forceinline__ u64 window_shfl_u64(u64 v, int src) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl(lo, src, 64);
    hi = __shfl(hi, src, 64);
    return ((u64)hi << 32) | lo;
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------------
template <typename T> struct wtype;
template <> struct wtype<i64> {
    static constexpr bool is_int = true;
    static __device__ __forceinline__ bool null(i64 v) { return v == RFX_NULL_I64_D; }
    static __device__ __forceinline__ i64 min0() { return RFX_INF_I64_D; }  // aggr_min_partial starts at INF_I64: all cells null -> INF_I64
    static __device__ __forceinline__ i64 max0() { return RFX_NULL_I64_D; } // aggr_max_partial starts at NULL_I64: all cells null -> NULL_I64
    static __device__ __forceinline__ u64 bits(i64 v) { return (u64)v; }
    static __device__ __forceinline__ i64 from(u64 b) { return (i64)b; }
    static __device__ __forceinline__ u64 nullbits() { return (u64)RFX_NULL_I64_D; }
};
template <> struct wtype<double> {
    static constexpr bool is_int = false;
    static __device__ __forceinline__ bool null(double v) { return v != v; }
    static __device__ __forceinline__ double min0() { return __longlong_as_double((i64)RFX_PINF_BITS); }           // INF_F64
    static __device__ __forceinline__ double max0() { return __longlong_as_double((i64)0xFFF0000000000000ULL); }   // (only read when a cell is not NaN)
    static __device__ __forceinline__ u64 bits(double v) { return (u64)__double_as_longlong(v); }
    static __device__ __forceinline__ double from(u64 b) { return __longlong_as_double((i64)b); }
    static __device__ __forceinline__ u64 nullbits() { return RFX_NAN_BITS; }
};

template <typename T> struct wacc {
    i64 isum;    // wrapping sum of the non-null cells (I64 columns)
    double fsum; // sum of the non-null cells as f64: avg of both types, sum of F64
    i64 cnt;     // non-null cells
    T mn, mx;
    i64 first, last; // positions of the first / last non-null cell
    __device__ __forceinline__ void init() {
        isum = 0; fsum = 0.0; cnt = 0;
        mn = wtype<T>::min0(); mx = wtype<T>::max0();
        first = RFX_INF_I64_D; last = -1;
    }
    __device__ __forceinline__ void add(T v, i64 pos) {
        if (wtype<T>::null(v)) return;
        if constexpr (wtype<T>::is_int) isum += (i64)v;
        fsum += (double)v;
        cnt++;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        first = pos < first ? pos : first;
        last = pos > last ? pos : last;
    }
    __device__ __forceinline__ void wave_reduce() {
        for (int m = 32; m; m >>= 1) {
            isum += (i64)rfx_shfl_xor_u64((u64)isum, m);
            fsum += __longlong_as_double((i64)rfx_shfl_xor_u64((u64)__double_as_longlong(fsum), m));
            cnt += (i64)rfx_shfl_xor_u64((u64)cnt, m);
            const T omn = wtype<T>::from(rfx_shfl_xor_u64(wtype<T>::bits(mn), m)), omx = wtype<T>::from(rfx_shfl_xor_u64(wtype<T>::bits(mx), m));
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            const i64 of = (i64)rfx_shfl_xor_u64((u64)first, m), ol = (i64)rfx_shfl_xor_u64((u64)last, m);
            first = of < first ? of : first;
            last = ol > last ? ol : last;
        }
    }
};

struct wouts { u64 *sum, *mn, *mx; i64 *cnt; double *avg; u64 *first, *last; };

// one row's answers from its accumulator.  li < 0: the null row -- count 0, every other aggregate the type's null.
template <typename T>
__device__ __forceinline__ void window_store(const wouts &o, i64 row, i64 li, i64 ri, const wacc<T> &a, const T *__restrict__ v) {
    const u64 nul = wtype<T>::nullbits();
    const bool isnull = li < 0;
    const i64 len = isnull ? 0 : ri - li + 1;
    constexpr bool is_i64 = wtype<T>::is_int;
    if (o.cnt) o.cnt[row] = len; // (counts every row of the window, nulls too)
    if (o.avg) o.avg[row] = (isnull || a.cnt == 0) ? __longlong_as_double((i64)RFX_NAN_BITS) : a.fsum / (double)a.cnt;
    // ADDI64 / ADDF64 propagate a null cell
    if (o.sum) o.sum[row] = (isnull || a.cnt < len) ? nul : (is_i64 ? (u64)a.isum : (u64)__double_as_longlong(a.fsum));
    if (o.mn) o.mn[row] = isnull ? nul : wtype<T>::bits(a.mn);
    // MAXF64(NaN, y) = y and `if (ISNANF64(out)) out = in`: over NaN cells only, max and first end as the LAST cell's own NaN
    const u64 allnull = (is_i64 || len <= 0) ? nul : wtype<T>::bits(v[isnull ? 0 : ri]);
    if (o.mx) o.mx[row] = isnull ? nul : (a.cnt ? wtype<T>::bits(a.mx) : allnull);
    if (o.first) o.first[row] = isnull ? nul : (a.cnt ? wtype<T>::bits(v[a.first]) : allnull);
    if (o.last) o.last[row] = (isnull || !a.cnt) ? nul : wtype<T>::bits(v[a.last]);
}

// v[0 .. nv): the value column in the sorted right table's order.  rpw (a power of two <= 64) rows per wave.
template <typename T>
__global__ __launch_bounds__(RFX_BLOCK) void k_window_fold(const T *__restrict__ v, i64 nv, const i64 *__restrict__ li_in, const i64 *__restrict__ ri_in, i64 n,
                                                           int rpw, wouts o) {
    typedef T v2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & (RFX_WAVE - 1);
    const i64 nwaves = (n + rpw - 1) / rpw;
    for (i64 w = blockIdx.x * (i64)(RFX_BLOCK / RFX_WAVE) + (threadIdx.x >> 6); w < nwaves; w += (i64)gridDim.x * (RFX_BLOCK / RFX_WAVE)) {
        const i64 row = w * rpw + lane;
        const bool mine = lane < rpw && row < n;
        i64 li = -1, ri = -2;
        if (mine) { li = li_in[row]; ri = ri_in[row]; }
        if (li >= 0 && (ri >= nv || ri < li - 1)) { li = -1; ri = -2; } // (cannot happen: positions of this table)
        const i64 len = li < 0 ? 0 : ri - li + 1;
        if (mine && len <= RFX_WINDOW_LANE_MAX) {
            wacc<T> a;
            a.init();
            for (i64 p = li; p <= ri; p++) a.add(v[p], p);
            window_store<T>(o, row, li, ri, a, v);
        }
        u64 todo = __ballot(mine && len > RFX_WINDOW_LANE_MAX);
        while (todo) {
            const int j = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const i64 L = (i64)window_shfl_u64((u64)li, j), R = (i64)window_shfl_u64((u64)ri, j);
            wacc<T> a;
            a.init();
            // pairs at even positions: 16-byte aligned loads (the column starts on an allocation boundary); two pairs per lane and step, both
            // loads issued before either is folded
            for (i64 p = (L & ~(i64)1) + 2 * lane; p <= R; p += 4 * RFX_WAVE) {
                const i64 q = p + 2 * RFX_WAVE;
                T x0, x1, y0 = 0, y1 = 0;
                if (p + 1 < nv) {
                    const v2 t = *(const v2 *)(v + p);
                    x0 = t.x; x1 = t.y;
                } else {
                    x0 = v[p]; x1 = x0; // (p <= R < nv; the cell after the column's last is never folded)
                }
                if (q <= R) {
                    if (q + 1 < nv) {
                        const v2 t = *(const v2 *)(v + q);
                        y0 = t.x; y1 = t.y;
                    } else {
                        y0 = v[q]; y1 = y0;
                    }
                }
                if (p >= L) a.add(x0, p);
                if (p + 1 <= R) a.add(x1, p + 1);
                if (q <= R) a.add(y0, q);
                if (q + 1 <= R) a.add(y1, q + 1);
            }
            a.wave_reduce();
            if (lane == j) window_store<T>(o, w * rpw + j, L, R, a, v);
        }
    }
}

static int window_grid(rfx_ctx *c, i64 blocks, int per_cu) {
    i64 grid = (i64)c->num_cus * per_cu;
    if (blocks < grid) grid = blocks;
    return (int)(grid < 1 ? 1 : grid);
}

extern "C" int rfx_hip_window_ranges(rfx_ctx_t *c, const int64_t *d_lo, const int64_t *d_hi, int64_t n, const int64_t *d_group, int64_t ngroups,
                                     const int64_t *d_seg, const int64_t *d_t, int closed, int64_t *d_li, int64_t *d_ri, uint64_t *d_stats) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    if (n <= 0) return RFX_OK;
    RFX_REQUIRE(d_lo && d_hi && d_group && d_li && d_ri && d_stats && ngroups >= 0 && (ngroups == 0 || (d_seg && d_t)), RFX_EINVAL, "NULL argument");
    // 8 blocks of 4 waves per CU: every wave slot, to hide the chains of dependent loads
    const int grid = window_grid(c, (n + RFX_BLOCK - 1) / RFX_BLOCK, 8);
    if (closed)
        hipLaunchKernelGGL(k_window_ranges<1>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_lo, (const i64 *)d_hi, (i64)n, (const i64 *)d_group,
                           (i64)ngroups, (const i64 *)d_seg, (const i64 *)d_t, (i64 *)d_li, (i64 *)d_ri, (u64 *)d_stats);
    else
        hipLaunchKernelGGL(k_window_ranges<0>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_lo, (const i64 *)d_hi, (i64)n, (const i64 *)d_group,
                           (i64)ngroups, (const i64 *)d_seg, (const i64 *)d_t, (i64 *)d_li, (i64 *)d_ri, (u64 *)d_stats);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_window_fold(rfx_ctx_t *c, const void *d_vals, int32_t type, int64_t nvals, const int64_t *d_li, const int64_t *d_ri, int64_t n,
                                   int64_t long_windows, void *const *d_outs) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    if (n <= 0) return RFX_OK;
    RFX_REQUIRE(d_li && d_ri && d_outs && nvals >= 0 && (d_vals || nvals == 0), RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(type == RFX_I64 || type == RFX_F64, RFX_EINVAL, "value columns are I64 or F64");
    RFX_REQUIRE(((uintptr_t)d_vals & 15) == 0, RFX_EINVAL, "the value column is not 16-byte aligned");
    wouts o;
    o.sum = (u64 *)d_outs[RFX_WAGG_SUM]; o.mn = (u64 *)d_outs[RFX_WAGG_MIN]; o.mx = (u64 *)d_outs[RFX_WAGG_MAX]; o.cnt = (i64 *)d_outs[RFX_WAGG_COUNT];
    o.avg = (double *)d_outs[RFX_WAGG_AVG]; o.first = (u64 *)d_outs[RFX_WAGG_FIRST]; o.last = (u64 *)d_outs[RFX_WAGG_LAST];
    // rows per wave: 64 while every window is a lane's; with long windows as few as it takes to give every wave slot of the device a wave
    int rpw = RFX_WAVE;
    if (long_windows > 0)
        while (rpw > 1 && (n + rpw - 1) / rpw < (i64)c->num_cus * 32) rpw >>= 1;
    const i64 nwaves = (n + rpw - 1) / rpw;
    const int grid = window_grid(c, (nwaves + 3) / 4, 8);
    if (type == RFX_I64)
        hipLaunchKernelGGL(k_window_fold<i64>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_vals, (i64)nvals, (const i64 *)d_li, (const i64 *)d_ri, (i64)n,
                           rpw, o);
    else
        hipLaunchKernelGGL(k_window_fold<double>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const double *)d_vals, (i64)nvals, (const i64 *)d_li, (const i64 *)d_ri,
                           (i64)n, rpw, o);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
