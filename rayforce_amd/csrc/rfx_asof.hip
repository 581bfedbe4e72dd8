// rfx_asof.hip -- the binary searches behind asof-join, bin and binr.
//
// Reference: asof-join (ray_asof_join, core/join.c:300-356) asks index_asof_join_obj (core/index.c:3194-3267) for, per LEFT row, a right row of
// the same equality-key tuple: the right rows of a tuple are kept as a list of row ids in ascending ROW order, and index_bin_i64
// (core/index.c:3121-3137) runs a closed-interval binary search over that list by time -- last probe position with rt[ids[mid]] <= lt[i].  The
// list is not sorted by time and nobody checks that it is: on unsorted times the answer is whatever this probe sequence lands on, so the
// sequence of `mid` values is the contract.  bin / binr (ray_bin / ray_binr, core/items.c:1399-1644) are the same loop over a whole vector by
// position (bin: last probe with x[mid] <= y, none = -1; binr: first probe with x[mid] >= y, none = len x).
//
//   k_asof_runs     from the group ids of the right rows in stable group order (equal ids adjacent), per group [start, end) -- written at
//                   the group's id, which is the group's FIRST right row: exactly what the equi-join index hands a left row
//   k_seg_search    one query per lane: its segment (a group's [start, end), or the whole array), then the reference's loop over ONE
//                   contiguous time array -- a chain of ~log2(len) dependent 8-byte loads -- and the answer mapped back to a row id
//
// The search is latency-bound: nothing is staged in LDS, the kernels hold a handful of registers and every wave slot of a CU is usable.
#include "rfx_common.hpp"

// seg[2 * g] = first position of group g's run in gs[], seg[2 * g + 1] = one past its last; cells of ids that head no group are never written
// (and never read: a query's group id is a group's first row or null).
__global__ __launch_bounds__(RFX_BLOCK) void k_asof_runs(const i64 *__restrict__ gs, i64 n, i64 *__restrict__ seg) {
    for (i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; j < n; j += (i64)gridDim.x * RFX_BLOCK) {
        const i64 g = gs[j];
        if ((u64)g >= (u64)n) continue; // (cannot happen: group ids are rows of this table)
        if (j == 0 || gs[j - 1] != g) seg[2 * g] = j;
        if (j == n - 1 || gs[j + 1] != g) seg[2 * g + 1] = j + 1;
    }
}

// RIGHT = 0: idx = last probe position with t[mid] <= q (asof, bin); RIGHT = 1: first probe position with t[mid] >= q (binr).
// group (optional): per query the id of its segment in seg[] (null: no segment -> `none`); without it every query searches t[0 .. len).
// rows (optional): position -> row id.  `none` is written as it is; a found position p is written as rows ? rows[p] : p - segment start.
// group and out may be the same array (cell i is read, then written, by the one lane that owns query i).
template <int RIGHT>
__global__ __launch_bounds__(RFX_BLOCK) void k_seg_search(const i64 *__restrict__ q, i64 n, const i64 *group, i64 ngroups, const i64 *__restrict__ seg,
                                                          i64 len, const i64 *__restrict__ t, const i64 *__restrict__ rows, i64 none, i64 *out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 y = q[i];
        i64 base = 0, left = 0, right = len - 1, idx = -1;
        if (group) {
            const i64 g = group[i];
            right = -1;
            if ((u64)g < (u64)ngroups) { // (a null id is negative: outside)
                base = seg[2 * g];
                right = seg[2 * g + 1] - base - 1;
            }
        }
        const i64 *__restrict__ ts = t + base;
        while (left <= right) {
            const i64 mid = left + ((right - left) >> 1);
            const i64 v = ts[mid];
            if (RIGHT ? (v >= y) : (v <= y)) {
                idx = mid;
                if (RIGHT) right = mid - 1;
                else left = mid + 1;
            } else {
                if (RIGHT) left = mid + 1;
                else right = mid - 1;
            }
        }
        out[i] = idx < 0 ? none : (rows ? rows[base + idx] : idx);
    }
}

static int asof_grid(rfx_ctx *c, i64 n, int per_cu) {
    const i64 blocks = (n + RFX_BLOCK - 1) / RFX_BLOCK;
    i64 grid = (i64)c->num_cus * per_cu;
    if (blocks < grid) grid = blocks;
    return (int)grid;
}

extern "C" int rfx_hip_asof_runs(rfx_ctx_t *c, const int64_t *d_sorted_groups, int64_t n, int64_t *d_seg) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    if (n <= 0) return RFX_OK;
    RFX_REQUIRE(d_sorted_groups && d_seg, RFX_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_asof_runs, dim3(asof_grid(c, n, 16)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_sorted_groups, (i64)n, (i64 *)d_seg);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

extern "C" int rfx_hip_seg_search(rfx_ctx_t *c, const int64_t *d_q, int64_t n, const int64_t *d_group, int64_t ngroups, const int64_t *d_seg, int64_t len,
                                  const int64_t *d_t, const int64_t *d_rows, int right, int64_t none, int64_t *d_out) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    if (n <= 0) return RFX_OK;
    RFX_REQUIRE(d_q && d_out, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(d_group ? (d_seg && ngroups >= 0 && (d_t || ngroups == 0)) : (len >= 0 && (d_t || len == 0)), RFX_EINVAL, "bad segment description");
    RFX_REQUIRE(d_q != d_out && (const int64_t *)d_t != d_out, RFX_EINVAL, "d_out may alias d_group only");
    // 8 blocks of 4 waves per CU: all 32 wave slots of a CU, which is what hides a chain of dependent loads
    const int grid = asof_grid(c, n, 8);
    if (right)
        hipLaunchKernelGGL(k_seg_search<1>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_q, (i64)n, (const i64 *)d_group, (i64)ngroups,
                           (const i64 *)d_seg, (i64)len, (const i64 *)d_t, (const i64 *)d_rows, (i64)none, (i64 *)d_out);
    else
        hipLaunchKernelGGL(k_seg_search<0>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_q, (i64)n, (const i64 *)d_group, (i64)ngroups,
                           (const i64 *)d_seg, (i64)len, (const i64 *)d_t, (const i64 *)d_rows, (i64)none, (i64 *)d_out);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
