// rfx_concat.hip -- concat (ray_concat, core/compose.c:465-823) and raze (ray_raze, core/compose.c:1096-1164) of plain vectors: S source spans of
// cells of one width laid end to end into one output, in ONE launch for any S; the table form does that for up to RFX_MAX_COLS columns per launch.
//   the span table   per column the prefix sums of the spans' BYTES (S + 1 cells) and their source addresses (S cells), every column's descriptor in
//                    front, uploaded for the call into a block of the context's pool.  Empty spans are dropped on the host (the prefix sums ascend
//                    strictly); an atom's cell bits sit in the table itself and its span points there, so the kernel knows bytes and nothing else.
//   the kernel       a workgroup owns one CC_TILE-byte tile of one column's output and finds the spans that overlap it by two binary searches over the
//                    prefix sums (wave-uniform).  A thread moves whole 16-byte accesses at 16-byte-aligned OUTPUT addresses.  Inside one span: source
//                    16-byte aligned -> one 16-byte load; else the two aligned 16-byte words around it, shifted together, when both lie inside the span;
//                    else -- the first and last accesses of a span, an access that crosses spans, the output's tail -- byte by byte, every byte from
//                    its own span, stored as the whole access when all 16 bytes are the output's, byte by byte at the tail.  Nothing is read outside
//                    a span or written outside the output.
#include "rfx_cells.hpp"

#define CC_UNROLL 4                           /* 16-byte accesses per thread */
#define CC_TILE (RFX_BLOCK * 16 * CC_UNROLL)  /* bytes of output per workgroup: 16 KB */

struct cc_col {
    const i64 *pref;          // S + 1 ascending byte offsets, pref[0] = 0, pref[S] = total
    const u64 *src;           // S source addresses
    unsigned char *out;       // 16-byte aligned
    i64 total;                // bytes
    i64 nspans;               // S >= 1
    i64 tile0;                // the column's first tile in the launch's grid
};

// the span holding output byte b (pref[s] <= b < pref[s + 1]) among spans [lo, hi]
__device__ __forceinline__ i64 cc_find(const i64 *__restrict__ pref, i64 lo, i64 hi, i64 b) {
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (pref[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(RFX_BLOCK) void k_concat_spans(const cc_col *__restrict__ cols, int ncols) {
    // which column's tile (ncols <= RFX_MAX_COLS: a walk)
    int k = 0;
    while (k + 1 < ncols && (i64)blockIdx.x >= cols[k + 1].tile0) k++;
    const i64 *__restrict__ pref = cols[k].pref;
    const u64 *__restrict__ src = cols[k].src;
    unsigned char *__restrict__ out = cols[k].out;
    const i64 total = cols[k].total;
    const i64 t0 = ((i64)blockIdx.x - cols[k].tile0) * (i64)CC_TILE;
    const i64 t1 = t0 + CC_TILE < total ? t0 + CC_TILE : total; // the tile is output bytes [t0, t1), t0 < total
    const i64 s_first = cc_find(pref, 0, cols[k].nspans - 1, t0);
    const i64 s_last = pref[s_first + 1] >= t1 ? s_first : cc_find(pref, s_first, cols[k].nspans - 1, t1 - 1);
#pragma unroll
    for (int u = 0; u < CC_UNROLL; u++) {
        const i64 b = t0 + ((i64)u * RFX_BLOCK + threadIdx.x) * 16;
        if (b >= t1) continue;
        i64 s = s_first == s_last ? s_first : cc_find(pref, s_first, s_last, b);
        const i64 p0 = pref[s], p1 = pref[s + 1];
        const bool whole = b + 16 <= total;
        if (whole && b + 16 <= p1) { // the access lies inside span s
            const u64 a = src[s] + (u64)(b - p0);
            const u64 k16 = a & 15;
            if (k16 == 0) {
                __builtin_nontemporal_store(__builtin_nontemporal_load((const rfx_v2q *)a), (rfx_v2q *)(out + b));
                continue;
            }
            const u64 a0 = a - k16;
            if (a0 >= src[s] && a0 + 32 <= src[s] + (u64)(p1 - p0)) { // both aligned words are the span's own
                const rfx_v2q lo = __builtin_nontemporal_load((const rfx_v2q *)a0), hi = __builtin_nontemporal_load((const rfx_v2q *)(a0 + 16));
                const bool up = k16 >= 8;
                const u64 w0 = up ? lo.y : lo.x, w1 = up ? hi.x : lo.y, w2 = up ? hi.y : hi.x;
                const unsigned sh = (unsigned)(k16 & 7) * 8;
                rfx_v2q o;
                o.x = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
                o.y = sh ? (w1 >> sh) | (w2 << (64 - sh)) : w1;
                __builtin_nontemporal_store(o, (rfx_v2q *)(out + b));
                continue;
            }
        }
        // byte by byte: every byte from the span it belongs to
        u64 lo = 0, hi = 0;
        const int nb = whole ? 16 : (int)(total - b);
        i64 q0 = p0, q1 = p1;
        const unsigned char *sp = (const unsigned char *)src[s];
        for (int j = 0; j < nb; j++) {
            const i64 at = b + j;
            while (at >= q1) { // (spans are never empty: at most one step per byte)
                s++;
                q0 = q1;
                q1 = pref[s + 1];
                sp = (const unsigned char *)src[s];
            }
            const u64 v = sp[at - q0];
            if (j < 8) lo |= v << (8 * j);
            else hi |= v << (8 * (j - 8));
        }
        if (whole) {
            rfx_v2q o;
            o.x = lo; o.y = hi;
            *(rfx_v2q *)(out + b) = o;
        } else {
            for (int j = 0; j < nb; j++) out[b + j] = (unsigned char)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFF);
        }
    }
}

extern "C" int rfx_hip_concat_cols(rfx_ctx_t *c, const rfx_concat_col_t *cols, int ncols) {
    RFX_REQUIRE(c && cols, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(ncols >= 1 && ncols <= RFX_MAX_COLS, RFX_EINVAL, "1 .. RFX_MAX_COLS columns per launch");
    // the table's size: per column with cells its descriptor, S + 1 prefix sums, S addresses, one cell per atom
    size_t words = 0;
    int live = 0;
    for (int k = 0; k < ncols; k++) {
        const rfx_concat_col_t *col = &cols[k];
        RFX_REQUIRE(rfx_width_ok(col->width), RFX_EINVAL, "a cell width that is not 1, 2, 4 or 8 bytes");
        RFX_REQUIRE(col->nspans >= 0 && (col->nspans == 0 || col->spans), RFX_EINVAL, "NULL span list");
        i64 s_live = 0, atoms = 0, cells = 0;
        for (i64 s = 0; s < col->nspans; s++) {
            const rfx_span_t *sp = &col->spans[s];
            RFX_REQUIRE(sp->cells >= 0 && (sp->d_ptr || sp->cells <= 1), RFX_EINVAL, "a span without an address that is not one atom");
            RFX_REQUIRE(!sp->d_ptr || ((uintptr_t)sp->d_ptr & (uintptr_t)(col->width - 1)) == 0, RFX_EINVAL, "a span that is not cell-aligned");
            if (!sp->cells) continue;
            RFX_REQUIRE(sp->cells <= (INT64_MAX >> 5) - cells, RFX_ELIMIT, "cells");
            cells += sp->cells;
            s_live++;
            atoms += sp->d_ptr == NULL;
        }
        if (!cells) continue;
        RFX_REQUIRE(col->d_out && ((uintptr_t)col->d_out & 15) == 0, RFX_EINVAL, "NULL result, or one that is not 16-byte aligned");
        words += sizeof(cc_col) / 8 + (size_t)(2 * s_live + 1 + atoms);
        live++;
    }
    if (!live) return RFX_OK;
    const size_t bytes = words * 8;
    u64 *h = (u64 *)malloc(bytes);
    RFX_REQUIRE(h, RFX_ENOMEM, "out of host memory");
    void *d_tab = NULL;
    const int rc = rfx_hip_malloc(c, &d_tab, bytes);
    if (rc != RFX_OK) {
        free(h);
        return rc;
    }
    const u64 base = (u64)(uintptr_t)d_tab;
    cc_col *desc = (cc_col *)h;
    size_t at = (size_t)live * (sizeof(cc_col) / 8);
    i64 tiles = 0;
    int d = 0;
    for (int k = 0; k < ncols; k++) {
        const rfx_concat_col_t *col = &cols[k];
        i64 s_live = 0, atoms = 0;
        for (i64 s = 0; s < col->nspans; s++)
            if (col->spans[s].cells) s_live++, atoms += col->spans[s].d_ptr == NULL;
        if (!s_live) continue;
        i64 *pref = (i64 *)(h + at);
        u64 *src = h + at + (size_t)s_live + 1, *atom = src + s_live;
        i64 j = 0, na = 0, off = 0;
        for (i64 s = 0; s < col->nspans; s++) {
            const rfx_span_t *sp = &col->spans[s];
            if (!sp->cells) continue;
            pref[j] = off;
            if (sp->d_ptr) src[j] = (u64)(uintptr_t)sp->d_ptr;
            else { // (little endian: the cell is the slot's low bytes)
                atom[na] = sp->bits;
                src[j] = base + (u64)((unsigned char *)&atom[na] - (unsigned char *)h);
                na++;
            }
            off += sp->cells * col->width;
            j++;
        }
        pref[j] = off;
        desc[d].pref = (const i64 *)(uintptr_t)(base + at * 8);
        desc[d].src = (const u64 *)(uintptr_t)(base + (at + (size_t)s_live + 1) * 8);
        desc[d].out = (unsigned char *)col->d_out;
        desc[d].total = off;
        desc[d].nspans = s_live;
        desc[d].tile0 = tiles;
        tiles += (off + CC_TILE - 1) / CC_TILE;
        at += (size_t)(2 * s_live + 1 + atoms);
        d++;
    }
    if (tiles > 0x7FFFFFFFLL) {
        free(h);
        rfx_hip_free(c, d_tab);
        RFX_REQUIRE(0, RFX_ELIMIT, "more output tiles than one grid holds");
    }
    rfx_ctx_device_written(c);
    hipError_t e = hipMemcpyAsync(d_tab, h, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (the table has left the host block)
    free(h);
    if (e == hipSuccess) {
        RFX_KERNEL_BEGIN(c);
        hipLaunchKernelGGL(k_concat_spans, dim3((unsigned)tiles), dim3(RFX_BLOCK), 0, c->stream, (const cc_col *)d_tab, live);
        RFX_KERNEL_END(c);
        e = hipGetLastError();
    }
    rfx_hip_free(c, d_tab); // (back to the context's pool: whoever takes the block next writes it on this stream, after the kernel)
    RFX_HIP_CHECK(e);
    return RFX_OK;
}

extern "C" int rfx_hip_concat(rfx_ctx_t *c, const rfx_span_t *spans, int64_t nspans, int32_t width, void *d_out) {
    rfx_concat_col_t col;
    col.spans = spans;
    col.nspans = nspans;
    col.width = width;
    col.d_out = d_out;
    return rfx_hip_concat_cols(c, &col, 1);
}
