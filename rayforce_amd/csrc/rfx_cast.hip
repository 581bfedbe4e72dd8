// rfx_cast.hip -- `as` over vectors of the nine numeric and temporal types (ray_cast_obj, core/compose.c:42-68 -> cast_obj's vector arms,
// core/rayforce.c:2558-2752): one plain C cast per cell, nulls not carried.  One streaming kernel templated over (source cell class x destination cell
// class), no LDS: a lane owns a run of consecutive cells per step, long enough that the narrow side is one 16-byte access and the wide side whole 16-byte
// accesses too (f64 -> u8: eight loads, sixteen results packed into one store); no lane stores a byte or a short outside the last partial run.
#include "rfx_common.hpp"

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// source cell classes: what a cell is read as; destination classes: what is stored
enum { SC_U8, SC_I16, SC_I32, SC_I32W, SC_I64, SC_F64 }; // (_I32W: 4-byte cells held as their widened 8-byte image, rfx_hip_widen_i32: the null's promotion undone)
enum { DC_1, DC_2, DC_4, DC_8, DC_F64 };
template <int SC> struct SrcBytes { static const int v = SC == SC_U8 ? 1 : (SC == SC_I16 ? 2 : (SC == SC_I32 ? 4 : 8)); };
template <int DC> struct DstBytes { static const int v = DC == DC_1 ? 1 : (DC == DC_2 ? 2 : (DC == DC_4 ? 4 : 8)); };
// cells of a lane's run: sixteen bytes of the narrower side, four cells at the least
template <int SC, int DC> struct Run {
    static const int narrow = SrcBytes<SC>::v < DstBytes<DC>::v ? SrcBytes<SC>::v : DstBytes<DC>::v;
    static const int v = 16 / narrow < 4 ? 4 : 16 / narrow;
};

// a source cell as 64 bits: an integer cell its value (u8 zero-extended, the others sign-extended), an f64 cell its bits
template <int SC> __device__ __forceinline__ u64 cast_widen(u64 raw) {
    if (SC == SC_U8) return raw & 0xFF;
    if (SC == SC_I16) return (u64)(i64)(short)raw;
    if (SC == SC_I32) return (u64)(i64)(int)raw;
    if (SC == SC_I32W) return (i64)raw == RFX_NULL_I64_D ? (u64)(i64)RFX_NULL_I32_D : raw;
    return raw;
}
// cell j of a run held as the dwords it was loaded as
template <int SC> __device__ __forceinline__ u64 cast_pick(const unsigned *w, int j) {
    if (SC == SC_U8) return cast_widen<SC>(w[j / 4] >> (8 * (j % 4)));
    if (SC == SC_I16) return cast_widen<SC>(w[j / 2] >> (16 * (j % 2)));
    if (SC == SC_I32) return cast_widen<SC>(w[j]);
    return cast_widen<SC>(((u64)w[2 * j + 1] << 32) | w[2 * j]);
}
template <int SC> __device__ __forceinline__ u64 cast_ld1(const void *p, i64 r) {
    if (SC == SC_U8) return cast_widen<SC>(((const unsigned char *)p)[r]);
    if (SC == SC_I16) return cast_widen<SC>(((const unsigned short *)p)[r]);
    if (SC == SC_I32) return cast_widen<SC>(((const unsigned *)p)[r]);
    return cast_widen<SC>(((const u64 *)p)[r]);
}
// the cast itself; the result's low DstBytes bytes are the cell (the store truncates: low byte, low 16 bits, low 32 bits)
template <int SC, int DC> __device__ __forceinline__ u64 cast_cell(u64 v) {
    if (SC == SC_F64) {
        if (DC == DC_F64) return v;
        const double x = rfx_as_f64(v);
        if (DC == DC_8) return (u64)rfx_f64_to_i64_x86(x);
        return (u64)(i64)rfx_f64_to_i32_x86(x); // I16 / U8 / B8: the 32-bit conversion, then its low bits
    }
    if (DC == DC_F64) return rfx_as_u64(SC == SC_I64 ? (double)(i64)v : (double)(int)v);
    return v;
}
template <int DC> __device__ __forceinline__ void cast_put(unsigned *w, int j, u64 v) {
    if (DC == DC_1) w[j / 4] |= ((unsigned)v & 0xFFu) << (8 * (j % 4));
    else if (DC == DC_2) w[j / 2] |= ((unsigned)v & 0xFFFFu) << (16 * (j % 2));
    else if (DC == DC_4) w[j] = (unsigned)v;
    else { w[2 * j] = (unsigned)v; w[2 * j + 1] = (unsigned)(v >> 32); }
}
template <int DC> __device__ __forceinline__ void cast_st1(void *p, i64 r, u64 v) {
    if (DC == DC_1) ((unsigned char *)p)[r] = (unsigned char)v;
    else if (DC == DC_2) ((unsigned short *)p)[r] = (unsigned short)v;
    else if (DC == DC_4) ((unsigned *)p)[r] = (unsigned)v;
    else ((u64 *)p)[r] = v;
}

// runs of Run<SC, DC>::v cells grid-strided, then the cells of the last partial run one by one
template <int SC, int DC>
__global__ __launch_bounds__(RFX_BLOCK) void k_cast(const void *__restrict__ src, i64 n, void *__restrict__ dst) {
    constexpr int R = Run<SC, DC>::v, NL = R * SrcBytes<SC>::v / 16, NS = R * DstBytes<DC>::v / 16;
    const i64 tid = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x, nt = (i64)gridDim.x * RFX_BLOCK, nr = n / R;
    for (i64 g = tid; g < nr; g += nt) {
        unsigned in[NL * 4], out[NS * 4];
        const v4u *s = (const v4u *)src + g * NL;
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const v4u t = __builtin_nontemporal_load(s + k);
            in[4 * k] = t.x; in[4 * k + 1] = t.y; in[4 * k + 2] = t.z; in[4 * k + 3] = t.w;
        }
#pragma unroll
        for (int k = 0; k < NS * 4; k++) out[k] = 0;
#pragma unroll
        for (int j = 0; j < R; j++) cast_put<DC>(out, j, cast_cell<SC, DC>(cast_pick<SC>(in, j)));
        v4u *d = (v4u *)dst + g * NS;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            v4u t;
            t.x = out[4 * k]; t.y = out[4 * k + 1]; t.z = out[4 * k + 2]; t.w = out[4 * k + 3];
            __builtin_nontemporal_store(t, d + k);
        }
    }
    for (i64 r = nr * R + tid; r < n; r += nt) cast_st1<DC>(dst, r, cast_cell<SC, DC>(cast_ld1<SC>(src, r)));
}
template <int SC, int DC>
static int cast_launch(rfx_ctx *c, const void *src, i64 n, void *dst) {
    i64 blocks = (n / Run<SC, DC>::v + RFX_BLOCK - 1) / RFX_BLOCK;
    int grid = rfx_grid(c);
    if (blocks < 1) blocks = 1;
    if (blocks < grid) grid = (int)blocks;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL((k_cast<SC, DC>), dim3(grid), dim3(RFX_BLOCK), 0, c->stream, src, n, dst);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}

// the reference's type codes -> cell classes (-1: not one of the nine)
static int cast_src_class(int t) {
    switch (t) {
        case RFX_CAST_B8: case RFX_CAST_U8: return SC_U8;
        case RFX_CAST_I16: return SC_I16;
        case RFX_CAST_I32: case RFX_CAST_DATE: case RFX_CAST_TIME: return SC_I32;
        case RFX_CAST_I64: case RFX_CAST_TIMESTAMP: return SC_I64;
        case RFX_CAST_F64: return SC_F64;
        default: return -1;
    }
}
static int cast_dst_class(int t) {
    switch (t) {
        case RFX_CAST_B8: case RFX_CAST_U8: return DC_1;
        case RFX_CAST_I16: return DC_2;
        case RFX_CAST_I32: case RFX_CAST_DATE: case RFX_CAST_TIME: return DC_4;
        case RFX_CAST_I64: case RFX_CAST_TIMESTAMP: return DC_8;
        case RFX_CAST_F64: return DC_F64;
        default: return -1;
    }
}
extern "C" int rfx_hip_cast_arm(int32_t src_type, int32_t dst_type) {
    const int st = src_type & ~RFX_CAST_WIDENED;
    const int sc = cast_src_class(st), dc = cast_dst_class(dst_type);
    if (sc < 0 || dc < 0 || st == dst_type) return 0; // (the same type is clone_obj: no cast runs)
    if ((src_type & RFX_CAST_WIDENED) && sc != SC_I32) return 0;
    if (sc == SC_U8 && dc == DC_1) return 0; // B8 <-> U8: cast_obj has no such case (its type error)
    return 1;
}
extern "C" int rfx_hip_cast(rfx_ctx_t *ctx, int32_t src_type, int32_t dst_type, const void *d_src, int64_t n, void *d_dst) {
    rfx_ctx *c = (rfx_ctx *)ctx;
    RFX_REQUIRE(c && n >= 0, RFX_EINVAL, "bad argument");
    RFX_REQUIRE(rfx_hip_cast_arm(src_type, dst_type), RFX_EINVAL, "the reference has no cast between these vector types");
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_src && d_dst && d_src != d_dst && ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 15) == 0, RFX_EINVAL, "16-byte aligned device buffers, the output one of its own, expected");
    const int sc = (src_type & RFX_CAST_WIDENED) ? SC_I32W : cast_src_class(src_type), dc = cast_dst_class(dst_type);
#define ARM(S, D) case (S) * 8 + (D): return cast_launch<S, D>(c, d_src, (i64)n, d_dst);
#define ARMS_INT(S) ARM(S, DC_1) ARM(S, DC_2) ARM(S, DC_4) ARM(S, DC_8) ARM(S, DC_F64)
    switch (sc * 8 + dc) {
        ARM(SC_U8, DC_2) ARM(SC_U8, DC_4) ARM(SC_U8, DC_8) ARM(SC_U8, DC_F64)
        ARM(SC_I16, DC_1) ARM(SC_I16, DC_4) ARM(SC_I16, DC_8) ARM(SC_I16, DC_F64)
        ARMS_INT(SC_I32)
        ARMS_INT(SC_I32W)
        ARMS_INT(SC_I64)
        ARM(SC_F64, DC_1) ARM(SC_F64, DC_2) ARM(SC_F64, DC_4) ARM(SC_F64, DC_8)
        default: break;
    }
#undef ARMS_INT
#undef ARM
    RFX_REQUIRE(0, RFX_EINVAL, "the reference has no cast between these vector types");
    return RFX_EINVAL;
}
