// rfx_cells.hpp -- what the column-moving kernel files share: cells of 1, 2, 4 and 8 bytes, the streaming grid, the one rule for writes to device
// memory.  Host-compiled files only: NOT one of the headers hiprtc compiles plan kernels from.
#pragma once
#include "rfx_common.hpp"

typedef u64 rfx_v2q __attribute__((ext_vector_type(2))); // one 16-byte access

template <int WID> __device__ __forceinline__ u64 rfx_cell_get(const unsigned char *__restrict__ in, i64 j) {
    if (WID == 8) return ((const u64 *)in)[j];
    if (WID == 4) return ((const unsigned *)in)[j];
    if (WID == 2) return ((const unsigned short *)in)[j];
    return in[j];
}
template <int WID> __device__ __forceinline__ void rfx_cell_put(unsigned char *__restrict__ out, i64 j, u64 v) {
    if (WID == 8) ((u64 *)out)[j] = v;
    else if (WID == 4) ((unsigned *)out)[j] = (unsigned)v;
    else if (WID == 2) ((unsigned short *)out)[j] = (unsigned short)v;
    else out[j] = (unsigned char)v;
}
static inline bool rfx_width_ok(int w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// the grid of a grid-stride kernel over `threads` items: one thread each, at most four resident grids, never empty
static inline int rfx_stream_grid(const rfx_ctx *c, i64 threads) {
    const i64 blocks = (threads + RFX_BLOCK - 1) / RFX_BLOCK, cap = (i64)rfx_grid(c) * 4;
    return (int)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

// Device memory is about to be written (an upload, a memset, a verb's result): every planner memo goes.  rfx_ctx.hip.
void rfx_ctx_device_written(rfx_ctx *c);
