// rfx_sort_key.hpp -- the sort key the radix sort (rfx_sort.hip) orders by and the merge of sorted runs (rfx_merge.hip) compares by: ONE function,
// so that a merged order can never differ from a sorted one.
// core/sort.c:266-285,311 -- the medians' key (rfx_median.hip): i64 x ^ 2^63; f64 NaN -> 0, negative -> ~bits, else bits | 2^63.
// A descending sort orders by ~key, so ties keep their ascending row order exactly as an ascending sort's do (core/sort.c:584-616).
#pragma once
#include "rfx_common.hpp"

__device__ __forceinline__ u64 sort_key(u64 x, int f64, int desc) {
    u64 k;
    if (!f64) k = x ^ 0x8000000000000000ULL;
    else if ((x & 0x7FFFFFFFFFFFFFFFULL) > 0x7FF0000000000000ULL) k = 0ULL; // NaN (either sign, any payload)
    else k = (x & 0x8000000000000000ULL) ? ~x : (x | 0x8000000000000000ULL);
    return desc ? ~k : k;
}

// ---- keys of at most 32 bits (core/sort.c:183-263,481-559: B8 / U8 by the unsigned byte, I16 / I32 / DATE / TIME by signed value) ----
// Source classes: what a cell is read as.  SK_I32W: a 4-byte column held as its widened 8-byte image (rfx_hip_widen_i32: NULL_I32 -> NULL_I64).
// The key occupies the low sort_key32_bytes() bytes; descending is the complement WITHIN that width, so the bytes above stay zero and ties keep
// their ascending row order.  INT32_MIN -- the null -- is key 0: first ascending, last descending.
enum { SK_U8 = 0, SK_I16 = 1, SK_I32 = 2, SK_I32W = 3 };
__host__ __device__ __forceinline__ constexpr int sort_key32_bytes(int cls) { return cls == SK_U8 ? 1 : (cls == SK_I16 ? 2 : 4); }
__host__ __device__ __forceinline__ constexpr int sort_src32_bytes(int cls) { return cls == SK_U8 ? 1 : (cls == SK_I16 ? 2 : (cls == SK_I32 ? 4 : 8)); }

__device__ __forceinline__ unsigned int sort_key32(u64 raw, int cls, int desc) {
    unsigned int k, full;
    if (cls == SK_U8) k = (unsigned int)raw & 0xFFu, full = 0xFFu;
    else if (cls == SK_I16) k = ((unsigned int)raw & 0xFFFFu) ^ 0x8000u, full = 0xFFFFu;
    else if (cls == SK_I32) k = (unsigned int)raw ^ 0x80000000u, full = 0xFFFFFFFFu;
    else k = ((i64)raw == RFX_NULL_I64_D) ? 0u : ((unsigned int)raw ^ 0x80000000u), full = 0xFFFFFFFFu;
    return desc ? k ^ full : k;
}
// the cell a key came from, in the column's own width (the low sort_key32_bytes() bytes): from the key alone, the null included
__device__ __forceinline__ unsigned int sort_cell32(unsigned int k, int cls, int desc) {
    if (cls == SK_U8) return desc ? k ^ 0xFFu : k;
    if (cls == SK_I16) return (desc ? k ^ 0xFFFFu : k) ^ 0x8000u;
    return (desc ? ~k : k) ^ 0x80000000u;
}
