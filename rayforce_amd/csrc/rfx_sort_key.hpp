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
