// rfx_set.hip -- the kernels behind distinct / find / in / sect / except / union over 8-byte keys.
//
// Reference: index_distinct_i64 (core/index.c:551-607), index_in_i64_i64 (:1291-1361), index_find_i64 (:1507-1574); sect / except are
// filter(x, in(x, y)) (core/items.c:898-948), union is distinct(concat(x, y)) (:1022-1029).  Two routes each, chosen by the planner
// (rfx_exec_set.c) from the key scopes exactly as the reference chooses them:
//
//   dense   k_set_mark        one streaming pass ORs a bit per cell into a bitmap over [kmin, kmin + range)       (distinct, union, the `in` set)
//           k_set_first_dense the same pass with an atomic MIN of the row id into a table of `range` cells        (find)
//   hash    k_set_hash_build  an open-addressed table (this library's own hash, a power of two of slots): key -> first row
//           k_set_prio_insert the REFERENCE's table -- P = next_prime(len / 0.75) cells, home = key % P, linear probing -- rebuilt in parallel:
//                             the sequential layout is the unique one in which every key is preceded, between its home cell and its own, only
//                             by keys of a smaller first row, so "atomic MIN of my first row, carry the displaced larger one on" reproduces it
//   probe   k_set_probe       what every cell of the other operand finds: B8 bytes (in), first rows (find) or one bit per cell (sect / except)
//   emit    k_set_count / k_set_scan / k_set_emit   ordered compaction of a bitmap's set bits: kmin + bit (dense distinct), the key at the row a
//                             cell holds (hash distinct: slot order), or the cell of x itself (sect / except: the VALUES, no id vector, no gather)
//
// Every kernel is a grid-stride streaming pass; the tables are too large for LDS on the hash route and the dense bitmap (<= 128 KB for 2^20
// keys, more when range <= len) is hit through L2 with a test before the atomic, so a column of few distinct keys issues few atomics.
#include "rfx_common.hpp"

#define SET_EMPTY RFX_NULL_I64_D
#define SET_NOBODY RFX_INF_I64_D
#define SET_TILE_BITS ((i64)RFX_BLOCK * 64) // one flag word per thread of a block

__device__ __forceinline__ u64 set_hash(i64 k) { // (murmur3's finaliser: the table order is never observed, only membership and first rows)
    u64 h = (u64)k;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdULL;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ULL;
    h ^= h >> 33;
    return h;
}

// out[0] = min, out[1] = max over all cells, out[2] = min over the non-null cells, out[3] = null cells (out pre-set to the identities)
__global__ __launch_bounds__(RFX_BLOCK) void k_set_scope(const i64 *__restrict__ a, i64 na, const i64 *__restrict__ b, i64 nb, i64 *out) {
    __shared__ i64 s[4][RFX_BLOCK];
    i64 mn = RFX_INF_I64_D, mx = RFX_NULL_I64_D, mnn = RFX_INF_I64_D, nulls = 0;
    const i64 n = na + nb;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 v = i < na ? a[i] : b[i - na];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        if (v == RFX_NULL_I64_D) nulls++;
        else mnn = v < mnn ? v : mnn;
    }
    const int t = threadIdx.x;
    s[0][t] = mn; s[1][t] = mx; s[2][t] = mnn; s[3][t] = nulls;
    __syncthreads();
    for (int w = RFX_BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            s[0][t] = s[0][t + w] < s[0][t] ? s[0][t + w] : s[0][t];
            s[1][t] = s[1][t + w] > s[1][t] ? s[1][t + w] : s[1][t];
            s[2][t] = s[2][t + w] < s[2][t] ? s[2][t + w] : s[2][t];
            s[3][t] += s[3][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        atomicMin((long long *)&out[0], s[0][0]);
        atomicMax((long long *)&out[1], s[1][0]);
        atomicMin((long long *)&out[2], s[2][0]);
        if (s[3][0]) atomicAdd((unsigned long long *)&out[3], (unsigned long long)s[3][0]);
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_set_mark(const i64 *__restrict__ a, i64 na, const i64 *__restrict__ b, i64 nb, i64 kmin, i64 range, u64 *bits) {
    const i64 n = na + nb;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const u64 d = (u64)(i < na ? a[i] : b[i - na]) - (u64)kmin;
        if (d >= (u64)range) continue;
        const u64 m = 1ULL << (d & 63);
        if (!(bits[d >> 6] & m)) atomicOr((unsigned long long *)&bits[d >> 6], m); // (a stale 0 only costs the atomic)
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_set_first_dense(const i64 *__restrict__ x, i64 nx, i64 kmin, i64 range, i64 *first) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < nx; i += (i64)gridDim.x * RFX_BLOCK) {
        const u64 d = (u64)x[i] - (u64)kmin;
        if (d >= (u64)range) continue;
        if (i < first[d]) atomicMin((long long *)&first[d], i);
    }
}

__global__ __launch_bounds__(RFX_BLOCK) void k_set_hash_build(const i64 *__restrict__ a, i64 na, const i64 *__restrict__ b, i64 nb, i64 *keys, i64 *first, i64 capacity) {
    const i64 n = na + nb;
    const u64 mask = (u64)capacity - 1;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 k = i < na ? a[i] : b[i - na];
        if (k == SET_EMPTY) continue;
        u64 s = set_hash(k) & mask;
        for (i64 step = 0; step < capacity; step++, s = (s + 1) & mask) {
            i64 c = keys[s];
            if (c == SET_EMPTY) c = (i64)atomicCAS((unsigned long long *)&keys[s], (unsigned long long)SET_EMPTY, (unsigned long long)k);
            if (c == SET_EMPTY || c == k) {
                if (first && i < first[s]) atomicMin((long long *)&first[s], i);
                break;
            }
        }
    }
}

// -1: not found; else the first row (0 where the structure keeps none)
__device__ __forceinline__ i64 set_find(const rfx_set_lookup_t &S, i64 k) {
    if (S.kind == RFX_SET_ATOM) return k == S.atom ? 0 : -1;
    if (S.kind == RFX_SET_HASH) {
        if (k == SET_EMPTY) return S.null_hit ? 0 : -1;
        const u64 mask = (u64)S.capacity - 1;
        u64 s = set_hash(k) & mask;
        for (i64 step = 0; step < S.capacity; step++, s = (s + 1) & mask) {
            const i64 c = S.d_keys[s];
            if (c == k) return S.d_first ? S.d_first[s] : 0;
            if (c == SET_EMPTY) return -1;
        }
        return -1;
    }
    const u64 d = (u64)k - (u64)S.kmin;
    if (d >= (u64)S.range) return -1;
    if (S.kind == RFX_SET_BITS) return ((S.d_bits[d >> 6] >> (d & 63)) & 1) ? 0 : -1;
    const i64 f = S.d_first[d];
    return f == SET_NOBODY ? -1 : f;
}

// B8, the comparison kernels' scheme (k_cmp_mask, rfx_scalar.hip): a wave owns 512 consecutive cells per step; lane l loads cells 2l, 2l + 1 of each
// 128-cell group (one 16-byte load per group, 1 KB contiguous per wave instruction; two 8-byte loads where q is not 16-byte aligned), looks its
// eight cells up, and the bytes leave TRANSPOSED: the step's eight ballots are wave-uniform words, lane l picks the two that hold cells
// 8l .. 8l + 7 (group l / 16, even and odd cells), spreads four bits of each into bytes and stores 8 bytes -- 512 contiguous bytes per wave
// instruction.  The cells past the last full step are block 0's, byte by byte.
template <bool A16>
__global__ __launch_bounds__(RFX_BLOCK) void k_set_probe_b8(rfx_set_lookup_t S, const i64 *__restrict__ q, i64 n, unsigned char *out) {
    const int lane = threadIdx.x & 63;
    const i64 wave_id = (i64)blockIdx.x * (RFX_BLOCK / RFX_WAVE) + (threadIdx.x >> 6);
    const i64 nwaves = (i64)gridDim.x * (RFX_BLOCK / RFX_WAVE);
    const i64 nfull = n / 512;
    for (i64 w = wave_id; w < nfull; w += nwaves) {
        const i64 base = w * 512 + lane * 2;
        i64 v[8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (A16) {
                const u64x2 t = rfx_ld2((const u64 *)(q + base + j * 128));
                v[2 * j] = (i64)t.x;
                v[2 * j + 1] = (i64)t.y;
            } else {
                v[2 * j] = q[base + j * 128];
                v[2 * j + 1] = q[base + j * 128 + 1];
            }
        }
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) m |= (unsigned)(set_find(S, v[j]) >= 0) << j;
        u64 be = 0, bo = 0; // ballots of the even / odd cells of this lane's OUTPUT group (lane / 16)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 b0 = __ballot((m >> (2 * j)) & 1u), b1 = __ballot((m >> (2 * j + 1)) & 1u);
            const bool mine = (lane >> 4) == j;
            be = mine ? b0 : be;
            bo = mine ? b1 : bo;
        }
        const unsigned sh = 4u * ((unsigned)lane & 15u);
        const unsigned x0 = (unsigned)(be >> sh) & 15u, x1 = (unsigned)(bo >> sh) & 15u; // cells 8l, 8l+2, 8l+4, 8l+6 / 8l+1, ...
        const unsigned lo = (x0 & 1u) | ((x1 & 1u) << 8) | (((x0 >> 1) & 1u) << 16) | (((x1 >> 1) & 1u) << 24);
        const unsigned hi = ((x0 >> 2) & 1u) | (((x1 >> 2) & 1u) << 8) | (((x0 >> 3) & 1u) << 16) | (((x1 >> 3) & 1u) << 24);
        __builtin_nontemporal_store(((u64)hi << 32) | lo, (u64 *)(out + w * 512 + lane * 8));
    }
    if (blockIdx.x == 0)
        for (i64 i = nfull * 512 + threadIdx.x; i < n; i += RFX_BLOCK) out[i] = set_find(S, q[i]) >= 0;
}
__global__ __launch_bounds__(RFX_BLOCK) void k_set_probe_first(rfx_set_lookup_t S, const i64 *__restrict__ q, i64 n, i64 *out) {
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * RFX_BLOCK) {
        const i64 f = set_find(S, q[i]);
        out[i] = f < 0 ? RFX_NULL_I64_D : f;
    }
}
// one bit per cell: every wave stores the ballot of its 64 cells (all lanes of a wave run the same number of rounds)
__global__ __launch_bounds__(RFX_BLOCK) void k_set_probe_flags(rfx_set_lookup_t S, const i64 *__restrict__ q, i64 n, int negate, u64 *flags) {
    const i64 rounded = (n + 63) & ~(i64)63;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < rounded; i += (i64)gridDim.x * RFX_BLOCK) {
        const bool hit = i < n && ((set_find(S, q[i]) >= 0) != (negate != 0));
        const u64 w = __ballot(hit);
        if ((threadIdx.x & 63) == 0) flags[i >> 6] = w;
    }
}
__global__ __launch_bounds__(RFX_BLOCK) void k_set_cells_flags(const i64 *__restrict__ cells, i64 P, u64 *flags) {
    const i64 rounded = (P + 63) & ~(i64)63;
    for (i64 i = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; i < rounded; i += (i64)gridDim.x * RFX_BLOCK) {
        const u64 w = __ballot(i < P && cells[i] != SET_NOBODY);
        if ((threadIdx.x & 63) == 0) flags[i >> 6] = w;
    }
}

// The reference's table, in parallel.  `mine` walks from its key's home cell; a cell keeps the smaller first row, the larger one walks on from the
// next cell (everything between ITS home and here was smaller than it when it passed, and cells only ever decrease).  Distinct keys < P, so an empty
// cell always exists and every walk ends; the step bound only keeps a corrupted table from spinning.
__global__ __launch_bounds__(RFX_BLOCK) void k_set_prio_insert(const i64 *__restrict__ keys, const i64 *__restrict__ first, i64 capacity, i64 P, i64 *cells) {
    for (i64 j = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x; j < capacity; j += (i64)gridDim.x * RFX_BLOCK) {
        const i64 k = keys[j];
        if (k == SET_EMPTY) continue;
        i64 mine = first[j];
        i64 s = (i64)((u64)k % (u64)P);
        for (i64 step = 0; step < 4 * P; step++) {
            const i64 old = atomicMin((long long *)&cells[s], mine);
            if (old == SET_NOBODY) break;
            if (old > mine) mine = old;
            s = s + 1 == P ? 0 : s + 1;
        }
    }
}

// ---- ordered compaction of a bitmap: per tile of 256 words its popcount, one block scans the tile sums, every tile writes at its offset
__global__ __launch_bounds__(RFX_BLOCK) void k_set_count(const u64 *__restrict__ flags, i64 nwords, i64 *scan) {
    __shared__ int s[RFX_BLOCK];
    const i64 w = blockIdx.x * (i64)RFX_BLOCK + threadIdx.x;
    s[threadIdx.x] = w < nwords ? __popcll(flags[w]) : 0;
    __syncthreads();
    for (int h = RFX_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) scan[blockIdx.x] = s[0];
}
// scan[0 .. nt) -> exclusive prefix sums in place, scan[nt] = the total.  One block of 1024 threads, a contiguous chunk each.
__global__ __launch_bounds__(1024) void k_set_scan(i64 *scan, i64 nt) {
    __shared__ i64 s[1024];
    const i64 chunk = (nt + 1023) / 1024, lo = (i64)threadIdx.x * chunk, hi = lo + chunk < nt ? lo + chunk : nt;
    i64 sum = 0;
    for (i64 i = lo; i < hi; i++) sum += scan[i];
    s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 run = 0;
        for (int i = 0; i < 1024; i++) {
            const i64 v = s[i];
            s[i] = run;
            run += v;
        }
        scan[nt] = run;
    }
    __syncthreads();
    i64 run = s[threadIdx.x];
    for (i64 i = lo; i < hi; i++) {
        const i64 v = scan[i];
        scan[i] = run;
        run += v;
    }
}
template <int MODE>
__global__ __launch_bounds__(RFX_BLOCK) void k_set_emit(const u64 *__restrict__ flags, i64 nwords, const i64 *__restrict__ scan, i64 kmin, const i64 *__restrict__ src,
                                                        const i64 *__restrict__ a, i64 na, const i64 *__restrict__ b, i64 cap, i64 *__restrict__ out) {
    __shared__ int s[RFX_BLOCK];
    const int t = threadIdx.x;
    const i64 w = blockIdx.x * (i64)RFX_BLOCK + t;
    u64 word = w < nwords ? flags[w] : 0;
    const int mine = __popcll(word);
    s[t] = mine;
    __syncthreads();
    for (int h = 1; h < RFX_BLOCK; h <<= 1) { // inclusive scan of the 256 popcounts
        const int v = t >= h ? s[t - h] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    i64 pos = scan[blockIdx.x] + s[t] - mine;
    while (word) {
        const i64 i = (w << 6) + __ffsll((long long)word) - 1;
        word &= word - 1;
        if (pos < cap) {
            if (MODE == RFX_SET_EMIT_OFFSET) out[pos] = kmin + i;
            else if (MODE == RFX_SET_EMIT_SRC) out[pos] = src[i];
            else {
                const i64 r = src[i];
                out[pos] = r < na ? a[r] : b[r - na];
            }
        }
        pos++;
    }
}

static int set_grid(rfx_ctx *c, i64 n, int per_cu) {
    const i64 blocks = (n + RFX_BLOCK - 1) / RFX_BLOCK;
    i64 grid = (i64)c->num_cus * per_cu;
    if (blocks < grid) grid = blocks;
    return (int)(grid < 1 ? 1 : grid);
}
static bool pow2(i64 v) { return v > 0 && (v & (v - 1)) == 0; }

extern "C" int rfx_hip_set_scope(rfx_ctx_t *c, const int64_t *d_a, int64_t na, const int64_t *d_b, int64_t nb, int64_t *out4) {
    RFX_REQUIRE(c && out4, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(na >= 0 && nb >= 0 && na + nb > 0 && (na == 0 || d_a) && (nb == 0 || d_b), RFX_EINVAL, "bad spans");
    void *d = NULL;
    int rc = rfx_hip_malloc(c, &d, 32);
    if (rc != RFX_OK) return rc;
    const int64_t init[4] = {RFX_INF_I64_D, RFX_NULL_I64_D, RFX_INF_I64_D, 0};
    if ((rc = rfx_hip_h2d(c, d, init, 32)) == RFX_OK) {
        hipLaunchKernelGGL(k_set_scope, dim3(set_grid(c, na + nb, 8)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_a, (i64)na, (const i64 *)d_b, (i64)nb, (i64 *)d);
        rc = hipGetLastError() == hipSuccess ? rfx_hip_d2h(c, out4, d, 32) : RFX_EHIP;
        if (rc == RFX_EHIP) rfx_set_error("rfx_hip_set_scope: launch failed");
    }
    rfx_hip_free(c, d);
    return rc;
}
extern "C" int rfx_hip_set_mark(rfx_ctx_t *c, const int64_t *d_a, int64_t na, const int64_t *d_b, int64_t nb, int64_t kmin, int64_t range, uint64_t *d_bits) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(na >= 0 && nb >= 0 && (na == 0 || d_a) && (nb == 0 || d_b) && range >= 0, RFX_EINVAL, "bad spans");
    if (na + nb == 0 || range == 0) return RFX_OK;
    RFX_REQUIRE(d_bits, RFX_EINVAL, "NULL bitmap");
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_set_mark, dim3(set_grid(c, na + nb, 8)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_a, (i64)na, (const i64 *)d_b, (i64)nb, (i64)kmin,
                       (i64)range, (u64 *)d_bits);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_set_first_dense(rfx_ctx_t *c, const int64_t *d_x, int64_t nx, int64_t kmin, int64_t range, int64_t *d_first) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(nx >= 0 && range >= 0, RFX_EINVAL, "bad sizes");
    if (nx == 0 || range == 0) return RFX_OK;
    RFX_REQUIRE(d_x && d_first, RFX_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_set_first_dense, dim3(set_grid(c, nx, 8)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_x, (i64)nx, (i64)kmin, (i64)range, (i64 *)d_first);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_set_hash_build(rfx_ctx_t *c, const int64_t *d_a, int64_t na, const int64_t *d_b, int64_t nb, int64_t *d_keys, int64_t *d_first,
                                      int64_t capacity) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    RFX_REQUIRE(na >= 0 && nb >= 0 && (na == 0 || d_a) && (nb == 0 || d_b), RFX_EINVAL, "bad spans");
    RFX_REQUIRE(d_keys && pow2(capacity) && capacity > na + nb, RFX_EINVAL, "capacity must be a power of two above the number of cells");
    if (na + nb == 0) return RFX_OK;
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_set_hash_build, dim3(set_grid(c, na + nb, 8)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_a, (i64)na, (const i64 *)d_b, (i64)nb,
                       (i64 *)d_keys, (i64 *)d_first, (i64)capacity);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_set_probe(rfx_ctx_t *c, const rfx_set_lookup_t *s, const int64_t *d_q, int64_t n, int out_mode, void *d_out) {
    RFX_REQUIRE(c && s, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(n >= 0 && out_mode >= RFX_SET_OUT_B8 && out_mode <= RFX_SET_OUT_NOT_FLAGS, RFX_EINVAL, "bad size or output mode");
    if (n == 0) return RFX_OK;
    RFX_REQUIRE(d_q && d_out, RFX_EINVAL, "NULL argument");
    switch (s->kind) {
    case RFX_SET_BITS: RFX_REQUIRE(s->range >= 0 && (s->range == 0 || s->d_bits), RFX_EINVAL, "bad bitmap"); break;
    case RFX_SET_DENSE_FIRST: RFX_REQUIRE(s->range >= 0 && (s->range == 0 || s->d_first), RFX_EINVAL, "bad first-row table"); break;
    case RFX_SET_HASH: RFX_REQUIRE(s->d_keys && pow2(s->capacity), RFX_EINVAL, "bad hashed table"); break;
    case RFX_SET_ATOM: break;
    default: RFX_REQUIRE(0, RFX_EINVAL, "bad lookup kind");
    }
    RFX_REQUIRE(out_mode != RFX_SET_OUT_B8 || ((uintptr_t)d_out & 7) == 0, RFX_EINVAL, "B8 output must be 8-byte aligned");
    RFX_KERNEL_BEGIN(c);
    if (out_mode == RFX_SET_OUT_B8) {
        const unsigned grid = set_grid(c, (n + 7) >> 3, 8); /* (a thread answers eight cells of a step) */
        if (((uintptr_t)d_q & 15) == 0) hipLaunchKernelGGL(k_set_probe_b8<true>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, *s, (const i64 *)d_q, (i64)n, (unsigned char *)d_out);
        else hipLaunchKernelGGL(k_set_probe_b8<false>, dim3(grid), dim3(RFX_BLOCK), 0, c->stream, *s, (const i64 *)d_q, (i64)n, (unsigned char *)d_out);
    } else if (out_mode == RFX_SET_OUT_FIRST)
        hipLaunchKernelGGL(k_set_probe_first, dim3(set_grid(c, n, 8)), dim3(RFX_BLOCK), 0, c->stream, *s, (const i64 *)d_q, (i64)n, (i64 *)d_out);
    else
        hipLaunchKernelGGL(k_set_probe_flags, dim3(set_grid(c, n, 8)), dim3(RFX_BLOCK), 0, c->stream, *s, (const i64 *)d_q, (i64)n,
                           (int)(out_mode == RFX_SET_OUT_NOT_FLAGS), (u64 *)d_out);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_set_priority_insert(rfx_ctx_t *c, const int64_t *d_keys, const int64_t *d_first, int64_t capacity, int64_t P, int64_t *d_cells) {
    RFX_REQUIRE(c && d_keys && d_first && d_cells, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(pow2(capacity) && P > 0 && P < ((int64_t)1 << 60), RFX_EINVAL, "bad table sizes");
    RFX_KERNEL_BEGIN(c);
    hipLaunchKernelGGL(k_set_prio_insert, dim3(set_grid(c, capacity, 8)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_keys, (const i64 *)d_first, (i64)capacity, (i64)P,
                       (i64 *)d_cells);
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_set_cells_flags(rfx_ctx_t *c, const int64_t *d_cells, int64_t P, uint64_t *d_flags) {
    RFX_REQUIRE(c, RFX_EINVAL, "ctx is NULL");
    if (P <= 0) return RFX_OK;
    RFX_REQUIRE(d_cells && d_flags, RFX_EINVAL, "NULL argument");
    hipLaunchKernelGGL(k_set_cells_flags, dim3(set_grid(c, P, 8)), dim3(RFX_BLOCK), 0, c->stream, (const i64 *)d_cells, (i64)P, (u64 *)d_flags);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
extern "C" int rfx_hip_set_compact(rfx_ctx_t *c, const uint64_t *d_flags, int64_t nbits, int mode, int64_t kmin, const int64_t *d_src, const int64_t *d_a, int64_t na,
                                   const int64_t *d_b, int64_t *d_scan, int64_t cap, int64_t *d_out, int64_t *count) {
    RFX_REQUIRE(c && count, RFX_EINVAL, "NULL argument");
    *count = 0;
    RFX_REQUIRE(nbits >= 0 && cap >= 0 && mode >= RFX_SET_EMIT_OFFSET && mode <= RFX_SET_EMIT_ROWKEY, RFX_EINVAL, "bad size or mode");
    if (nbits == 0) return RFX_OK;
    RFX_REQUIRE(d_flags && d_scan, RFX_EINVAL, "NULL argument");
    RFX_REQUIRE(mode == RFX_SET_EMIT_OFFSET || d_src, RFX_EINVAL, "this mode reads d_src");
    RFX_REQUIRE(mode != RFX_SET_EMIT_ROWKEY || (na >= 0 && (na == 0 || d_a)), RFX_EINVAL, "this mode reads the key spans");
    const i64 nwords = (nbits + 63) >> 6, nt = (nwords + RFX_BLOCK - 1) / RFX_BLOCK;
    RFX_REQUIRE(nt < ((i64)1 << 31), RFX_ELIMIT, "too many tiles for one grid");
    hipLaunchKernelGGL(k_set_count, dim3((unsigned)nt), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_flags, nwords, (i64 *)d_scan);
    hipLaunchKernelGGL(k_set_scan, dim3(1), dim3(1024), 0, c->stream, (i64 *)d_scan, nt);
    RFX_HIP_CHECK(hipGetLastError());
    int64_t total = 0;
    int rc = rfx_hip_d2h(c, &total, d_scan + nt, 8);
    if (rc != RFX_OK) return rc;
    *count = total;
    if (total > cap) {
        rfx_set_error("rfx_hip_set_compact: %lld set bits, room for %lld", (long long)total, (long long)cap);
        return RFX_ELIMIT;
    }
    if (total == 0) return RFX_OK;
    RFX_REQUIRE(d_out, RFX_EINVAL, "NULL output");
    RFX_KERNEL_BEGIN(c);
#define SET_EMIT(M)                                                                                                                                             \
    hipLaunchKernelGGL(k_set_emit<M>, dim3((unsigned)nt), dim3(RFX_BLOCK), 0, c->stream, (const u64 *)d_flags, nwords, (const i64 *)d_scan, (i64)kmin, (const i64 *)d_src, \
                       (const i64 *)d_a, (i64)na, (const i64 *)d_b, (i64)cap, (i64 *)d_out)
    if (mode == RFX_SET_EMIT_OFFSET) SET_EMIT(RFX_SET_EMIT_OFFSET);
    else if (mode == RFX_SET_EMIT_SRC) SET_EMIT(RFX_SET_EMIT_SRC);
    else SET_EMIT(RFX_SET_EMIT_ROWKEY);
#undef SET_EMIT
    RFX_KERNEL_END(c);
    RFX_HIP_CHECK(hipGetLastError());
    return RFX_OK;
}
