// What the whole-graph miners share (gv_mine_scores in k_mine.hip, gv_transe_mine in k_transe_mine.hip): the ordered key, the
// filter re-bucketed per (subject tile, object tile) -- count, scan, fill: three small kernels, integer atomics -- the per-relation
// filter words of a 64 x 64 tile pair, and the EMIT / HIST epilogues.  A workgroup of either miner is 256 threads on one 64 x 64 tile
// pair; a candidate is (local row rl, local column cl) of it.
#pragma once
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace gv {

constexpr int MINE_FL_CAP = 1024;      // listed triplets of a tile pair kept in LDS (the rest is read from memory)
constexpr int MINE_HIST_BITS = 12;
constexpr int MINE_REL_BITS = 19;      // packed filter entry: relation << 12 | local subject << 6 | local object

// the key of gv_topk_scores' order (k_gemm.hip: topk_key), logit part
__device__ __forceinline__ unsigned mine_key(float x) {
    unsigned u = __float_as_uint(x);
    if (x != x) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float mine_key_logit(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// ---- the filter, re-bucketed per (subject tile, object tile): count, scan, fill ------------------------------------------
struct MineFiltParams {
    const int* lo;
    const int* hi;
    const int* ent;
    int n_ent, n, num_rels, o_tiles;
    int* cnt;                  // [tiles]: counts, then the fill cursors
    int* ptr;                  // [tiles + 1]
    unsigned* out;             // [n_ent]
};

template <bool FILL>
__global__ __launch_bounds__(256) void k_mine_filt(const MineFiltParams f) {
    const long long keys = (long long)f.n * f.num_rels;
    for (long long key = (long long)blockIdx.x * 256 + threadIdx.x; key < keys; key += (long long)gridDim.x * 256) {
        const int lo = min(max(f.lo[key], 0), f.n_ent), hi = min(max(f.hi[key], lo), f.n_ent);
        if (lo == hi) continue;
        const int s = (int)(key / f.num_rels), r = (int)(key - (long long)s * f.num_rels);
        for (int j = lo; j < hi; ++j) {
            const int o = f.ent[j];
            if (o < 0 || o >= f.n) continue;
            const int tile = (s >> 6) * f.o_tiles + (o >> 6);
            if (!FILL) atomicAdd(f.cnt + tile, 1);
            else {
                const int pos = atomicAdd(f.cnt + tile, 1);
                if (pos >= 0 && pos < f.n_ent) f.out[pos] = ((unsigned)r << 12) | ((unsigned)(s & 63) << 6) | (unsigned)(o & 63);
            }
        }
    }
}

// exclusive scan of the tile counts (one workgroup: a thread sums a contiguous slice, the slices are scanned in LDS)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_mine_filt_scan(int* cnt, int* ptr, int tiles) {
    __shared__ int part[THREADS];
    const int t = threadIdx.x;
    const int per = (tiles + THREADS - 1) / THREADS;
    const int i0 = min(t * per, tiles), i1 = min(i0 + per, tiles);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < THREADS; ++i) { const int v = part[i]; part[i] = run; run += v; }
        ptr[tiles] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int i = i0; i < i1; ++i) {
        const int v = cnt[i];
        ptr[i] = run;
        cnt[i] = run;          // the fill cursor
        run += v;
    }
}

inline int64_t mine_align16(int64_t b) { return (b + 15) / 16 * 16; }

// bytes of the re-bucketed filter of an n-entity table with n_filt_ent listed objects (0 for an empty table)
inline int64_t mine_filter_workspace_bytes(int n, int n_filt_ent) {
    if (n <= 0 || n_filt_ent < 0) return 0;
    const int64_t tiles = (int64_t)((n + 63) / 64) * ((n + 63) / 64);
    return mine_align16(tiles * 4) + mine_align16((tiles + 1) * 4) + mine_align16((int64_t)(n_filt_ent > 0 ? n_filt_ent : 1) * 4);
}

// the three launches; *tile_ptr [tiles + 1] and *tile_ent then point into the workspace.  false: a launch could not be queued.
inline bool mine_filter_rebucket(const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int n,
                                 int num_rels, void* workspace, hipStream_t st, const int** tile_ptr, const unsigned** tile_ent) {
    const int tiles_1d = (n + 63) / 64, tiles = tiles_1d * tiles_1d;
    char* ws = (char*)workspace;
    MineFiltParams f{};
    f.lo = filt_lo; f.hi = filt_hi; f.ent = filt_ent; f.n_ent = n_filt_ent; f.n = n; f.num_rels = num_rels; f.o_tiles = tiles_1d;
    f.cnt = (int*)ws;
    f.ptr = (int*)(ws + mine_align16((int64_t)tiles * 4));
    f.out = (unsigned*)(ws + mine_align16((int64_t)tiles * 4) + mine_align16((int64_t)(tiles + 1) * 4));
    if (fill_words(f.cnt, 0u, (size_t)tiles * 4, st) != hipSuccess) return false;
    const long long keys = (long long)n * num_rels;
    const unsigned fb = (unsigned)std::min<long long>((keys + 255) / 256, 65535);
    hipLaunchKernelGGL(k_mine_filt<false>, dim3(fb), dim3(256), 0, st, f);
    hipLaunchKernelGGL(k_mine_filt_scan<1024>, dim3(1), dim3(1024), 0, st, f.cnt, f.ptr, tiles);
    hipLaunchKernelGGL(k_mine_filt<true>, dim3(fb), dim3(256), 0, st, f);
    *tile_ptr = f.ptr; *tile_ent = f.out;
    return true;
}

// ---- device side: a workgroup's share of the re-bucketed filter ---------------------------------------------------------------
// its range of tile_ent, the first MINE_FL_CAP entries copied into flist (visible after the caller's next barrier)
__device__ __forceinline__ void mine_filter_load(const int* tile_ptr, const unsigned* tile_ent, int tile, unsigned* flist, int t,
                                                 int* f_base, int* f_cnt) {
    *f_base = 0; *f_cnt = 0;
    if (tile_ptr) {
        *f_base = tile_ptr[tile];
        *f_cnt = tile_ptr[tile + 1] - *f_base;
        for (int i = t; i < min(*f_cnt, MINE_FL_CAP); i += 256) flist[i] = tile_ent[*f_base + i];
    }
}

// relation r's listed objects per subject row -> mask [64] (zeroed before, behind a barrier), *any set when there is one
__device__ __forceinline__ void mine_filter_relation(const unsigned* flist, const unsigned* tile_ent, int f_base, int f_cnt, int r,
                                                     int t, unsigned long long* mask, int* any) {
    for (int i = t; i < f_cnt; i += 256) {
        const unsigned ent = i < MINE_FL_CAP ? flist[i] : tile_ent[f_base + i];
        if ((int)(ent >> 12) == r) {
            atomicOr(&mask[(ent >> 6) & 63u], 1ull << (ent & 63u));
            *any = 1;
        }
    }
}

// ---- device side: the two epilogues -------------------------------------------------------------------------------------------
// EMIT, called by every lane of a wave together: one wave-aggregated integer atomicAdd reserves the slots of the lanes with `ok`,
// (s, r, o, value bits) go out as one 16-byte store while the slot is below the capacity; the counter keeps counting.
__device__ __forceinline__ void mine_emit(bool ok, int lane, int s, int r, int o, int value_bits, int4* out, long long capacity,
                                          unsigned long long* counter) {
    const unsigned long long m = __ballot(ok);
    if (m) {
        const int leader = __builtin_ctzll(m);
        unsigned long long base = 0ull;
        if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
        const unsigned blo = (unsigned)__shfl((int)(unsigned)base, leader);
        const unsigned bhi = (unsigned)__shfl((int)(unsigned)(base >> 32), leader);
        base = ((unsigned long long)bhi << 32) | blo;
        if (ok) {
            const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (slot < (unsigned long long)capacity) out[slot] = make_int4(s, r, o, value_bits);
        }
    }
}

// HIST: the workgroup's LDS histogram into the global one (after a barrier)
__device__ __forceinline__ void mine_hist_flush(const unsigned* hist_s, unsigned long long* hist, unsigned bin_mask, int t) {
    for (int i = t; i <= (int)bin_mask; i += 256) {
        const unsigned c = hist_s[i];
        if (c) atomicAdd(hist + i, (unsigned long long)c);
    }
}

}  // namespace gv
