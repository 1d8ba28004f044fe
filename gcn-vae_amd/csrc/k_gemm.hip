// K2/K4: dense fp32 GEMM on the gfx950 f32 MFMA (v_mfma_f32_32x32x2_f32).
//
//   C[M,N] = act( op(A)[M,K] @ op(B)[K,N] + bias[N] ) (+ C)
//
// The MFMA result is bit-for-bit a k-ordered fp32 fma chain (no reduced-precision path exists on
// gfx950), so parity with the CPU reference is at fp32 rounding.  Block tile 128x64x16, four waves
// in a 2x2 grid, each wave owns a 64x32 patch = two 32x32 accumulators.  Operands are staged
// through LDS k-major (As[k][m], Bs[k][n], +1 padding) so that the MFMA operand read -- lane l
// needs A[m = l&31][k = l>>5] and B[k = l>>5][n = l&31] -- is a conflict-free ds_read_b32 for both
// 32-lane halves.  Global loads of tile t+1 are issued before the MFMAs of tile t (register
// staging); the shapes on this path are skinny (K = N = 200..400, M = nodes), so the kernel is
// sized for many small blocks rather than for a 256^2 pipeline.
// split-K (grid.z) writes raw partial tiles to a workspace that a second kernel sums in order.
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "k_riders.h"
#include "k_mc.h"
#include "k_query_args.h"
#include "k_topk.h"

namespace gv {


typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmParams {
    const float* a;
    const float* b;
    float* c;
    const float* bias;
    const float* a_mask;   // optional, same layout as A: A is read as (a_mask > 0 ? A : 0)  (ReLU backward folded in)
    float* ws;
    int m, n, k, lda, ldb, ldc;
    int act, accumulate, split_k, k_chunk;
    int vec_a, vec_b;
    const int* rows_dev;   // optional device scalar: only the first *rows_dev rows of the stored A exist (padding of a static-shape batch)
    // B known to be zero in whole blocks (an autoregressive mask folded into the weights): per 64-column tile of C one word, bit c set =
    // B holds non-zero entries in k-chunk c (16 wide); chunks with a clear bit are not loaded and not multiplied (BK = 16, no split-K)
    const unsigned long long* kmask;
    // C known to be zero in whole 64 x 64 tiles (the weight gradient of such a layer): bit (i * tmask_ld + j) set = tile (i, j) is wanted;
    // other tiles are stored as zeros (nothing when accumulating) without reading A or B
    const unsigned long long* tmask;
    int tmask_ld;
    int tmask_wanted;      // > 0 (split-K only): the launch holds ONE block row per wanted tile -- block x is the x-th set bit of tmask
};

// guarded load of VPT consecutive floats (VPT % 4 == 0) along the contiguous dimension; `lim` bounds that
// dimension, `ok` says the other coordinate is inside the matrix
template <int VPT>
__device__ __forceinline__ void load_run(const float* src, int pos, int lim, bool ok, bool vec, float (&r)[VPT], int off) {
#pragma unroll
    for (int h = 0; h < VPT / 4; ++h) {
        const int q = pos + 4 * h;
        if (ok && vec && q + 3 < lim) {
            const float4 v = *reinterpret_cast<const float4*>(src + 4 * h);
            r[off + 4 * h] = v.x; r[off + 4 * h + 1] = v.y; r[off + 4 * h + 2] = v.z; r[off + 4 * h + 3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[off + 4 * h + i] = (ok && q + i < lim) ? src[4 * h + i] : 0.f;
        }
    }
}

// the same run of the mask matrix zeroes the entries whose mask value is not positive
template <int VPT>
__device__ __forceinline__ void mask_run(const float* msk, int pos, int lim, bool ok, bool vec, float (&r)[VPT]) {
    float mv[VPT];
    load_run<VPT>(msk, pos, lim, ok, vec, mv, 0);
#pragma unroll
    for (int i = 0; i < VPT; ++i) r[i] = mv[i] > 0.f ? r[i] : 0.f;
}

// ---- global -> registers: BM*BK/256 floats of A and BN*BK/256 floats of B per thread, zero outside the matrix
template <bool TA, int BM, int BK>
__device__ __forceinline__ void load_a(const GemmParams& p, int m0, int k0, int kend, float (&r)[BM * BK / 256]) {
    constexpr int APT = BM * BK / 256;
    const int t = threadIdx.x;
    if constexpr (!TA) {               // A is [M, K], K contiguous: BK/APT threads per row
        constexpr int TPR = BK / APT;
        const int m = m0 + t / TPR, kk = k0 + (t % TPR) * APT;
        load_run<APT>(p.a + (size_t)m * p.lda + kk, kk, kend, m < p.m, p.vec_a, r, 0);
        if (p.a_mask) mask_run<APT>(p.a_mask + (size_t)m * p.lda + kk, kk, kend, m < p.m, p.vec_a, r);
    } else {                           // A is stored [K, M], M contiguous: BM/APT threads per k
        constexpr int TPK = BM / APT;
        const int kq = k0 + t / TPK, m = m0 + (t % TPK) * APT;
        load_run<APT>(p.a + (size_t)kq * p.lda + m, m, p.m, kq < kend, p.vec_a, r, 0);
        if (p.a_mask) mask_run<APT>(p.a_mask + (size_t)kq * p.lda + m, m, p.m, kq < kend, p.vec_a, r);
    }
}

template <bool TB, int BN, int BK>
__device__ __forceinline__ void load_b(const GemmParams& p, int n0, int k0, int kend, float (&r)[BN * BK / 256]) {
    constexpr int BPT = BN * BK / 256;
    const int t = threadIdx.x;
    if constexpr (!TB) {               // B is [K, N], N contiguous: BN/BPT threads per k
        constexpr int TPK = BN / BPT;
        const int kq = k0 + t / TPK, n = n0 + (t % TPK) * BPT;
        load_run<BPT>(p.b + (size_t)kq * p.ldb + n, n, p.n, kq < kend, p.vec_b, r, 0);
    } else {                           // B is stored [N, K], K contiguous: BK/BPT threads per n
        constexpr int TPN = BK / BPT;
        const int n = n0 + t / TPN, kq = k0 + (t % TPN) * BPT;
        load_run<BPT>(p.b + (size_t)n * p.ldb + kq, kq, kend, n < p.n, p.vec_b, r, 0);
    }
}

template <bool TA, int BM, int BK>
__device__ __forceinline__ void stage_a(float* As, const float (&r)[BM * BK / 256]) {
    constexpr int APT = BM * BK / 256, LDA_S = BM + 1;
    const int t = threadIdx.x;
    if constexpr (!TA) {
        constexpr int TPR = BK / APT;
        const int m = t / TPR, kk = (t % TPR) * APT;
#pragma unroll
        for (int i = 0; i < APT; ++i) As[(kk + i) * LDA_S + m] = r[i];
    } else {
        constexpr int TPK = BM / APT;
        const int kq = t / TPK, m = (t % TPK) * APT;
#pragma unroll
        for (int i = 0; i < APT; ++i) As[kq * LDA_S + m + i] = r[i];
    }
}

template <bool TB, int BN, int BK>
__device__ __forceinline__ void stage_b(float* Bs, const float (&r)[BN * BK / 256]) {
    constexpr int BPT = BN * BK / 256, LDB_S = BN + 1;
    const int t = threadIdx.x;
    if constexpr (!TB) {
        constexpr int TPK = BN / BPT;
        const int kq = t / TPK, n = (t % TPK) * BPT;
#pragma unroll
        for (int i = 0; i < BPT; ++i) Bs[kq * LDB_S + n + i] = r[i];
    } else {
        constexpr int TPN = BK / BPT;
        const int n = t / TPN, kq = (t % TPN) * BPT;
#pragma unroll
        for (int i = 0; i < BPT; ++i) Bs[(kq + i) * LDB_S + n] = r[i];
    }
}

// The workgroup's body: (bx, by, bz) = its tile coordinates in dispatch order (x fastest), (ntn, ntm) = the product's OWN tile counts
// along n and m -- not the launch's grid, which may hold workgroups that are no tiles (k_gemm_f32_riders).
template <bool TA, bool TB, int MT, int NT, int BK>
__device__ __forceinline__ void gemm_f32_body(const GemmParams& p, const int bx, const int by, const int bz, const int ntn,
                                              const int ntm) {
    constexpr int BM = 64 * MT, BN = 64 * NT, LDA_S = BM + 1, LDB_S = BN + 1;
    __shared__ float As[BK * LDA_S];
    __shared__ float Bs[BK * LDB_S];
    // Workgroups are dealt round-robin to the 8 XCDs.  The n-tiles of one m-tile share the A rows: give them CONSECUTIVE slots of
    // the SAME XCD, so that a tall A (configs[4]: 800 MB, far beyond the Infinity Cache) crosses the fabric once instead of once
    // per n-tile.  (Whole groups of 8 m-tiles only; the ragged end keeps the plain order.)
    int mt_i = by, nt_i = bx;
    if (p.tmask_wanted > 0) {
        // the x-th wanted 64 x 64 tile (MT = NT = 1): no block exists for the others -- with one block per tile, wanted or not, the CUs
        // that were dealt 4 wanted blocks set the launch's time whatever the others hold (2-4 per CU under a triangular mask)
        int rank = bx, bit = -1;
        for (int w = 0; bit < 0; ++w) {
            unsigned long long word = p.tmask[w];
            const int pc = __popcll(word);
            if (rank >= pc) { rank -= pc; continue; }
            for (int i = 0; i < rank; ++i) word &= word - 1;
            bit = 64 * w + __builtin_ctzll(word);
        }
        mt_i = bit / p.tmask_ld;
        nt_i = bit - mt_i * p.tmask_ld;
    } else {
        const int lin = by * ntn + bx;
        const int full = (ntm / 8) * 8 * ntn;
        if (lin < full) {
            const int xcd = lin & 7, j = lin >> 3;
            // (rotated by the m-tile group: an XCD deals its slots to its 32 CUs in turn, so with 8 column tiles a CU would receive the
            // SAME column tile every time -- and under k-chunk words the column tiles differ in length: 72 us instead of ~55 on the 500 x 500
            // MADE layer, the CUs holding the unmasked tiles finishing last)
            nt_i = (j + j / ntn) % ntn;
            mt_i = (j / ntn) * 8 + xcd;
            // wanted-tile words (a block-triangular weight gradient): XCD x would hold row-tile x of every column tile, i.e. 1 .. 8 wanted
            // tiles, and a CU -- dealt every 32nd slot of its XCD -- the SAME tile of every k-split.  Tiles with (row + column) % 8 = x
            // go to XCD x (4-5 wanted ones each under a triangular mask), the column rotated with the split so that a CU's blocks differ
            if (p.tmask) {
                const int z = bz;
                nt_i = (nt_i + z + (z >> 2)) % ntn;
                mt_i = (j / ntn) * 8 + ((xcd - nt_i) & 7);
            }
        }
    }
    const int m0 = mt_i * BM, n0 = nt_i * BN;
    const int kbeg = bz * p.k_chunk;
    int kend = min(p.k, kbeg + p.k_chunk);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32 * MT, wn = (wid & 1) * 32 * NT;
    const int l31 = lane & 31, lhi = lane >> 5;
    if (p.rows_dev) {
        // a static-shape batch pads its node arrays: rows [*rows_dev, ...) of the stored A are padding.  A row-major A: a tile that
        // holds only padding rows is not computed -- zeros are stored (nothing when accumulating); A stored [K, M]: K ends there
        const int live = *p.rows_dev;
        if constexpr (TA) {
            kend = max(kbeg, min(kend, live));
        } else if (m0 >= live && p.split_k == 1) {
            if (!p.accumulate)
                for (int i = threadIdx.x; i < BM * BN; i += 256) {
                    const int row = m0 + i / BN, col = n0 + i % BN;
                    if (row < p.m && col < p.n) p.c[(size_t)row * p.ldc + col] = 0.f;
                }
            return;
        }
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;

    bool wanted = true;
    if (p.tmask) {      // a tile of C that the caller knows to be zero: every 64 x 64 part of it is unwanted
        wanted = false;
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int bit = (mt_i * MT + t) * p.tmask_ld + nt_i * NT + u;
                if ((mt_i * MT + t) * 64 < p.m && (nt_i * NT + u) * 64 < p.n) wanted = wanted || ((p.tmask[bit >> 6] >> (bit & 63)) & 1ull);
            }
    }
    // the k-chunks to walk: all of [kbeg, kend), or the ones whose bit is set in this column tile's word (NT == 1, BK == 16)
    unsigned long long todo = ~0ull;
    const bool sparse = p.kmask != nullptr;
    if (sparse) {
        todo = p.kmask[nt_i];                                  // bits count 16-wide chunks
        if (BK == 32) {                                        // a 32-deep step is walked when either of its halves is marked
            unsigned long long t = (todo | (todo >> 1)) & 0x5555555555555555ull, packed = 0ull;
            for (int i = 0; i < 32; ++i) packed |= ((t >> (2 * i)) & 1ull) << i;
            todo = packed;
        }
    }
    if (!wanted) todo = 0ull;
    auto next_chunk = [&](int from) -> int {      // first chunk >= from inside the k range that is to be walked, or kend
        if (!sparse && wanted) return from;
        const int c = from / BK;
        const unsigned long long rest = c < 64 ? (todo >> c) : 0ull;
        if (!rest) return kend;
        return (c + __builtin_ctzll(rest)) * BK;
    };

    float ra[BM * BK / 256], rb[BN * BK / 256];
    int k0 = min(next_chunk(kbeg), kend);
    if (k0 < kend) {
        load_a<TA, BM, BK>(p, m0, k0, kend, ra);
        load_b<TB, BN, BK>(p, n0, k0, kend, rb);
    }
    while (k0 < kend) {
        stage_a<TA, BM, BK>(As, ra);
        stage_b<TB, BN, BK>(Bs, rb);
        __syncthreads();
        const int k1 = min(next_chunk(k0 + BK), kend);
        if (k1 < kend) {  // next tile's loads fly under this tile's MFMAs
            load_a<TA, BM, BK>(p, m0, k1, kend, ra);
            load_b<TB, BN, BK>(p, n0, k1, kend, rb);
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float bf[NT], af[MT];
#pragma unroll
            for (int u = 0; u < NT; ++u) bf[u] = Bs[(kk + lhi) * LDB_S + wn + 32 * u + l31];
#pragma unroll
            for (int t = 0; t < MT; ++t) af[t] = As[(kk + lhi) * LDA_S + wm + 32 * t + l31];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t], bf[u], acc[t][u], 0, 0, 0);
        }
        __syncthreads();
        k0 = k1;
    }
    // C/D map of the 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int col = n0 + wn + 32 * u + l31;
        if (col >= p.n) continue;
        const float bv = (p.bias && p.split_k == 1) ? p.bias[col] : 0.f;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (p.tmask && MT * NT > 1) {
                // a block of several 64 x 64 tiles ran because one of them is wanted: the unwanted ones still hold zeros
                const int ti = (m0 + wm + 32 * t) >> 6, tj = (n0 + wn + 32 * u) >> 6;
                const int bit = ti * p.tmask_ld + tj;
                if (ti * 64 < p.m && !((p.tmask[bit >> 6] >> (bit & 63)) & 1ull))
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;
            }
            // accumulate: the 16 previous values of this tile column are requested TOGETHER (load, add, store per element in
            // source order makes the compiler wait for every load before the next: 16 round trips per tile)
            float old[16];
            const bool acc_old = p.accumulate && p.split_k == 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                old[r] = 0.f;
                if (acc_old && row < p.m) old[r] = p.c[(size_t)row * p.ldc + col];
            }
            // ... added in a loop of their own, and stored in a third: a store loop that reads no loaded register needs no wait
            float val[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[t][u][r];
                if (p.split_k == 1) {
                    v = apply_act(v + bv, p.act);
                    v = acc_old ? old[r] + v : v;
                }
                val[r] = v;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (row >= p.m) continue;
                if (p.split_k > 1) p.ws[((size_t)bz * p.m + row) * p.n + col] = val[r];
                else p.c[(size_t)row * p.ldc + col] = val[r];
            }
        }
    }
}

// MT / NT = 32-row / 32-column MFMA tiles per wave: block tile (64*MT) x (64*NT) x BK, four waves as 2 (M) x 2 (N).
template <bool TA, bool TB, int MT, int NT, int BK>
__global__ __launch_bounds__(256) void k_gemm_f32(const GemmParams p) {
    gemm_f32_body<TA, TB, MT, NT, BK>(p, blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x, gridDim.y);
}

// The same product with RIDERS (k_riders.h): a 1-D launch of ntn * ntm tile workgroups, in the plain kernel's dispatch order, and
// n_riders workgroups that run independent small jobs on the VALUs and the memory system the product leaves free.  The branch is
// block-uniform.  riders_front: the rider workgroups are dispatched first (n_riders is then a multiple of 8, so that every tile
// workgroup keeps the XCD it has in the plain launch); otherwise they follow the tiles.  No split-K, no k-chunk / tile words.
// <false, false>: the forward's x @ loop_weight; <false, true>: the backward's dL/dx = g @ loop_weight^T (_loop_grads), which
// carries the gradient finishers.  A rider workgroup's 4 KiB scratch stands beside the tile's staging arrays (12.4 of 160 KiB).
template <bool TA, bool TB, int MT, int NT, int BK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MT == 2 ? 5 : 7))) void k_gemm_f32_riders(const GemmParams p, const RiderSet rs, const int ntn, const int ntm,
                                                         const int n_riders, const int riders_front) {
    __shared__ float rider_sm[64][16];
    const int tiles = ntn * ntm;
    int b = blockIdx.x;
    if (riders_front) {
        if (b < n_riders) { rider_body(rs, b, n_riders, rider_sm); return; }
        b -= n_riders;
    } else if (b >= tiles) {
        rider_body(rs, b - tiles, n_riders, rider_sm);
        return;
    }
    const int by = b / ntn;
    gemm_f32_body<TA, TB, MT, NT, BK>(p, b - by * ntn, by, 0, ntn, ntm);
}

// ---- the 64 x 64 score tile of the entity queries: acc = Q[m0 .., :] @ E[n0 .., :]^T -------------------------------------------
// The rankers and the top-k scorer all take their logits from here, and it runs the SAME k-ordered fp32 MFMA chain as
// k_gemm_f32<false, true, 1, 1, 16>: a target's logit is bit-identical to the element a later pass recomputes, every count equals
// the one taken on a materialised score matrix, and top-k logits equal gv_gemm_f32 + bias.  The caller has issued the loads of
// the first k-chunk into ra / rb (so they fly under whatever it does first); the later chunks' loads fly under the MFMAs here.
constexpr int SC_BM = 64, SC_BN = 64, SC_BK = 16, SC_LDA = SC_BM + 1, SC_LDB = SC_BN + 1;

__device__ __forceinline__ f32x16 score_tile(const GemmParams& p, int m0, int n0, float (&ra)[SC_BM * SC_BK / 256],
                                             float (&rb)[SC_BN * SC_BK / 256], float* As, float* Bs) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < p.k; k0 += SC_BK) {
        stage_a<false, SC_BM, SC_BK>(As, ra);
        stage_b<true, SC_BN, SC_BK>(Bs, rb);
        __syncthreads();
        if (k0 + SC_BK < p.k) {
            load_a<false, SC_BM, SC_BK>(p, m0, k0 + SC_BK, p.k, ra);
            load_b<true, SC_BN, SC_BK>(p, n0, k0 + SC_BK, p.k, rb);
        }
#pragma unroll
        for (int kk = 0; kk < SC_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + lhi) * SC_LDA + wm + l31], Bs[(kk + lhi) * SC_LDB + wn + l31],
                                                       acc, 0, 0, 0);
        __syncthreads();
    }
    return acc;
}

// score_tile_with: score_tile with the query rows supplied by the caller -- load_a_chunk(k0, ra) fills ra with this thread's share
// of Q[m0 .., k0 ..] in load_a's layout (gv_entity_topk_scores gathers and scales them on the way).  The same staging, the same
// chain; score_tile keeps its own spelling because routing it through here moves instructions in the rankers' and selectors' code.
template <class LoadA>
__device__ __forceinline__ f32x16 score_tile_with(const GemmParams& p, LoadA load_a_chunk, int n0, float (&ra)[SC_BM * SC_BK / 256],
                                                  float (&rb)[SC_BN * SC_BK / 256], float* As, float* Bs) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < p.k; k0 += SC_BK) {
        stage_a<false, SC_BM, SC_BK>(As, ra);
        stage_b<true, SC_BN, SC_BK>(Bs, rb);
        __syncthreads();
        if (k0 + SC_BK < p.k) {
            load_a_chunk(k0 + SC_BK, ra);
            load_b<true, SC_BN, SC_BK>(p, n0, k0 + SC_BK, p.k, rb);
        }
#pragma unroll
        for (int kk = 0; kk < SC_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + lhi) * SC_LDA + wm + l31], Bs[(kk + lhi) * SC_LDB + wn + l31],
                                                       acc, 0, 0, 0);
        __syncthreads();
    }
    return acc;
}

// score_tile_gather: score_tile_with with the entity rows supplied by the caller as well -- load_b_chunk(k0, rb) fills rb with this
// thread's share of the tile's 64 entity rows in load_b's layout (gv_entity_topk_scores_typed gathers them through member ids).
// The same staging, the same chain: a gathered row's logits are the bits score_tile gives that row.
template <class LoadA, class LoadB>
__device__ __forceinline__ f32x16 score_tile_gather(const GemmParams& p, LoadA load_a_chunk, LoadB load_b_chunk,
                                                    float (&ra)[SC_BM * SC_BK / 256], float (&rb)[SC_BN * SC_BK / 256], float* As,
                                                    float* Bs) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < p.k; k0 += SC_BK) {
        stage_a<false, SC_BM, SC_BK>(As, ra);
        stage_b<true, SC_BN, SC_BK>(Bs, rb);
        __syncthreads();
        if (k0 + SC_BK < p.k) {
            load_a_chunk(k0 + SC_BK, ra);
            load_b_chunk(k0 + SC_BK, rb);
        }
#pragma unroll
        for (int kk = 0; kk < SC_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + lhi) * SC_LDA + wm + l31], Bs[(kk + lhi) * SC_LDB + wn + l31],
                                                       acc, 0, 0, 0);
        __syncthreads();
    }
    return acc;
}

// ---- the Monte-Carlo posterior-predictive tile (gv_rank_scores_mc, gv_topk_scores_mc): a loop over samples around score_tile ----
// Sample s has its own query matrix at q + s * q_stride and its own entity table at e + s * e_stride (the leading dimensions are
// shared) and an optional bias[s]; logit_s comes from score_tile unchanged, and
//   pbar[i, j] = (sum over s ascending of sig(logit_s[i, j] + bias[s])) * (1.0f / S)
// stays in 16 registers per lane from the MFMA accumulator to the caller's vote or selection.
struct McSamples {
    long long q_stride, e_stride;      // elements between consecutive samples' Q / E
    int n_samples;                     // 0: not a Monte-Carlo launch
    float inv_s;                       // 1.0f / n_samples (exact for a power of two: the same sample twice gives the sample's value)
};

// (sig is mc_sig of k_mc.h, the one form the typed MC miner of k_mine.hip uses too.)

// The caller has issued sample 0's first k-chunk of tile (m0, n0) into ra / rb.  Under each sample's epilogue (16 exp + 16 rcp per
// lane) the next sample's first k-chunk is already in flight; under the last one, sample 0's of the tile at n0_next (< 0: none).
__device__ __forceinline__ f32x16 mc_pbar_tile(const GemmParams& g, const McSamples& mc, const float* bias, int m0, int n0,
                                               int n0_next, float (&ra)[SC_BM * SC_BK / 256], float (&rb)[SC_BN * SC_BK / 256],
                                               float* As, float* Bs) {
    f32x16 sum;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum[i] = 0.f;
    GemmParams p = g;
    for (int s = 0; s < mc.n_samples; ++s) {
        const f32x16 acc = score_tile(p, m0, n0, ra, rb, As, Bs);
        const float bv = bias ? bias[s] : 0.f;
        if (s + 1 < mc.n_samples) {
            p.a += mc.q_stride;
            p.b += mc.e_stride;
            load_a<false, SC_BM, SC_BK>(p, m0, 0, p.k, ra);
            load_b<true, SC_BN, SC_BK>(p, n0, 0, p.k, rb);
        } else if (n0_next >= 0) {
            load_a<false, SC_BM, SC_BK>(g, m0, 0, g.k, ra);
            load_b<true, SC_BN, SC_BK>(g, n0_next, 0, g.k, rb);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) sum[i] += mc_sig(acc[i] + bv);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) sum[i] *= mc.inv_s;
    return sum;
}

// ---- evaluation scorer with a rank-count epilogue (perturb_and_get_rank, kgvae/utils.py:180-221) ----
// S = Q (m x h) @ E^T (E: v x h), prob = sigmoid(S + *bias).  The reference materialises an (h, Eb, V) tensor, sorts every
// row and looks the target up; here the probabilities never leave the registers:
//   PASS 0  tgt[row]    = logit[row, target[row]]                     (written by the one lane that owns that element)
//   PASS 1  count[row] += #{ col != target[row] : logit[row, col] > tgt[row] }   (wave ballots, one int atomic per 32 columns)
// Both passes take the logit from score_tile, so tgt is bit-identical to the element the second pass recomputes.
struct RankParams {
    GemmParams g;            // a = Q, b = E (stored [v, h]), m, n = v, k = h
    const int* target;
    const float* bias;
    float* tgt;
    int* count;
};

// This half-wave's ballots for the 32 columns it holds of `row`: bit j of `above` / `equal` = the candidate in column
// (col - l31) + j beats / ties with the row's target.  Ranked on the LOGIT: monotone with the reference's sigmoid
// (kgvae/utils.py:208) but free of its saturation, where every candidate ties at 1.0f.  A count is 2 * #above + #equal, i.e. twice
// the mid-rank under ties; a candidate that is NaN, or any candidate when the target itself is NaN, counts as above (never
// optimistic).  The target's own column and everything outside the matrix vote nowhere.
struct RankVotes {
    unsigned above, equal;
};

// (a row is never negative: indexed unsigned, an access costs no sign extension)
__device__ __forceinline__ RankVotes rank_votes(const RankParams& rp, float logit, int row, int col, int lhi) {
    const bool live = row < rp.g.m;
    const int tcol = live ? rp.target[(unsigned)row] : -1;
    const float t = live ? rp.tgt[(unsigned)row] : 0.f;
    const bool other = live && col < rp.g.n && col != tcol;
    const bool above = other && !(logit <= t);          // greater, or either side NaN
    const bool equal = other && logit == t;
    const unsigned long long ma = __ballot(above), me = __ballot(equal);
    return {(unsigned)(lhi ? (ma >> 32) : (ma & 0xffffffffull)), (unsigned)(lhi ? (me >> 32) : (me & 0xffffffffull))};
}

__device__ __forceinline__ void rank_count_add(int* count, int row, unsigned above, unsigned equal) {
    const int c = 2 * __popc(above) + __popc(equal);
    if (c) atomicAdd(count + (unsigned)row, c);
}

template <int PASS>
__global__ __launch_bounds__(256) void k_rank_scores(const RankParams rp) {
    __shared__ float As[SC_BK * SC_LDA];
    __shared__ float Bs[SC_BK * SC_LDB];
    const GemmParams& p = rp.g;
    const int m0 = blockIdx.y * SC_BM, n0 = blockIdx.x * SC_BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    float ra[SC_BM * SC_BK / 256], rb[SC_BN * SC_BK / 256];
    load_a<false, SC_BM, SC_BK>(p, m0, 0, p.k, ra);
    load_b<true, SC_BN, SC_BK>(p, n0, 0, p.k, rb);
    const f32x16 acc = score_tile(p, m0, n0, ra, rb, As, Bs);
    const float bv = rp.bias ? *rp.bias : 0.f;
    const int col = n0 + (wid & 1) * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + (wid >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        const float logit = acc[r] + bv;
        if (PASS == 0) {
            if (row < p.m && col < p.n && col == rp.target[row]) rp.tgt[row] = logit;
        } else {
            const RankVotes vt = rank_votes(rp, logit, row, col, lhi);
            if (l31 == 0 && row < p.m) rank_count_add(rp.count, row, vt.above, vt.equal);
        }
    }
}

// ---- the rank counts: raw, filtered (the filtered MRR protocol) and type-constrained, from one pass over the scores ------------
// tgt comes from k_rank_scores<0>; every count is taken from the ballots of k_rank_scores<1> (rank_votes) on the same logits, so the
// raw count equals gv_rank_scores' bit for bit, and the filtered one drops the candidates listed in the query's filter range:
//   count_filt[row] += #{ col != target[row], col not in filt_ent[filt_lo[row] .. filt_hi[row]) : logit > tgt (or NaN) } * 2 + ties
// The filter of the 64 x 64 tile is a 64-bit word per row in LDS (bit j = column n0 + j is filtered), built before the MFMA loop:
// two lower-bound searches per row for the window [n0, n0 + 64) of its sorted list, then the window's entries (<= 64 per row) set
// bits one lane each.  A filtered NaN candidate counts nowhere: exclusion acts on the ballot of the very logit that is counted.
struct RankFiltParams {
    RankParams rp;           // rp.count = the raw count (may be NULL)
    const int* filt_lo;
    const int* filt_hi;
    const int* filt_ent;
    int n_ent;               // length of filt_ent: every range is clamped into it
    int* count_filt;
    TopkCand cs;             // CAND only (gv_rank_scores_constrained, gv_rank_scores_mc_constrained)
    int* count_raw_c;
    int* count_filt_c;       // NULL (as count_filt, filt_lo) when no filter is given
    McSamples mc;            // MC only (gv_rank_scores_mc, gv_rank_scores_mc_constrained): rp.bias then holds one value per sample
};

// CAND: the type-constrained protocol on top.  The tile's 64 columns are two words of the row's set (topk_cand_pair), loaded once
// per row and tile into LDS next to the filter word and ANDed into the same ballots, so the constrained counts see the very logits
// of the unconstrained ones.  The filter is optional there.
// MC: the posterior-predictive ranker (gv_rank_scores_mc).  The value that votes is pbar from mc_pbar_tile instead of the logit --
// bounded, so it CAN saturate: candidates whose every sample rounds to 1.0f tie with such a target and share the mid-rank -- and
// rp.tgt comes from k_rank_target_mc, which runs the same sample loop.  Filter, ballots and counts are the ones above; the filter
// is optional (raw count only without one).  Its 16 extra accumulators are held inside the single-sample rankers' 8 waves / SIMD
// (waves_per_eu: 64 registers; the single-sample instantiations keep the default and their code).
// CAND and MC together (gv_rank_scores_mc_constrained): all four counts vote on the one pbar; the set words are in LDS before the
// sample loop starts, so the constraint holds no register across it and the budget is the MC ranker's.
template <bool CAND, bool MC = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MC ? 8 : 1))) void k_rank_scores_filtered(const RankFiltParams fp) {
    constexpr int BM = SC_BM, BN = SC_BN, BK = SC_BK;
    __shared__ float As[BK * SC_LDA];
    __shared__ float Bs[BK * SC_LDB];
    __shared__ unsigned long long fmask[CAND ? 2 * BM : BM];       // 512 B: the tile's filter, one word per row (CAND: + the set's)
    __shared__ int win_lo[BM], win_hi[BM];         // each row's entries inside [n0, n0 + 64)
    const RankParams& rp = fp.rp;
    const GemmParams& p = rp.g;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    float ra[BM * BK / 256], rb[BN * BK / 256];
    load_a<false, BM, BK>(p, m0, 0, p.k, ra);      // the first operand loads fly under the filter searches
    load_b<true, BN, BK>(p, n0, 0, p.k, rb);

    // filter window: thread t < 64 searches row t's list for n0, thread 64 + t for n0 + 64 (two waves, one search each)
    const bool filtered = (!CAND && !MC) || fp.filt_lo != nullptr;
    if (threadIdx.x < 2 * BM) {
        const int rl = threadIdx.x & (BM - 1), row = m0 + rl;
        int lo = 0, hi = 0;
        if (row < p.m && filtered) {
            lo = min(max(fp.filt_lo[row], 0), fp.n_ent);
            hi = min(max(fp.filt_hi[row], lo), fp.n_ent);
        }
        const int pos = lower_bound_i32(fp.filt_ent, lo, hi, threadIdx.x < BM ? n0 : n0 + BN);
        if (threadIdx.x < BM) { win_lo[rl] = pos; fmask[rl] = 0ull; }
        else win_hi[rl] = pos;
    } else if (CAND && threadIdx.x < 3 * BM) {     // the third wave: row t's two set words for columns [n0, n0 + 64)
        const int rl = threadIdx.x & (BM - 1);
        fmask[BM + rl] = topk_cand_pair(fp.cs, m0 + rl, p.m, n0, p.n);
    }
    __syncthreads();
    // the window's entries, staged cooperatively: wave w takes rows 16 w .. 16 w + 15, one entry per lane (a long list costs its
    // window's entries only, never its length; an empty window -- most rows of most tiles -- costs one LDS read)
    for (int i = 0; i < BM / 4; ++i) {
        const int rl = wid * (BM / 4) + i;
        const int a = win_lo[rl], cnt = win_hi[rl] - a;
        for (int j = lane; j < cnt; j += 64) {
            const unsigned bit = (unsigned)(fp.filt_ent[a + j] - n0);
            if (bit < 64u) atomicOr(&fmask[rl], 1ull << bit);
        }
    }

    f32x16 acc;
    float bv = 0.f;
    if constexpr (MC) {
        acc = mc_pbar_tile(p, fp.mc, rp.bias, m0, n0, -1, ra, rb, As, Bs);
    } else {
        acc = score_tile(p, m0, n0, ra, rb, As, Bs);
        bv = rp.bias ? *rp.bias : 0.f;
    }
    const int col = n0 + wn + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rl = wm + (r & 3) + 8 * (r >> 2) + 4 * lhi, row = m0 + rl;
        const RankVotes vt = rank_votes(rp, MC ? acc[r] : acc[r] + bv, row, col, lhi);
        if (l31 == 0 && row < p.m) {
            const unsigned keep = ~(unsigned)(fmask[rl] >> wn);    // this half-wave's 32 columns of the row's filter word
            if (rp.count) rank_count_add(rp.count, row, vt.above, vt.equal);
            if ((!CAND && !MC) || fp.count_filt) rank_count_add(fp.count_filt, row, vt.above & keep, vt.equal & keep);
            if (CAND) {      // the votes have dropped the columns >= v already, whatever the set's padding bits hold
                const unsigned member = (unsigned)(fmask[BM + rl] >> wn);
                rank_count_add(fp.count_raw_c, row, vt.above & member, vt.equal & member);
                if (fp.count_filt_c) rank_count_add(fp.count_filt_c, row, vt.above & keep & member, vt.equal & keep & member);
            }
        }
    }
}

// The first pass of gv_rank_scores_mc: tgt[row] = pbar[row, target[row]], from the same sample loop the second pass runs, so the
// element is recomputed there bit for bit.  A workgroup reads its 64 targets first and leaves when none falls in its 64 columns:
// of the whole grid, at most 64 workgroups per row tile do any arithmetic.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_rank_target_mc(const RankFiltParams fp) {
    __shared__ float As[SC_BK * SC_LDA];
    __shared__ float Bs[SC_BK * SC_LDB];
    const RankParams& rp = fp.rp;
    const GemmParams& p = rp.g;
    const int m0 = blockIdx.y * SC_BM, n0 = blockIdx.x * SC_BN;
    bool mine = false;
    if (threadIdx.x < SC_BM && m0 + (int)threadIdx.x < p.m)
        mine = (unsigned)(rp.target[m0 + threadIdx.x] - n0) < (unsigned)SC_BN;
    if (!__syncthreads_or(mine)) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    float ra[SC_BM * SC_BK / 256], rb[SC_BN * SC_BK / 256];
    load_a<false, SC_BM, SC_BK>(p, m0, 0, p.k, ra);
    load_b<true, SC_BN, SC_BK>(p, n0, 0, p.k, rb);
    const f32x16 pbar = mc_pbar_tile(p, fp.mc, rp.bias, m0, n0, -1, ra, rb, As, Bs);
    const int col = n0 + (wid & 1) * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + (wid >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (row < p.m && col < p.n && col == rp.target[row]) rp.tgt[row] = pbar[r];
    }
}

// ---- top-k link prediction (gv_topk_scores): the rankers' score pass with a selection epilogue ----------------------------
// logit[i, j] = q_i . e_j + bias comes from score_tile, as the rankers' does (so it equals gv_gemm_f32 + bias bit
// for bit); the score matrix is never stored.  Candidates are ordered by a 64-bit key, larger = better:
//   key = ordered_u32(logit) << 32 | ~id      ordered_u32: the sign-flip map, -0 -> +0, NaN -> 0 (after -inf)
// a strict total order (ties on the logit by lower id); key 0 is "no candidate" and decodes to id -1, logit -inf.
// Stage 1 (k_topk_span): a workgroup owns a 64-row query tile and sweeps a span of 64-column entity tiles in ascending order.  The
// tile's logits go through LDS; wave w then takes rows 16 w .. 16 w + 15, one lane per column: a key that beats the row's running
// threshold (its current k-th key) is inserted into the row's sorted list (LDS, k keys per row), one wave-wide shift per
// survivor.  Once a list is warm almost nothing passes, so a tile costs a compare and a ballot per row.  Filtered columns get key 0
// through a per-row cursor into the sorted filter list (the next listed id is kept in LDS: a window without entries reads
// nothing).  The span's k keys per row go to the workspace.  Stage 2 (k_topk_merge): one wave per row merges the S span lists.
// Key, list, cursor, the epilogue's set-up / row loop / hand-on (topk_span_*) and the merge live in k_topk.h, which the other three
// span kernels share; a kernel keeps the making of its tile and, as lambdas, the row's cursor set-up and the row's key.
struct TopkParams {
    GemmParams g;                 // a = Q, b = E (stored [v, h]), m, n = v, k = h
    const float* bias;
    const int* filt_lo;           // NULL: no filter
    const int* filt_hi;
    const int* filt_ent;
    int n_ent;                    // length of filt_ent: every range is clamped into it
    int topk;                     // 1..128
    int span_tiles;               // 64-column tiles per span (blockIdx.y = span)
    int n_spans;
    unsigned long long* part;     // [m][n_spans][topk] keys, each span's list sorted descending
    TopkCand cs;                  // CAND only (gv_topk_scores_constrained, gv_topk_scores_mc_constrained)
    McSamples mc;                 // MC only (gv_topk_scores_mc, gv_topk_scores_mc_constrained): bias then holds one value per sample
};

// MC: the key's value is pbar from mc_pbar_tile (the very values gv_rank_scores_mc votes on) instead of the logit; held to the
// 5 waves / SIMD of the single-sample scorer (which its LDS allows at most anyway).  With CAND on top (gv_topk_scores_mc_constrained)
// the tile's set word is requested ahead of the sample loop; cand_row is the one value the 96-register ceiling sends to scratch,
// reloaded once per column tile outside the sample loop.
template <int NK, bool CAND, bool MC = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MC ? 5 : 1))) void k_topk_span(const TopkParams tp) {
    constexpr int BM = SC_BM, BN = SC_BN, BK = SC_BK, LDL = BN + 1;
    __shared__ float As[BK * SC_LDA];
    __shared__ float Bs[BK * SC_LDB];
    __shared__ float Ls[BM * LDL];                 // the tile's logits, row-major
    __shared__ unsigned long long thr[BM];         // each row's k-th key
    __shared__ int cur[BM], fhi[BM], nxt[BM];      // filter cursor, range end, the id at the cursor (INT_MAX: none left)
    __shared__ int fl[4][64];                      // per wave: column j of the row at hand is listed <=> fl[w][j] == tag
    extern __shared__ unsigned long long lists[];  // [BM][topk]
    const GemmParams& p = tp.g;
    const int k = tp.topk;
    const int m0 = blockIdx.x * BM;
    const int t_begin = blockIdx.y * tp.span_tiles;
    const int t_end = min(t_begin + tp.span_tiles, (p.n + BN - 1) / BN);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const bool filtered = tp.filt_lo != nullptr;
    float ra[BM * BK / 256], rb[BN * BK / 256];
    if (t_begin < t_end) {
        load_a<false, BM, BK>(p, m0, 0, p.k, ra);
        load_b<true, BN, BK>(p, t_begin * BN, 0, p.k, rb);
    }
    topk_span_clear<BM>(lists, k, fl, thr, lane, wid, [&](int rl) {
        const int row = m0 + rl;
        topk_filter_begin(tp.filt_lo, tp.filt_hi, tp.filt_ent, tp.n_ent, filtered && row < p.m, row, t_begin * BN, &cur[rl], &fhi[rl],
                          &nxt[rl]);
    });
    const float bv = (!MC && tp.bias) ? *tp.bias : 0.f;
    const uint32_t* cand_row = CAND ? topk_cand_row(tp.cs, m0 + wid * (BM / 4), p.m, lane) : nullptr;

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * BN;
        const unsigned cand_w = CAND ? topk_cand_word(cand_row, n0, p.n, lane) : 0u;     // lands under the MFMA chain
        f32x16 acc;
        if constexpr (MC) {                                        // (the next tile's first operands are requested in there)
            acc = mc_pbar_tile(p, tp.mc, tp.bias, m0, n0, t + 1 < t_end ? n0 + BN : -1, ra, rb, As, Bs);
        } else {
            acc = score_tile(p, m0, n0, ra, rb, As, Bs);
            if (t + 1 < t_end) {                                   // the next tile's first operands fly under the selection
                load_a<false, BM, BK>(p, m0, 0, p.k, ra);
                load_b<true, BN, BK>(p, n0 + BN, 0, p.k, rb);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            Ls[(wm + (r & 3) + 8 * (r >> 2) + 4 * lhi) * LDL + wn + l31] = MC ? acc[r] : acc[r] + bv;
        __syncthreads();                                           // (Ls is rewritten after the next tile's first barrier)

        const int col = n0 + lane;
        topk_span_select<NK, BM>(m0, p.m, lists, thr, k, lane, wid, [&](int rl, int i) {
            unsigned long long key = col < p.n ? topk_key(Ls[rl * LDL + lane], col) : 0ull;
            if (filtered && nxt[rl] < n0 + BN &&                  // this row lists ids inside the tile: mark them, advance the cursor
                topk_filter_window(tp.filt_ent, n0, (t - t_begin) * BM + rl + 1, lane, &cur[rl], &fhi[rl], &nxt[rl], fl[wid]))
                key = 0ull;
            if (CAND && !topk_cand_member(cand_w, i, lane)) key = 0ull;
            return key;
        });
    }
    topk_span_hand_on<BM>(m0, p.m, lists, k, tp.part, tp.n_spans, lane, wid);
}

// ---- per-entity completion (gv_entity_topk_scores): one list per query entity over ALL relations -------------------------------
// Query row i is entity a = ents[i]; its candidates are the pairs (r, x), logit = (E[a] * w[r]) . E[x] + bias -- k_topk_span with
// the relations walked INSIDE the row's list, so neither an (entity x relation) query matrix nor m * R * k intermediate results
// exist.  The columns of a row are the sequence of (relation, 64-column tile) pairs, r-major: tile t = r * col_tiles + ct, candidate
// id = r * N + x (< 2^31), so the ordered key of k_topk.h already says "logit, then relation, then entity".  A workgroup owns a
// 64-row tile of query entities and a contiguous span of that sequence.  The query operand is made while it is staged: a thread's
// four floats of E[a] (gathered through ents) times the same four of w[r], one f32 multiply each -- the value gv_mul stores --
// and goes through score_tile's K-chunked staging, so LDS is k_topk_span's (27 KiB + the lists) at any width and k = 128 fits
// beside it.  At the first tile of a relation (and of the span) the 64 rows' filter cursors are re-opened on key a * R + r.
struct EntityTopkParams {
    GemmParams g;                 // b = E (stored [N, h]), m, n = N, k = h; a is not read
    const int* ents;              // [m] query entities; an id outside [0, N) is a row without candidates
    const float* w;               // [R, ld_w]
    int ld_w, vec_a;              // vec_a: four floats of a row of E and of w may be read as one
    int num_rels, exclude_self;
    const float* bias;
    const int* filt_lo;           // key a * R + r; NULL: no filter
    const int* filt_hi;
    const int* filt_ent;
    int n_ent;
    int topk;
    int span_tiles, n_spans;      // (relation, column tile) pairs per span (blockIdx.y = span)
    unsigned long long* part;     // [m][n_spans][topk]
};

// MC (gv_entity_topk_scores_mc): the samples beside the parent's parameters, which keep their layout; e.bias then holds one value
// per sample
struct EntityTopkMcParams {
    EntityTopkParams e;
    McSamples mc;
};

__device__ __forceinline__ const EntityTopkParams& entity_topk_params(const EntityTopkParams& pp) { return pp; }
__device__ __forceinline__ const EntityTopkParams& entity_topk_params(const EntityTopkMcParams& pp) { return pp.e; }

// MC: the key's value is pbar -- mc_pbar_tile's arithmetic around score_tile_with, sample s reading the table at b + s * e_stride
// for the query rows E_s[a] and the candidate rows alike, the one w shared -- written to Ls and selected ONCE per tile; the walk,
// the cursors and the selection never see a sample.  Under each sample's sigmoids the next sample's first k-chunk is in flight,
// under the last one's the next tile's sample-0 chunk.  The samples come in a wrapper struct and the single-sample branch keeps
// the parent's statements spelled out (no helper shared with the MC branch): either a longer EntityTopkParams or a shared lambda
// costs the single-sample kernel two registers and its fifth wave; the typed kernel below does the same.
template <int NK, bool MC = false>
__global__ __launch_bounds__(256) void k_entity_topk_span(const std::conditional_t<MC, EntityTopkMcParams, EntityTopkParams> pp) {
    constexpr int BM = SC_BM, BN = SC_BN, BK = SC_BK, LDL = BN + 1, APT = BM * BK / 256;
    __shared__ float As[BK * SC_LDA];
    __shared__ float Bs[BK * SC_LDB];
    __shared__ float Ls[BM * LDL];
    __shared__ unsigned long long thr[BM];
    __shared__ int cur[BM], fhi[BM], nxt[BM];
    __shared__ int fl[4][64];
    __shared__ int ent_s[BM];                      // the rows' entities (-1: no such row)
    extern __shared__ unsigned long long lists[];  // [BM][topk]
    const EntityTopkParams& ep = entity_topk_params(pp);
    const GemmParams& p = ep.g;
    const int k = ep.topk;
    const int m0 = blockIdx.x * BM;
    const int col_tiles = (p.n + BN - 1) / BN;
    const int t_begin = blockIdx.y * ep.span_tiles;
    const int t_end = min(t_begin + ep.span_tiles, ep.num_rels * col_tiles);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const bool filtered = ep.filt_lo != nullptr;

    // this thread's share of the query operand: row threadIdx.x / 4 of the tile, APT floats from column (threadIdx.x % 4) * APT on
    const int a_row = m0 + threadIdx.x / (BK / APT), a_col = (threadIdx.x % (BK / APT)) * APT;
    const int a_ent = a_row < p.m ? ep.ents[a_row] : -1;
    const bool a_ok = (unsigned)a_ent < (unsigned)p.n;
    const float* a_src = p.b + (a_ok ? (size_t)a_ent * p.ldb : 0) + a_col;     // (MC: of the sample at hand)
    const float* w_src = ep.w + a_col;             // + r * ld_w
    auto load_q = [&](int k0, float (&r)[APT]) {
        float wv[APT];
        load_run<APT>(a_src + k0, a_col + k0, p.k, a_ok, ep.vec_a, r, 0);
        load_run<APT>(w_src + k0, a_col + k0, p.k, a_ok, ep.vec_a, wv, 0);
#pragma unroll
        for (int i = 0; i < APT; ++i) r[i] *= wv[i];
    };

    TopkPairWalk walk(t_begin, col_tiles);
    float ra[APT], rb[BN * BK / 256];
    if (t_begin < t_end) {
        w_src += (size_t)walk.r * ep.ld_w;
        load_q(0, ra);
        load_b<true, BN, BK>(p, walk.ct * BN, 0, p.k, rb);
    }
    topk_span_clear<BM>(lists, k, fl, thr, lane, wid, [&](int rl) { topk_pair_entity(ep.ents, m0, rl, p.m, p.n, ent_s); });
    const float bv = (!MC && ep.bias) ? *ep.bias : 0.f;

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = walk.ct * BN;
        f32x16 acc;
        TopkPairTile tile;
        if constexpr (MC) {
            const McSamples& mc = pp.mc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            GemmParams ps = p;                                     // b: the table of the sample at hand
            for (int s = 0; s < mc.n_samples; ++s) {
                const f32x16 lg = score_tile_with(ps, load_q, n0, ra, rb, As, Bs);
                const float bs = ep.bias ? ep.bias[s] : 0.f;
                if (s + 1 < mc.n_samples) {                        // the next sample's first operands fly under the sigmoids
                    a_src += mc.e_stride;
                    ps.b += mc.e_stride;
                    load_q(0, ra);
                    load_b<true, BN, BK>(ps, n0, 0, p.k, rb);
                } else {                                           // ... under the last one's, the next tile's of sample 0
                    a_src -= (long long)s * mc.e_stride;
                    tile = walk.step(col_tiles, t == t_begin);
                    if (walk.r != tile.r) w_src += ep.ld_w;
                    if (t + 1 < t_end) {
                        load_q(0, ra);
                        load_b<true, BN, BK>(p, walk.ct * BN, 0, p.k, rb);
                    }
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += mc_sig(lg[i] + bs);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] *= mc.inv_s;
        } else {
            acc = score_tile_with(p, load_q, n0, ra, rb, As, Bs);
            tile = walk.step(col_tiles, t == t_begin);
            if (walk.r != tile.r) w_src += ep.ld_w;
            if (t + 1 < t_end) {                                   // the next tile's first operands fly under the selection
                load_q(0, ra);
                load_b<true, BN, BK>(p, walk.ct * BN, 0, p.k, rb);
            }
        }
        // (every wave is past score_tile's last barrier: nobody still reads the previous relation's cursors, or Ls)
        if (tile.opens && threadIdx.x < BM)
            topk_pair_reopen(ep.filt_lo, ep.filt_hi, ep.filt_ent, ep.n_ent, ent_s, ep.num_rels, tile, cur, fhi, nxt);
#pragma unroll
        for (int i = 0; i < 16; ++i) Ls[(wm + (i & 3) + 8 * (i >> 2) + 4 * lhi) * LDL + wn + l31] = acc[i] + bv;
        __syncthreads();

        const int col = n0 + lane;
        topk_span_select<NK, BM>(m0, p.m, lists, thr, k, lane, wid, [&](int rl, int) {
            const int a = ent_s[rl];
            unsigned long long key = col < p.n ? topk_key(Ls[rl * LDL + lane], tile.r * p.n + col) : 0ull;
            if (filtered && nxt[rl] < n0 + BN &&
                topk_filter_window(ep.filt_ent, n0, (int)((unsigned)(t - t_begin) * BM + rl + 1u), lane, &cur[rl], &fhi[rl], &nxt[rl],
                                   fl[wid]))
                key = 0ull;
            return ep.exclude_self && col == a ? 0ull : key;
        }, [&](int rl) { return ent_s[rl] >= 0; });
    }
    topk_span_hand_on<BM>(m0, p.m, lists, k, ep.part, ep.n_spans, lane, wid);
}

// ---- per-entity completion among TYPE-CORRECT facts (gv_entity_topk_scores_typed) -----------------------------------------------
// k_entity_topk_span with a row's columns taken from the relations' candidate member lists instead of the whole table: the r-major
// sequence of (relation, 64-member tile of set cand_base + r) pairs, sum_r ceil(|C_r| / 64) tiles (TopkTyped, k_topk.h).  A
// workgroup finds its span's first relation by bisection on tile_ptr and walks forward.  The entity operand is GATHERED through
// the tile's 64 ids -- kept in LDS, three buffers deep: the tile at hand (its selection reads them), the next one (its first
// operands are requested under the selection) and the one a slower wave may still be selecting on -- and goes through the same
// k-chunks as score_tile (score_tile_gather), so a candidate's logit is the untyped kernel's, bit for bit.  The candidate id is
// r * N + ids[slot]; the lists ascend, so the key's order is the rule's.  At a relation's (or the span's) first tile thread rl < 64
// decides whether its entity is a member of the query-side set of r (bisection of that list) -- a row that is not is passed over
// -- and re-opens the row's filter cursor at the tile's first id.  The filter of a gathered tile is topk_typed_filter_window: it
// assumes neither that listed ids are members nor that fewer than 64 of them lie between two members.
struct EntityTopkTypedParams {
    EntityTopkParams e;           // span_tiles / n_spans count tiles of the member lists
    TopkTyped ty;
};

struct EntityTopkTypedMcParams {  // MC (gv_entity_topk_scores_typed_mc), as EntityTopkMcParams
    EntityTopkTypedParams t;
    McSamples mc;
};

__device__ __forceinline__ const EntityTopkTypedParams& entity_topk_params(const EntityTopkTypedParams& pp) { return pp; }
__device__ __forceinline__ const EntityTopkTypedParams& entity_topk_params(const EntityTopkTypedMcParams& pp) { return pp.t; }

// MC: k_entity_topk_span's sample loop around score_tile_gather -- the gathered member rows and the query rows both read at
// + s * e_stride -- with the membership test, the id buffers and the filter window outside it.
template <int NK, bool MC = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MC ? 4 : 1))) void k_entity_topk_typed_span(
    const std::conditional_t<MC, EntityTopkTypedMcParams, EntityTopkTypedParams> pp) {
    constexpr int BM = SC_BM, BN = SC_BN, BK = SC_BK, LDL = BN + 1, APT = BM * BK / 256, BPT = BN * BK / 256;
    __shared__ float As[BK * SC_LDA];
    __shared__ float Bs[BK * SC_LDB];
    __shared__ float Ls[BM * LDL];
    __shared__ unsigned long long thr[BM];
    __shared__ int cur[BM], fhi[BM], nxt[BM];
    __shared__ int fl[4][64];
    __shared__ int ent_s[BM];                      // the rows' entities (-1: no such row)
    __shared__ int live_s[BM];                     // the row's entity is on the query side of the relation at hand
    __shared__ int ids_s[3][BN];                   // the member ids of the tile at hand, the next and the previous one (-1: none)
    extern __shared__ unsigned long long lists[];  // [BM][topk]
    const EntityTopkTypedParams& tp = entity_topk_params(pp);
    const EntityTopkParams& ep = tp.e;
    const TopkTyped& ty = tp.ty;
    const GemmParams& p = ep.g;
    const int k = ep.topk, num_rels = ep.num_rels;
    const int m0 = blockIdx.x * BM;
    const int t_begin = blockIdx.y * ep.span_tiles;
    const int t_end = min(t_begin + ep.span_tiles, ty.n_tiles);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const bool filtered = ep.filt_lo != nullptr;

    // this thread's share of the query operand, as k_entity_topk_span forms it
    const int a_row = m0 + threadIdx.x / (BK / APT), a_col = (threadIdx.x % (BK / APT)) * APT;
    const int a_ent = a_row < p.m ? ep.ents[a_row] : -1;
    const bool a_ok = (unsigned)a_ent < (unsigned)p.n;
    const float* a_src = p.b + (a_ok ? (size_t)a_ent * p.ldb : 0) + a_col;
    const float* w_src = ep.w + a_col;             // + r * ld_w
    auto load_q = [&](int k0, float (&r)[APT]) {
        float wv[APT];
        load_run<APT>(a_src + k0, a_col + k0, p.k, a_ok, ep.vec_a, r, 0);
        load_run<APT>(w_src + k0, a_col + k0, p.k, a_ok, ep.vec_a, wv, 0);
#pragma unroll
        for (int i = 0; i < APT; ++i) r[i] *= wv[i];
    };
    // ... and of the entity operand: row threadIdx.x / 4 of the tile is table row ids[threadIdx.x / 4], load_b's columns
    const int b_slot = threadIdx.x / (BK / BPT), b_col = (threadIdx.x % (BK / BPT)) * BPT;
    const float* b_src = p.b + b_col;
    bool b_ok = false;
    auto gather_from = [&](const int* ids) {
        const int id = ids[b_slot];
        b_ok = id >= 0;
        b_src = p.b + (b_ok ? (size_t)id * p.ldb : 0) + b_col;
    };
    auto load_e = [&](int k0, float (&r)[BPT]) { load_run<BPT>(b_src + k0, b_col + k0, p.k, b_ok, p.vec_b, r, 0); };

    TopkTypedTile tile{};
    if (t_begin < t_end) {
        tile = topk_typed_seek(ty, num_rels, t_begin);
        if (threadIdx.x < BN) ids_s[0][threadIdx.x] = topk_typed_id(ty, tile, p.n, threadIdx.x);
    }
    topk_span_clear<BM>(lists, k, fl, thr, lane, wid, [&](int rl) { topk_pair_entity(ep.ents, m0, rl, p.m, p.n, ent_s); });
    __syncthreads();                               // the first tile's ids, ahead of the first gather
    float ra[APT], rb[BPT];
    if (t_begin < t_end) {
        w_src = ep.w + (size_t)tile.r * ep.ld_w + a_col;
        gather_from(ids_s[0]);
        load_q(0, ra);
        load_e(0, rb);
    }
    const float bv = (!MC && ep.bias) ? *ep.bias : 0.f;

    int buf = 0;
    for (int t = t_begin; t < t_end; ++t) {
        const bool more = t + 1 < t_end;
        const int nbuf = buf == 2 ? 0 : buf + 1;
        TopkTypedTile next = tile;
        if (more) {
            // the next tile's ids: its buffer was last read by the selection two tiles back, which every wave left before this
            // wave passed the previous tile's barriers; the barriers below publish it
            next = topk_typed_next(ty, num_rels, tile, t);
            if (threadIdx.x < BN) ids_s[nbuf][threadIdx.x] = topk_typed_id(ty, next, p.n, threadIdx.x);
        }
        f32x16 acc;
        if constexpr (MC) {
            const McSamples& mc = pp.mc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            for (int s = 0; s < mc.n_samples; ++s) {
                const f32x16 lg = score_tile_gather(p, load_q, load_e, ra, rb, As, Bs);
                const float bs = ep.bias ? ep.bias[s] : 0.f;
                if (s + 1 < mc.n_samples) {                        // the next sample's first operands fly under the sigmoids
                    a_src += mc.e_stride;
                    b_src += mc.e_stride;
                    load_q(0, ra);
                    load_e(0, rb);
                } else {                                           // ... under the last one's, the next tile's of sample 0
                    a_src -= (long long)s * mc.e_stride;
                    if (more) {                                    // (gather_from starts over from sample 0's table)
                        w_src = ep.w + (size_t)next.r * ep.ld_w + a_col;
                        gather_from(ids_s[nbuf]);
                        load_q(0, ra);
                        load_e(0, rb);
                    }
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += mc_sig(lg[i] + bs);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] *= mc.inv_s;
        } else {
            acc = score_tile_gather(p, load_q, load_e, ra, rb, As, Bs);
            if (more) {                                            // the next tile's first operands fly under the selection
                w_src = ep.w + (size_t)next.r * ep.ld_w + a_col;
                gather_from(ids_s[nbuf]);
                load_q(0, ra);
                load_e(0, rb);
            }
        }
        const int* ids = ids_s[buf];
        // (every wave is past the tile's last barrier: nobody still reads the previous relation's cursors or flags, or Ls)
        if ((tile.ct == 0 || t == t_begin) && threadIdx.x < BM) {
            const int rl = threadIdx.x, a = ent_s[rl];
            const bool live = a >= 0 && topk_typed_member(ty, num_rels, tile.r, a);
            live_s[rl] = live;
            topk_filter_begin(ep.filt_lo, ep.filt_hi, ep.filt_ent, ep.n_ent, filtered && live, (long long)a * num_rels + tile.r,
                              max(ids[0], 0), &cur[rl], &fhi[rl], &nxt[rl]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) Ls[(wm + (i & 3) + 8 * (i >> 2) + 4 * lhi) * LDL + wn + l31] = acc[i] + bv;
        __syncthreads();

        const int cnt = max(tile.live(), 1);
        const int x = ids[lane], id_max = ids[cnt - 1];
        topk_span_select<NK, BM>(m0, p.m, lists, thr, k, lane, wid, [&](int rl, int) {
            const int a = ent_s[rl];
            unsigned long long key = x >= 0 ? topk_key(Ls[rl * LDL + lane], tile.r * p.n + x) : 0ull;
            if (filtered && nxt[rl] <= id_max &&
                topk_typed_filter_window(ep.filt_ent, ids, cnt, id_max, (int)((unsigned)(t - t_begin) * BM + rl + 1u), lane, &cur[rl],
                                         &fhi[rl], &nxt[rl], fl[wid]))
                key = 0ull;
            return ep.exclude_self && x == a ? 0ull : key;
        }, [&](int rl) { return live_s[rl] != 0; });
        tile = next;
        buf = nbuf;
    }
    topk_span_hand_on<BM>(m0, p.m, lists, k, ep.part, ep.n_spans, lane, wid);
}

// ---- the spread of a selected pair's probability over the samples (gv_pair_prob_std_mc) ----------------------------------
// One thread per pair (i, ids[i, c]): p_s = sig(q_s[i] . e_s[id] + bias[s]) with the dot a plain ascending-k fmaf chain from 0 -- NOT
// the tile's MFMA chain, so p_s may differ from the tile's value in the last bits -- then the two-pass population standard
// deviation in fp32: mean = (sum p_s) / S, std = sqrt((sum (p_s - mean)^2) / S), the p_s recomputed for the second pass (the same
// chain, bit for bit; nothing is stored, S is unbounded).  A padding id (< 0, or >= v) gives 0; S = 1 gives p - p = 0 exactly.
__global__ __launch_bounds__(256) void k_pair_prob_std_mc(const float* q, int ld_q, const float* e, int ld_e, const McSamples mc,
                                                         const float* bias, const int* ids, float* out_std, long long pairs, int k,
                                                         int v, int h) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= pairs) return;
    const int id = ids[i];
    if ((unsigned)id >= (unsigned)v) {
        out_std[i] = 0.f;
        return;
    }
    const float* qr = q + (i / k) * ld_q;
    const float* er = e + (long long)id * ld_e;
    auto prob = [&](int s) {
        const float* a = qr + s * mc.q_stride;
        const float* b = er + s * mc.e_stride;
        float dot = 0.f;
        for (int j = 0; j < h; ++j) dot = fmaf(a[j], b[j], dot);
        return mc_sig(dot + (bias ? bias[s] : 0.f));
    };
    float sum = 0.f;
    for (int s = 0; s < mc.n_samples; ++s) sum += prob(s);
    const float mean = sum / (float)mc.n_samples;
    float dev = 0.f;
    for (int s = 0; s < mc.n_samples; ++s) {
        const float d = prob(s) - mean;
        dev = fmaf(d, d, dev);
    }
    out_std[i] = sqrtf(dev / (float)mc.n_samples);
}

// ---- relation-grouped products for dense per-relation weights (the `basis` regulariser) ----------------
// With W_r = sum_b w_comp[r, b] V_b a full (in x out) matrix, a message is a 2*in*out-flop mat-vec: MFMA work.  Edges are
// taken in BY-RELATION order (ops.RelationIndex.by_rel), so the messages of one relation are one GEMM whose A rows are
// GATHERED through an index (no materialised x[src] copy):
//   rows, TB = false  Msg[p]  = x[src_by_rel[p]] @ W_r           p in relation r's range       (forward)
//   rows, TB = true   Msg2[p] = g[dst_by_rel[p]] @ W_r^T                                       (backward w.r.t. x)
//   gradw             dW_r    = sum_{p in r} x[src_by_rel[p]]^T (norm_p g[dst_by_rel[p]])      (K = the relation's edge range)
// A 64-row tile never crosses a relation boundary: `tiles` lists (first row, end row, relation) per block row.  The
// per-destination sum of the messages (x norm) is the K1 aggregation with 1x1 blocks over Msg (k_bdd.hip), as in DistMult.
struct RelGemmParams {
    const float* a;          // feature table the A rows are gathered from
    const int* a_rows;       // row id per position (by-relation order)
    const float* w;          // [R, in, out] dense relation weights
    float* c;                // rows: [E, n]; gradw: [R, in, out]
    const int4* tiles;       // rows: (row0, row_end, relation, -)
    const float* b_feat;     // gradw: second gathered table (g)
    const int* b_rows;       // gradw: row id per position into b_feat
    const float* b_scale;    // gradw: per-position scale (edge norm in by-relation order), may be NULL
    const int* relptr;       // gradw: [R + 1] position ranges
    int lda, ldb_feat, in_feat, out_feat, n, k;      // rows: C is [*, n], inner dimension k
    int vec;
};

template <bool TB>
__global__ __launch_bounds__(256) void k_rel_rows(const RelGemmParams p) {
    constexpr int BM = 64, BN = 64, BK = 16, LDA_S = BM + 1, LDB_S = BN + 1, APT = 4, BPT = 4;
    __shared__ float As[BK * LDA_S];
    __shared__ float Bs[BK * LDB_S];
    const int4 tile = p.tiles[blockIdx.y];
    const int m0 = tile.x, m_end = tile.y;
    const float* wr = p.w + (size_t)tile.z * p.in_feat * p.out_feat;
    const int ldb = p.out_feat;                           // W_r is [in, out] row-major
    const int n0 = blockIdx.x * BN;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32, l31 = lane & 31, lhi = lane >> 5;
    // A: 4 threads per row (4 consecutive k each); the row pointer is resolved once
    const int am = m0 + t / 4, akk = (t % 4) * APT;
    const bool a_ok = am < m_end;
    const float* arow = p.a + (size_t)(a_ok ? p.a_rows[am] : 0) * p.lda;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float ra[APT], rb[BPT];
    auto load_tiles = [&](int k0) {
        load_run<APT>(arow + k0 + akk, k0 + akk, p.k, a_ok, p.vec, ra, 0);
        if (!TB) {          // B[k][n] = W_r[k][n]: 16 threads per k row
            const int kq = k0 + t / 16, n = n0 + (t % 16) * BPT;
            load_run<BPT>(wr + (size_t)kq * ldb + n, n, p.n, kq < p.k, p.vec, rb, 0);
        } else {            // B[k][n] = W_r[n][k]: 4 threads per n
            const int n = n0 + t / 4, kq = k0 + (t % 4) * BPT;
            load_run<BPT>(wr + (size_t)n * ldb + kq, kq, p.k, n < p.n, p.vec, rb, 0);
        }
    };
    load_tiles(0);
    for (int k0 = 0; k0 < p.k; k0 += BK) {
        stage_a<false, BM, BK>(As, ra);
        stage_b<TB, BN, BK>(Bs, rb);
        __syncthreads();
        if (k0 + BK < p.k) load_tiles(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + lhi) * LDA_S + wm + l31], Bs[(kk + lhi) * LDB_S + wn + l31],
                                                       acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = n0 + wn + l31;
    if (col >= p.n) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (row < m_end) p.c[(size_t)row * p.n + col] = acc[r];
    }
}

// dW_r[i][o] = sum_p x[a_rows[p]][i] * scale_p * g[b_rows[p]][o] over the relation's positions; grid (out/64, in/64, R)
__global__ __launch_bounds__(256) void k_rel_gradw(const RelGemmParams p) {
    constexpr int BM = 64, BN = 64, BK = 16, LDA_S = BM + 1, LDB_S = BN + 1, APT = 4, BPT = 4;
    __shared__ float As[BK * LDA_S];
    __shared__ float Bs[BK * LDB_S];
    const int rel = blockIdx.z;
    const int kbeg = p.relptr[rel], kend = p.relptr[rel + 1];
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32, l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float ra[APT], rb[BPT];
    auto load_tiles = [&](int k0) {      // both operands: 16 threads per position (k), 4 consecutive columns each
        const int kq = k0 + t / 16;
        const bool ok = kq < kend;
        const int m = m0 + (t % 16) * APT, n = n0 + (t % 16) * BPT;
        const float* xa = p.a + (size_t)(ok ? p.a_rows[kq] : 0) * p.lda + m;
        const float* gb = p.b_feat + (size_t)(ok ? p.b_rows[kq] : 0) * p.ldb_feat + n;
        load_run<APT>(xa, m, p.in_feat, ok, p.vec, ra, 0);
        load_run<BPT>(gb, n, p.out_feat, ok, p.vec, rb, 0);
        if (p.b_scale && ok) {
            const float sc = p.b_scale[kq];
#pragma unroll
            for (int i = 0; i < BPT; ++i) rb[i] *= sc;
        }
    };
    if (kbeg < kend) load_tiles(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        stage_a<true, BM, BK>(As, ra);
        stage_b<false, BN, BK>(Bs, rb);
        __syncthreads();
        if (k0 + BK < kend) load_tiles(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(kk + lhi) * LDA_S + wm + l31], Bs[(kk + lhi) * LDB_S + wn + l31],
                                                       acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = n0 + wn + l31;
    if (col >= p.out_feat) return;
    float* cr = p.c + (size_t)rel * p.in_feat * p.out_feat;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (row < p.in_feat) cr[(size_t)row * p.out_feat + col] = acc[r];
    }
}

// ---- bf16-operand variant (BASELINE configs[2]: bf16 with fp32 accumulation) --------------------------------------
// Same contract and epilogue as k_gemm_f32; A and B are read as fp32 from memory, rounded to bf16 (RNE,
// v_cvt_pk_bf16_f32) on their way into LDS and multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulators:
// a bf16 x bf16 product is exact in fp32, so the result equals an fp32 GEMM of the rounded operands up to summation
// order.  Block tile 64 x 64 x 32, four waves 2 x 2, one 32x32 accumulator per wave, two MFMAs per tile.
// LDS holds both tiles k-contiguous, [row][32 k + 8 pad] bf16: the operand fragment of lane l (row l&31, k = 8*(l>>5)
// .. +7) is ONE 16-byte ds_read_b128, conflict-free at the 80-byte row pitch.  Staging: an operand whose k runs
// along memory (A [M,K]; B stored [N,K]) is read as 2 x 16 B per thread; one whose k is the row index (A stored [K,M];
// B [K,N]) as 8 coalesced 4-B loads (64 consecutive rows per wave instruction) -- either way 8 k-values of one row per
// thread, packed into one 16-byte LDS store.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int HB_BK = 32, HB_LD = 40;      // bf16 elements per LDS row (80 B)

// KC: element (row, k) at base[row * ld + k]
__device__ __forceinline__ void hb_load_kc(const float* base, const float* mask, int ld, int row0, int rows, int k0, int kend,
                                           bool vec, float (&r)[8]) {
    const int t = threadIdx.x;
    const int row = row0 + (t >> 2), kk = k0 + (t & 3) * 8;
    const bool ok = row < rows;
    const float* src = base + (size_t)row * ld + kk;
    load_run<8>(src, kk, kend, ok, vec, r, 0);
    if (mask) mask_run<8>(mask + (size_t)row * ld + kk, kk, kend, ok, vec, r);
}

// KS: element (row, k) at base[k * ld + row]
__device__ __forceinline__ void hb_load_ks(const float* base, const float* mask, int ld, int row0, int rows, int k0, int kend,
                                           float (&r)[8]) {
    const int t = threadIdx.x;
    const int row = row0 + (t & 63), kk = k0 + (t >> 6) * 8;
    const bool ok = row < rows;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool in = ok && kk + j < kend;
        float v = in ? base[(size_t)(kk + j) * ld + row] : 0.f;
        if (mask && in) v = mask[(size_t)(kk + j) * ld + row] > 0.f ? v : 0.f;
        r[j] = v;
    }
}

template <bool KC>
__device__ __forceinline__ void hb_stage(__bf16* S, const float (&r)[8]) {
    const int t = threadIdx.x;
    const int row = KC ? (t >> 2) : (t & 63), kk = KC ? (t & 3) * 8 : (t >> 6) * 8;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (__bf16)r[j];
    *reinterpret_cast<bf16x8*>(S + row * HB_LD + kk) = v;
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_gemm_bf16(const GemmParams p) {
    __shared__ __attribute__((aligned(16))) __bf16 As[64 * HB_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[64 * HB_LD];
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int kbeg = blockIdx.z * p.k_chunk;
    const int kend = min(p.k, kbeg + p.k_chunk);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    float ra[8], rb[8];
    auto load_tiles = [&](int k0) {
        if constexpr (!TA) hb_load_kc(p.a, p.a_mask, p.lda, m0, p.m, k0, kend, p.vec_a, ra);
        else hb_load_ks(p.a, p.a_mask, p.lda, m0, p.m, k0, kend, ra);
        if constexpr (TB) hb_load_kc(p.b, nullptr, p.ldb, n0, p.n, k0, kend, p.vec_b, rb);
        else hb_load_ks(p.b, nullptr, p.ldb, n0, p.n, k0, kend, rb);
    };
    load_tiles(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += HB_BK) {
        hb_stage<!TA>(As, ra);
        hb_stage<TB>(Bs, rb);
        __syncthreads();
        if (k0 + HB_BK < kend) load_tiles(k0 + HB_BK);     // next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < HB_BK; kk += 16) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(As + (wm + l31) * HB_LD + kk + 8 * lhi);
            const bf16x8 bf = *reinterpret_cast<const bf16x8*>(Bs + (wn + l31) * HB_LD + kk + 8 * lhi);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = n0 + wn + l31;
    if (col >= p.n) return;
    const float bv = (p.bias && p.split_k == 1) ? p.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (row >= p.m) continue;
        float v = acc[r];
        if (p.split_k > 1) {
            p.ws[((size_t)blockIdx.z * p.m + row) * p.n + col] = v;
        } else {
            v = apply_act(v + bv, p.act);
            float* dst = p.c + (size_t)row * p.ldc + col;
            *dst = p.accumulate ? *dst + v : v;
        }
    }
}

__global__ __launch_bounds__(256) void k_gemm_splitk_reduce(const GemmParams p) {
    const size_t total = (size_t)p.m * p.n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        // 8 partial tiles in flight (4 chains, fixed combine: the order does not depend on the launch geometry)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int z = 0;
        for (; z + 8 <= p.split_k; z += 8) {
            float t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = p.ws[(size_t)(z + q) * total + i];
            a0 += t[0]; a1 += t[1]; a2 += t[2]; a3 += t[3];
            a0 += t[4]; a1 += t[5]; a2 += t[6]; a3 += t[7];
        }
        for (; z < p.split_k; ++z) a0 += p.ws[(size_t)z * total + i];
        float v = (a0 + a1) + (a2 + a3);
        const int row = (int)(i / p.n), col = (int)(i - (size_t)row * p.n);
        if (p.tmask_wanted > 0) {      // no block wrote the partial tiles of an unwanted tile
            const int bit = (row >> 6) * p.tmask_ld + (col >> 6);
            if (!((p.tmask[bit >> 6] >> (bit & 63)) & 1ull)) v = 0.f;
        }
        if (p.bias) v += p.bias[col];
        v = apply_act(v, p.act);
        float* dst = p.c + (size_t)row * p.ldc + col;
        *dst = p.accumulate ? *dst + v : v;
    }
}

// column sums: grid (column tiles of 64, row slices); the 4 waves of a block interleave the slice's rows
// (4 loads in flight per lane), combine through LDS in wave order; a second kernel sums the slices in order.
constexpr int COLSUM_SLICES = 64;

__global__ __launch_bounds__(256) void k_colsum_part(const float* x, const float* msk, int64_t m, int n, int ld, float* part) {
    __shared__ float sm[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t per = (m + gridDim.y - 1) / gridDim.y;
    const int64_t r0 = blockIdx.y * per, r1 = min(m, r0 + per);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (c < n) {
        int64_t r = r0 + w;
        if (msk) {
            for (; r + 12 < r1; r += 16) {
                const float v0 = x[r * ld + c], v1 = x[(r + 4) * ld + c], v2 = x[(r + 8) * ld + c], v3 = x[(r + 12) * ld + c];
                const float m0 = msk[r * ld + c], m1 = msk[(r + 4) * ld + c], m2 = msk[(r + 8) * ld + c], m3 = msk[(r + 12) * ld + c];
                a0 += m0 > 0.f ? v0 : 0.f; a1 += m1 > 0.f ? v1 : 0.f; a2 += m2 > 0.f ? v2 : 0.f; a3 += m3 > 0.f ? v3 : 0.f;
            }
            for (; r < r1; r += 4) a0 += msk[r * ld + c] > 0.f ? x[r * ld + c] : 0.f;
        } else {
            for (; r + 12 < r1; r += 16) {
                const float v0 = x[r * ld + c], v1 = x[(r + 4) * ld + c], v2 = x[(r + 8) * ld + c], v3 = x[(r + 12) * ld + c];
                a0 += v0; a1 += v1; a2 += v2; a3 += v3;
            }
            for (; r < r1; r += 4) a0 += x[r * ld + c];
        }
    }
    sm[w][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (w == 0 && c < n) part[(size_t)blockIdx.y * n + c] = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
}

__global__ __launch_bounds__(256) void k_colsum_final(const float* part, int n, int nsl, float* out, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int s = 0;
    for (; s + 4 <= nsl; s += 4) {
        const float v0 = part[(size_t)s * n + c], v1 = part[(size_t)(s + 1) * n + c];
        const float v2 = part[(size_t)(s + 2) * n + c], v3 = part[(size_t)(s + 3) * n + c];
        a0 += v0; a1 += v1; a2 += v2; a3 += v3;
    }
    for (; s < nsl; ++s) a0 += part[(size_t)s * n + c];
    const float acc = (a0 + a1) + (a2 + a3);
    out[c] = accumulate ? out[c] + acc : acc;
}

// final pass over many slices: 16 columns per 1024-thread block (common.h: sum_slices_16x64)
__global__ __launch_bounds__(1024) void k_colsum_final_wide(const float* part, int n, int nsl, float* out, int accumulate) {
    __shared__ float sm[64][16];
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    const float acc = sum_slices_16x64(part, n, nsl, c, sm);
    if ((threadIdx.x >> 4) == 0 && c < n) colsum_final_store(acc, c, out, accumulate);      // (k_riders.h: a rider does the same)
}

}  // namespace gv

using namespace gv;

static int k_chunk_for(int k, int split_k) {
    int per = (k + split_k - 1) / split_k;
    return ((per + 31) / 32) * 32;
}

extern "C" int64_t gv_gemm_workspace_bytes(int m, int n, int k, int split_k) {
    (void)k;
    return split_k > 1 ? (int64_t)split_k * m * n * (int64_t)sizeof(float) : 0;
}

static int gemm_any(bool bf16, int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b,
                    int ldb, float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                    const float* a_relu_mask, void* workspace, int64_t workspace_bytes, void* stream, const int32_t* rows_dev = nullptr,
                    const uint64_t* kmask = nullptr, const uint64_t* tmask = nullptr, int tiles_wanted = 0) {
    GV_REQUIRE(m >= 0 && n >= 0 && k >= 0, GV_ERR_SHAPE, "gv_gemm_f32: negative size");
    if (m == 0 || n == 0) return GV_OK;
    GV_REQUIRE(c && (k == 0 || (a && b)), GV_ERR_NULL, "gv_gemm_f32: NULL matrix");      // k == 0: act(bias) (+ C), A and B unread
    GV_REQUIRE(lda >= (trans_a ? m : k) && ldb >= (trans_b ? k : n) && ldc >= n, GV_ERR_SHAPE,
               "gv_gemm_f32: leading dimension too small (lda=%d ldb=%d ldc=%d)", lda, ldb, ldc);
    GV_REQUIRE(act == GV_ACT_NONE || act == GV_ACT_RELU, GV_ERR_SHAPE, "gv_gemm_f32: unknown act %d", act);
    if (split_k < 1) split_k = 1;
    if (k == 0) split_k = 1;
    GemmParams p;
    p.a = a; p.b = b; p.c = c; p.bias = bias; p.a_mask = a_relu_mask; p.ws = (float*)workspace;
    p.m = m; p.n = n; p.k = k; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.act = act; p.accumulate = accumulate;
    p.k_chunk = k_chunk_for(k > 0 ? k : 1, split_k);
    split_k = k > 0 ? (k + p.k_chunk - 1) / p.k_chunk : 1;
    p.split_k = split_k;
    p.vec_a = aligned16(a) && (lda % 4 == 0) && (!a_relu_mask || aligned16(a_relu_mask));
    p.vec_b = aligned16(b) && (ldb % 4 == 0);
    p.rows_dev = bf16 ? nullptr : rows_dev;
    GV_REQUIRE(!kmask || (!bf16 && split_k == 1 && k <= 64 * 16), GV_ERR_SHAPE,
               "gv_gemm_f32_sparse: k-chunk words cover fp32 products of k <= 1024 without split-K (k=%d split_k=%d)", k, split_k);
    GV_REQUIRE(!tmask || !bf16, GV_ERR_SHAPE, "gv_gemm_f32_sparse: fp32 only");
    p.kmask = (const unsigned long long*)kmask;
    p.tmask = (const unsigned long long*)tmask;
    p.tmask_ld = (n + 63) / 64;
    GV_REQUIRE(tiles_wanted >= 0 && tiles_wanted <= ((m + 63) / 64) * ((n + 63) / 64), GV_ERR_SHAPE, "gv_gemm_f32_sparse: c_tiles_wanted=%d", tiles_wanted);
    // one block row per WANTED tile (and nothing for the others) where the partial tiles go through the split-K sum, which knows the words too
    p.tmask_wanted = (tmask && tiles_wanted > 0 && split_k > 1) ? tiles_wanted : 0;
    if (split_k > 1) {
        GV_REQUIRE(workspace, GV_ERR_NULL, "gv_gemm_f32: split_k needs a workspace");
        GV_REQUIRE(workspace_bytes >= gv_gemm_workspace_bytes(m, n, k, split_k), GV_ERR_WORKSPACE,
                   "gv_gemm_f32: workspace %lld < %lld bytes", (long long)workspace_bytes,
                   (long long)gv_gemm_workspace_bytes(m, n, k, split_k));
    }
    hipStream_t st = (hipStream_t)stream;
    if (bf16) {
        dim3 grid((n + 63) / 64, (m + 63) / 64, split_k), block(256);
        if (!trans_a && !trans_b) hipLaunchKernelGGL((k_gemm_bf16<false, false>), grid, block, 0, st, p);
        else if (!trans_a && trans_b) hipLaunchKernelGGL((k_gemm_bf16<false, true>), grid, block, 0, st, p);
        else if (trans_a && !trans_b) hipLaunchKernelGGL((k_gemm_bf16<true, false>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((k_gemm_bf16<true, true>), grid, block, 0, st, p);
        int rcb = launch_status("gv_gemm_bf16");
        if (rcb != GV_OK) return rcb;
        if (split_k > 1) {
            const size_t total = (size_t)m * n;
            const int blocks = (int)min((size_t)2048, (total + 255) / 256);
            hipLaunchKernelGGL(k_gemm_splitk_reduce, dim3(blocks), dim3(256), 0, st, p);
            return launch_status("gv_gemm_bf16(split-k reduce)");
        }
        return GV_OK;
    }
    // Tile choice (measured on the C2 shapes, tools/microbench.py): 64-row tiles unless 128-row tiles still give every
    // CU >= 4 blocks; 64-column tiles; BK = 16 for the row-major-A
    // products (K = 200..400), 32 for the split-K weight-gradient products (A stored [K, M], K = nodes).
    static const int mt_env = getenv("GV_GEMM_MT") ? atoi(getenv("GV_GEMM_MT")) : 0;   // tuning knobs
    static const int nt_env = getenv("GV_GEMM_NT") ? atoi(getenv("GV_GEMM_NT")) : 0;
    static const int bk_env = getenv("GV_GEMM_BK") ? atoi(getenv("GV_GEMM_BK")) : 0;
    const int nt = (nt_env == 2 && !kmask && !(tmask && tiles_wanted > 0 && split_k > 1)) ? 2 : 1;        // 128-column tiles measured 8-12 % slower on every C2 shape: opt-in only
    const int bn = 64 * nt;
    const long blocks128 = (long)((n + bn - 1) / bn) * ((m + 127) / 128) * split_k;
    const int mt = p.tmask_wanted ? 1 : (mt_env ? mt_env : (blocks128 >= 1024 ? 2 : 1));
    // with k-chunk words: 16-deep steps = exactly the marked chunks (GV_GEMM_SPARSE_BK=32: 32-deep steps walked when either half is
    // marked -- measured the same, 66 us on the 500 x 500 MADE layer against 92 dense)
    static const int sparse_bk = getenv("GV_GEMM_SPARSE_BK") ? atoi(getenv("GV_GEMM_SPARSE_BK")) : 16;
    const int bk = kmask ? (sparse_bk == 32 ? 32 : 16) : (bk_env ? (bk_env == 16 ? 16 : 32) : (trans_a ? 32 : 16));
    dim3 grid((n + bn - 1) / bn, (m + 64 * mt - 1) / (64 * mt), split_k), block(256);
    if (p.tmask_wanted) { grid.x = p.tmask_wanted; grid.y = 1; }
#define GV_GEMM_CFG(TA_, TB_, MT_, NT_, BK_) \
    if (mt == MT_ && nt == NT_ && bk == BK_) hipLaunchKernelGGL((k_gemm_f32<TA_, TB_, MT_, NT_, BK_>), grid, block, 0, st, p);
#define GV_GEMM_LAUNCH(TA_, TB_)                                                                       \
    do {                                                                                               \
        GV_GEMM_CFG(TA_, TB_, 1, 1, 16) GV_GEMM_CFG(TA_, TB_, 1, 1, 32) GV_GEMM_CFG(TA_, TB_, 1, 2, 16) \
        GV_GEMM_CFG(TA_, TB_, 1, 2, 32) GV_GEMM_CFG(TA_, TB_, 2, 1, 16) GV_GEMM_CFG(TA_, TB_, 2, 1, 32) \
        GV_GEMM_CFG(TA_, TB_, 2, 2, 16) GV_GEMM_CFG(TA_, TB_, 2, 2, 32)                                 \
    } while (0)
    if (!trans_a && !trans_b) GV_GEMM_LAUNCH(false, false);
    else if (!trans_a && trans_b) GV_GEMM_LAUNCH(false, true);
    else if (trans_a && !trans_b) GV_GEMM_LAUNCH(true, false);
    else GV_GEMM_LAUNCH(true, true);
#undef GV_GEMM_LAUNCH
#undef GV_GEMM_CFG
    int rc = launch_status("gv_gemm_f32");
    if (rc != GV_OK) return rc;
    if (split_k > 1) {
        const size_t total = (size_t)m * n;
        const int blocks = (int)min((size_t)2048, (total + 255) / 256);
        hipLaunchKernelGGL(k_gemm_splitk_reduce, dim3(blocks), dim3(256), 0, st, p);
        return launch_status("gv_gemm_f32(split-k reduce)");
    }
    return GV_OK;
}

extern "C" int gv_gemm_f32(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b,
                           int ldb, float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                           const float* a_relu_mask, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemm_any(false, trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask,
                    workspace, workspace_bytes, stream);
}

// ---- the product with riders (k_riders.h) ----------------------------------------------------------------------------------------
namespace {
struct Extent { const char* lo; const char* hi; };      // [lo, hi) in bytes; lo == NULL: nothing
inline Extent extent_of(const void* p, int64_t bytes) {
    return p && bytes > 0 ? Extent{(const char*)p, (const char*)p + bytes} : Extent{nullptr, nullptr};
}
inline bool overlaps(const Extent& a, const Extent& b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }
inline int64_t matrix_bytes(int rows, int cols, int ld) { return rows > 0 && cols > 0 ? ((int64_t)(rows - 1) * ld + cols) * 4 : 0; }
}  // namespace

static const gv_riders NO_RIDERS = {};

// riders: the forward head's kinds; fin (gv_gemm_f32_riders_fin only): the prior sampler and the backward's gradient finishers
static int gemm_riders(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b, int ldb,
                       float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                       const float* a_relu_mask, void* workspace, int64_t workspace_bytes, const gv_riders* riders,
                       const gv_riders_fin* fin, void* stream) {
    const bool any_fin = fin && (fin->prior_z_pre || fin->kl_part || fin->cs_part);
    const bool any = (riders && (riders->rng_jobs > 0 || riders->pack_weight || riders->mix_z_pre)) || any_fin;
    if (!any)       // no riders: the plain kernel, exactly as gv_gemm_f32 launches it
        return gemm_any(false, trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask,
                        workspace, workspace_bytes, stream);
    if (!riders) riders = &NO_RIDERS;
    GV_REQUIRE(split_k <= 1, GV_ERR_SHAPE, "gv_gemm_f32_riders: riders do not ride on a split-K product (split_k=%d)", split_k);
    GV_REQUIRE(!trans_a && (!trans_b || fin), GV_ERR_SHAPE,
               "gv_gemm_f32_riders: riders ride on A @ B (the forward self-loop product) and, through gv_gemm_f32_riders_fin, on "
               "A @ B^T (the backward's) only");
    GV_REQUIRE(m > 0 && n > 0 && k >= 0, GV_ERR_SHAPE, "gv_gemm_f32_riders: m=%d n=%d k=%d", m, n, k);
    GV_REQUIRE(c && (k == 0 || (a && b)), GV_ERR_NULL, "gv_gemm_f32_riders: NULL matrix");
    GV_REQUIRE(lda >= k && ldb >= (trans_b ? k : n) && ldc >= n, GV_ERR_SHAPE,
               "gv_gemm_f32_riders: leading dimension too small (lda=%d ldb=%d ldc=%d)", lda, ldb, ldc);
    GV_REQUIRE(act == GV_ACT_NONE || act == GV_ACT_RELU, GV_ERR_SHAPE, "gv_gemm_f32_riders: unknown act %d", act);
    GemmParams p;
    p.a = a; p.b = b; p.c = c; p.bias = bias; p.a_mask = a_relu_mask; p.ws = nullptr;
    p.m = m; p.n = n; p.k = k; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.act = act; p.accumulate = accumulate;
    p.k_chunk = k_chunk_for(k > 0 ? k : 1, 1);
    p.split_k = 1;
    p.vec_a = aligned16(a) && (lda % 4 == 0) && (!a_relu_mask || aligned16(a_relu_mask));
    p.vec_b = aligned16(b) && (ldb % 4 == 0);
    p.rows_dev = nullptr; p.kmask = nullptr; p.tmask = nullptr; p.tmask_ld = (n + 63) / 64; p.tmask_wanted = 0;
    // the tile rule of gv_gemm_f32 for A @ B: 64-column tiles, 16-deep steps, 128-row tiles once they still give every CU >= 4 blocks
    const int ntn = (n + 63) / 64;
    const int mt = (long)ntn * ((m + 127) / 128) >= 1024 ? 2 : 1;
    const int ntm = (m + 64 * mt - 1) / (64 * mt);
    GV_REQUIRE((int64_t)ntn * ntm < (1ll << 30), GV_ERR_SHAPE, "gv_gemm_f32_riders: %d x %d tiles", ntn, ntm);

    // what the product reads and writes, against what the riders read and write
    const Extent ea = extent_of(a, matrix_bytes(m, k, lda)), eb = extent_of(b, trans_b ? matrix_bytes(n, k, ldb) : matrix_bytes(k, n, ldb)),
                 ec = extent_of(c, matrix_bytes(m, n, ldc)), ebias = extent_of(bias, (int64_t)n * 4),
                 emask = extent_of(a_relu_mask, matrix_bytes(m, k, lda));
    auto written_ok = [&](const Extent& w) { return !(overlaps(w, ea) || overlaps(w, eb) || overlaps(w, ec) || overlaps(w, ebias) || overlaps(w, emask)); };
    auto read_ok = [&](const Extent& r) { return !overlaps(r, ec); };

    RiderSet rs;
    memset(&rs, 0, sizeof(rs));
    // the measured defaults: see NOTES.md ("Riders on the forward self-loop products")
    static const int per_thread = getenv("GV_RIDER_GROUPS") ? std::max(1, atoi(getenv("GV_RIDER_GROUPS"))) : 8;
    static const int front = getenv("GV_RIDERS_FRONT") ? atoi(getenv("GV_RIDERS_FRONT")) : 1;
    int nblk = 0;
    rs.first[0] = 0;
    if (riders->rng_jobs > 0) {
        GV_REQUIRE(riders->rng_state, GV_ERR_NULL, "gv_gemm_f32_riders: NULL rng_state");
        GV_REQUIRE(riders->rng_jobs <= GV_RNG_MAX_JOBS, GV_ERR_SHAPE, "gv_gemm_f32_riders: rng_jobs=%d (1..%d)", riders->rng_jobs,
                   GV_RNG_MAX_JOBS);
        GV_REQUIRE(read_ok(extent_of(riders->rng_state, 16)), GV_ERR_SHAPE, "gv_gemm_f32_riders: rng_state overlaps C");
        rs.rng_state = riders->rng_state;
        long long g = 0;
        for (int j = 0; j < GV_RNG_MAX_JOBS; ++j) {
            rs.rng.group0[j] = g;
            if (j >= riders->rng_jobs) continue;
            void* ptr = riders->rng_ptr[j];
            const int64_t cnt = riders->rng_count[j];
            const int kind = riders->rng_kind[j];
            const float dp = riders->rng_drop_p[j];
            GV_REQUIRE(ptr && cnt > 0 && cnt < (1ll << 34), GV_ERR_SHAPE, "gv_gemm_f32_riders: rng job %d: bad buffer/count", j);
            GV_REQUIRE(kind == GV_RNG_KEEP_MASK || kind == GV_RNG_NORMAL, GV_ERR_SHAPE, "gv_gemm_f32_riders: rng job %d: kind %d", j, kind);
            GV_REQUIRE((reinterpret_cast<uintptr_t>(ptr) & (kind == GV_RNG_NORMAL ? 15u : 3u)) == 0, GV_ERR_ALIGN,
                       "gv_gemm_f32_riders: rng job %d: buffer alignment", j);
            GV_REQUIRE(kind == GV_RNG_NORMAL || (dp >= 0.f && dp < 1.f), GV_ERR_SHAPE, "gv_gemm_f32_riders: rng job %d: p=%f", j, dp);
            GV_REQUIRE(written_ok(extent_of(ptr, cnt * (kind == GV_RNG_NORMAL ? 4 : 1))), GV_ERR_SHAPE,
                       "gv_gemm_f32_riders: rng job %d writes into an operand of the product", j);
            rs.rng.ptr[j] = ptr; rs.rng.n[j] = cnt; rs.rng.kind[j] = kind; rs.rng.stream[j] = riders->rng_stream[j];
            const double th = (double)dp * 4294967296.0;          // as gv_rng_fill
            rs.rng.thresh[j] = th >= 4294967295.0 ? 4294967295u : (uint32_t)th;
            g += (cnt + 3) / 4;
        }
        rs.rng.group0[GV_RNG_MAX_JOBS] = g;
        for (int j = riders->rng_jobs; j <= GV_RNG_MAX_JOBS; ++j) rs.rng.group0[j] = g;
        rs.rng.n_jobs = riders->rng_jobs;
        const long long want = (g + 256ll * per_thread - 1) / (256ll * per_thread);
        nblk += (int)std::min<long long>(std::max<long long>(want, 1), 1 << 16);
    }
    rs.first[1] = nblk;
    if (riders->pack_weight) {
        const int nb = riders->pack_bases, bi = riders->pack_blk_in, bo = riders->pack_blk_out, r = riders->pack_rels;
        GV_REQUIRE(riders->packed, GV_ERR_NULL, "gv_gemm_f32_riders: NULL packed");
        GV_REQUIRE(r > 0 && nb > 0 && bi > 0 && bo > 0 && (int64_t)r * nb * bi * bo < (1ll << 31), GV_ERR_SHAPE,
                   "gv_gemm_f32_riders: pack shape R=%d nb=%d %dx%d", r, nb, bi, bo);
        GV_REQUIRE(!riders->packed_pair || !riders->pack_transpose, GV_ERR_SHAPE,
                   "gv_gemm_f32_riders: the pair is (blk_in, blk_out, transpose 0) + its backward-x layout");
        PackJob& pj = rs.pack;
        GV_REQUIRE(pack_job_plan(nb, bi, bo, riders->pack_transpose != 0, &pj.bpl, &pj.adj) &&
                       (!riders->packed_pair || pack_job_plan(nb, bo, bi, true, &pj.bpl2, &pj.adj2)),
                   GV_ERR_SHAPE, "gv_gemm_f32_riders: no lane-packed kernel for num_bases=%d blocks %dx%d trans=%d", nb, bi, bo,
                   riders->pack_transpose);
        GV_REQUIRE(aligned16(riders->pack_weight) && aligned16(riders->packed) && aligned16(riders->packed_pair), GV_ERR_ALIGN,
                   "gv_gemm_f32_riders: pack buffers need 16-B alignment");
        const int64_t wbytes = (int64_t)r * nb * bi * bo * 4;
        const Extent ew = extent_of(riders->pack_weight, wbytes), e1 = extent_of(riders->packed, wbytes),
                     e2 = extent_of(riders->packed_pair, wbytes);
        GV_REQUIRE(read_ok(ew) && written_ok(e1) && written_ok(e2) && !overlaps(ew, e1) && !overlaps(ew, e2) && !overlaps(e1, e2),
                   GV_ERR_SHAPE, "gv_gemm_f32_riders: a pack buffer overlaps an operand of the product or another pack buffer");
        pj.w = riders->pack_weight; pj.packed = riders->packed; pj.packed2 = riders->packed_pair;
        pj.num_rels = r; pj.nb = nb; pj.pq = bi * bo;
        const int total = r * nb * bi * bo / 4;
        pj.blocks = std::min(2048, (total + 255) / 256);
        nblk += pj.blocks * (riders->packed_pair ? 2 : 1);
    }
    rs.first[2] = nblk;
    if (riders->mix_z_pre) {
        const int mk = riders->mix_k, mh = riders->mix_h;
        GV_REQUIRE(riders->mix, GV_ERR_NULL, "gv_gemm_f32_riders: NULL mix");
        GV_REQUIRE(mk > 0 && mh > 0 && (int64_t)mk * mh < (1ll << 28), GV_ERR_SHAPE, "gv_gemm_f32_riders: mix k=%d h=%d", mk, mh);
        const Extent ez = extent_of(riders->mix_z_pre, (int64_t)2 * mk * mh * 4), em = extent_of(riders->mix, (int64_t)3 * mk * mh * 4);
        GV_REQUIRE(read_ok(ez) && written_ok(em) && !overlaps(ez, em), GV_ERR_SHAPE,
                   "gv_gemm_f32_riders: a mix buffer overlaps an operand of the product or z_pre");
        rs.mix.z_pre = riders->mix_z_pre; rs.mix.mix = riders->mix; rs.mix.k = mk; rs.mix.h = mh;
        nblk += (mk * mh + 255) / 256;
    }
    rs.first[3] = nblk;
    // what the finishers write, against each other
    Extent fin_out[3] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    if (any_fin && fin->prior_z_pre) {
        const int s = fin->prior_s, pk = fin->prior_k, ph = fin->prior_h;
        GV_REQUIRE(fin->prior_eps && fin->prior_out, GV_ERR_NULL, "gv_gemm_f32_riders_fin: NULL prior buffer");
        GV_REQUIRE(s > 0 && pk > 0 && ph > 0 && (int64_t)s * ph < (1ll << 28) && (int64_t)pk * ph < (1ll << 28), GV_ERR_SHAPE,
                   "gv_gemm_f32_riders_fin: prior s=%d k=%d h=%d", s, pk, ph);
        const Extent ez = extent_of(fin->prior_z_pre, (int64_t)2 * pk * ph * 4), ee = extent_of(fin->prior_eps, (int64_t)s * ph * 4),
                     eo = extent_of(fin->prior_out, (int64_t)s * ph * 4);
        GV_REQUIRE(read_ok(ez) && read_ok(ee) && written_ok(eo) && !overlaps(eo, ez) && !overlaps(eo, ee), GV_ERR_SHAPE,
                   "gv_gemm_f32_riders_fin: a prior sampler buffer overlaps an operand of the product or its own input");
        // its noise must be complete before this launch: a draw of the same launch is no such thing
        for (int j = 0; j < riders->rng_jobs; ++j) {
            const Extent ej = extent_of(riders->rng_ptr[j], riders->rng_count[j] * (riders->rng_kind[j] == GV_RNG_NORMAL ? 4 : 1));
            GV_REQUIRE(!overlaps(ej, ee) && !overlaps(ej, ez) && !overlaps(ej, eo), GV_ERR_SHAPE,
                       "gv_gemm_f32_riders_fin: the prior sampler reads or writes what rng job %d of the same launch writes", j);
        }
        GV_REQUIRE(!overlaps(eo, extent_of(riders->mix, (int64_t)3 * riders->mix_k * riders->mix_h * 4)), GV_ERR_SHAPE,
                   "gv_gemm_f32_riders_fin: the prior samples overlap the mixture table");
        rs.prior.z_pre = fin->prior_z_pre; rs.prior.eps = fin->prior_eps; rs.prior.out = fin->prior_out;
        rs.prior.s = s; rs.prior.k = pk; rs.prior.h = ph;
        fin_out[0] = eo;
        nblk += (s * ph + 255) / 256;                  // as gv_prior_sample_fwd's grid
    }
    rs.first[4] = nblk;
    if (any_fin && fin->kl_part) {
        const int kh_ = fin->kl_h, kk = fin->kl_k, nsl = fin->kl_slices;
        GV_REQUIRE(fin->kl_z_pre && fin->kl_g_zpre, GV_ERR_NULL, "gv_gemm_f32_riders_fin: NULL KL finisher buffer");
        GV_REQUIRE(kh_ > 0 && kk > 0 && nsl > 0 && fin->kl_n > 0 && (int64_t)(2 * kk + 2) * kh_ < (1ll << 28), GV_ERR_SHAPE,
                   "gv_gemm_f32_riders_fin: KL finisher n=%lld h=%d k=%d slices=%d", (long long)fin->kl_n, kh_, kk, nsl);
        const int cols = (2 * kk + (fin->kl_g_bias ? 2 : 0)) * kh_;
        const Extent ep = extent_of(fin->kl_part, (int64_t)nsl * cols * 4), ez = extent_of(fin->kl_z_pre, (int64_t)2 * kk * kh_ * 4),
                     eg = extent_of(fin->kl_gkl, 4), eo = extent_of(fin->kl_g_zpre, (int64_t)2 * kk * kh_ * 4),
                     ebo = extent_of(fin->kl_g_bias, (int64_t)2 * kh_ * 4);
        GV_REQUIRE(read_ok(ep) && read_ok(ez) && read_ok(eg) && written_ok(eo) && written_ok(ebo) && !overlaps(eo, ebo) &&
                       !overlaps(eo, ep) && !overlaps(eo, ez) && !overlaps(eo, eg) && !overlaps(ebo, ep) && !overlaps(ebo, ez) &&
                       !overlaps(ebo, eg) && !overlaps(eo, fin_out[0]) && !overlaps(ebo, fin_out[0]),
                   GV_ERR_SHAPE, "gv_gemm_f32_riders_fin: a KL finisher buffer overlaps an operand of the product or another rider buffer");
        KlFinJob& kj = rs.klfin;
        kj.part = fin->kl_part; kj.z_pre = fin->kl_z_pre; kj.gkl = fin->kl_gkl; kj.gscale = fin->kl_gscale;
        kj.g_zpre = fin->kl_g_zpre; kj.g_bias = fin->kl_g_bias; kj.n = fin->kl_n; kj.accumulate = fin->kl_accumulate;
        kj.accumulate_bias = fin->kl_accumulate_bias; kj.h = kh_; kj.k = kk; kj.nsl = nsl;
        fin_out[1] = eo; fin_out[2] = ebo;
        nblk += (cols + 15) / 16;                      // 16 columns per workgroup, as k_kl_bwd_mix_final's blocks
    }
    rs.first[5] = nblk;
    if (any_fin && fin->cs_part) {
        const int cn = fin->cs_n, nsl = fin->cs_slices;
        GV_REQUIRE(fin->cs_out, GV_ERR_NULL, "gv_gemm_f32_riders_fin: NULL column-sum target");
        GV_REQUIRE(cn > 0 && nsl > 0 && (int64_t)cn * nsl < (1ll << 28), GV_ERR_SHAPE, "gv_gemm_f32_riders_fin: column sums n=%d slices=%d",
                   cn, nsl);
        const Extent ep = extent_of(fin->cs_part, (int64_t)nsl * cn * 4), eo = extent_of(fin->cs_out, (int64_t)cn * 4);
        GV_REQUIRE(read_ok(ep) && written_ok(eo) && !overlaps(eo, ep) && !overlaps(eo, fin_out[0]) && !overlaps(eo, fin_out[1]) &&
                       !overlaps(eo, fin_out[2]) && !overlaps(ep, fin_out[0]) && !overlaps(ep, fin_out[1]) && !overlaps(ep, fin_out[2]),
                   GV_ERR_SHAPE, "gv_gemm_f32_riders_fin: a column-sum buffer overlaps an operand of the product or another rider buffer");
        rs.colsum.part = fin->cs_part; rs.colsum.out = fin->cs_out; rs.colsum.n = cn; rs.colsum.nsl = nsl;
        rs.colsum.accumulate = fin->cs_accumulate;
        nblk += (cn + 15) / 16;
    }
    rs.first[6] = nblk;
    // riders in front: pad their count to a multiple of 8, so that tile workgroup i keeps XCD i % 8 (the padding blocks leave at once)
    const int n_riders = front ? (nblk + 7) / 8 * 8 : nblk;
    const dim3 grid((unsigned)(ntn * ntm + n_riders)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define GV_RIDERS_LAUNCH(TB_, MT_) \
    hipLaunchKernelGGL((k_gemm_f32_riders<false, TB_, MT_, 1, 16>), grid, block, 0, st, p, rs, ntn, ntm, n_riders, front ? 1 : 0)
    if (trans_b) { if (mt == 2) GV_RIDERS_LAUNCH(true, 2); else GV_RIDERS_LAUNCH(true, 1); }
    else { if (mt == 2) GV_RIDERS_LAUNCH(false, 2); else GV_RIDERS_LAUNCH(false, 1); }
#undef GV_RIDERS_LAUNCH
    return launch_status("gv_gemm_f32_riders");
}

extern "C" int gv_gemm_f32_riders(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b, int ldb,
                                  float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                                  const float* a_relu_mask, void* workspace, int64_t workspace_bytes, const gv_riders* riders,
                                  void* stream) {
    return gemm_riders(trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask, workspace,
                       workspace_bytes, riders, nullptr, stream);
}

extern "C" int gv_gemm_f32_riders_fin(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b, int ldb,
                                      float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                                      const float* a_relu_mask, void* workspace, int64_t workspace_bytes, const gv_riders* riders,
                                      const gv_riders_fin* fin, void* stream) {
    static const gv_riders_fin none = {};
    return gemm_riders(trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask, workspace,
                       workspace_bytes, riders, fin ? fin : &none, stream);
}

extern "C" int gv_gemm_f32_live_rows(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b,
                                     int ldb, float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                                     const float* a_relu_mask, void* workspace, int64_t workspace_bytes, const int32_t* rows_dev,
                                     void* stream) {
    return gemm_any(false, trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask,
                    workspace, workspace_bytes, stream, rows_dev);
}

extern "C" int gv_gemm_f32_sparse(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b, int ldb,
                                  float* c, int ldc, const float* bias, int act, int accumulate, int split_k, const float* a_relu_mask,
                                  void* workspace, int64_t workspace_bytes, const int32_t* rows_dev, const uint64_t* b_k_chunks,
                                  const uint64_t* c_tiles, int c_tiles_wanted, void* stream) {
    return gemm_any(false, trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask,
                    workspace, workspace_bytes, stream, rows_dev, b_k_chunks, c_tiles, c_tiles_wanted);
}

extern "C" int gv_gemm_bf16(int trans_a, int trans_b, int m, int n, int k, const float* a, int lda, const float* b,
                            int ldb, float* c, int ldc, const float* bias, int act, int accumulate, int split_k,
                            const float* a_relu_mask, void* workspace, int64_t workspace_bytes, void* stream) {
    return gemm_any(true, trans_a, trans_b, m, n, k, a, lda, b, ldb, c, ldc, bias, act, accumulate, split_k, a_relu_mask,
                    workspace, workspace_bytes, stream);
}

// the product behind every entity query: S = Q (m x h) @ E^T (E stored [v, h]), nothing stored, no epilogue
static GemmParams score_gemm_params(const float* q, int ld_q, const float* e, int ld_e, int m, int v, int h) {
    GemmParams p;
    p.a = q; p.b = e; p.c = nullptr; p.bias = nullptr; p.a_mask = nullptr; p.ws = nullptr;
    p.m = m; p.n = v; p.k = h; p.lda = ld_q; p.ldb = ld_e; p.ldc = v;
    p.act = GV_ACT_NONE; p.accumulate = 0; p.split_k = 1; p.k_chunk = h;
    p.vec_a = aligned16(q) && (ld_q % 4 == 0);
    p.vec_b = aligned16(e) && (ld_e % 4 == 0);
    p.rows_dev = nullptr; p.kmask = nullptr; p.tmask = nullptr; p.tmask_ld = 0; p.tmask_wanted = 0;
    return p;
}

// ---- Monte-Carlo posterior-predictive ranking and top-k (gv_rank_scores_mc, gv_topk_scores_mc, gv_pair_prob_std_mc) -----------
// the sample geometry shared by the three entries: n_samples >= 1, and with more than one sample each stride spans its matrix
static int mc_samples_args(const char* name, const float* q, int ld_q, int64_t q_stride, const float* e, int ld_e, int64_t e_stride,
                           int n_samples, int m, int v, int h, McSamples* mc) {
    GV_REQUIRE(n_samples >= 1, GV_ERR_SHAPE, "%s: n_samples=%d", name, n_samples);
    GV_REQUIRE(ld_q >= h && ld_e >= h, GV_ERR_SHAPE, "%s: leading dimension too small", name);
    GV_REQUIRE(n_samples == 1 || (q_stride >= (int64_t)(m > 0 ? m - 1 : 0) * ld_q + h && e_stride >= (int64_t)(v - 1) * ld_e + h),
               GV_ERR_SHAPE, "%s: sample stride shorter than the rows it spans (q_stride=%lld e_stride=%lld)", name,
               (long long)q_stride, (long long)e_stride);
    mc->q_stride = n_samples > 1 ? q_stride : 0;
    mc->e_stride = n_samples > 1 ? e_stride : 0;
    mc->n_samples = n_samples;
    mc->inv_s = 1.0f / (float)n_samples;
    return GV_OK;
}

// score_gemm_params for sample 0; the 16-byte loads need every sample's base aligned (no samples: strides 0, score_gemm_params')
static GemmParams mc_gemm_params(const float* q, int ld_q, const float* e, int ld_e, const McSamples& mc, int m, int v, int h) {
    GemmParams p = score_gemm_params(q, ld_q, e, ld_e, m, v, h);
    p.vec_a = p.vec_a && mc.q_stride % 4 == 0;
    p.vec_b = p.vec_b && mc.e_stride % 4 == 0;
    return p;
}

// The launches of every ranker; mc.n_samples == 0: not Monte-Carlo.  Pass 0 writes tgt[row], the target's logit or pbar (it does not
// depend on filter or set); pass 1 votes all its counts on the one value.  Without a filter the filtered counts are not written.
// Single-sample: gv_rank_scores (no filter, no set) runs the raw count alone, with no filter word to build.
static int rank_launch(const char* name, const McSamples& mc, const float* q, int ld_q, const float* e, int ld_e, const int* target,
                       const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent,
                       const TopkCand& cs, float* tgt, int* count_raw, int* count_filt, int* count_raw_c, int* count_filt_c, int m,
                       int v, int h, void* stream) {
    RankFiltParams fp{};
    RankParams& rp = fp.rp;
    fp.mc = mc;
    rp.g = mc_gemm_params(q, ld_q, e, ld_e, mc, m, v, h);
    rp.target = target; rp.bias = bias; rp.tgt = tgt; rp.count = count_raw;
    fp.filt_lo = filt_lo; fp.filt_hi = filt_hi; fp.filt_ent = filt_ent; fp.n_ent = n_filt_ent;
    fp.count_filt = filt_lo ? count_filt : nullptr;
    fp.cs = cs;
    fp.count_raw_c = count_raw_c; fp.count_filt_c = filt_lo ? count_filt_c : nullptr;
    hipStream_t st = (hipStream_t)stream;
    for (int* c : {count_raw, fp.count_filt, fp.count_raw_c, fp.count_filt_c})
        if (c && fill_words(c, 0u, (size_t)m * sizeof(int), st) != hipSuccess) return launch_status(name);
    dim3 grid((v + 63) / 64, (m + 63) / 64), block(256);
    if (mc.n_samples) {
        hipLaunchKernelGGL(k_rank_target_mc, grid, block, 0, st, fp);
        if (cs.cand) hipLaunchKernelGGL((k_rank_scores_filtered<true, true>), grid, block, 0, st, fp);
        else hipLaunchKernelGGL((k_rank_scores_filtered<false, true>), grid, block, 0, st, fp);
    } else {
        hipLaunchKernelGGL(k_rank_scores<0>, grid, block, 0, st, rp);
        if (!fp.count_filt && !cs.cand) hipLaunchKernelGGL(k_rank_scores<1>, grid, block, 0, st, rp);
        else if (cs.cand) hipLaunchKernelGGL(k_rank_scores_filtered<true>, grid, block, 0, st, fp);
        else hipLaunchKernelGGL(k_rank_scores_filtered<false>, grid, block, 0, st, fp);
    }
    return launch_status(name);
}

extern "C" int gv_rank_scores(const float* q, int ld_q, const float* e, int ld_e, const int* target, const float* bias,
                              float* tgt, int* count, int m, int v, int h, void* stream) {
    const char* name = "gv_rank_scores";
    GV_CHECK(query_sizes(name, m, v, h));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && target && tgt && count));
    GV_CHECK(query_leading(name, ld_q, ld_e, h));
    return rank_launch(name, McSamples{}, q, ld_q, e, ld_e, target, bias, nullptr, nullptr, nullptr, 0, TopkCand{}, tgt, count, nullptr,
                       nullptr, nullptr, m, v, h, stream);
}

extern "C" int gv_rank_scores_filtered(const float* q, int ld_q, const float* e, int ld_e, const int* target, const float* bias,
                                       const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent, float* tgt,
                                       int* count_raw, int* count_filt, int m, int v, int h, void* stream) {
    const char* name = "gv_rank_scores_filtered";
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && target && tgt && count_filt));
    GV_REQUIRE(filt_lo && filt_hi && filt_ent, GV_ERR_NULL, "gv_rank_scores_filtered: NULL filter pointer");
    GV_CHECK(query_leading(name, ld_q, ld_e, h));
    return rank_launch(name, McSamples{}, q, ld_q, e, ld_e, target, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, TopkCand{}, tgt,
                       count_raw, count_filt, nullptr, nullptr, m, v, h, stream);
}

extern "C" int gv_rank_scores_constrained(const float* q, int ld_q, const float* e, int ld_e, const int* target, const float* bias,
                                          const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent,
                                          const uint32_t* cand, int ld_cand, int n_sets, const int32_t* cand_set, float* tgt,
                                          int* count_raw, int* count_filt, int* count_raw_c, int* count_filt_c, int m, int v, int h,
                                          void* stream) {
    const char* name = "gv_rank_scores_constrained";
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(query_cand_shape(name, n_sets, ld_cand, v));
    GV_CHECK(query_leading(name, ld_q, ld_e, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    GV_CHECK(query_cand_given(name, cand, cand_set));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && target && tgt && count_raw && count_raw_c));
    GV_CHECK(query_filter_needs(name, filt_lo, count_filt && count_filt_c, "both filtered counts"));
    return rank_launch(name, McSamples{}, q, ld_q, e, ld_e, target, bias, filt_lo, filt_hi, filt_ent, n_filt_ent,
                       TopkCand{cand, cand_set, ld_cand, n_sets}, tgt, count_raw, count_filt, count_raw_c, count_filt_c, m, v, h, stream);
}

extern "C" int gv_rank_scores_mc(const float* q, int ld_q, int64_t q_stride, const float* e, int ld_e, int64_t e_stride, int n_samples,
                                 const int* target, const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_ent,
                                 int n_filt_ent, float* tgt, int* count_raw, int* count_filt, int m, int v, int h, void* stream) {
    const char* name = "gv_rank_scores_mc";
    McSamples mc;
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(mc_samples_args(name, q, ld_q, q_stride, e, ld_e, e_stride, n_samples, m, v, h, &mc));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && target && tgt && count_raw));
    GV_CHECK(query_filter_needs(name, filt_lo, count_filt, "count_filt"));
    return rank_launch(name, mc, q, ld_q, e, ld_e, target, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, TopkCand{}, tgt, count_raw,
                       count_filt, nullptr, nullptr, m, v, h, stream);
}

extern "C" int gv_rank_scores_mc_constrained(const float* q, int ld_q, int64_t q_stride, const float* e, int ld_e, int64_t e_stride,
                                             int n_samples, const int* target, const float* bias, const int* filt_lo,
                                             const int* filt_hi, const int* filt_ent, int n_filt_ent, const uint32_t* cand,
                                             int ld_cand, int n_sets, const int32_t* cand_set, float* tgt, int* count_raw,
                                             int* count_filt, int* count_raw_c, int* count_filt_c, int m, int v, int h, void* stream) {
    const char* name = "gv_rank_scores_mc_constrained";
    McSamples mc;
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(mc_samples_args(name, q, ld_q, q_stride, e, ld_e, e_stride, n_samples, m, v, h, &mc));
    GV_CHECK(query_cand_shape(name, n_sets, ld_cand, v));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    GV_CHECK(query_cand_given(name, cand, cand_set));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && target && tgt && count_raw && count_raw_c));
    GV_CHECK(query_filter_needs(name, filt_lo, count_filt && count_filt_c, "both filtered counts"));
    return rank_launch(name, mc, q, ld_q, e, ld_e, target, bias, filt_lo, filt_hi, filt_ent, n_filt_ent,
                       TopkCand{cand, cand_set, ld_cand, n_sets}, tgt, count_raw, count_filt, count_raw_c, count_filt_c, m, v, h, stream);
}

extern "C" int64_t gv_topk_scores_workspace_bytes(int m, int v, int k) {
    if (m <= 0 || v <= 0 || k < 1 || k > TOPK_MAX) return 0;
    int span_tiles = 0, n_spans = 0;
    topk_spans(m, v, &span_tiles, &n_spans);
    return (int64_t)m * n_spans * k * (int64_t)sizeof(unsigned long long);
}

// the launches of gv_topk_scores and its forms: CAND with cs.cand, MC with mc.n_samples > 0 (the running lists: <= 64 KiB of LDS
// beside 27 KiB static, so only k > 64 needs the limit raised)
template <bool CAND, bool MC>
static int topk_launch(const char* name, const McSamples& mc, const float* q, int ld_q, const float* e, int ld_e, const float* bias,
                       const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent, const TopkCand& cs, int k,
                       int* out_ids, float* out_values, void* workspace, int m, int v, int h, void* stream) {
    TopkParams tp{};
    tp.mc = mc;
    tp.g = mc_gemm_params(q, ld_q, e, ld_e, mc, m, v, h);
    tp.bias = bias;
    tp.filt_lo = filt_lo; tp.filt_hi = filt_hi; tp.filt_ent = filt_ent; tp.n_ent = n_filt_ent;
    tp.topk = k;
    topk_spans(m, v, &tp.span_tiles, &tp.n_spans);
    tp.part = (unsigned long long*)workspace;
    tp.cs = cs;
    return topk_span_merge<k_topk_span<1, CAND, MC>, k_topk_span<2, CAND, MC>, false, 64>(
        name, dim3((m + 63) / 64, tp.n_spans), tp, tp.part, m, tp.n_spans, k, TopkOut<int, topk_key_logit>{out_ids, out_values}, (hipStream_t)stream);
}

extern "C" int gv_topk_scores(const float* q, int ld_q, const float* e, int ld_e, const float* bias, const int* filt_lo,
                              const int* filt_hi, const int* filt_ent, int n_filt_ent, int k, int* out_ids, float* out_logits,
                              void* workspace, int m, int v, int h, void* stream) {
    const char* name = "gv_topk_scores";
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(query_k(name, k));
    GV_CHECK(query_leading(name, ld_q, ld_e, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && out_ids && out_logits && workspace));
    return topk_launch<false, false>(name, McSamples{}, q, ld_q, e, ld_e, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, TopkCand{}, k,
                                     out_ids, out_logits, workspace, m, v, h, stream);
}

extern "C" int gv_topk_scores_constrained(const float* q, int ld_q, const float* e, int ld_e, const float* bias, const int* filt_lo,
                                          const int* filt_hi, const int* filt_ent, int n_filt_ent, const uint32_t* cand, int ld_cand,
                                          int n_sets, const int32_t* cand_set, int k, int* out_ids, float* out_logits,
                                          void* workspace, int m, int v, int h, void* stream) {
    const char* name = "gv_topk_scores_constrained";
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(query_k(name, k));
    GV_CHECK(query_cand_shape(name, n_sets, ld_cand, v));
    GV_CHECK(query_leading(name, ld_q, ld_e, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    GV_CHECK(query_cand_given(name, cand, cand_set));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && out_ids && out_logits && workspace));
    return topk_launch<true, false>(name, McSamples{}, q, ld_q, e, ld_e, bias, filt_lo, filt_hi, filt_ent, n_filt_ent,
                                    TopkCand{cand, cand_set, ld_cand, n_sets}, k, out_ids, out_logits, workspace, m, v, h, stream);
}

extern "C" int gv_topk_scores_mc(const float* q, int ld_q, int64_t q_stride, const float* e, int ld_e, int64_t e_stride, int n_samples,
                                 const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent, int k,
                                 int* out_ids, float* out_prob, void* workspace, int m, int v, int h, void* stream) {
    const char* name = "gv_topk_scores_mc";
    McSamples mc;
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(query_k(name, k));
    GV_CHECK(mc_samples_args(name, q, ld_q, q_stride, e, ld_e, e_stride, n_samples, m, v, h, &mc));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && out_ids && out_prob && workspace));
    return topk_launch<false, true>(name, mc, q, ld_q, e, ld_e, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, TopkCand{}, k, out_ids,
                                    out_prob, workspace, m, v, h, stream);
}

extern "C" int gv_topk_scores_mc_constrained(const float* q, int ld_q, int64_t q_stride, const float* e, int ld_e, int64_t e_stride,
                                             int n_samples, const float* bias, const int* filt_lo, const int* filt_hi,
                                             const int* filt_ent, int n_filt_ent, const uint32_t* cand, int ld_cand, int n_sets,
                                             const int32_t* cand_set, int k, int* out_ids, float* out_prob, void* workspace, int m,
                                             int v, int h, void* stream) {
    const char* name = "gv_topk_scores_mc_constrained";
    McSamples mc;
    GV_CHECK(query_sizes(name, m, v, h, n_filt_ent));
    GV_CHECK(query_k(name, k));
    GV_CHECK(mc_samples_args(name, q, ld_q, q_stride, e, ld_e, e_stride, n_samples, m, v, h, &mc));
    GV_CHECK(query_cand_shape(name, n_sets, ld_cand, v));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    GV_CHECK(query_cand_given(name, cand, cand_set));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && out_ids && out_prob && workspace));
    return topk_launch<true, true>(name, mc, q, ld_q, e, ld_e, bias, filt_lo, filt_hi, filt_ent, n_filt_ent,
                                   TopkCand{cand, cand_set, ld_cand, n_sets}, k, out_ids, out_prob, workspace, m, v, h, stream);
}

extern "C" int gv_pair_prob_std_mc(const float* q, int ld_q, int64_t q_stride, const float* e, int ld_e, int64_t e_stride, int n_samples,
                                   const float* bias, const int* ids, int k, float* out_std, int m, int v, int h, void* stream) {
    const char* name = "gv_pair_prob_std_mc";
    GV_REQUIRE(m >= 0 && v > 0 && h > 0 && k >= 1, GV_ERR_SHAPE, "gv_pair_prob_std_mc: m=%d v=%d h=%d k=%d", m, v, h, k);
    McSamples mc;
    GV_CHECK(mc_samples_args(name, q, ld_q, q_stride, e, ld_e, e_stride, n_samples, m, v, h, &mc));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, q && e && ids && out_std));
    const long long pairs = (long long)m * k;
    hipLaunchKernelGGL(k_pair_prob_std_mc, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, ld_q, e, ld_e,
                       mc, bias, ids, out_std, pairs, k, v, h);
    return launch_status(name);
}

// ---- per-entity completion (gv_entity_topk_scores{,_mc}): the spans and their checks are entity_query_* of k_query_args.h -------
extern "C" int64_t gv_entity_topk_scores_workspace_bytes(int m, int n, int num_rels, int k) {
    return entity_query_workspace_bytes(m, n, num_rels, k, 0);      // (the library's rule: a caller's span_tiles sizes its own)
}

// the sample geometry of the two Monte-Carlo per-entity entries, reported where the parents report their leading dimensions:
// n_samples >= 1, and with more than one sample the stride spans the table (mc_samples_args without a query stack)
static int entity_mc_samples_args(const char* name, int ld_e, int ld_w, int64_t e_stride, int n_samples, int n, int h, McSamples* mc) {
    GV_REQUIRE(n_samples >= 1, GV_ERR_SHAPE, "%s: n_samples=%d", name, n_samples);
    GV_CHECK(query_leading(name, ld_e, ld_w, h));
    GV_REQUIRE(n_samples == 1 || e_stride >= (int64_t)(n - 1) * ld_e + h, GV_ERR_SHAPE,
               "%s: sample stride shorter than the table it spans (e_stride=%lld)", name, (long long)e_stride);
    mc->q_stride = 0;
    mc->e_stride = n_samples > 1 ? e_stride : 0;
    mc->n_samples = n_samples;
    mc->inv_s = 1.0f / (float)n_samples;
    return GV_OK;
}

// the parent's parameters inside an entry's own (the MC forms carry the samples beside them)
static EntityTopkParams& entity_topk_host_params(EntityTopkParams& pp, const McSamples&) { return pp; }
static EntityTopkParams& entity_topk_host_params(EntityTopkMcParams& pp, const McSamples& mc) { pp.mc = mc; return pp.e; }
static EntityTopkTypedParams& entity_topk_host_params(EntityTopkTypedParams& pp, const McSamples&) { return pp; }
static EntityTopkTypedParams& entity_topk_host_params(EntityTopkTypedMcParams& pp, const McSamples& mc) { pp.mc = mc; return pp.t; }

// what the four per-entity entries put into EntityTopkParams alike (mc.n_samples == 0: not Monte-Carlo); the spans follow
static void entity_topk_fill(EntityTopkParams& ep, const McSamples& mc, const int32_t* ents, int m, const float* e, int ld_e,
                             const float* w, int ld_w, const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_ent,
                             int n_filt_ent, int exclude_self, int k, int n, int num_rels, int h) {
    ep.g = mc_gemm_params(nullptr, ld_e, e, ld_e, mc, m, n, h);     // (the 16-byte loads need every sample's table aligned)
    ep.ents = ents; ep.w = w; ep.ld_w = ld_w;
    ep.vec_a = ep.g.vec_b && aligned16(w) && (ld_w % 4 == 0);
    ep.num_rels = num_rels; ep.exclude_self = exclude_self != 0;
    ep.bias = bias;
    ep.filt_lo = filt_lo; ep.filt_hi = filt_hi; ep.filt_ent = filt_ent; ep.n_ent = n_filt_ent;
    ep.topk = k;
}

template <bool MC>
static int entity_topk_entry(const char* name, const int32_t* ents, int m, const float* e, int ld_e, int64_t e_stride, int n_samples,
                             const float* w, int ld_w, const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_ent,
                             int n_filt_ent, int exclude_self, int k, int span_tiles, int32_t* out_rel, int32_t* out_ent,
                             float* out_values, void* workspace, int64_t workspace_bytes, int n, int num_rels, int h, void* stream) {
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && h > 0 && n_filt_ent >= 0, GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d h=%d n_filt_ent=%d", name,
               m, n, num_rels, h, n_filt_ent);
    GV_CHECK(entity_query_shape(name, n, num_rels, k, span_tiles));
    McSamples mc{};
    if constexpr (MC) GV_CHECK(entity_mc_samples_args(name, ld_e, ld_w, e_stride, n_samples, n, h, &mc));
    else GV_CHECK(query_leading(name, ld_e, ld_w, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, ents && e && w && out_rel && out_ent && out_values && workspace));
    std::conditional_t<MC, EntityTopkMcParams, EntityTopkParams> pp;
    EntityTopkParams& ep = entity_topk_host_params(pp, mc);
    entity_topk_fill(ep, mc, ents, m, e, ld_e, w, ld_w, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, k, n, num_rels, h);
    entity_query_spans(m, n, num_rels, span_tiles, &ep.span_tiles, &ep.n_spans);
    GV_CHECK(entity_query_workspace(name, m, k, span_tiles, ep.n_spans, workspace_bytes));
    ep.part = (unsigned long long*)workspace;
    return topk_span_merge<k_entity_topk_span<1, MC>, k_entity_topk_span<2, MC>, false, 64>(      // (<= 64 KiB of lists + 28 KiB static)
        name, dim3((m + 63) / 64, ep.n_spans), pp, ep.part, m, ep.n_spans, k, TopkPairOut<int, topk_key_logit>{out_rel, out_ent, out_values, n},
        (hipStream_t)stream);
}

extern "C" int gv_entity_topk_scores(const int32_t* ents, int m, const float* e, int ld_e, const float* w, int ld_w, const float* bias,
                                     const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent, int exclude_self,
                                     int k, int span_tiles, int32_t* out_rel, int32_t* out_ent, float* out_logits, void* workspace,
                                     int64_t workspace_bytes, int n, int num_rels, int h, void* stream) {
    return entity_topk_entry<false>("gv_entity_topk_scores", ents, m, e, ld_e, 0, 0, w, ld_w, bias, filt_lo, filt_hi, filt_ent, n_filt_ent,
                                    exclude_self, k, span_tiles, out_rel, out_ent, out_logits, workspace, workspace_bytes, n, num_rels, h,
                                    stream);
}

extern "C" int gv_entity_topk_scores_mc(const int32_t* ents, int m, const float* e, int ld_e, int64_t e_stride, int n_samples, const float* w,
                                        int ld_w, const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_ent,
                                        int n_filt_ent, int exclude_self, int k, int span_tiles, int32_t* out_rel, int32_t* out_ent,
                                        float* out_prob, void* workspace, int64_t workspace_bytes, int n, int num_rels, int h,
                                        void* stream) {
    return entity_topk_entry<true>("gv_entity_topk_scores_mc", ents, m, e, ld_e, e_stride, n_samples, w, ld_w, bias, filt_lo, filt_hi,
                                   filt_ent, n_filt_ent, exclude_self, k, span_tiles, out_rel, out_ent, out_prob, workspace,
                                   workspace_bytes, n, num_rels, h, stream);
}

// ---- per-entity completion among type-correct facts (gv_entity_topk_scores_typed{,_mc}): spans of the member lists' tiles --------
extern "C" int64_t gv_entity_topk_scores_typed_workspace_bytes(int m, int n_tiles, int k, int span_tiles) {
    return entity_typed_workspace_bytes(m, n_tiles, k, span_tiles);
}

template <bool MC>
static int entity_topk_typed_entry(const char* name, const int32_t* ents, int m, const float* e, int ld_e, int64_t e_stride, int n_samples,
                                   const float* w, int ld_w, const float* bias, const int* filt_lo, const int* filt_hi,
                                   const int* filt_ent, int n_filt_ent, const int64_t* set_ptr, const int32_t* set_ids,
                                   const int32_t* tile_ptr, int n_tiles, int cand_base, int exclude_self, int k, int span_tiles,
                                   int32_t* out_rel, int32_t* out_ent, float* out_values, void* workspace, int64_t workspace_bytes, int n,
                                   int num_rels, int h, void* stream) {
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && h > 0 && n_filt_ent >= 0, GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d h=%d n_filt_ent=%d", name,
               m, n, num_rels, h, n_filt_ent);
    GV_CHECK(entity_query_shape(name, n, num_rels, k, span_tiles));
    GV_CHECK(entity_typed_shape(name, num_rels, n_tiles, cand_base));
    McSamples mc{};
    if constexpr (MC) GV_CHECK(entity_mc_samples_args(name, ld_e, ld_w, e_stride, n_samples, n, h, &mc));
    else GV_CHECK(query_leading(name, ld_e, ld_w, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_ent));
    if (m == 0) return GV_OK;
    GV_CHECK(query_pointers(name, ents && e && w && out_rel && out_ent && out_values && workspace));
    GV_CHECK(entity_typed_given(name, set_ptr, set_ids, tile_ptr, n_tiles));
    std::conditional_t<MC, EntityTopkTypedMcParams, EntityTopkTypedParams> pp;
    EntityTopkTypedParams& tp = entity_topk_host_params(pp, mc);
    EntityTopkParams& ep = tp.e;
    entity_topk_fill(ep, mc, ents, m, e, ld_e, w, ld_w, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, k, n, num_rels, h);
    entity_typed_spans(m, n_tiles, span_tiles, &ep.span_tiles, &ep.n_spans);
    GV_CHECK(entity_query_workspace(name, m, k, span_tiles, ep.n_spans, workspace_bytes));
    ep.part = (unsigned long long*)workspace;
    tp.ty = TopkTyped{(const long long*)set_ptr, set_ids, tile_ptr, cand_base, n_tiles};
    const TopkPairOut<int, topk_key_logit> out{out_rel, out_ent, out_values, n};
    if (n_tiles == 0) return topk_all_padding(name, ep.part, m, k, out, (hipStream_t)stream);
    return topk_span_merge<k_entity_topk_typed_span<1, MC>, k_entity_topk_typed_span<2, MC>, false, 64>(      // (<= 64 KiB of lists + 28 KiB static)
        name, dim3((m + 63) / 64, ep.n_spans), pp, ep.part, m, ep.n_spans, k, out, (hipStream_t)stream);
}

extern "C" int gv_entity_topk_scores_typed(const int32_t* ents, int m, const float* e, int ld_e, const float* w, int ld_w, const float* bias,
                                           const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_filt_ent,
                                           const int64_t* set_ptr, const int32_t* set_ids, const int32_t* tile_ptr, int n_tiles,
                                           int cand_base, int exclude_self, int k, int span_tiles, int32_t* out_rel, int32_t* out_ent,
                                           float* out_logits, void* workspace, int64_t workspace_bytes, int n, int num_rels, int h,
                                           void* stream) {
    return entity_topk_typed_entry<false>("gv_entity_topk_scores_typed", ents, m, e, ld_e, 0, 0, w, ld_w, bias, filt_lo, filt_hi, filt_ent,
                                          n_filt_ent, set_ptr, set_ids, tile_ptr, n_tiles, cand_base, exclude_self, k, span_tiles, out_rel,
                                          out_ent, out_logits, workspace, workspace_bytes, n, num_rels, h, stream);
}

extern "C" int gv_entity_topk_scores_typed_mc(const int32_t* ents, int m, const float* e, int ld_e, int64_t e_stride, int n_samples,
                                              const float* w, int ld_w, const float* bias, const int* filt_lo, const int* filt_hi,
                                              const int* filt_ent, int n_filt_ent, const int64_t* set_ptr, const int32_t* set_ids,
                                              const int32_t* tile_ptr, int n_tiles, int cand_base, int exclude_self, int k,
                                              int span_tiles, int32_t* out_rel, int32_t* out_ent, float* out_prob, void* workspace,
                                              int64_t workspace_bytes, int n, int num_rels, int h, void* stream) {
    return entity_topk_typed_entry<true>("gv_entity_topk_scores_typed_mc", ents, m, e, ld_e, e_stride, n_samples, w, ld_w, bias, filt_lo,
                                         filt_hi, filt_ent, n_filt_ent, set_ptr, set_ids, tile_ptr, n_tiles, cand_base, exclude_self, k,
                                         span_tiles, out_rel, out_ent, out_prob, workspace, workspace_bytes, n, num_rels, h, stream);
}

namespace gv {

// ---- relation prediction (gv_pair_rel_scores): the query is an entity pair, the candidates are the relations ---------------------
// logit[i, r] = (e[s_i] * e[o_i]) . w[r] + bias.  The product row is made while it is staged, as k_entity_topk_span makes
// e[a] * w[r] -- a thread's four floats of e[s] times the same four of e[o], one f32 multiply each, the value gv_mul stores -- and
// the relation rows go through load_b, so the tile is score_tile_with's and a logit is gv_gemm_f32(gv_mul(e[s], e[o]), w^T) + bias
// bit for bit.  There are 11 .. 1 345 candidates, one to 22 column tiles: a workgroup owns a 64-pair row tile and walks ALL of them
// itself, in ascending order -- no spans, no workspace, no merge, one launch for ranks and list together.  Per tile the logits go
// through Ls; wave w then takes rows 16 w .. 16 w + 15, one lane per column (topk_pair_rel_tile of k_topk.h, shared with
// k_transe_pair_rel): the row's filter window (the cursor is shared by the count and the list), two ballots against the target's
// logit for the counts, and the key into the row's sorted list.  A row's counts and list sit in LDS for the whole walk and belong to one wave, so nothing is atomic and the
// epilogue is that wave's plain stores.
// The target's logit is a tile's own element.  With one column tile it is read back from Ls; with more, one extra tile is made
// ahead of the walk with the relation rows GATHERED through the rows' targets (score_tile_gather: the same staging, the same chain,
// so a gathered row's logits are the bits score_tile gives that row) and its element (j, j) is row j's -- the walk proper
// recomputes it bit for bit, as k_rank_scores<1> recomputes what k_rank_scores<0> wrote.
// CAND (gv_pair_rel_scores_constrained): the pair's type-correct relations -- the AND of two rows of the relation bitmask
// (TopkPairCand, k_topk.h) -- add two counts per row and narrow the list; the raw and filtered counts, the target's value and
// every logit are the unconstrained kernel's.  Thread rl < 64 fetches the row's two words per tile once the tile's MFMAs are
// done (every wave is then past the previous tile's selection), the tile's barrier publishes them.
// MC (gv_pair_rel_scores_mc): the value is pbar = (sum over s ascending of mc_sig(logit_s + bias[s])) * inv_s -- the sample loop of
// k_entity_topk_span<.., MC> around score_tile_with, sample s reading the pair's rows at e + s * e_stride against the one w, pbar
// in the 16 accumulator registers, written to Ls and selected ONCE per tile.  Under each sample's sigmoids the next sample's first
// k-chunk is in flight, under the last one's the next tile's of sample 0.  The gathered tile of the targets runs the same loop
// around score_tile_gather, so a target's pbar is the walk's own element bit for bit.
// The default corner keeps the statements it had (the new corners' parameters come in a wrapper struct, their code under
// if constexpr): its results and its code are the parent's.
struct PairRelParams {
    GemmParams g;                 // b = w (stored [R, h]), m, n = R, k = h; a is not read
    const float* e;               // [n_entities, ld_e]
    int ld_e, vec_a;              // vec_a: four floats of a row of e may be read as one
    const int* s;                 // [m] the pairs' entities, trusted to lie in [0, n_entities)
    const int* o;
    const int* target;            // NULL: no ranks
    const float* bias;
    const int* filt_lo;           // NULL: no filter
    const int* filt_hi;
    const int* filt_rel;
    int n_filt;                   // length of filt_rel: every range is clamped into it
    int topk;                     // 0: no list
    float* tgt;
    int* count_raw;               // may be NULL
    int* count_filt;              // NULL without a filter
    int* out_ids;
    float* out_logits;
};

// what the CAND / MC corners carry beside the parent's parameters (mc.n_samples == 0: not Monte-Carlo; cs.cand NULL: no sets)
struct PairRelXParams {
    PairRelParams p;              // p.bias: one value per sample with MC
    McSamples mc;                 // e_stride: elements between consecutive samples' tables
    TopkPairCand cs;
    int* count_raw_c;             // may be NULL
    int* count_filt_c;            // NULL without a filter
};

__device__ __forceinline__ const PairRelParams& pair_rel_params(const PairRelParams& pp) { return pp; }
__device__ __forceinline__ const PairRelParams& pair_rel_params(const PairRelXParams& px) { return px.p; }

// rank_votes' predicates: greater, or either side NaN; the key of gv_topk_scores
struct PairRelRule {
    static __device__ __forceinline__ bool above(float v, float t) { return !(v <= t); }
    static __device__ __forceinline__ unsigned long long key(float v, int col) { return topk_key(v, col); }
};

template <int NK, bool CAND = false, bool MC = false>      // NK: keys per lane of a row's list: 0 (ranks only), 1 (k <= 64), 2
__global__ __launch_bounds__(256) void k_pair_rel(const std::conditional_t<CAND || MC, PairRelXParams, PairRelParams> px) {
    constexpr int BM = SC_BM, BN = SC_BN, BK = SC_BK, LDL = BN + 1, APT = BM * BK / 256;
    const PairRelParams& pp = pair_rel_params(px);
    __shared__ float As[BK * SC_LDA];
    __shared__ float Bs[BK * SC_LDB];
    __shared__ float Ls[BM * LDL];                 // the tile's logits, row-major
    __shared__ unsigned long long thr[BM];         // each row's k-th key
    __shared__ int cur[BM], fhi[BM], nxt[BM];      // filter cursor (k_topk.h)
    __shared__ int fl[4][64];
    __shared__ int tcol_s[BM];                     // the rows' targets (-1: none)
    __shared__ float tgt_s[BM];                    // ... and their logits
    __shared__ int cnt_s[CAND ? 4 : 2][BM];        // 2 #better + #equal: raw, filtered (CAND: and the two among the allowed)
    __shared__ int so_s[CAND ? 2 : 1][CAND ? BM : 1];              // CAND: the rows' pairs (-1: no such row)
    __shared__ unsigned long long allow_s[CAND ? BM : 1];          // ... and their allowed relations of the tile at hand
    extern __shared__ unsigned long long lists[];  // [BM][topk]
    const GemmParams& p = pp.g;
    const int k = pp.topk;
    const int m0 = blockIdx.x * BM;
    const int col_tiles = (p.n + BN - 1) / BN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const bool filtered = pp.filt_lo != nullptr, ranked = pp.target != nullptr;
    const TopkPairRel st{lists, thr, cur, fhi, nxt, fl, tcol_s, tgt_s, cnt_s, allow_s};

    // this thread's share of the query operand: row threadIdx.x / 4 of the tile, APT floats from column (threadIdx.x % 4) * APT on
    const int a_row = m0 + threadIdx.x / (BK / APT), a_col = (threadIdx.x % (BK / APT)) * APT;
    const bool a_ok = a_row < p.m;
    const float* s_src = pp.e + (a_ok ? (size_t)pp.s[a_row] * pp.ld_e : 0) + a_col;     // (MC: of the sample at hand)
    const float* o_src = pp.e + (a_ok ? (size_t)pp.o[a_row] * pp.ld_e : 0) + a_col;
    auto load_q = [&](int k0, float (&r)[APT]) {
        float ov[APT];
        load_run<APT>(s_src + k0, a_col + k0, p.k, a_ok, pp.vec_a, r, 0);
        load_run<APT>(o_src + k0, a_col + k0, p.k, a_ok, pp.vec_a, ov, 0);
#pragma unroll
        for (int i = 0; i < APT; ++i) r[i] *= ov[i];
    };

    if constexpr (NK > 0)
        for (int i = threadIdx.x; i < BM * k; i += 256) lists[i] = 0ull;
    fl[wid][lane] = 0;
    if (threadIdx.x < BM) {
        const int rl = threadIdx.x, row = m0 + rl;
        thr[rl] = 0ull;
        cnt_s[0][rl] = 0; cnt_s[1][rl] = 0;
        if constexpr (CAND) {
            cnt_s[2][rl] = 0; cnt_s[3][rl] = 0;
            so_s[0][rl] = row < p.m ? pp.s[row] : -1;
            so_s[1][rl] = row < p.m ? pp.o[row] : -1;
        }
        tcol_s[rl] = (ranked && row < p.m) ? pp.target[row] : -1;
        tgt_s[rl] = __uint_as_float(0x7fc00000u);  // a target outside [0, R) ranks last
        topk_filter_begin(pp.filt_lo, pp.filt_hi, pp.filt_rel, pp.n_filt, filtered && row < p.m, row, 0, &cur[rl], &fhi[rl], &nxt[rl]);
    }
    const float bv = (!MC && pp.bias) ? *pp.bias : 0.f;
    float ra[APT], rb[BN * BK / 256];
    // MC: pbar of one tile.  one_sample() is the tile's MFMA chain on the operands in ra / rb; load_sample() requests the first
    // k-chunk of the sample s_src / o_src point at, load_next() what follows the tile (s_src / o_src are back at sample 0 then).
    auto pbar_tile = [&](auto&& one_sample, auto&& load_sample, auto&& load_next) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        if constexpr (MC) {
            const McSamples& mc = px.mc;
            for (int s = 0; s < mc.n_samples; ++s) {
                const f32x16 lg = one_sample();
                const float bs = pp.bias ? pp.bias[s] : 0.f;
                if (s + 1 < mc.n_samples) {                            // the next sample's first operands fly under the sigmoids
                    s_src += mc.e_stride;
                    o_src += mc.e_stride;
                    load_sample();
                } else {                                               // ... under the last one's, what follows the tile
                    s_src -= (long long)s * mc.e_stride;
                    o_src -= (long long)s * mc.e_stride;
                    load_next();
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += mc_sig(lg[i] + bs);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] *= mc.inv_s;
        }
        return acc;
    };

    if (ranked && col_tiles > 1) {                 // the targets' logits: ONE gathered tile whose column j is w[target of row j]
        const int tc = a_ok ? pp.target[a_row] : -1;                      // (this thread's B slot is its A row: threadIdx.x / 4)
        const bool t_ok = (unsigned)tc < (unsigned)p.n;
        const float* t_src = p.b + (t_ok ? (size_t)tc * p.ldb : 0) + a_col;
        auto load_t = [&](int k0, float (&r)[BN * BK / 256]) { load_run<BN * BK / 256>(t_src + k0, a_col + k0, p.k, t_ok, p.vec_b, r, 0); };
        load_q(0, ra);
        load_t(0, rb);
        f32x16 acc;
        if constexpr (MC)
            acc = pbar_tile([&] { return score_tile_gather(p, load_q, load_t, ra, rb, As, Bs); },
                            [&] { load_q(0, ra); load_t(0, rb); }, [] {});
        else
            acc = score_tile_gather(p, load_q, load_t, ra, rb, As, Bs);              // (its barriers publish the set-up)
        const int cl = wn + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {                                    // element (j, j) is row j's own
            const int rl = wm + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (rl == cl && (unsigned)tcol_s[rl] < (unsigned)p.n) tgt_s[rl] = acc[r] + bv;
        }
    }

    load_q(0, ra);
    load_b<true, BN, BK>(p, 0, 0, p.k, rb);
    for (int t = 0; t < col_tiles; ++t) {
        const int n0 = t * BN;
        // score_tile_with's first barrier publishes the set-up (and the gathered tile's tgt_s) and ends the last tile's reads of Ls
        f32x16 acc;
        if constexpr (MC) {
            acc = pbar_tile([&] { return score_tile_with(p, load_q, n0, ra, rb, As, Bs); },
                            [&] { load_q(0, ra); load_b<true, BN, BK>(p, n0, 0, p.k, rb); },
                            [&] {
                                if (t + 1 < col_tiles) {
                                    load_q(0, ra);
                                    load_b<true, BN, BK>(p, n0 + BN, 0, p.k, rb);
                                }
                            });
        } else {
            acc = score_tile_with(p, load_q, n0, ra, rb, As, Bs);
            if (t + 1 < col_tiles) {               // the next tile's first operands fly under the selection
                load_q(0, ra);
                load_b<true, BN, BK>(p, n0 + BN, 0, p.k, rb);
            }
        }
        if constexpr (CAND)                        // (every wave is past the tile's first barrier: nobody still reads the last tile's)
            if (threadIdx.x < BM) allow_s[threadIdx.x] = topk_pair_rel_allow(px.cs, so_s[0][threadIdx.x], so_s[1][threadIdx.x], n0, p.n);
#pragma unroll
        for (int r = 0; r < 16; ++r) Ls[(wm + (r & 3) + 8 * (r >> 2) + 4 * lhi) * LDL + wn + l31] = acc[r] + bv;
        __syncthreads();
        if (ranked && col_tiles == 1) {            // the one tile holds every target
            if (threadIdx.x < BM && (unsigned)tcol_s[threadIdx.x] < (unsigned)p.n)
                tgt_s[threadIdx.x] = Ls[threadIdx.x * LDL + tcol_s[threadIdx.x]];
            __syncthreads();
        }
        topk_pair_rel_tile<NK, PairRelRule, CAND>(st, m0, p.m, n0, p.n, t, k, ranked, pp.filt_rel, lane, wid,
                                                  [&](int rl) { return Ls[rl * LDL + lane]; });
    }
    if constexpr (CAND)
        topk_pair_rel_store<NK, int, topk_key_logit, true>(st, m0, p.m, k, ranked, pp.tgt, pp.count_raw, pp.count_filt, pp.out_ids,
                                                           pp.out_logits, lane, wid, px.count_raw_c, px.count_filt_c);
    else
        topk_pair_rel_store<NK, int, topk_key_logit>(st, m0, p.m, k, ranked, pp.tgt, pp.count_raw, pp.count_filt, pp.out_ids,
                                                     pp.out_logits, lane, wid);
}

}  // namespace gv

// what every pair entry puts into PairRelParams (e_stride: of the MC forms, 0 otherwise: the 16-byte loads need every sample's
// table aligned)
static void pair_rel_fill(PairRelParams& pp, const float* e, int ld_e, long long e_stride, const float* w, int ld_w, int num_rels,
                          const int32_t* s, const int32_t* o, const int32_t* target, const float* bias, const int* filt_lo,
                          const int* filt_hi, const int* filt_rel, int n_filt_rel, int k, float* tgt, int* count_raw, int* count_filt,
                          int* out_ids, float* out_values, int m, int h) {
    pp.g = score_gemm_params(nullptr, ld_e, w, ld_w, m, num_rels, h);
    pp.e = e; pp.ld_e = ld_e;
    pp.vec_a = aligned16(e) && (ld_e % 4 == 0) && (e_stride % 4 == 0);
    pp.s = s; pp.o = o; pp.target = target; pp.bias = bias;
    pp.filt_lo = filt_lo; pp.filt_hi = filt_hi; pp.filt_rel = filt_rel; pp.n_filt = n_filt_rel;
    pp.topk = k;
    pp.tgt = tgt; pp.count_raw = count_raw; pp.count_filt = filt_lo ? count_filt : nullptr;
    pp.out_ids = out_ids; pp.out_logits = out_values;
}

extern "C" int gv_pair_rel_scores(const float* e, int ld_e, int n, const float* w, int ld_w, int num_rels, const int32_t* s,
                                  const int32_t* o, const int32_t* target, const float* bias, const int* filt_lo, const int* filt_hi,
                                  const int* filt_rel, int n_filt_rel, int k, float* tgt, int* count_raw, int* count_filt, int* out_ids,
                                  float* out_logits, int m, int h, void* stream) {
    const char* name = "gv_pair_rel_scores";
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && h > 0 && n_filt_rel >= 0, GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d h=%d n_filt_rel=%d", name,
               m, n, num_rels, h, n_filt_rel);
    GV_CHECK(pair_query_asks(name, k, target));
    GV_CHECK(query_leading(name, ld_e, ld_w, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_rel, "filt_lo / filt_hi / filt_rel"));
    if (m == 0) return GV_OK;
    GV_CHECK(pair_query_given(name, e && w && s && o, target, tgt, k, out_ids, out_logits, filt_lo, count_filt));
    PairRelParams pp{};
    pair_rel_fill(pp, e, ld_e, 0, w, ld_w, num_rels, s, o, target, bias, filt_lo, filt_hi, filt_rel, n_filt_rel, k, tgt, count_raw,
                  count_filt, out_ids, out_logits, m, h);
    constexpr int KEY = (int)sizeof(unsigned long long);
    const dim3 grid((unsigned)((m + 63) / 64)), block(256);
    hipStream_t st = (hipStream_t)stream;
    static unsigned long long raised = 0;          // (<= 64 KiB of lists beside 28 KiB static: only k > 64 needs the limit raised)
    if (k == 0) hipLaunchKernelGGL(k_pair_rel<0>, grid, block, 0, st, pp);
    else if (k <= 64) hipLaunchKernelGGL(k_pair_rel<1>, grid, block, 64 * k * KEY, st, pp);
    else {
        if (!raise_dynamic_lds((const void*)k_pair_rel<2>, 64 * TOPK_MAX * KEY, raised, name)) return GV_ERR_SHAPE;
        hipLaunchKernelGGL(k_pair_rel<2>, grid, block, 64 * k * KEY, st, pp);
    }
    return launch_status(name);
}

// ---- the type-constrained and the posterior-predictive forms (gv_pair_rel_scores_constrained / _mc / _mc_constrained) -----------
// gv_pair_rel_scores' checks in its order; the sample geometry stands where it reports its leading dimensions
// (entity_mc_samples_args), the candidate group follows the filter group.  One launch, no workspace.
template <bool CAND, bool MC>
static int pair_rel_entry(const char* name, const float* e, int ld_e, int64_t e_stride, int n_samples, int n, const float* w, int ld_w,
                          int num_rels, const int32_t* s, const int32_t* o, const int32_t* target, const float* bias,
                          const int* filt_lo, const int* filt_hi, const int* filt_rel, int n_filt_rel, const uint32_t* cand,
                          int ld_cand, int n_sets, int k, float* tgt, int* count_raw, int* count_filt, int* count_raw_c,
                          int* count_filt_c, int* out_ids, float* out_values, int m, int h, void* stream) {
    GV_REQUIRE(m >= 0 && n > 0 && num_rels > 0 && h > 0 && n_filt_rel >= 0, GV_ERR_SHAPE, "%s: m=%d n=%d num_rels=%d h=%d n_filt_rel=%d", name,
               m, n, num_rels, h, n_filt_rel);
    GV_CHECK(pair_query_asks(name, k, target));
    PairRelXParams px{};
    if constexpr (MC) GV_CHECK(entity_mc_samples_args(name, ld_e, ld_w, e_stride, n_samples, n, h, &px.mc));
    else GV_CHECK(query_leading(name, ld_e, ld_w, h));
    GV_CHECK(query_filter(name, filt_lo, filt_hi, filt_rel, "filt_lo / filt_hi / filt_rel"));
    if constexpr (CAND) GV_CHECK(pair_query_cand(name, cand, ld_cand, n_sets, n, num_rels));
    if (m == 0) return GV_OK;
    GV_CHECK(pair_query_given(name, e && w && s && o, target, tgt, k, out_ids, out_values, filt_lo, count_filt));
    if constexpr (CAND) GV_CHECK(pair_query_given_cand(name, target, filt_lo, count_filt_c));
    pair_rel_fill(px.p, e, ld_e, px.mc.e_stride, w, ld_w, num_rels, s, o, target, bias, filt_lo, filt_hi, filt_rel, n_filt_rel, k, tgt,
                  count_raw, count_filt, out_ids, out_values, m, h);
    if constexpr (CAND) {
        px.cs = TopkPairCand{cand, ld_cand, n};
        px.count_raw_c = count_raw_c; px.count_filt_c = filt_lo ? count_filt_c : nullptr;
    }
    constexpr int KEY = (int)sizeof(unsigned long long);
    const dim3 grid((unsigned)((m + 63) / 64)), block(256);
    hipStream_t st = (hipStream_t)stream;
    static unsigned long long raised = 0;          // (one per instantiation of this template, i.e. per NK = 2 kernel)
    if (k == 0) hipLaunchKernelGGL((k_pair_rel<0, CAND, MC>), grid, block, 0, st, px);
    else if (k <= 64) hipLaunchKernelGGL((k_pair_rel<1, CAND, MC>), grid, block, 64 * k * KEY, st, px);
    else {
        if (!raise_dynamic_lds((const void*)k_pair_rel<2, CAND, MC>, 64 * TOPK_MAX * KEY, raised, name)) return GV_ERR_SHAPE;
        hipLaunchKernelGGL((k_pair_rel<2, CAND, MC>), grid, block, 64 * k * KEY, st, px);
    }
    return launch_status(name);
}

extern "C" int gv_pair_rel_scores_constrained(const float* e, int ld_e, int n, const float* w, int ld_w, int num_rels, const int32_t* s,
                                              const int32_t* o, const int32_t* target, const float* bias, const int* filt_lo,
                                              const int* filt_hi, const int* filt_rel, int n_filt_rel, const uint32_t* cand, int ld_cand,
                                              int n_sets, int k, float* tgt, int* count_raw, int* count_filt, int* count_raw_c,
                                              int* count_filt_c, int* out_ids, float* out_logits, int m, int h, void* stream) {
    return pair_rel_entry<true, false>("gv_pair_rel_scores_constrained", e, ld_e, 0, 0, n, w, ld_w, num_rels, s, o, target, bias, filt_lo,
                                       filt_hi, filt_rel, n_filt_rel, cand, ld_cand, n_sets, k, tgt, count_raw, count_filt, count_raw_c,
                                       count_filt_c, out_ids, out_logits, m, h, stream);
}

extern "C" int gv_pair_rel_scores_mc(const float* e, int ld_e, int64_t e_stride, int n_samples, int n, const float* w, int ld_w,
                                     int num_rels, const int32_t* s, const int32_t* o, const int32_t* target, const float* bias,
                                     const int* filt_lo, const int* filt_hi, const int* filt_rel, int n_filt_rel, int k, float* tgt,
                                     int* count_raw, int* count_filt, int* out_ids, float* out_prob, int m, int h, void* stream) {
    return pair_rel_entry<false, true>("gv_pair_rel_scores_mc", e, ld_e, e_stride, n_samples, n, w, ld_w, num_rels, s, o, target, bias,
                                       filt_lo, filt_hi, filt_rel, n_filt_rel, nullptr, 0, 0, k, tgt, count_raw, count_filt, nullptr,
                                       nullptr, out_ids, out_prob, m, h, stream);
}

extern "C" int gv_pair_rel_scores_mc_constrained(const float* e, int ld_e, int64_t e_stride, int n_samples, int n, const float* w, int ld_w,
                                                 int num_rels, const int32_t* s, const int32_t* o, const int32_t* target,
                                                 const float* bias, const int* filt_lo, const int* filt_hi, const int* filt_rel,
                                                 int n_filt_rel, const uint32_t* cand, int ld_cand, int n_sets, int k, float* tgt,
                                                 int* count_raw, int* count_filt, int* count_raw_c, int* count_filt_c, int* out_ids,
                                                 float* out_prob, int m, int h, void* stream) {
    return pair_rel_entry<true, true>("gv_pair_rel_scores_mc_constrained", e, ld_e, e_stride, n_samples, n, w, ld_w, num_rels, s, o, target,
                                      bias, filt_lo, filt_hi, filt_rel, n_filt_rel, cand, ld_cand, n_sets, k, tgt, count_raw, count_filt,
                                      count_raw_c, count_filt_c, out_ids, out_prob, m, h, stream);
}

extern "C" int gv_rel_rows_gemm(const float* feat, int ld_feat, const int32_t* rows, const float* w, int num_rels, int in_feat,
                                int out_feat, int transpose_w, const int32_t* tiles, int n_tiles, float* msg, void* stream) {
    GV_REQUIRE(num_rels > 0 && in_feat > 0 && out_feat > 0 && n_tiles >= 0, GV_ERR_SHAPE, "gv_rel_rows_gemm: bad sizes");
    if (n_tiles == 0) return GV_OK;
    GV_REQUIRE(feat && rows && w && tiles && msg, GV_ERR_NULL, "gv_rel_rows_gemm: NULL pointer");
    const int k = transpose_w ? out_feat : in_feat, n = transpose_w ? in_feat : out_feat;
    GV_REQUIRE(ld_feat >= k, GV_ERR_SHAPE, "gv_rel_rows_gemm: ld_feat=%d < %d", ld_feat, k);
    RelGemmParams p{};
    p.a = feat; p.a_rows = rows; p.w = w; p.c = msg; p.tiles = (const int4*)tiles;
    p.lda = ld_feat; p.in_feat = in_feat; p.out_feat = out_feat; p.n = n; p.k = k;
    p.vec = aligned16(feat) && aligned16(w) && (ld_feat % 4 == 0) && (in_feat % 4 == 0) && (out_feat % 4 == 0);
    dim3 grid((n + 63) / 64, n_tiles), block(256);
    if (transpose_w) hipLaunchKernelGGL(k_rel_rows<true>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(k_rel_rows<false>, grid, block, 0, (hipStream_t)stream, p);
    return launch_status("gv_rel_rows_gemm");
}

extern "C" int gv_rel_gradw_gemm(const float* x, int ld_x, const int32_t* x_rows, const float* g, int ld_g, const int32_t* g_rows,
                                 const float* scale, const int32_t* relptr, int num_rels, int in_feat, int out_feat,
                                 float* grad_w, void* stream) {
    GV_REQUIRE(num_rels > 0 && in_feat > 0 && out_feat > 0, GV_ERR_SHAPE, "gv_rel_gradw_gemm: bad sizes");
    GV_REQUIRE(x && x_rows && g && g_rows && relptr && grad_w, GV_ERR_NULL, "gv_rel_gradw_gemm: NULL pointer");
    GV_REQUIRE(ld_x >= in_feat && ld_g >= out_feat, GV_ERR_SHAPE, "gv_rel_gradw_gemm: leading dimension too small");
    GV_REQUIRE(num_rels <= 65535, GV_ERR_SHAPE, "gv_rel_gradw_gemm: more than 65535 relation types");
    RelGemmParams p{};
    p.a = x; p.a_rows = x_rows; p.lda = ld_x; p.b_feat = g; p.b_rows = g_rows; p.ldb_feat = ld_g; p.b_scale = scale;
    p.relptr = relptr; p.c = grad_w; p.in_feat = in_feat; p.out_feat = out_feat;
    p.vec = aligned16(x) && aligned16(g) && (ld_x % 4 == 0) && (ld_g % 4 == 0);
    dim3 grid((out_feat + 63) / 64, (in_feat + 63) / 64, num_rels), block(256);
    hipLaunchKernelGGL(k_rel_gradw, grid, block, 0, (hipStream_t)stream, p);
    return launch_status("gv_rel_gradw_gemm");
}

extern "C" int gv_colsum_finish(const float* part, int n, int n_slices, float* out, int accumulate, void* stream) {
    GV_REQUIRE(part && out, GV_ERR_NULL, "gv_colsum_finish: NULL pointer");
    GV_REQUIRE(n > 0 && n_slices > 0, GV_ERR_SHAPE, "gv_colsum_finish: n=%d n_slices=%d", n, n_slices);
    hipLaunchKernelGGL(k_colsum_final_wide, dim3((n + 15) / 16), dim3(1024), 0, (hipStream_t)stream, part, n, n_slices, out,
                       accumulate);
    return launch_status("gv_colsum_finish");
}

extern "C" int gv_colsum(const float* x, const float* relu_mask, int64_t m, int n, int ld, float* out, float* workspace,
                         int accumulate, void* stream) {
    GV_REQUIRE((x || m == 0) && out && workspace, GV_ERR_NULL, "gv_colsum: NULL pointer");      // m == 0: sums of zero rows
    GV_REQUIRE(m >= 0 && n > 0 && ld >= n, GV_ERR_SHAPE, "gv_colsum: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const int nsl = COLSUM_SLICES;     // workspace is sized for 64 slices
    hipLaunchKernelGGL(k_colsum_part, dim3((n + 63) / 64, nsl), dim3(256), 0, st, x, relu_mask, m, n, ld, workspace);
    hipLaunchKernelGGL(k_colsum_final, dim3((n + 63) / 64), dim3(64), 0, st, workspace, n, nsl, out, accumulate);
    return launch_status("gv_colsum");
}
