// Whole-graph triplet mining for TransE (gv_transe_mine): every (s, r, o) of the normalised tables en (n, dim), rn (R, dim)
//
//   q[c] = en[s][c] + rn[r][c]          d[s, r, o] = ||q - en[o]||_p
//
// bit for bit gv_transe_distances on the query rows of gv_transe_queries (head = 0): one f32 add per subject element, then
// te_pair_term (k_transe.h) over the columns in order into ONE accumulator per pair, sqrtf for p = 2.  L1 has no matrix form and the
// L2 identity |q|^2 + |e|^2 - 2 q.e rounds differently, so this is vector-ALU work: 4 x 4 pairs a lane, as te_tile.
//
// Loop order: a workgroup owns one 64 x 64 (subject tile, object tile) pair and walks the RELATIONS over it.  Up to TM_KC_MAX columns
// both tiles of en sit in LDS, column-major ([k][64 + 4]: a lane's four subjects and four objects are one 16-byte read each), staged
// once; a relation then costs its dim-float row of rn, added to the subject side on the fly.  The two tiles fill most of the LDS, so
// a compute unit holds ONE workgroup: it is 1 024 threads, four groups of 256 that each take every fourth relation of the span over
// the same two tiles (four waves a SIMD: with one, every LDS read's latency showed -- 1.28 s a sweep against 0.26 s of arithmetic).
// Wider tables are staged in TM_KC_MAX-column chunks per round of four relations; the 16 accumulators live across the chunks of a
// relation, so the summation order is the same.
//
// Partial sums only grow (every term is >= 0 and f32 addition is monotone), so once every pair of a wave is past the distance the
// pass still cares about -- the emission threshold, or the upper edge of the histogram prefix -- the wave leaves the column loop
// (checked every TM_CHECK columns; NaN never compares greater, so NaN pairs run to the end and are dropped by their key).  What a
// pair's key is compared with is unchanged, so the result is too.
//
// Candidates, keys (those of -d: larger = nearer, 0 = NaN only), the filter and the EMIT / HIST epilogues: k_mine.h, which both
// miners share, as they share the host set-up before the launch (mine_prepare, k_mine.hip); a record's fourth word is the bits of d
// itself (never -0: the sums start at +0 and add |.| or squares).
#include <algorithm>

#include "common.h"
#include "k_mine.h"
#include "k_transe.h"

namespace gv {

constexpr int TM_LD = TE_TQ + 4;        // LDS row pitch of a column of 64 rows
constexpr int TM_KC_MAX = 224;          // columns per staged chunk: (2 x 68 + 4) x 224 floats = 123 KiB (+ 22 KiB static) of the 160
constexpr int TM_CHECK = 32;            // columns between two looks at the partial sums
constexpr int TM_GROUPS = 4;            // groups of 256 threads on one tile pair, each walking its own relations
constexpr int TM_THREADS = 256 * TM_GROUPS;

struct TeMineParams {
    const float* en;
    const float* rn;
    int dim;
    int kc, n_chunks;                  // chunk width and count; one chunk: the tiles stay in LDS
    MineSelect sel;
};

// columns [k0, k0 + kn) of rows row0 .. row0 + 63 of en into dst [kn][TM_LD]; zeros past the table
__device__ __forceinline__ void tm_stage(float* dst, const float* __restrict__ en, int row0, int n, int dim, int k0, int kn) {
    for (int x = threadIdx.x; x < TE_TQ * kn; x += TM_THREADS) {
        const int row = x / kn, k = x - row * kn;
        dst[k * TM_LD + row] = row0 + row < n ? en[(size_t)(row0 + row) * dim + k0 + k] : 0.f;
    }
}

// the largest accumulator value this pass looks at: keys below kmin are dropped by the epilogue whatever their value
template <int P, bool HIST>
__device__ __forceinline__ float tm_bound(const MineSelect& sel) {
    const unsigned kmin = HIST ? (sel.prefix_bits ? sel.prefix << (32 - sel.prefix_bits) : 0u) : sel.key_min;
    float bound = INFINITY;                              // in the accumulator's unit: the distance, or (p = 2) its square, rounded up
    if (kmin > 0x007fffffu) {                            // above the key of +inf
        const float dmax = -mine_key_logit(kmin);
        // p = 2: a few ulps above dmax^2, and never in the subnormals, so that acc > bound implies sqrtf(acc) > dmax
        bound = P == 1 || dmax < 0.f ? dmax : fmaxf(dmax * dmax * 1.000001f, 1e-30f);
    }
    return bound;
}

template <int P, bool HIST>
__global__ __launch_bounds__(TM_THREADS) void k_transe_mine(const TeMineParams p) {
    extern __shared__ __attribute__((aligned(16))) float tm_smem[];
    __shared__ unsigned long long fmask[TM_GROUPS][64];  // a group's relation: its listed objects per subject row
    __shared__ int fany[TM_GROUPS];
    __shared__ unsigned flist[MINE_FL_CAP];
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const int kc = p.kc;
    float* As = tm_smem;                                 // [kc][TM_LD] subjects
    float* Bs = As + kc * TM_LD;                         // [kc][TM_LD] objects
    const int t = threadIdx.x, g = t >> 8, tl = t & 255, lane = t & 63, tx = tl & 15, ty = tl >> 4;
    float* Rs = Bs + kc * TM_LD + g * kc;                // [TM_GROUPS][kc] each group's relation row
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const MineSelect& sel = p.sel;
    const int n = sel.n;
    const int r0 = blockIdx.z * sel.rel_span, r1 = min(r0 + sel.rel_span, sel.num_rels);
    const bool resident = p.n_chunks == 1;
    const bool diag = sel.exclude_self && m0 == n0;

    const float bound = tm_bound<P, HIST>(sel);

    int f_base, f_cnt;
    mine_filter_load(sel.tile_ptr, sel.tile_ent, blockIdx.y * gridDim.x + blockIdx.x, flist, tl, &f_base, &f_cnt);   // every group: the same words
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += TM_THREADS) hist_s[i] = 0u;
    if (resident) {
        tm_stage(As, p.en, m0, n, p.dim, 0, p.dim);
        tm_stage(Bs, p.en, n0, n, p.dim, 0, p.dim);
    }
    const float* a_ptr = As + 4 * ty;
    const float* b_ptr = Bs + 4 * tx;

    // group g takes relations r0 + g, r0 + g + TM_GROUPS, ...; every group makes every round's barriers, with or without a relation
    for (int rb = r0; rb < r1; rb += TM_GROUPS) {
        const int r = rb + g;
        const bool live = r < r1;
        __syncthreads();                                 // the last round's reads of Rs and fmask are over
        if (tl < 64) fmask[g][tl] = 0ull;
        if (tl == 64) fany[g] = 0;
        if (resident && live)
            for (int k = tl; k < p.dim; k += 256) Rs[k] = p.rn[(size_t)r * p.dim + k];
        __syncthreads();
        if (live) mine_filter_relation(flist, sel.tile_ent, f_base, f_cnt, r, tl, fmask[g], &fany[g]);

        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
        bool past = !live;                               // wave-uniform: every pair of the wave is beyond the bound
        for (int c = 0; c < p.n_chunks; ++c) {
            const int k0 = c * kc, kn = min(kc, p.dim - k0);
            if (!resident) {
                __syncthreads();
                tm_stage(As, p.en, m0, n, p.dim, k0, kn);
                tm_stage(Bs, p.en, n0, n, p.dim, k0, kn);
                if (live)
                    for (int k = tl; k < kn; k += 256) Rs[k] = p.rn[(size_t)r * p.dim + k0 + k];
                __syncthreads();
            }
            for (int kb = 0; kb < kn && !past; kb += TM_CHECK) {
                const int ke = min(kb + TM_CHECK, kn);
#pragma unroll 4
                for (int k = kb; k < ke; ++k) {
                    const float4 qa = *reinterpret_cast<const float4*>(a_ptr + k * TM_LD);
                    const float4 eb = *reinterpret_cast<const float4*>(b_ptr + k * TM_LD);
                    const float rv = Rs[k];
                    const float qv[4] = {qa.x + rv, qa.y + rv, qa.z + rv, qa.w + rv}, ev[4] = {eb.x, eb.y, eb.z, eb.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[a][b] = te_pair_term(acc[a][b], qv[a], ev[b], P);
                }
                bool all_past = true;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) all_past = all_past && acc[a][b] > bound;
                past = __all(all_past) != 0;
            }
        }
        __syncthreads();                                 // fmask / fany of this round are complete

        // ---- epilogue (k_mine.h): lane (tx, ty) holds subjects 4 ty + a, objects 4 tx + b
        unsigned key[4][4];
        bool want = false;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (P == 2) acc[a][b] = sqrtf(acc[a][b]);
                const int rl = 4 * ty + a, cl = 4 * tx + b;
                unsigned k = mine_key(-acc[a][b]);
                if (!live || m0 + rl >= n || n0 + cl >= n || (diag && rl == cl)) k = 0u;
                key[a][b] = mine_gate<HIST>(k, sel);
                want = want || key[a][b] != 0u;
            }
        if (__ballot(want) == 0ull) continue;
        const bool listed = fany[g] != 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                mine_take<HIST>(key[a][b], __float_as_int(acc[a][b]), 4 * ty + a, 4 * tx + b, m0, n0, r, lane, listed, fmask[g], hist_s, sel);
    }
    if (HIST) {
        __syncthreads();
        if (t < 256) mine_hist_flush(hist_s, sel, t);
    }
}

template <int P, bool HIST>
static int tm_launch(const TeMineParams& p, dim3 grid, int lds, int lds_max, hipStream_t st) {
    static unsigned long long raised = 0;
    if (!raise_dynamic_lds((const void*)k_transe_mine<P, HIST>, lds_max, raised, "gv_transe_mine")) return GV_ERR_SHAPE;
    hipLaunchKernelGGL((k_transe_mine<P, HIST>), grid, dim3(TM_THREADS), lds, st, p);
    return launch_status("gv_transe_mine");
}

// ---- the type-constrained sweep (gv_transe_mine_typed) -----------------------------------------------------------------------------
// Loop order, transposed (k_mine.h): a workgroup owns one unit = (relation r, one 64-row tile of r's subject members, a span of
// 64-row tiles of r's object members), rows gathered through the member ids.  No second relation can reuse an object tile (its rows
// are r's list), so the four groups of 256 threads that k_transe_mine spreads over four relations here take four OBJECT tiles of
// the span against the one subject tile and the one row of rn: five tiles at a time, in TMT_KC-column chunks (5 x 68 x 64 floats =
// 85 KiB + 20 KiB static: one workgroup of 16 waves a compute unit, the occupancy of k_transe_mine).  The 16 accumulators live
// across a pair's chunks and te_pair_term walks the columns in order, so a distance is k_transe_mine's bit for bit; the monotone
// early exit is kept per wave, and a round whose every wave is past the bound stops staging chunks.
constexpr int TMT_KC = 64;

struct TeMineTypedParams {
    TeMineParams p;
    MineTyped ty;
};

// columns [k0, k0 + kn) of the rows ids_s[0 .. 63] of en into dst [kn][TM_LD] by `threads` threads tl; zeros for id -1
__device__ __forceinline__ void tm_stage_gather(float* dst, const float* __restrict__ en, const int* ids_s, int dim, int k0, int kn,
                                                int tl, int threads) {
    for (int x = tl; x < TE_TQ * kn; x += threads) {
        const int row = x / kn, k = x - row * kn, id = ids_s[row];
        dst[k * TM_LD + row] = id >= 0 ? en[(size_t)id * dim + k0 + k] : 0.f;
    }
}

template <int P, bool HIST>
__global__ __launch_bounds__(TM_THREADS) void k_transe_mine_typed(const TeMineTypedParams tp) {
    extern __shared__ __attribute__((aligned(16))) float tm_smem[];
    __shared__ unsigned long long fmask[TM_GROUPS][64];  // a group's object tile: its listed objects per subject row
    __shared__ int sid_s[64], oid_s[TM_GROUPS][64];      // the tiles' entity ids, -1 past the lists
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const TeMineParams& p = tp.p;
    const MineTyped& ty = tp.ty;
    const MineSelect& sel = p.sel;
    const int kc = p.kc;
    const int t = threadIdx.x, g = t >> 8, tl = t & 255, lane = t & 63, tx = tl & 15, ty4 = tl >> 4;
    float* As = tm_smem;                                 // [kc][TM_LD] subjects
    float* Bs = As + (1 + g) * kc * TM_LD;               // [TM_GROUPS][kc][TM_LD] each group's objects
    float* Rs = As + (1 + TM_GROUPS) * kc * TM_LD;       // [kc] the relation's row
    const int4 unit = ty.units[blockIdx.x];
    const int r = unit.x;
    if (r < 0 || r >= sel.num_rels) return;              // uniform: not a unit
    const float bound = tm_bound<P, HIST>(sel);

    mine_typed_ids(ty, sel.num_rels + r, unit.y, sel.n, t, sid_s);
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += TM_THREADS) hist_s[i] = 0u;
    const float* a_ptr = As + 4 * ty4;
    const float* b_ptr = Bs + 4 * tx;

    // group g takes object tiles unit.z + g, unit.z + g + TM_GROUPS, ...; every group makes every round's barriers
    for (int ob = unit.z; ob < unit.w; ob += TM_GROUPS) {
        const int ot = ob + g;
        const bool live = ot < unit.w;
        __syncthreads();                                 // the last round's reads of oid_s and fmask are over; sid_s is there
        mine_typed_ids(ty, r, live ? ot : -1, sel.n, tl, oid_s[g]);
        if (tl < 64) fmask[g][tl] = 0ull;
        __syncthreads();
        if (live) mine_typed_filter(ty, sel.num_rels, r, sid_s, oid_s[g], tl, fmask[g]);

        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
        bool past = !live;                               // wave-uniform: every pair of the wave is beyond the bound
        for (int k0 = 0; k0 < p.dim; k0 += kc) {
            const int kn = min(kc, p.dim - k0);
            if (__syncthreads_and(past)) break;          // the last chunk's reads are over; nothing left to look at: uniform
            tm_stage_gather(As, p.en, sid_s, p.dim, k0, kn, t, TM_THREADS);
            if (live) tm_stage_gather(Bs, p.en, oid_s[g], p.dim, k0, kn, tl, 256);
            for (int k = t; k < kn; k += TM_THREADS) Rs[k] = p.rn[(size_t)r * p.dim + k0 + k];
            __syncthreads();
            for (int kb = 0; kb < kn && !past; kb += TM_CHECK) {
                const int ke = min(kb + TM_CHECK, kn);
#pragma unroll 4
                for (int k = kb; k < ke; ++k) {
                    const float4 qa = *reinterpret_cast<const float4*>(a_ptr + k * TM_LD);
                    const float4 eb = *reinterpret_cast<const float4*>(b_ptr + k * TM_LD);
                    const float rv = Rs[k];
                    const float qv[4] = {qa.x + rv, qa.y + rv, qa.z + rv, qa.w + rv}, ev[4] = {eb.x, eb.y, eb.z, eb.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[a][b] = te_pair_term(acc[a][b], qv[a], ev[b], P);
                }
                bool all_past = true;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) all_past = all_past && acc[a][b] > bound;
                past = __all(all_past) != 0;
            }
        }
        __syncthreads();                                 // fmask of this round is complete

        // ---- epilogue (k_mine.h): lane (tx, ty4) holds subjects 4 ty4 + a, objects 4 tx + b, ids through the member lists
        unsigned key[4][4];
        bool want = false;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (P == 2) acc[a][b] = sqrtf(acc[a][b]);
                const int s = sid_s[4 * ty4 + a], o = oid_s[g][4 * tx + b];
                unsigned k = mine_key(-acc[a][b]);
                if (!live || s < 0 || o < 0 || (sel.exclude_self && s == o)) k = 0u;
                key[a][b] = mine_gate<HIST>(k, sel);
                want = want || key[a][b] != 0u;
            }
        if (__ballot(want) == 0ull) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int rl = 4 * ty4 + a, cl = 4 * tx + b;
                const bool ok = key[a][b] != 0u && !((fmask[g][rl] >> cl) & 1ull);
                mine_put<HIST>(ok, key[a][b], __float_as_int(acc[a][b]), sid_s[rl], r, oid_s[g][cl], lane, hist_s, sel);
            }
    }
    if (HIST) {
        __syncthreads();
        if (t < 256) mine_hist_flush(hist_s, sel, t);
    }
}

template <int P, bool HIST>
static int tmt_launch(const TeMineTypedParams& tp, unsigned n_units, int lds, hipStream_t st) {
    static unsigned long long raised = 0;
    const int lds_max = ((1 + TM_GROUPS) * TM_LD + 1) * TMT_KC * (int)sizeof(float);
    if (!raise_dynamic_lds((const void*)k_transe_mine_typed<P, HIST>, lds_max, raised, "gv_transe_mine_typed")) return GV_ERR_SHAPE;
    hipLaunchKernelGGL((k_transe_mine_typed<P, HIST>), dim3(n_units), dim3(TM_THREADS), lds, st, tp);
    return launch_status("gv_transe_mine_typed");
}

}  // namespace gv

using namespace gv;

extern "C" int64_t gv_transe_mine_workspace_bytes(int n, int num_rels, int n_filt_ent) {
    (void)num_rels;
    return mine_filter_workspace_bytes(n, n_filt_ent);
}

extern "C" int gv_transe_mine(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm, const int32_t* filt_lo,
                              const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int exclude_self, int mode,
                              uint32_t key_min, int prefix_bits, uint32_t prefix, int bin_bits, int32_t* out, int64_t capacity,
                              uint64_t* counter, uint64_t* hist, void* workspace, int64_t workspace_bytes, void* stream) {
    GV_REQUIRE(dim >= 1 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2), GV_ERR_SHAPE,
               "gv_transe_mine: dim=%d (1..%d) p_norm=%d (1 or 2)", dim, GV_TRANSE_MAX_DIM, p_norm);
    GV_REQUIRE(n <= 0 || (en && rn), GV_ERR_NULL, "gv_transe_mine: NULL table");
    hipStream_t st = (hipStream_t)stream;
    TeMineParams p{};
    dim3 grid;
    const int rc = mine_prepare("gv_transe_mine", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, key_min,
                                prefix_bits, prefix, bin_bits, out, capacity, counter, hist, workspace, workspace_bytes, st, &p.sel, &grid);
    if (rc != GV_OK || n == 0) return rc;
    p.en = en; p.rn = rn; p.dim = dim;
    p.kc = std::min(dim, TM_KC_MAX);
    p.n_chunks = (dim + p.kc - 1) / p.kc;
    const int lds = (2 * TM_LD + TM_GROUPS) * p.kc * (int)sizeof(float);
    const int lds_max = (2 * TM_LD + TM_GROUPS) * TM_KC_MAX * (int)sizeof(float);
    if (mode == GV_MINE_EMIT) return p_norm == 1 ? tm_launch<1, false>(p, grid, lds, lds_max, st) : tm_launch<2, false>(p, grid, lds, lds_max, st);
    return p_norm == 1 ? tm_launch<1, true>(p, grid, lds, lds_max, st) : tm_launch<2, true>(p, grid, lds, lds_max, st);
}

extern "C" int gv_transe_mine_typed(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm, const int64_t* set_ptr,
                                    const int32_t* set_ids, const int32_t* units, int64_t n_units, const int32_t* filt_lo,
                                    const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int exclude_self, int mode,
                                    uint32_t key_min, int prefix_bits, uint32_t prefix, int bin_bits, int32_t* out, int64_t capacity,
                                    uint64_t* counter, uint64_t* hist, void* stream) {
    GV_REQUIRE(dim >= 1 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2), GV_ERR_SHAPE,
               "gv_transe_mine_typed: dim=%d (1..%d) p_norm=%d (1 or 2)", dim, GV_TRANSE_MAX_DIM, p_norm);
    GV_REQUIRE(n <= 0 || (en && rn), GV_ERR_NULL, "gv_transe_mine_typed: NULL table");
    hipStream_t st = (hipStream_t)stream;
    TeMineTypedParams tp{};
    TeMineParams& p = tp.p;
    const int rc = mine_typed_prepare("gv_transe_mine_typed", n, num_rels, set_ptr, set_ids, units, n_units, filt_lo, filt_hi, filt_ent,
                                      n_filt_ent, exclude_self, mode, key_min, prefix_bits, prefix, bin_bits, out, capacity, counter, hist,
                                      st, &p.sel, &tp.ty);
    if (rc != GV_OK || n == 0 || n_units == 0) return rc;
    p.en = en; p.rn = rn; p.dim = dim;
    p.kc = std::min(dim, TMT_KC);
    p.n_chunks = (dim + p.kc - 1) / p.kc;
    const int lds = ((1 + TM_GROUPS) * TM_LD + 1) * p.kc * (int)sizeof(float);
    const unsigned nu = (unsigned)n_units;
    if (mode == GV_MINE_EMIT) return p_norm == 1 ? tmt_launch<1, false>(tp, nu, lds, st) : tmt_launch<2, false>(tp, nu, lds, st);
    return p_norm == 1 ? tmt_launch<1, true>(tp, nu, lds, st) : tmt_launch<2, true>(tp, nu, lds, st);
}
