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
// The type-constrained sweep gv_transe_mine_typed (k_transe_mine_typed, further down) walks the transposed order over gathered rows.
// The two kernels own their loop order, barriers and LDS layout and share the rest: tm_stage_rows (one stager, the row source a
// callable), tm_bound and tm_columns (the column loop with its early exit, so a distance is the same whichever sweep computed it),
// the selection rule of k_mine.h (keys of -d: larger = nearer, 0 = NaN only; candidates, gate, filter, EMIT / HIST: through
// tm_epilogue and mine_select16 in the typed kernel, written out in k_transe_mine, which is two VGPRs and 1 % of an L2 top-K run
// better off that way) and, on the host, tm_params and what every mining entry does before its launch (MineCall, mine_prepare /
// mine_typed_prepare, mine_launch: k_mine.h, k_mine.hip).  A record's fourth word is the bits of d itself (never -0: the sums start
// at +0 and add |.| or squares).
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

// columns [k0, k0 + kn) of 64 rows of en into dst [kn][TM_LD] by `threads` threads tl: local row `row` is table row row_of(row), or
// zeros when that is outside [0, n) (past the table's end; -1 past a member list)
template <class RowOf>
__device__ __forceinline__ void tm_stage_rows(float* dst, const float* __restrict__ en, RowOf row_of, int n, int dim, int k0, int kn,
                                              int tl, int threads) {
    for (int x = tl; x < TE_TQ * kn; x += threads) {
        const int row = x / kn, k = x - row * kn, id = row_of(row);
        dst[k * TM_LD + row] = (unsigned)id < (unsigned)n ? en[(size_t)id * dim + k0 + k] : 0.f;
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

// kn staged columns into a lane's 4 x 4 accumulators: subjects a_ptr[k * TM_LD + 0 .. 3] + Rs[k] against objects b_ptr[k * TM_LD +
// 0 .. 3], te_pair_term in column order.  Both sweeps run their arithmetic here, so a distance does not depend on which of them
// computed it.  `past` (wave-uniform) is set once every pair of the wave is beyond `bound`, looked at every TM_CHECK columns; a
// wave that comes in past does nothing.
template <int P>
__device__ __forceinline__ void tm_columns(float (&acc)[4][4], const float* a_ptr, const float* b_ptr, const float* Rs, int kn, float bound,
                                           bool& past) {
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

// The typed kernel's epilogue (k_mine.h: mine_select16) for lane (tx, ty), which holds local rows 4 ty + a and columns 4 tx + b of the tile pair:
// sqrtf for p = 2, the key of -d.  ids_of(rl, cl) is the candidate's (s, o), an id outside [0, n) for none; `live` false: the
// lane's group has nothing this round; `exclude`: s == o is to be dropped and can occur here.  A record's value is d itself.
template <int P, bool HIST, class IdsOf>
__device__ __forceinline__ void tm_epilogue(float (&acc)[4][4], bool live, bool exclude, int tx, int ty, int lane, IdsOf ids_of, int r,
                                            bool listed, const unsigned long long* mask, unsigned* hist_s, const MineSelect& sel) {
    mine_select16<HIST>(
        live, exclude,
        [&](int i) {
            float& d = acc[i >> 2][i & 3];
            if (P == 2) d = sqrtf(d);
            return mine_key(-d);
        },
        [&](int i) {
            const int rl = 4 * ty + (i >> 2), cl = 4 * tx + (i & 3);
            const int2 so = ids_of(rl, cl);
            return make_int4(rl, cl, so.x, so.y);
        },
        [&](int i, unsigned) { return __float_as_int(acc[i >> 2][i & 3]); }, r, listed, mask, lane, hist_s, sel);
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
    const auto s_row = [=](int rl) { return m0 + rl; };                   // table rows of the tiles' local rows, >= n past the table
    const auto o_row = [=](int cl) { return n0 + cl; };
    const float bound = tm_bound<P, HIST>(sel);

    int f_base, f_cnt;
    mine_filter_load(sel.tile_ptr, sel.tile_ent, blockIdx.y * gridDim.x + blockIdx.x, flist, tl, &f_base, &f_cnt);   // every group: the same words
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += TM_THREADS) hist_s[i] = 0u;
    if (resident) {
        tm_stage_rows(As, p.en, s_row, n, p.dim, 0, p.dim, t, TM_THREADS);
        tm_stage_rows(Bs, p.en, o_row, n, p.dim, 0, p.dim, t, TM_THREADS);
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
                tm_stage_rows(As, p.en, s_row, n, p.dim, k0, kn, t, TM_THREADS);
                tm_stage_rows(Bs, p.en, o_row, n, p.dim, k0, kn, t, TM_THREADS);
                if (live)
                    for (int k = tl; k < kn; k += 256) Rs[k] = p.rn[(size_t)r * p.dim + k0 + k];
                __syncthreads();
            }
            tm_columns<P>(acc, a_ptr, b_ptr, Rs, kn, bound, past);
        }
        __syncthreads();                                 // fmask / fany of this round are complete

        // ---- epilogue, this kernel's own: lane (tx, ty) holds subjects 4 ty + a, objects 4 tx + b.  It is the rule of mine_select16
        // (k_mine.h) with positional ids, written out: through mine_select16 this kernel took two more VGPRs for p = 1 and an L2
        // top-K run 1 % longer (profiles/mine_shared).  Change the two together.
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
            for (int b = 0; b < 4; ++b) {
                const int rl = 4 * ty + a, cl = 4 * tx + b;
                bool ok = key[a][b] != 0u;
                if (listed && ok) ok = !((fmask[g][rl] >> cl) & 1ull);
                mine_put<HIST>(ok, key[a][b], __float_as_int(acc[a][b]), m0 + rl, r, n0 + cl, lane, hist_s, sel);
            }
    }
    if (HIST) {
        __syncthreads();
        if (t < 256) mine_hist_flush(hist_s, sel, t);
    }
}

// ---- the whole-graph sweep with selection state per relation (gv_transe_mine_by_relation) -------------------------------------------
// k_transe_mine's loop order, staging and arithmetic over the SLOTS' relations (k_mine.h: MineSlots): a workgroup owns its tile pair
// and the slots [blockIdx.z * rel_span, + rel_span), whose LIVE ones its four groups take in turn, four a round; an empty slot costs
// one scalar load, so a subset of the relations costs its share of a sweep.  Four slots are in flight at once, so everything a slot
// owns is the GROUP's: the select narrowed to the slot (mine_slot_select; all four waves of a group read the same slot, the values
// stay wave-uniform), the early-exit bound taken from THAT select every round -- the slots' prefixes and thresholds differ, and a
// bound shared between them would let the partial sums of the relation with the larger distances leave the column loop early and be
// counted in the wrong bins --, and one 256-bin LDS histogram per group (levels 8 + 8 + 8 + 8).  A group's histogram is complete at
// the next round's first barrier and is flushed into its slot's global histogram right behind it (mine_hist_flush_clear), two
// barriers before the group counts into it again; the last one is flushed behind the barrier after the loop.  No barrier is added
// to k_transe_mine's.
struct TeMineRelParams {
    TeMineParams p;
    MineSlots sl;
};

template <int P, bool HIST>
__global__ __launch_bounds__(TM_THREADS) void k_transe_mine_rel(const TeMineRelParams rp) {
    extern __shared__ __attribute__((aligned(16))) float tm_smem[];
    __shared__ unsigned long long fmask[TM_GROUPS][64];  // a group's relation: its listed objects per subject row
    __shared__ int fany[TM_GROUPS];
    __shared__ unsigned flist[MINE_FL_CAP];
    __shared__ unsigned hist_s[HIST ? TM_GROUPS : 1][HIST ? (1 << MINE_SLOT_HIST_BITS) : 1];
    const TeMineParams& p = rp.p;
    const MineSlots& sl = rp.sl;
    const int kc = p.kc;
    float* As = tm_smem;                                 // [kc][TM_LD] subjects
    float* Bs = As + kc * TM_LD;                         // [kc][TM_LD] objects
    const int t = threadIdx.x, tl = t & 255, lane = t & 63, tx = tl & 15, ty = tl >> 4;
    const int g = (int)mine_uniform((unsigned)(t >> 8));
    float* Rs = Bs + kc * TM_LD + g * kc;                // [TM_GROUPS][kc] each group's relation row
    unsigned* const hist_g = hist_s[HIST ? g : 0];       // and its histogram
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const MineSelect& pass = p.sel;
    const int n = pass.n;
    const int i0 = blockIdx.z * pass.rel_span, i1 = min(i0 + pass.rel_span, sl.m);
    const bool resident = p.n_chunks == 1;
    const bool diag = pass.exclude_self && m0 == n0;
    const auto s_row = [=](int rl) { return m0 + rl; };
    const auto o_row = [=](int cl) { return n0 + cl; };
    const auto live_from = [&](int i) {                  // the first live slot at or after i, i1 when there is none (uniform)
        while (i < i1 && mine_slot_relation(sl, i, pass.num_rels) < 0) ++i;
        return i;
    };

    int i = live_from(i0);
    if (i >= i1) return;                                 // uniform: no live slot in this span
    int f_base, f_cnt;
    mine_filter_load(pass.tile_ptr, pass.tile_ent, blockIdx.y * gridDim.x + blockIdx.x, flist, tl, &f_base, &f_cnt);   // every group: the same words
    if (HIST) hist_g[tl] = 0u;                           // 256 threads a group, 256 bins
    if (resident) {
        tm_stage_rows(As, p.en, s_row, n, p.dim, 0, p.dim, t, TM_THREADS);
        tm_stage_rows(Bs, p.en, o_row, n, p.dim, 0, p.dim, t, TM_THREADS);
    }
    const float* a_ptr = As + 4 * ty;
    const float* b_ptr = Bs + 4 * tx;

    int before = -1;                                     // the slot whose histogram waits in hist_s[g]
    while (i < i1) {
        int mine = -1;                                   // this round's live slots, one a group; every group makes every round's barriers
        for (int j = 0; j < TM_GROUPS && i < i1; ++j) {
            if (j == g) mine = i;
            i = live_from(i + 1);
        }
        const int r = mine_slot_relation(sl, mine, pass.num_rels);
        const bool live = r >= 0;
        const MineSelect sel = mine_slot_select<HIST>(pass, sl, live ? mine : i0);     // a group without a slot reads a valid one and uses nothing of it
        const float bound = tm_bound<P, HIST>(sel);      // the slot's own: never the pass's
        __syncthreads();                                 // the last round's reads of Rs and fmask and its counts into hist_s are over
        if (HIST && before >= 0)
            mine_hist_flush_clear(hist_g, pass.hist + ((size_t)before << pass.bin_bits), pass.bin_bits, tl);
        if (tl < 64) fmask[g][tl] = 0ull;
        if (tl == 64) fany[g] = 0;
        if (resident && live)
            for (int k = tl; k < p.dim; k += 256) Rs[k] = p.rn[(size_t)r * p.dim + k];
        __syncthreads();
        if (live) mine_filter_relation(flist, pass.tile_ent, f_base, f_cnt, r, tl, fmask[g], &fany[g]);

        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
        bool past = !live;                               // wave-uniform: every pair of the wave is beyond the slot's bound
        for (int c = 0; c < p.n_chunks; ++c) {
            const int k0 = c * kc, kn = min(kc, p.dim - k0);
            if (!resident) {
                __syncthreads();
                tm_stage_rows(As, p.en, s_row, n, p.dim, k0, kn, t, TM_THREADS);
                tm_stage_rows(Bs, p.en, o_row, n, p.dim, k0, kn, t, TM_THREADS);
                if (live)
                    for (int k = tl; k < kn; k += 256) Rs[k] = p.rn[(size_t)r * p.dim + k0 + k];
                __syncthreads();
            }
            tm_columns<P>(acc, a_ptr, b_ptr, Rs, kn, bound, past);
        }
        __syncthreads();                                 // fmask / fany of this round are complete

        tm_epilogue<P, HIST>(acc, live, diag, tx, ty, lane, [&](int rl, int cl) { return make_int2(s_row(rl), o_row(cl)); }, r,
                             fany[g] != 0, fmask[g], hist_g, sel);
        before = live ? mine : -1;
    }
    if (HIST) {
        __syncthreads();
        if (before >= 0) mine_hist_flush_clear(hist_g, pass.hist + ((size_t)before << pass.bin_bits), pass.bin_bits, tl);
    }
}

// ---- the type-constrained sweep (gv_transe_mine_typed) -----------------------------------------------------------------------------
// Loop order, transposed (k_mine.h): a workgroup owns one unit = (relation r, one 64-row tile of r's subject members, a span of
// 64-row tiles of r's object members), rows gathered through the member ids.  No second relation can reuse an object tile (its rows
// are r's list), so the four groups of 256 threads that k_transe_mine spreads over four relations here take four OBJECT tiles of
// the span against the one subject tile and the one row of rn: five tiles at a time, in TMT_KC-column chunks (5 x 68 x 64 floats =
// 85 KiB + 20 KiB static: one workgroup of 16 waves a compute unit, the occupancy of k_transe_mine).  The 16 accumulators live
// across a pair's chunks and tm_columns walks the columns in order, so a distance is k_transe_mine's bit for bit; the monotone
// early exit is kept per wave, and a round whose every wave is past the bound stops staging chunks.
constexpr int TMT_KC = 64;

struct TeMineTypedParams {
    TeMineParams p;
    MineTyped ty;
};

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
            tm_stage_rows(As, p.en, [&](int row) { return sid_s[row]; }, sel.n, p.dim, k0, kn, t, TM_THREADS);
            if (live) tm_stage_rows(Bs, p.en, [&](int row) { return oid_s[g][row]; }, sel.n, p.dim, k0, kn, tl, 256);
            for (int k = t; k < kn; k += TM_THREADS) Rs[k] = p.rn[(size_t)r * p.dim + k0 + k];
            __syncthreads();
            tm_columns<P>(acc, a_ptr, b_ptr, Rs, kn, bound, past);
        }
        __syncthreads();                                 // fmask of this round is complete

        // ids through the member lists, -1 past them and for a group without a tile; fmask is always read
        tm_epilogue<P, HIST>(acc, live, sel.exclude_self != 0, tx, ty4, lane,
                             [&](int rl, int cl) { return make_int2(sid_s[rl], oid_s[g][cl]); }, r, true, fmask[g], hist_s, sel);
    }
    if (HIST) {
        __syncthreads();
        if (t < 256) mine_hist_flush(hist_s, sel, t);
    }
}

// ---- the type-constrained sweep with selection state per relation (gv_transe_mine_typed_by_relation) -------------------------------
// k_transe_mine_typed, a unit's first word being the SLOT whose relation it walks (as k_mine_typed_rel, k_mine.hip): the workgroup
// owns one relation already, so the selection is narrowed to the slot once (mine_slot_select), the bound comes from that select, and
// the 4 096-bin LDS histogram, its 12 + 10 + 10 levels and its one flush stay k_transe_mine_typed's; only their destination is the
// slot's.
struct TeMineTypedRelParams {
    TeMineParams p;
    MineTyped ty;
    MineSlots sl;
};

template <int P, bool HIST>
__global__ __launch_bounds__(TM_THREADS) void k_transe_mine_typed_rel(const TeMineTypedRelParams tp) {
    extern __shared__ __attribute__((aligned(16))) float tm_smem[];
    __shared__ unsigned long long fmask[TM_GROUPS][64];  // a group's object tile: its listed objects per subject row
    __shared__ int sid_s[64], oid_s[TM_GROUPS][64];      // the tiles' entity ids, -1 past the lists
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const TeMineParams& p = tp.p;
    const MineTyped& ty = tp.ty;
    const int kc = p.kc;
    const int t = threadIdx.x, g = t >> 8, tl = t & 255, lane = t & 63, tx = tl & 15, ty4 = tl >> 4;
    float* As = tm_smem;                                 // [kc][TM_LD] subjects
    float* Bs = As + (1 + g) * kc * TM_LD;               // [TM_GROUPS][kc][TM_LD] each group's objects
    float* Rs = As + (1 + TM_GROUPS) * kc * TM_LD;       // [kc] the relation's row
    const int4 unit = ty.units[blockIdx.x];
    const int slot = (int)mine_uniform((unsigned)unit.x);
    const int r = mine_slot_relation(tp.sl, slot, p.sel.num_rels);
    if (r < 0) return;                                   // uniform: not a unit, or an empty slot
    const MineSelect sel = mine_slot_select<HIST>(p.sel, tp.sl, slot);
    const float bound = tm_bound<P, HIST>(sel);          // the slot's

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
            tm_stage_rows(As, p.en, [&](int row) { return sid_s[row]; }, sel.n, p.dim, k0, kn, t, TM_THREADS);
            if (live) tm_stage_rows(Bs, p.en, [&](int row) { return oid_s[g][row]; }, sel.n, p.dim, k0, kn, tl, 256);
            for (int k = t; k < kn; k += TM_THREADS) Rs[k] = p.rn[(size_t)r * p.dim + k0 + k];
            __syncthreads();
            tm_columns<P>(acc, a_ptr, b_ptr, Rs, kn, bound, past);
        }
        __syncthreads();                                 // fmask of this round is complete

        tm_epilogue<P, HIST>(acc, live, sel.exclude_self != 0, tx, ty4, lane,
                             [&](int rl, int cl) { return make_int2(sid_s[rl], oid_s[g][cl]); }, r, true, fmask[g], hist_s, sel);
    }
    if (HIST) {
        __syncthreads();
        if (t < 256) mine_hist_flush(hist_s, sel, t);
    }
}

// What both entries check of their tables and the norm; then *p filled but for the selection, in chunks of at most kc_max columns.
static int tm_params(const char* who, const float* en, const float* rn, int n, int dim, int p_norm, int kc_max, TeMineParams* p) {
    GV_REQUIRE(dim >= 1 && dim <= GV_TRANSE_MAX_DIM && (p_norm == 1 || p_norm == 2), GV_ERR_SHAPE, "%s: dim=%d (1..%d) p_norm=%d (1 or 2)",
               who, dim, GV_TRANSE_MAX_DIM, p_norm);
    GV_REQUIRE(n <= 0 || (en && rn), GV_ERR_NULL, "%s: NULL table", who);
    p->en = en; p->rn = rn; p->dim = dim;
    p->kc = std::min(dim, kc_max);
    p->n_chunks = (dim + p->kc - 1) / p->kc;
    return GV_OK;
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
    const MineCall c{"gv_transe_mine", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, key_min, prefix_bits,
                     prefix, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    TeMineParams p{};
    dim3 grid;
    int rc = tm_params(c.who, en, rn, n, dim, p_norm, TM_KC_MAX, &p);
    if (rc == GV_OK) rc = mine_prepare(c, workspace, workspace_bytes, &p.sel, &grid);
    if (rc != GV_OK || n == 0) return rc;
    const int lds = (2 * TM_LD + TM_GROUPS) * p.kc * (int)sizeof(float);
    const int lds_max = (2 * TM_LD + TM_GROUPS) * TM_KC_MAX * (int)sizeof(float);
    if (mode == GV_MINE_EMIT)
        return p_norm == 1 ? mine_launch<k_transe_mine<1, false>>(p, grid, TM_THREADS, lds, lds_max, c)
                           : mine_launch<k_transe_mine<2, false>>(p, grid, TM_THREADS, lds, lds_max, c);
    return p_norm == 1 ? mine_launch<k_transe_mine<1, true>>(p, grid, TM_THREADS, lds, lds_max, c)
                       : mine_launch<k_transe_mine<2, true>>(p, grid, TM_THREADS, lds, lds_max, c);
}

extern "C" int gv_transe_mine_typed(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm, const int64_t* set_ptr,
                                    const int32_t* set_ids, const int32_t* units, int64_t n_units, const int32_t* filt_lo,
                                    const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int exclude_self, int mode,
                                    uint32_t key_min, int prefix_bits, uint32_t prefix, int bin_bits, int32_t* out, int64_t capacity,
                                    uint64_t* counter, uint64_t* hist, void* stream) {
    const MineCall c{"gv_transe_mine_typed", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, key_min,
                     prefix_bits, prefix, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    TeMineTypedParams tp{};
    int rc = tm_params(c.who, en, rn, n, dim, p_norm, TMT_KC, &tp.p);
    if (rc == GV_OK) rc = mine_typed_prepare(c, set_ptr, set_ids, units, n_units, &tp.p.sel, &tp.ty);
    if (rc != GV_OK || n == 0 || n_units == 0) return rc;
    const int lds = ((1 + TM_GROUPS) * TM_LD + 1) * tp.p.kc * (int)sizeof(float);
    const int lds_max = ((1 + TM_GROUPS) * TM_LD + 1) * TMT_KC * (int)sizeof(float);
    const dim3 grid((unsigned)n_units);
    if (mode == GV_MINE_EMIT)
        return p_norm == 1 ? mine_launch<k_transe_mine_typed<1, false>>(tp, grid, TM_THREADS, lds, lds_max, c)
                           : mine_launch<k_transe_mine_typed<2, false>>(tp, grid, TM_THREADS, lds, lds_max, c);
    return p_norm == 1 ? mine_launch<k_transe_mine_typed<1, true>>(tp, grid, TM_THREADS, lds, lds_max, c)
                       : mine_launch<k_transe_mine_typed<2, true>>(tp, grid, TM_THREADS, lds, lds_max, c);
}

extern "C" int gv_transe_mine_by_relation(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm,
                                          const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent,
                                          int exclude_self, int mode, const int32_t* rels, int m, const uint32_t* key_min,
                                          int prefix_bits, const uint32_t* prefix, int bin_bits, int32_t* out, int64_t capacity,
                                          const int64_t* out_base, uint64_t* counter, uint64_t* hist, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    const MineCall c{"gv_transe_mine_by_relation", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, 0u,
                     prefix_bits, 0u, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    TeMineRelParams rp{};
    dim3 grid;
    int rc = tm_params(c.who, en, rn, n, dim, p_norm, TM_KC_MAX, &rp.p);
    if (rc == GV_OK) rc = mine_select_args(c, &rp.p.sel);
    if (rc == GV_OK) rc = mine_slots_args(c, rels, m, key_min, prefix, out_base, MINE_SLOT_HIST_BITS, &rp.sl);
    if (rc != GV_OK || n == 0) return rc;
    rc = mine_slots_prepare(c, m, workspace, workspace_bytes, &rp.p.sel, &grid);
    if (rc != GV_OK) return rc;
    const int lds = (2 * TM_LD + TM_GROUPS) * rp.p.kc * (int)sizeof(float);
    const int lds_max = (2 * TM_LD + TM_GROUPS) * TM_KC_MAX * (int)sizeof(float);
    if (mode == GV_MINE_EMIT)
        return p_norm == 1 ? mine_launch<k_transe_mine_rel<1, false>>(rp, grid, TM_THREADS, lds, lds_max, c)
                           : mine_launch<k_transe_mine_rel<2, false>>(rp, grid, TM_THREADS, lds, lds_max, c);
    return p_norm == 1 ? mine_launch<k_transe_mine_rel<1, true>>(rp, grid, TM_THREADS, lds, lds_max, c)
                       : mine_launch<k_transe_mine_rel<2, true>>(rp, grid, TM_THREADS, lds, lds_max, c);
}

extern "C" int gv_transe_mine_typed_by_relation(const float* en, const float* rn, int n, int num_rels, int dim, int p_norm,
                                                const int64_t* set_ptr, const int32_t* set_ids, const int32_t* units, int64_t n_units,
                                                const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent,
                                                int exclude_self, int mode, const int32_t* rels, int m, const uint32_t* key_min,
                                                int prefix_bits, const uint32_t* prefix, int bin_bits, int32_t* out, int64_t capacity,
                                                const int64_t* out_base, uint64_t* counter, uint64_t* hist, void* stream) {
    const MineCall c{"gv_transe_mine_typed_by_relation", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, 0u,
                     prefix_bits, 0u, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    TeMineTypedRelParams tp{};
    MineSelect checked;
    int rc = tm_params(c.who, en, rn, n, dim, p_norm, TMT_KC, &tp.p);
    if (rc == GV_OK) rc = mine_select_args(c, &checked);
    if (rc == GV_OK) rc = mine_slots_args(c, rels, m, key_min, prefix, out_base, MINE_HIST_BITS, &tp.sl);
    if (rc == GV_OK) rc = mine_typed_prepare(c, set_ptr, set_ids, units, n_units, &tp.p.sel, &tp.ty, m);
    if (rc != GV_OK || n == 0 || n_units == 0) return rc;
    const int lds = ((1 + TM_GROUPS) * TM_LD + 1) * tp.p.kc * (int)sizeof(float);
    const int lds_max = ((1 + TM_GROUPS) * TM_LD + 1) * TMT_KC * (int)sizeof(float);
    const dim3 grid((unsigned)n_units);
    if (mode == GV_MINE_EMIT)
        return p_norm == 1 ? mine_launch<k_transe_mine_typed_rel<1, false>>(tp, grid, TM_THREADS, lds, lds_max, c)
                           : mine_launch<k_transe_mine_typed_rel<2, false>>(tp, grid, TM_THREADS, lds, lds_max, c);
    return p_norm == 1 ? mine_launch<k_transe_mine_typed_rel<1, true>>(tp, grid, TM_THREADS, lds, lds_max, c)
                       : mine_launch<k_transe_mine_typed_rel<2, true>>(tp, grid, TM_THREADS, lds, lds_max, c);
}
