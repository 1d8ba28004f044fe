// Whole-graph triplet mining (gv_mine_scores): every (s, r, o) of a DistMult decoder scored on the f32 MFMA, selected globally.
//
//   logit[s, r, o] = (E[s] * w[r]) . E[o] + bias
//
// bit for bit gv_gemm_f32(gv_mul(E, w[r]), E^T) + bias: one f32 multiply per subject element, the k-ordered
// v_mfma_f32_32x32x2_f32 chain over k = 0 .. ceil16(h) - 1 (zeros past h, as the GEMM's 16-deep steps pad), one add.  The subject
// side carries w[r]: (E[s] * w) . E[o] and (E[o] * w) . E[s] differ in rounding, so the s <-> o symmetry is not used.
//
// Loop order: a workgroup owns one 64 x 64 (subject tile, object tile) pair and walks the RELATIONS over it.  With ceil16(h) <= 240
// both tiles of E are staged in LDS once (2 x 64 x 212 floats at h = 200) and a relation costs its 800-byte row of w; wider
// tables are staged in 240-deep k-chunks per relation.  LDS rows hold the even k of a chunk, then the odd k: lane l of the MFMA
// needs k = 2 j + (l >> 5) for consecutive j, so ONE ds_read_b128 per operand feeds four MFMAs (row pitch kc + 4 floats: the
// 16 lanes of a b128 group fall on 16 distinct 16-byte slots).
//
// The type-constrained sweep gv_mine_scores_typed (k_mine_typed, further down) walks the transposed order over gathered rows.  The
// two kernels own their loop order, barriers and staging schedule and share the rest: mine_stage_rows (one stager, the row source
// a callable), mine_mfma_chunk (the arithmetic of a staged chunk, so a logit is the same whichever sweep computed it), mine_epilogue
// (bias, keys, then the selection of k_mine.h: candidates, gate, filter, EMIT / HIST; a record's fourth word is the logit,
// mine_key_logit of its key: -0 as +0) and, on the host, mine_params and mine_launch.  This file is also the one home of what every
// mining entry does on the host before its launch (mine_select_args, mine_prepare, mine_typed_prepare on a MineCall) and of the
// three small kernels that re-bucket the filter.
//
// gv_mine_scores_by_relation / gv_mine_scores_typed_by_relation (k_mine_rel, k_mine_typed_rel) are the two sweeps with the selection
// state PER RELATION (k_mine.h: MineSlots, mine_slot_select): the loops, the staging and the arithmetic of k_mine / k_mine_typed over
// the chosen relations, each relation selected against its own threshold, prefix, histogram, counter and output segment.
#include <limits.h>

#include <algorithm>
#include <utility>

#include "common.h"
#include "k_mc.h"
#include "k_mine.h"

namespace gv {

typedef float mine_f32x16 __attribute__((ext_vector_type(16)));

constexpr int MINE_KC_MAX = 240;       // k per staged chunk (multiple of 16): 2 x 64 x 244 floats = 122 KiB of the 160

struct MineParams {
    const float* e;
    const float* w;
    const float* bias;
    int h, ld_e, ld_w;
    int vec_e, vec_w;
    int kc, n_chunks;                  // chunk depth (multiple of 16) and count; one chunk: the tiles stay in LDS
    MineSelect sel;
};

// 64 rows of E, columns [k0, k0 + kc), into LDS: row pitch kc + 4, even k first, then odd k.  Local row rl is table row row_of(rl),
// or zeros when that is outside [0, n) (past the table's end; -1 past a member list).
template <class RowOf>
__device__ __forceinline__ void mine_stage_rows(float* dst, const float* e, int ld, bool vec, RowOf row_of, int n, int k0, int h, int kc) {
    const int q4 = kc >> 2, pitch = kc + 4, half = kc >> 1;
    for (int idx = threadIdx.x; idx < 64 * q4; idx += 256) {
        const int rl = idx / q4, q = idx - rl * q4;
        const int row = row_of(rl), k = k0 + 4 * q;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)row < (unsigned)n) {
            const float* src = e + (size_t)row * ld + k;
            if (vec && k + 3 < h) {
                const float4 t = *reinterpret_cast<const float4*>(src);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = k + i < h ? src[i] : 0.f;
            }
        }
        float* d = dst + rl * pitch + 2 * q;
        *reinterpret_cast<float2*>(d) = make_float2(v[0], v[2]);
        *reinterpret_cast<float2*>(d + half) = make_float2(v[1], v[3]);
    }
}

// four floats of w[r] at k (zeros past h)
__device__ __forceinline__ float4 mine_load_w(const MineParams& p, int r, int k) {
    const float* src = p.w + (size_t)r * p.ld_w + k;
    if (p.vec_w && k + 3 < p.h) return *reinterpret_cast<const float4*>(src);
    float4 v;
    v.x = k < p.h ? src[0] : 0.f;
    v.y = k + 1 < p.h ? src[1] : 0.f;
    v.z = k + 2 < p.h ? src[2] : 0.f;
    v.w = k + 3 < p.h ? src[3] : 0.f;
    return v;
}

__device__ __forceinline__ void mine_store_w(float* ws, int kc, int t, float4 v) {      // thread t holds k = 4 t .. 4 t + 3 of the chunk
    *reinterpret_cast<float2*>(ws + 2 * t) = make_float2(v.x, v.z);
    *reinterpret_cast<float2*>(ws + (kc >> 1) + 2 * t) = make_float2(v.y, v.w);
}

// One staged chunk into a wave's 32 x 32 accumulators: `groups` groups of 8 k from the lane's a (subject row), b (object row) and w
// positions in LDS, (a * w) in f32 on the subject side, the k-ordered MFMA chain.  Both sweeps run their arithmetic here, so a
// logit does not depend on which of them computed it.  (acc goes in and out by value: by reference it costs k_mine<HIST> 4 VGPRs.)
__device__ __forceinline__ mine_f32x16 mine_mfma_chunk(mine_f32x16 acc, const float* a, const float* b, const float* w, int groups) {
    // one wave per SIMD: the next group's three reads are issued before this group's MFMAs, or their latency is exposed
    // every 256 cycles.  (The read past the last group lands in the row's / the buffer's four floats of padding: unused.)
    float4 a_n = *reinterpret_cast<const float4*>(a);
    float4 b_n = *reinterpret_cast<const float4*>(b);
    float4 w_n = *reinterpret_cast<const float4*>(w);
#pragma unroll 2
    for (int g = 0; g < groups; ++g) {
        const float4 a4 = a_n, b4 = b_n, w4 = w_n;
        a_n = *reinterpret_cast<const float4*>(a + 4 * g + 4);
        b_n = *reinterpret_cast<const float4*>(b + 4 * g + 4);
        w_n = *reinterpret_cast<const float4*>(w + 4 * g + 4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x * w4.x, b4.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y * w4.y, b4.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z * w4.z, b4.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w * w4.w, b4.w, acc, 0, 0, 0);
    }
    return acc;
}

// 8 k per group, whole 16-deep steps as the GEMM walks them
__device__ __forceinline__ int mine_groups(int kc, int h, int k0) { return (min(kc, h - k0) + 15) / 16 * 2; }

// The epilogue (k_mine.h: mine_select16) of a wave's 32 x 32 block at (wm, wn) of the tile pair, C/D map of the 32x32 MFMA: col =
// lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  ids_of(rl, cl) is the candidate's (s, o), an id outside [0, n) for
// none, `exclude` whether s == o is to be dropped and can occur here; a record's value is the logit of its key.
template <bool HIST, class IdsOf>
__device__ __forceinline__ void mine_epilogue(mine_f32x16 acc, float bv, int wm, int wn, int lane, bool exclude, IdsOf ids_of, int r,
                                              bool listed, const unsigned long long* mask, unsigned* hist_s, const MineSelect& sel) {
    const int cl = wn + (lane & 31), lhi = lane >> 5;
    mine_select16<HIST>(
        true, exclude, [&](int i) { return mine_key(acc[i] + bv); },
        [&](int i) {
            const int rl = wm + (i & 3) + 8 * (i >> 2) + 4 * lhi;
            const int2 so = ids_of(rl, cl);
            return make_int4(rl, cl, so.x, so.y);
        },
        [](int, unsigned k) { return __float_as_int(mine_key_logit(k)); }, r, listed, mask, lane, hist_s, sel);
}

template <bool HIST>
__global__ __launch_bounds__(256) void k_mine(const MineParams p) {
    extern __shared__ __attribute__((aligned(16))) float mine_smem[];
    __shared__ unsigned long long fmask[3][64];          // the relation's listed objects per subject row, three relations in flight
    __shared__ int fany[3];
    __shared__ unsigned flist[MINE_FL_CAP];
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const int kc = p.kc, pitch = kc + 4, half = kc >> 1;
    float* As = mine_smem;
    float* Bs = As + 64 * pitch;
    float* Ws = Bs + 64 * pitch;                         // [2][kc + 4]
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const MineSelect& sel = p.sel;
    const int n = sel.n;
    const int r0 = blockIdx.z * sel.rel_span, r1 = min(r0 + sel.rel_span, sel.num_rels);
    const bool resident = p.n_chunks == 1;
    const float bv = p.bias ? *p.bias : 0.f;
    const auto s_row = [=](int rl) { return m0 + rl; };                   // table rows of the tiles' local rows, >= n past the table
    const auto o_row = [=](int cl) { return n0 + cl; };

    int f_base, f_cnt;
    mine_filter_load(sel.tile_ptr, sel.tile_ent, blockIdx.y * gridDim.x + blockIdx.x, flist, t, &f_base, &f_cnt);
    if (t < 64) { fmask[0][t] = 0ull; fmask[1][t] = 0ull; fmask[2][t] = 0ull; }
    if (t < 3) fany[t] = 0;
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += 256) hist_s[i] = 0u;
    if (resident) {
        mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, sel.n, 0, p.h, kc);
        mine_stage_rows(Bs, p.e, p.ld_e, p.vec_e, o_row, sel.n, 0, p.h, kc);
        if (t < (kc >> 2) && r0 < r1) mine_store_w(Ws, kc, t, mine_load_w(p, r0, 4 * t));
    }
    __syncthreads();

    const int a_off = (wm + l31) * pitch + lhi * half, b_off = (wn + l31) * pitch + lhi * half, w_off = lhi * half;

    for (int r = r0; r < r1; ++r) {
        const int it = r - r0, fb = it % 3, wb = resident ? (it & 1) : 0;
        // this relation's listed triplets -> fmask[fb]; the buffer of the relation after it is cleared (last read two relations ago)
        if (t < 64) fmask[(it + 1) % 3][t] = 0ull;
        if (t == 64) fany[(it + 1) % 3] = 0;
        mine_filter_relation(flist, sel.tile_ent, f_base, f_cnt, r, t, fmask[fb], &fany[fb]);
        float4 wnext = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool w_pre = resident && t < (kc >> 2) && r + 1 < r1;
        if (w_pre) wnext = mine_load_w(p, r + 1, 4 * t);          // flies under the MFMA chain

        mine_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int c = 0; c < p.n_chunks; ++c) {
            const int k0 = c * kc;
            if (!resident) {
                __syncthreads();
                mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, sel.n, k0, p.h, kc);
                mine_stage_rows(Bs, p.e, p.ld_e, p.vec_e, o_row, sel.n, k0, p.h, kc);
                if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, k0 + 4 * t));
                __syncthreads();
            }
            acc = mine_mfma_chunk(acc, As + a_off, Bs + b_off, Ws + wb * (kc + 4) + w_off, mine_groups(kc, p.h, k0));
        }
        if (w_pre) mine_store_w(Ws + ((it + 1) & 1) * (kc + 4), kc, t, wnext);
        __syncthreads();

        // positional ids.  An id is >= n outside the table, and s == o exactly when the tiles coincide and rl == cl (m0, n0 are
        // multiples of 64 and rl, cl < 64): the predicate m0 + rl >= n || n0 + cl >= n || (exclude_self && m0 == n0 && rl == cl).
        mine_epilogue<HIST>(acc, bv, wm, wn, lane, sel.exclude_self && m0 == n0,
                            [&](int rl, int cl) { return make_int2(s_row(rl), o_row(cl)); }, r, fany[fb] != 0, fmask[fb], hist_s, sel);
    }
    if (HIST) {
        __syncthreads();
        mine_hist_flush(hist_s, sel, t);
    }
}

// ---- the whole-graph sweep with selection state per relation (gv_mine_scores_by_relation) -----------------------------------------
// k_mine's loop order, staging and arithmetic over the SLOTS' relations: a workgroup owns its tile pair and walks the live slots of
// [blockIdx.z * rel_span, + rel_span), so a subset of the relations costs its share of a sweep and an empty slot costs one scalar
// load.  Per relation the selection is narrowed to the slot (mine_slot_select) and handed to the same mine_epilogue.  HIST: the LDS
// histogram is the slot's, 256 bins, two of them: relation `it` counts into buffer it & 1 while the buffer of the relation before
// it -- complete since the barrier behind this relation's MFMA chain -- is flushed to that slot's global histogram and cleared
// (mine_hist_flush_clear: one LDS read per thread).  No barrier is added to k_mine's one per relation.
struct MineRelParams {
    MineParams p;
    MineSlots sl;
};

template <bool HIST>
__global__ __launch_bounds__(256) void k_mine_rel(const MineRelParams rp) {
    extern __shared__ __attribute__((aligned(16))) float mine_smem[];
    __shared__ unsigned long long fmask[3][64];          // the relation's listed objects per subject row, three relations in flight
    __shared__ int fany[3];
    __shared__ unsigned flist[MINE_FL_CAP];
    __shared__ unsigned hist_s[HIST ? 2 : 1][HIST ? (1 << MINE_SLOT_HIST_BITS) : 1];
    const MineParams& p = rp.p;
    const MineSlots& sl = rp.sl;
    const int kc = p.kc, pitch = kc + 4, half = kc >> 1;
    float* As = mine_smem;
    float* Bs = As + 64 * pitch;
    float* Ws = Bs + 64 * pitch;                         // [2][kc + 4]
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const MineSelect& pass = p.sel;
    const int i0 = blockIdx.z * pass.rel_span, i1 = min(i0 + pass.rel_span, sl.m);
    const bool resident = p.n_chunks == 1;
    const float bv = p.bias ? *p.bias : 0.f;
    const auto s_row = [=](int rl) { return m0 + rl; };
    const auto o_row = [=](int cl) { return n0 + cl; };
    const auto live_from = [&](int i) {                  // the first live slot at or after i, i1 when there is none (uniform)
        while (i < i1 && mine_slot_relation(sl, i, pass.num_rels) < 0) ++i;
        return i;
    };

    int i = live_from(i0);
    if (i >= i1) return;                                 // uniform: no live slot in this span
    int f_base, f_cnt;
    mine_filter_load(pass.tile_ptr, pass.tile_ent, blockIdx.y * gridDim.x + blockIdx.x, flist, t, &f_base, &f_cnt);
    if (t < 64) { fmask[0][t] = 0ull; fmask[1][t] = 0ull; fmask[2][t] = 0ull; }
    if (t < 3) fany[t] = 0;
    if (HIST) { hist_s[0][t] = 0u; hist_s[1][t] = 0u; }  // 256 threads, 256 bins
    if (resident) {
        mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, pass.n, 0, p.h, kc);
        mine_stage_rows(Bs, p.e, p.ld_e, p.vec_e, o_row, pass.n, 0, p.h, kc);
        if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, mine_slot_relation(sl, i, pass.num_rels), 4 * t));
    }
    __syncthreads();

    const int a_off = (wm + l31) * pitch + lhi * half, b_off = (wn + l31) * pitch + lhi * half, w_off = lhi * half;

    int before = -1;                                     // the slot whose histogram waits in hist_s[(it - 1) & 1]
    for (int it = 0; i < i1; ++it) {
        const int r = mine_slot_relation(sl, i, pass.num_rels), i_next = live_from(i + 1);
        const int fb = it % 3, wb = resident ? (it & 1) : 0;
        if (t < 64) fmask[(it + 1) % 3][t] = 0ull;
        if (t == 64) fany[(it + 1) % 3] = 0;
        mine_filter_relation(flist, pass.tile_ent, f_base, f_cnt, r, t, fmask[fb], &fany[fb]);
        float4 wnext = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool w_pre = resident && t < (kc >> 2) && i_next < i1;
        if (w_pre) wnext = mine_load_w(p, mine_slot_relation(sl, i_next, pass.num_rels), 4 * t);

        mine_f32x16 acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        for (int c = 0; c < p.n_chunks; ++c) {
            const int k0 = c * kc;
            if (!resident) {
                __syncthreads();
                mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, pass.n, k0, p.h, kc);
                mine_stage_rows(Bs, p.e, p.ld_e, p.vec_e, o_row, pass.n, k0, p.h, kc);
                if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, k0 + 4 * t));
                __syncthreads();
            }
            acc = mine_mfma_chunk(acc, As + a_off, Bs + b_off, Ws + wb * (kc + 4) + w_off, mine_groups(kc, p.h, k0));
        }
        if (w_pre) mine_store_w(Ws + ((it + 1) & 1) * (kc + 4), kc, t, wnext);
        __syncthreads();

        if (HIST && before >= 0)
            mine_hist_flush_clear(hist_s[(it + 1) & 1], pass.hist + ((size_t)before << pass.bin_bits), pass.bin_bits, t);
        const MineSelect sel = mine_slot_select<HIST>(pass, sl, i);
        mine_epilogue<HIST>(acc, bv, wm, wn, lane, pass.exclude_self && m0 == n0,
                            [&](int rl, int cl) { return make_int2(s_row(rl), o_row(cl)); }, r, fany[fb] != 0, fmask[fb],
                            hist_s[HIST ? (it & 1) : 0], sel);
        before = i;
        i = i_next;
        if (HIST && i >= i1) {                           // the last relation's histogram
            __syncthreads();
            mine_hist_flush_clear(hist_s[it & 1], pass.hist + ((size_t)before << pass.bin_bits), pass.bin_bits, t);
        }
    }
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

static int64_t mine_align16(int64_t b) { return (b + 15) / 16 * 16; }

int64_t mine_filter_workspace_bytes(int n, int n_filt_ent) {
    if (n <= 0 || n_filt_ent < 0) return 0;
    const int64_t tiles = (int64_t)((n + 63) / 64) * ((n + 63) / 64);
    return mine_align16(tiles * 4) + mine_align16((tiles + 1) * 4) + mine_align16((int64_t)(n_filt_ent > 0 ? n_filt_ent : 1) * 4);
}

// the three launches; *tile_ptr [tiles + 1] and *tile_ent then point into the workspace.  false: a launch could not be queued.
static bool mine_filter_rebucket(const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int n,
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

int mine_select_args(const MineCall& c, MineSelect* sel) {
    const char* who = c.who;
    const int n = c.n, num_rels = c.num_rels;
    GV_REQUIRE(n >= 0 && num_rels > 0 && c.n_filt_ent >= 0, GV_ERR_SHAPE, "%s: n=%d num_rels=%d n_filt_ent=%d", who, n, num_rels,
               c.n_filt_ent);
    GV_REQUIRE(c.mode == GV_MINE_EMIT || c.mode == GV_MINE_HIST, GV_ERR_SHAPE, "%s: unknown mode %d", who, c.mode);
    GV_REQUIRE((long long)n * num_rels < (1LL << 31), GV_ERR_SHAPE, "%s: n * num_rels = %lld reaches 2^31", who,
               (long long)n * num_rels);
    GV_REQUIRE(num_rels <= (1 << MINE_REL_BITS), GV_ERR_SHAPE, "%s: more than %d relations", who, 1 << MINE_REL_BITS);
    GV_REQUIRE((n + 63) / 64 <= 46340, GV_ERR_SHAPE, "%s: n=%d: more than 2^31 tile pairs", who, n);
    if (c.mode == GV_MINE_EMIT)
        GV_REQUIRE(c.capacity >= 0 && c.capacity <= INT_MAX, GV_ERR_SHAPE, "%s: capacity=%lld outside [0, 2^31)", who,
                   (long long)c.capacity);
    else
        GV_REQUIRE(c.bin_bits >= 1 && c.bin_bits <= MINE_HIST_BITS && c.prefix_bits >= 0 && c.prefix_bits + c.bin_bits <= 32 &&
                       (c.prefix >> c.prefix_bits) == 0u,
                   GV_ERR_SHAPE, "%s: prefix_bits=%d prefix=%u bin_bits=%d out of range", who, c.prefix_bits, c.prefix, c.bin_bits);
    GV_REQUIRE((c.filt_lo && c.filt_hi && c.filt_ent) || (!c.filt_lo && !c.filt_hi && !c.filt_ent), GV_ERR_NULL,
               "%s: filt_lo / filt_hi / filt_ent must be all given or all NULL", who);
    *sel = MineSelect{};
    sel->n = n; sel->num_rels = num_rels;
    sel->rel_span = num_rels;
    sel->exclude_self = c.exclude_self ? 1 : 0;
    sel->key_min = c.key_min; sel->prefix_bits = c.prefix_bits; sel->bin_bits = c.bin_bits; sel->prefix = c.prefix;
    sel->out = (int4*)c.out; sel->capacity = c.capacity;
    sel->counter = (unsigned long long*)c.counter; sel->hist = (unsigned long long*)c.hist;
    if (n == 0) return GV_OK;
    if (c.mode == GV_MINE_EMIT) {
        GV_REQUIRE(c.counter && (c.out || c.capacity == 0), GV_ERR_NULL, "%s: NULL output", who);
        GV_REQUIRE(aligned16(c.out), GV_ERR_SHAPE, "%s: out is not 16-byte aligned", who);        // int4 records
    } else {
        GV_REQUIRE(c.hist, GV_ERR_NULL, "%s: NULL histogram", who);
    }
    return GV_OK;
}

static int mine_fill_status(const MineCall& c) {
    char fill[64];
    snprintf(fill, sizeof fill, "%s(fill)", c.who);
    return launch_status(fill);
}

// the counters (EMIT) or the histograms (HIST) of `slots` selections cleared on the stream
static int mine_clear(const MineCall& c, int slots = 1) {
    const bool emit = c.mode == GV_MINE_EMIT;
    if (fill_words(emit ? (void*)c.counter : (void*)c.hist, 0u, (size_t)slots * (emit ? 8 : (size_t)8 << c.bin_bits), c.st) != hipSuccess)
        return mine_fill_status(c);
    return GV_OK;
}

// A whole-graph sweep over `count` relations (or slots) of an n-entity table, n > 0: the workspace checked, sel->rel_span and *grid
// set, the filter re-bucketed on the stream.
static int mine_sweep_prepare(const MineCall& c, int count, void* workspace, int64_t workspace_bytes, MineSelect* sel, dim3* grid) {
    const int n = c.n;
    const bool filtered = c.filt_lo != nullptr;
    if (filtered) {
        GV_REQUIRE(workspace, GV_ERR_NULL, "%s: a filter needs the workspace", c.who);
        GV_REQUIRE(aligned16(workspace), GV_ERR_WORKSPACE, "%s: the workspace is not 16-byte aligned", c.who);
        GV_REQUIRE(workspace_bytes >= mine_filter_workspace_bytes(n, c.n_filt_ent), GV_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes",
                   c.who, (long long)workspace_bytes, (long long)mine_filter_workspace_bytes(n, c.n_filt_ent));
    }
    const int tiles_1d = (n + 63) / 64;
    const int tiles = tiles_1d * tiles_1d;
    long long spans = (4LL * 256 + tiles - 1) / tiles;
    spans = std::max(1LL, std::min(spans, (long long)count));
    sel->rel_span = (int)((count + spans - 1) / spans);
    *grid = dim3(tiles_1d, tiles_1d, (count + sel->rel_span - 1) / sel->rel_span);

    if (filtered && !mine_filter_rebucket(c.filt_lo, c.filt_hi, c.filt_ent, c.n_filt_ent, n, c.num_rels, workspace, c.st, &sel->tile_ptr,
                                          &sel->tile_ent))
        return mine_fill_status(c);
    return GV_OK;
}

int mine_prepare(const MineCall& c, void* workspace, int64_t workspace_bytes, MineSelect* sel, dim3* grid) {
    int rc = mine_select_args(c, sel);
    if (rc != GV_OK || c.n == 0) return rc;
    rc = mine_sweep_prepare(c, c.num_rels, workspace, workspace_bytes, sel, grid);
    return rc != GV_OK ? rc : mine_clear(c);
}

int mine_slots_prepare(const MineCall& c, int m, void* workspace, int64_t workspace_bytes, MineSelect* sel, dim3* grid) {
    const int rc = mine_sweep_prepare(c, m, workspace, workspace_bytes, sel, grid);
    return rc != GV_OK ? rc : mine_clear(c, m);
}

int mine_slots_args(const MineCall& c, const int32_t* rels, int m, const uint32_t* key_min, const uint32_t* prefix,
                    const int64_t* out_base, int max_bin_bits, MineSlots* sl) {
    GV_REQUIRE(m >= 1 && m <= c.num_rels, GV_ERR_SHAPE, "%s: m=%d slots outside [1, num_rels=%d]", c.who, m, c.num_rels);
    if (c.mode == GV_MINE_HIST) {
        GV_REQUIRE(c.bin_bits <= max_bin_bits, GV_ERR_SHAPE, "%s: bin_bits=%d above %d", c.who, c.bin_bits, max_bin_bits);
        GV_REQUIRE(((long long)m << c.bin_bits) <= MINE_SLOT_HIST_WORDS, GV_ERR_SHAPE, "%s: m << bin_bits = %lld histogram words, more than %lld",
                   c.who, (long long)m << c.bin_bits, MINE_SLOT_HIST_WORDS);
    }
    *sl = MineSlots{};
    sl->rels = rels; sl->m = m; sl->key_min = key_min; sl->prefix = prefix; sl->out_base = (const long long*)out_base;
    if (c.n == 0) return GV_OK;
    GV_REQUIRE(rels, GV_ERR_NULL, "%s: NULL rels", c.who);
    if (c.mode == GV_MINE_EMIT)
        GV_REQUIRE(key_min && out_base, GV_ERR_NULL, "%s: NULL key_min / out_base", c.who);
    else
        GV_REQUIRE(prefix || c.prefix_bits == 0, GV_ERR_NULL, "%s: NULL prefix", c.who);
    return GV_OK;
}

int mine_typed_prepare(const MineCall& c, const int64_t* set_ptr, const int32_t* set_ids, const int32_t* units, int64_t n_units,
                       MineSelect* sel, MineTyped* ty, int slots) {
    const int rc = mine_select_args(c, sel);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(n_units >= 0 && n_units <= INT_MAX, GV_ERR_SHAPE, "%s: n_units=%lld outside [0, 2^31)", c.who, (long long)n_units);
    if (c.n == 0) return GV_OK;
    GV_REQUIRE(n_units == 0 || (set_ptr && set_ids && units), GV_ERR_NULL, "%s: NULL member lists or unit list", c.who);
    GV_REQUIRE(aligned16(units), GV_ERR_SHAPE, "%s: units is not 16-byte aligned", c.who);          // int4 records
    *ty = MineTyped{};
    ty->set_ptr = (const long long*)set_ptr; ty->set_ids = set_ids; ty->units = (const int4*)units;
    ty->filt_lo = c.filt_lo; ty->filt_hi = c.filt_hi; ty->filt_ent = c.filt_ent; ty->n_filt_ent = c.n_filt_ent;
    return mine_clear(c, slots);
}

// What both DistMult entries check of their tables; then *p filled but for the selection.
static int mine_params(const char* who, const float* e, int ld_e, const float* w, int ld_w, const float* bias, int n, int num_rels, int h,
                       int n_filt_ent, MineParams* p) {
    GV_REQUIRE(n >= 0 && num_rels > 0 && h > 0 && n_filt_ent >= 0, GV_ERR_SHAPE, "%s: n=%d num_rels=%d h=%d n_filt_ent=%d", who, n,
               num_rels, h, n_filt_ent);
    GV_REQUIRE(ld_e >= h && ld_w >= h, GV_ERR_SHAPE, "%s: leading dimension too small (ld_e=%d ld_w=%d h=%d)", who, ld_e, ld_w, h);
    GV_REQUIRE(n == 0 || (e && w), GV_ERR_NULL, "%s: NULL table", who);
    p->e = e; p->w = w; p->bias = bias;
    p->h = h; p->ld_e = ld_e; p->ld_w = ld_w;
    p->vec_e = aligned16(e) && (ld_e % 4 == 0);
    p->vec_w = aligned16(w) && (ld_w % 4 == 0);
    const int h16 = (h + 15) / 16 * 16;
    p->kc = h16 <= MINE_KC_MAX ? h16 : MINE_KC_MAX;
    p->n_chunks = (h + p->kc - 1) / p->kc;
    return GV_OK;
}

// ---- the type-constrained sweep (gv_mine_scores_typed) -----------------------------------------------------------------------------
// Loop order, transposed: a workgroup owns one unit = (relation r, one 64-row tile of r's subject members, a span of 64-row tiles
// of r's object members).  Rows of E are GATHERED through the member ids (mine_stage_rows) into the same LDS layout; the subject tile
// and w[r] are staged once per unit while the table fits one chunk, an object tile once per tile pair (no other relation could
// reuse it: its rows belong to r's list).  The arithmetic per pair is mine_mfma_chunk and mine_epilogue, the very code k_mine runs,
// so a surviving triplet's logit is the unconstrained miner's, bit for bit.
struct MineTypedParams {
    MineParams p;
    MineTyped ty;
};

template <bool HIST>
__global__ __launch_bounds__(256) void k_mine_typed(const MineTypedParams tp) {
    extern __shared__ __attribute__((aligned(16))) float mine_smem[];
    __shared__ unsigned long long fmask[64];             // the tile pair's listed objects per subject row
    __shared__ int sid_s[64], oid_s[64];                 // the tiles' entity ids, -1 past the lists
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const MineParams& p = tp.p;
    const MineTyped& ty = tp.ty;
    const MineSelect& sel = p.sel;
    const int kc = p.kc, pitch = kc + 4, half = kc >> 1;
    float* As = mine_smem;
    float* Bs = As + 64 * pitch;
    float* Ws = Bs + 64 * pitch;                         // [kc + 4]
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const auto s_row = [&](int rl) { return sid_s[rl]; };                 // table rows of the tiles' local rows: the member ids
    const auto o_row = [&](int cl) { return oid_s[cl]; };
    const int4 unit = ty.units[blockIdx.x];
    const int r = unit.x;
    if (r < 0 || r >= sel.num_rels) return;              // uniform: not a unit
    const bool resident = p.n_chunks == 1;
    const float bv = p.bias ? *p.bias : 0.f;

    mine_typed_ids(ty, sel.num_rels + r, unit.y, sel.n, t, sid_s);
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += 256) hist_s[i] = 0u;
    __syncthreads();
    if (resident) {
        mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, sel.n, 0, p.h, kc);
        if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, 4 * t));
    }
    const int a_off = (wm + l31) * pitch + lhi * half, b_off = (wn + l31) * pitch + lhi * half, w_off = lhi * half;

    for (int ot = unit.z; ot < unit.w; ++ot) {
        __syncthreads();                                 // the last tile's reads of Bs, oid_s and fmask are over
        mine_typed_ids(ty, r, ot, sel.n, t, oid_s);
        if (t < 64) fmask[t] = 0ull;
        __syncthreads();
        mine_typed_filter(ty, sel.num_rels, r, sid_s, oid_s, t, fmask);

        mine_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int c = 0; c < p.n_chunks; ++c) {
            const int k0 = c * kc;
            if (c > 0) __syncthreads();
            if (!resident) {
                mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, sel.n, k0, p.h, kc);
                if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, k0 + 4 * t));
            }
            mine_stage_rows(Bs, p.e, p.ld_e, p.vec_e, o_row, sel.n, k0, p.h, kc);
            __syncthreads();
            acc = mine_mfma_chunk(acc, As + a_off, Bs + b_off, Ws + w_off, mine_groups(kc, p.h, k0));
        }

        // ids through the member lists, -1 past them; fmask is complete (a barrier followed the filter's atomics) and always read
        const int o = oid_s[wn + l31];
        mine_epilogue<HIST>(acc, bv, wm, wn, lane, sel.exclude_self != 0, [&](int rl, int) { return make_int2(sid_s[rl], o); }, r, true,
                            fmask, hist_s, sel);
    }
    if (HIST) {
        __syncthreads();
        mine_hist_flush(hist_s, sel, t);
    }
}

// ---- the type-constrained sweep with selection state per relation (gv_mine_scores_typed_by_relation) --------------------------------
// k_mine_typed, a unit's first word being the SLOT whose relation it walks: the workgroup owns one relation already, so the
// selection is narrowed to the slot once (mine_slot_select) and the LDS histogram, its 12 + 10 + 10 levels and its one flush stay
// k_mine_typed's; only their destination is the slot's.
struct MineTypedRelParams {
    MineParams p;
    MineTyped ty;
    MineSlots sl;
};

template <bool HIST>
__global__ __launch_bounds__(256) void k_mine_typed_rel(const MineTypedRelParams tp) {
    extern __shared__ __attribute__((aligned(16))) float mine_smem[];
    __shared__ unsigned long long fmask[64];             // the tile pair's listed objects per subject row
    __shared__ int sid_s[64], oid_s[64];                 // the tiles' entity ids, -1 past the lists
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const MineParams& p = tp.p;
    const MineTyped& ty = tp.ty;
    const int kc = p.kc, pitch = kc + 4, half = kc >> 1;
    float* As = mine_smem;
    float* Bs = As + 64 * pitch;
    float* Ws = Bs + 64 * pitch;                         // [kc + 4]
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const auto s_row = [&](int rl) { return sid_s[rl]; };
    const auto o_row = [&](int cl) { return oid_s[cl]; };
    const int4 unit = ty.units[blockIdx.x];
    const int slot = (int)mine_uniform((unsigned)unit.x);
    const int r = mine_slot_relation(tp.sl, slot, p.sel.num_rels);
    if (r < 0) return;                                   // uniform: not a unit, or an empty slot
    const MineSelect sel = mine_slot_select<HIST>(p.sel, tp.sl, slot);
    const bool resident = p.n_chunks == 1;
    const float bv = p.bias ? *p.bias : 0.f;

    mine_typed_ids(ty, sel.num_rels + r, unit.y, sel.n, t, sid_s);
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += 256) hist_s[i] = 0u;
    __syncthreads();
    if (resident) {
        mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, sel.n, 0, p.h, kc);
        if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, 4 * t));
    }
    const int a_off = (wm + l31) * pitch + lhi * half, b_off = (wn + l31) * pitch + lhi * half, w_off = lhi * half;

    for (int ot = unit.z; ot < unit.w; ++ot) {
        __syncthreads();                                 // the last tile's reads of Bs, oid_s and fmask are over
        mine_typed_ids(ty, r, ot, sel.n, t, oid_s);
        if (t < 64) fmask[t] = 0ull;
        __syncthreads();
        mine_typed_filter(ty, sel.num_rels, r, sid_s, oid_s, t, fmask);

        mine_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int c = 0; c < p.n_chunks; ++c) {
            const int k0 = c * kc;
            if (c > 0) __syncthreads();
            if (!resident) {
                mine_stage_rows(As, p.e, p.ld_e, p.vec_e, s_row, sel.n, k0, p.h, kc);
                if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, k0 + 4 * t));
            }
            mine_stage_rows(Bs, p.e, p.ld_e, p.vec_e, o_row, sel.n, k0, p.h, kc);
            __syncthreads();
            acc = mine_mfma_chunk(acc, As + a_off, Bs + b_off, Ws + w_off, mine_groups(kc, p.h, k0));
        }

        const int o = oid_s[wn + l31];
        mine_epilogue<HIST>(acc, bv, wm, wn, lane, sel.exclude_self != 0, [&](int rl, int) { return make_int2(sid_s[rl], o); }, r, true,
                            fmask, hist_s, sel);
    }
    if (HIST) {
        __syncthreads();
        mine_hist_flush(hist_s, sel, t);
    }
}

// ---- the type-constrained sweep on the Monte-Carlo posterior predictive (gv_mine_scores_typed_mc) -----------------------------------
// k_mine_typed with S entity tables: sample s reads e + s * e_stride (shared ld_e), the one w, bias[s].  The value selected is
//   pbar = (sum over s ascending of mc_sig(logit_s + bias[s])) * (1.0f / S)
// with logit_s from mine_mfma_chunk unchanged, so pbar is gv_topk_scores_mc's out_prob for the query (s, r) at entity o, bit for bit.
// Loop order: the SAMPLE loop is outside the unit's object tiles.  A unit's span is walked in groups of MINE_MC_SPAN tiles; per
// (group, sample) the subject tile is staged once and per (object tile, sample) the object tile once -- the single-sample
// kernel's staging count per sample -- while one 16-register pbar accumulator per tile of the group stays live across the samples
// (one wave per SIMD: the register file is otherwise nearly empty).  On the resident path the next object tile of a sample is
// gathered into registers (mine_fetch_rows) before this tile's MFMA chain and written to LDS behind it.  The accumulators are indexed by a compile-time tile number (mine_each)
// only, a group's missing tiles are predicated off.  Filter, ids and mine_epilogue run per tile after the last sample; w[r] does
// not depend on the sample and stays staged per unit on the resident path.  The chunked path stages both tiles per (tile, sample,
// chunk): it works, it is not fast.
constexpr int MINE_MC_SPAN = 8;        // object tiles whose pbar a workgroup holds in registers at once (= ops.MINE_TYPED_SPAN)
constexpr int MINE_FETCH_MAX = (64 * (MINE_KC_MAX / 4) + 255) / 256;      // 16-byte pieces of a staged tile per thread, at most

// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>), in order: the tile loops of k_mine_typed_mc written out, so that
// the per-tile accumulators are indexed by constants whatever the loop unroller's size limit makes of a body this large (as a
// `#pragma unroll` loop the accumulators went to scratch once the register gather was added).
template <class F, int... J>
__device__ __forceinline__ void mine_each(F&& f, std::integer_sequence<int, J...>) {
    (f(std::integral_constant<int, J>{}), ...);
}

// mine_stage_rows in two halves -- a thread's pieces of a tile's rows into registers, and from there into the LDS layout -- so that
// the NEXT object tile's gather is in flight under the MFMA chain of this one (all loads issued together, no LDS touched).
template <class RowOf>
__device__ __forceinline__ void mine_fetch_rows(float4 (&v)[MINE_FETCH_MAX], const float* e, int ld, bool vec, RowOf row_of, int n, int h,
                                                int kc) {
    const int q4 = kc >> 2;
#pragma unroll
    for (int i = 0; i < MINE_FETCH_MAX; ++i) {
        const int idx = threadIdx.x + 256 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < 64 * q4) {
            const int rl = idx / q4, k = 4 * (idx - rl * q4);
            const int row = row_of(rl);
            if ((unsigned)row < (unsigned)n) {
                const float* src = e + (size_t)row * ld + k;
                if (vec && k + 3 < h) {
                    v[i] = *reinterpret_cast<const float4*>(src);
                } else {
                    v[i].x = k < h ? src[0] : 0.f;
                    v[i].y = k + 1 < h ? src[1] : 0.f;
                    v[i].z = k + 2 < h ? src[2] : 0.f;
                    v[i].w = k + 3 < h ? src[3] : 0.f;
                }
            }
        }
    }
}

__device__ __forceinline__ void mine_commit_rows(float* dst, const float4 (&v)[MINE_FETCH_MAX], int kc) {
    const int q4 = kc >> 2, pitch = kc + 4, half = kc >> 1;
#pragma unroll
    for (int i = 0; i < MINE_FETCH_MAX; ++i) {
        const int idx = threadIdx.x + 256 * i;
        if (idx < 64 * q4) {
            const int rl = idx / q4, q = idx - rl * q4;
            float* d = dst + rl * pitch + 2 * q;
            *reinterpret_cast<float2*>(d) = make_float2(v[i].x, v[i].z);
            *reinterpret_cast<float2*>(d + half) = make_float2(v[i].y, v[i].w);
        }
    }
}

struct MineTypedMcParams {
    MineParams p;                      // p.bias: one value per sample, or NULL
    MineTyped ty;
    long long e_stride;                // elements between consecutive samples' tables
    int n_samples;
    float inv_s;                       // 1.0f / n_samples
};

template <bool HIST>
__global__ __launch_bounds__(256) void k_mine_typed_mc(const MineTypedMcParams tp) {
    extern __shared__ __attribute__((aligned(16))) float mine_smem[];
    __shared__ unsigned long long fmask[64];             // the tile pair's listed objects per subject row
    __shared__ int sid_s[64], oid_s[MINE_MC_SPAN][64];   // the subject tile's and the group's object tiles' entity ids, -1 past the lists
    __shared__ unsigned hist_s[HIST ? (1 << MINE_HIST_BITS) : 1];
    const MineParams& p = tp.p;
    const MineTyped& ty = tp.ty;
    const MineSelect& sel = p.sel;
    const int kc = p.kc, pitch = kc + 4, half = kc >> 1;
    float* As = mine_smem;
    float* Bs = As + 64 * pitch;
    float* Ws = Bs + 64 * pitch;                         // [kc + 4]
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
    const int l31 = lane & 31, lhi = lane >> 5;
    const auto s_row = [&](int rl) { return sid_s[rl]; };
    const int4 unit = ty.units[blockIdx.x];
    const int r = unit.x;
    if (r < 0 || r >= sel.num_rels) return;              // uniform: not a unit
    const bool resident = p.n_chunks == 1;

    mine_typed_ids(ty, sel.num_rels + r, unit.y, sel.n, t, sid_s);
    if (HIST)
        for (int i = t; i < (1 << MINE_HIST_BITS); i += 256) hist_s[i] = 0u;
    if (resident && t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, 4 * t));
    const int a_off = (wm + l31) * pitch + lhi * half, b_off = (wn + l31) * pitch + lhi * half, w_off = lhi * half;

    for (int og = unit.z; og < unit.w; og += MINE_MC_SPAN) {
        __syncthreads();                                 // the last group's reads of oid_s are over (and sid_s is written)
        for (int j = wid; j < MINE_MC_SPAN; j += 4)      // a tile past the span's end: all -1
            mine_typed_ids(ty, r, og + j < unit.w ? og + j : -1, sel.n, lane, oid_s[j]);

        mine_f32x16 pbar[MINE_MC_SPAN];
#pragma unroll
        for (int j = 0; j < MINE_MC_SPAN; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) pbar[j][i] = 0.f;

        for (int s = 0; s < tp.n_samples; ++s) {
            const float* es = p.e + (long long)s * tp.e_stride;
            const float bv = p.bias ? p.bias[s] : 0.f;
            mine_each([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                if (og + j < unit.w) {                   // uniform
                    const auto o_row = [&](int cl) { return oid_s[j][cl]; };
                    mine_f32x16 acc;
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                    if (resident) {
                        // tile 0 of a sample is staged directly with the subject tile; every later tile was gathered into registers
                        // under the chain of the tile before it and committed behind that chain's barrier
                        if (j == 0) {
                            __syncthreads();             // the last chain's reads of As / Bs are over, oid_s is written
                            mine_stage_rows(As, es, p.ld_e, p.vec_e, s_row, sel.n, 0, p.h, kc);
                            mine_stage_rows(Bs, es, p.ld_e, p.vec_e, o_row, sel.n, 0, p.h, kc);
                        }
                        __syncthreads();
                        const bool more = j + 1 < MINE_MC_SPAN && og + j + 1 < unit.w;      // uniform
                        float4 next[MINE_FETCH_MAX];
                        if (more)
                            mine_fetch_rows(next, es, p.ld_e, p.vec_e, [&](int cl) { return oid_s[j + 1 < MINE_MC_SPAN ? j + 1 : j][cl]; },
                                            sel.n, p.h, kc);
                        acc = mine_mfma_chunk(acc, As + a_off, Bs + b_off, Ws + w_off, mine_groups(kc, p.h, 0));
                        if (more) {
                            __syncthreads();             // every wave's reads of Bs are over
                            mine_commit_rows(Bs, next, kc);
                        }
                    } else {
                        for (int c = 0; c < p.n_chunks; ++c) {
                            const int k0 = c * kc;
                            __syncthreads();             // the last chain's reads of As / Bs / Ws are over, oid_s is written
                            mine_stage_rows(As, es, p.ld_e, p.vec_e, s_row, sel.n, k0, p.h, kc);
                            if (t < (kc >> 2)) mine_store_w(Ws, kc, t, mine_load_w(p, r, k0 + 4 * t));
                            mine_stage_rows(Bs, es, p.ld_e, p.vec_e, o_row, sel.n, k0, p.h, kc);
                            __syncthreads();
                            acc = mine_mfma_chunk(acc, As + a_off, Bs + b_off, Ws + w_off, mine_groups(kc, p.h, k0));
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) pbar[j][i] += mc_sig(acc[i] + bv);
                }
            }, std::make_integer_sequence<int, MINE_MC_SPAN>{});
        }

        mine_each([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (og + j < unit.w) {                       // uniform
                __syncthreads();                         // the last tile's reads of fmask are over
                if (t < 64) fmask[t] = 0ull;
                __syncthreads();
                mine_typed_filter(ty, sel.num_rels, r, sid_s, oid_s[j], t, fmask);
                __syncthreads();                         // fmask is complete
#pragma unroll
                for (int i = 0; i < 16; ++i) pbar[j][i] *= tp.inv_s;
                // the key is pbar's (never -0: a sum of sigmoids), the record's fourth word its bits
                const int o = oid_s[j][wn + l31];
                mine_epilogue<HIST>(pbar[j], 0.f, wm, wn, lane, sel.exclude_self != 0, [&](int rl, int) { return make_int2(sid_s[rl], o); },
                                    r, true, fmask, hist_s, sel);
            }
        }, std::make_integer_sequence<int, MINE_MC_SPAN>{});
    }
    if (HIST) {
        __syncthreads();
        mine_hist_flush(hist_s, sel, t);
    }
}

}  // namespace gv

using namespace gv;

extern "C" int64_t gv_mine_scores_workspace_bytes(int n, int num_rels, int n_filt_ent) {
    (void)num_rels;
    return mine_filter_workspace_bytes(n, n_filt_ent);
}

extern "C" int gv_mine_scores(const float* e, int ld_e, const float* w, int ld_w, const float* bias, const int32_t* filt_lo,
                              const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int exclude_self, int mode,
                              uint32_t key_min, int prefix_bits, uint32_t prefix, int bin_bits, int32_t* out, int64_t capacity,
                              uint64_t* counter, uint64_t* hist, void* workspace, int64_t workspace_bytes, int n, int num_rels,
                              int h, void* stream) {
    const MineCall c{"gv_mine_scores", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, key_min, prefix_bits,
                     prefix, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    MineParams p{};
    dim3 grid;
    int rc = mine_params(c.who, e, ld_e, w, ld_w, bias, n, num_rels, h, n_filt_ent, &p);
    if (rc == GV_OK) rc = mine_prepare(c, workspace, workspace_bytes, &p.sel, &grid);
    if (rc != GV_OK || n == 0) return rc;
    const int lds = (2 * 64 * (p.kc + 4) + 2 * (p.kc + 4)) * (int)sizeof(float);
    const int lds_max = (2 * 64 * (MINE_KC_MAX + 4) + 2 * (MINE_KC_MAX + 4)) * (int)sizeof(float);
    return mode == GV_MINE_EMIT ? mine_launch<k_mine<false>>(p, grid, 256, lds, lds_max, c)
                                : mine_launch<k_mine<true>>(p, grid, 256, lds, lds_max, c);
}

extern "C" int gv_mine_scores_typed(const float* e, int ld_e, const float* w, int ld_w, const float* bias, const int64_t* set_ptr,
                                    const int32_t* set_ids, const int32_t* units, int64_t n_units, const int32_t* filt_lo,
                                    const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int exclude_self, int mode,
                                    uint32_t key_min, int prefix_bits, uint32_t prefix, int bin_bits, int32_t* out, int64_t capacity,
                                    uint64_t* counter, uint64_t* hist, int n, int num_rels, int h, void* stream) {
    const MineCall c{"gv_mine_scores_typed", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, key_min,
                     prefix_bits, prefix, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    MineTypedParams tp{};
    int rc = mine_params(c.who, e, ld_e, w, ld_w, bias, n, num_rels, h, n_filt_ent, &tp.p);
    if (rc == GV_OK) rc = mine_typed_prepare(c, set_ptr, set_ids, units, n_units, &tp.p.sel, &tp.ty);
    if (rc != GV_OK || n == 0 || n_units == 0) return rc;
    const int lds = (2 * 64 + 1) * (tp.p.kc + 4) * (int)sizeof(float);
    const int lds_max = (2 * 64 + 1) * (MINE_KC_MAX + 4) * (int)sizeof(float);
    const dim3 grid((unsigned)n_units);
    return mode == GV_MINE_EMIT ? mine_launch<k_mine_typed<false>>(tp, grid, 256, lds, lds_max, c)
                                : mine_launch<k_mine_typed<true>>(tp, grid, 256, lds, lds_max, c);
}

extern "C" int gv_mine_scores_by_relation(const float* e, int ld_e, const float* w, int ld_w, const float* bias, const int32_t* filt_lo,
                                          const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent, int exclude_self, int mode,
                                          const int32_t* rels, int m, const uint32_t* key_min, int prefix_bits, const uint32_t* prefix,
                                          int bin_bits, int32_t* out, int64_t capacity, const int64_t* out_base, uint64_t* counter,
                                          uint64_t* hist, void* workspace, int64_t workspace_bytes, int n, int num_rels, int h,
                                          void* stream) {
    const MineCall c{"gv_mine_scores_by_relation", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, 0u,
                     prefix_bits, 0u, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    MineRelParams rp{};
    dim3 grid;
    int rc = mine_params(c.who, e, ld_e, w, ld_w, bias, n, num_rels, h, n_filt_ent, &rp.p);
    if (rc == GV_OK) rc = mine_select_args(c, &rp.p.sel);
    if (rc == GV_OK) rc = mine_slots_args(c, rels, m, key_min, prefix, out_base, MINE_SLOT_HIST_BITS, &rp.sl);
    if (rc != GV_OK || n == 0) return rc;
    rc = mine_slots_prepare(c, m, workspace, workspace_bytes, &rp.p.sel, &grid);
    if (rc != GV_OK) return rc;
    const int lds = (2 * 64 * (rp.p.kc + 4) + 2 * (rp.p.kc + 4)) * (int)sizeof(float);
    const int lds_max = (2 * 64 * (MINE_KC_MAX + 4) + 2 * (MINE_KC_MAX + 4)) * (int)sizeof(float);
    return mode == GV_MINE_EMIT ? mine_launch<k_mine_rel<false>>(rp, grid, 256, lds, lds_max, c)
                                : mine_launch<k_mine_rel<true>>(rp, grid, 256, lds, lds_max, c);
}

extern "C" int gv_mine_scores_typed_by_relation(const float* e, int ld_e, const float* w, int ld_w, const float* bias,
                                                const int64_t* set_ptr, const int32_t* set_ids, const int32_t* units, int64_t n_units,
                                                const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent, int n_filt_ent,
                                                int exclude_self, int mode, const int32_t* rels, int m, const uint32_t* key_min,
                                                int prefix_bits, const uint32_t* prefix, int bin_bits, int32_t* out, int64_t capacity,
                                                const int64_t* out_base, uint64_t* counter, uint64_t* hist, int n, int num_rels, int h,
                                                void* stream) {
    const MineCall c{"gv_mine_scores_typed_by_relation", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, 0u,
                     prefix_bits, 0u, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    MineTypedRelParams tp{};
    MineSelect checked;
    int rc = mine_params(c.who, e, ld_e, w, ld_w, bias, n, num_rels, h, n_filt_ent, &tp.p);
    if (rc == GV_OK) rc = mine_select_args(c, &checked);
    if (rc == GV_OK) rc = mine_slots_args(c, rels, m, key_min, prefix, out_base, MINE_HIST_BITS, &tp.sl);
    if (rc == GV_OK) rc = mine_typed_prepare(c, set_ptr, set_ids, units, n_units, &tp.p.sel, &tp.ty, m);
    if (rc != GV_OK || n == 0 || n_units == 0) return rc;
    const int lds = (2 * 64 + 1) * (tp.p.kc + 4) * (int)sizeof(float);
    const int lds_max = (2 * 64 + 1) * (MINE_KC_MAX + 4) * (int)sizeof(float);
    const dim3 grid((unsigned)n_units);
    return mode == GV_MINE_EMIT ? mine_launch<k_mine_typed_rel<false>>(tp, grid, 256, lds, lds_max, c)
                                : mine_launch<k_mine_typed_rel<true>>(tp, grid, 256, lds, lds_max, c);
}

extern "C" int gv_mine_scores_typed_mc(const float* e, int ld_e, int64_t e_stride, int n_samples, const float* w, int ld_w,
                                       const float* bias, const int64_t* set_ptr, const int32_t* set_ids, const int32_t* units,
                                       int64_t n_units, const int32_t* filt_lo, const int32_t* filt_hi, const int32_t* filt_ent,
                                       int n_filt_ent, int exclude_self, int mode, uint32_t key_min, int prefix_bits, uint32_t prefix,
                                       int bin_bits, int32_t* out, int64_t capacity, uint64_t* counter, uint64_t* hist, int n,
                                       int num_rels, int h, void* stream) {
    const MineCall c{"gv_mine_scores_typed_mc", n, num_rels, filt_lo, filt_hi, filt_ent, n_filt_ent, exclude_self, mode, key_min,
                     prefix_bits, prefix, bin_bits, out, capacity, counter, hist, (hipStream_t)stream};
    MineTypedMcParams tp{};
    int rc = mine_params(c.who, e, ld_e, w, ld_w, bias, n, num_rels, h, n_filt_ent, &tp.p);
    if (rc != GV_OK) return rc;
    GV_REQUIRE(n_samples >= 1, GV_ERR_SHAPE, "%s: n_samples=%d", c.who, n_samples);
    GV_REQUIRE(n_samples == 1 || e_stride >= (int64_t)(n > 0 ? n - 1 : 0) * ld_e + h, GV_ERR_SHAPE,
               "%s: sample stride shorter than the rows it spans (e_stride=%lld)", c.who, (long long)e_stride);
    tp.e_stride = n_samples > 1 ? e_stride : 0;
    tp.n_samples = n_samples;
    tp.inv_s = 1.0f / (float)n_samples;
    tp.p.vec_e = tp.p.vec_e && tp.e_stride % 4 == 0;     // the 16-byte loads need every sample's base aligned
    rc = mine_typed_prepare(c, set_ptr, set_ids, units, n_units, &tp.p.sel, &tp.ty);
    if (rc != GV_OK || n == 0 || n_units == 0) return rc;
    const int lds = (2 * 64 + 1) * (tp.p.kc + 4) * (int)sizeof(float);
    const int lds_max = (2 * 64 + 1) * (MINE_KC_MAX + 4) * (int)sizeof(float);
    const dim3 grid((unsigned)n_units);
    return mode == GV_MINE_EMIT ? mine_launch<k_mine_typed_mc<false>>(tp, grid, 256, lds, lds_max, c)
                                : mine_launch<k_mine_typed_mc<true>>(tp, grid, 256, lds, lds_max, c);
}
