// Top-k selection shared by the four span kernels -- k_topk_span, k_entity_topk_span (k_gemm.hip: MFMA logits) and
// k_transe_topk_span, k_transe_entity_topk_span (k_transe.hip: L1 / L2 distances): the ordered 64-bit key, the per-row sorted list
// with its wave-wide insert, the cursor over a row's sorted filter list, the selection epilogue (set-up, the wave's row loop, the
// hand-on of the lists), the per-entity kernels' walk over (relation, column tile) pairs, the span geometry, the merge of the spans'
// lists with its two output decoders and the host's launch of the pair.  The kernels differ in how a 64 x 64 tile of values is
// made, not in how the best k of a row are kept.
// The two type-constrained per-entity kernels (k_entity_topk_typed_span, k_transe_entity_topk_typed_span) share all of it but the
// filter window, and their columns -- tiles of the relations' member lists -- are the TopkTyped pieces below.
// The two pair kernels (k_pair_rel, k_transe_pair_rel: the relations of an entity pair) take the key, the list update and the filter
// cursor, and share their own row loop and stores (topk_pair_rel_*): a workgroup there walks all of a row's few column tiles itself,
// so there are no spans, no hand-on and no merge.
//
// Candidates are ordered by a 64-bit key, larger = better:
//   key = ordered_u32(value) << 32 | ~id      ordered_u32: the sign-flip map, -0 -> +0, NaN -> 0 (after -inf)
// a strict total order (ties on the value by lower id); key 0 is "no candidate" and decodes to id -1, value -inf.
#pragma once
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace gv {

constexpr int TOPK_MAX = 128;

__device__ __forceinline__ unsigned long long topk_key(float x, int col) {
    unsigned u = __float_as_uint(x);
    if (x != x) u = 0u;
    else {
        if (u == 0x80000000u) u = 0u;
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | (unsigned)~col;
}

__device__ __forceinline__ float topk_key_logit(unsigned long long key) {
    const unsigned o = (unsigned)(key >> 32);
    if (key == 0ull) return -__builtin_huge_valf();
    if (o == 0u) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ int topk_key_id(unsigned long long key) { return (int)~(unsigned)key; }

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long x, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// insert `key` into the wave's sorted (descending) list: lane l holds positions l + 64 j in a[j]; the last position falls off
template <int NK>
__device__ __forceinline__ void topk_insert(unsigned long long (&a)[NK], unsigned long long key, int lane) {
    unsigned long long up[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) up[j] = __shfl(a[j], (lane + 63) & 63);     // lane l gets lane l - 1's (lane 0: lane 63's)
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const unsigned long long prev = lane ? up[j] : (j ? up[j - 1] : ~0ull);
        a[j] = a[j] > key ? a[j] : (prev > key ? key : prev);
    }
}

template <int NK>
__device__ __forceinline__ void topk_insert_mask(unsigned long long (&a)[NK], unsigned long long keyv, unsigned long long sv, int lane) {
    while (sv) {
        const int c = __builtin_ctzll(sv);
        sv &= sv - 1ull;
        topk_insert<NK>(a, readlane_u64(keyv, c), lane);
    }
}

__device__ __forceinline__ int lower_bound_i32(const int* a, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- the filter cursor of one query row (state in LDS, one entry per row of the workgroup's tile) ------------------------
// cur: the position in filt_ent of the first listed id not yet passed, fhi: the row's range end, nxt: the id at the cursor
// (INT_MAX: none left), so that a window without listed ids reads nothing from memory.
__device__ __forceinline__ void topk_filter_begin(const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_ent, bool live,
                                                  long long row, int first_col, int* cur, int* fhi, int* nxt) {
    int lo = 0, hi = 0;
    if (live) {
        lo = min(max(filt_lo[row], 0), n_ent);
        hi = min(max(filt_hi[row], lo), n_ent);
        lo = lower_bound_i32(filt_ent, lo, hi, first_col);
    }
    *cur = lo; *fhi = hi;
    *nxt = lo < hi ? filt_ent[lo] : INT_MAX;
}

// One wave, one lane per column of the window [n0, n0 + 64) of a row whose cursor says it lists ids inside the window: marks the
// listed columns in the wave's flag words (flw[j] == tag <=> column j of the row at hand is listed; tags are unique per row and
// window, so the flags are never cleared), advances the cursor past the window and returns whether this lane's column is listed.
__device__ __forceinline__ bool topk_filter_window(const int* filt_ent, int n0, int tag, int lane, int* cur, const int* fhi, int* nxt,
                                                   int* flw) {
    const int c0 = *cur, hi = *fhi;
    const int idx = c0 + lane;
    const int ent = idx < hi ? filt_ent[idx] : INT_MAX;
    const bool win = ent < n0 + 64;
    const int cnt = __popcll(__ballot(win));
    const unsigned bit = (unsigned)(ent - n0);
    if (win && bit < 64u) flw[bit] = tag;
    const bool listed = flw[lane] == tag;
    const int c1 = c0 + cnt;
    const int nx = cnt < 64 ? __shfl(ent, cnt) : (c1 < hi ? filt_ent[c1] : INT_MAX);
    if (lane == 0) { *cur = c1; *nxt = nx; }
    return listed;
}

// One wave: the lanes' keys that beat the row's k-th key (*thr) go into the row's sorted list lst[0, k) (LDS), *thr follows.
template <int NK>
__device__ __forceinline__ void topk_list_update(unsigned long long key, unsigned long long* lst, unsigned long long* thr, int k,
                                                 int lane) {
    const unsigned long long sv = __ballot(key > *thr);
    if (sv) {
        unsigned long long a[NK];
#pragma unroll
        for (int j = 0; j < NK; ++j) a[j] = lane + 64 * j < k ? lst[lane + 64 * j] : 0ull;
        topk_insert_mask<NK>(a, key, sv, lane);
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            if (lane + 64 * j < k) lst[lane + 64 * j] = a[j];
            if (lane + 64 * j == k - 1) *thr = a[j];
        }
    }
}

// ---- per-query candidate sets (the type-constrained top-k) -----------------------------------------------------------------
// Entity j is bit j & 31 of word j >> 5 of row cand_set[query] of `cand` ([n_sets, ld_cand]); a set id outside [0, n_sets) is the
// empty set.  A wave owns 16 consecutive query rows, so the two words a 64-column tile needs of each row are 32 words: lane l < 32
// keeps word (l >> 4) of row (l & 15) in a register -- loaded before the tile's arithmetic, read back by readlane when the row's
// turn comes -- and the span kernels' LDS stays as it is.  The second word is guarded by the used word count ceil(v / 32), not by
// ld_cand: an odd count has none for the last tile, and a row's padding words are never read.
struct TopkCand {
    const uint32_t* cand;
    const int* cand_set;
    int ld_cand, n_sets;
};

__device__ __forceinline__ const uint32_t* topk_cand_row(const TopkCand& cs, long long first_row, long long m, int lane) {
    const long long row = first_row + (lane & 15);
    const int set = (lane < 32 && row < m) ? cs.cand_set[row] : -1;
    return (unsigned)set < (unsigned)cs.n_sets ? cs.cand + (size_t)set * cs.ld_cand : nullptr;
}

__device__ __forceinline__ unsigned topk_cand_word(const uint32_t* row_words, int n0, int v, int lane) {
    const int w = (n0 >> 5) + ((lane >> 4) & 1);
    return (row_words && w < (v + 31) >> 5) ? row_words[w] : 0u;      // never past the set's last used word
}

// is column `lane` of the tile a member of the set of the wave's i-th row (i wave-uniform, 0..15)?
__device__ __forceinline__ bool topk_cand_member(unsigned word, int i, int lane) {
    const unsigned w0 = (unsigned)__builtin_amdgcn_readlane((int)word, i);
    const unsigned w1 = (unsigned)__builtin_amdgcn_readlane((int)word, 16 + i);
    return ((lane < 32 ? w0 : w1) >> (lane & 31)) & 1u;
}

// The rankers keep a row's two words for the 64-column tile at n0 in LDS instead (one thread per row): both at once, the second
// under the same guard.  n0 < v, so the first word lies inside ceil(v / 32) <= ld_cand.
__device__ __forceinline__ unsigned long long topk_cand_pair(const TopkCand& cs, long long row, long long m, int n0, int v) {
    const int set = row < m ? cs.cand_set[row] : -1;
    if ((unsigned)set >= (unsigned)cs.n_sets) return 0ull;
    const uint32_t* words = cs.cand + (size_t)set * cs.ld_cand;
    const int w0 = n0 >> 5;
    unsigned long long cw = words[w0];
    if (w0 + 1 < (v + 31) >> 5) cw |= (unsigned long long)words[w0 + 1] << 32;     // never past the set's last used word
    return cw;
}

// ---- stage 1's selection epilogue: what the four span kernels do around their own tile of values ---------------------------
// A span kernel is 256 threads on a ROWS-row query tile: it declares the LDS state itself (lists [ROWS][k], thr [ROWS], the
// cursor's cur / fhi / nxt [ROWS], fl [4][64]) and hands it to these pieces by pointer.  Wave w owns rows w * ROWS / 4 onwards.
// set-up, every thread: empty lists (key 0), no flag set, each row's k-th key 0 -- and row_setup(rl), what else thread rl < ROWS
// prepares for its row.  The tile's first barrier publishes it.  (k_transe_entity_topk_span keeps its own copy: see there.)
template <int ROWS, class RowSetup>
__device__ __forceinline__ void topk_span_clear(unsigned long long* lists, int k, int (*fl)[64], unsigned long long* thr, int lane,
                                                int wid, RowSetup&& row_setup) {
    for (int i = threadIdx.x; i < ROWS * k; i += 256) lists[i] = 0ull;
    fl[wid][lane] = 0;
    if (threadIdx.x < ROWS) {
        thr[threadIdx.x] = 0ull;
        row_setup((int)threadIdx.x);
    }
}

struct TopkEveryRow {
    __device__ __forceinline__ bool operator()(int) const { return true; }
};

// The wave's rows of the tile at hand, one lane per column: row_key(rl, i) is the lane's key of tile row rl (the wave's i-th) --
// the kernel's own value read, id, filter window and drop rule -- and what beats the row's k-th key goes into the row's list.  A
// row that row_live(rl) denies is passed over (a per-entity row without an entity); rows from m on (row0 + rl) end the loop.
template <int NK, int ROWS, class Idx, class RowKey, class RowLive = TopkEveryRow>
__device__ __forceinline__ void topk_span_select(Idx row0, Idx m, unsigned long long* lists, unsigned long long* thr, int k,
                                                 int lane, int wid, RowKey&& row_key, RowLive&& row_live = RowLive{}) {
    for (int i = 0; i < ROWS / 4; ++i) {
        const int rl = wid * (ROWS / 4) + i;
        if (row0 + rl >= m) break;
        if (!row_live(rl)) continue;
        topk_list_update<NK>(row_key(rl, i), lists + rl * k, &thr[rl], k, lane);
    }
}

// the hand-on: each wave copies its own rows' lists to part[row][span][k] (written by this wave only: no barrier)
template <int ROWS, class Idx>
__device__ __forceinline__ void topk_span_hand_on(Idx row0, Idx m, const unsigned long long* lists, int k, unsigned long long* part,
                                                  int n_spans, int lane, int wid) {
    for (int i = 0; i < ROWS / 4; ++i) {
        const int rl = wid * (ROWS / 4) + i;
        const Idx row = row0 + rl;
        if (row >= m) break;
        unsigned long long* dst = part + ((size_t)row * n_spans + blockIdx.y) * k;
        for (int j = lane; j < k; j += 64) dst[j] = lists[rl * k + j];
    }
}

// ---- the pair kernels' selection (k_pair_rel of k_gemm.hip, k_transe_pair_rel of k_transe.hip) -------------------------------------
// A workgroup there owns a 64-row tile and walks ALL of its few column tiles, so a row's rank counts and its list stay in LDS from
// the first tile to the stores and belong to one wave (wave w: rows 16 w .. 16 w + 15): no span, no hand-on, no merge, no atomics.
// The kernel declares the state and hands it over by pointer; what differs between the two -- which value is better, and the key's
// sign -- is a Rule: Rule::above(v, t) (v beats the target's t, or either is NaN) and Rule::key(v, col).  A tie is v == t in both.
struct TopkPairRel {
    unsigned long long* lists;    // [64][k]
    unsigned long long* thr;      // [64] each row's k-th key
    int* cur; int* fhi; int* nxt; // [64] the filter cursor
    int (*fl)[64];                // [4][64] the waves' flag words
    const int* tcol;              // [64] the rows' targets (-1: none)
    const float* tgt;             // [64] ... and their values
    int (*cnt)[64];               // [2][64] 2 #better + #equal: raw, filtered; CAND: [4][64], + the two among the allowed
    const unsigned long long* allow;      // CAND: [64] the rows' allowed columns of the tile at hand, bit j = column n0 + j
};

// ---- the pair kernels' candidate sets (the *_constrained entries): the type-correct relations of a pair -------------------------
// `cand` is ranking.TypeConstraint.relation_words: [2 n_ent, ld_cand] words, relation r = bit r & 31 of word r >> 5, row e the
// relations entity e was subject of, row n_ent + e those it was object of.  The set of pair (s, o) is the AND of rows s and
// n_ent + o -- no set id per row -- and a 64-relation tile needs two words of each: thread rl < 64 reads them once per tile into
// allow[rl], the wave that owns the row reads that back wave-uniform, and a lane's own bit is (mask >> lane) & 1.  The second word
// is guarded by the used word count ceil(v / 32) (n0 < v, so the first lies inside it); bits from column v on may be set: every
// use below is under col < v.
struct TopkPairCand {
    const uint32_t* cand;
    int ld_cand, n_ent;
};

__device__ __forceinline__ unsigned long long topk_pair_rel_allow(const TopkPairCand& pc, int s, int o, int n0, int v) {
    if (s < 0) return 0ull;                                              // no such row
    const uint32_t* a = pc.cand + (size_t)s * pc.ld_cand;
    const uint32_t* b = pc.cand + ((size_t)pc.n_ent + o) * pc.ld_cand;
    const int w0 = n0 >> 5;
    unsigned long long mask = a[w0] & b[w0];
    if (w0 + 1 < (v + 31) >> 5) mask |= (unsigned long long)(a[w0 + 1] & b[w0 + 1]) << 32;
    return mask;
}

// The wave's rows of the tile at n0 (the t-th), one lane per column: value(rl) is the lane's value of tile row rl.  One pass of the
// row's filter window serves the counts and the list alike; the target itself and the columns from v on vote nowhere, a listed
// column votes in the raw count only and is no candidate.  CAND: the row's allowed mask (st.allow) adds the two counts among the
// allowed columns -- the target is never counted, allowed or not -- and only an allowed column is a candidate of the list.
template <int NK, class Rule, bool CAND = false, class Value>
__device__ __forceinline__ void topk_pair_rel_tile(const TopkPairRel& st, int m0, int m, int n0, int v, int t, int k, bool ranked,
                                                   const int* filt_ids, int lane, int wid, Value&& value) {
    const int col = n0 + lane;
    for (int i = 0; i < 16; ++i) {
        const int rl = wid * 16 + i;
        if (m0 + rl >= m) break;
        const float x = value(rl);
        bool listed = false;
        if (filt_ids && st.nxt[rl] < n0 + 64)     // this row lists ids inside the tile: mark them, advance the cursor
            listed = topk_filter_window(filt_ids, n0, t * 64 + rl + 1, lane, &st.cur[rl], &st.fhi[rl], &st.nxt[rl], st.fl[wid]);
        unsigned long long am = ~0ull;
        if constexpr (CAND) am = st.allow[rl];
        if (ranked) {
            const float tg = st.tgt[rl];
            const bool other = col < v && col != st.tcol[rl];
            const unsigned long long ma = __ballot(other && Rule::above(x, tg)), me = __ballot(other && x == tg);
            const unsigned long long keep = __ballot(!listed);
            if (lane == 0) {
                st.cnt[0][rl] += 2 * __popcll(ma) + __popcll(me);
                st.cnt[1][rl] += 2 * __popcll(ma & keep) + __popcll(me & keep);
                if constexpr (CAND) {
                    st.cnt[2][rl] += 2 * __popcll(ma & am) + __popcll(me & am);
                    st.cnt[3][rl] += 2 * __popcll(ma & keep & am) + __popcll(me & keep & am);
                }
            }
        }
        if constexpr (NK > 0 && CAND)
            topk_list_update<NK>((col < v && !listed && ((am >> lane) & 1ull)) ? Rule::key(x, col) : 0ull, st.lists + rl * k, &st.thr[rl],
                                 k, lane);
        else if constexpr (NK > 0)
            topk_list_update<NK>((col < v && !listed) ? Rule::key(x, col) : 0ull, st.lists + rl * k, &st.thr[rl], k, lane);
    }
}

// Each wave hands out its own rows: what it reads it wrote itself (tgt: ahead of the last barrier).  count_raw / count_filt may be
// NULL; Decode is the key's value back (topk_key_logit, or te_key_dist for a key made of -distance).  CAND: the two counts among
// the allowed columns go out beside them (either may be NULL).
template <int NK, class Id, float (*Decode)(unsigned long long), bool CAND = false>
__device__ __forceinline__ void topk_pair_rel_store(const TopkPairRel& st, int m0, int m, int k, bool ranked, float* tgt, int* count_raw,
                                                    int* count_filt, Id* out_ids, float* out_values, int lane, int wid,
                                                    int* count_raw_c = nullptr, int* count_filt_c = nullptr) {
    for (int i = 0; i < 16; ++i) {
        const int rl = wid * 16 + i, row = m0 + rl;
        if (row >= m) break;
        if (ranked && lane == 0) {
            tgt[row] = st.tgt[rl];
            if (count_raw) count_raw[row] = st.cnt[0][rl];
            if (count_filt) count_filt[row] = st.cnt[1][rl];
            if constexpr (CAND) {
                if (count_raw_c) count_raw_c[row] = st.cnt[2][rl];
                if (count_filt_c) count_filt_c[row] = st.cnt[3][rl];
            }
        }
        if constexpr (NK > 0)
            for (int j = lane; j < k; j += 64) {
                const unsigned long long key = st.lists[rl * k + j];
                out_ids[(size_t)row * k + j] = (Id)topk_key_id(key);
                out_values[(size_t)row * k + j] = Decode(key);
            }
    }
}

// ---- the per-entity kernels' columns: the sequence of (relation, 64-column tile) pairs, r-major -------------------------------
// Tile t = r * col_tiles + ct, candidate id = r * N + x.  A span starts at tile t_begin.
struct TopkPairTile {
    int r, c0;      // the tile's relation and first column
    bool opens;     // the relation's (or the span's) first tile: the rows' filter cursors are re-opened
};

struct TopkPairWalk {
    int r, ct;      // the NEXT tile's relation and column tile
    __device__ __forceinline__ TopkPairWalk(int t_begin, int col_tiles) : r(t_begin / col_tiles), ct(t_begin - r * col_tiles) {}
    // the pair at hand; the walk moves on to the next one (`first`: t == t_begin)
    __device__ __forceinline__ TopkPairTile step(int col_tiles, bool first) {
        const TopkPairTile now{r, ct * 64, ct == 0 || first};
        if (++ct == col_tiles) { ct = 0; ++r; }
        return now;
    }
};

// set-up, thread rl < ROWS: the row's entity into ent_s (-1: no such row, or an id outside [0, n))
__device__ __forceinline__ void topk_pair_entity(const int* ents, int row0, int rl, int m, int n, int* ent_s) {
    const int a = row0 + rl < m ? ents[row0 + rl] : -1;
    ent_s[rl] = (unsigned)a < (unsigned)n ? a : -1;
}

// at a tile that `opens`, thread rl < ROWS: the row's cursor on the list of key a * R + r, from the tile's first column on.  The
// caller places this where no wave still reads the previous relation's cursors (each kernel says where that is).
__device__ __forceinline__ void topk_pair_reopen(const int* filt_lo, const int* filt_hi, const int* filt_ent, int n_ent, const int* ent_s,
                                                 int num_rels, const TopkPairTile& tile, int* cur, int* fhi, int* nxt) {
    const int rl = threadIdx.x, a = ent_s[rl];
    topk_filter_begin(filt_lo, filt_hi, filt_ent, n_ent, filt_lo != nullptr && a >= 0, (long long)a * num_rels + tile.r, tile.c0,
                      &cur[rl], &fhi[rl], &nxt[rl]);
}

// ---- the TYPED per-entity kernels' columns: (relation, 64-member tile of the relation's candidate list) pairs, r-major ---------
// (k_entity_topk_typed_span, k_transe_entity_topk_typed_span.)  The sets are ranking.TypeConstraint.members: set j's members ascending
// in set_ids[set_ptr[j] : set_ptr[j + 1]], 2 R sets.  Relation r's candidates are set cand_base + r, and a query entity has
// candidates under r only as a member of set R - cand_base + r (cand_base 0: objects wanted, the entity a subject; R: the other way
// round).  tile_ptr [R + 1] is the prefix of ceil(|candidates of r| / 64): tile t belongs to the relation r with tile_ptr[r] <= t <
// tile_ptr[r + 1].  A slot past the list's end, or an id outside [0, n), is -1: it gathers nothing and gets key 0.
struct TopkTyped {
    const long long* set_ptr;     // [2 R + 1]
    const int* set_ids;
    const int* tile_ptr;          // [R + 1], tile_ptr[R] = n_tiles
    int cand_base, n_tiles;
};

struct TopkTypedTile {
    int r, ct;                    // the tile's relation, its index in the relation's candidate list
    int t_end;                    // tile_ptr[r + 1]: the relation's tiles end here
    long long base, len;          // the candidate list: set_ids[base : base + len]
    __device__ __forceinline__ int live() const { return (int)min(64ll, len - 64ll * ct); }     // the tile's slots that hold a member
};

__device__ __forceinline__ void topk_typed_relation(const TopkTyped& ty, int r, TopkTypedTile* tile) {
    tile->r = r; tile->ct = 0;
    tile->t_end = ty.tile_ptr[r + 1];
    tile->base = ty.set_ptr[ty.cand_base + r];
    tile->len = ty.set_ptr[ty.cand_base + r + 1] - tile->base;
}

// tile t < n_tiles: its relation by bisection on tile_ptr (the last r with tile_ptr[r] <= t: relations without a tile are passed)
__device__ __forceinline__ TopkTypedTile topk_typed_seek(const TopkTyped& ty, int num_rels, int t) {
    int lo = 0, hi = num_rels;                           // the first r in (0, R] with tile_ptr[r] > t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ty.tile_ptr[mid + 1] > t) hi = mid;
        else lo = mid + 1;
    }
    TopkTypedTile tile;
    topk_typed_relation(ty, min(lo, num_rels - 1), &tile);
    tile.ct = t - ty.tile_ptr[tile.r];
    return tile;
}

// tile t's successor, tile t + 1 (< n_tiles)
__device__ __forceinline__ TopkTypedTile topk_typed_next(const TopkTyped& ty, int num_rels, const TopkTypedTile& now, int t) {
    TopkTypedTile nx = now;
    ++nx.ct;
    if (t + 1 >= now.t_end) {
        int r = now.r + 1;
        while (r < num_rels - 1 && ty.tile_ptr[r + 1] <= t + 1) ++r;
        topk_typed_relation(ty, r, &nx);
    }
    return nx;
}

// the tile's 64 member ids, one per thread tl < 64
__device__ __forceinline__ int topk_typed_id(const TopkTyped& ty, const TopkTypedTile& tile, int n, int tl) {
    const long long at = 64ll * tile.ct + tl;
    const int id = (tile.ct >= 0 && at < tile.len) ? ty.set_ids[tile.base + at] : -1;
    return (unsigned)id < (unsigned)n ? id : -1;
}

// is entity a (>= 0) a member of the QUERY-side set of relation r?  (bisection of that set's ascending list)
__device__ __forceinline__ bool topk_typed_member(const TopkTyped& ty, int num_rels, int r, int a) {
    const int set = num_rels - ty.cand_base + r;
    const long long lo = ty.set_ptr[set], hi = ty.set_ptr[set + 1];
    long long x = lo, y = hi;
    while (x < y) {
        const long long mid = x + ((y - x) >> 1);
        if (ty.set_ids[mid] < a) x = mid + 1;
        else y = mid;
    }
    return x < hi && ty.set_ids[x] == a;
}

// The filter of a gathered tile.  One wave, a row whose cursor says that its next listed id is <= the tile's last member id_max:
// every listed id up to id_max is taken off the cursor, 64 at a time -- however many of them lie between two members, and member
// or not -- and looked up among the tile's `cnt` ascending ids (LDS) by bisection; a hit marks its slot in the wave's flag words
// (flw[j] == tag <=> slot j is listed; tags are unique per row and tile, so the flags are never cleared).  Returns whether this
// lane's slot is listed.
__device__ __forceinline__ bool topk_typed_filter_window(const int* filt_ent, const int* ids, int cnt, int id_max, int tag, int lane,
                                                         int* cur, const int* fhi, int* nxt, int* flw) {
    int c = *cur;
    const int hi = *fhi;
    int nx;
    for (;;) {
        const int idx = c + lane;
        const int ent = idx < hi ? filt_ent[idx] : INT_MAX;
        const bool win = ent <= id_max;
        const int got = __popcll(__ballot(win));
        if (win) {
            int x = 0, y = cnt;                          // the first slot with id >= ent
            while (x < y) { const int mid = (x + y) >> 1; if (ids[mid] < ent) x = mid + 1; else y = mid; }
            if (x < cnt && ids[x] == ent) flw[x] = tag;
        }
        c += got;
        if (got < 64) { nx = __shfl(ent, got); break; }
    }
    const bool listed = flw[lane] == tag;
    if (lane == 0) { *cur = c; *nxt = nx; }
    return listed;
}

// ---- stage 2: one wave per row merges the n_spans sorted lists of k keys and hands the first k to `out` --------------------
// Out::put(i, key) decodes key into entry i of the (m, k) outputs.  Id: the outputs' integer type; Value: the key's value back
// (topk_key_logit, or te_key_dist of k_transe.hip for a key made of -distance).
template <class Id, float (*Value)(unsigned long long)>
struct TopkOut {                     // id / value
    Id* ids;
    float* values;
    __device__ __forceinline__ void put(size_t i, unsigned long long key) const {
        ids[i] = (Id)topk_key_id(key);
        values[i] = Value(key);
    }
};

template <class Id, float (*Value)(unsigned long long)>
struct TopkPairOut {                 // relation / entity / value: the candidate id r * n + x taken apart (key 0 -> -1 / -1)
    Id* rel;
    Id* ent;
    float* values;
    int n;
    __device__ __forceinline__ void put(size_t i, unsigned long long key) const {
        const int id = topk_key_id(key);
        rel[i] = id < 0 ? -1 : id / n;
        ent[i] = id < 0 ? -1 : id % n;
        values[i] = Value(key);
    }
};

template <int NK, class Out>
__global__ __launch_bounds__(256) void k_topk_merge(const unsigned long long* part, int m, int n_spans, int k, const Out out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const unsigned long long* src = part + (size_t)row * n_spans * k;
    unsigned long long a[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) a[j] = lane + 64 * j < k ? src[lane + 64 * j] : 0ull;     // span 0 is sorted already
    for (int s = 1; s < n_spans; ++s) {
        const unsigned long long t = readlane_u64(a[(k - 1) >> 6], (k - 1) & 63);
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            const unsigned long long key = lane + 64 * j < k ? src[(size_t)s * k + lane + 64 * j] : 0ull;
            topk_insert_mask<NK>(a, key, __ballot(key > t), lane);
        }
    }
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const int pos = lane + 64 * j;
        if (pos < k) out.put((size_t)row * k + pos, a[j]);
    }
}

// The launch pair of every top-k entry: the span kernel -- Span1 (NK = 1) up to k = 64, Span2 (NK = 2) beyond -- then k_topk_merge.
// ROWS: query rows per span tile (ROWS * k keys of dynamic LDS); RAISE1: the NK = 1 kernel's static LDS leaves less than ROWS * 64
// keys under the default limit, so it is raised for both.  One device mask per span kernel: the statics below belong to one
// instantiation of this template, i.e. to one kernel pair.
template <auto Span1, auto Span2, bool RAISE1, int ROWS, class Params, class Out>
int topk_span_merge(const char* name, dim3 grid, const Params& p, unsigned long long* part, int m, int n_spans, int k, const Out& out,
                    hipStream_t st) {
    constexpr int KEY = (int)sizeof(unsigned long long);
    const dim3 block(256), mgrid((unsigned)((m + 3) / 4));
    static unsigned long long raised1 = 0, raised2 = 0;
    if (k <= 64) {
        if (RAISE1 && !raise_dynamic_lds((const void*)Span1, ROWS * 64 * KEY, raised1, name)) return GV_ERR_SHAPE;
        hipLaunchKernelGGL(Span1, grid, block, ROWS * k * KEY, st, p);
        hipLaunchKernelGGL((k_topk_merge<1, Out>), mgrid, block, 0, st, part, m, n_spans, k, out);
    } else {
        if (!raise_dynamic_lds((const void*)Span2, ROWS * TOPK_MAX * KEY, raised2, name)) return GV_ERR_SHAPE;
        hipLaunchKernelGGL(Span2, grid, block, ROWS * k * KEY, st, p);
        hipLaunchKernelGGL((k_topk_merge<2, Out>), mgrid, block, 0, st, part, m, n_spans, k, out);
    }
    return launch_status(name);
}

// No column to walk (a typed query whose candidate lists are all empty): the m * k keys of one span of empty lists, then the merge
// alone, which decodes them to the outputs' padding.
template <class Out>
int topk_all_padding(const char* name, unsigned long long* part, int m, int k, const Out& out, hipStream_t st) {
    const hipError_t e = fill_words(part, 0u, (size_t)m * k * sizeof(unsigned long long), st);
    if (e != hipSuccess) {
        set_error("%s: %s", name, hipGetErrorString(e));
        return (int)e;
    }
    const dim3 block(256), mgrid((unsigned)((m + 3) / 4));
    if (k <= 64) hipLaunchKernelGGL((k_topk_merge<1, Out>), mgrid, block, 0, st, part, m, 1, k, out);
    else hipLaunchKernelGGL((k_topk_merge<2, Out>), mgrid, block, 0, st, part, m, 1, k, out);
    return launch_status(name);
}

// spans per query-row tile: about 4 workgroups per CU of the MI355X (256 CUs) at any m, each span at least 8 column tiles long so
// the running lists warm up.  A fixed CU count keeps the workspace size a function of (m, v, k) alone.
// topk_spans_of: the same rule on a sequence of `col_tiles` tiles, at most `max_spans` of them per row tile (what stage 2 walks).
inline void topk_spans_of(long long m, long long col_tiles, long long max_spans, int* span_tiles, int* n_spans) {
    const long long row_tiles = (m + 63) / 64;
    long long s = (4 * 256 + row_tiles - 1) / row_tiles;
    s = std::min(s, std::max(1LL, col_tiles / 8));
    s = std::max(1LL, std::min(s, max_spans));
    const long long per = (col_tiles + s - 1) / s;
    *span_tiles = (int)per;
    *n_spans = (int)((col_tiles + per - 1) / per);
}

inline void topk_spans(long long m, int v, int* span_tiles, int* n_spans) {
    topk_spans_of(m, ((long long)v + 63) / 64, 64, span_tiles, n_spans);
}

}  // namespace gv
