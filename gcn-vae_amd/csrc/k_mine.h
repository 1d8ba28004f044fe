// What the mining sweeps share (gv_mine_scores / gv_mine_scores_typed and its Monte-Carlo form gv_mine_scores_typed_mc in k_mine.hip,
// gv_transe_mine / gv_transe_mine_typed in k_transe_mine.hip): everything about SELECTING candidates.  A workgroup of a whole-graph sweep is 256 threads (or groups of 256)
// on one 64 x 64 (subject tile, object tile) pair of the table, walking the relations; a candidate is (local row rl, local column
// cl) of it under relation r, with a value the kernel computed its own way.
//
// Candidates: all (s, r, o) with s, o < n, less the listed triplets (filter), less s == o (exclude_self), less NaN values.  Each
// has the ordered key of gv_topk_scores (sign-flip map, -0 -> +0, NaN -> 0 = never a candidate), larger = better; a distance d keys
// as -d.  A lane hands its 16 keys to mine_select16 with where each candidate sits, (rl, cl), and who it is, (s, o); that
//   zeroes    the keys of candidates with an id outside [0, n) (outside the table; -1 past a list) or with s == o when excluded;
//   mine_gate drops the keys this pass does not look at.
//       EMIT  key >= key_min stays.
//       HIST  keys whose top prefix_bits equal `prefix` stay.
//   __ballot  a wave with no key left skips the rest: nearly every relation of nearly every tile in EMIT and refining HIST passes.
//   filter    a key whose bit cl of mask[rl] is set is dropped; then mine_put:
//       EMIT  one wave-aggregated integer atomicAdd reserves slots on a 64-bit counter, (s, r, o, value bits) go out as plain
//             16-byte vector stores while the slot is below the capacity; the counter keeps counting, so the host learns the true
//             total.  Arrival order is arbitrary: the caller sorts.
//       HIST  the key's next bin_bits index an LDS histogram that is flushed with integer atomics (mine_hist_flush); the host
//             walks 12 + 10 + 10 bits to the key of the K-th best candidate (at most three such passes).
// The filter: the (lo, hi, ent) ranges per key s * R + r are re-bucketed per tile pair first (mine_prepare), so a workgroup reads
// ITS listed triplets once into LDS (mine_filter_load) and a relation without one -- nearly all of them -- costs one LDS flag
// (mine_filter_relation).  No float atomics anywhere.
//
// The type-constrained sweeps walk the transposed order -- a workgroup owns relation r, one 64-row tile of r's SUBJECT member list
// and a span of 64-row tiles of r's OBJECT member list, rows gathered through the member ids.  What differs for selection is
// where a candidate's ids come from (the member lists, MineTyped) and the filter: gathered tiles do not fit the per-tile-pair
// buckets, so a workgroup reads the (lo, hi, ent) ranges of its 64 subjects directly (mine_typed_filter).
//
// The by-relation sweeps keep all of this and give every relation its own selection: a MineSelect narrowed to the relation's slot
// (MineSlots, mine_slot_select) is what mine_select16 then sees.
//
// Host side: an entry states its selection arguments once, as a MineCall; mine_prepare / mine_typed_prepare check them and queue
// what precedes the sweep, mine_launch raises the kernel's LDS limit and launches it.
#pragma once
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

// ---- what a pass selects, as every kernel's parameter struct embeds it ---------------------------------------------------------
struct MineSelect {
    int n, num_rels;
    int rel_span;                      // relations per blockIdx.z
    int exclude_self;
    unsigned key_min;                  // EMIT
    int prefix_bits, bin_bits;         // HIST
    unsigned prefix;
    const int* tile_ptr;               // [s_tiles * o_tiles + 1], NULL: no filter
    const unsigned* tile_ent;
    int4* out;
    long long capacity;
    unsigned long long* counter;
    unsigned long long* hist;
};

// ---- the member lists and the work units of the type-constrained miners ----------------------------------------------------------
struct MineTyped {
    const long long* set_ptr;          // [2 R + 1]: set r = the objects of r, set R + r = its subjects (ranking.TypeConstraint)
    const int* set_ids;                // each set's members, ascending
    const int4* units;                 // (r, subject tile, first object tile, end object tile), tiles of 64 members
    const int* filt_lo;                // the filter as given: key s * R + r -> filt_ent[lo:hi], ascending; NULL: none
    const int* filt_hi;
    const int* filt_ent;
    int n_filt_ent;
};

// ---- selection state PER RELATION (gv_mine_scores_by_relation, gv_mine_scores_typed_by_relation and their TransE twins
// gv_transe_mine_by_relation, gv_transe_mine_typed_by_relation in k_transe_mine.hip) ------------------------------------------------
// A slot i is one relation rels[i] with its own threshold, prefix, counter, histogram and output segment; the pass's MineSelect
// carries what the slots share (sizes, level, the filter, the bases of out / counter / hist).  An id outside [0, num_rels): the slot
// is empty this pass.
constexpr int MINE_SLOT_HIST_BITS = 8;         // bins of the whole-graph form's per-relation LDS histogram (flushed per relation)

struct MineSlots {
    const int* rels;                   // [m]
    int m;
    const unsigned* key_min;           // [m], EMIT
    const unsigned* prefix;            // [m], HIST (not read at prefix_bits 0)
    const long long* out_base;         // [m + 1], EMIT: slot i's records go to out[out_base[i] .. out_base[i + 1])
};

// ---- host side, compiled once (k_mine.hip) -----------------------------------------------------------------------------------
// bytes of the re-bucketed filter of an n-entity table with n_filt_ent listed objects (0 for an empty table)
int64_t mine_filter_workspace_bytes(int n, int n_filt_ent);

// the selection arguments every mining entry takes, as it was given them; `who` is the entry's name in every message
struct MineCall {
    const char* who;
    int n, num_rels;
    const int32_t* filt_lo;
    const int32_t* filt_hi;
    const int32_t* filt_ent;
    int n_filt_ent, exclude_self, mode;
    uint32_t key_min;
    int prefix_bits;
    uint32_t prefix;
    int bin_bits;
    int32_t* out;
    int64_t capacity;
    uint64_t* counter;
    uint64_t* hist;
    hipStream_t st;
};

// What all four entries check alike: sizes, mode, the capacity or the histogram level, the filter given whole or not at all and
// (n > 0) the outputs of the mode; *sel filled but for rel_span and the filter.
int mine_select_args(const MineCall& c, MineSelect* sel);

// What the two type-constrained entries do before their launch: mine_select_args, the checks of the member lists and the unit list,
// *ty filled, the counter (EMIT) or the histogram (HIST) -- of each of `slots` selections -- cleared on the stream.  GV_OK: launch
// n_units workgroups, unless n == 0 or n_units == 0.
int mine_typed_prepare(const MineCall& c, const int64_t* set_ptr, const int32_t* set_ids, const int32_t* units, int64_t n_units,
                       MineSelect* sel, MineTyped* ty, int slots = 1);

// What the two by-relation entries check of their slots (after mine_select_args on the shared arguments): 1 <= m <= num_rels, HIST
// levels of at most max_bin_bits bits whose m << bin_bits histogram words stay within MINE_SLOT_HIST_WORDS, and (n > 0) the
// per-slot arrays of the mode; *sl filled.  The arrays' contents are device memory: an id outside [0, num_rels) is an empty slot,
// a segment is clamped into out, a prefix that is no prefix matches nothing.
constexpr long long MINE_SLOT_HIST_WORDS = 1LL << 24;
int mine_slots_args(const MineCall& c, const int32_t* rels, int m, const uint32_t* key_min, const uint32_t* prefix,
                    const int64_t* out_base, int max_bin_bits, MineSlots* sl);

// What the two whole-graph entries do before their launch: mine_select_args, then
// *sel completed (rel_span: about four workgroups per CU of the MI355X when the table has few tiles; the result does not depend on
// it), the filter re-bucketed per tile pair into the workspace (count, scan, fill: three small kernels, integer atomics), the
// counter or the histogram cleared, *grid = (object tiles, subject tiles, relation spans).  GV_OK: launch, unless n == 0 (nothing
// was queued, nothing is to be done).
int mine_prepare(const MineCall& c, void* workspace, int64_t workspace_bytes, MineSelect* sel, dim3* grid);

// What the whole-graph by-relation entries (gv_mine_scores_by_relation, gv_transe_mine_by_relation) do before their launch, after
// mine_select_args and mine_slots_args, n > 0: mine_prepare's geometry over the m SLOTS (sel->rel_span slots per blockIdx.z), the
// filter re-bucketed, the m counters (EMIT) or the m << bin_bits histogram words (HIST) cleared.
int mine_slots_prepare(const MineCall& c, int m, void* workspace, int64_t workspace_bytes, MineSelect* sel, dim3* grid);

// one sweep's launch: the kernel's dynamic-LDS limit raised to lds_max once per device (one flag per kernel instantiation)
template <auto KERNEL, class Params>
static int mine_launch(const Params& p, dim3 grid, int threads, int lds, int lds_max, const MineCall& c) {
    static unsigned long long raised = 0;
    if (!raise_dynamic_lds((const void*)KERNEL, lds_max, raised, c.who)) return GV_ERR_SHAPE;
    hipLaunchKernelGGL(KERNEL, grid, dim3(threads), lds, c.st, p);
    return launch_status(c.who);
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

// ---- device side: gate, put, the epilogue, flush ------------------------------------------------------------------------------------------
// the key when this pass looks at it, else 0
template <bool HIST>
__device__ __forceinline__ unsigned mine_gate(unsigned key, const MineSelect& sel) {
    if (HIST) {
        if (sel.prefix_bits && (key >> (32 - sel.prefix_bits)) != sel.prefix) key = 0u;
    } else {
        if (key < sel.key_min) key = 0u;
    }
    return key;
}

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

// One gated key of candidate (s, r, o), called by every lane of a wave together (`ok` false: this lane has none to put): counted in
// hist_s or emitted with value_bits.
template <bool HIST>
__device__ __forceinline__ void mine_put(bool ok, unsigned key, int value_bits, int s, int r, int o, int lane, unsigned* hist_s,
                                         const MineSelect& sel) {
    if (HIST) {
        if (ok) atomicAdd(&hist_s[(key >> (32 - sel.prefix_bits - sel.bin_bits)) & ((1u << sel.bin_bits) - 1u)], 1u);
    } else {
        mine_emit(ok, lane, s, r, o, value_bits, sel.out, sel.capacity, sel.counter);
    }
}

// The epilogue of the sweeps (k_transe_mine writes the same rule out: see there), called by every lane of a wave together with its 16 candidates under relation r: key_of(i) is
// candidate i's key, where(i) the candidate as (rl, cl, s, o) -- its place in the tile pair and its entity ids -- and
// bits(i, key) its value as the record carries it.  No candidate: an id outside [0, n) (outside the table; -1 past a member list),
// s == o when `exclude` (exclude_self, and the tile pair can hold such a pair: off the diagonal of the whole-graph sweeps the 16
// comparisons are skipped), or `live` false (the wave's group has no relation / no tile this round).  `listed`: mask [64] may hold
// a bit (false: the relation has no listed triplet here, the mask is not read).
// Contract with the callables: key_of(i) is called exactly once per candidate, in the first loop, and bits(i, .) only after it
// (tm_epilogue takes its square root in key_of).  Constraint on the spelling: `live` is tested FIRST and a dead group is said
// through `live`, not through ids of -1 -- tested last it becomes control flow that costs the TransE kernels 28 VGPRs and
// scratch (profiles/mine_shared/resources.txt); recompile to assembly and compare with that table after any change here.
template <bool HIST, class KeyOf, class Where, class Bits>
__device__ __forceinline__ void mine_select16(bool live, bool exclude, KeyOf key_of, Where where, Bits bits, int r, bool listed,
                                              const unsigned long long* mask, int lane, unsigned* hist_s, const MineSelect& sel) {
    unsigned key[16];
    bool want = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        key[i] = key_of(i);
        const int4 c = where(i);
        if (!live || (unsigned)c.z >= (unsigned)sel.n || (unsigned)c.w >= (unsigned)sel.n || (exclude && c.z == c.w)) key[i] = 0u;
        key[i] = mine_gate<HIST>(key[i], sel);
        want = want || key[i] != 0u;
    }
    if (__ballot(want) == 0ull) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int4 c = where(i);
        bool ok = key[i] != 0u;
        if (listed && ok) ok = !((mask[c.x] >> c.y) & 1ull);
        mine_put<HIST>(ok, key[i], bits(i, key[i]), c.z, r, c.w, lane, hist_s, sel);
    }
}

// ---- device side: the type-constrained miners' tiles -----------------------------------------------------------------------------
// the member ids of 64-row tile `tile` of set `set` into ids_s [64] (-1 past the list's end or for an id outside the table, which
// then is no candidate and gathers nothing), by the threads with 0 <= tl < 64
__device__ __forceinline__ void mine_typed_ids(const MineTyped& ty, int set, int tile, int n, int tl, int* ids_s) {
    if (tl < 64) {
        const long long at = ty.set_ptr[set] + (long long)tile * 64 + tl;
        int id = -1;
        if (tile >= 0 && at < ty.set_ptr[set + 1]) id = ty.set_ids[at];
        ids_s[tl] = (unsigned)id < (unsigned)n ? id : -1;
    }
}

// The listed objects of relation r per subject row of a gathered tile pair -> mask [64] (zeroed before, behind a barrier), by 256
// threads tl, four per row.  The tile's object ids are ascending, so a row's listed objects inside their range are one window of its
// sorted list: found by bisection, walked, each entry looked up among the 64 ids in LDS.  A row without a list costs its two loads.
__device__ __forceinline__ void mine_typed_filter(const MineTyped& ty, int num_rels, int r, const int* sid_s, const int* oid_s, int tl,
                                                  unsigned long long* mask) {
    if (!ty.filt_lo) return;
    const int row = tl >> 2, s = sid_s[row];
    if (s < 0 || oid_s[0] < 0) return;
    const long long key = (long long)s * num_rels + r;
    const int lo = min(max(ty.filt_lo[key], 0), ty.n_filt_ent), hi = min(max(ty.filt_hi[key], lo), ty.n_filt_ent);
    if (lo == hi) return;
    int cnt = 64;                                        // the tile's live columns: a prefix
    if (oid_s[63] < 0) {
        int a = 0, b = 63;                               // oid_s[a] >= 0 > oid_s[b]
        while (b - a > 1) { const int m = (a + b) >> 1; if (oid_s[m] >= 0) a = m; else b = m; }
        cnt = b;
    }
    const int o_min = oid_s[0], o_max = oid_s[cnt - 1];
    int a = lo, b = hi;                                  // the first entry >= o_min
    while (a < b) { const int m = (a + b) >> 1; if (ty.filt_ent[m] < o_min) a = m + 1; else b = m; }
    for (int j = a + (tl & 3); j < hi; j += 4) {
        const int e = ty.filt_ent[j];
        if (e > o_max) break;
        int x = 0, y = cnt;                              // the first column with id >= e
        while (x < y) { const int m = (x + y) >> 1; if (oid_s[m] < e) x = m + 1; else y = m; }
        if (x < cnt && oid_s[x] == e) atomicOr(&mask[row], 1ull << x);
    }
}

// HIST: the workgroup's LDS histogram into the global one (after a barrier)
__device__ __forceinline__ void mine_hist_flush(const unsigned* hist_s, const MineSelect& sel, int t) {
    for (int i = t; i < (1 << sel.bin_bits); i += 256) {
        const unsigned c = hist_s[i];
        if (c) atomicAdd(sel.hist + i, (unsigned long long)c);
    }
}

// ---- device side: a slot's selection -----------------------------------------------------------------------------------------------
// The per-slot arrays are uniform over the workgroup: one lane's load, broadcast, so that the values live in SGPRs.
__device__ __forceinline__ unsigned mine_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ long long mine_uniform(long long v) {
    const unsigned lo = mine_uniform((unsigned)v), hi = mine_uniform((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// relation of slot i, or -1 for an empty slot (i outside [0, m) or an id outside [0, num_rels))
__device__ __forceinline__ int mine_slot_relation(const MineSlots& sl, int i, int num_rels) {
    if ((unsigned)i >= (unsigned)sl.m) return -1;
    const int r = (int)mine_uniform((unsigned)sl.rels[i]);
    return (unsigned)r < (unsigned)num_rels ? r : -1;
}

// The pass's selection narrowed to slot i, read once per relation: its prefix and histogram (HIST) or its threshold, counter and
// output segment (EMIT; the segment clamped into out [0, capacity), the counter keeps counting past it).  mine_select16 and what it
// calls then run unchanged on the result.
template <bool HIST>
__device__ __forceinline__ MineSelect mine_slot_select(const MineSelect& pass, const MineSlots& sl, int i) {
    MineSelect s = pass;
    if (HIST) {
        if (pass.prefix_bits) s.prefix = mine_uniform(sl.prefix[i]);
        s.hist = pass.hist + ((size_t)i << pass.bin_bits);
    } else {
        s.key_min = mine_uniform(sl.key_min[i]);
        const long long cap = pass.capacity;
        long long b0 = mine_uniform(sl.out_base[i]), b1 = mine_uniform(sl.out_base[i + 1]);
        b0 = b0 < 0 ? 0 : (b0 > cap ? cap : b0);
        b1 = b1 < b0 ? b0 : (b1 > cap ? cap : b1);
        s.out = pass.out + b0;
        s.capacity = b1 - b0;
        s.counter = pass.counter + i;
    }
    return s;
}

// HIST, per relation: a 1 << MINE_SLOT_HIST_BITS bin LDS histogram into the slot's global one and back to zero -- one LDS read per
// thread, an atomic and a store only where something was counted (after a barrier; the bins are next written after another).
__device__ __forceinline__ void mine_hist_flush_clear(unsigned* hist_s, unsigned long long* hist, int bin_bits, int t) {
    if (t < (1 << bin_bits)) {
        const unsigned c = hist_s[t];
        if (c) {
            atomicAdd(hist + t, (unsigned long long)c);
            hist_s[t] = 0u;
        }
    }
}

}  // namespace gv
