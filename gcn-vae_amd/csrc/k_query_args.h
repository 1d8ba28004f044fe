// The argument checks the entity-query entries share (host only): gv_rank_scores* / gv_topk_scores* / gv_entity_topk_scores{,_typed}
// / gv_pair_rel_scores (k_gemm.hip) and gv_transe_rank_* / gv_transe_topk* / gv_transe_entity_topk{,_typed} / gv_transe_pair_rel
// (k_transe.hip).  One function per group of arguments; each takes the entry's
// name, sets the library's error text and returns the code, GV_OK when the group is fine.  An entry lists its groups in the order
// in which it reports them -- tests/test_query_entries_host.py (the pair entries: tests/test_relation_host.py and
// tests/test_relation_typed_mc_host.py) pins every text and, with two faults at once, that order -- then returns for m == 0, then
// asks for its own pointers.
#pragma once
#include "common.h"
#include "k_topk.h"

#define GV_CHECK(call)                 \
    do {                               \
        const int rc_ = (call);        \
        if (rc_ != GV_OK) return rc_;  \
    } while (0)

namespace gv {

inline int query_sizes(const char* name, int m, int v, int h) {
    GV_REQUIRE(m >= 0 && v > 0 && h > 0, GV_ERR_SHAPE, "%s: m=%d v=%d h=%d", name, m, v, h);
    return GV_OK;
}

inline int query_sizes(const char* name, int m, int v, int h, int n_filt_ent) {
    GV_REQUIRE(m >= 0 && v > 0 && h > 0 && n_filt_ent >= 0, GV_ERR_SHAPE, "%s: m=%d v=%d h=%d n_filt_ent=%d", name, m, v, h, n_filt_ent);
    return GV_OK;
}

inline int query_k(const char* name, int k) {
    GV_REQUIRE(k >= 1 && k <= TOPK_MAX, GV_ERR_SHAPE, "%s: k=%d outside [1, %d]", name, k, TOPK_MAX);
    return GV_OK;
}

inline int query_leading(const char* name, int ld_a, int ld_b, int h) {
    GV_REQUIRE(ld_a >= h && ld_b >= h, GV_ERR_SHAPE, "%s: leading dimension too small", name);
    return GV_OK;
}

// the filter's three arrays come together or not at all (`names`: how the entry spells them)
inline int query_filter(const char* name, const void* lo, const void* hi, const void* ent, const char* names = "filt_lo / filt_hi / filt_ent") {
    GV_REQUIRE((lo && hi && ent) || (!lo && !hi && !ent), GV_ERR_NULL, "%s: %s must be all given or all NULL", name, names);
    return GV_OK;
}

// the candidate sets: their geometry, and -- reported after the filter -- their two arrays
inline int query_cand_shape(const char* name, int n_sets, int ld_cand, int v) {
    GV_REQUIRE(n_sets >= 1 && ld_cand >= (v + 31) / 32, GV_ERR_SHAPE, "%s: n_sets=%d ld_cand=%d (>= %d)", name, n_sets, ld_cand, (v + 31) / 32);
    return GV_OK;
}

inline int query_cand_given(const char* name, const void* cand, const void* cand_set) {
    GV_REQUIRE(cand && cand_set, GV_ERR_NULL, "%s: NULL cand / cand_set", name);
    return GV_OK;
}

inline int query_pointers(const char* name, bool all_given) {
    GV_REQUIRE(all_given, GV_ERR_NULL, "%s: NULL pointer", name);
    return GV_OK;
}

// what comes with a filter: somewhere to count what it leaves (`what`: count_filt, or both filtered counts)
inline int query_filter_needs(const char* name, const void* filt_lo, bool given, const char* what) {
    GV_REQUIRE(!filt_lo || given, GV_ERR_NULL, "%s: a filter needs %s", name, what);
    return GV_OK;
}

// ---- the pair queries (gv_pair_rel_scores, gv_transe_pair_rel and their _constrained / _mc forms): ranks, a top-k, or both ----------
// k = 0 is "no top-k" there, and a call has to ask for something
inline int pair_query_asks(const char* name, int k, const void* target) {
    GV_REQUIRE(k >= 0 && k <= TOPK_MAX, GV_ERR_SHAPE, "%s: k=%d outside [0, %d]", name, k, TOPK_MAX);
    GV_REQUIRE(k >= 1 || target, GV_ERR_SHAPE, "%s: neither ranks (target) nor a top-k (k >= 1) asked for", name);
    return GV_OK;
}

// after m == 0: the tables and the pairs, then what each request writes to, then what comes with a filter
inline int pair_query_given(const char* name, bool tables, const void* target, const void* tgt, int k, const void* out_ids,
                            const void* out_values, const void* filt_lo, const void* count_filt) {
    GV_CHECK(query_pointers(name, tables && (!target || tgt) && (k == 0 || (out_ids && out_values))));
    GV_REQUIRE(!filt_lo || !target || count_filt, GV_ERR_NULL, "%s: a filter needs count_filt", name);
    GV_REQUIRE(filt_lo || !count_filt, GV_ERR_NULL, "%s: count_filt needs a filter", name);
    return GV_OK;
}

// the *_constrained pair entries, after the filter group: the relation bitmask's geometry (row e and row n + e of every entity:
// n_sets >= 2 n; ld_cand spans the relations), then the array itself
inline int pair_query_cand(const char* name, const void* cand, int ld_cand, int n_sets, int n, int num_rels) {
    GV_REQUIRE(n_sets >= 2 * (long long)n && ld_cand >= (num_rels + 31) / 32, GV_ERR_SHAPE, "%s: n_sets=%d (>= 2 n = %lld) ld_cand=%d (>= %d)",
               name, n_sets, 2 * (long long)n, ld_cand, (num_rels + 31) / 32);
    GV_REQUIRE(cand, GV_ERR_NULL, "%s: NULL cand", name);
    return GV_OK;
}

// ... and after pair_query_given: count_filt_c comes exactly with a filter and targets
inline int pair_query_given_cand(const char* name, const void* target, const void* filt_lo, const void* count_filt_c) {
    GV_REQUIRE(!filt_lo || !target || count_filt_c, GV_ERR_NULL, "%s: a filter needs count_filt_c", name);
    GV_REQUIRE((filt_lo && target) || !count_filt_c, GV_ERR_NULL, "%s: count_filt_c needs a filter and targets", name);
    return GV_OK;
}

// ---- the per-entity queries (gv_entity_topk_scores, gv_transe_entity_topk) -------------------------------------------------------
// spans of the R * ceil(N / 64) (relation, 64-column tile) pairs: span_tiles of them each when the caller says so (> 0), else
// topk_spans' rule with up to 256 spans, so that a single query entity still fills the chip (its one row tile is all the
// parallelism there is besides)
inline void entity_query_spans(long long m, int n, int num_rels, int span_tiles, int* per, int* n_spans) {
    const long long tiles = (long long)num_rels * (((long long)n + 63) / 64);
    if (span_tiles > 0) {
        *per = (int)std::min<long long>(span_tiles, tiles);
        *n_spans = (int)((tiles + *per - 1) / *per);
    } else {
        topk_spans_of(m, tiles, 256, per, n_spans);
    }
}

// what gv_*_workspace_bytes answer: the spans' lists, 0 for sizes the entry refuses
inline int64_t entity_query_workspace_bytes(int m, int n, int num_rels, int k, int span_tiles) {
    if (m <= 0 || n <= 0 || num_rels <= 0 || (long long)n * num_rels > INT_MAX || k < 1 || k > TOPK_MAX || span_tiles < 0) return 0;
    int per = 0, n_spans = 0;
    entity_query_spans(m, n, num_rels, span_tiles, &per, &n_spans);
    return (int64_t)m * n_spans * k * (int64_t)sizeof(unsigned long long);
}

// what follows an entry's own sizes: a candidate (r, x) is the id r * n + x of a key; k; the caller's span
inline int entity_query_shape(const char* name, int n, int num_rels, int k, int span_tiles) {
    GV_REQUIRE((long long)n * num_rels <= INT_MAX, GV_ERR_SHAPE, "%s: n * num_rels = %lld does not fit 31 bits", name,
               (long long)n * num_rels);
    GV_CHECK(query_k(name, k));
    GV_REQUIRE(span_tiles >= 0, GV_ERR_SHAPE, "%s: span_tiles=%d (0: the library's rule)", name, span_tiles);
    return GV_OK;
}

// the spans are a grid dimension; the workspace holds every span's lists
inline int entity_query_workspace(const char* name, int m, int k, int span_tiles, int n_spans, int64_t workspace_bytes) {
    GV_REQUIRE(n_spans <= 65535, GV_ERR_SHAPE, "%s: span_tiles=%d gives %d spans (at most 65535)", name, span_tiles, n_spans);
    const int64_t need = (int64_t)m * n_spans * k * (int64_t)sizeof(unsigned long long);
    GV_REQUIRE(workspace_bytes >= need, GV_ERR_SHAPE, "%s: workspace of %lld bytes, %lld needed", name, (long long)workspace_bytes,
               (long long)need);
    return GV_OK;
}

// ---- the type-constrained per-entity queries (gv_entity_topk_scores_typed, gv_transe_entity_topk_typed) ---------------------------
// spans of the n_tiles (relation, 64-member tile) pairs of the candidate lists, by entity_query_spans' rule; no tile at all is one
// span of padding (nothing is walked: the merge decodes empty lists)
inline void entity_typed_spans(long long m, int n_tiles, int span_tiles, int* per, int* n_spans) {
    if (n_tiles <= 0) {
        *per = 1; *n_spans = 1;
    } else if (span_tiles > 0) {
        *per = std::min(span_tiles, n_tiles);
        *n_spans = (n_tiles + *per - 1) / *per;
    } else {
        topk_spans_of(m, n_tiles, 256, per, n_spans);
    }
}

// what gv_*_typed_workspace_bytes answer: the spans' lists, m * n_spans * k keys, 0 for sizes the entry refuses
inline int64_t entity_typed_workspace_bytes(int m, int n_tiles, int k, int span_tiles) {
    if (m <= 0 || n_tiles < 0 || k < 1 || k > TOPK_MAX || span_tiles < 0) return 0;
    int per = 0, n_spans = 0;
    entity_typed_spans(m, n_tiles, span_tiles, &per, &n_spans);
    return (int64_t)m * n_spans * k * (int64_t)sizeof(unsigned long long);
}

// what follows entity_query_shape: the tile count and which side holds the candidates
inline int entity_typed_shape(const char* name, int num_rels, int n_tiles, int cand_base) {
    GV_REQUIRE(n_tiles >= 0, GV_ERR_SHAPE, "%s: n_tiles=%d", name, n_tiles);
    GV_REQUIRE(cand_base == 0 || cand_base == num_rels, GV_ERR_SHAPE, "%s: cand_base=%d (0: the objects of r are the candidates, %d: its subjects)",
               name, cand_base, num_rels);
    return GV_OK;
}

// the member lists and the tile prefix (set_ids may be NULL when no set has a member: then there is no tile either)
inline int entity_typed_given(const char* name, const void* set_ptr, const void* set_ids, const void* tile_ptr, int n_tiles) {
    GV_REQUIRE(set_ptr && tile_ptr && (set_ids || n_tiles == 0), GV_ERR_NULL, "%s: NULL set_ptr / set_ids / tile_ptr", name);
    return GV_OK;
}

}  // namespace gv
