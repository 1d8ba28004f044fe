"""Type-constrained ranking and top-k on the GPU (gv_rank_scores_constrained, gv_transe_rank_constrained,
gv_topk_scores_constrained, gv_transe_topk_constrained and their drivers) against the plain-torch rules on the materialised
scores the kernels compare: ops.gemm(..., precision='f32') + bias for DistMult, -ops.transe_distances for TransE.  Every
assertion is an equality of integers or bit patterns.  pytest -m gpu."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
M = 70                       # two 64-row query tiles, the second partial
N_SETS = 6


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def _pack(member):
    """(n_sets, n) bool -> int32 words (n_sets, ceil(n / 32)), entity j = bit j & 31 of word j >> 5."""
    n_sets, n = member.shape
    w = (n + 31) // 32
    pad = torch.zeros(n_sets, w * 32, dtype=torch.long)
    pad[:, :n] = member.long()
    words = (pad.view(n_sets, w, 32) << torch.arange(32)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _eq4(got, want):
    assert len(got) == 4 and len(want) == 4
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == torch.float32 and torch.equal(g, w.to(g.device))


class Case:
    """m = 70 queries over n entities and 6 sets: 0 empty, 1 full, 2 a single member, 3..5 random.  Entity rows 1 and 2 are equal
    (an exact tie) with 1 inside and 2 outside sets 3 and 4; rows 5 and 6 are NaN with 5 inside and 6 outside them.  Query 0 and 1
    carry out-of-range set ids; targets include the tie pair, a NaN row and entities outside their query's set; every query has a
    sorted filter list that overlaps its set."""

    def __init__(self, n, width, seed):
        gen = torch.Generator().manual_seed(seed)
        self.n = n
        member = torch.rand(N_SETS, n, generator=gen) < 0.4
        member[0], member[1], member[2] = False, True, False
        member[2, n - 1] = True                                      # the last entity: the last used bit of the last word
        member[3:5, 1], member[3:5, 2], member[3:5, 5], member[3:5, 6] = True, False, True, False
        self.member = member
        self.words = _pack(member).to(DEV)
        table = torch.randn(n, width, generator=gen) * 0.5
        table[2] = table[1]
        table[5], table[6] = float('nan'), float('nan')
        self.table = table.to(DEV)
        self.q = torch.randn(M, width, generator=gen).to(DEV)
        sets = torch.randint(0, N_SETS, (M,), generator=gen)
        sets[0], sets[1] = N_SETS, -1                                # out of range: the empty set
        sets[2:8] = torch.tensor([0, 1, 2, 3, 4, 3])
        sets[66:70] = torch.tensor([3, 4, 2, 1])                     # the partial row tile too
        target = torch.randint(0, n, (M,), generator=gen)
        target[5], target[6], target[7], target[66], target[67] = 1, 2, 5, 2, 1
        target[4] = n - 1
        self.sets, self.target = sets.to(DEV), target.to(DEV)
        inside = member[sets.clamp(0, N_SETS - 1), target] & (sets >= 0) & (sets < N_SETS)
        assert bool(inside.any()) and bool((~inside[2:]).any())
        lists = []
        for i in range(M):
            e = torch.randint(0, n, (6,), generator=gen).tolist() + ([1, 5] if i % 3 == 0 else []) + ([n - 1] if i % 5 == 0 else [])
            lists.append(sorted(set(e)))
        lens = torch.tensor([len(e) for e in lists])
        self.hi = torch.cumsum(lens, 0).to(DEV)
        self.lo = self.hi - lens.to(DEV)
        self.ent = torch.tensor([x for e in lists for x in e]).to(DEV)
        self.cand = torch.zeros(M, n, dtype=torch.bool)
        ok = (sets >= 0) & (sets < N_SETS)
        self.cand[ok] = member[sets[ok]]
        self.cand = self.cand.to(DEV)
        from gcn_vae_amd import ranking
        self.listed = ranking._listed_mask(self.lo, self.hi, self.ent, M, n, DEV)
        assert bool((self.listed & self.cand).any())


_CASES = {}


def _case(n, width):
    if (n, width) not in _CASES:
        _CASES[(n, width)] = Case(n, width, seed=n + width)
    return _CASES[(n, width)]


# ---- 1, 2, 3: the four ranks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [203, 33, 64])
def test_distmult_ranks_equal_the_rule_and_the_filtered_ranker(ops, n):
    from gcn_vae_amd import ranking
    c = _case(n, 40)                                                 # h = 40: the last k-step is partial
    bias = torch.tensor(0.375, device=DEV)
    score = ops.gemm(c.q, c.table, trans_b=True, precision='f32') + bias
    want = ranking.rank_from_scores_constrained(score, c.target, c.cand, c.listed)
    got = ops.rank_scores_constrained(c.q, c.table, c.target, c.words, c.sets, c.lo, c.hi, c.ent, bias)
    _eq4(got, want)
    assert bool((got[2][:2] == 0).all()) and bool((got[3][:2] == 0).all())        # out-of-range set ids: the empty set
    assert bool((got[2][c.sets == 0] == 0).all())
    raw, filt = ops.rank_scores_filtered(c.q, c.table, c.target, c.lo, c.hi, c.ent, bias)
    assert torch.equal(got[0], raw) and torch.equal(got[1], filt)
    # without a filter: the filtered pair is not produced, the other two are unchanged
    nof = ops.rank_scores_constrained(c.q, c.table, c.target, c.words, c.sets, bias=bias)
    assert nof[1] is None and nof[3] is None and torch.equal(nof[0], got[0]) and torch.equal(nof[2], got[2])
    # an all-ones mask (padding bits set too): the constrained ranks are the unconstrained ones
    ones = torch.full_like(c.words, -1)
    full = ops.rank_scores_constrained(c.q, c.table, c.target, ones, c.sets.clamp(0, N_SETS - 1), c.lo, c.hi, c.ent, bias)
    assert torch.equal(full[0], raw) and torch.equal(full[1], filt) and torch.equal(full[2], raw) and torch.equal(full[3], filt)


@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('n', [203, 33, 64])
def test_transe_ranks_equal_the_rule_and_the_filtered_ranker(ops, n, p_norm):
    from gcn_vae_amd import ranking
    c = _case(n, 50)                                                 # dim = 50: the second LDS stage is partial
    score = -ops.transe_distances(c.q, c.table, p_norm)
    want = ranking.rank_from_scores_constrained(score, c.target, c.cand, c.listed)
    got = ops.transe_rank_constrained(c.q, c.table, c.target, p_norm, c.words, c.sets, c.lo, c.hi, c.ent)
    _eq4(got, want)
    assert bool((got[2][:2] == 0).all()) and bool((got[3][:2] == 0).all())
    raw, filt = ops.transe_rank_filtered(c.q, c.table, c.target, p_norm, c.lo, c.hi, c.ent)
    assert torch.equal(got[0], raw) and torch.equal(got[1], filt)
    nof = ops.transe_rank_constrained(c.q, c.table, c.target, p_norm, c.words, c.sets)
    assert nof[1] is None and nof[3] is None and torch.equal(nof[0], got[0]) and torch.equal(nof[2], got[2])
    ones = torch.full_like(c.words, -1)
    full = ops.transe_rank_constrained(c.q, c.table, c.target, p_norm, ones, c.sets.clamp(0, N_SETS - 1), c.lo, c.hi, c.ent)
    assert torch.equal(full[0], raw) and torch.equal(full[1], filt) and torch.equal(full[2], raw) and torch.equal(full[3], filt)


@pytest.mark.parametrize('p_norm,norm_flag', [(1, True), (2, True), (1, False), (2, False)])
def test_transe_driver_fused_equals_unfused(p_norm, norm_flag):
    from gcn_vae_amd import data, ranking, transe
    kg = data.load_data('synthetic:203:3:900:60:35:2')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device=DEV)
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, device=DEV)      # test left out: targets outside
    gen = torch.Generator().manual_seed(3)
    ent, rel = torch.randn(203, 50, generator=gen).to(DEV), torch.randn(3, 50, generator=gen).to(DEV)
    ent[9] = ent[4]
    trip = torch.as_tensor(np.asarray(kg.test), dtype=torch.long)
    got = transe.rank_transe_constrained(ent, rel, trip, p_norm, norm_flag, tc, fi)
    want = transe.rank_transe_constrained_unfused(ent, rel, trip, p_norm, norm_flag, tc, fi)
    _eq4(got, want)
    raw, filt = transe.rank_transe(ent, rel, trip, p_norm, norm_flag, fi)
    assert torch.equal(got[0], raw) and torch.equal(got[1], filt) and got[0].numel() == 2 * len(trip)


# ---- 3, 4: top-k --------------------------------------------------------------------------------------------------------------
def _topk_inputs(n, width, m, gen):
    """Sets for the top-k shape: 0 empty, 1 full, 2 a single member, 3 a handful (fewer than any k > 5), 4 about ninety (fewer than
    128) holding the tie group, 5 a random half.  Rows 3, 70 and n - 4 of the table are equal: for n = 1301 they sit in different
    column tiles and in both spans."""
    member = torch.rand(N_SETS, n, generator=gen) < 0.5
    member[0], member[1], member[2], member[3] = False, True, False, False
    member[2, n // 2] = True
    member[3, [0, min(n - 1, 65), n - 1, 3, n - 4]] = True
    member[4] = torch.rand(n, generator=gen) < min(1.0, 90.0 / n)
    ties = [3, min(n - 5, 70), n - 4]
    member[4, ties] = True
    member[5, ties[0]], member[5, ties[1]], member[5, ties[2]] = True, False, True
    table = torch.randn(n, width, generator=gen) * 0.5
    for j in ties[1:]:
        table[j] = table[ties[0]]
    table[7], table[n - 2] = float('nan'), float('nan')
    member[4, 7], member[4, n - 2] = True, False
    q = torch.randn(m, width, generator=gen)
    q[3] = table[3] * 4                                               # the tie group near the top of a row
    sets = torch.randint(0, N_SETS, (m,), generator=gen)
    sets[:8] = torch.tensor([N_SETS, 0, 1, 4, 2, 3, 5, 4])
    sets[m - 3:] = torch.tensor([4, 5, 3])
    lists = [sorted(set(torch.randint(0, n, (5,), generator=gen).tolist() + ([3, n - 1] if i % 4 == 0 else []))) for i in range(m)]
    lens = torch.tensor([len(e) for e in lists])
    hi = torch.cumsum(lens, 0)
    ent = torch.tensor([x for e in lists for x in e])
    cand = torch.zeros(m, n, dtype=torch.bool)
    ok = sets < N_SETS
    cand[ok] = member[sets[ok]]
    return [t.to(DEV) for t in (_pack(member), table, q, sets, hi - lens, hi, ent, cand)]


_TOPK = {}


def _topk_case(n, width):
    if (n, width) not in _TOPK:
        _TOPK[(n, width)] = _topk_inputs(n, width, M, torch.Generator().manual_seed(n * 3 + width))
    return _TOPK[(n, width)]


@pytest.mark.parametrize('k', [1, 10, 128])
@pytest.mark.parametrize('n', [1301, 203, 33, 64])
def test_distmult_topk_equals_the_rule(ops, n, k):
    from gcn_vae_amd import ranking
    words, table, q, sets, lo, hi, ent, cand = _topk_case(n, 40)
    bias = torch.tensor(-0.25, device=DEV)
    score = ops.gemm(q, table, trans_b=True, precision='f32') + bias
    got = ops.topk_scores_constrained(q, table, k, words, sets, bias, lo, hi, ent)
    assert got[0].dtype == torch.int64 and got[0].shape == (M, k)
    assert _same(got, ranking.topk_from_scores(score, k, lo, hi, ent, cand=cand))
    assert bool((got[0][:2] == -1).all()) and bool((got[1][:2] == float('-inf')).all())       # out of range / empty: all padding
    nof = ops.topk_scores_constrained(q, table, k, words, sets, bias)
    assert _same(nof, ranking.topk_from_scores(score, k, cand=cand))
    assert nof[0][4].tolist() == [n // 2] + [-1] * (k - 1)                                    # the single member, then padding
    if k == 128:
        assert int((got[0][5] >= 0).sum()) <= 5 and bool((got[0][3] == -1).any())             # sets with fewer than k members pad
        row = nof[0][3].tolist()
        at = row.index(3)
        assert row[at:at + 3] == [3, min(n - 5, 70), n - 4]                                    # the exact ties, by id
    ones = torch.full_like(words, -1)
    inside = sets.clamp(0, N_SETS - 1)
    assert _same(ops.topk_scores_constrained(q, table, k, ones, inside, bias, lo, hi, ent), ops.topk_scores(q, table, k, bias, lo, hi, ent))
    assert _same(ops.topk_scores_constrained(q, table, k, ones, inside), ops.topk_scores(q, table, k))


@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('k', [1, 10, 128])
@pytest.mark.parametrize('n', [1301, 203, 33, 64])
def test_transe_topk_equals_the_rule(ops, n, k, p_norm):
    from gcn_vae_amd import transe
    words, table, q, sets, lo, hi, ent, cand = _topk_case(n, 50)
    dist = ops.transe_distances(q, table, p_norm)
    got = ops.transe_topk_constrained(q, table, k, p_norm, words, sets, lo, hi, ent)
    assert _same(got, transe.topk_from_distances(dist, k, lo, hi, ent, cand))
    assert bool((got[0][:2] == -1).all()) and bool((got[1][:2] == float('inf')).all())
    nof = ops.transe_topk_constrained(q, table, k, p_norm, words, sets)
    assert _same(nof, transe.topk_from_distances(dist, k, cand=cand))
    if k == 128:
        row = nof[0][3].tolist()
        at = row.index(3)
        assert row[at:at + 3] == [3, min(n - 5, 70), n - 4]
    ones = torch.full_like(words, -1)
    inside = sets.clamp(0, N_SETS - 1)
    assert _same(ops.transe_topk_constrained(q, table, k, p_norm, ones, inside, lo, hi, ent),
                 ops.transe_topk(q, table, k, p_norm, lo, hi, ent))


# ---- 5: Hits@10 on the constrained filtered rank == membership in the constrained filtered top-10 ----------------------------
def test_hits_at_10_equals_membership_in_the_top_10():
    from gcn_vae_amd import data, ranking, transe
    kg = data.load_data('synthetic:400:5:3000:100:300:4')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, device=DEV)
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device=DEV)
    gen = torch.Generator().manual_seed(8)
    emb = (torch.randn(400, 24, generator=gen) * 0.4).to(DEV)        # continuous random rows: no ties at a target
    w = torch.randn(5, 24, generator=gen).to(DEV)
    trip = torch.as_tensor(np.asarray(kg.test), dtype=torch.long, device=DEV)
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    seen = 0
    for a, b, d in ((o, s, 's'), (s, o, 'o')):
        lo, hi = fi.lookup(a, r, d)
        listed = ranking._listed_mask(lo, hi, fi.entities(d, DEV), len(b), 400, DEV)
        keep = ~listed[torch.arange(len(b), device=DEV), b]          # the target is not in its own filter list
        assert bool(tc.contains(r, b, d).all())                      # and, the sets holding the test split, always a member
        ranks = ranking.perturb_and_get_rank_constrained(emb, w, a, r, b, len(b), fi, tc, d)
        ids, _ = ranking.predict_topk(emb, w, a, r, 10, direction=d, filter_index=fi, type_constraint=tc)
        assert torch.equal((ranks[3] + 1 <= 10)[keep], (ids == b.view(-1, 1)).any(1)[keep])
        assert _same((ids, _), ranking.predict_topk_unfused(emb, w, a, r, 10, direction=d, filter_index=fi, type_constraint=tc))
        rt = transe.rank_transe_constrained(emb, w, trip, 1, True, tc, fi)[3][(0 if d == 's' else len(b)):][:len(b)]
        idt, dt = transe.predict_topk((emb, w, 1, True), a, r, 10, direction=d, filter_index=fi, type_constraint=tc)
        assert torch.equal((rt + 1 <= 10)[keep], (idt == b.view(-1, 1)).any(1)[keep])
        assert _same((idt, dt), transe.predict_topk_unfused((emb, w, 1, True), a, r, 10, direction=d, filter_index=fi,
                                                             type_constraint=tc))
        seen += int(keep.sum())
        assert 0 < int(((ranks[3] + 1 <= 10) & keep).sum()) < int(keep.sum())
    assert seen > 300
    out = ranking.calc_constrained_mrr(emb, w, trip, fi, tc, verbose=False)
    ref = ranking.calc_filtered_mrr(emb, w, trip, fi, verbose=False)
    assert out['mrr_raw'] == ref['mrr_raw'] and out['mrr_filtered'] == ref['mrr_filtered']
    assert out['hits_raw'] == ref['hits_raw'] and out['hits_filtered'] == ref['hits_filtered']
    assert out['mrr_raw_constrained'] >= out['mrr_raw'] and out['mrr_filtered_constrained'] >= out['mrr_filtered']


# ---- 6: strides ---------------------------------------------------------------------------------------------------------------
def test_row_table_and_mask_strides(ops):
    c = _case(203, 40)
    gen = torch.Generator().manual_seed(12)
    wide_q = torch.randn(2 * M, 56, generator=gen).to(DEV)
    wide_e = torch.randn(203, 47, generator=gen).to(DEV)
    q, table = wide_q[::2, 3:43], wide_e[:, 5:45]                    # ld_q = 112, ld_e = 47, both pointers off 16-byte alignment
    wide_w = torch.randint(-2 ** 31, 2 ** 31 - 1, (N_SETS, 11), generator=gen).to(torch.int32).to(DEV)
    wide_w[:, 2:9] = c.words
    words = wide_w[:, 2:9]                                           # ld_cand = 11 > W = 7, junk around every row
    assert words.stride(0) == 11
    qc, tc_, wc = q.contiguous(), table.contiguous(), words.contiguous()
    _eq4(ops.rank_scores_constrained(q, table, c.target, words, c.sets, c.lo, c.hi, c.ent),
         ops.rank_scores_constrained(qc, tc_, c.target, wc, c.sets, c.lo, c.hi, c.ent))
    assert _same(ops.topk_scores_constrained(q, table, 17, words, c.sets, None, c.lo, c.hi, c.ent),
                 ops.topk_scores_constrained(qc, tc_, 17, wc, c.sets, None, c.lo, c.hi, c.ent))
    t50 = _case(203, 50)
    wide_w[:, 2:9] = t50.words
    _eq4(ops.transe_rank_constrained(t50.q, t50.table, t50.target, 1, words, t50.sets, t50.lo, t50.hi, t50.ent),
         ops.transe_rank_constrained(t50.q, t50.table, t50.target, 1, t50.words, t50.sets, t50.lo, t50.hi, t50.ent))
    assert _same(ops.transe_topk_constrained(t50.q, t50.table, 17, 2, words, t50.sets, t50.lo, t50.hi, t50.ent),
                 ops.transe_topk_constrained(t50.q, t50.table, 17, 2, t50.words, t50.sets, t50.lo, t50.hi, t50.ent))
    assert ops.topk_scores_constrained(q[:0], table, 5, words, c.sets[:0])[0].shape == (0, 5)
    with pytest.raises(ValueError):
        ops.rank_scores_constrained(qc, tc_, c.target, wc[:, :6], c.sets)          # fewer than ceil(v / 32) words
    with pytest.raises(ValueError):
        ops.rank_scores_constrained(qc, tc_, c.target, wc, c.sets[:-1])            # one set id per query


# ---- 7: the ABI's argument checks ----------------------------------------------------------------------------------------------
def test_c_entries_validate_the_candidate_arguments_before_any_launch():
    from gcn_vae_amd import lib
    l = lib.load()
    null, shape = -1, -2                                             # GV_ERR_NULL, GV_ERR_SHAPE
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)

    def rank_dm(cand, ld, n_sets, cs, filt=(None, None, None), cf=(p, p)):
        return l.gv_rank_scores_constrained(p, 8, p, 8, p, None, *filt, 0, cand, ld, n_sets, cs, p, p, cf[0], p, cf[1], 4, 70, 8, None)

    def topk_dm(cand, ld, n_sets, cs):
        return l.gv_topk_scores_constrained(p, 8, p, 8, None, None, None, None, 0, cand, ld, n_sets, cs, 5, p, p, p, 4, 70, 8, None)

    def rank_te(cand, ld, n_sets, cs, filt=(None, None, None), cf=(p, p)):
        return l.gv_transe_rank_constrained(p, 4, p, 70, 8, 1, p, *filt, cand, ld, n_sets, cs, p, cf[0], p, cf[1], None)

    def topk_te(cand, ld, n_sets, cs):
        return l.gv_transe_topk_constrained(p, 4, p, 70, 8, 1, None, None, None, 0, cand, ld, n_sets, cs, 5, p, p, p, None)

    for fn in (rank_dm, topk_dm, rank_te, topk_te):                  # v = 70: three words per set
        assert fn(None, 3, 6, p) == null and 'cand' in lib.last_error()
        assert fn(p, 3, 6, None) == null and 'cand' in lib.last_error()
        assert fn(p, 2, 6, p) == shape and 'ld_cand=2' in lib.last_error()
        assert fn(p, 3, 0, p) == shape and 'n_sets=0' in lib.last_error()
    for fn in (rank_dm, rank_te):
        assert fn(p, 3, 6, p, filt=(p, None, p)) == null             # the filter is all or none
        assert fn(p, 3, 6, p, filt=(p, p, p), cf=(p, None)) == null  # and needs both filtered counts
    assert l.gv_rank_scores_constrained(None, 8, None, 8, None, None, None, None, None, 0, p, 3, 6, p, None, None, None, None, None,
                                        0, 70, 8, None) == 0        # m == 0: nothing to do
    assert l.gv_transe_topk_constrained(None, 0, None, 70, 8, 1, None, None, None, 0, p, 3, 6, p, 5, None, None, None, None) == 0


# ---- 8: the CLIs -----------------------------------------------------------------------------------------------------------------
KINDS = ('raw', 'filtered', 'raw_constrained', 'filtered_constrained')


def _check_tsv(path, kg, k):
    from gcn_vae_amd import ranking
    rows = [line.rstrip('\n').split('\t') for line in open(path)]
    assert len(rows) == 2 * len(kg.test) * k
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    real = [(x[0], int(x[1]), int(x[2]), int(x[4])) for x in rows if int(x[4]) >= 0]
    assert real
    for d in ('o', 's'):
        part = [x for x in real if x[0] == d]
        assert part and bool(tc.contains(torch.tensor([x[2] for x in part]), torch.tensor([x[3] for x in part]), d).all())
    assert all(((a, r, e) if d == 'o' else (e, r, a)) not in known for d, a, r, e in real)


def test_cli_train_reports_four_ways_and_writes_members_only(tmp_path, capsys):
    from gcn_vae_amd import data, train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:300:7:2000:100:80:3'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt, out = str(tmp_path / 'm.pth'), str(tmp_path / 'pred.tsv')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                            '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file', ckpt,
                                            '--filtered-eval', '--type-constrain', '--predict-topk', '30', '--predict-out', out])
    train.main(args)
    text = capsys.readouterr().out
    for kind in KINDS:
        assert f'MRR ({kind}): ' in text and f'Hits ({kind}) @ 10: ' in text
    _check_tsv(out, kg, 30)


def test_cli_transe_reports_four_ways_and_writes_members_only(tmp_path):
    from gcn_vae_amd import data
    spec = 'synthetic:300:6:4000:200:200:1'
    env = dict(os.environ, PYTHONPATH=ROOT)
    ck, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'pred.tsv')
    cmd = [sys.executable, '-m', 'gcn_vae_amd.transe', '-d', spec, '--gpu', '0', '--seed', '0', '--dim', '32', '--nbatches', '10',
           '--neg-ent', '5', '--checkpoint', ck, '--filtered-eval']

    def run(extra):
        r = subprocess.run(['timeout', '-k', '10', '300'] + cmd + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout

    text = run(['--train-times', '1', '--type-constrain', '--predict-topk', '100', '--predict-out', out])
    for kind in KINDS:
        assert re.search(rf'MRR \({kind}\): \d\.\d+ \| MR \({kind}\): \d+\.\d+', text) and f'Hits ({kind}) @ 10: ' in text
    # the raw and filtered lines are those of a run without the flag
    plain = run(['--test-mode'])
    assert [x for x in text.splitlines() if '(raw)' in x or '(filtered)' in x] == \
           [x for x in plain.splitlines() if '(raw)' in x or '(filtered)' in x]
    assert 'constrained' not in plain
    _check_tsv(out, data.load_data(spec), 100)
