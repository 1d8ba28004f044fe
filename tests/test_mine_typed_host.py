"""Type-constrained whole-graph mining, the parts that need no GPU: TypeConstraint.members, the typed rule in plain torch
(cand_subj / cand_obj of mine_from_scores / mine_from_distances) against mine_cases.brute_force with the type-incorrect triplets
added to its excluded set, the unit plan, the CLIs' flag checks, and the wrappers' checks of the member lists (which run before
any launch).  Every comparison is exact."""
import argparse
import itertools

import pytest
import torch

from gcn_vae_amd import ops, ranking, train, transe
from mine_cases import brute_force, filter_arrays, same


def _triplets(n, num_rels, m, gen):
    return torch.stack([torch.randint(0, n, (m,), generator=gen), torch.randint(0, num_rels, (m,), generator=gen),
                        torch.randint(0, n, (m,), generator=gen)], 1)


@pytest.mark.parametrize('n', [1, 31, 32, 33, 65])
def test_members_are_the_sets_in_ascending_order(n):
    gen = torch.Generator().manual_seed(n)
    num_rels = 4                                          # relation 3 never occurs: both of its sets are empty
    trip = _triplets(n, 3, 2 * n, gen)
    tc = ranking.TypeConstraint(n, num_rels, trip)
    ptr, ids = tc.members()
    assert ptr.dtype == torch.int64 and ids.dtype == torch.int32 and ptr.shape == (2 * num_rels + 1,)
    assert int(ptr[0]) == 0 and int(ptr[-1]) == ids.numel()
    for r in range(num_rels):
        objects = sorted({int(o) for s, q, o in trip.tolist() if q == r})
        subjects = sorted({int(s) for s, q, o in trip.tolist() if q == r})
        assert ids[ptr[r]:ptr[r + 1]].tolist() == objects
        assert ids[ptr[num_rels + r]:ptr[num_rels + r + 1]].tolist() == subjects
    assert ptr[4] == ptr[3] and ptr[8] == ptr[7]
    assert torch.equal(ptr[1:] - ptr[:-1], tc.sizes)


def _typed_case(n, num_rels, seed):
    gen = torch.Generator().manual_seed(seed)
    val = torch.randn(num_rels, n, n, generator=gen)
    val[0, 1, 2], val[0, 2, 3], val[1, 0, 4] = float('nan'), float('inf'), float('-inf')
    val[1, 3, 1], val[1, 3, 2], val[0, 4, 0] = -0.0, 0.0, val[0, 3, 0]          # signed zeros and a tie
    cs = torch.rand(num_rels, n, generator=gen) < 0.6
    co = torch.rand(num_rels, n, generator=gen) < 0.6
    cs[0, [1, 2, 3, 4]] = True
    co[0, [0, 2, 3]] = True
    cs[1, [0, 3]] = True
    co[1, [1, 2, 4]] = True
    if num_rels > 2:
        cs[2] = False                                     # an empty side: relation 2 contributes nothing
    known = {(int(s), int(r), int(o)) for s, r, o in _triplets(n, num_rels, 3 * n, gen).tolist()}
    wrong = {(s, r, o) for s, r, o in itertools.product(range(n), range(num_rels), range(n)) if not (cs[r, s] and co[r, o])}
    return val, cs, co, known, wrong


@pytest.mark.parametrize('ascending', [False, True])
@pytest.mark.parametrize('exclude_self', [True, False])
@pytest.mark.parametrize('filtered', [False, True])
def test_the_typed_rule_against_brute_force(ascending, exclude_self, filtered):
    n, num_rels = 9, 3
    val, cs, co, known, wrong = _typed_case(n, num_rels, 5)
    rule = transe.mine_from_distances if ascending else ranking.mine_from_scores
    f = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filter_arrays(known, n, num_rels))) if filtered else {}
    excluded = wrong | (known if filtered else set())
    for sel in ({'k': 1}, {'k': 7}, {'k': 10 ** 6}, {'threshold': 0.0}, {'threshold': 0.3}, {'threshold': -0.3},
                {'threshold': float('inf')}, {'threshold': float('-inf')}):
        got = rule(val, exclude_self=exclude_self, cand_subj=cs, cand_obj=co, **sel, **f)
        want = brute_force(val, ascending, filt=excluded, exclude_self=exclude_self, **sel)
        assert same(got, want), sel
        assert not any(tuple(t) in excluded for t in got[0].tolist())


def test_one_sided_masks_and_unchanged_calls():
    n, num_rels = 9, 3
    val, cs, co, known, _ = _typed_case(n, num_rels, 6)
    full = torch.ones(num_rels, n, dtype=torch.bool)
    plain = ranking.mine_from_scores(val, k=20)
    assert same(ranking.mine_from_scores(val, k=20, cand_subj=full, cand_obj=full), (plain[0], plain[1], plain[2]['count']))
    only_s = {(s, r, o) for s, r, o in itertools.product(range(n), range(num_rels), range(n)) if not cs[r, s]}
    assert same(ranking.mine_from_scores(val, k=20, cand_subj=cs), brute_force(val, False, k=20, filt=only_s))
    with pytest.raises(ValueError):
        ranking.mine_from_scores(val, k=3, cand_subj=cs[:, :-1])
    with pytest.raises(ValueError):
        ranking.mine_from_scores(val, k=3, cand_obj=co.long())


@pytest.mark.parametrize('span', [1, 2, 3, 4, 8, None])
def test_the_plan_covers_every_member_pair_once(span):
    lens_o = [0, 1, 63, 64, 65, 130, 130, 5]
    lens_s = [7, 0, 130, 65, 64, 63, 1, 130]
    num_rels = len(lens_o)
    sizes = torch.tensor(lens_o + lens_s)
    ptr = torch.zeros(2 * num_rels + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(sizes, 0)
    for multiple in (1, 4):
        units = ops.mine_typed_plan(ptr, num_rels, span, multiple=multiple)
        assert units.dtype == torch.int32 and units.shape[1] == 4
        seen = {}
        for r, ts, t0, t1 in units.tolist():
            assert 0 <= r < num_rels and t0 < t1
            if span is None:
                assert (t1 - t0) <= ops.MINE_TYPED_SPAN
            for i in range(ts * 64, min(ts * 64 + 64, lens_s[r])):
                for to in range(t0, t1):
                    for j in range(to * 64, min(to * 64 + 64, lens_o[r])):
                        seen[(r, i, j)] = seen.get((r, i, j), 0) + 1
        want = {(r, i, j) for r in range(num_rels) for i in range(lens_s[r]) for j in range(lens_o[r])}
        assert set(seen) == want and set(seen.values()) <= {1}
    empty = ops.mine_typed_plan(torch.zeros(2 * num_rels + 1, dtype=torch.int64), num_rels)
    assert empty.shape == (0, 4)
    with pytest.raises(ValueError):
        ops.mine_typed_plan(ptr, num_rels, 0)


def test_a_plan_beyond_int32_units_is_an_argument_error():
    ptr = torch.tensor([0, 64 * 50000, 2 * 64 * 50000], dtype=torch.int64)          # 50 000 x 50 000 tile pairs, span 1
    with pytest.raises(ValueError, match='units'):
        ops.mine_typed_plan(ptr, 1, 1)


def test_check_args_of_both_clis():
    ok = transe.build_parser().parse_args(['-d', 'x', '--complete-topk', '5', '--complete-typed'])
    transe.check_args(ok)                                                             # no --filtered-eval needed
    transe.check_args(transe.build_parser().parse_args(['-d', 'x', '--complete-threshold', '2.5', '--complete-typed']))
    with pytest.raises(ValueError, match='--complete-typed'):
        transe.check_args(transe.build_parser().parse_args(['-d', 'x', '--complete-typed']))
    base = dict(test_mode=True, complete_topk=0, complete_threshold=None, complete_typed=True)
    with pytest.raises(ValueError, match='--complete-typed'):
        train.check_args(argparse.Namespace(**base))
    train.check_args(argparse.Namespace(**{**base, 'complete_topk': 5}))
    train.check_args(argparse.Namespace(**{**base, 'complete_threshold': 0.9}))
    train.check_args(argparse.Namespace(**{**base, 'complete_typed': False}))


@pytest.mark.parametrize('route', ['distmult', 'transe'])
def test_bad_member_lists_are_refused_before_any_launch(route):
    n, num_rels, h = 10, 2, 4
    emb, w = torch.randn(n, h), torch.randn(num_rels, h)                              # CPU tensors: a launch would be an error of its own

    def call(ptr, ids):
        ptr, ids = torch.tensor(ptr, dtype=torch.int64), torch.tensor(ids, dtype=torch.int32)
        if route == 'distmult':
            return ops.mine_scores_typed(emb, w, ptr, ids, k=3)
        return ops.transe_mine_typed(emb, w, 1, ptr, ids, k=3)

    good_ids = [0, 1, 2, 3, 4, 5]
    for ptr, ids in (([0, 2, 1, 4, 6], good_ids),             # decreasing
                     ([0, 2, 3, 4, 5], good_ids),             # does not end at ids.numel()
                     ([1, 2, 3, 4, 6], good_ids),             # does not start at 0
                     ([0, 2, 3, 4], good_ids[:4]),            # not 2 R + 1 entries
                     ([0, 2, 3, 4, 6], [0, 1, 2, 3, -1, 5]),  # an id < 0
                     ([0, 2, 3, 4, 6], [0, 1, 2, 3, 4, n]),   # an id >= n
                     ([0, 2, 3, 4, 6], [1, 0, 2, 3, 4, 5]),   # a set that is not ascending
                     ([0, 2, 3, 4, 6], [1, 1, 2, 3, 4, 5])):  # a repeated member
        with pytest.raises(ValueError):
            call(ptr, ids)
    with pytest.raises(RuntimeError):                          # good lists: the CPU tables are what is refused next
        call([0, 2, 3, 4, 6], good_ids)


def test_a_constraint_of_other_sizes_is_refused():
    tc = ranking.TypeConstraint(5, 2, torch.tensor([[0, 1, 2]]))
    with pytest.raises(ValueError, match='TypeConstraint'):
        ranking.mine_triplets(torch.randn(6, 4), torch.randn(2, 4), k=3, type_constraint=tc)
    with pytest.raises(ValueError, match='TypeConstraint'):
        ranking.mine_triplets_unfused(torch.randn(5, 4), torch.randn(3, 4), k=3, type_constraint=tc)


def test_the_c_entries_report_bad_arguments_before_any_launch():
    """Return codes, not launches (runs without a GPU): the checks gv_mine_scores makes, plus the unit count."""
    from gcn_vae_amd import lib
    l = lib.load()
    one = 1 << 4                                            # any non-NULL, 16-byte aligned address: nothing is dereferenced on the host

    def distmult(n=10, num_rels=2, h=4, e=one, units=one, n_units=1, mode=0, capacity=8, out=one, counter=one, bin_bits=1,
                 filt=(None, None, None)):
        return l.gv_mine_scores_typed(e, h, one, h, None, one, one, units, n_units, *filt, 0, 1, mode, 0, 0, 0, bin_bits, out, capacity,
                                      counter, one, n, num_rels, h, None)

    def te(n=10, num_rels=2, dim=4, p=1, en=one, units=one, n_units=1, mode=0, capacity=8, out=one):
        return l.gv_transe_mine_typed(en, one, n, num_rels, dim, p, one, one, units, n_units, None, None, None, 0, 1, mode, 0, 0, 0, 1,
                                      out, capacity, one, one, None)

    assert distmult(n=0) == 0 and te(n=0) == 0                                  # no entity: nothing to do
    for bad in (dict(n_units=2 ** 31), dict(n_units=-1), dict(mode=7), dict(capacity=-1), dict(capacity=2 ** 31), dict(e=None),
                dict(out=None), dict(out=one + 4), dict(units=None), dict(units=one + 4), dict(counter=None), dict(num_rels=0),
                dict(h=0), dict(n=-1), dict(mode=1, bin_bits=13), dict(filt=(one, None, None))):
        assert distmult(**bad) != 0, bad
        assert 'gv_mine_scores_typed' in lib.last_error()
    assert distmult(n_units=2 ** 31) != 0 and 'n_units' in lib.last_error()
    for bad in (dict(n_units=2 ** 31), dict(mode=7), dict(en=None), dict(out=one + 4), dict(units=one + 4), dict(dim=0),
                dict(dim=ops.TRANSE_MAX_DIM + 1), dict(p=3)):
        assert te(**bad) != 0, bad
        assert 'gv_transe_mine_typed' in lib.last_error()
