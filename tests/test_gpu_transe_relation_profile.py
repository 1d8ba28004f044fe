"""Per-relation completion for the TransE baseline on the GPU (gv_transe_mine_by_relation / gv_transe_mine_typed_by_relation,
ops.transe_relation_topk[_typed], transe.complete_relations, the CLI) against the rule stated on distances materialised on the
device by the expression that defines them (ops.transe_queries + ops.transe_distances per relation), selected by
transe.complete_relations_from_distances.  Every comparison is exact: ids equal, distances equal as bit patterns, per-relation
counts equal.  The relations live at scales 2^-6 .. 2^6 with the tables passed un-normalised, so every slot has its own threshold,
prefix and early-exit bound; a tight ``max_results`` makes the slots resolve at different histogram levels.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from mine_cases import _lists
from mine_typed_cases import member_lists, member_masks
from relation_profile_cases import same_rows
from transe_relation_profile_cases import first_level_bins, scaled_tables

pytestmark = pytest.mark.gpu

SHAPES = [(50, 8, 3),          # one partial tile, fewer slots than groups
          (64, 64, 1),         # a single slot
          (130, 200, 7),       # 3 x 3 tile pairs, resident tiles, two full TM_CHECK blocks: the early exit runs
          (65, 301, 5),        # two column chunks, the last partial
          (65, 512, 2),        # three chunks
          (1300, 8, 13)]       # 441 tile pairs: rel_span 5 -- a group walks two rounds and flushes two slots' histograms, idle groups in the last


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def _materialise(ops, en, rn, p):
    """dist[r, s, o], by the expression that defines the distance (the tables are used as they are: norm_flag off)."""
    n = en.shape[0]
    subjects = torch.arange(n, device=en.device)
    table = ops.transe_queries(en, norm_flag=False)
    return torch.stack([ops.transe_distances(ops.transe_queries(en, rn, subjects, torch.full_like(subjects, r), head=False, norm_flag=False),
                                             table, p) for r in range(rn.shape[0])])


def _tables(n, num_rels, dim, seed):
    en, rn, gen = scaled_tables(n, num_rels, dim, seed)
    return en.cuda(), rn.cuda(), gen


def _ks(n, m, rule):
    """(k, max_results): 1, 10, 1 000 and more than any relation's candidates at the default cap, and 10 with the TIGHTEST share that
    cannot overflow -- the largest tie block at a 10th distance, read off the reference ``rule(k)`` (relations at scale 2^6 over
    entities of length 2^-10 quantise their distances: exact ties are common), at least 12 -- which walks the histogram levels down
    until every slot's edge fits: slots resolve at different levels and sit out the later sweeps."""
    share = max(12, int(rule(10)[3]['count'].max()))
    return [(1, 1 << 22), (10, 1 << 22), (1000, 1 << 22), (n * n + 5, m * (n * n + 5)), (10, share * m)]


@pytest.mark.parametrize('p', [1, 2])
@pytest.mark.parametrize('n,dim,num_rels', SHAPES)
def test_every_relations_list_equals_the_definition(ops, n, dim, num_rels, p):
    from gcn_vae_amd import transe
    en, rn, gen = _tables(n, num_rels, dim, 3 * n + num_rels + dim)
    dist = _materialise(ops, en, rn, p)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=n <= 70)
    deepest = 0
    for filt, exclude_self in (({}, True), (dict(filt_lo=lo, filt_hi=hi, filt_ent=ent), True), (dict(filt_lo=lo, filt_hi=hi, filt_ent=ent), False)):
        for k, cap in _ks(n, num_rels, lambda k: transe.complete_relations_from_distances(dist, k, exclude_self=exclude_self, **filt)):
            kw = dict(exclude_self=exclude_self, max_results=cap, **filt)
            got = ops.transe_relation_topk(en, rn, k, p, **kw)
            assert got[0].dtype == got[1].dtype == torch.int64 and got[2].dtype == torch.float32
            assert got[0].shape == got[1].shape == got[2].shape == (num_rels, k) and got[3]['count'].shape == (num_rels,)
            assert same_rows(got, transe.complete_relations_from_distances(dist, k, **kw)), (k, cap, exclude_self, bool(filt))
            assert 2 <= got[3]['passes'] <= len(ops.MINE_RELATION_LEVELS) + 1
            deepest = max(deepest, got[3]['passes'])
    assert deepest > 2                                # the tight share made some slot walk below the first level
    # every relation's 10th distance in its own first-level bin (relations a binade apart share one: two binades a bin)
    kth = transe.complete_relations_from_distances(dist, 10)[2][:, 9]
    assert len(set(first_level_bins(kth))) >= (num_rels if num_rels <= 7 else 7)
    if num_rels > 1:                                  # the global miner's one threshold: the graph's nearest 500 leave relations out
        trip = ops.transe_mine(en, rn, p, k=500)[0]
        assert len(set(trip[:, 1].tolist())) < num_rels


@pytest.mark.parametrize('p', [1, 2])
def test_ties_zeros_nan_and_inf(ops, p):
    """Duplicated rows of en across tile boundaries (exact ties at the K-th value, zero distances under a zero relation), a NaN
    relation row (an all-padding row, count 0), an inf entity row (+inf candidates, last)."""
    from gcn_vae_amd import transe
    n, dim, num_rels = 130, 200, 7
    en, rn, gen = _tables(n, num_rels, dim, 17 + p)
    for j in (7, 63, 64, 70, 128, 129):
        en[j] = en[3]
    en[20, 5] = float('inf')
    rn[1] = 0.0                                       # d(s, 1, o) = d(o, 1, s), and 0 between the duplicated rows
    rn[4] = float('nan')
    dist = _materialise(ops, en, rn, p)
    for k in (1, 4, 10, 1000, n * n):
        got = ops.transe_relation_topk(en, rn, k, p, max_results=num_rels * n * n)
        assert same_rows(got, transe.complete_relations_from_distances(dist, k, max_results=num_rels * n * n)), k
        assert got[0][4].tolist() == [-1] * k and bool(torch.isinf(got[2][4]).all()) and int(got[3]['count'][4]) == 0
        assert not bool(torch.isnan(got[2]).any())
    zero = got[2] == 0
    assert int(zero[1].sum()) == 7 * 6 and not bool(torch.signbit(got[2][zero]).any())          # the seven equal rows, s != o
    live = got[0][0] >= 0                             # +inf candidates are kept, after every finite one: row 20 as subject or object
    assert bool(torch.isinf(got[2][0][live][-(2 * (n - 1)):]).all()) and not bool(torch.isinf(got[2][0][live][:-(2 * (n - 1))]).any())


def test_a_subset_in_any_order_equals_the_rows_of_the_whole(ops):
    from gcn_vae_amd import transe
    n, dim, num_rels, p = 130, 200, 7, 1
    en, rn, gen = _tables(n, num_rels, dim, 23)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=False)
    kw = dict(filt_lo=lo, filt_hi=hi, filt_ent=ent)
    whole = ops.transe_relation_topk(en, rn, 50, p, **kw)
    for rels in ([5, 0, 2], torch.tensor([6]), torch.tensor([2, 5, 0], device='cuda', dtype=torch.int32)):
        part = ops.transe_relation_topk(en, rn, 50, p, relations=rels, **kw)
        rows = torch.as_tensor(rels).cpu().long()
        assert part[0].shape == (len(rows), 50) and same_rows(part, whole, None, rows)
    dist = _materialise(ops, en, rn, p)
    assert same_rows(ops.transe_relation_topk(en, rn, 50, p, relations=[5, 0, 2], **kw),
                     transe.complete_relations_from_distances(dist, 50, relations=[5, 0, 2], **kw))


@pytest.mark.parametrize('p', [1, 2])
def test_the_routes_agree_with_each_other(ops, p):
    """complete_relations = complete_relations_unfused = per relation transe_mine(en, rn[r:r+1], k=K) with that relation's filter."""
    from gcn_vae_amd import ranking, transe
    n, dim, num_rels, k = 130, 200, 7, 40
    ent, rel, gen = _tables(n, num_rels, dim, 29)
    trip = torch.stack([torch.randint(0, n, (900,), generator=gen), torch.randint(0, num_rels, (900,), generator=gen),
                        torch.randint(0, n, (900,), generator=gen)], 1)
    fi = ranking.FilterIndex(n, num_rels, trip.numpy(), device='cuda')
    for norm_flag in (False, True):
        tables = (ent, rel, p, norm_flag)
        got = transe.complete_relations(tables, k, filter_index=fi)
        assert same_rows(got, transe.complete_relations_unfused(tables, k, filter_index=fi))
        en, rn = ops.transe_queries(ent, norm_flag=norm_flag), ops.transe_queries(rel, norm_flag=norm_flag)
        lo, hi, f_ent = ranking._mine_filter(fi, n, num_rels, ent.device)
        for r in range(num_rels):
            t, d, info = ops.transe_mine(en, rn[r:r + 1].contiguous(), p, k=k, filt_lo=lo[r::num_rels], filt_hi=hi[r::num_rels], filt_ent=f_ent)
            assert torch.equal(t[:, 0], got[0][r]) and torch.equal(t[:, 2], got[1][r]) and bool((t[:, 1] == 0).all())
            assert torch.equal(d.view(torch.int32), got[2][r].view(torch.int32)) and info['count'] == int(got[3]['count'][r])
        known = {tuple(x) for x in trip.tolist()}
        assert not any((int(s), r, int(o)) in known for r in range(num_rels) for s, o in zip(got[0][r].tolist(), got[1][r].tolist()))


def test_a_tie_above_the_share_is_an_overflow_naming_the_relation(ops):
    ones, r1 = torch.ones(100, 8, device='cuda'), torch.ones(2, 8, device='cuda')
    with pytest.raises(ops.MineOverflow) as err:
        ops.transe_relation_topk(ones, r1, 300, 1, max_results=2 * 9899)
    assert err.value.count == 9900 and 'relation 0' in str(err.value) and '9900' in str(err.value)
    assert 'at or below the K-th distance' in str(err.value)
    subj, obj, dist, info = ops.transe_relation_topk(ones, r1, 300, 1, max_results=2 * 9900)      # one more slot of share
    want = [(s, o) for s in range(100) for o in range(100) if s != o][:300]
    for r in range(2):
        assert list(zip(subj[r].tolist(), obj[r].tolist())) == want and bool((dist[r] == 8).all())
    assert info['count'].tolist() == [9900, 9900]
    with pytest.raises(ops.MineOverflow) as err:                 # only the tied relation is named
        r2 = torch.ones(2, 8, device='cuda')
        r2[0, 0] = float('nan')
        ops.transe_relation_topk(ones, r2, 300, 1, max_results=2 * 9899)
    assert 'relation 1' in str(err.value)


# ---- among type-correct pairs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [1, 2])
@pytest.mark.parametrize('n,dim,num_rels', [(50, 8, 3), (130, 200, 7), (70, 500, 6), (300, 16, 12)])
def test_typed_lists_equal_the_definition_on_masked_distances(ops, n, dim, num_rels, p):
    """mine_typed_cases' member lists: both sets full, 63 / 65, 64 / 1, an EMPTY subject set, 65 / 63, 1 / full."""
    from gcn_vae_amd import transe
    en, rn, gen = _tables(n, num_rels, dim, 5 * n + num_rels + dim)
    cs, co = member_masks(n, num_rels, gen)
    set_ptr, set_ids = member_lists(cs, co)
    dist = _materialise(ops, en, rn, p)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=n <= 70)
    masks = dict(cand_subj=cs.cuda(), cand_obj=co.cuda())
    for filt, exclude_self in (({}, True), (dict(filt_lo=lo, filt_hi=hi, filt_ent=ent), False)):
        for k, cap in _ks(n, num_rels, lambda k: transe.complete_relations_from_distances(dist, k, exclude_self=exclude_self, **masks, **filt)):
            kw = dict(exclude_self=exclude_self, max_results=cap, **filt)
            got = ops.transe_relation_topk_typed(en, rn, k, p, set_ptr, set_ids, **kw)
            assert same_rows(got, transe.complete_relations_from_distances(dist, k, **masks, **kw)), (k, cap, exclude_self, bool(filt))
            assert got[3]['passes'] <= len(ops.MINE_RELATION_TYPED_LEVELS) + 1
            if num_rels > 3:                         # relation 3 has no subject
                assert got[0][3].tolist() == [-1] * k and int(got[3]['count'][3]) == 0
    # a surviving fact's distance is the untyped call's, bit for bit
    k = n * n
    typed = ops.transe_relation_topk_typed(en, rn, k, p, set_ptr, set_ids, max_results=num_rels * k)
    plain = ops.transe_relation_topk(en, rn, k, p, max_results=num_rels * k)
    for r in range(num_rels):
        bits = torch.full((n, n), -1, dtype=torch.int64, device='cuda')
        live = plain[0][r] >= 0
        bits[plain[0][r][live], plain[1][r][live]] = plain[2][r][live].view(torch.int32).long()
        live = typed[0][r] >= 0
        assert torch.equal(bits[typed[0][r][live], typed[1][r][live]], typed[2][r][live].view(torch.int32).long())
    # a subset, and the spans: the result does not depend on them
    part = ops.transe_relation_topk_typed(en, rn, 10, p, set_ptr, set_ids, relations=[2, 0])
    whole = ops.transe_relation_topk_typed(en, rn, 10, p, set_ptr, set_ids)
    assert same_rows(part, whole, None, torch.tensor([2, 0]))
    for span in (1, 1000):
        assert same_rows(ops.transe_relation_topk_typed(en, rn, 10, p, set_ptr, set_ids, span=span), whole)


def test_typed_through_a_type_constraint_and_its_cross_check(ops):
    from gcn_vae_amd import ranking, transe
    n, dim, num_rels, k = 130, 200, 7, 25
    ent, rel, gen = _tables(n, num_rels, dim, 31)
    tables = (ent, rel, 1, True)
    trip = torch.stack([torch.randint(0, n, (600,), generator=gen), torch.randint(0, num_rels - 1, (600,), generator=gen),
                        torch.randint(0, n, (600,), generator=gen)], 1).numpy()      # relation 6 is never seen: empty sets
    fi, tc = ranking.FilterIndex(n, num_rels, trip, device='cuda'), ranking.TypeConstraint(n, num_rels, trip, device='cuda')
    got = transe.complete_relations(tables, k, relations=[6, 1, 4], filter_index=fi, type_constraint=tc)
    assert same_rows(got, transe.complete_relations_unfused(tables, k, relations=[6, 1, 4], filter_index=fi, type_constraint=tc))
    assert got[0][0].tolist() == [-1] * k
    mined = transe.mine_triplets(tables, threshold=float('inf'), filter_index=fi, type_constraint=tc, max_results=2 ** 31 - 1)
    for i, r in enumerate([6, 1, 4]):                # mine_triplets(type_constraint=)'s rule, on the same member lists
        of_r = mined[0][:, 1] == r
        assert torch.equal(mined[0][of_r][:k, 0], got[0][i][got[0][i] >= 0]) and torch.equal(mined[0][of_r][:k, 2], got[1][i][got[1][i] >= 0])
        assert torch.equal(mined[1][of_r][:k].view(torch.int32), got[2][i][got[0][i] >= 0].view(torch.int32))


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_relation_profiles(tmp_path):
    from gcn_vae_amd import data, transe
    spec = 'synthetic:60:4:400:40:40'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    ckpt = str(tmp_path / 'transe.ckpt')
    model.save_checkpoint(ckpt)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    seen_s = {r: {t[0] for t in known if t[1] == r} for r in range(kg.num_rels)}
    seen_o = {r: {t[2] for t in known if t[1] == r} for r in range(kg.num_rels)}
    which, k = [kg.num_rels - 1, 0, 2], 7
    base = ['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt, '--relation-profile-topk', str(k)]
    for typed in (False, True):
        out = str(tmp_path / f'relations_{typed}.tsv')
        transe.main(transe.build_parser().parse_args(base + ['--relation-profile-ids', ','.join(map(str, which)), '--relation-profile-out', out]
                                                     + (['--relation-profile-typed'] if typed else [])))
        rows = [line.rstrip('\n').split('\t') for line in open(out)]
        assert all(len(row) == 5 for row in rows) and 0 < len(rows) <= len(which) * k
        groups = [int(row[1]) for row in rows]
        assert [r for i, r in enumerate(groups) if i == 0 or groups[i - 1] != r] == [r for r in which if r in groups]      # the order asked
        for r in set(groups):
            mine = [row for row in rows if int(row[1]) == r]
            assert [int(row[3]) for row in mine] == list(range(1, len(mine) + 1))                                          # rank from 1
            dists = [float(row[4]) for row in mine]
            assert dists == sorted(dists) and (typed or len(mine) == k)
            for s, _, o, _, _ in mine:
                assert (int(s), r, int(o)) not in known and s != o
                assert not typed or (int(s) in seen_s[r] and int(o) in seen_o[r])
    everything = str(tmp_path / 'all.tsv')
    transe.main(transe.build_parser().parse_args(base + ['--relation-profile-out', everything]))
    rows = [line.split('\t') for line in open(everything)]
    assert len(rows) == kg.num_rels * k and [int(row[1]) for row in rows] == [r for r in range(kg.num_rels) for _ in range(k)]
