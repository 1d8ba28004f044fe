"""Type-constrained whole-graph TransE mining on the GPU (gv_transe_mine_typed / ops.transe_mine_typed / transe.mine_triplets(...,
type_constraint=) / --complete-typed) against the definition: mine_cases.brute_force on the materialised distances
(ops.transe_queries + ops.transe_distances per relation at full (R, N, N)) with the known and the type-incorrect triplets
excluded, and against the existing unconstrained kernel.  Every comparison is exact.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from mine_cases import _lists, _same
from mine_typed_cases import Oracle, check_against, excluded, member_lists, member_masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def _normalised(ops, ent, rel, norm_flag):
    return ops.transe_queries(ent.contiguous(), norm_flag=norm_flag), ops.transe_queries(rel.contiguous(), norm_flag=norm_flag)


def _materialise(ops, ent, rel, p, norm_flag):
    """dist[r, s, o], by the kernels that define the distance: the tail queries of (s, r) against the normalised table."""
    ent, rel = ent.contiguous(), rel.contiguous()
    en = ops.transe_queries(ent, norm_flag=norm_flag)
    s = torch.arange(ent.shape[0], device='cuda')
    return torch.stack([ops.transe_distances(ops.transe_queries(ent, rel, s, torch.full_like(s, r), head=False, norm_flag=norm_flag),
                                             en, p) for r in range(rel.shape[0])])


def _tables(n, dim, num_rels, seed, scale=0.5):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, dim, generator=gen) * scale).cuda(), (torch.randn(num_rels, dim, generator=gen) * scale).cuda(), gen


@pytest.mark.parametrize('norm_flag', [0, 1])
@pytest.mark.parametrize('p', [1, 2])
@pytest.mark.parametrize('n,dim,num_rels', [(1, 1, 1), (7, 5, 2), (65, 37, 3), (130, 200, 4), (130, 500, 2)])
def test_typed_mining_equals_the_definition(ops, n, dim, num_rels, p, norm_flag):
    """One tile, a tile edge, one column chunk (dim <= 64) and several with a partial last one (200, 500); member lists of 0, 1,
    63, 64, 65 and n entities (more than four object tiles never fit 130 entities: test_against_the_unconstrained_kernel has
    them), relation 0 with both sets full; no filter, a sparse and a dense one; exclude_self on and off."""
    ent, rel, gen = _tables(n, dim, num_rels, n * 7 + dim + num_rels)
    cs, co = member_masks(n, num_rels, gen)
    ptr, ids = member_lists(cs, co)
    dist = _materialise(ops, ent, rel, p, norm_flag)
    en, rn = _normalised(ops, ent, rel, norm_flag)
    for filt in (None, _lists(n * num_rels, n, gen, dense=False), _lists(n * num_rels, n, gen, dense=True)):
        excl = excluded(cs, co, filt)
        f = {} if filt is None else dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filt))
        for exclude_self in (True, False):
            oracle = Oracle(dist, True, excl, exclude_self)
            check_against(oracle, lambda **sel: ops.transe_mine_typed(en, rn, p, ptr, ids, exclude_self=exclude_self, **f, **sel),
                          thresholds=(float('inf'), 0.0, -1.0))


@pytest.mark.parametrize('p', [1, 2])
def test_against_the_unconstrained_kernel(ops, p):
    """gv_transe_mine at threshold +inf returns every candidate; filtered on the host with TypeConstraint.contains its first K and
    the count at the K-th value are the typed route's, bit for bit.  With all sets full the two routes agree outright; the
    grouping of object tiles into spans (more than one round of four among them) does not change the result."""
    from gcn_vae_amd import ranking
    n, dim, num_rels = 130, 64, 4
    ent, rel, gen = _tables(n, dim, num_rels, 77)
    en, rn = _normalised(ops, ent, rel, 1)
    known = torch.stack([torch.randint(0, n, (900,), generator=gen), torch.randint(0, num_rels, (900,), generator=gen),
                         torch.randint(0, n, (900,), generator=gen)], 1)
    tc = ranking.TypeConstraint(n, num_rels, known[:300], device='cuda')
    fi = ranking.FilterIndex(n, num_rels, known, device='cuda')
    lo, hi, f_ent = ranking._mine_filter(fi, n, num_rels, en.device)
    f = dict(filt_lo=lo, filt_hi=hi, filt_ent=f_ent)
    trip, d, _ = ops.transe_mine(en, rn, p, threshold=float('inf'), **f)
    keep = tc.contains(trip[:, 1], trip[:, 0], 's') & tc.contains(trip[:, 1], trip[:, 2], 'o')
    trip, d = trip[keep], d[keep]
    assert 1000 < trip.shape[0] < n * num_rels * n
    ptr, ids = tc.members('cuda')
    for k in (1, 10, 1000, trip.shape[0], trip.shape[0] + 1):
        got = ops.transe_mine_typed(en, rn, p, ptr, ids, k=k, **f)
        m = min(k, trip.shape[0])
        assert torch.equal(got[0], trip[:m]) and torch.equal(got[1].view(torch.int32), d[:m].view(torch.int32))
        assert got[2]['count'] == int((d <= d[m - 1]).sum())
    full = ranking.TypeConstraint(n, num_rels, torch.stack([torch.arange(n).repeat(num_rels), torch.arange(num_rels).repeat_interleave(n),
                                                            torch.arange(n).repeat(num_rels)], 1), device='cuda')
    ptr, ids = full.members('cuda')
    for sel in (dict(k=1), dict(k=5000), dict(threshold=float(d[2000])), dict(threshold=float('inf'))):
        for exclude_self in (True, False):
            assert _same(ops.transe_mine_typed(en, rn, p, ptr, ids, exclude_self=exclude_self, **f, **sel),
                         ops.transe_mine(en, rn, p, exclude_self=exclude_self, **f, **sel))
    ent3, rel3, gen3 = _tables(600, 24, 3, 78)
    cs, co = member_masks(600, 3, gen3, lengths=[(None, None), (200, 590), (65, 130)])
    ptr, ids = member_lists(cs, co)
    want = ops.transe_mine_typed(ent3, rel3, p, ptr, ids, k=2000, span=1)
    for span in (2, 4, 5, 8, 12, None):
        assert _same(ops.transe_mine_typed(ent3, rel3, p, ptr, ids, k=2000, span=span), want)


@pytest.mark.parametrize('p', [1, 2])
def test_ties_and_the_refining_passes(ops, p):
    from gcn_vae_amd import transe
    # an all-equal table, relation rows of ones: every type-correct candidate ties at ||1||_p over 8 columns
    n, num_rels = 100, 2
    ent, rel = torch.ones(n, 8, device='cuda'), torch.ones(num_rels, 8, device='cuda')
    cs, co = member_masks(n, num_rels, torch.Generator().manual_seed(1), lengths=[(70, 65), (64, None)])
    ptr, ids = member_lists(cs, co)
    want = [(s, r, o) for s in range(n) for r in range(num_rels) for o in range(n) if s != o and cs[r, s] and co[r, o]]
    trip, d, info = ops.transe_mine_typed(ent, rel, p, ptr, ids, k=300)
    assert [tuple(x) for x in trip.tolist()] == want[:300] and info['count'] == len(want)
    assert bool((d == (8.0 if p == 1 else np.sqrt(np.float32(8.0)))).all())
    with pytest.raises(ops.MineOverflow) as err:
        ops.transe_mine_typed(ent, rel, p, ptr, ids, k=300, max_results=len(want) - 1)
    assert err.value.count == len(want)
    # distances packed into one bin of the first histogram: a small cap forces the second and third levels
    gen = torch.Generator().manual_seed(3)
    n, num_rels, dim, k = 300, 2, 16, 1000
    ent = (0.001 * torch.rand(n, dim, generator=gen)).cuda()
    rel = torch.ones(num_rels, dim, device='cuda')
    cs, co = member_masks(n, num_rels, gen, lengths=[(None, None), (130, 200)])
    ptr, ids = member_lists(cs, co)
    dist = _materialise(ops, ent, rel, p, 0)
    want = transe.mine_from_distances(dist, k=k, cand_subj=cs.cuda(), cand_obj=co.cuda())
    got = ops.transe_mine_typed(ent, rel, p, ptr, ids, k=k, max_results=5000)
    assert got[2]['passes'] > 2 and _same(got, want)
    roomy = ops.transe_mine_typed(ent, rel, p, ptr, ids, k=k)
    assert _same(roomy, want)
    tight = ops.transe_mine_typed(ent, rel, p, ptr, ids, k=k, max_results=want[2]['count'])
    assert tight[2]['passes'] > 2 and _same(tight, want)


@pytest.mark.parametrize('p', [1, 2])
def test_special_values_inside_and_outside_the_member_lists(ops, p):
    n, dim, num_rels = 130, 8, 2
    ent, rel, gen = _tables(n, dim, num_rels, 5)
    cs, co = member_masks(n, num_rels, gen, lengths=[(65, 70), (64, 65)])
    cs[:, [3, 5, 6, 7, 8]] = True
    co[:, [3, 5, 6, 7, 8]] = True
    cs[:, 4] = False
    co[:, 4] = False
    ptr, ids = member_lists(cs, co)
    base = ops.transe_mine_typed(ent, rel, p, ptr, ids, threshold=float('inf'))
    ent[4] = float('nan')                                     # a NaN row outside every set changes nothing
    assert _same(ops.transe_mine_typed(ent, rel, p, ptr, ids, threshold=float('inf')), base)
    ent[3] = float('nan')
    ent[5] = 0.0
    ent[5, 0] = float('inf')                                  # +inf against every other row
    ent[6] = 0.0
    ent[6, 0] = float('-inf')
    ent[7] = 0.0                                              # with the zero relation: distance +0
    ent[8] = -0.0
    rel[1] = 0.0
    dist = _materialise(ops, ent, rel, p, 0)
    oracle = Oracle(dist, True, excluded(cs, co), True)
    check_against(oracle, lambda **sel: ops.transe_mine_typed(ent, rel, p, ptr, ids, **sel), ks=(1, 10, 3000),
                  thresholds=(float('inf'), 0.0, -0.0, -1.0))
    got = ops.transe_mine_typed(ent, rel, p, ptr, ids, threshold=float('inf'))
    assert bool(torch.isinf(got[1][-1])) and not bool(torch.isnan(got[1]).any()) and not bool(torch.signbit(got[1]).any())
    assert not bool(((got[0][:, 0] == 3) | (got[0][:, 2] == 3)).any())


def test_strided_tables_are_made_contiguous(ops):
    gen = torch.Generator().manual_seed(9)
    base_e, base_r = torch.randn(300, 50, generator=gen).cuda(), torch.randn(6, 50, generator=gen).cuda()
    ent, rel = base_e[::2, 3:40], base_r[::2, 5:42]          # ld > dim, odd width, bases that are not 16-byte aligned
    n, num_rels = ent.shape[0], rel.shape[0]
    cs, co = member_masks(n, num_rels, gen)
    ptr, ids = member_lists(cs, co)
    oracle = Oracle(_materialise(ops, ent, rel, 1, 0), True, excluded(cs, co), True)
    check_against(oracle, lambda **sel: ops.transe_mine_typed(ent, rel, 1, ptr, ids, **sel), ks=(1, 333), thresholds=(12.0,))


def test_empty_results(ops):
    ent, rel, gen = _tables(70, 12, 3, 2)
    nobody = torch.zeros(3, 70, dtype=torch.bool)
    cs, co = member_masks(70, 3, gen)
    for masks in ((nobody, nobody), (cs, nobody), (nobody, co)):
        ptr, ids = member_lists(*masks)
        for sel in (dict(k=5), dict(threshold=float('inf'))):
            got = ops.transe_mine_typed(ent, rel, 2, ptr, ids, **sel)
            assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2] == {'count': 0, 'passes': 0}        # no launch
    ptr, ids = member_lists(cs, co)
    got = ops.transe_mine_typed(ent, rel, 2, ptr, ids, threshold=-1.0)
    assert got[0].shape == (0, 3) and got[2]['count'] == 0
    none = ops.transe_mine_typed(ent[:0], rel, 2, torch.zeros(7, dtype=torch.int64, device='cuda'),
                                 torch.zeros(0, dtype=torch.int32, device='cuda'), k=5)
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2]['count'] == 0
    with pytest.raises(ValueError):
        ops.transe_mine_typed(ent, rel, 2, ptr, torch.where(ids == ids.max(), 70, ids), k=5)


def test_wrappers_fused_equals_unfused():
    from gcn_vae_amd import data, ranking, transe
    kg = data.load_data('synthetic:300:7:2000:100:100')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    ent, rel, _ = _tables(kg.num_nodes, 32, kg.num_rels, 4)
    for p, norm_flag in ((1, True), (2, False)):
        tables = (ent, rel, p, norm_flag)
        for sel in (dict(k=1), dict(k=500), dict(k=10 ** 7), dict(threshold=4.0 if p == 1 else 1.0)):
            for kw in (dict(filter_index=fi), dict(exclude_self=False)):
                got = transe.mine_triplets(tables, type_constraint=tc, **sel, **kw)
                assert _same(got, transe.mine_triplets_unfused(tables, type_constraint=tc, **sel, **kw))
                assert bool((tc.contains(got[0][:, 1], got[0][:, 0], 's') & tc.contains(got[0][:, 1], got[0][:, 2], 'o')).all())
    with pytest.raises(ValueError, match='TypeConstraint'):
        transe.mine_triplets((ent[:-1], rel, 1, True), k=3, type_constraint=tc)


def test_cli_writes_type_correct_completions(tmp_path):
    from gcn_vae_amd import data, ranking, transe
    spec = 'synthetic:300:7:2000:100:100'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    ckpt, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'typed.tsv')
    model.save_checkpoint(ckpt)
    args = transe.build_parser().parse_args(['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                             '--complete-topk', '200', '--complete-typed', '--complete-out', out])
    transe.main(args)
    rows = np.array([[int(x) for x in line.split('\t')[:4]] for line in open(out)])
    assert rows.shape == (200, 4) and rows[:, 3].tolist() == list(range(200))
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test)
    s, r, o = (torch.from_numpy(rows[:, i]) for i in range(3))
    assert bool(tc.contains(r, s, 's').all()) and bool(tc.contains(r, o, 'o').all())
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    assert all(tuple(x[:3]) not in known and x[0] != x[2] for x in rows.tolist())


@pytest.mark.parametrize('p', [1, 2])
def test_fb15k237_size_fused_equals_unfused_and_times(p, capsys):
    """FB15k-237-synthetic size, dim 200, K = 100 000, sets and filter from train + valid + test: exact agreement of the two typed
    routes; the times are printed, no ratio is asserted."""
    import time
    from gcn_vae_amd import data, ranking, transe
    kg = data.load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    ent, rel, _ = _tables(kg.num_nodes, 200, kg.num_rels, 5, scale=0.3)
    out = {}
    for name, fn in (('fused', transe.mine_triplets), ('unfused', transe.mine_triplets_unfused)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out[name] = fn((ent, rel, p, True), k=100000, filter_index=fi, type_constraint=tc)
        torch.cuda.synchronize()
        out[name + '_s'] = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\ntyped TransE L{p} mining, FB15k-237-synthetic, dim=200, K=100000 (first call each): fused {out['fused_s'] * 1e3:.1f} ms, "
              f"unfused {out['unfused_s'] * 1e3:.1f} ms")
    assert out['fused'][0].shape == (100000, 3) and _same(out['fused'], out['unfused'])
