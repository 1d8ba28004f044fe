"""Whole-graph TransE mining on the GPU (gv_transe_mine / ops.transe_mine / transe.mine_triplets / the CLI) against the rule
stated on materialised distances: ops.transe_queries + ops.transe_distances per relation, selected by
transe.mine_from_distances.  Every comparison is exact: triplets equal, distances equal as bit patterns, counts equal.
pytest -m gpu."""
import numpy as np
import pytest
import torch

from mine_cases import _lists, _same

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
    n = ent.shape[0]
    en = ops.transe_queries(ent, norm_flag=norm_flag)
    s = torch.arange(n, device='cuda')
    return torch.stack([ops.transe_distances(ops.transe_queries(ent, rel, s, torch.full_like(s, r), head=False, norm_flag=norm_flag),
                                             en, p) for r in range(rel.shape[0])])


def _tables(n, dim, num_rels, seed, scale=0.5):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, dim, generator=gen) * scale).cuda(), (torch.randn(num_rels, dim, generator=gen) * scale).cuda(), gen


SHAPES = [(1, 1, 1), (7, 5, 2), (64, 37, 9), (65, 200, 2), (65, 512, 1), (130, 301, 2), (777, 100, 9), (777, 512, 2), (1300, 200, 2),
          (3001, 5, 9)]


@pytest.mark.parametrize('norm_flag', [0, 1])
@pytest.mark.parametrize('p', [1, 2])
@pytest.mark.parametrize('n,dim,num_rels', SHAPES)
def test_mining_equals_the_definition(ops, n, dim, num_rels, p, norm_flag):
    """Tile edges (1, 7, 64, 65, 130, 777, 1300, 3001 rows), one column chunk (dim <= 224), several (301, 512) with a partial last
    one, widths around the LDS-resident limit, one and several relation spans."""
    from gcn_vae_amd import transe
    ent, rel, gen = _tables(n, dim, num_rels, n * 7 + dim + num_rels)
    dist = _materialise(ops, ent, rel, p, norm_flag)
    en, rn = _normalised(ops, ent, rel, norm_flag)
    lo, hi, f_ent = _lists(n * num_rels, n, gen, dense=n <= 65)
    for filt in ({}, dict(filt_lo=lo, filt_hi=hi, filt_ent=f_ent)):
        for exclude_self in (True, False):
            kw = dict(exclude_self=exclude_self, **filt)
            everything = transe.mine_from_distances(dist, threshold=float('inf'), max_results=2 ** 31 - 1, **kw)[1]
            for k in sorted({1, 10, 1000, max(1, min(everything.numel() // 3, 50000))}):
                got = ops.transe_mine(en, rn, p, k=k, **kw)
                assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (min(k, everything.numel()), 3)
                assert _same(got, transe.mine_from_distances(dist, k=k, **kw)), (k, exclude_self, bool(filt))
            cuts = [0.0, -1.0] + ([float('inf')] if everything.numel() <= 200000 else [])
            if everything.numel():
                cuts += [float(everything[min(everything.numel() - 1, 500)]), float(everything[min(everything.numel() - 1, 20000)])]
            for t in cuts:
                got = ops.transe_mine(en, rn, p, threshold=t, **kw)
                assert _same(got, transe.mine_from_distances(dist, threshold=t, **kw)), (t, exclude_self, bool(filt))
                assert got[2]['passes'] == 1
            assert ops.transe_mine(en, rn, p, threshold=-1.0, **kw)[0].shape == (0, 3)


@pytest.mark.parametrize('p', [1, 2])
def test_ties_nan_inf_and_zero(ops, p):
    from gcn_vae_amd import transe
    dim, n, num_rels = 8, 1300, 3
    gen = torch.Generator().manual_seed(0)
    ent = torch.randn(n, dim, generator=gen).cuda()
    rel = torch.randn(num_rels, dim, generator=gen).cuda()
    for j in (7, 70, 130, 200, 299, 1000, 1299):             # exact ties across tiles
        ent[j] = ent[3]
    ent[10] = float('nan')
    ent[250] = float('nan')
    ent[20] = 0.0                                            # zero rows and a zero relation: distance +0
    ent[21] = -0.0
    rel[1] = 0.0
    ent[40] = 0.0
    ent[40, 0] = float('inf')                                # +inf against every other row, inf - inf = NaN against itself
    ent[41] = 0.0
    ent[41, 0] = float('-inf')
    dist = _materialise(ops, ent, rel, p, 0)
    assert float(dist[1, 20, 21]) == 0.0 and bool(torch.isinf(dist[0, 40, 5])) and bool(torch.isnan(dist[0, 40, 40]))
    for exclude_self in (True, False):
        kw = dict(exclude_self=exclude_self)
        for k in (1, 10, 5000, 200000):
            assert _same(ops.transe_mine(ent, rel, p, k=k, **kw), transe.mine_from_distances(dist, k=k, **kw))
        for t in (0.0, -0.0, 1.5, float(torch.nan_to_num(dist, nan=float('inf')).flatten().kthvalue(30000).values)):
            got = ops.transe_mine(ent, rel, p, threshold=t, **kw)
            assert _same(got, transe.mine_from_distances(dist, threshold=t, **kw))
            assert not bool(torch.isnan(got[1]).any())
        got = ops.transe_mine(ent, rel, p, threshold=0.0, **kw)
        assert got[0].shape[0] > 0 and bool((got[1] == 0).all()) and not bool(torch.signbit(got[1]).any())      # +0, never -0
        if exclude_self:
            assert bool((got[0][:, 0] != got[0][:, 2]).all())
    # +inf distances are candidates and come last; NaN ones (a NaN row, inf - inf) never come
    sub = torch.tensor([3, 10, 20, 21, 40, 41, 5, 7], device='cuda')
    e2 = ent[sub].contiguous()
    d2 = _materialise(ops, e2, rel, p, 0)
    got = ops.transe_mine(e2, rel, p, threshold=float('inf'), exclude_self=False)
    assert _same(got, transe.mine_from_distances(d2, threshold=float('inf'), exclude_self=False))
    assert got[0].shape[0] == int((~torch.isnan(d2)).sum()) and bool(torch.isinf(got[1][-1])) and not bool(torch.isnan(got[1]).any())
    n_inf = int(torch.isinf(d2).sum())
    assert n_inf > 0 and bool(torch.isinf(got[1][-n_inf:]).all()) and not bool(torch.isinf(got[1][:-n_inf]).any())
    assert not bool(((got[0][:, 0] == 1) | (got[0][:, 2] == 1)).any())                  # the NaN row
    assert not bool(((got[0][:, 0] == 4) & (got[0][:, 2] == 4)).any())                  # inf - inf
    # an all-equal table: the first K triplets in (s, r, o) order; a cap below the tie block is the error, with its size
    ones, r1 = torch.ones(100, 8, device='cuda'), torch.ones(2, 8, device='cuda')
    trip, d, info = ops.transe_mine(ones, r1, p, k=300)
    want = [(s, r, o) for s in range(100) for r in range(2) for o in range(100) if s != o][:300]
    assert [tuple(x) for x in trip.tolist()] == want and bool((d == (8.0 if p == 1 else float(torch.tensor(8.0).sqrt()))).all()) and info['count'] == 19800
    with pytest.raises(ops.MineOverflow) as err:
        ops.transe_mine(ones, r1, p, k=300, max_results=19799)
    assert err.value.count == 19800 and '19800' in str(err.value)
    assert ops.transe_mine(ones, r1, p, k=300, max_results=19800)[0].shape == (300, 3)
    assert ops.transe_mine(ones, r1, p, k=10 ** 6)[0].shape == (19800, 3)                # K beyond the candidates: all of them


@pytest.mark.parametrize('p', [1, 2])
def test_dense_distances_take_the_refining_passes(ops, p):
    """Every distance inside ONE bin of the first, 12-bit histogram (sign, exponent, three mantissa bits of -d).  With a cap below
    that bin's population the threshold is narrowed by further histogram passes before anything is emitted."""
    from gcn_vae_amd import transe
    gen = torch.Generator().manual_seed(3)
    n, num_rels, dim, k = 300, 2, 16, 1000
    ent = (0.01 * torch.rand(n, dim, generator=gen)).cuda()
    rel = torch.full((num_rels, dim), 1.03, device='cuda')         # p = 1: d ~ 16.5 in [16, 18); p = 2: d ~ 4.12 in [4, 4.5)
    dist = _materialise(ops, ent, rel, p, 0)
    bins = (-dist).view(torch.int32) >> 20
    assert int(bins.min()) == int(bins.max())
    want = transe.mine_from_distances(dist, k=k)
    got = ops.transe_mine(ent, rel, p, k=k, max_results=5000)
    assert got[2]['passes'] > 2 and _same(got, want)
    roomy = ops.transe_mine(ent, rel, p, k=k)
    assert roomy[2]['passes'] == 2 and _same(roomy, want)                  # one histogram, one emission
    tight = ops.transe_mine(ent, rel, p, k=k, max_results=want[2]['count'])     # down to the exact value of the K-th distance
    assert tight[2]['passes'] > 2 and _same(tight, want)


def test_topk_is_a_prefix_of_the_threshold_run_and_counts_are_exact(ops):
    from gcn_vae_amd import ranking, transe
    ent, rel, gen = _tables(900, 48, 4, 21)
    lo, hi, f_ent = _lists(900 * 4, 900, gen, dense=False)
    filt = dict(filt_lo=lo, filt_hi=hi, filt_ent=f_ent)
    en, rn = _normalised(ops, ent, rel, 1)
    k = 700
    trip, d, info = ops.transe_mine(en, rn, 1, k=k, **filt)
    t = float(d[-1])
    trip_t, d_t, info_t = ops.transe_mine(en, rn, 1, threshold=t, **filt)
    assert torch.equal(trip_t[:k], trip) and torch.equal(d_t[:k].view(torch.int32), d.view(torch.int32))
    assert info['count'] == info_t['count'] == trip_t.shape[0]
    dist = _materialise(ops, ent, rel, 1, 1)
    listed = ranking._listed_mask(lo, hi, f_ent, 900 * 4, 900, 'cuda').view(900, 4, 900).permute(1, 0, 2)
    dist[listed] = float('nan')
    dist[:, torch.arange(900), torch.arange(900)] = float('nan')
    cut = float(torch.nan_to_num(dist, nan=float('inf')).flatten().kthvalue(3000).values)
    for c in (t, cut, 0.0):
        assert ops.transe_mine(en, rn, 1, threshold=c, **filt)[2]['count'] == int((dist <= c).sum())
    true = int((dist <= cut).sum())                               # overflow: the message's count is the true one
    assert true >= 3000
    with pytest.raises(ops.MineOverflow) as err:
        ops.transe_mine(en, rn, 1, threshold=cut, max_results=true - 1, **filt)
    assert err.value.count == true and str(true) in str(err.value)
    with pytest.raises(ops.MineOverflow) as err:
        ops.transe_mine(en, rn, 1, threshold=cut, max_results=3, **filt)
    assert err.value.count == true
    assert ops.transe_mine(en, rn, 1, threshold=cut, max_results=true, **filt)[0].shape[0] == true


def test_strided_tables_and_an_empty_one(ops):
    from gcn_vae_amd import transe
    gen = torch.Generator().manual_seed(9)
    base_e, base_r = torch.randn(300, 50, generator=gen).cuda(), torch.randn(6, 50, generator=gen).cuda()
    en, rn = base_e[::2, 3:40], base_r[::2, 5:42]            # non-contiguous rows, odd width, unaligned
    assert not en.is_contiguous() and not rn.is_contiguous()
    for p in (1, 2):
        dist = _materialise(ops, en, rn, p, 0)
        cut = float(dist.flatten().kthvalue(2000).values)
        assert _same(ops.transe_mine(en, rn, p, k=333), transe.mine_from_distances(dist, k=333))
        assert _same(ops.transe_mine(en, rn, p, threshold=cut), transe.mine_from_distances(dist, threshold=cut))
        assert _same(transe.mine_triplets((en, rn, p, False), k=333), transe.mine_from_distances(dist, k=333))
        assert _same(ops.transe_mine(en.t().contiguous().t(), rn, p, k=333), transe.mine_from_distances(dist, k=333))   # column-major
    for fn in (lambda: ops.transe_mine(en[:0], rn, 1, k=5), lambda: transe.mine_triplets((en[:0], rn, 1, True), k=5),
               lambda: transe.mine_triplets_unfused((en[:0], rn, 1, True), threshold=3.0)):
        none = fn()
        assert none[0].shape == (0, 3) and none[0].dtype == torch.int64 and none[1].shape == (0,) and none[2]['count'] == 0


@pytest.mark.parametrize('p', [1, 2])
def test_crosscheck_with_predict_topk(ops, p):
    """Every (s, r) group of the mined list is the head of that query's predict_topk list (same filter, same order, bit-equal
    distances).  predict_topk keeps s == o, so self triplets stay in here."""
    from gcn_vae_amd import ranking, transe
    n, num_rels, dim, k = 2500, 5, 64, 2000
    ent, rel, gen = _tables(n, dim, num_rels, 11, scale=1.0)
    known = torch.stack([torch.randint(0, n, (4000,), generator=gen), torch.randint(0, num_rels, (4000,), generator=gen),
                         torch.randint(0, n, (4000,), generator=gen)], 1)
    fi = ranking.FilterIndex(n, num_rels, known, device='cuda')
    tables = (ent, rel, p, True)
    trip, d, _ = transe.mine_triplets(tables, k=k, filter_index=fi, exclude_self=False)
    assert trip.shape[0] == k
    group = trip[:, 0] * num_rels + trip[:, 1]
    keys, sizes = torch.unique(group, return_counts=True)
    assert int(sizes.max()) < 128                             # what makes the comparison with k = 128 lists complete
    ids, dd = transe.predict_topk(tables, keys // num_rels, keys % num_rels, 128, direction='o', filter_index=fi)
    for i, (key, size) in enumerate(zip(keys.tolist(), sizes.tolist())):
        mine = group == key                                   # the mined list is sorted: a group's members keep its order
        assert torch.equal(trip[mine, 2], ids[i, :size])
        assert torch.equal(d[mine].view(torch.int32), dd[i, :size].view(torch.int32))


@pytest.mark.parametrize('p', [1, 2])
def test_fused_equals_unfused_with_a_filter_index(p):
    from gcn_vae_amd import ranking, transe
    n, num_rels, dim = 3001, 9, 200
    ent, rel, gen = _tables(n, dim, num_rels, 17, scale=0.1)
    known = torch.stack([torch.randint(0, n, (20000,), generator=gen), torch.randint(0, num_rels, (20000,), generator=gen),
                         torch.randint(0, n, (20000,), generator=gen)], 1)
    fi = ranking.FilterIndex(n, num_rels, known, device='cuda')
    model = transe.TransE(n, num_rels, dim=dim, p_norm=p, norm_flag=True).cuda()
    model.ent_embeddings.weight.data.copy_(ent)
    model.rel_embeddings.weight.data.copy_(rel)
    got = transe.mine_triplets(model, k=20000, filter_index=fi)
    want = transe.mine_triplets_unfused(model, k=20000, filter_index=fi)
    assert got[0].shape == (20000, 3) and _same(got, want) and want[2]['passes'] == num_rels
    lin = lambda t: (t[:, 0] * num_rels + t[:, 1]) * n + t[:, 2]
    assert not bool(torch.isin(lin(got[0]), lin(known.cuda())).any()) and bool((got[0][:, 0] != got[0][:, 2]).all())
    t = float(got[1][4999])
    assert _same(transe.mine_triplets(model, threshold=t, filter_index=fi), transe.mine_triplets_unfused(model, threshold=t, filter_index=fi))


def test_cli_writes_the_mined_completions(tmp_path):
    from gcn_vae_amd import data, ranking, transe
    spec = 'synthetic:300:7:2000:100:80:3'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    ckpt, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'done.tsv')
    model.save_checkpoint(ckpt)
    args = transe.build_parser().parse_args(['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                             '--complete-topk', '50', '--complete-out', out])
    transe.main(args)
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert len(rows) == 50 and all(len(x) == 5 for x in rows)
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    loaded = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    loaded.load_checkpoint(ckpt)
    trip, d, _ = transe.mine_triplets(loaded.cuda(), k=50, filter_index=fi)
    assert [[int(x[0]), int(x[1]), int(x[2])] for x in rows] == trip.tolist()
    assert [int(x[3]) for x in rows] == list(range(50))
    assert [np.float32(x[4]) for x in rows] == d.cpu().numpy().tolist()              # %.9g round-trips a float32
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    assert all((int(x[0]), int(x[1]), int(x[2])) not in known and x[0] != x[2] for x in rows)
    # both flags: the K nearest, cut at D
    cut = float(d[19])
    n_cut = int((d <= cut).sum())
    args = transe.build_parser().parse_args(['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                             '--complete-topk', '50', '--complete-threshold', repr(cut), '--complete-out', out])
    transe.main(args)
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert len(rows) == n_cut and [[int(x[0]), int(x[1]), int(x[2])] for x in rows] == trip[:n_cut].tolist()
