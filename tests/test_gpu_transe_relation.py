"""Relation prediction for TransE on the GPU (gv_transe_pair_rel / ops.transe_pair_relations / transe.rank_relations,
predict_relations) against the materialised twin: ops.transe_distances(en[o] - en[s], rn, p), ranked by ranking.mid_ranks on the
negated distances and ordered by transe.topk_from_distances.  Every comparison is exact: ids and ranks by torch.equal, distances
by their bits.  pytest -m gpu."""
import pytest
import torch

import relation_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def transe():
    from gcn_vae_amd import transe as _transe
    return _transe


def _tables(num_rels, dim, gen):
    return (torch.randn(rc.N, dim, generator=gen) * 0.5).cuda(), (torch.randn(num_rels, dim, generator=gen) * 0.5).cuda()


def _twin(transe, en, rn, s, o, p, target, k, filt=(None, None, None)):
    from gcn_vae_amd import ranking
    dist = transe.pair_distances_unfused(en, rn, s, o, p)
    return ranking.relation_ranks_from_scores(-dist, target, *filt), transe.topk_from_distances(dist, k, *filt)


def _check_all_forms(ops, transe, en, rn, s, o, p, target, k):
    """Fused == twin, with and without a filter; ranks only, top-k only and both in one call agree; count_raw does not depend on
    the filter."""
    gen = torch.Generator().manual_seed(int(target.sum()) + k + p)
    filt = rc.relation_lists(s.numel(), rn.shape[0], target.cpu(), gen)
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    (raw0, none), top0 = ops.transe_pair_relations(en, rn, s, o, p, target=target, k=k)
    want_ranks, want_top = _twin(transe, en, rn, s, o, p, target, k)
    assert none is None and torch.equal(raw0, want_ranks[0]) and rc.same_lists(top0, want_top)
    (raw, filtered), top = ops.transe_pair_relations(en, rn, s, o, p, target=target, k=k, **names)
    want_ranks, want_top = _twin(transe, en, rn, s, o, p, target, k, filt)
    assert torch.equal(raw, want_ranks[0]) and torch.equal(filtered, want_ranks[1]) and rc.same_lists(top, want_top)
    assert torch.equal(raw, raw0)                                         # count_raw with and without a filter
    assert top[0].dtype == torch.int64 and top[0].shape == (s.numel(), k) and top[1].dtype == torch.float32
    ranks_only, no_top = ops.transe_pair_relations(en, rn, s, o, p, target=target, **names)
    no_ranks, top_only = ops.transe_pair_relations(en, rn, s, o, p, k=k, **names)
    assert no_top is None and no_ranks is None
    assert torch.equal(ranks_only[0], raw) and torch.equal(ranks_only[1], filtered) and rc.same_lists(top_only, top)
    left = rn.shape[0] - (filt[1] - filt[0])                              # relations left per row: the rest is padding
    pos = torch.arange(k, device=top[0].device).view(1, -1)
    assert torch.equal(top[0] < 0, pos >= left.view(-1, 1)) and bool((top[1][top[0] < 0] == float('inf')).all())
    return raw, filtered, top


@pytest.mark.parametrize('p', [1, 2])
@pytest.mark.parametrize('m,num_rels,dim,k', rc.SHAPES)
def test_fused_equals_the_twin(ops, transe, m, num_rels, dim, k, p):
    gen = torch.Generator().manual_seed(m * 7 + num_rels + dim + k + p)
    en, rn = _tables(num_rels, dim, gen)
    s, o = rc.pairs(m, gen)
    target = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    _check_all_forms(ops, transe, en, rn, s, o, p, target, k)
    empty = ops.transe_pair_relations(en, rn, s[:0], o[:0], p, target=target[:0], k=k)
    assert empty[0][0].shape == (0,) and empty[1][0].shape == (0, k)


@pytest.mark.parametrize('p', [1, 2])
def test_ties_nan_inf_and_zero(ops, transe, p):
    num_rels, dim, m = 128, 24, 65                 # two exact tiles: the k = 128 lists hold every relation
    gen = torch.Generator().manual_seed(3 + p)
    en, rn = _tables(num_rels, dim, gen)
    rn[70] = rn[3]                                 # two identical relation rows, across the tile boundary
    rn[9] = rn[5]; rn[127] = rn[5]                 # three
    rn[20] = float('nan')
    rn[100] = float('inf')                         # distance +inf: after every number, before the NaN
    rn[64] = en[11] - en[10]                       # the pair (10, 11) is at distance +0 from relation 64
    s, o = rc.pairs(m, gen)
    s[2], o[2] = 10, 11
    target = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    target[:7] = torch.tensor([3, 70, 5, 9, 127, 20, 100]).cuda()
    for k in (1, 10, 128):
        raw, _, top = _check_all_forms(ops, transe, en, rn, s, o, p, target, k)
    ids, dist = ops.transe_pair_relations(en, rn, s, o, p, k=128)[1]
    for row in ids.tolist():
        assert row.index(3) + 1 == row.index(70) and row.index(5) + 1 == row.index(9) and row.index(9) + 1 == row.index(127)
    assert ids[:, -2:].tolist() == [[100, 20]] * m and bool((dist[:, -2] == float('inf')).all())
    assert dist[:, -1].view(torch.int32).tolist() == [0x7fc00000] * m
    assert ids[2, 0] == 64 and dist[2, :1].view(torch.int32).tolist() == [0]                   # +0
    full = ops.transe_pair_relations(en, rn, s[:1].repeat(5), o[:1].repeat(5), p, target=torch.tensor([3, 70, 5, 9, 127]).cuda())[0][0]
    assert full[0] == full[1] and full[2] == full[3] == full[4] and full[0] % 1 == 0.5 and full[2] % 1 == 0.0
    assert raw[5] == num_rels - 1                                         # a NaN target ranks last


def test_chunked_equals_unchunked_and_the_report(transe, monkeypatch):
    from gcn_vae_amd import ranking
    m, num_rels, dim, k = 130, 65, 16, 10
    gen = torch.Generator().manual_seed(11)
    ent, rel = _tables(num_rels, dim, gen)
    s, o = rc.pairs(m, gen)
    r = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    trip = torch.stack([s, r, o], 1)
    known = torch.cat([trip, torch.stack([s, (r + 1) % num_rels, o], 1), torch.stack([s, (r + 64) % num_rels, o], 1)])
    pf = ranking.PairFilterIndex(rc.N, num_rels, known.cpu(), device='cuda')
    for tables in ((ent, rel, 1, True), (ent, rel, 2, False)):
        whole = (transe.rank_relations(tables, trip, pf), transe.predict_relations(tables, s, o, k, pf))
        twin = (transe.rank_relations_unfused(tables, trip, pf), transe.predict_relations_unfused(tables, s, o, k, pf))
        with monkeypatch.context() as mp:
            mp.setattr(transe, 'MAX_QUERY_ROWS', 64)
            parts = (transe.rank_relations(tables, trip, pf), transe.predict_relations(tables, s, o, k, pf))
        for got in (parts, twin):
            assert torch.equal(got[0][0], whole[0][0]) and torch.equal(got[0][1], whole[0][1]) and rc.same_lists(got[1], whole[1])
        assert not bool(((whole[1][0] == r.view(-1, 1)) & (whole[1][0] >= 0)).any())      # known relations are never proposed
        assert bool((whole[0][1] <= whole[0][0]).all())
        report = transe.evaluate_relations(tables, trip.cpu().numpy(), pf, verbose=False)
        assert report == transe.evaluate_relations(tables, trip.cpu().numpy(), pf, unfused=True, verbose=False)
        assert set(report) == {'mrr_raw', 'mr_raw', 'hits_raw', 'mrr_filtered', 'mr_filtered', 'hits_filtered'}
        assert report['mrr_filtered'] >= report['mrr_raw']
        assert set(transe.evaluate_relations(tables, trip.cpu().numpy(), verbose=False)) == {'mrr_raw', 'mr_raw', 'hits_raw'}


@pytest.mark.parametrize('p', [1, 2])
def test_distances_within_the_float64_bound(ops, p):
    """The reference is ||s + r - o||_p in float64 from the fp32 tables; with a_c = o_c - s_c and x_c = a_c - r_c (exact) the
    kernel forms q_c = fl(a_c) = a_c (1 + d1) and t_c = fl(q_c - r_c) = (x_c + a_c d1)(1 + d2), |d| <= u = 2^-24: two roundings
    of the difference, so e_c = t_c - x_c has |e_c| <= u (1 + u) |a_c| + u |x_c|.
    L1: |t_c| is exact and the h terms are added in h - 1 rounded additions (the first lands on 0), so
      |d^ - d| <= gamma(h - 1) sum |t_c| + sum |e_c| <= [gamma(h - 1) (1 + 2 u) + 2 u] (sum |a_c| + sum |x_c|)
               <= gamma(h + 2) (||a||_1 + ||x||_1).
    L2: each column is one fma (one rounding: S^ = sum t_c^2 (1 + theta_c), |theta_c| <= gamma(h)), then one correctly rounded
    square root: d^ = sqrt(S^) (1 + d3).  |sqrt(1 + theta) - 1| <= |theta|, so |sqrt(S^) - ||t||_2| <= gamma(h) ||t||_2, and
    | ||t||_2 - ||x||_2 | <= ||e||_2 <= u (1 + u) ||a||_2 + u ||x||_2.  Together
      |d^ - d| <= (gamma(h) + u (1 + gamma(h))) (||x||_2 + ||e||_2) + ||e||_2 <= gamma(h + 4) (||a||_2 + ||x||_2).
    The float64 reference's own error is 2^-29 of that and is ignored.  Every distance of every pair: the k = num_rels lists hold
    all of them."""
    m, num_rels, h = 130, 128, 200
    gen = torch.Generator().manual_seed(5 + p)
    en, rn = _tables(num_rels, h, gen)
    s, o = rc.pairs(m, gen)
    ids, dist = ops.transe_pair_relations(en, rn, s, o, p, k=num_rels)[1]
    assert bool((ids.sort(1).values == torch.arange(num_rels, device=ids.device)).all()) and bool(torch.isfinite(dist).all())
    a = en[o].double() - en[s].double()                                   # (m, h), exact in float64
    x = a.unsqueeze(1) - rn.double().unsqueeze(0)                         # (m, R, h) = -(s + r - o)
    exact = (en[s].double().unsqueeze(1) + rn.double().unsqueeze(0) - en[o].double().unsqueeze(1)).norm(p=p, dim=2)
    bound = rc.gamma(h + 2 if p == 1 else h + 4) * (a.norm(p=p, dim=1, keepdim=True) + x.norm(p=p, dim=2))
    err = (dist.double() - exact.gather(1, ids)).abs()
    ratio = float((err / bound.gather(1, ids)).max())
    print(f'p={p}: max |d - f64| / bound = {ratio:.4f}, max error {float(err.max()):.3e}')
    assert bool((err <= bound.gather(1, ids)).all())


def test_cli_reports_and_writes_relation_predictions(tmp_path, capsys, transe):
    from gcn_vae_amd import data
    kg = data.load_data(rc.CLI_SPEC)
    torch.manual_seed(0)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    ckpt, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'transe_rel.tsv')
    model.save_checkpoint(ckpt)
    res = transe.main(transe.build_parser().parse_args([
        '-d', rc.CLI_SPEC, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt, '--relation-eval', '--filtered-eval',
        '--predict-relations', str(rc.CLI_K), '--relations-out', out]))
    rel, text = res['relations'], capsys.readouterr().out
    assert set(rel) == {'mrr_raw', 'mr_raw', 'hits_raw', 'mrr_filtered', 'mr_filtered', 'hits_filtered'}
    assert rel['mrr_filtered'] >= rel['mrr_raw'] > 0
    for kind in ('raw', 'filtered'):
        assert f'Relation MRR ({kind}): ' in text and all(f'Relation Hits ({kind}) @ {h}: ' in text for h in (1, 3, 10))
    rows = rc.check_relation_tsv(out, kg, rc.CLI_K)                        # (the same key columns as train.py's file: see there)
    assert all(float(x[4]) >= 0 for x in rows)
