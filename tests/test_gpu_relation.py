"""Relation prediction on the GPU (gv_pair_rel_scores / ops.pair_relation_scores / ranking.rank_relations, predict_relations)
against the materialised twin: ops.gemm(ops.mul(E[s], E[o]), w^T) + bias, ranked by ranking.mid_ranks and ordered by
ranking.topk_from_scores.  Every comparison is exact: ids and ranks by torch.equal, values by their bits.  pytest -m gpu."""
import numpy as np
import pytest
import torch

import relation_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def ranking():
    from gcn_vae_amd import ranking as _ranking
    return _ranking


def _tables(num_rels, h, gen, pad=0):
    """(emb, w): with ``pad`` > 0 both are views of wider storage (leading dimension h + pad)."""
    emb = (torch.randn(rc.N, h + pad, generator=gen) * 0.5).cuda()[:, :h]
    w = torch.randn(num_rels, h + pad, generator=gen).cuda()[:, :h]
    return emb, w


def _twin(ranking, emb, w, s, o, target, k, bias=None, filt=(None, None, None)):
    score = ranking.pair_scores_unfused(emb, w, s, o, bias)
    return ranking.relation_ranks_from_scores(score, target, *filt), ranking.topk_from_scores(score, k, *filt)


def _check_all_forms(ops, ranking, emb, w, s, o, target, k, bias=None):
    """Fused == twin, with and without a filter; ranks only, top-k only and both in one call agree; count_raw does not depend on
    the filter."""
    gen = torch.Generator().manual_seed(int(target.sum()) + k)
    filt = rc.relation_lists(s.numel(), w.shape[0], target.cpu(), gen)
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    (raw0, none), top0 = ops.pair_relation_scores(emb, w, s, o, target=target, k=k, bias=bias)
    want_ranks, want_top = _twin(ranking, emb, w, s, o, target, k, bias)
    assert none is None and torch.equal(raw0, want_ranks[0]) and rc.same_lists(top0, want_top)
    (raw, filtered), top = ops.pair_relation_scores(emb, w, s, o, target=target, k=k, bias=bias, **names)
    want_ranks, want_top = _twin(ranking, emb, w, s, o, target, k, bias, filt)
    assert torch.equal(raw, want_ranks[0]) and torch.equal(filtered, want_ranks[1]) and rc.same_lists(top, want_top)
    assert torch.equal(raw, raw0)                                         # count_raw with and without a filter
    assert top[0].dtype == torch.int64 and top[0].shape == (s.numel(), k) and top[1].dtype == torch.float32
    ranks_only, no_top = ops.pair_relation_scores(emb, w, s, o, target=target, bias=bias, **names)
    no_ranks, top_only = ops.pair_relation_scores(emb, w, s, o, k=k, bias=bias, **names)
    assert no_top is None and no_ranks is None
    assert torch.equal(ranks_only[0], raw) and torch.equal(ranks_only[1], filtered) and rc.same_lists(top_only, top)
    left = w.shape[0] - (filt[1] - filt[0])                               # relations left per row: the rest is padding
    pos = torch.arange(k, device=top[0].device).view(1, -1)
    assert torch.equal(top[0] < 0, pos >= left.view(-1, 1)) and bool((top[1][top[0] < 0] == float('-inf')).all())
    return raw, filtered, top


@pytest.mark.parametrize('pad', [0, 4])
@pytest.mark.parametrize('m,num_rels,h,k', rc.SHAPES)
def test_fused_equals_the_twin(ops, ranking, m, num_rels, h, k, pad):
    gen = torch.Generator().manual_seed(m * 7 + num_rels + h + k)
    emb, w = _tables(num_rels, h, gen, pad)
    s, o = rc.pairs(m, gen)
    target = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    _check_all_forms(ops, ranking, emb, w, s, o, target, k)
    empty = ops.pair_relation_scores(emb, w, s[:0], o[:0], target=target[:0], k=k)
    assert empty[0][0].shape == (0,) and empty[1][0].shape == (0, k)


def test_ties_nan_inf_and_a_saturating_bias(ops, ranking):
    num_rels, h, m = 128, 24, 65                   # two exact tiles: the k = 128 lists hold every relation
    gen = torch.Generator().manual_seed(3)
    emb, w = _tables(num_rels, h, gen)
    w[70] = w[3]                                   # two identical relation rows, across the tile boundary
    w[9] = w[5]; w[127] = w[5]                     # three
    w[20] = float('nan')
    w[100] = float('inf')
    emb[7] = emb[7].abs() + 0.1                    # a pair whose product row is positive: logit +inf under relation 100, no NaN
    s, o = rc.pairs(m, gen)
    s[2], o[2] = 7, 7
    target = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    target[:6] = torch.tensor([3, 70, 5, 9, 127, 20]).cuda()
    target[6] = 100
    for k in (1, 10, 128):
        raw, _, top = _check_all_forms(ops, ranking, emb, w, s, o, target, k)
    ids, val = ops.pair_relation_scores(emb, w, s, o, k=128)[1]
    for row in ids.tolist():
        assert row.index(3) + 1 == row.index(70) and row.index(5) + 1 == row.index(9) and row.index(9) + 1 == row.index(127)
    # +inf first; NaN last and by id among themselves (a mixed-sign product row makes relation 100 inf - inf = NaN as well)
    assert ids[2, 0] == 100 and val[2, 0] == float('inf') and ids[2, -1] == 20
    mixed = [i for i in range(m) if i != 2 and bool(torch.isnan(val[i, -2]))]
    assert len(mixed) > m // 2 and all(ids[i, -2:].tolist() == [20, 100] for i in mixed)
    assert val[:, -1].view(torch.int32).tolist() == [0x7fc00000] * m
    # exact ties hit the mid-rank: the two rows of a tie group differ by nothing, the three by nothing
    full = ops.pair_relation_scores(emb, w, s[:1].repeat(5), o[:1].repeat(5), target=torch.tensor([3, 70, 5, 9, 127]).cuda())[0][0]
    assert full[0] == full[1] and full[2] == full[3] == full[4] and full[0] % 1 == 0.5 and full[2] % 1 == 0.0
    assert raw[5] == num_rels - 1                                         # a NaN target ranks last
    # a bias under which every sigmoid is 1.0f: the ranks are taken on the logit and stay those of the twin (not one big tie)
    bias = torch.tensor([64.0]).cuda()
    raw_b, _, top_b = _check_all_forms(ops, ranking, emb, w, s, o, target, 10, bias)
    finite = torch.isfinite(top_b[1])
    assert bool((torch.sigmoid(top_b[1][finite]) == 1.0).all())
    assert int((raw_b != (num_rels - 1) / 2).sum()) >= m - 2 and raw_b.unique().numel() > m // 4


def test_chunked_equals_unchunked(ranking, monkeypatch):
    m, num_rels, h, k = 130, 65, 16, 10
    gen = torch.Generator().manual_seed(11)
    emb, w = _tables(num_rels, h, gen)
    s, o = rc.pairs(m, gen)
    r = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    trip = torch.stack([s, r, o], 1)
    known = torch.cat([trip, torch.stack([s, (r + 1) % num_rels, o], 1), torch.stack([s, (r + 64) % num_rels, o], 1)])
    pf = ranking.PairFilterIndex(rc.N, num_rels, known.cpu(), device='cuda')
    bias = torch.tensor([0.25]).cuda()
    whole = (ranking.rank_relations(emb, w, trip, pf, bias), ranking.predict_relations(emb, w, s, o, k, pf, bias))
    twin = (ranking.rank_relations_unfused(emb, w, trip, pf, bias), ranking.predict_relations_unfused(emb, w, s, o, k, pf, bias))
    monkeypatch.setattr(ranking, 'MAX_QUERY_ROWS', 64)
    parts = (ranking.rank_relations(emb, w, trip, pf, bias), ranking.predict_relations(emb, w, s, o, k, pf, bias))
    for got in (parts, twin):
        assert torch.equal(got[0][0], whole[0][0]) and torch.equal(got[0][1], whole[0][1]) and rc.same_lists(got[1], whole[1])
    assert not bool(((whole[1][0] == r.view(-1, 1)) & (whole[1][0] >= 0)).any())          # known relations are never proposed
    assert bool((whole[0][1] <= whole[0][0]).all())
    report = ranking.calc_relation_mrr(emb, w, trip, pf, flow_log_prob=bias, verbose=False)
    again = ranking.calc_relation_mrr_unfused(emb, w, trip, pf, flow_log_prob=bias, verbose=False)
    assert report == again and set(report) == {'mrr_raw', 'hits_raw', 'mrr_filtered', 'hits_filtered'}
    assert set(ranking.calc_relation_mrr(emb, w, trip, verbose=False)) == {'mrr_raw', 'hits_raw'}
    # the drivers check a whole query set once (the chunks pass ids_checked=True): a bad id anywhere is refused before any launch
    bad = trip.clone()
    bad[100, 2] = rc.N
    for fn in (ranking.rank_relations, ranking.rank_relations_unfused):
        with pytest.raises(ValueError, match='pair entities must lie in'):
            fn(emb, w, bad, pf)
    bad = trip.clone()
    bad[100, 1] = num_rels
    with pytest.raises(ValueError, match='targets must lie in'):
        ranking.rank_relations(emb, w, bad, pf)
    with pytest.raises(ValueError, match='pair entities must lie in'):
        ranking.predict_relations(emb, w, s, o.clone().fill_(-1), k, pf)
    with pytest.raises(ValueError, match='pair_filter was built for'):
        ranking.rank_relations(emb, w[:-1], trip % (num_rels - 1), pf)


def test_logits_within_the_float64_bound(ops):
    """|logit - f64| <= gamma(h + 1) * sum_d |e[s, d] e[o, d] w[r, d]|, gamma(j) = j u / (1 - j u), u = 2^-24: one rounding for
    the product e[s, d] * e[o, d], and at most h for the chain of h multiply-adds into the accumulator, whatever order the MFMA
    takes them in (h - 1 additions and the products, which the MFMA may or may not round on their own: h covers both).  The float64
    reference's own error is 2^-29 of that and is ignored.  Every logit of every pair: the k = num_rels lists hold all of them."""
    m, num_rels, h = 130, 128, 200
    gen = torch.Generator().manual_seed(5)
    emb, w = _tables(num_rels, h, gen)
    s, o = rc.pairs(m, gen)
    ids, val = ops.pair_relation_scores(emb, w, s, o, k=num_rels)[1]
    assert bool((ids.sort(1).values == torch.arange(num_rels, device=ids.device)).all()) and bool(torch.isfinite(val).all())
    q = emb[s].double() * emb[o].double()
    exact = q @ w.double().T
    bound = rc.gamma(h + 1) * (q.abs() @ w.double().abs().T)
    err = (val.double() - exact.gather(1, ids)).abs()
    ratio = float((err / bound.gather(1, ids)).max())
    print(f'max |logit - f64| / bound = {ratio:.4f}, max error {float(err.max()):.3e}')
    assert bool((err <= bound.gather(1, ids)).all())


def test_cli_reports_and_writes_relation_predictions(tmp_path, capsys):
    from gcn_vae_amd import data, train
    from gcn_vae_amd.encoders import KGVAE
    kg = data.load_data(rc.CLI_SPEC)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt, out = str(tmp_path / 'm.pth'), str(tmp_path / 'rel.tsv')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    train.main(train.build_parser().parse_args([
        '-d', rc.CLI_SPEC, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1', '--mog-k', '4', '--n-flows', '2',
        '--test-mode', 'True', '--model-state-file', ckpt, '--relation-eval', '--filtered-eval', '--predict-relations', str(rc.CLI_K),
        '--relations-out', out]))
    text = capsys.readouterr().out
    mrr = {}
    for kind in ('raw', 'filtered'):
        line = next(x for x in text.splitlines() if x.startswith(f'Relation MRR ({kind}): '))
        mrr[kind] = float(line.split(': ')[1])
        assert all(f'Relation Hits ({kind}) @ {h}: ' in text for h in (1, 3, 10))
    assert mrr['filtered'] >= mrr['raw'] > 0
    rows = rc.check_relation_tsv(out, kg, rc.CLI_K)
    assert all(np.isfinite(float(x[4])) or int(x[3]) < 0 for x in rows)
