"""Whole-graph triplet mining on the GPU (gv_mine_scores / ops.mine_scores / ranking.mine_triplets / generate.sample_graph)
against the rule stated on materialised logits: the same f32 product (ops.mul + ops.gemm per relation), selected by
ranking.mine_from_scores.  Every comparison is exact: triplets equal, logits equal as bit patterns.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from mine_cases import _lists, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def _materialise(ops, emb, w, bias=None):
    """score[r, s, o], by the expression that defines the logit."""
    emb = emb.contiguous()
    out = torch.stack([ops.gemm(ops.mul(emb, w[r].expand_as(emb).contiguous()), emb, trans_b=True, precision='f32')
                       for r in range(w.shape[0])])
    return out if bias is None else out + bias


def _tables(n, h, num_rels, seed, scale=0.5):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, h, generator=gen) * scale).cuda(), torch.randn(num_rels, h, generator=gen).cuda(), gen


@pytest.mark.parametrize('n,h,num_rels,flp', [(1, 1, 1, None), (7, 5, 2, 0.25), (64, 37, 9, None), (65, 200, 2, -1.5), (65, 500, 1, None),
                                              (777, 37, 2, 3.0), (777, 200, 9, None), (777, 500, 2, 0.5), (3001, 5, 9, None),
                                              (3001, 200, 2, -0.75), (3001, 1, 1, None), (7, 500, 9, None), (64, 1, 2, 1.0)])
def test_mining_equals_the_definition(ops, n, h, num_rels, flp):
    from gcn_vae_amd import ranking
    emb, w, gen = _tables(n, h, num_rels, n * 7 + h + num_rels)
    bias = None if flp is None else torch.tensor(flp, device='cuda')
    score = _materialise(ops, emb, w, bias)
    lo, hi, ent = _lists(n * num_rels, n, gen, dense=n <= 65)
    for filt in ({}, dict(filt_lo=lo, filt_hi=hi, filt_ent=ent)):
        for exclude_self in (True, False):
            kw = dict(exclude_self=exclude_self, **filt)
            everything = ranking.mine_from_scores(score, threshold=float('-inf'), max_results=2 ** 31 - 1, **kw)[1]
            for k in sorted({1, 10, 1000, max(1, min(everything.numel() // 3, 50000))}):
                got = ops.mine_scores(emb, w, k=k, bias=bias, **kw)
                assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (min(k, everything.numel()), 3)
                assert _same(got, ranking.mine_from_scores(score, k=k, **kw)), (k, exclude_self, bool(filt))
            cuts = [float('inf')] + ([0.0, float('-inf')] if everything.numel() <= 200000 else [])
            if everything.numel():
                cuts += [float(everything[min(everything.numel() - 1, 500)]), float(everything[min(everything.numel() - 1, 20000)])]
            for t in cuts:
                got = ops.mine_scores(emb, w, threshold=t, bias=bias, **kw)
                assert _same(got, ranking.mine_from_scores(score, threshold=t, **kw)), (t, exclude_self, bool(filt))
                assert got[2]['passes'] == 1
    if n == 3001 and h == 200:                    # threshold -inf: everything but NaN, and the count is the whole product
        got = ops.mine_scores(emb[:300], w, threshold=float('-inf'), exclude_self=False)
        assert got[2]['count'] == 300 * num_rels * 300 == got[0].shape[0]


def test_ties_nan_inf_and_signed_zero(ops):
    from gcn_vae_amd import ranking
    h, n, num_rels = 8, 1300, 3
    gen = torch.Generator().manual_seed(0)
    emb = torch.randn(n, h, generator=gen).cuda()
    w = torch.randn(num_rels, h, generator=gen).cuda()
    for j in (7, 70, 130, 200, 299, 1000, 1299):             # exact ties across tiles
        emb[j] = emb[3]
    emb[10] = float('nan')
    emb[250] = float('nan')
    emb[20] = 0.0                                            # logits +0 and -0
    emb[21] = -0.0
    emb[40] = 0.0
    emb[40, 0] = float('inf')                                # +-inf logits, NaN against a zero
    emb[41] = 0.0
    emb[41, 0] = float('-inf')
    w[1] = 1.0                                               # relation 1: logit = e_s . e_o, symmetric ties
    score = _materialise(ops, emb, w)
    for k in (1, 10, 5000, 200000):
        assert _same(ops.mine_scores(emb, w, k=k), ranking.mine_from_scores(score, k=k))
    for t in (float('inf'), 0.0, -0.0, 3.5):
        got = ops.mine_scores(emb, w, threshold=t)
        assert _same(got, ranking.mine_from_scores(score, threshold=t))
        assert not bool(torch.isnan(got[1]).any())
    got = ops.mine_scores(emb, w, threshold=0.0)
    zero = got[1] == 0
    assert int(zero.sum()) > 0 and not bool(torch.signbit(got[1][zero]).any())          # -0 == +0, reported as +0
    assert bool((got[0][:, 0] != got[0][:, 2]).all())
    assert not bool(((got[0][:, 0] == 10) | (got[0][:, 2] == 250)).any())               # NaN is never emitted
    # an all-equal table: the first K triplets in (s, r, o) order; a cap below the tie block is the error, with its size
    ones, w1 = torch.ones(100, 8, device='cuda'), torch.ones(2, 8, device='cuda')
    trip, logits, info = ops.mine_scores(ones, w1, k=300)
    want = [(s, r, o) for s in range(100) for r in range(2) for o in range(100) if s != o][:300]
    assert [tuple(x) for x in trip.tolist()] == want and bool((logits == 8).all()) and info['count'] == 19800
    with pytest.raises(ops.MineOverflow) as err:
        ops.mine_scores(ones, w1, k=300, max_results=19799)
    assert err.value.count == 19800 and '19800' in str(err.value)
    assert ops.mine_scores(ones, w1, k=300, max_results=19800)[0].shape == (300, 3)
    assert ops.mine_scores(ones, w1, k=10 ** 6)[0].shape == (19800, 3)                   # K beyond the candidates: all of them


def test_dense_logits_take_the_refining_passes(ops):
    """Every logit in [16, 17): one bin of the first, 12-bit histogram (sign, exponent, three mantissa bits).  With a cap below that
    bin's population the threshold is narrowed by further histogram passes before anything is emitted."""
    from gcn_vae_amd import ranking
    gen = torch.Generator().manual_seed(3)
    n, num_rels, h, k = 300, 2, 16, 1000
    emb = (1.0 + 0.01 * torch.rand(n, h, generator=gen)).cuda()
    w = torch.ones(num_rels, h, device='cuda')
    score = _materialise(ops, emb, w)
    assert bool(((score >= 16) & (score < 17)).all())
    want = ranking.mine_from_scores(score, k=k)
    got = ops.mine_scores(emb, w, k=k, max_results=5000)
    assert got[2]['passes'] > 2 and _same(got, want)
    roomy = ops.mine_scores(emb, w, k=k)
    assert roomy[2]['passes'] == 2 and _same(roomy, want)                  # one histogram, one emission
    tight = ops.mine_scores(emb, w, k=k, max_results=want[2]['count'])     # down to the exact value of the K-th logit
    assert tight[2]['passes'] > 2 and _same(tight, want)


def test_topk_is_a_prefix_of_the_threshold_run_and_counts_are_exact(ops):
    from gcn_vae_amd import ranking
    emb, w, gen = _tables(900, 48, 4, 21)
    lo, hi, ent = _lists(900 * 4, 900, gen, dense=False)
    filt = dict(filt_lo=lo, filt_hi=hi, filt_ent=ent)
    bias = torch.tensor(0.4, device='cuda')
    k = 700
    trip, logits, info = ops.mine_scores(emb, w, k=k, bias=bias, **filt)
    t = float(logits[-1])
    trip_t, logits_t, info_t = ops.mine_scores(emb, w, threshold=t, bias=bias, **filt)
    assert torch.equal(trip_t[:k], trip) and torch.equal(logits_t[:k].view(torch.int32), logits.view(torch.int32))
    assert info['count'] == info_t['count'] == trip_t.shape[0]
    score = _materialise(ops, emb, w, bias)
    listed = ranking._listed_mask(lo, hi, ent, 900 * 4, 900, 'cuda').view(900, 4, 900).permute(1, 0, 2)
    score[listed] = float('nan')
    score[:, torch.arange(900), torch.arange(900)] = float('nan')
    for cut in (t, 0.0, 2.5):
        assert ops.mine_scores(emb, w, threshold=cut, bias=bias, **filt)[2]['count'] == int((score >= cut).sum())
    # overflow: the message's count is the true one
    true = int((score >= 2.5).sum())
    assert true > 10
    with pytest.raises(ops.MineOverflow) as err:
        ops.mine_scores(emb, w, threshold=2.5, bias=bias, max_results=true - 1, **filt)
    assert err.value.count == true and str(true) in str(err.value)
    with pytest.raises(ops.MineOverflow) as err:
        ops.mine_scores(emb, w, threshold=2.5, bias=bias, max_results=3, **filt)
    assert err.value.count == true
    assert ops.mine_scores(emb, w, threshold=2.5, bias=bias, max_results=true, **filt)[0].shape[0] == true


def test_row_and_width_stride(ops):
    from gcn_vae_amd import ranking
    gen = torch.Generator().manual_seed(9)
    base_e, base_w = torch.randn(300, 50, generator=gen).cuda(), torch.randn(6, 50, generator=gen).cuda()
    emb, w = base_e[::2, 3:40], base_w[::2, 5:42]            # non-contiguous rows, odd width, unaligned
    score = _materialise(ops, emb.contiguous(), w.contiguous())
    assert _same(ops.mine_scores(emb, w, k=333), ranking.mine_from_scores(score, k=333))
    assert _same(ops.mine_scores(emb, w, threshold=4.0), ranking.mine_from_scores(score, threshold=4.0))
    none = ops.mine_scores(emb[:0], w, k=5)
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2]['count'] == 0


def test_crosscheck_with_predict_topk(ops):
    """Every (s, r) group of the mined list is the head of that query's predict_topk list (same filter, same order, bit-equal
    logits).  predict_topk keeps s == o, so self triplets stay in here."""
    from gcn_vae_amd import ranking
    n, num_rels, h, k = 2500, 5, 64, 2000
    emb, w, gen = _tables(n, h, num_rels, 11, scale=1.0)
    trip_known = torch.stack([torch.randint(0, n, (4000,), generator=gen), torch.randint(0, num_rels, (4000,), generator=gen),
                              torch.randint(0, n, (4000,), generator=gen)], 1)
    fi = ranking.FilterIndex(n, num_rels, trip_known, device='cuda')
    flp = torch.tensor(0.75, device='cuda')
    trip, logits, _ = ranking.mine_triplets(emb, w, k=k, filter_index=fi, flow_log_prob=flp, exclude_self=False)
    assert trip.shape[0] == k
    group = trip[:, 0] * num_rels + trip[:, 1]
    keys, sizes = torch.unique(group, return_counts=True)
    assert int(sizes.max()) < 128                             # what makes the comparison with k = 128 lists complete
    ids, lg = ranking.predict_topk(emb, w, keys // num_rels, keys % num_rels, 128, direction='o', filter_index=fi, flow_log_prob=flp)
    for i, (key, size) in enumerate(zip(keys.tolist(), sizes.tolist())):
        mine = group == key                                   # the mined list is sorted: a group's members keep its order
        assert torch.equal(trip[mine, 2], ids[i, :size])
        assert torch.equal(logits[mine].view(torch.int32), lg[i, :size].view(torch.int32))


def test_full_fb15k237_size_against_the_unfused_path():
    """14 541 entities x 237 relations x 14 541 entities (5.0e10 triplets), h = 200, the 100 000 best new ones with the synthetic
    dataset's train + valid + test triplets filtered: the fused sweep equals the per-relation materialised one exactly."""
    from gcn_vae_amd import data, ranking
    kg = data.load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    gen = torch.Generator().manual_seed(5)
    emb = (torch.randn(kg.num_nodes, 200, generator=gen) * 0.3).cuda()
    w = torch.randn(kg.num_rels, 200, generator=gen).cuda()
    flp = torch.tensor(0.3, device='cuda')
    got = ranking.mine_triplets(emb, w, k=100000, filter_index=fi, flow_log_prob=flp)
    want = ranking.mine_triplets_unfused(emb, w, k=100000, filter_index=fi, flow_log_prob=flp)
    assert got[0].shape == (100000, 3) and _same(got, want)
    known = torch.from_numpy(np.concatenate([kg.train, kg.valid, kg.test])).cuda().long()
    lin = lambda t: (t[:, 0] * kg.num_rels + t[:, 1]) * kg.num_nodes + t[:, 2]
    assert not bool(torch.isin(lin(got[0]), lin(known)).any())
    assert bool((got[0][:, 0] != got[0][:, 2]).all())


def _model(n_flows, h=16, nodes=300, rels=7):
    from gcn_vae_amd import train
    from gcn_vae_amd.encoders import KGVAE
    torch.manual_seed(0)
    return train.LinkPredict(KGVAE, nodes, h, rels, num_bases=4, num_hidden_layers=1, dropout=0.0, use_cuda=True, reg_param=0.01,
                             kl_param=1e-3, mmd_param=0.0, k=4, n_flows=n_flows).cuda().eval()


@pytest.mark.parametrize('n_flows', [0, 2])
def test_sample_graph(n_flows):
    from gcn_vae_amd import generate, ranking
    net = _model(n_flows)
    z, trip, logits = generate.sample_graph(net, 150, k=400, seed=4)
    z2, trip2, logits2 = generate.sample_graph(net, 150, k=400, seed=4)
    assert torch.equal(z, z2) and torch.equal(trip, trip2) and torch.equal(logits.view(torch.int32), logits2.view(torch.int32))
    assert z.shape == (150, 16) and trip.shape == (400, 3)
    want = ranking.mine_triplets(z, net.w_relation, k=400)
    assert torch.equal(trip, want[0]) and torch.equal(logits.view(torch.int32), want[1].view(torch.int32))
    assert int(trip[:, [0, 2]].min()) >= 0 and int(trip[:, [0, 2]].max()) < 150
    assert int(trip[:, 1].min()) >= 0 and int(trip[:, 1].max()) < net.w_relation.shape[0] == 7
    assert not torch.equal(generate.sample_graph(net, 150, k=400, seed=5)[0], z)
    _, by_t, lg_t = generate.sample_graph(net, 150, threshold=float(logits[-1]), seed=4)
    assert torch.equal(by_t[:400], trip) and bool((lg_t >= logits[-1]).all())


def test_cli_writes_the_mined_completions(tmp_path, monkeypatch):
    from gcn_vae_amd import ranking, train
    spec = 'synthetic:300:7:2000:100:80:3'
    kg = __import__('gcn_vae_amd.data', fromlist=['load_data']).load_data(spec)
    net = _model(2, nodes=kg.num_nodes, rels=kg.num_rels)
    ckpt, out, sampled = str(tmp_path / 'm.pth'), str(tmp_path / 'done.tsv'), str(tmp_path / 'graph.tsv')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    seen = []
    real = ranking.mine_triplets

    def spy(embed, w, **kw):
        seen.append((embed.detach().clone(), w.detach().clone(), dict(kw)))
        return real(embed, w, **kw)
    monkeypatch.setattr(ranking, 'mine_triplets', spy)
    args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                            '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file', ckpt,
                                            '--complete-topk', '50', '--complete-out', out, '--sample-graph', '40',
                                            '--sample-topk', '25', '--sample-out', sampled])
    train.main(args)
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert len(rows) == 50 and len(seen) == 2
    embed, w, kw = seen[0]
    assert kw['k'] == 50 and kw['filter_index'] is not None and kw['flow_log_prob'] is not None
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    trip, logits, _ = real(embed, w, k=50, filter_index=fi, flow_log_prob=kw['flow_log_prob'])
    assert [[int(x[0]), int(x[1]), int(x[2])] for x in rows] == trip.tolist()
    assert [int(x[3]) for x in rows] == list(range(50))
    assert np.allclose([float(x[4]) for x in rows], logits.cpu().numpy(), rtol=1e-7, atol=0)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    assert all((int(x[0]), int(x[1]), int(x[2])) not in known and x[0] != x[2] for x in rows)
    graph = [line.rstrip('\n').split('\t') for line in open(sampled)]
    assert len(graph) == 25 and seen[1][0].shape == (40, 16) and 'filter_index' not in seen[1][2]
    assert all(0 <= int(x[0]) < 40 and 0 <= int(x[2]) < 40 and 0 <= int(x[1]) < kg.num_rels for x in graph)
