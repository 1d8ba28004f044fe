"""Type-constrained whole-graph mining on the GPU (gv_mine_scores_typed / ops.mine_scores_typed / ranking.mine_triplets(...,
type_constraint=) / --complete-typed) against the definition: mine_cases.brute_force on the materialised logits (ops.mul +
ops.gemm per relation at full (R, N, N)) with the known and the type-incorrect triplets excluded, and against the existing
unconstrained kernel.  Every comparison is exact: triplets, logits as bit patterns, counts.  pytest -m gpu."""
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


def _materialise(ops, emb, w, bias=None):
    """score[r, s, o], by the expression that defines the logit."""
    emb = emb.contiguous()
    out = torch.stack([ops.gemm(ops.mul(emb, w[r].expand_as(emb).contiguous()), emb, trans_b=True, precision='f32')
                       for r in range(w.shape[0])])
    return out if bias is None else out + bias


def _tables(n, h, num_rels, seed, scale=0.5):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(n, h, generator=gen) * scale).cuda(), torch.randn(num_rels, h, generator=gen).cuda(), gen


@pytest.mark.parametrize('n,h,num_rels', [(1, 1, 1), (7, 5, 2), (65, 37, 3), (130, 200, 4), (130, 500, 2)])
def test_typed_mining_equals_the_definition(ops, n, h, num_rels):
    """One tile, a tile edge, the resident width (h = 200) and the chunked path (h = 500); member lists of 0, 1, 63, 64, 65 and n
    entities, relation 0 with both sets full; no filter, a sparse and a dense one; bias and exclude_self on and off."""
    emb, w, gen = _tables(n, h, num_rels, n * 7 + h + num_rels)
    cs, co = member_masks(n, num_rels, gen)
    ptr, ids = member_lists(cs, co)
    plain = _materialise(ops, emb, w)
    filters = [None, _lists(n * num_rels, n, gen, dense=False), _lists(n * num_rels, n, gen, dense=True)]
    for flp in (None, 0.25):
        bias = None if flp is None else torch.tensor(flp, device='cuda')
        score = plain if bias is None else plain + bias
        for filt in filters:
            excl = excluded(cs, co, filt)
            f = {} if filt is None else dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filt))
            for exclude_self in (True, False):
                oracle = Oracle(score, False, excl, exclude_self)
                check_against(oracle, lambda **sel: ops.mine_scores_typed(emb, w, ptr, ids, bias=bias, exclude_self=exclude_self,
                                                                          **f, **sel),
                              thresholds=(float('-inf'), float('inf'), 0.0))


def test_against_the_unconstrained_kernel(ops):
    """gv_mine_scores at threshold -inf returns every candidate; filtered on the host with TypeConstraint.contains its first K and
    the count at the K-th value are the typed route's, bit for bit.  With all sets full the two routes agree outright."""
    from gcn_vae_amd import ranking
    n, h, num_rels = 130, 64, 4
    emb, w, gen = _tables(n, h, num_rels, 77)
    known = torch.stack([torch.randint(0, n, (900,), generator=gen), torch.randint(0, num_rels, (900,), generator=gen),
                         torch.randint(0, n, (900,), generator=gen)], 1)
    tc = ranking.TypeConstraint(n, num_rels, known[:300], device='cuda')
    fi = ranking.FilterIndex(n, num_rels, known, device='cuda')
    lo, hi, ent = ranking._mine_filter(fi, n, num_rels, emb.device)
    f = dict(filt_lo=lo, filt_hi=hi, filt_ent=ent)
    trip, logits, _ = ops.mine_scores(emb, w, threshold=float('-inf'), **f)
    keep = tc.contains(trip[:, 1], trip[:, 0], 's') & tc.contains(trip[:, 1], trip[:, 2], 'o')
    trip, logits = trip[keep], logits[keep]
    assert 1000 < trip.shape[0] < n * num_rels * n
    ptr, ids = tc.members('cuda')
    for k in (1, 10, 1000, trip.shape[0], trip.shape[0] + 1):
        got = ops.mine_scores_typed(emb, w, ptr, ids, k=k, **f)
        m = min(k, trip.shape[0])
        assert torch.equal(got[0], trip[:m]) and torch.equal(got[1].view(torch.int32), logits[:m].view(torch.int32))
        assert got[2]['count'] == int((logits >= logits[m - 1]).sum())
    full = ranking.TypeConstraint(n, num_rels, torch.stack([torch.arange(n).repeat(num_rels), torch.arange(num_rels).repeat_interleave(n),
                                                            torch.arange(n).repeat(num_rels)], 1), device='cuda')
    ptr, ids = full.members('cuda')
    for sel in (dict(k=1), dict(k=5000), dict(threshold=2.0), dict(threshold=float('-inf'))):
        for exclude_self in (True, False):
            assert _same(ops.mine_scores_typed(emb, w, ptr, ids, exclude_self=exclude_self, **f, **sel),
                         ops.mine_scores(emb, w, exclude_self=exclude_self, **f, **sel))
    # how the object tiles are grouped into spans does not change the result
    emb3, w3, gen3 = _tables(300, 24, 3, 78)
    cs, co = member_masks(300, 3, gen3, lengths=[(None, None), (200, 290), (65, 130)])
    ptr, ids = member_lists(cs, co)
    want = ops.mine_scores_typed(emb3, w3, ptr, ids, k=2000, span=1)
    for span in (2, 3, 8, None):
        assert _same(ops.mine_scores_typed(emb3, w3, ptr, ids, k=2000, span=span), want)


def test_ties_and_the_refining_passes(ops):
    from gcn_vae_amd import ranking
    # all-ones tables: every type-correct candidate ties, K lands inside the tie, the count is that of the whole tie
    n, num_rels = 100, 2
    ones, w1 = torch.ones(n, 8, device='cuda'), torch.ones(num_rels, 8, device='cuda')
    cs, co = member_masks(n, num_rels, torch.Generator().manual_seed(1), lengths=[(70, 65), (64, None)])
    ptr, ids = member_lists(cs, co)
    want = [(s, r, o) for s in range(n) for r in range(num_rels) for o in range(n) if s != o and cs[r, s] and co[r, o]]
    trip, logits, info = ops.mine_scores_typed(ones, w1, ptr, ids, k=300)
    assert [tuple(x) for x in trip.tolist()] == want[:300] and bool((logits == 8).all()) and info['count'] == len(want)
    with pytest.raises(ops.MineOverflow) as err:
        ops.mine_scores_typed(ones, w1, ptr, ids, k=300, max_results=len(want) - 1)
    assert err.value.count == len(want)
    assert ops.mine_scores_typed(ones, w1, ptr, ids, k=10 ** 6)[0].shape == (len(want), 3)
    # every logit in [16, 17): one bin of the first histogram, so a small cap forces the second and third levels
    gen = torch.Generator().manual_seed(3)
    n, num_rels, h, k = 300, 2, 16, 1000
    emb = (1.0 + 0.01 * torch.rand(n, h, generator=gen)).cuda()
    w = torch.ones(num_rels, h, device='cuda')
    cs, co = member_masks(n, num_rels, gen, lengths=[(None, None), (130, 200)])
    ptr, ids = member_lists(cs, co)
    score = _materialise(ops, emb, w)
    want = ranking.mine_from_scores(score, k=k, cand_subj=cs.cuda(), cand_obj=co.cuda())
    got = ops.mine_scores_typed(emb, w, ptr, ids, k=k, max_results=5000)
    assert got[2]['passes'] > 2 and _same(got, want)
    roomy = ops.mine_scores_typed(emb, w, ptr, ids, k=k)
    assert roomy[2]['passes'] == 2 and _same(roomy, want)
    tight = ops.mine_scores_typed(emb, w, ptr, ids, k=k, max_results=want[2]['count'])
    assert tight[2]['passes'] > 2 and _same(tight, want)


def test_special_values_inside_and_outside_the_member_lists(ops):
    n, h, num_rels = 130, 8, 2
    emb, w, gen = _tables(n, h, num_rels, 5)
    cs, co = member_masks(n, num_rels, gen, lengths=[(65, 70), (64, 65)])
    special = {'nan_in': 3, 'nan_out': 4, 'inf': 5, 'ninf': 6, 'zero': 7, 'nzero': 8}
    cs[:, [3, 5, 6, 7, 8]] = True
    co[:, [3, 5, 6, 7, 8]] = True
    cs[:, 4] = False
    co[:, 4] = False
    ptr, ids = member_lists(cs, co)
    base = ops.mine_scores_typed(emb, w, ptr, ids, threshold=float('-inf'))
    poisoned = emb.clone()
    poisoned[special['nan_out']] = float('nan')
    assert _same(ops.mine_scores_typed(poisoned, w, ptr, ids, threshold=float('-inf')), base)      # a NaN row outside every set
    emb = poisoned
    emb[special['nan_in']] = float('nan')
    emb[special['inf']] = 0.0
    emb[special['inf'], 0] = float('inf')
    emb[special['ninf']] = 0.0
    emb[special['ninf'], 0] = float('-inf')
    emb[special['zero']] = 0.0
    emb[special['nzero']] = -0.0
    score = _materialise(ops, emb, w)
    oracle = Oracle(score, False, excluded(cs, co), True)
    check_against(oracle, lambda **sel: ops.mine_scores_typed(emb, w, ptr, ids, **sel), ks=(1, 10, 3000),
                  thresholds=(float('-inf'), float('inf'), 0.0, -0.0))
    got = ops.mine_scores_typed(emb, w, ptr, ids, threshold=0.0)
    zero = got[1] == 0
    assert int(zero.sum()) > 0 and not bool(torch.signbit(got[1][zero]).any())                     # -0 is reported as +0
    assert not bool(torch.isnan(got[1]).any())
    assert not bool(((got[0][:, 0] == special['nan_in']) | (got[0][:, 2] == special['nan_in'])).any())


def test_strided_tables(ops):
    gen = torch.Generator().manual_seed(9)
    base_e, base_w = torch.randn(300, 50, generator=gen).cuda(), torch.randn(6, 50, generator=gen).cuda()
    emb, w = base_e[::2, 3:40], base_w[::2, 5:42]            # ld > h, odd width, bases that are not 16-byte aligned
    n, num_rels = emb.shape[0], w.shape[0]
    cs, co = member_masks(n, num_rels, gen)
    ptr, ids = member_lists(cs, co)
    oracle = Oracle(_materialise(ops, emb.contiguous(), w.contiguous()), False, excluded(cs, co), True)
    check_against(oracle, lambda **sel: ops.mine_scores_typed(emb, w, ptr, ids, **sel), ks=(1, 333), thresholds=(2.0,))


def test_empty_results(ops):
    emb, w, gen = _tables(70, 12, 3, 2)
    nobody = torch.zeros(3, 70, dtype=torch.bool)
    cs, co = member_masks(70, 3, gen)
    for masks in ((nobody, nobody), (cs, nobody), (nobody, co)):
        ptr, ids = member_lists(*masks)
        for sel in (dict(k=5), dict(threshold=float('-inf'))):
            got = ops.mine_scores_typed(emb, w, ptr, ids, **sel)
            assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2] == {'count': 0, 'passes': 0}        # no launch
    ptr, ids = member_lists(cs, co)
    got = ops.mine_scores_typed(emb, w, ptr, ids, threshold=1e30)
    assert got[0].shape == (0, 3) and got[2]['count'] == 0
    got = ops.mine_scores_typed(emb, w, ptr, ids, threshold=float('inf'))
    assert got[0].shape == (0, 3) and got[2]['count'] == 0
    none = ops.mine_scores_typed(emb[:0], w, torch.zeros(7, dtype=torch.int64, device='cuda'),
                                 torch.zeros(0, dtype=torch.int32, device='cuda'), k=5)
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2]['count'] == 0
    with pytest.raises(ValueError):                            # a bad id never reaches a launch, on the device either
        ops.mine_scores_typed(emb, w, ptr, torch.where(ids == ids.max(), 70, ids), k=5)


def test_wrappers_fused_equals_unfused():
    from gcn_vae_amd import data, ranking
    kg = data.load_data('synthetic:300:7:2000:100:100')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    emb, w, _ = _tables(kg.num_nodes, 32, kg.num_rels, 4)
    flp = torch.tensor(0.3, device='cuda')
    for sel in (dict(k=1), dict(k=500), dict(k=10 ** 7), dict(threshold=1.0)):
        for kw in (dict(filter_index=fi, flow_log_prob=flp), dict(exclude_self=False)):
            got = ranking.mine_triplets(emb, w, type_constraint=tc, **sel, **kw)
            assert _same(got, ranking.mine_triplets_unfused(emb, w, type_constraint=tc, **sel, **kw))
            assert bool((tc.contains(got[0][:, 1], got[0][:, 0], 's') & tc.contains(got[0][:, 1], got[0][:, 2], 'o')).all())
    with pytest.raises(ValueError, match='TypeConstraint'):
        ranking.mine_triplets(emb[:-1], w, k=3, type_constraint=tc)


def test_cli_writes_type_correct_completions(tmp_path):
    from gcn_vae_amd import data, ranking, train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:300:7:2000:100:100'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0, use_cuda=True,
                            reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda().eval()
    ckpt, out = str(tmp_path / 'm.pth'), str(tmp_path / 'typed.tsv')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                            '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file', ckpt,
                                            '--complete-topk', '200', '--complete-typed', '--complete-out', out])
    train.main(args)
    rows = np.array([[int(x) for x in line.split('\t')[:4]] for line in open(out)])
    assert rows.shape == (200, 4) and rows[:, 3].tolist() == list(range(200))
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test)
    s, r, o = (torch.from_numpy(rows[:, i]) for i in range(3))
    assert bool(tc.contains(r, s, 's').all()) and bool(tc.contains(r, o, 'o').all())
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    assert all(tuple(x[:3]) not in known and x[0] != x[2] for x in rows.tolist())


def test_fb15k237_size_fused_equals_unfused_and_times(capsys):
    """FB15k-237-synthetic size, h = 200, K = 100 000, sets and filter from train + valid + test: exact agreement of the two typed
    routes; the times are printed, no ratio is asserted."""
    import time
    from gcn_vae_amd import data, ranking
    kg = data.load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    gen = torch.Generator().manual_seed(5)
    emb = (torch.randn(kg.num_nodes, 200, generator=gen) * 0.3).cuda()
    w = torch.randn(kg.num_rels, 200, generator=gen).cuda()
    times = {}
    for name, fn in (('fused', ranking.mine_triplets), ('unfused', ranking.mine_triplets_unfused)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        times[name] = fn(emb, w, k=100000, filter_index=fi, type_constraint=tc)
        torch.cuda.synchronize()
        times[name + '_s'] = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\ntyped DistMult mining, FB15k-237-synthetic, h=200, K=100000 (first call each): fused {times['fused_s'] * 1e3:.1f} ms, "
              f"unfused {times['unfused_s'] * 1e3:.1f} ms")
    assert times['fused'][0].shape == (100000, 3) and _same(times['fused'], times['unfused'])
