"""Type-correct completion on the Monte-Carlo posterior predictive on the GPU (gv_mine_scores_typed_mc / ops.mine_scores_typed_mc /
ranking.mine_triplets_mc / --mc-complete).

Exact checks: against the existing MC scorer (every pbar[s, r, o] taken from gv_topk_scores_mc's tile with k = n <= 128, then the
host rule ranking.mine_from_probs), span invariance, duplicated samples, S = 1 against the single-sample miner, saturation and
ties, the refining histogram passes, NaN / inf / out-of-range ids, strided stacks, empty results.  Beyond 128 entities the values
are held to the float64 definition within the bound of tests/test_gpu_mc_rank.py

    eps = mean_s(gamma (|q_s| . |e_s| + |bias_s|) / 4) + C_SIG u + S u,   gamma = (h + 2) u,  C_SIG = 4

and every selection to the host rule on the kernel's own emitted values.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from mine_cases import _lists, _same
from mine_typed_cases import member_lists, member_masks
from mine_mc_cases import candidates, dense_of, emit_through_the_c_entry, pbar64, pbar_from_topk, stack

pytestmark = pytest.mark.gpu

NINF = float('-inf')
# (subject members, object members) per relation: together 0, 1, 63, 64, 65 and n entities; relation 0 with both sets full
LENGTHS = {(1, 1, 1, 1): [(None, None)], (2, 7, 5, 2): [(None, None), (1, 0)], (3, 65, 37, 3): [(None, None), (0, 64), (65, 1)],
           (4, 128, 200, 3): [(None, None), (63, 65), (64, 1)], (2, 128, 500, 2): [(None, None), (65, 63)]}


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def ranking():
    from gcn_vae_amd import ranking as _ranking
    return _ranking


def _filt(f):
    return {} if f is None else dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), f))


@pytest.mark.parametrize('shape', sorted(LENGTHS))
def test_exact_against_the_existing_mc_scorer(ops, ranking, shape):
    """The mined pbar is gv_topk_scores_mc's out_prob bit for bit, so the host rule on that scorer's probabilities gives the
    miner's triplets, values (as bit patterns) and count: thresholds -inf, 0.5, 2.0; k of 1, a mid value, the candidate count and
    one more; bias on and off; no, a sparse and a dense filter; exclude_self on and off."""
    s, n, h, num_rels = shape
    z, w, bias, gen = stack(s, n, h, num_rels, sum(shape))
    cs, co = member_masks(n, num_rels, gen, lengths=LENGTHS[shape])
    ptr, ids = member_lists(cs, co)
    filters = [None, _lists(n * num_rels, n, gen, dense=False), _lists(n * num_rels, n, gen, dense=True)]
    for b in (None, bias):
        pbar = pbar_from_topk(ops, ranking, z, w, b)
        for filt in filters:
            for exclude_self in (True, False):
                kw = dict(exclude_self=exclude_self, **_filt(filt))
                host = dict(cand_subj=cs.cuda(), cand_obj=co.cuda(), **kw)
                everything = ranking.mine_from_probs(pbar, threshold=NINF, **host)
                total = everything[2]['count']
                assert total == int(candidates(cs, co, filt, exclude_self).sum())
                sels = [dict(threshold=NINF), dict(threshold=0.5), dict(threshold=2.0)]
                sels += [dict(k=k) for k in sorted({1, max(1, total // 2), max(1, total), total + 1})]
                for sel in sels:
                    got = ops.mine_scores_typed_mc(z, w, ptr, ids, bias=b, **kw, **sel)
                    assert _same(got, ranking.mine_from_probs(pbar, **host, **sel)), (b is not None, filt is not None, exclude_self, sel)


@pytest.mark.parametrize('shape', [(3, 300, 24, 3), (2, 200, 500, 2)])
def test_float64_bound_beyond_128_entities(ops, ranking, shape):
    """More than one tile per side, the resident and the chunked path: the emitted set is the definition's, every value within eps
    of the float64 pbar, every selection the host rule on the kernel's own values."""
    s, n, h, num_rels = shape
    z, w, bias, gen = stack(s, n, h, num_rels, sum(shape))
    cs, co = member_masks(n, num_rels, gen, lengths=[(None, None), (200, 290), (65, 130)])
    ptr, ids = member_lists(cs, co)
    filt = _lists(n * num_rels, n, gen, dense=False)
    kw = dict(bias=bias, **_filt(filt))
    got = ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=NINF, **kw)
    cand = candidates(cs, co, filt, True)
    emitted = torch.zeros_like(cand)
    emitted[got[0][:, 1].cpu(), got[0][:, 0].cpu(), got[0][:, 2].cpu()] = True
    assert got[0].shape[0] == int(cand.sum()) == got[2]['count'] and torch.equal(emitted, cand)
    ref, eps = pbar64(z, w, bias)
    t = got[0].cpu().numpy()
    err = np.abs(got[1].cpu().numpy().astype(np.float64) - ref[t[:, 1], t[:, 0], t[:, 2]]) / eps[t[:, 1], t[:, 0], t[:, 2]]
    print(f'typed MC miner {shape}: worst |pbar - pbar64| / eps {err.max():.3f} over {err.size} triplets')
    assert err.max() <= 1.0
    own = dense_of(got, n, num_rels)
    mid = float(got[1][got[1].numel() // 2])
    for sel in (dict(k=1), dict(k=1000), dict(k=got[0].shape[0] + 1), dict(threshold=mid), dict(threshold=0.9), dict(threshold=2.0)):
        assert _same(ops.mine_scores_typed_mc(z, w, ptr, ids, **kw, **sel), ranking.mine_from_probs(own, exclude_self=False, **sel)), sel


def test_span_invariance(ops):
    """How a relation's object tiles are grouped into units does not change the result -- nor does a span longer than the group of
    tiles whose accumulators a workgroup holds at once (16 tiles of a 10-tile list: two groups)."""
    z, w, bias, gen = stack(3, 300, 24, 3, 31)
    cs, co = member_masks(300, 3, gen, lengths=[(None, None), (200, 290), (65, 130)])
    ptr, ids = member_lists(cs, co)
    want = ops.mine_scores_typed_mc(z, w, ptr, ids, k=2000, bias=bias, span=1)
    assert want[0].shape == (2000, 3)
    for span in (2, 3, 8, None):
        assert _same(ops.mine_scores_typed_mc(z, w, ptr, ids, k=2000, bias=bias, span=span), want), span
    z, w, bias, gen = stack(2, 600, 8, 1, 32)
    cs, co = member_masks(600, 1, gen, lengths=[(70, None)])
    ptr, ids = member_lists(cs, co)
    want = ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=0.6, span=1)
    assert want[0].shape[0] > 1000
    for span in (8, 9, 16):
        assert _same(ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=0.6, span=span), want), span


def test_duplicated_samples(ops):
    """The same sample twice or four times: 2 p * 0.5 and 4 p * 0.25 are exact, so the bits are those of the one sample."""
    z, w, bias, gen = stack(1, 130, 40, 3, 41)
    cs, co = member_masks(130, 3, gen)
    ptr, ids = member_lists(cs, co)
    want = ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=NINF, bias=bias)
    assert want[0].shape[0] > 10000
    for times in (2, 4):
        assert _same(ops.mine_scores_typed_mc(z.repeat(times, 1, 1), w, ptr, ids, threshold=NINF, bias=bias.repeat(times)), want)


def test_one_sample_against_the_single_sample_miner(ops):
    """S = 1: the candidates are mine_scores_typed's, and over them pbar is non-decreasing in that miner's logit."""
    z, w, bias, gen = stack(1, 200, 200, 3, 51)
    cs, co = member_masks(200, 3, gen, lengths=[(None, None), (63, 65), (130, 64)])
    ptr, ids = member_lists(cs, co)
    filt = _filt(_lists(200 * 3, 200, gen, dense=False))
    prob = ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=NINF, bias=bias, **filt)
    logit = ops.mine_scores_typed(z[0], w, ptr, ids, threshold=NINF, bias=bias, **filt)
    assert prob[2]['count'] == logit[2]['count'] == prob[0].shape[0] > 10000

    def by_triplet(res):
        lin = (res[0][:, 0] * 3 + res[0][:, 1]) * 200 + res[0][:, 2]
        order = torch.argsort(lin)
        return lin[order], res[1][order]
    (lin_p, p), (lin_l, x) = by_triplet(prob), by_triplet(logit)
    assert torch.equal(lin_p, lin_l)
    assert bool((p[torch.argsort(x, stable=True)].diff() >= 0).all())


def test_saturation_and_ties(ops):
    """z = 3 * ones, h = 8, w = ones: every logit is (3 * 1) * 3 * 8 = 72 in every sample, 1 + exp(-72) rounds to 1, so pbar ==
    1.0f exactly and every type-correct candidate ties.  K inside the tie: (s, r, o) ascending, the count is the whole tie, and a
    cap one below it raises MineOverflow with the count."""
    n, num_rels = 100, 2
    z, w1 = 3.0 * torch.ones(3, n, 8, device='cuda'), torch.ones(num_rels, 8, device='cuda')
    cs, co = member_masks(n, num_rels, torch.Generator().manual_seed(1), lengths=[(70, 65), (64, None)])
    ptr, ids = member_lists(cs, co)
    want = [(s, r, o) for s in range(n) for r in range(num_rels) for o in range(n) if s != o and cs[r, s] and co[r, o]]
    trip, probs, info = ops.mine_scores_typed_mc(z, w1, ptr, ids, k=300)
    assert [tuple(x) for x in trip.tolist()] == want[:300] and info['count'] == len(want)
    assert torch.equal(probs.view(torch.int32), torch.ones(300, device='cuda').view(torch.int32))
    with pytest.raises(ops.MineOverflow) as err:
        ops.mine_scores_typed_mc(z, w1, ptr, ids, k=300, max_results=len(want) - 1)
    assert err.value.count == len(want)
    assert ops.mine_scores_typed_mc(z, w1, ptr, ids, k=10 ** 6)[0].shape == (len(want), 3)
    assert ops.mine_scores_typed_mc(z, w1, ptr, ids, threshold=1.0)[2]['count'] == len(want)


def test_the_refining_passes(ops, ranking):
    """All-positive tables: every pbar lies in [0.5, 1), here within one bin of the first histogram (logits in [0.16, 0.164), pbar
    in [0.539, 0.541): sign, exponent and three mantissa bits shared), so a small cap forces the second and third levels."""
    gen = torch.Generator().manual_seed(3)
    s, n, num_rels, h, k = 3, 300, 2, 16, 1000
    z = (0.1 * (1.0 + 0.01 * torch.rand(s, n, h, generator=gen))).cuda()
    w = torch.ones(num_rels, h, device='cuda')
    cs, co = member_masks(n, num_rels, gen, lengths=[(None, None), (130, 200)])
    ptr, ids = member_lists(cs, co)
    everything = ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=NINF)
    assert 0.5 <= float(everything[1].min()) and float(everything[1].max()) < 0.5625
    want = ranking.mine_from_probs(dense_of(everything, n, num_rels), k=k, exclude_self=False)
    got = ops.mine_scores_typed_mc(z, w, ptr, ids, k=k, max_results=5000)
    assert got[2]['passes'] > 2 and _same(got, want)
    roomy = ops.mine_scores_typed_mc(z, w, ptr, ids, k=k)
    assert roomy[2]['passes'] == 2 and _same(roomy, want)
    tight = ops.mine_scores_typed_mc(z, w, ptr, ids, k=k, max_results=want[2]['count'])
    assert tight[2]['passes'] > 2 and _same(tight, want)


def test_nan_inf_and_ids_outside_the_table(ops):
    s, n, h, num_rels = 2, 130, 8, 2
    z, w, _, gen = stack(s, n, h, num_rels, 61, bias=False)
    cs, co = member_masks(n, num_rels, gen, lengths=[(65, 70), (64, 65)])
    cs[:, [3, 5, 6]] = True
    co[:, [3, 5, 6]] = True
    ptr, ids = member_lists(cs, co)
    # a NaN in ONE sample of entity 3's row: no triplet touches 3, the others are what they are without it in the lists
    poisoned = z.clone()
    poisoned[1, 3, 2] = float('nan')
    got = ops.mine_scores_typed_mc(poisoned, w, ptr, ids, threshold=NINF)
    assert not bool(torch.isnan(got[1]).any()) and not bool(((got[0][:, 0] == 3) | (got[0][:, 2] == 3)).any())
    cs3, co3 = cs.clone(), co.clone()
    cs3[:, 3] = False
    co3[:, 3] = False
    assert got[0].shape[0] > 1000 and _same(got, ops.mine_scores_typed_mc(z, w, *member_lists(cs3, co3), threshold=NINF))
    for k in (1, 500):
        assert _same(ops.mine_scores_typed_mc(poisoned, w, ptr, ids, k=k), ops.mine_scores_typed_mc(z, w, *member_lists(cs3, co3), k=k))
    # +inf / -inf logits in every sample: the probabilities are 1 / 0 and the triplets stay candidates
    special = z.clone()
    special[:, 5] = 0.0
    special[:, 5, 0] = float('inf')
    special[:, 6] = 0.0
    special[:, 6, 0] = float('-inf')
    got = ops.mine_scores_typed_mc(special, w, ptr, ids, threshold=NINF)
    assert got[2]['count'] == int(candidates(cs, co, None, True).sum()) == got[0].shape[0]
    touched = (got[0][:, 0] == 5) | (got[0][:, 2] == 5) | (got[0][:, 0] == 6) | (got[0][:, 2] == 6)
    assert int(touched.sum()) > 100 and not bool(torch.isnan(got[1]).any())
    assert bool(torch.isin(got[1][touched], torch.tensor([0.0, 0.5, 1.0], device='cuda')).all())
    # through the C entry an id outside [0, n) is no member: n in place of a set's largest member, -1 in place of its smallest
    zc, wc = z.contiguous(), w.contiguous()
    clean = emit_through_the_c_entry(ops, zc, wc, ptr, ids, 1 << 16)
    assert _same(clean, ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=NINF))
    bad, cs_b, co_b = ids.clone(), cs.clone(), co.clone()
    last, first = int(ptr[1]) - 1, int(ptr[num_rels])          # set 0 = the objects of relation 0, set R = its subjects
    co_b[0, int(ids[last])] = False
    cs_b[0, int(ids[first])] = False
    bad[last], bad[first] = n, -1
    got = emit_through_the_c_entry(ops, zc, wc, ptr, bad, 1 << 16)
    assert _same(got, ops.mine_scores_typed_mc(z, w, *member_lists(cs_b, co_b), threshold=NINF)) and got[2]['count'] < clean[2]['count']


def test_strided_stacks_and_empty_results(ops):
    gen = torch.Generator().manual_seed(9)
    base = torch.randn(2, 160, 50, generator=gen).cuda() * 0.4
    z = base[:, :150, 3:40]                                  # ld 50 > h = 37, a sample stride of 160 rows, bases off 16 bytes
    w = torch.randn(6, 50, generator=gen).cuda()[::2, 5:42]
    n, num_rels = 150, 3
    assert ops._mine_sample_stack(z, 'z')[1:] == (50, 160 * 50)                  # the strides reach the kernel as they are
    cs, co = member_masks(n, num_rels, gen)
    ptr, ids = member_lists(cs, co)
    bias = torch.tensor([0.3, -0.2], device='cuda')
    for sel in (dict(k=1), dict(k=333), dict(threshold=0.7), dict(threshold=NINF)):
        got = ops.mine_scores_typed_mc(z, w, ptr, ids, bias=bias, **sel)
        assert got[0].shape[0] > 0 and _same(got, ops.mine_scores_typed_mc(z.contiguous(), w.contiguous(), ptr, ids, bias=bias, **sel))
    # an empty plan: no launch
    nobody = torch.zeros(num_rels, n, dtype=torch.bool)
    for masks in ((nobody, nobody), (cs, nobody), (nobody, co)):
        for sel in (dict(k=5), dict(threshold=NINF)):
            got = ops.mine_scores_typed_mc(z, w, *member_lists(*masks), **sel)
            assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[2] == {'count': 0, 'passes': 0}
    # every candidate filtered: every key lists every entity
    keys = n * num_rels
    lo = torch.arange(keys, device='cuda') * n
    everyone = dict(filt_lo=lo, filt_hi=lo + n, filt_ent=torch.arange(n, device='cuda').repeat(keys))
    for sel in (dict(k=5), dict(threshold=NINF)):
        got = ops.mine_scores_typed_mc(z, w, ptr, ids, **everyone, **sel)
        assert got[0].shape == (0, 3) and got[2]['count'] == 0
    assert ops.mine_scores_typed_mc(z, w, ptr, ids, threshold=1.5)[2]['count'] == 0
    none = ops.mine_scores_typed_mc(z[:, :0], w, torch.zeros(7, dtype=torch.int64, device='cuda'),
                                    torch.zeros(0, dtype=torch.int32, device='cuda'), k=5)
    assert none[0].shape == (0, 3) and none[2]['count'] == 0


def test_wrappers_fused_against_unfused(ranking):
    """The two routes differ in the sigmoid's last bits, so the comparison is the bound's: the same triplets wherever the K-th
    value leaves no doubt (more than 2 eps from it), values within eps, the spread within test_gpu_mc_rank.py's tolerance."""
    from gcn_vae_amd import data
    kg = data.load_data('synthetic:300:7:2000:100:100')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    z, w, flps, _ = stack(3, kg.num_nodes, 32, kg.num_rels, 4)
    n, num_rels = kg.num_nodes, kg.num_rels

    def keyed(res):
        lin = (res[0][:, 0] * num_rels + res[0][:, 1]) * n + res[0][:, 2]
        return lin, eps[res[0][:, 1], res[0][:, 0], res[0][:, 2]]

    for kw in (dict(filter_index=fi, flow_log_probs=flps), dict(exclude_self=False)):
        eps = torch.from_numpy(pbar64(z, w, kw.get('flow_log_probs'))[1]).cuda()
        for sel in (dict(k=1), dict(k=500), dict(k=10 ** 7), dict(threshold=0.8)):
            got = ranking.mine_triplets_mc(z, w, type_constraint=tc, **sel, **kw)
            ref = ranking.mine_triplets_mc_unfused(z, w, type_constraint=tc, **sel, **kw)
            assert got[0].shape[0] > 0 and got[1].shape == got[2].shape == (got[0].shape[0],)
            assert bool((tc.contains(got[0][:, 1], got[0][:, 0], 's') & tc.contains(got[0][:, 1], got[0][:, 2], 'o')).all())
            (lin_g, eps_g), (lin_r, eps_r) = keyed(got), keyed(ref)
            edge = min(float(got[1].min()), float(ref[1].min())) if 'k' in sel else sel['threshold']
            sure_g, sure_r = got[1].double() > edge + 2 * eps_g, ref[1].double() > edge + 2 * eps_r
            assert bool(torch.isin(lin_g[sure_g], lin_r).all()) and bool(torch.isin(lin_r[sure_r], lin_g).all())
            assert int(sure_g.sum()) >= 0.9 * got[0].shape[0] - 1               # the doubtful band is thin
            if sel.get('k') == 10 ** 7:                                         # fewer candidates than K: all of them, no edge
                assert torch.equal(lin_g.sort().values, lin_r.sort().values) and got[3]['count'] == ref[3]['count'] == lin_g.numel()
            order_g, order_r = torch.argsort(lin_g), torch.argsort(lin_r)
            common_g, common_r = torch.isin(lin_g[order_g], lin_r), torch.isin(lin_r[order_r], lin_g)
            ig, ir = order_g[common_g], order_r[common_r]
            assert torch.equal(lin_g[ig], lin_r[ir])
            assert bool(((got[1][ig] - ref[1][ir]).abs().double() <= eps_g[ig]).all())
            assert bool(((got[2][ig] - ref[2][ir]).abs().double() <= 1e-5 + 2 * eps_g[ig]).all())
            assert bool((got[2] >= 0).all()) and bool((got[2] <= 0.5).all())
    with pytest.raises(ValueError, match='type_constraint'):
        ranking.mine_triplets_mc(z, w, k=3, filter_index=fi)
    with pytest.raises(ValueError, match='TypeConstraint'):
        ranking.mine_triplets_mc(z[:, :-1], w, k=3, type_constraint=tc)


def test_cli_writes_reproducible_type_correct_mc_completions(tmp_path):
    from gcn_vae_amd import data, ranking, train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:300:7:2000:100:100'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0, use_cuda=True,
                            reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda().eval()
    ckpt = str(tmp_path / 'm.pth')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    texts = []
    for run in range(2):
        out = str(tmp_path / f'mc{run}.tsv')
        args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                                '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file', ckpt,
                                                '--mc-samples', '3', '--mc-seed', '0', '--complete-topk', '50', '--complete-typed',
                                                '--complete-out', str(tmp_path / 'typed.tsv'), '--mc-complete', '--mc-complete-out', out])
        train.main(args)
        texts.append(open(out).read())
    assert texts[0] == texts[1]
    lines = [line.split('\t') for line in texts[0].splitlines()]
    assert len(lines) == 50 and all(len(x) == 6 for x in lines)
    rows = np.array([[int(v) for v in x[:4]] for x in lines])
    mean, std = np.array([float(x[4]) for x in lines]), np.array([float(x[5]) for x in lines])
    assert rows[:, 3].tolist() == list(range(1, 51))                            # ranks run 1 .. n
    assert (np.diff(mean) <= 0).all() and (0 <= mean).all() and (mean <= 1).all() and (0 <= std).all() and (std <= 0.5).all()
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test)
    s, r, o = (torch.from_numpy(rows[:, i]) for i in range(3))
    assert bool(tc.contains(r, s, 's').all()) and bool(tc.contains(r, o, 'o').all())
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    assert all(tuple(x[:3]) not in known and x[0] != x[2] for x in rows.tolist())
