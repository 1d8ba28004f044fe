"""Monte-Carlo posterior-predictive ranking and top-k on the GPU (gv_rank_scores_mc / gv_topk_scores_mc / gv_pair_prob_std_mc,
ops.*_mc, ranking.calc_mc_mrr / predict_topk_mc, KGVAE.posterior_samples, train.py --mc-samples).

Two kinds of checks.  Exact ones (torch.equal) need no arithmetic twin: the ranker's counts against a recount on the host from
the top-k scorer's own probabilities (one tile arithmetic), invariance under duplicated samples, permuted queries and relabelled
entities, and the tie / NaN / saturation rules.  The float64 ones hold every count inside the interval that a per-element
error bound leaves open:

    eps[i, j] = mean_s(gamma (|Q_s[i]| . |E_s[j]| + |bias_s|) / 4) + C_SIG u + S u,   u = 2^-24, gamma = (h + 2) u

(the logit's forward error through the sigmoid's Lipschitz constant 1/4, the device sigmoid's own error, the S-term sum), with
the interval's total slack capped at 0.002 of the comparisons so that the test cannot pass by leaving cases open.  C_SIG is
twice the largest error of the device sigmoid against float64 measured over logits in [-30, 30] (NOTES.md), rounded up.
pytest -m gpu."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_SIG = 4.0                # measured 1.83 u (at x = 3.61), doubled and rounded up
SLACK_CAP = 0.002
SHAPES = [(1, 1, 5, 8), (1, 70, 130, 8), (5, 130, 777, 40), (3, 37, 1000, 200), (2, 129, 300, 500), (4, 64, 6400, 24)]
SMALL = [(1, 1, 5, 8), (3, 70, 128, 24), (2, 37, 100, 200)]          # v <= 128: k = v returns every probability


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def ranking():
    from gcn_vae_amd import ranking as _ranking
    return _ranking


def _sig64(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-x))


def _object_lists(m, v, rng, target):
    """Per-query sorted unique entity lists -- empty, a few, across a 64-column boundary, one whole 64-column window, listing the
    query's own target -- as a list of arrays."""
    out = []
    for i in range(m):
        kind = i % 5
        if kind == 0:
            e = np.zeros(0, dtype=np.int64)
        elif kind == 1:
            e = np.unique(rng.integers(0, v, 5))
        elif kind == 2:
            c = 64 * int(rng.integers(1, max(2, v // 64)))
            e = np.arange(max(0, c - 3), min(v, c + 3))
        elif kind == 3:
            c = 64 * int(rng.integers(0, max(1, v // 64)))
            e = np.arange(c, min(v, c + 64))
        else:
            e = np.unique(np.concatenate([rng.integers(0, v, 3), [target[i]]]))
        out.append(e.astype(np.int64))
    return out


def _pack(lists):
    lens = np.array([len(e) for e in lists], dtype=np.int64)
    hi = np.cumsum(lens)
    ent = np.concatenate(lists) if lens.sum() else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(hi - lens).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(ent).cuda()


def _dense(lists, v):
    mask = np.zeros((len(lists), v), dtype=bool)
    for i, e in enumerate(lists):
        mask[i, e] = True
    return mask


@functools.lru_cache(maxsize=None)
def _case(s, m, v, h):
    """The issue's input recipe, its float64 reference and the per-element bound; computed once per shape and left unchanged."""
    from gcn_vae_amd import ranking
    rng = np.random.default_rng(s + m + v + h)
    scale = 0.8 * h ** -0.25
    base = scale * rng.standard_normal((v, h))
    z = (base[None] + 0.5 * scale * rng.standard_normal((s, v, h))).astype(np.float32)
    w = rng.standard_normal((9, h)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(s)).astype(np.float32)
    a, r, b = rng.integers(0, v, m), rng.integers(0, 9, m), rng.integers(0, v, m)
    q = z[:, a] * w[r][None]                                    # one fp32 multiply per element, as ops.mul forms it
    lists = _object_lists(m, v, rng, b)
    # queries that share (a, r) share their known objects
    known = {}
    for i in range(m):
        known.setdefault((int(a[i]), int(r[i])), set()).update(lists[i].tolist())
    lists = [np.array(sorted(known[(int(a[i]), int(r[i]))]), dtype=np.int64) for i in range(m)]
    trip = np.array([(k[0], k[1], o) for k, objs in known.items() for o in objs], dtype=np.int64).reshape(-1, 3)
    q64, z64 = q.astype(np.float64), z.astype(np.float64)
    logit = q64 @ z64.transpose(0, 2, 1) + bias.astype(np.float64)[:, None, None]
    p_s = _sig64(logit)
    pbar = p_s.sum(axis=0) / s
    std = np.sqrt(((p_s - pbar[None]) ** 2).sum(axis=0) / s)
    gamma = (h + 2) * U
    mag = np.abs(q64) @ np.abs(z64).transpose(0, 2, 1) + np.abs(bias.astype(np.float64))[:, None, None]
    eps = (gamma * mag / 4).mean(axis=0) + C_SIG * U + s * U
    dev = dict(z=torch.from_numpy(z).cuda(), w=torch.from_numpy(w).cuda(), bias=torch.from_numpy(bias).cuda(),
               q=torch.from_numpy(q).cuda(), a=torch.from_numpy(a).cuda(), r=torch.from_numpy(r).cuda(), b=torch.from_numpy(b).cuda())
    fi = ranking.FilterIndex(v, 9, trip, device='cuda')
    return dict(dev, lists=lists, listed=_dense(lists, v), pbar=pbar, std=std, eps=eps, b_np=b, fi=fi, shape=(s, m, v, h))


def _interval(c, listed):
    """(lower, upper) 0-based ranks per query that the bound leaves open, over the candidates that count."""
    pbar, eps, b = c['pbar'], c['eps'], c['b_np']
    m, v = pbar.shape
    rows = np.arange(m)
    counts = np.ones((m, v), dtype=bool)
    counts[rows, b] = False
    if listed is not None:
        counts &= ~listed
    pt, et = pbar[rows, b][:, None], eps[rows, b][:, None]
    lower = ((pbar > pt + eps + et) & counts).sum(axis=1)
    upper = ((pbar >= pt - eps - et) & counts).sum(axis=1)
    return lower, upper


def _assert_inside(c, raw, filt, label):
    s, m, v, h = c['shape']
    for name, got, listed in (('raw', raw, None), ('filtered', filt, c['listed'])):
        lower, upper = _interval(c, listed)
        got = got.cpu().numpy().astype(np.float64)
        slack = float((upper - lower).sum()) / max(m * (v - 1), 1)
        print(f'{label} {c["shape"]} {name}: slack share {slack:.3e}, '
              f'outside {int(((got < lower) | (got > upper)).sum())} of {m}')
        assert slack <= SLACK_CAP
        assert bool(((got >= lower) & (got <= upper)).all())


@pytest.mark.parametrize('shape', SHAPES)
def test_ranks_lie_inside_the_float64_interval(ranking, shape):
    c = _case(*shape)
    m = shape[1]
    raw, filt = ranking.perturb_and_get_rank_mc(c['z'], c['w'], c['a'], c['r'], c['b'], m, c['fi'], 'o', flow_log_probs=c['bias'])
    _assert_inside(c, raw, filt, 'fused')
    raw_only, none = ranking.perturb_and_get_rank_mc(c['z'], c['w'], c['a'], c['r'], c['b'], m, flow_log_probs=c['bias'])
    assert none is None and torch.equal(raw_only, raw)               # the raw counts with a filter equal the counts without one


def test_unfused_route_is_held_to_the_same_interval(ranking):
    c = _case(*SHAPES[2])
    raw, filt = ranking.perturb_and_get_rank_mc_unfused(c['z'], c['w'], c['a'], c['r'], c['b'], SHAPES[2][1], c['fi'], 'o',
                                                        flow_log_probs=c['bias'])
    _assert_inside(c, raw, filt, 'unfused')


@pytest.mark.parametrize('shape', SHAPES)
def test_topk_mean_and_std_against_float64(ranking, shape):
    c = _case(*shape)
    s, m, v, h = shape
    k = 10
    ids, mean, std = ranking.predict_topk_mc(c['z'], c['w'], c['a'], c['r'], k, 'o', c['fi'], c['bias'])
    ids, mean, std = ids.cpu().numpy(), mean.cpu().numpy().astype(np.float64), std.cpu().numpy().astype(np.float64)
    pbar, eps = c['pbar'], c['eps']
    worst_mean = worst_std = 0.0
    for i in range(m):
        cand = np.nonzero(~c['listed'][i])[0]
        kk = min(k, len(cand))
        got = ids[i, :kk]
        assert (ids[i, kk:] == -1).all() and (mean[i, kk:] == -np.inf).all() and (std[i, kk:] == 0).all()
        assert len(set(got.tolist())) == kk and not c['listed'][i, got].any()
        worst_mean = max(worst_mean, float((np.abs(mean[i, :kk] - pbar[i, got]) / eps[i, got]).max(initial=0.0)))
        worst_std = max(worst_std, float((np.abs(std[i, :kk] - c['std'][i, got]) / (1e-5 + 2 * eps[i, got])).max(initial=0.0)))
        assert (np.diff(mean[i, :kk]) <= 0).all()                    # best first
        # no returned candidate is decidedly worse than one left out: the symmetric difference to the float64 top-k lies
        # inside the undecided band, and is empty where the k-th / (k+1)-th gap exceeds the two elements' eps
        out = np.setdiff1d(cand, got)
        if len(out) and kk:
            assert (pbar[i, got] + eps[i, got]).min() >= (pbar[i, out] - eps[i, out]).max()
        order = cand[np.argsort(-pbar[i, cand], kind='stable')]
        if kk and len(order) > kk:
            kth, nxt = order[kk - 1], order[kk]
            if pbar[i, kth] - pbar[i, nxt] > eps[i, kth] + eps[i, nxt]:
                assert set(got.tolist()) == set(order[:kk].tolist())
    print(f'top-k {shape}: worst |mean - pbar64| / eps {worst_mean:.3f}, worst std error / bound {worst_std:.3f}')
    assert worst_mean <= 1.0 and worst_std <= 1.0


def _small_inputs(s, m, v, h, seed=0):
    gen = torch.Generator().manual_seed(1000 * s + m + v + h + seed)
    e = (torch.randn(s, v, h, generator=gen) * 0.7 * h ** -0.25).cuda()
    q = (torch.randn(s, m, h, generator=gen) * h ** -0.25).cuda()
    bias = (torch.randn(s, generator=gen) * 0.5).cuda()
    rng = np.random.default_rng(seed + m + v)
    target = rng.integers(0, v, m)
    target[-1] = v - 1                                              # a target in the last (partial) tile
    lists = _object_lists(m, v, rng, target)
    return q, e, bias, torch.from_numpy(target).cuda(), lists


def _dense_probs(ops, q, e, bias, v):
    """Every pbar[i, j] as the device computes it: the unfiltered top-k scorer with k = v, scattered back by id."""
    ids, prob = ops.topk_scores_mc(q, e, v, bias)
    assert bool((ids >= 0).all())
    dense = torch.empty_like(prob)
    dense.scatter_(1, ids, prob)
    assert torch.equal(ids.sort(dim=1).values, torch.arange(v, device='cuda').expand_as(ids))
    return dense


@pytest.mark.parametrize('shape', SMALL)
def test_counts_equal_the_recount_from_the_topk_probabilities(ops, ranking, shape):
    s, m, v, h = shape
    q, e, bias, target, lists = _small_inputs(*shape)
    lo, hi, ent = _pack(lists)
    listed = torch.from_numpy(_dense(lists, v)).cuda()
    pbar = _dense_probs(ops, q, e, bias, v)
    raw, filt, tgt = ops.rank_scores_mc(q, e, target, bias, lo, hi, ent)
    w_raw, w_filt = ranking.mc_ranks_from_probs(pbar, target, listed)
    assert raw.dtype == torch.float32 and torch.equal(raw, w_raw) and torch.equal(filt, w_filt)
    assert torch.equal(tgt, pbar.gather(1, target.view(-1, 1)).view(-1))           # tgt is the out_prob of the target's id
    # raw - filtered = the votes of the listed candidates, counted the same way
    t = pbar.gather(1, target.view(-1, 1))
    votes = listed & torch.ones_like(listed).scatter_(1, target.view(-1, 1), False)
    assert torch.equal(raw - filt, ((pbar > t) & votes).sum(1).float() + 0.5 * ((pbar == t) & votes).sum(1).float())
    # the raw counts with a filter equal the counts without one
    raw0, none, tgt0 = ops.rank_scores_mc(q, e, target, bias)
    assert none is None and torch.equal(raw0, raw) and torch.equal(tgt0, tgt)
    # the filtered top-k is the rule of topk_from_scores on those very probabilities, bit for bit
    k = min(v, 17)
    ids, prob = ops.topk_scores_mc(q, e, k, bias, lo, hi, ent)
    w_ids, w_prob = ranking.topk_from_scores(pbar, k, lo, hi, ent)
    assert torch.equal(ids, w_ids) and torch.equal(prob, w_prob)
    assert bool(((pbar >= 0) & (pbar <= 1)).all())


@pytest.mark.parametrize('shape', [(1, 70, 130, 8), (1, 37, 1000, 200)])
def test_a_sample_given_twice_is_the_sample(ops, shape):
    s, m, v, h = shape
    q, e, bias, target, lists = _small_inputs(*shape)
    lo, hi, ent = _pack(lists)
    one = ops.rank_scores_mc(q, e, target, bias, lo, hi, ent)
    two = ops.rank_scores_mc(q.repeat(2, 1, 1), e.repeat(2, 1, 1), target, bias.repeat(2), lo, hi, ent)      # p + p and * 0.5f are exact
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    ids1, prob1 = ops.topk_scores_mc(q, e, 10, bias, lo, hi, ent)
    ids2, prob2 = ops.topk_scores_mc(q.repeat(2, 1, 1), e.repeat(2, 1, 1), 10, bias.repeat(2), lo, hi, ent)
    assert torch.equal(ids1, ids2) and torch.equal(prob1, prob2)
    # one sample: the key's value is sigmoid of the single-sample scorer's logit, so the order is its order wherever those differ
    l_ids, logits = ops.topk_scores(q[0], e[0], 10, bias, lo, hi, ent)
    distinct = (prob1[:, 1:] != prob1[:, :-1]).all(dim=1)
    assert torch.equal(ids1[distinct], l_ids[distinct])
    # the spread of one sample, and of one sample given four times, is exactly zero
    assert not ops.pair_prob_std_mc(q, e, ids1, bias).any()
    assert not ops.pair_prob_std_mc(q.repeat(4, 1, 1), e.repeat(4, 1, 1), ids1, bias.repeat(4)).any()


def test_permuted_queries_and_relabelled_entities(ops):
    s, m, v, h = 3, 130, 300, 40
    q, e, bias, target, lists = _small_inputs(s, m, v, h)
    lo, hi, ent = _pack(lists)
    raw, filt, tgt = ops.rank_scores_mc(q, e, target, bias, lo, hi, ent)
    ids, prob = ops.topk_scores_mc(q, e, 10, bias, lo, hi, ent)
    gen = torch.Generator().manual_seed(9)
    # permuting the query rows permutes the outputs
    pm = torch.randperm(m, generator=gen)
    lo_p, hi_p, ent_p = _pack([lists[i] for i in pm.tolist()])
    pm = pm.cuda()
    raw_p, filt_p, tgt_p = ops.rank_scores_mc(q[:, pm].contiguous(), e, target[pm], bias, lo_p, hi_p, ent_p)
    assert torch.equal(raw_p, raw[pm]) and torch.equal(filt_p, filt[pm]) and torch.equal(tgt_p, tgt[pm])
    ids_p, prob_p = ops.topk_scores_mc(q[:, pm].contiguous(), e, 10, bias, lo_p, hi_p, ent_p)
    assert torch.equal(ids_p, ids[pm]) and torch.equal(prob_p, prob[pm])
    # relabelling the entities (new id = label[old id]) leaves every count and every probability unchanged
    label = torch.randperm(v, generator=gen)
    e_new = torch.empty_like(e)
    e_new[:, label.cuda()] = e
    lo_l, hi_l, ent_l = _pack([np.sort(label.numpy()[x]) for x in lists])
    raw_l, filt_l, tgt_l = ops.rank_scores_mc(q, e_new, label.cuda()[target], bias, lo_l, hi_l, ent_l)
    assert torch.equal(raw_l, raw) and torch.equal(filt_l, filt) and torch.equal(tgt_l, tgt)


def test_ties_nan_and_saturation(ops):
    s, h, v = 2, 8, 100
    gen = torch.Generator().manual_seed(0)
    e = (torch.randn(s, v, h, generator=gen) * 0.5).cuda()
    e[:, 7] = e[:, 3]
    e[:, 99] = e[:, 3]
    e[:, 90] = e[:, 3]
    q = e[:, [3, 3, 3]].clone()
    target = torch.tensor([3, 3, 7], device='cuda')
    # query 0: entity 7 (a tie) listed; query 1: nothing listed; query 2: 3 and 90 (ties) listed, 99 not
    lo, hi, ent = _pack([np.array([7]), np.zeros(0, dtype=np.int64), np.array([3, 90])])
    raw, filt, tgt = ops.rank_scores_mc(q, e, target, None, lo, hi, ent)
    pbar = _dense_probs(ops, q, e, None, v)
    better = [int((pbar[i] > pbar[i, int(target[i])]).sum()) for i in range(3)]
    assert float(raw[0]) == better[0] + 1.5 and float(filt[0]) == better[0] + 1.0         # duplicate rows tie at the mid-rank
    assert float(filt[1]) == float(raw[1]) == better[1] + 1.5
    assert float(raw[2]) == better[2] + 1.5 and float(filt[2]) == better[2] + 0.5
    # a NaN row in ONE sample makes the candidate NaN: it counts as above unless listed
    bad = e.clone()
    bad[1, 10] = float('nan')
    bad[0, 20] = float('nan')
    one = torch.zeros(1, dtype=torch.int64, device='cuda')
    qq, t3 = e[:, [3]].clone(), torch.tensor([3], device='cuda')
    raw, filt, _ = ops.rank_scores_mc(qq, bad, t3, None, one, one + 1, torch.tensor([10], device='cuda'))
    pb = _dense_probs(ops, qq, e, None, v)[0]
    b = int((pb > pb[3]).sum()) - int(pb[10] > pb[3]) - int(pb[20] > pb[3])                 # above among the others
    assert float(raw[0]) == b + 2 + 1.5 and float(filt[0]) == b + 1 + 1.5
    ids, prob = ops.topk_scores_mc(qq, bad, v, None)
    assert sorted(ids[0, -2:].tolist()) == [10, 20] and bool(torch.isnan(prob[0, -2:]).all())    # NaN after everything
    # a NaN target ranks last among the candidates that count
    bad_t = e.clone()
    bad_t[1, 3] = float('nan')
    raw, filt, tgt = ops.rank_scores_mc(qq, bad_t, t3, None, one, one + 5, torch.arange(5, device='cuda'))
    assert float(raw[0]) == v - 1 and float(filt[0]) == v - 1 - 4 and bool(torch.isnan(tgt[0]))
    # all-equal tables: the middle rank of the candidates that count
    same = torch.ones(s, v, h, device='cuda')
    tq = torch.tensor([0, 64], device='cuda')
    lo2, hi2 = torch.tensor([0, 0], device='cuda'), torch.tensor([10, 10], device='cuda')
    raw, filt, _ = ops.rank_scores_mc(torch.ones(s, 2, h, device='cuda'), same, tq, None, lo2, hi2, torch.arange(10, device='cuda'))
    assert torch.equal(raw.cpu(), torch.full((2,), (v - 1) / 2.0))
    assert float(filt[0]) == (v - 10) / 2.0 and float(filt[1]) == (v - 1 - 10) / 2.0
    # saturation: logits of 40 and more round every probability to 1.0f -- a tie the logit ranker would not see -- and logits of
    # -110 to 0.0f (or a denormal) in every sample
    big = e.clone() * 0 + torch.linspace(5.0, 6.0, v, device='cuda').view(1, v, 1)
    raw, _, tgt = ops.rank_scores_mc(torch.ones(s, 2, h, device='cuda'), big, tq, None)
    assert torch.equal(tgt.cpu(), torch.ones(2)) and torch.equal(raw.cpu(), torch.full((2,), (v - 1) / 2.0))
    ids, prob = ops.topk_scores_mc(torch.ones(s, 1, h, device='cuda'), big, 5, None)
    assert ids[0].tolist() == [0, 1, 2, 3, 4] and bool((prob == 1).all())                   # ties by lower id
    _, _, tgt = ops.rank_scores_mc(-torch.ones(s, 2, h, device='cuda') * 2.5, big, tq, None)
    assert bool((tgt >= 0).all()) and bool((tgt < 1e-37).all())
    # +-inf logits in a sample: 1 and 0
    inf_e = torch.zeros(1, 2, 1, device='cuda')
    inf_e[0, 0, 0], inf_e[0, 1, 0] = float('inf'), float('-inf')
    ids, prob = ops.topk_scores_mc(torch.ones(1, 1, 1, device='cuda'), inf_e, 2, None)
    assert ids[0].tolist() == [0, 1] and prob[0].tolist() == [1.0, 0.0]


def test_argument_errors(ops):
    q, e = torch.zeros(2, 4, 8, device='cuda'), torch.zeros(2, 50, 8, device='cuda')
    t = torch.zeros(4, dtype=torch.int64, device='cuda')
    lo, hi, ent = t.clone(), t.clone() + 2, torch.arange(2, device='cuda')
    ops.rank_scores_mc(q, e, t, torch.zeros(2, device='cuda'), lo, hi, ent)
    with pytest.raises(ValueError, match='samples'):
        ops.rank_scores_mc(q, e[:1], t)                                          # S differs between q and e
    with pytest.raises(ValueError, match='samples'):
        ops.topk_scores_mc(q[:1], e, 3)
    with pytest.raises(ValueError, match='bias'):
        ops.rank_scores_mc(q, e, t, torch.zeros(3, device='cuda'))               # one bias per sample
    with pytest.raises(ValueError, match='bias'):
        ops.pair_prob_std_mc(q, e, torch.zeros(4, 2, dtype=torch.int64, device='cuda'), torch.zeros(1, device='cuda'))
    with pytest.raises(ValueError, match='k must lie'):
        ops.topk_scores_mc(q, e, ops.TOPK_MAX + 1)
    with pytest.raises(ValueError):
        ops.rank_scores_mc(q, e, t, None, lo, hi + 1, ent)                       # a range past the end of the list
    with pytest.raises(ValueError):
        ops.topk_scores_mc(q, e, 3, None, lo, hi, ent + 50)                      # ids out of [0, v)
    with pytest.raises(ValueError):
        ops.rank_scores_mc(q, e, t, None, lo, None, ent)                         # all of the filter or none
    with pytest.raises(ValueError):
        ops.rank_scores_mc(q, e, t + 50)                                         # targets out of [0, v)
    with pytest.raises(ValueError, match='width'):
        ops.rank_scores_mc(q, e[:, :, :4], t)
    with pytest.raises(ValueError):
        ops.pair_prob_std_mc(q, e, torch.full((4, 2), 50, dtype=torch.int64, device='cuda'))
    with pytest.raises(TypeError):
        ops.rank_scores_mc(q[0], e[0], t)                                        # the single-sample operands
    # the entry itself refuses a stride shorter than the rows it spans
    from gcn_vae_amd import lib
    tgt, cnt = torch.zeros(4, device='cuda'), torch.zeros(4, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError, match='stride'):
        lib.call('gv_rank_scores_mc', lib.ptr(q), 8, 31, lib.ptr(e), 8, 400, 2, lib.ptr(t.int()), None, None, None, None, 0,
                 lib.ptr(tgt), lib.ptr(cnt), None, 4, 50, 8, lib.stream())
    with pytest.raises(RuntimeError, match='n_samples'):
        lib.call('gv_rank_scores_mc', lib.ptr(q), 8, 32, lib.ptr(e), 8, 400, 0, lib.ptr(t.int()), None, None, None, None, 0,
                 lib.ptr(tgt), lib.ptr(cnt), None, 4, 50, 8, lib.stream())


# ---- end to end: a real encoder's posterior samples -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    from gcn_vae_amd import ranking, sampling
    from gcn_vae_amd.data import synthetic_kg
    from gcn_vae_amd.encoders import KGVAE
    from gcn_vae_amd.train import LinkPredict
    kg = synthetic_kg(400, 9, 3000, 200, 300, seed=4)
    torch.manual_seed(0)
    net = LinkPredict(KGVAE, kg.num_nodes, 32, kg.num_rels, num_bases=4, num_hidden_layers=2, dropout=0.0, use_cuda=True,
                      reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda().eval()
    graph, rel, norm = sampling.build_test_graph(kg.num_nodes, kg.num_rels, kg.train)
    node_id = torch.arange(kg.num_nodes, device='cuda').view(-1, 1)
    enorm = sampling.node_norm_to_edge_norm(graph, torch.from_numpy(norm).view(-1, 1)).cuda()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    return kg, net, (graph, node_id, torch.from_numpy(rel).cuda(), enorm), fi


def test_posterior_samples_are_seeded_prefix_stable_and_share_one_encoder_pass():
    kg, net, inputs, _ = _model()
    enc = net.encoder
    calls = []
    real = enc.rconv_layer_1.forward
    enc.rconv_layer_1.forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        z4, f4 = enc.posterior_samples(*inputs, 4, seed=11)
    finally:
        del enc.rconv_layer_1.forward
    assert len(calls) == 1                                            # the layers ran once for the four samples
    assert tuple(z4.shape) == (4, kg.num_nodes, 32) and z4.dtype == torch.float32 and z4.is_contiguous()
    assert tuple(f4.shape) == (4,) and f4.dtype == torch.float32
    assert bool(torch.isfinite(z4).all()) and not torch.equal(z4[0], z4[1])
    assert torch.equal(enc.flow_log_prob.reshape(()), f4[3])          # the state a forward would leave after the last sample
    z4b, f4b = enc.posterior_samples(*inputs, 4, seed=11)
    assert torch.equal(z4, z4b) and torch.equal(f4, f4b)              # the same seed: the same samples, bit for bit
    z2, f2 = enc.posterior_samples(*inputs, 2, seed=11)
    assert torch.equal(z2, z4[:2]) and torch.equal(f2, f4[:2])        # prefix-stable in S
    assert not torch.equal(enc.posterior_samples(*inputs, 2, seed=12)[0], z2)
    override = torch.zeros(kg.num_nodes, 32, device='cuda')
    enc.eps_override = override
    try:
        assert torch.equal(enc.posterior_samples(*inputs, 2, seed=11)[0], z2) and enc.eps_override is override
    finally:
        enc.eps_override = None
    # a sample is what forward() computes from the same noise
    gen = torch.Generator(device='cuda').manual_seed(11)
    enc.eps_override = torch.randn(kg.num_nodes, 32, generator=gen, device='cuda')
    try:
        with torch.no_grad():
            z_fwd = net(*inputs)
    finally:
        enc.eps_override = None
    assert torch.equal(z_fwd, z4[0]) and torch.equal(enc.get_flow_log_prob().reshape(()), f4[0])
    no_flows = type(enc)(kg.num_nodes, 32, 32, 2 * kg.num_rels, num_bases=4, k=4, n_flows=0).cuda().eval()
    z, f = no_flows.posterior_samples(*inputs, 2, seed=0)
    assert f is None and tuple(z.shape) == (2, kg.num_nodes, 32)


MC_SEED = 11


def _host_restatement(ranking, kg, z, w, flps, a, b, r, side):
    """float64 on the host, from the known-triplet sets: per query the interval of 0-based ranks that the per-element bound
    leaves open, raw and filtered, and the number of undecided comparisons."""
    z64, w64, f64 = z.cpu().double(), w.detach().cpu().double(), flps.cpu().double()
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    n, h, s = kg.num_nodes, z.shape[2], z.shape[0]
    pbar = ranking.mc_mean_prob(z64, w64, a, r, f64).numpy()
    mag = torch.einsum('smh,svh->smv', (z64[:, a] * w64[r]).abs(), z64.abs()).numpy() + f64.abs().numpy()[:, None, None]
    eps = ((h + 2) * U * mag / 4).mean(axis=0) + C_SIG * U + s * U
    out = {'raw': ([], []), 'filtered': ([], [])}
    undecided = 0
    for i in range(len(a)):
        t, qa, rel = int(b[i]), int(a[i]), int(r[i])
        listed = np.array([((j, rel, qa) if side == 's' else (qa, rel, j)) in known for j in range(n)])
        for kind, counts in (('raw', np.ones(n, dtype=bool)), ('filtered', ~listed)):
            counts = counts.copy()
            counts[t] = False
            band = eps[i] + eps[i, t]
            lower = int((pbar[i] > pbar[i, t] + band)[counts].sum())
            upper = int((pbar[i] >= pbar[i, t] - band)[counts].sum())
            out[kind][0].append(lower)
            out[kind][1].append(upper)
            undecided += upper - lower
    return out, undecided


def test_calc_mc_mrr_end_to_end(ranking):
    """Real posterior samples of a seeded synthetic KG, S = 4, against a float64 restatement on the host: every query's raw and
    filtered rank lies in the interval the per-element bound leaves open, the reported MRR / Hits are those of these ranks and lie
    between the restatement's figures at the two ends of the intervals to 1e-6 -- where the restatement finds no undecided
    comparison the two ends coincide and this is agreement to 1e-6 --, filtered >= raw, and the materialised route reports the same.

    The restatement does NOT come out free of undecided comparisons on this model: its encoder is untrained, the probabilities of
    a query's 400 candidates crowd into a narrow band around 0.5, and of the 2 x 300 x 399 comparisons a few dozen fall inside
    eps_j + eps_t (58 of the 478 800 counted over raw + filtered at seed 11; no seed can be expected to leave none at that density).
    So the undecided ones are bounded instead of asserted absent: at most 0.002 of the comparisons, the cap of the interval tests."""
    kg, net, inputs, fi = _model()
    z, flps = net.encoder.posterior_samples(*inputs, 4, seed=MC_SEED)
    test = torch.from_numpy(kg.test).cuda()
    hits = [1, 3, 10]
    out = ranking.calc_mc_mrr(z, net.w_relation, test, fi, flps, hits=hits, eval_bz=50, verbose=False)
    assert out['n_samples'] == 4 and set(out) == {'n_samples', 'mrr_raw', 'hits_raw', 'mrr_filtered', 'hits_filtered'}
    raw_only = ranking.calc_mc_mrr(z, net.w_relation, test, None, flps, hits=hits, verbose=False)
    assert set(raw_only) == {'n_samples', 'mrr_raw', 'hits_raw'} and raw_only['mrr_raw'] == out['mrr_raw']
    s_, r_, o_ = test[:, 0], test[:, 1], test[:, 2]
    got, ends, undecided = {'raw': [], 'filtered': []}, {'raw': ([], []), 'filtered': ([], [])}, 0
    for a, b, side in ((o_, s_, 's'), (s_, o_, 'o')):
        raw, filt = ranking.perturb_and_get_rank_mc(z, net.w_relation, a, r_, b, len(b), fi, side, flow_log_probs=flps)
        got['raw'].append(raw.cpu().double())
        got['filtered'].append(filt.cpu().double())
        iv, n_open = _host_restatement(ranking, kg, z, net.w_relation, flps, a.cpu(), b.cpu(), r_.cpu(), side)
        undecided += n_open
        for kind in ends:
            ends[kind][0].extend(iv[kind][0])
            ends[kind][1].extend(iv[kind][1])
    comparisons = 2 * 2 * len(kg.test) * (kg.num_nodes - 1)
    print(f'end to end: {undecided} undecided of {comparisons} comparisons')
    assert undecided <= SLACK_CAP * comparisons
    for kind in ('raw', 'filtered'):
        rk = torch.cat(got[kind])
        lower, upper = (torch.tensor(x, dtype=torch.float64) for x in ends[kind])
        assert bool(((rk >= lower) & (rk <= upper)).all())
        assert abs(out['mrr_' + kind] - float((1.0 / (rk + 1)).mean())) < 1e-6
        assert float((1.0 / (upper + 1)).mean()) - 1e-6 <= out['mrr_' + kind] <= float((1.0 / (lower + 1)).mean()) + 1e-6
        for k in hits:
            assert float((upper + 1 <= k).double().mean()) - 1e-6 <= out['hits_' + kind][k] <= float((lower + 1 <= k).double().mean()) + 1e-6
    assert out['mrr_filtered'] >= out['mrr_raw']
    assert all(out['hits_filtered'][k] >= out['hits_raw'][k] for k in hits)
    unfused = ranking.calc_mc_mrr_unfused(z, net.w_relation, test, fi, flps, hits=hits, verbose=False)
    for kind in ('raw', 'filtered'):
        lower, upper = (torch.tensor(x, dtype=torch.float64) for x in ends[kind])
        assert float((1.0 / (upper + 1)).mean()) - 1e-6 <= unfused['mrr_' + kind] <= float((1.0 / (lower + 1)).mean()) + 1e-6


def test_cli_reports_and_writes_mc_predictions(ops, tmp_path, capsys, monkeypatch):
    from gcn_vae_amd import train
    from gcn_vae_amd.data import load_data
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:300:7:2000:100:80:3'
    kg = load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt = str(tmp_path / 'm.pth')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    base = ['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1', '--mog-k', '4', '--n-flows', '2',
            '--test-mode', 'True', '--model-state-file', ckpt, '--predict-topk', '3', '--filtered-eval']
    runs = {}
    for name, extra in (('plain', []), ('mc', ['--mc-samples', '4', '--mc-seed', '5'])):
        out, mc_out = str(tmp_path / f'{name}.tsv'), str(tmp_path / f'{name}_mc.tsv')
        # the same noise in both runs: the device RNG restarts when torch's seed changes, and a model's draws are keyed by the
        # process-unique stream ids it takes at construction -- both runs' models get the same ones
        torch.manual_seed(2)
        ops.device_rng(torch.device('cuda', 0)).tick()
        torch.manual_seed(1)
        monkeypatch.setattr(ops, '_rng_streams', itertools.count(1 << 20))
        mrr = train.main(train.build_parser().parse_args(base + extra + ['--predict-out', out, '--mc-predict-out', mc_out]))
        runs[name] = (mrr, open(out).read(), capsys.readouterr().out.replace(out, 'OUT'), mc_out)
    assert runs['plain'][0] == runs['mc'][0]                             # the return value is unchanged
    assert runs['plain'][1] == runs['mc'][1]                             # predictions.tsv is the same file
    assert runs['mc'][2].startswith(runs['plain'][2])                    # everything printed today, then the MC report
    report = runs['mc'][2][len(runs['plain'][2]):]
    assert 'MC MRR (raw, 4 samples)' in report and 'MC MRR (filtered, 4 samples)' in report and 'MC Hits (filtered) @ 10' in report
    assert not __import__('os').path.exists(runs['plain'][3])            # no MC file without the flag
    rows = [line.rstrip('\n').split('\t') for line in open(runs['mc'][3])]
    n_test = len(kg.test)
    assert len(rows) == 2 * n_test * 3 and all(len(x) == 7 for x in rows)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    for j, d in enumerate(('o', 's')):
        block = rows[j * n_test * 3:(j + 1) * n_test * 3]
        assert all(x[0] == d for x in block) and [int(x[3]) for x in block] == [0, 1, 2] * n_test
        assert [int(x[1]) for x in block[::3]] == kg.test[:, 0 if d == 'o' else 2].tolist()
        assert [int(x[2]) for x in block[::3]] == kg.test[:, 1].tolist()
        for x in block:
            qa, rel, e_, mean, std = int(x[1]), int(x[2]), int(x[4]), float(x[5]), float(x[6])
            assert e_ >= 0 and ((qa, rel, e_) if d == 'o' else (e_, rel, qa)) not in known          # new facts only
            assert 0.0 <= mean <= 1.0 and 0.0 <= std <= 0.5
        means = np.array([float(x[5]) for x in block]).reshape(n_test, 3)
        assert (np.diff(means, axis=1) <= 0).all()
