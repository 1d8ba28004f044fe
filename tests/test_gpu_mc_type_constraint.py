"""Type-constrained ranking and top-k on the Monte-Carlo posterior predictive, on the GPU (gv_rank_scores_mc_constrained /
gv_topk_scores_mc_constrained, ops.*_mc_constrained, ranking.calc_mc_constrained_mrr / predict_topk_mc(type_constraint=...),
train.py --mc-type-constrain).

Exact checks (torch.equal) need no arithmetic twin: the unconstrained outputs against ops.rank_scores_mc, the all-ones / empty /
out-of-range sets, the four counts and the constrained selection against a recount on the host from the top-k scorer's own
probabilities, padding bits, a strided mask, an odd word count, duplicated samples, permuted queries, the one-sample order and
the tie / NaN / saturation rules.  The float64 ones reuse the recipe, bound and constants of tests/test_gpu_mc_rank.py:

    eps[i, j] = mean_s(gamma (|Q_s[i]| . |E_s[j]| + |bias_s|) / 4) + C_SIG u + S u,   u = 2^-24, gamma = (h + 2) u

with every one of the four ranks held inside the interval the bound leaves open over ITS pool, and the share of undecided
comparisons taken over that pool's counted comparisons and capped at SLACK_CAP.  On the float64 reference alone (no device) the
constrained pools of these cases leave 0 or 1 comparison undecided per shape, a share of at most 9.5e-5 (``_case_host`` needs
no GPU).  pytest -m gpu."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_SIG = 4.0                # the device sigmoid's measured error against float64, 1.83 u (at x = 3.61), doubled and rounded up
SLACK_CAP = 0.002
SHAPES = [(1, 1, 5, 8), (1, 70, 130, 8), (5, 130, 777, 40), (3, 37, 1000, 200), (2, 129, 300, 500), (4, 64, 6400, 24)]
SMALL = [(1, 1, 5, 8), (3, 70, 128, 24), (2, 37, 100, 200)]          # v <= 128: k = v returns every probability
N_SETS = 18
DENSITIES = (0.0, 1.0, 0.5, 0.065, 0.3, 0.02)
KINDS = ('raw', 'filtered', 'raw_constrained', 'filtered_constrained')


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


def _sets(v, seed):
    """N_SETS sets as a dense (N_SETS, v) bool: member densities cycling through DENSITIES, drawn from a generator of their own;
    the third empty one holds the last three ids instead."""
    rng = np.random.default_rng(7919 + seed)
    sets = np.stack([rng.random(v) < DENSITIES[j % len(DENSITIES)] for j in range(N_SETS)])
    sets[12] = False
    sets[12, max(0, v - 3):] = True
    return sets


def _words(sets, extra_words=0, fill=0):
    """The bitmask of a dense (n_sets, v) bool: int32 (n_sets, ceil(v / 32) + extra_words) on the GPU, entity j = bit j & 31 of
    word j >> 5; ``fill`` (0 or 1) goes to every bit at a position >= v."""
    n, v = sets.shape
    w = (v + 31) // 32 + extra_words
    bits = np.full((n, 32 * w), bool(fill))
    bits[:, :v] = sets
    packed = np.packbits(bits, axis=1, bitorder='little').view(np.uint32).astype(np.int64)
    packed = np.where(packed >= 2 ** 31, packed - 2 ** 32, packed).astype(np.int32)
    return torch.from_numpy(packed.reshape(n, w)).cuda()


def _case_host(s, m, v, h):
    """The input recipe of tests/test_gpu_mc_rank.py, its float64 reference and the per-element bound, plus the candidate sets and
    one uniformly drawn set id per query; numpy only."""
    rng = np.random.default_rng(s + m + v + h)
    scale = 0.8 * h ** -0.25
    base = scale * rng.standard_normal((v, h))
    z = (base[None] + 0.5 * scale * rng.standard_normal((s, v, h))).astype(np.float32)
    w = rng.standard_normal((9, h)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(s)).astype(np.float32)
    a, r, b = rng.integers(0, v, m), rng.integers(0, 9, m), rng.integers(0, v, m)
    q = z[:, a] * w[r][None]                                    # one fp32 multiply per element, as ops.mul forms it
    lists = _object_lists(m, v, rng, b)
    known = {}
    for i in range(m):                                          # queries that share (a, r) share their known objects
        known.setdefault((int(a[i]), int(r[i])), set()).update(lists[i].tolist())
    lists = [np.array(sorted(known[(int(a[i]), int(r[i]))]), dtype=np.int64) for i in range(m)]
    q64, z64 = q.astype(np.float64), z.astype(np.float64)
    logit = q64 @ z64.transpose(0, 2, 1) + bias.astype(np.float64)[:, None, None]
    p_s = _sig64(logit)
    pbar = p_s.sum(axis=0) / s
    std = np.sqrt(((p_s - pbar[None]) ** 2).sum(axis=0) / s)
    gamma = (h + 2) * U
    mag = np.abs(q64) @ np.abs(z64).transpose(0, 2, 1) + np.abs(bias.astype(np.float64))[:, None, None]
    eps = (gamma * mag / 4).mean(axis=0) + C_SIG * U + s * U
    sets = _sets(v, s + m + v + h)
    set_id = np.random.default_rng(104729 + s + m + v + h).integers(0, N_SETS, m)
    return dict(z=z, q=q, bias=bias, b_np=b, lists=lists, listed=_dense(lists, v), pbar=pbar, std=std, eps=eps, sets=sets,
                set_id=set_id, member=sets[set_id], shape=(s, m, v, h))


@functools.lru_cache(maxsize=None)
def _case(s, m, v, h):
    """``_case_host`` with its operands on the GPU; computed once per shape and left unchanged."""
    c = _case_host(s, m, v, h)
    lo, hi, ent = _pack(c['lists'])
    c['dev'] = dict(q=torch.from_numpy(c['q']).cuda(), z=torch.from_numpy(c['z']).cuda(), bias=torch.from_numpy(c['bias']).cuda(),
                    b=torch.from_numpy(c['b_np']).cuda(), lo=lo, hi=hi, ent=ent, words=_words(c['sets']),
                    set_id=torch.from_numpy(c['set_id']).cuda())
    return c


def _pools(c):
    """The four candidate pools as dense (m, v) bools, the target left out of every one."""
    m, v = c['pbar'].shape
    other = np.ones((m, v), dtype=bool)
    other[np.arange(m), c['b_np']] = False
    keep = ~c['listed']
    return dict(zip(KINDS, (other, other & keep, other & c['member'], other & c['member'] & keep)))


def _interval(c, counts):
    """(lower, upper) 0-based ranks per query that the bound leaves open, over the candidates that count."""
    pbar, eps, b = c['pbar'], c['eps'], c['b_np']
    rows = np.arange(pbar.shape[0])
    pt, et = pbar[rows, b][:, None], eps[rows, b][:, None]
    lower = ((pbar > pt + eps + et) & counts).sum(axis=1)
    upper = ((pbar >= pt - eps - et) & counts).sum(axis=1)
    return lower, upper


def _assert_inside(c, ranks, label):
    for name, got in zip(KINDS, ranks):
        counts = _pools(c)[name]
        lower, upper = _interval(c, counts)
        got = got.cpu().numpy().astype(np.float64)
        slack = float((upper - lower).sum()) / max(int(counts.sum()), 1)
        print(f'{label} {c["shape"]} {name}: {int((upper - lower).sum())} undecided of {int(counts.sum())} (share {slack:.3e}), '
              f'outside {int(((got < lower) | (got > upper)).sum())} of {len(got)}')
        assert slack <= SLACK_CAP
        assert bool(((got >= lower) & (got <= upper)).all())


@pytest.mark.parametrize('shape', SHAPES)
def test_four_ranks_lie_inside_the_float64_interval_of_their_pool(ops, shape):
    c = _case(*shape)
    d = c['dev']
    out = ops.rank_scores_mc_constrained(d['q'], d['z'], d['b'], d['words'], d['set_id'], d['bias'], d['lo'], d['hi'], d['ent'])
    _assert_inside(c, out[:4], 'fused')
    # the unconstrained outputs are the unconstrained entry's, bit for bit
    raw, filt, tgt = ops.rank_scores_mc(d['q'], d['z'], d['b'], d['bias'], d['lo'], d['hi'], d['ent'])
    assert torch.equal(out[0], raw) and torch.equal(out[1], filt) and torch.equal(out[4], tgt)
    # without a filter: the filtered kinds are None, the others unchanged
    nf = ops.rank_scores_mc_constrained(d['q'], d['z'], d['b'], d['words'], d['set_id'], d['bias'])
    assert nf[1] is None and nf[3] is None and torch.equal(nf[0], raw) and torch.equal(nf[4], tgt)
    lower, upper = _interval(c, _pools(c)['raw_constrained'])
    got = nf[2].cpu().numpy().astype(np.float64)
    assert bool(((got >= lower) & (got <= upper)).all())
    assert bool((out[3] <= out[2]).all()) and bool((out[2] <= out[0]).all()) and bool((out[3] <= out[1]).all())


@pytest.mark.parametrize('shape', SHAPES)
def test_constrained_topk_mean_and_std_against_float64(ops, shape):
    c = _case(*shape)
    d = c['dev']
    s, m, v, h = shape
    k = 10
    ids, mean = ops.topk_scores_mc_constrained(d['q'], d['z'], k, d['words'], d['set_id'], d['bias'], d['lo'], d['hi'], d['ent'])
    std = ops.pair_prob_std_mc(d['q'], d['z'], ids, d['bias'])
    ids, mean, std = ids.cpu().numpy(), mean.cpu().numpy().astype(np.float64), std.cpu().numpy().astype(np.float64)
    pbar, eps = c['pbar'], c['eps']
    worst_mean = worst_std = 0.0
    for i in range(m):
        cand = np.nonzero(c['member'][i] & ~c['listed'][i])[0]           # the members not listed
        kk = min(k, len(cand))
        got = ids[i, :kk]
        assert (ids[i, kk:] == -1).all() and (mean[i, kk:] == -np.inf).all() and (std[i, kk:] == 0).all()
        assert len(set(got.tolist())) == kk and c['member'][i, got].all() and not c['listed'][i, got].any()
        worst_mean = max(worst_mean, float((np.abs(mean[i, :kk] - pbar[i, got]) / eps[i, got]).max(initial=0.0)))
        worst_std = max(worst_std, float((np.abs(std[i, :kk] - c['std'][i, got]) / (1e-5 + 2 * eps[i, got])).max(initial=0.0)))
        assert (np.diff(mean[i, :kk]) <= 0).all()                        # best first
        # nothing returned is decidedly worse than a member left out
        out = np.setdiff1d(cand, got)
        if len(out) and kk:
            assert (pbar[i, got] + eps[i, got]).min() >= (pbar[i, out] - eps[i, out]).max()
        order = cand[np.argsort(-pbar[i, cand], kind='stable')]
        if kk and len(order) > kk:
            kth, nxt = order[kk - 1], order[kk]
            if pbar[i, kth] - pbar[i, nxt] > eps[i, kth] + eps[i, nxt]:
                assert set(got.tolist()) == set(order[:kk].tolist())
    print(f'constrained top-k {shape}: worst |mean - pbar64| / eps {worst_mean:.3f}, worst std error / bound {worst_std:.3f}')
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
    sets = _sets(v, seed + m + v)
    set_id = np.random.default_rng(31 + seed + m + v).integers(0, N_SETS, m)
    return q, e, bias, torch.from_numpy(target).cuda(), lists, sets, set_id


def _dense_probs(ops, q, e, bias, v):
    """Every pbar[i, j] as the device computes it: the unfiltered top-k scorer with k = v, scattered back by id."""
    ids, prob = ops.topk_scores_mc(q, e, v, bias)
    assert bool((ids >= 0).all())
    dense = torch.empty_like(prob)
    dense.scatter_(1, ids, prob)
    assert torch.equal(ids.sort(dim=1).values, torch.arange(v, device='cuda').expand_as(ids))
    return dense


def _same(xs, ys):
    return len(xs) == len(ys) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(xs, ys))


@pytest.mark.parametrize('shape', SMALL)
def test_counts_and_selection_equal_the_recount_from_the_topk_probabilities(ops, ranking, shape):
    s, m, v, h = shape
    q, e, bias, target, lists, sets, set_id = _small_inputs(*shape)
    lo, hi, ent = _pack(lists)
    listed = torch.from_numpy(_dense(lists, v)).cuda()
    mask = torch.from_numpy(sets[set_id]).cuda()
    words, sid = _words(sets), torch.from_numpy(set_id).cuda()
    pbar = _dense_probs(ops, q, e, bias, v)
    out = ops.rank_scores_mc_constrained(q, e, target, words, sid, bias, lo, hi, ent)
    want = ranking.rank_from_scores_constrained(pbar, target, mask, listed)
    assert all(x.dtype == torch.float32 for x in out) and _same(out[:4], want)
    assert torch.equal(out[4], pbar.gather(1, target.view(-1, 1)).view(-1))
    nf = ops.rank_scores_mc_constrained(q, e, target, words, sid, bias)
    assert _same(nf[:4], ranking.rank_from_scores_constrained(pbar, target, mask))
    # the unconstrained outputs equal ops.rank_scores_mc, with and without a filter
    assert _same((out[0], out[1], out[4]), ops.rank_scores_mc(q, e, target, bias, lo, hi, ent))
    assert _same((nf[0], nf[1], nf[4]), ops.rank_scores_mc(q, e, target, bias))
    ks = [min(v, 17)] + ([100] if shape == (3, 70, 128, 24) else [])            # k = 100: the two-keys-per-lane instantiation
    for k in ks:
        for f in ((lo, hi, ent), (None, None, None)):
            ids, prob = ops.topk_scores_mc_constrained(q, e, k, words, sid, bias, *f)
            w_ids, w_prob = ranking.topk_from_scores(pbar, k, *f, cand=mask)
            assert torch.equal(ids, w_ids) and torch.equal(prob, w_prob)


@pytest.mark.parametrize('shape', [(3, 70, 128, 24), (2, 37, 100, 200), (2, 70, 130, 8), (3, 130, 777, 40)])
def test_all_ones_empty_and_out_of_range_sets(ops, shape):
    s, m, v, h = shape
    q, e, bias, target, lists, sets, set_id = _small_inputs(*shape)
    lo, hi, ent = _pack(lists)
    sets = np.zeros((3, v), dtype=bool)
    sets[1] = True                                                   # set 0 and 2 empty, set 1 everything
    words = _words(sets)
    ones = torch.ones(m, dtype=torch.int64, device='cuda')
    for f in ((lo, hi, ent), (None, None, None)):
        raw, filt, tgt = ops.rank_scores_mc(q, e, target, bias, *f)
        out = ops.rank_scores_mc_constrained(q, e, target, words, ones, bias, *f)
        assert _same(out, (raw, filt, raw, filt, tgt))
        for k in (10, 100):
            assert _same(ops.topk_scores_mc_constrained(q, e, k, words, ones, bias, *f), ops.topk_scores_mc(q, e, k, bias, *f))
        # the empty set, and ids on either side of [0, n_sets): rank 0 in both constrained kinds, an all-padding row
        none = torch.tensor([0, 2, -1, 3, 2 ** 31 - 1, -2 ** 31], device='cuda')[torch.arange(m, device='cuda') % 6]
        out = ops.rank_scores_mc_constrained(q, e, target, words, none, bias, *f)
        assert _same((out[0], out[1], out[4]), (raw, filt, tgt))
        assert not out[2].any() and (out[3] is None if f[0] is None else not out[3].any())
        ids, prob = ops.topk_scores_mc_constrained(q, e, 10, words, none, bias, *f)
        assert bool((ids == -1).all()) and bool((prob == float('-inf')).all())
        assert not ops.pair_prob_std_mc(q, e, ids, bias).any()


@pytest.mark.parametrize('shape', [(2, 37, 100, 200), (2, 70, 130, 8), (3, 130, 777, 40)])
def test_padding_bits_and_a_strided_mask_change_nothing(ops, shape):
    s, m, v, h = shape
    q, e, bias, target, lists, sets, set_id = _small_inputs(*shape)
    lo, hi, ent = _pack(lists)
    sid = torch.from_numpy(set_id).cuda()
    w = (v + 31) // 32
    clean = _words(sets)
    rank = ops.rank_scores_mc_constrained(q, e, target, clean, sid, bias, lo, hi, ent)
    top = ops.topk_scores_mc_constrained(q, e, 10, clean, sid, bias, lo, hi, ent)
    garbage = _words(sets, fill=1)                                   # every bit at a position >= v set
    assert v % 32 == 0 or not torch.equal(garbage, clean)
    wide = _words(sets, extra_words=3, fill=1)                       # ld_cand = W + 3, the padding words all ones
    strided = wide[:, :w]
    assert strided.stride(0) == w + 3 and not strided.is_contiguous()
    uint = clean.view(torch.uint32)
    for words in (garbage, strided, uint):
        assert _same(ops.rank_scores_mc_constrained(q, e, target, words, sid, bias, lo, hi, ent), rank)
        assert _same(ops.topk_scores_mc_constrained(q, e, 10, words, sid, bias, lo, hi, ent), top)


@pytest.mark.parametrize('shape,first', [((2, 70, 130, 8), 128), ((3, 70, 777, 40), 768)])
def test_odd_word_count_with_members_in_the_last_tile_only(ops, ranking, shape, first):
    """v = 130 is W = 5 words, v = 777 is W = 25: the last 64-column tile has ONE word of the set, and the members sit there only.
    The reference is the recount on the sub-table of the members and the targets (<= 128 entities: k = v' returns every
    probability; an element's value does not depend on its column)."""
    s, m, v, h = shape
    q, e, bias, target, lists, _, _ = _small_inputs(*shape)
    assert ((v + 31) // 32) % 2 == 1 and first == 64 * ((v - 1) // 64)
    sets = np.zeros((3, v), dtype=bool)
    sets[0, first:] = True
    sets[1, [first, v - 1]] = True
    sets[2, v - 1] = True
    set_id = np.arange(m) % 3
    words, sid = _words(sets), torch.from_numpy(set_id).cuda()
    sub = np.unique(np.concatenate([np.arange(first, v), target.cpu().numpy()]))
    assert len(sub) <= 128
    sub_t = torch.from_numpy(sub).cuda()
    pbar = _dense_probs(ops, q, e[:, sub_t].contiguous(), bias, len(sub))
    mask = torch.from_numpy(sets[set_id][:, sub]).cuda()
    t_sub = torch.from_numpy(np.searchsorted(sub, target.cpu().numpy())).cuda()
    out = ops.rank_scores_mc_constrained(q, e, target, words, sid, bias)
    want = ranking.rank_from_scores_constrained(pbar, t_sub, mask)
    assert torch.equal(out[2], want[2]) and torch.equal(out[4], pbar.gather(1, t_sub.view(-1, 1)).view(-1))
    ids, prob = ops.topk_scores_mc_constrained(q, e, 12, words, sid, bias)
    w_ids, w_prob = ranking.topk_from_scores(pbar, 12, cand=mask)
    w_ids = torch.where(w_ids >= 0, sub_t[w_ids.clamp(min=0)], w_ids)
    assert torch.equal(ids, w_ids) and torch.equal(prob, w_prob)
    assert bool(((ids >= first) | (ids == -1)).all())


@pytest.mark.parametrize('shape', [(1, 70, 130, 8), (1, 37, 1000, 200)])
def test_a_sample_given_twice_is_the_sample_and_one_sample_keeps_the_logit_order(ops, shape):
    s, m, v, h = shape
    q, e, bias, target, lists, sets, set_id = _small_inputs(*shape)
    lo, hi, ent = _pack(lists)
    words, sid = _words(sets), torch.from_numpy(set_id).cuda()
    q2, e2, b2 = q.repeat(2, 1, 1), e.repeat(2, 1, 1), bias.repeat(2)            # p + p and * 0.5f are exact
    assert _same(ops.rank_scores_mc_constrained(q, e, target, words, sid, bias, lo, hi, ent),
                 ops.rank_scores_mc_constrained(q2, e2, target, words, sid, b2, lo, hi, ent))
    ids1, prob1 = ops.topk_scores_mc_constrained(q, e, 10, words, sid, bias, lo, hi, ent)
    assert _same((ids1, prob1), ops.topk_scores_mc_constrained(q2, e2, 10, words, sid, b2, lo, hi, ent))
    # one sample: the key's value is sigmoid of the single-sample scorer's logit, so the order is its order wherever those differ
    l_ids, _ = ops.topk_scores_constrained(q[0], e[0], 10, words, sid, bias, lo, hi, ent)
    distinct = (prob1[:, 1:] != prob1[:, :-1]).all(dim=1)
    assert bool(distinct.any()) and torch.equal(ids1[distinct], l_ids[distinct])


def test_permuted_queries_with_their_set_ids(ops):
    s, m, v, h = 3, 130, 300, 40
    q, e, bias, target, lists, sets, set_id = _small_inputs(s, m, v, h)
    lo, hi, ent = _pack(lists)
    words, sid = _words(sets), torch.from_numpy(set_id).cuda()
    rank = ops.rank_scores_mc_constrained(q, e, target, words, sid, bias, lo, hi, ent)
    ids, prob = ops.topk_scores_mc_constrained(q, e, 10, words, sid, bias, lo, hi, ent)
    pm = torch.randperm(m, generator=torch.Generator().manual_seed(9))
    lo_p, hi_p, ent_p = _pack([lists[i] for i in pm.tolist()])
    pm = pm.cuda()
    qp = q[:, pm].contiguous()
    rank_p = ops.rank_scores_mc_constrained(qp, e, target[pm], words, sid[pm], bias, lo_p, hi_p, ent_p)
    assert _same(rank_p, tuple(x[pm] for x in rank))
    ids_p, prob_p = ops.topk_scores_mc_constrained(qp, e, 10, words, sid[pm], bias, lo_p, hi_p, ent_p)
    assert torch.equal(ids_p, ids[pm]) and torch.equal(prob_p, prob[pm])


def test_ties_nan_and_saturation(ops):
    s, h, v = 2, 8, 100
    gen = torch.Generator().manual_seed(0)
    e = (torch.randn(s, v, h, generator=gen) * 0.5).cuda()
    e[:, 7] = e[:, 3]
    e[:, 99] = e[:, 3]
    e[:, 90] = e[:, 3]
    sets = np.zeros((2, v), dtype=bool)
    sets[0, [3, 7, 99, 10, 40, 41, 42]] = True                       # 90 (a tie) and 20 are no members
    sets[1, ::2] = True                                              # the 50 even ids
    words = _words(sets)
    zero = torch.zeros(1, dtype=torch.int64, device='cuda')
    q = e[:, [3, 3]].clone()
    target = torch.tensor([3, 7], device='cuda')
    lo, hi, ent = _pack([np.array([7]), np.array([3, 90])])
    out = ops.rank_scores_mc_constrained(q, e, target, words, zero.repeat(2), None, lo, hi, ent)
    pbar = _dense_probs(ops, q, e, None, v)
    above = [sum(int(pbar[i, j] > pbar[i, int(target[i])]) for j in (10, 40, 41, 42)) for i in range(2)]
    # duplicate member rows share the mid-rank: of the ties 7 / 3, 99 (members) and 90 (not one), two count half each
    assert float(out[2][0]) == above[0] + 1.0 and float(out[3][0]) == above[0] + 0.5          # 7 listed
    assert float(out[2][1]) == above[1] + 1.0 and float(out[3][1]) == above[1] + 0.5          # 3 listed (90 is no member anyway)
    # a NaN in ONE sample of a member counts as above; a NaN non-member counts nowhere in the constrained kinds
    bad = e.clone()
    bad[1, 10] = float('nan')                                        # member
    bad[0, 20] = float('nan')                                        # non-member
    qq, t3 = e[:, [3]].clone(), torch.tensor([3], device='cuda')
    pb = _dense_probs(ops, qq, e, None, v)[0]
    b = sum(int(pb[j] > pb[3]) for j in (40, 41, 42))
    out = ops.rank_scores_mc_constrained(qq, bad, t3, words, zero, None, zero, zero + 1, torch.tensor([20], device='cuda'))
    all_above = int((pb > pb[3]).sum()) - int(pb[10] > pb[3]) - int(pb[20] > pb[3])
    assert float(out[0][0]) == all_above + 2 + 1.5 and float(out[1][0]) == all_above + 1 + 1.5
    assert float(out[2][0]) == b + 1 + 1.0 and float(out[3][0]) == b + 1 + 1.0               # ties 7, 99; NaN member 10 above
    out = ops.rank_scores_mc_constrained(qq, bad, t3, words, zero, None, zero, zero + 1, torch.tensor([10], device='cuda'))
    assert float(out[2][0]) == b + 1 + 1.0 and float(out[3][0]) == b + 1.0                   # the NaN member, listed
    ids, prob = ops.topk_scores_mc_constrained(qq, bad, 10, words, zero, None)
    assert ids[0, 6].item() == 10 and bool(torch.isnan(prob[0, 6])) and ids[0, 7:].tolist() == [-1, -1, -1]     # NaN after everything
    assert 20 not in ids[0].tolist() and 90 not in ids[0].tolist()
    # a NaN target ranks last among the members
    bad_t = e.clone()
    bad_t[1, 3] = float('nan')
    out = ops.rank_scores_mc_constrained(qq, bad_t, t3, words, zero, None, zero, zero + 5, torch.tensor([0, 1, 2, 7, 40], device='cuda'))
    assert float(out[0][0]) == v - 1 and float(out[2][0]) == 6 and float(out[3][0]) == 4 and bool(torch.isnan(out[4][0]))
    # all-saturated tables: the middle rank of the set, the target a member (0) or not (65); ties by lower id in the top-k
    big = e.clone() * 0 + torch.linspace(5.0, 6.0, v, device='cuda').view(1, v, 1)
    tq = torch.tensor([0, 65], device='cuda')
    lo2, hi2 = torch.tensor([0, 0], device='cuda'), torch.tensor([10, 10], device='cuda')
    ones2 = torch.ones(s, 2, h, device='cuda')
    out = ops.rank_scores_mc_constrained(ones2, big, tq, words, zero.repeat(2) + 1, None, lo2, hi2, torch.arange(10, device='cuda'))
    assert torch.equal(out[4].cpu(), torch.ones(2)) and torch.equal(out[0].cpu(), torch.full((2,), (v - 1) / 2.0))
    assert out[2].tolist() == [49 / 2.0, 50 / 2.0] and out[3].tolist() == [(49 - 4) / 2.0, (50 - 5) / 2.0]
    ids, prob = ops.topk_scores_mc_constrained(ones2, big, 5, words, zero.repeat(2) + 1, None)
    assert ids.tolist() == [[0, 2, 4, 6, 8]] * 2 and bool((prob == 1).all())


def test_argument_errors(ops):
    from gcn_vae_amd import lib
    q, e = torch.zeros(2, 4, 8, device='cuda'), torch.zeros(2, 50, 8, device='cuda')
    t = torch.zeros(4, dtype=torch.int64, device='cuda')
    lo, hi, ent = t.clone(), t.clone() + 2, torch.arange(2, device='cuda')
    cand, sets = torch.zeros(3, 2, dtype=torch.int32, device='cuda'), t.clone()
    bias = torch.zeros(2, device='cuda')
    ops.rank_scores_mc_constrained(q, e, t, cand, sets, bias, lo, hi, ent)
    ops.topk_scores_mc_constrained(q, e, 3, cand, sets, bias, lo, hi, ent)
    for call in (lambda **kw: ops.rank_scores_mc_constrained(kw.get('q', q), kw.get('e', e), kw.get('t', t), kw.get('cand', cand),
                                                             kw.get('sets', sets), kw.get('bias'), *kw.get('f', (None,) * 3)),
                 lambda **kw: ops.topk_scores_mc_constrained(kw.get('q', q), kw.get('e', e), kw.get('k', 3), kw.get('cand', cand),
                                                             kw.get('sets', sets), kw.get('bias'), *kw.get('f', (None,) * 3))):
        with pytest.raises(ValueError, match='samples'):
            call(e=e[:1])
        with pytest.raises(ValueError, match='bias'):
            call(bias=torch.zeros(3, device='cuda'))                             # one bias per sample
        with pytest.raises(ValueError, match='width'):
            call(e=e[:, :, :4])
        with pytest.raises(TypeError):
            call(q=q[0], e=e[0])                                                 # the single-sample operands
        with pytest.raises(ValueError):
            call(f=(lo, hi + 1, ent))                                            # a range past the end of the list
        with pytest.raises(ValueError):
            call(f=(lo, hi, ent + 50))                                           # ids out of [0, v)
        with pytest.raises(ValueError):
            call(f=(lo, None, ent))                                              # all of the filter or none
        with pytest.raises(ValueError, match='words per set'):
            call(cand=cand[:, :1])                                               # fewer than ceil(v / 32) words
        with pytest.raises(TypeError, match='bitmask'):
            call(cand=cand.float())
        with pytest.raises(RuntimeError, match='cand'):
            call(cand=cand.cpu())
        with pytest.raises(ValueError, match='set id per query'):
            call(sets=sets[:3])
    with pytest.raises(ValueError):
        ops.rank_scores_mc_constrained(q, e, t + 50, cand, sets)                 # targets out of [0, v)
    with pytest.raises(ValueError, match='one target'):
        ops.rank_scores_mc_constrained(q, e, t[:3], cand, sets)
    with pytest.raises(ValueError, match='k must lie'):
        ops.topk_scores_mc_constrained(q, e, ops.TOPK_MAX + 1, cand, sets)
    # no queries: nothing launched
    r0 = ops.rank_scores_mc_constrained(q[:, :0], e, t[:0], cand, sets[:0])
    assert r0[0].numel() == 0 and r0[1] is None and r0[2].numel() == 0
    assert tuple(ops.topk_scores_mc_constrained(q[:, :0], e, 3, cand, sets[:0])[0].shape) == (0, 3)
    # the raw entries refuse n_sets = 0, a short ld_cand, a short sample stride and half a filter
    p = lib.ptr
    tgt, cnt = torch.zeros(4, device='cuda'), torch.zeros(4, 4, dtype=torch.int32, device='cuda')
    t32, s32, lo32, ent32 = t.int(), sets.int(), lo.int(), ent.int()

    def rank(q_stride=32, n_sets=3, ld_cand=2, f=(None, None, None)):
        lib.call('gv_rank_scores_mc_constrained', p(q), 8, q_stride, p(e), 8, 400, 2, p(t32), None, *f, 2 if f[2] is not None else 0,
                 p(cand), ld_cand, n_sets, p(s32), p(tgt), p(cnt[0]), p(cnt[1]), p(cnt[2]), p(cnt[3]), 4, 50, 8, lib.stream())

    ids, prob = torch.zeros(4, 3, dtype=torch.int32, device='cuda'), torch.zeros(4, 3, device='cuda')
    ws = torch.empty(int(lib.load().gv_topk_scores_workspace_bytes(4, 50, 3)), dtype=torch.uint8, device='cuda')

    def topk(q_stride=32, n_sets=3, ld_cand=2, f=(None, None, None)):
        lib.call('gv_topk_scores_mc_constrained', p(q), 8, q_stride, p(e), 8, 400, 2, None, *f, 2 if f[2] is not None else 0,
                 p(cand), ld_cand, n_sets, p(s32), 3, p(ids), p(prob), p(ws), 4, 50, 8, lib.stream())

    for entry in (rank, topk):
        entry()
        with pytest.raises(RuntimeError, match='n_sets'):
            entry(n_sets=0)
        with pytest.raises(RuntimeError, match='ld_cand'):
            entry(ld_cand=1)
        with pytest.raises(RuntimeError, match='stride'):
            entry(q_stride=31)
        with pytest.raises(RuntimeError, match='all given or all NULL'):
            entry(f=(p(lo32), None, p(ent32)))


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
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    return kg, net, (graph, node_id, torch.from_numpy(rel).cuda(), enorm), fi, tc


MC_SEED = 11


def _host_restatement(ranking, kg, z, w, flps, a, b, r, side):
    """float64 on the host, from the triplet sets themselves: per query and kind the interval of 0-based ranks that the
    per-element bound leaves open, and per kind the undecided and the counted comparisons."""
    z64, w64, f64 = z.cpu().double(), w.detach().cpu().double(), flps.cpu().double()
    trips = np.concatenate([kg.train, kg.valid, kg.test]).tolist()
    known = {tuple(x) for x in trips}
    seen = {(x[1], x[0 if side == 's' else 2]) for x in trips}       # (relation, entity seen on the side that is asked for)
    n, h, s = kg.num_nodes, z.shape[2], z.shape[0]
    pbar = ranking.mc_mean_prob(z64, w64, a, r, f64).numpy()
    mag = torch.einsum('smh,svh->smv', (z64[:, a] * w64[r]).abs(), z64.abs()).numpy() + f64.abs().numpy()[:, None, None]
    eps = ((h + 2) * U * mag / 4).mean(axis=0) + C_SIG * U + s * U
    out = {kind: ([], []) for kind in KINDS}
    undecided, counted = dict.fromkeys(KINDS, 0), dict.fromkeys(KINDS, 0)
    for i in range(len(a)):
        t, qa, rel = int(b[i]), int(a[i]), int(r[i])
        listed = np.array([((j, rel, qa) if side == 's' else (qa, rel, j)) in known for j in range(n)])
        member = np.array([(rel, j) in seen for j in range(n)])
        for kind, counts in zip(KINDS, (np.ones(n, dtype=bool), ~listed, member, member & ~listed)):
            counts = counts.copy()
            counts[t] = False
            band = eps[i] + eps[i, t]
            lower = int((pbar[i] > pbar[i, t] + band)[counts].sum())
            upper = int((pbar[i] >= pbar[i, t] - band)[counts].sum())
            out[kind][0].append(lower)
            out[kind][1].append(upper)
            undecided[kind] += upper - lower
            counted[kind] += int(counts.sum())
    return out, undecided, counted


def test_calc_mc_constrained_mrr_end_to_end(ranking):
    """Real posterior samples of the seeded 400-entity model, S = 4, against a float64 restatement on the host that takes the sets
    from the triplets themselves: the raw and filtered figures are calc_mc_mrr's exactly, every kind's ranks lie in the interval
    the per-element bound leaves open and its MRR / Hits between the figures at the interval's two ends to 1e-6, the undecided
    comparisons of each kind stay within SLACK_CAP of those counted, and the materialised route is held to the same intervals."""
    kg, net, inputs, fi, tc = _model()
    z, flps = net.encoder.posterior_samples(*inputs, 4, seed=MC_SEED)
    test = torch.from_numpy(kg.test).cuda()
    hits = [1, 3, 10]
    out = ranking.calc_mc_constrained_mrr(z, net.w_relation, test, fi, tc, flps, hits=hits, eval_bz=50, verbose=False)
    assert out['n_samples'] == 4 and set(out) == {'n_samples'} | {p + k for p in ('mrr_', 'hits_') for k in KINDS}
    plain = ranking.calc_mc_mrr(z, net.w_relation, test, fi, flps, hits=hits, verbose=False)
    for kind in ('raw', 'filtered'):
        assert out['mrr_' + kind] == plain['mrr_' + kind] and out['hits_' + kind] == plain['hits_' + kind]
    no_filter = ranking.calc_mc_constrained_mrr(z, net.w_relation, test, None, tc, flps, hits=hits, verbose=False)
    assert set(no_filter) == {'n_samples', 'mrr_raw', 'hits_raw', 'mrr_raw_constrained', 'hits_raw_constrained'}
    assert no_filter['mrr_raw_constrained'] == out['mrr_raw_constrained']
    s_, r_, o_ = test[:, 0], test[:, 1], test[:, 2]
    got, ends = {k: [] for k in KINDS}, {k: ([], []) for k in KINDS}
    undecided, counted = dict.fromkeys(KINDS, 0), dict.fromkeys(KINDS, 0)
    for a, b, side in ((o_, s_, 's'), (s_, o_, 'o')):
        ranks = ranking.perturb_and_get_rank_mc_constrained(z, net.w_relation, a, r_, b, len(b), fi, tc, side, flow_log_probs=flps)
        iv, n_open, n_all = _host_restatement(ranking, kg, z, net.w_relation, flps, a.cpu(), b.cpu(), r_.cpu(), side)
        for kind, rk in zip(KINDS, ranks):
            got[kind].append(rk.cpu().double())
            ends[kind][0].extend(iv[kind][0])
            ends[kind][1].extend(iv[kind][1])
            undecided[kind] += n_open[kind]
            counted[kind] += n_all[kind]
    unfused = ranking.calc_mc_constrained_mrr_unfused(z, net.w_relation, test, fi, tc, flps, hits=hits, verbose=False)
    for kind in KINDS:
        print(f'end to end {kind}: {undecided[kind]} undecided of {counted[kind]} comparisons')
        assert undecided[kind] <= SLACK_CAP * counted[kind]
        rk = torch.cat(got[kind])
        lower, upper = (torch.tensor(x, dtype=torch.float64) for x in ends[kind])
        assert bool(((rk >= lower) & (rk <= upper)).all())
        assert abs(out['mrr_' + kind] - float((1.0 / (rk + 1)).mean())) < 1e-6
        lo_mrr, hi_mrr = float((1.0 / (upper + 1)).mean()) - 1e-6, float((1.0 / (lower + 1)).mean()) + 1e-6
        assert lo_mrr <= out['mrr_' + kind] <= hi_mrr and lo_mrr <= unfused['mrr_' + kind] <= hi_mrr
        for k in hits:
            lo_h, hi_h = float((upper + 1 <= k).double().mean()) - 1e-6, float((lower + 1 <= k).double().mean()) + 1e-6
            assert lo_h <= out['hits_' + kind][k] <= hi_h and lo_h <= unfused['hits_' + kind][k] <= hi_h
    assert out['mrr_filtered_constrained'] >= out['mrr_raw_constrained'] >= out['mrr_raw']
    assert out['mrr_filtered_constrained'] >= out['mrr_filtered']
    # the constrained proposals, fused and materialised: members only, new facts only, the same entities where both are padded
    ids, mean, std = ranking.predict_topk_mc(z, net.w_relation, s_, r_, 5, 'o', fi, flps, type_constraint=tc)
    u_ids, u_mean, u_std = ranking.predict_topk_mc_unfused(z, net.w_relation, s_, r_, 5, 'o', fi, flps, type_constraint=tc)
    real = ids >= 0
    assert torch.equal(real, u_ids >= 0) and bool(real.any())
    assert bool(tc.contains(r_.view(-1, 1).expand_as(ids)[real], ids[real], 'o').all())
    agree = real & (ids == u_ids)                                    # (two near-equal means may come out in either order)
    assert float((mean[real] - u_mean[real]).abs().max()) < 1e-5 and float((std - u_std)[agree].abs().max()) < 1e-5
    assert int(agree.sum()) >= 0.9 * int(real.sum())
    assert bool((mean[~real] == float('-inf')).all()) and not std[~real].any()
    # no constraint: today's path
    assert _same(ranking.predict_topk_mc(z, net.w_relation, s_, r_, 5, 'o', fi, flps, None),
                 ranking.predict_topk_mc(z, net.w_relation, s_, r_, 5, 'o', fi, flps))


def test_cli_reports_four_kinds_and_writes_type_correct_mc_predictions(ops, ranking, tmp_path, capsys, monkeypatch):
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
            '--test-mode', 'True', '--model-state-file', ckpt, '--predict-topk', '3', '--filtered-eval', '--mc-samples', '4',
            '--mc-seed', '5']
    runs = {}
    for name, extra in (('mc', []), ('typed', ['--mc-type-constrain']), ('again', ['--mc-type-constrain'])):
        out, mc_out = str(tmp_path / f'{name}.tsv'), str(tmp_path / f'{name}_mc.tsv')
        # the same noise in every run: the device RNG restarts when torch's seed changes, and a model's draws are keyed by the
        # process-unique stream ids it takes at construction -- every run's model gets the same ones
        torch.manual_seed(2)
        ops.device_rng(torch.device('cuda', 0)).tick()
        torch.manual_seed(1)
        monkeypatch.setattr(ops, '_rng_streams', itertools.count(1 << 20))
        mrr = train.main(train.build_parser().parse_args(base + extra + ['--predict-out', out, '--mc-predict-out', mc_out]))
        runs[name] = (mrr, open(out).read(), capsys.readouterr().out.replace(out, 'OUT').replace(mc_out, 'MC_OUT'), open(mc_out).read())
    assert runs['mc'][0] == runs['typed'][0] and runs['mc'][1] == runs['typed'][1]        # the single-draw results are untouched
    assert runs['typed'][3] == runs['again'][3] and runs['typed'][2] == runs['again'][2]  # the same seed: the same file and report
    report = runs['typed'][2]
    for kind in KINDS:
        assert f'MC MRR ({kind}, 4 samples)' in report and f'MC Hits ({kind}) @ 10' in report
    assert 'MC MRR (raw_constrained' not in runs['mc'][2]
    # the unconstrained kinds are printed as without the flag
    for line in runs['mc'][2].splitlines():
        if line.startswith('MC MRR') or line.startswith('MC Hits'):
            assert line in report.splitlines()
    tc = ranking.TypeConstraint(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test)
    rows = [line.rstrip('\n').split('\t') for line in runs['typed'][3].splitlines()]
    n_test = len(kg.test)
    assert len(rows) == 2 * n_test * 3 and all(len(x) == 7 for x in rows)                 # the layout is unchanged
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    proposed = 0
    for j, d in enumerate(('o', 's')):
        block = rows[j * n_test * 3:(j + 1) * n_test * 3]
        assert all(x[0] == d for x in block) and [int(x[3]) for x in block] == [0, 1, 2] * n_test
        assert [int(x[1]) for x in block[::3]] == kg.test[:, 0 if d == 'o' else 2].tolist()
        for x in block:
            qa, rel, e_, mean, std = int(x[1]), int(x[2]), int(x[4]), float(x[5]), float(x[6])
            if e_ < 0:
                assert e_ == -1 and mean == float('-inf') and std == 0.0
                continue
            proposed += 1
            assert ((qa, rel, e_) if d == 'o' else (e_, rel, qa)) not in known                # new facts only
            assert bool(tc.contains(torch.tensor([rel]), torch.tensor([e_]), d)[0])           # type-correct
            assert 0.0 <= mean <= 1.0 and 0.0 <= std <= 0.5
    assert proposed > 0
    assert runs['typed'][3] != runs['mc'][3]                            # the unconstrained file proposes other entities somewhere
