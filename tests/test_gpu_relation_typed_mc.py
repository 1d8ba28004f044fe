"""Relation prediction under type sets and on the posterior predictive, on the GPU: gv_pair_rel_scores_constrained / _mc /
_mc_constrained and gv_transe_pair_rel_constrained through ops.pair_relation_scores(cand=), ops.pair_relation_scores_mc,
ops.transe_pair_relations(cand=), the ranking / transe drivers and both CLIs.

Exact checks (torch.equal, values by their bits): the constrained entries against their materialised twins (ranking.mid_ranks with
a cand_mask, topk_from_scores(cand=)) and against the unconstrained entry; the MC entries against the existing MC kernels composed
on the stacks q = mul(z[:, s], z[:, o]), entities = w repeated per sample.  Float64 check: the MC ranks inside the interval of
tests/test_gpu_mc_rank.py (same constants, same eps formula).  pytest -m gpu."""
import functools

import numpy as np
import pytest
import torch

import relation_cases as rc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_SIG = 4.0                # tests/test_gpu_mc_rank.py: measured 1.83 u (NOTES.md), doubled and rounded up
SLACK_CAP = 0.002
SAMPLES = (1, 2, 3, 4, 16)
MC_F64_SHAPES = [(1, 1, 1, 7), (3, 63, 11, 16), (4, 64, 64, 24), (2, 65, 65, 200), (3, 130, 130, 7), (4, 130, 237, 200),
                 (16, 65, 237, 24), (1, 130, 237, 200)]          # (S, m, R, h)


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def ranking():
    from gcn_vae_amd import ranking as _ranking
    return _ranking


@pytest.fixture(scope='module')
def transe():
    from gcn_vae_amd import transe as _transe
    return _transe


def _tables(num_rels, h, gen):
    return (torch.randn(rc.N, h, generator=gen) * 0.5).cuda(), torch.randn(num_rels, h, generator=gen).cuda()


def relation_masks(num_rels, gen):
    """The (2 N, ceil(R / 32)) int32 relation bitmask, its kinds cycling by entity id on both sides: none, all, dense (p = 0.7),
    sparse (p = 0.1), only the window 64..127 (where it exists, else dense), only relation R - 1, and every bit of every word
    set -- the columns >= num_rels among them, which the kernels must ignore.  Returns (cand on the device, dense bool (2 N, R))."""
    n_words = (num_rels + 31) // 32
    dense = torch.zeros(2 * rc.N, num_rels, dtype=torch.bool)
    beyond = torch.zeros(2 * rc.N, dtype=torch.bool)
    for row in range(2 * rc.N):
        kind = (row % rc.N + (3 if row >= rc.N else 0)) % 7
        if kind == 1:
            dense[row] = True
        elif kind == 2 or (kind == 4 and num_rels <= 64):
            dense[row] = torch.rand(num_rels, generator=gen) < 0.7
        elif kind == 3:
            dense[row] = torch.rand(num_rels, generator=gen) < 0.1
        elif kind == 4:
            dense[row, 64:128] = True
        elif kind == 5:
            dense[row, num_rels - 1] = True
        elif kind == 6:
            dense[row] = True
            beyond[row] = True
    bits = torch.zeros(2 * rc.N, n_words * 32, dtype=torch.long)
    bits[:, :num_rels] = dense.long()
    bits[beyond] = 1
    words = (bits.view(2 * rc.N, n_words, 32) << torch.arange(32)).sum(2)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return words.cuda(), dense.cuda()


def _pair_mask(dense, s, o):
    return dense[s] & dense[rc.N + o]


def _case(m, num_rels, h, k, seed=0):
    gen = torch.Generator().manual_seed(m * 7 + num_rels + h + k + seed)
    emb, w = _tables(num_rels, h, gen)
    s, o = rc.pairs(m, gen)
    if m > 2:
        s[1], o[1] = 0, 4              # kinds none x all: no type-correct relation at all
    target = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    cand, dense = relation_masks(num_rels, gen)
    filt = rc.relation_lists(m, num_rels, target.cpu(), gen)
    return emb, w, s, o, target, cand, _pair_mask(dense, s, o), filt


def _check_constrained(fused, unconstrained, twin, s, o, target, k, cand, mask, filt, pad_value):
    """One model's constrained entry against its twin and its unconstrained entry, with and without a filter, ranks only, list
    only and both in one call."""
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    for given in ({}, names):
        ranks, top = fused(target=target, k=k, cand=cand, **given)
        want_ranks, want_top = twin(mask, tuple(given.values()) if given else (None, None, None))
        plain_ranks, _ = unconstrained(target=target, k=k, **given)
        assert len(ranks) == 4
        for got, want in zip(ranks, want_ranks):
            assert (got is None and want is None) or torch.equal(got, want)
        assert (ranks[1] is None) == (not given) and (ranks[3] is None) == (not given)
        assert torch.equal(ranks[0], plain_ranks[0]) and (not given or torch.equal(ranks[1], plain_ranks[1]))
        assert rc.same_lists(top, want_top)
        ranks_only, none = fused(target=target, cand=cand, **given)
        nothing, top_only = fused(k=k, cand=cand, **given)
        assert none is None and nothing is None and rc.same_lists(top_only, top)
        assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(ranks_only, ranks))
        bare = ~mask.any(1)                                                # rows without any type-correct relation
        assert bool((ranks[2][bare] == 0).all()) and bool((top[0][bare] == -1).all()) and bool((top[1][bare] == pad_value).all())
        assert bool(((top[0] < 0) | mask.gather(1, top[0].clamp(min=0))).all())       # only type-correct relations are proposed
    return ranks, top


@pytest.mark.parametrize('m,num_rels,h,k', rc.SHAPES)
def test_constrained_distmult_equals_the_twin(ops, ranking, m, num_rels, h, k):
    emb, w, s, o, target, cand, mask, filt = _case(m, num_rels, h, k)
    bias = torch.tensor([0.25]).cuda()
    score = ranking.pair_scores_unfused(emb, w, s, o, bias)
    ranks, _ = _check_constrained(
        lambda **kw: ops.pair_relation_scores(emb, w, s, o, bias=bias, **kw),
        lambda **kw: ops.pair_relation_scores(emb, w, s, o, bias=bias, **kw),
        lambda mk, f: (ranking.relation_ranks_from_scores(score, target, *f, cand_mask=mk), ranking.topk_from_scores(score, k, *f, cand=mk)),
        s, o, target, k, cand, mask, filt, float('-inf'))
    if m > 2:
        assert not bool(mask[1].any()) and ranks[2][1] == 0 and ranks[3][1] == 0
    empty = ops.pair_relation_scores(emb, w, s[:0], o[:0], target=target[:0], k=k, cand=cand)
    assert len(empty[0]) == 4 and empty[0][2].shape == (0,) and empty[1][0].shape == (0, k)


@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('m,num_rels,h,k', rc.SHAPES)
def test_constrained_transe_equals_the_twin(ops, ranking, transe, m, num_rels, h, k, p_norm):
    en, rn, s, o, target, cand, mask, filt = _case(m, num_rels, h, k, seed=p_norm)
    dist = transe.pair_distances_unfused(en, rn, s, o, p_norm)
    _check_constrained(
        lambda **kw: ops.transe_pair_relations(en, rn, s, o, p_norm, **kw),
        lambda **kw: ops.transe_pair_relations(en, rn, s, o, p_norm, **kw),
        lambda mk, f: (ranking.relation_ranks_from_scores(-dist, target, *f, cand_mask=mk), transe.topk_from_distances(dist, k, *f, cand=mk)),
        s, o, target, k, cand, mask, filt, float('inf'))


# ---- the posterior predictive -----------------------------------------------------------------------------------------------------
def _mc_case(n_samples, m, num_rels, h, k):
    gen = torch.Generator().manual_seed(n_samples * 1000 + m * 7 + num_rels + h + k)
    base = torch.randn(rc.N, h, generator=gen) * 0.5
    z = (base + 0.3 * torch.randn(n_samples, rc.N, h, generator=gen)).cuda()
    w = torch.randn(num_rels, h, generator=gen).cuda()
    bias = (0.5 * torch.randn(n_samples, generator=gen)).cuda()
    s, o = rc.pairs(m, gen)
    target = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    cand, dense = relation_masks(num_rels, gen)
    filt = rc.relation_lists(m, num_rels, target.cpu(), gen)
    return z, w, bias, s, o, target, cand, _pair_mask(dense, s, o), filt


def _stacks(ops, z, w, s, o):
    return ops.mul(z[:, s].contiguous(), z[:, o].contiguous()), w.unsqueeze(0).repeat(z.shape[0], 1, 1)


@pytest.mark.parametrize('case', range(len(rc.SHAPES)))
def test_mc_equals_the_composed_mc_kernels(ops, case):
    (m, num_rels, h, k), n_samples = rc.SHAPES[case], SAMPLES[case % len(SAMPLES)]
    z, w, bias, s, o, target, cand, mask, filt = _mc_case(n_samples, m, num_rels, h, k)
    q, ent = _stacks(ops, z, w, s, o)
    rows = cand[s] & cand[rc.N + o]
    sets = torch.arange(m, device='cuda')
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    for b in (bias, None):
        for given in ({}, names):
            f = tuple(given.values()) if given else (None, None, None)
            ranks, top, tgt = ops.pair_relation_scores_mc(z, w, s, o, target=target, k=k, bias=b, **given)
            raw, filtered, want_tgt = ops.rank_scores_mc(q, ent, target, b, *f)
            assert len(ranks) == 2 and torch.equal(ranks[0], raw) and rc.same_values(tgt, want_tgt)
            assert (ranks[1] is None and filtered is None) or torch.equal(ranks[1], filtered)
            assert rc.same_lists(top, ops.topk_scores_mc(q, ent, k, b, *f))
            ranks_c, top_c, tgt_c = ops.pair_relation_scores_mc(z, w, s, o, target=target, k=k, bias=b, cand=cand, **given)
            want = ops.rank_scores_mc_constrained(q, ent, target, rows, sets, b, *f)
            assert len(ranks_c) == 4 and rc.same_values(tgt_c, want[4]) and rc.same_values(tgt_c, tgt)
            assert all((a is None and c is None) or torch.equal(a, c) for a, c in zip(ranks_c, want[:4]))
            assert rc.same_lists(top_c, ops.topk_scores_mc_constrained(q, ent, k, rows, sets, b, *f))
            assert bool(((top_c[0] < 0) | mask.gather(1, top_c[0].clamp(min=0))).all())
    # the target's pbar is the list's value of the same relation
    kk = min(num_rels, 128)
    (ids, val), tgt = ops.pair_relation_scores_mc(z, w, s, o, target=target, k=kk, bias=bias)[1:]
    hit = ids == target.view(-1, 1)
    assert bool(hit.any(1).all()) or num_rels > 128
    assert rc.same_values(val[hit], tgt[hit.any(1)])


@pytest.mark.parametrize('m,num_rels,h,k', [rc.SHAPES[1], rc.SHAPES[5]])
def test_mc_sample_twice_saturation_and_nan(ops, m, num_rels, h, k):
    z, w, bias, s, o, target, cand, mask, filt = _mc_case(1, m, num_rels, h, k)
    one = ops.pair_relation_scores_mc(z, w, s, o, target=target, k=k, bias=bias, cand=cand)
    two = ops.pair_relation_scores_mc(z.repeat(2, 1, 1), w, s, o, target=target, k=k, bias=bias.repeat(2), cand=cand)
    assert all(torch.equal(a, b) for a, b in zip(one[0][::2], two[0][::2])) and rc.same_lists(one[1], two[1])
    assert rc.same_values(one[2], two[2])
    # a bias under which every sigmoid is 1.0f: one big tie, the mid-rank of the pool
    z3 = _mc_case(3, m, num_rels, h, k)[0]
    ranks, (ids, val), tgt = ops.pair_relation_scores_mc(z3, w, s, o, target=target, k=k, bias=torch.full((3,), 100.0).cuda(), cand=cand)
    assert bool((tgt == 1.0).all()) and bool((val[ids >= 0] == 1.0).all())
    assert bool((ranks[0] == (num_rels - 1) / 2).all())
    others = (mask & (torch.arange(num_rels, device='cuda').view(1, -1) != target.view(-1, 1))).sum(1)
    assert torch.equal(ranks[2], others.float() / 2)
    # a NaN in one sample's row: that pair's target ranks last, NaN is never optimistic
    bad = z3.clone()
    row = m // 2
    bad[1, s[row]] = float('nan')
    ranks = ops.pair_relation_scores_mc(bad, w, s, o, target=target, bias=bias.repeat(3))[0]
    hit = (s == s[row]) | (o == s[row])
    assert bool((ranks[0][hit] == num_rels - 1).all()) and bool((ranks[0][~hit] <= num_rels - 1).all())


@functools.lru_cache(maxsize=None)
def _f64_case(n_samples, m, num_rels, h):
    """The issue's recipe, its float64 reference and the per-element bound of tests/test_gpu_mc_rank.py with Q_s = fp32(z_s[s] *
    z_s[o]) against w; computed once per shape and left unchanged."""
    rng = np.random.default_rng(n_samples + m + num_rels + h)
    scale = 0.8 * h ** -0.25
    base = scale * rng.standard_normal((rc.N, h))
    z = (base[None] + 0.5 * scale * rng.standard_normal((n_samples, rc.N, h))).astype(np.float32)
    w = rng.standard_normal((num_rels, h)).astype(np.float32)
    bias = (0.5 * rng.standard_normal(n_samples)).astype(np.float32)
    s, o, t = rng.integers(0, rc.N, m), rng.integers(0, rc.N, m), rng.integers(0, num_rels, m)
    q64 = (z[:, s] * z[:, o]).astype(np.float64)                       # one fp32 multiply per element, as the kernel forms it
    w64 = w.astype(np.float64)
    logit = q64 @ w64.T + bias.astype(np.float64)[:, None, None]
    with np.errstate(over='ignore'):
        pbar = (1.0 / (1.0 + np.exp(-logit))).sum(axis=0) / n_samples
    mag = np.abs(q64) @ np.abs(w64).T + np.abs(bias.astype(np.float64))[:, None, None]
    eps = ((h + 2) * U * mag / 4).mean(axis=0) + C_SIG * U + n_samples * U
    gen = torch.Generator().manual_seed(m + num_rels)
    lo, hi, rel = rc.relation_lists(m, num_rels, torch.from_numpy(t), gen)
    listed = np.zeros((m, num_rels), dtype=bool)
    for i in range(m):
        listed[i, rel[int(lo[i]):int(hi[i])].cpu().numpy()] = True
    dev = [torch.from_numpy(x).cuda() for x in (z, w, bias, s, o, t)]
    return dev, (lo, hi, rel), listed, pbar, eps, t


@pytest.mark.parametrize('shape', MC_F64_SHAPES)
def test_mc_ranks_lie_inside_the_float64_interval(ops, shape):
    (z, w, bias, s, o, target), filt, listed, pbar, eps, t = _f64_case(*shape)
    m, num_rels = pbar.shape
    ranks = ops.pair_relation_scores_mc(z, w, s, o, target=target, bias=bias, filt_lo=filt[0], filt_hi=filt[1], filt_rel=filt[2])[0]
    rows = np.arange(m)
    for name, got, mask in (('raw', ranks[0], None), ('filtered', ranks[1], listed)):
        counts = np.ones((m, num_rels), dtype=bool)
        counts[rows, t] = False
        if mask is not None:
            counts &= ~mask
        pt, et = pbar[rows, t][:, None], eps[rows, t][:, None]
        lower = ((pbar > pt + eps + et) & counts).sum(axis=1)
        upper = ((pbar >= pt - eps - et) & counts).sum(axis=1)
        got = got.cpu().numpy().astype(np.float64)
        slack = float((upper - lower).sum()) / max(m * (num_rels - 1), 1)
        print(f'{shape} {name}: slack share {slack:.3e}, outside {int(((got < lower) | (got > upper)).sum())} of {m}')
        assert slack <= SLACK_CAP
        assert bool(((got >= lower) & (got <= upper)).all())


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------
def _driver_case(ranking, num_rels=65, m=130, h=16, n_samples=3):
    gen = torch.Generator().manual_seed(17)
    z = (torch.randn(rc.N, h, generator=gen) * 0.5 + 0.3 * torch.randn(n_samples, rc.N, h, generator=gen)).cuda()
    w = torch.randn(num_rels, h, generator=gen).cuda()
    s, o = rc.pairs(m, gen)
    r = torch.randint(0, num_rels, (m,), generator=gen).cuda()
    trip = torch.stack([s, r, o], 1)
    known = torch.cat([trip, torch.stack([s, (r + 1) % num_rels, o], 1), torch.stack([s, (r + 64) % num_rels, o], 1)])
    seen = torch.stack([torch.randint(0, rc.N, (3000,), generator=gen), torch.randint(0, num_rels, (3000,), generator=gen),
                        torch.randint(0, rc.N, (3000,), generator=gen)], 1)
    pf = ranking.PairFilterIndex(rc.N, num_rels, known.cpu(), device='cuda')
    tc = ranking.TypeConstraint(rc.N, num_rels, seen, trip[::2].cpu(), device='cuda')
    return z, w, s, o, trip, pf, tc


def _same_ranks(a, b):
    return len(a) == len(b) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def test_chunked_equals_unchunked_and_the_twins(ranking, transe, monkeypatch):
    z, w, s, o, trip, pf, tc = _driver_case(ranking)
    emb, k = z[0], 10
    bias, flps = torch.tensor([0.25]).cuda(), torch.tensor([0.25, -0.5, 0.0]).cuda()
    tables = (emb, w, 1, False)

    def run():
        return (ranking.rank_relations(emb, w, trip, pf, bias, type_constraint=tc), ranking.rank_relations_mc(z, w, trip, pf, flps, tc),
                ranking.rank_relations_mc(z, w, trip, pf, flps), ranking.rank_relations(emb, w, trip, None, bias, tc),
                transe.rank_relations(tables, trip, pf, tc),
                ranking.predict_relations(emb, w, s, o, k, pf, bias, tc), ranking.predict_relations_mc(z, w, s, o, k, pf, flps, tc),
                ranking.predict_relations_mc(z, w, s, o, k, pf, flps), transe.predict_relations(tables, s, o, k, pf, tc))
    whole = run()
    twins = (ranking.rank_relations_unfused(emb, w, trip, pf, bias, tc), None, None, ranking.rank_relations_unfused(emb, w, trip, None, bias, tc),
             transe.rank_relations_unfused(tables, trip, pf, tc), ranking.predict_relations_unfused(emb, w, s, o, k, pf, bias, tc), None, None,
             transe.predict_relations_unfused(tables, s, o, k, pf, tc))
    monkeypatch.setattr(ranking, 'MAX_QUERY_ROWS', 64)
    monkeypatch.setattr(transe, 'MAX_QUERY_ROWS', 64)
    parts = run()
    assert [len(x) for x in whole[:5]] == [4, 4, 2, 4, 4] and whole[3][1] is None and whole[3][3] is None
    for got in (parts, twins):
        for i in range(5):
            assert got[i] is None or _same_ranks(got[i], whole[i])
        for i in range(5, 9):
            assert got[i] is None or (rc.same_lists(got[i][:2], whole[i][:2]) and (len(got[i]) == 2 or rc.same_values(got[i][2], whole[i][2])))
    # the constrained kinds never count more than the unconstrained ones; the first two are the unconstrained call's
    assert _same_ranks(whole[0][:2], ranking.rank_relations(emb, w, trip, pf, bias))
    assert bool((whole[0][2] <= whole[0][0]).all()) and bool((whole[0][3] <= whole[0][1]).all())
    # proposals: type-correct, new, with the spread of ops.pair_prob_std_mc
    ids, mean, std = whole[6]
    ok = tc.pair_mask(s, o, 'cuda')
    assert bool(((ids < 0) | ok.gather(1, ids.clamp(min=0))).all())
    assert not bool(((ids == trip[:, 1:2]) & (ids >= 0)).any())
    assert bool((std >= 0).all()) and bool((std[ids < 0] == 0).all()) and bool((mean[ids >= 0] <= 1).all())
    # the MC twins agree to rounding: they sum the same sigmoids of GEMM logits with torch's sigmoid, not the device's.  The logits
    # are the same bits and pbar <= 1, so the two differ by the sigmoids' own errors (a few u each, C_SIG u = 2.4e-7 bounds the
    # device's) and the S-term sums' (S u): 1e-5 is some 40 times that, a guard against a wrong sample or bias, not an error bound
    um, us = ranking.predict_relations_mc_unfused(z, w, s, o, 65, pf, flps, tc)[1:]
    fm, fs = ranking.predict_relations_mc(z, w, s, o, 65, pf, flps, tc)[1:]
    fin = torch.isfinite(fm)
    assert torch.equal(fin, torch.isfinite(um))
    assert float((fm[fin].sort().values - um[fin].sort().values).abs().max()) < 1e-5
    report = ranking.calc_relation_mrr(emb, w, trip, pf, flow_log_prob=bias, verbose=False, type_constraint=tc)
    assert report == ranking.calc_relation_mrr_unfused(emb, w, trip, pf, flow_log_prob=bias, verbose=False, type_constraint=tc)
    assert set(report) == {f'{a}_{b}' for a in ('mrr', 'hits') for b in ranking.CONSTRAINED_KINDS}
    mc = ranking.calc_relation_mc_mrr(z, w, trip, None, flps, verbose=False, type_constraint=tc)
    assert set(mc) == {'n_samples', 'mrr_raw', 'hits_raw', 'mrr_raw_constrained', 'hits_raw_constrained'} and mc['n_samples'] == 3
    out = transe.evaluate_relations(tables, trip, pf, verbose=False, type_constraint=tc)
    assert {'mrr_raw_constrained', 'mr_filtered_constrained', 'hits_filtered_constrained'} <= set(out)
    with pytest.raises(ValueError, match='type_constraint was built for'):
        ranking.rank_relations(emb, w[:-1], trip % 64, None, None, tc)


# ---- both CLIs end to end ----------------------------------------------------------------------------------------------------------
def _typed_rows(path, kg, k, width):
    """check_relation_tsv's block rules with the relations left over counted over the type-correct ones."""
    rows = [line.rstrip('\n').split('\t') for line in open(path)]
    every = np.concatenate([kg.train, kg.valid, kg.test])
    known = {(s, o, r) for s, r, o in every.tolist()}
    subj, obj = {(s, r) for s, r, _ in every.tolist()}, {(o, r) for _, r, o in every.tolist()}
    assert len(rows) == k * len(kg.test) and all(len(x) == width for x in rows)
    assert [x[:3] for x in rows] == [[str(s), str(o), str(p)] for s, _, o in kg.test.tolist() for p in range(k)]
    for at in range(0, len(rows), k):
        block = [int(x[3]) for x in rows[at:at + k]]
        real = [r for r in block if r >= 0]
        s, o = int(rows[at][0]), int(rows[at][1])
        assert block == real + [-1] * (k - len(real)) and len(set(real)) == len(real)
        assert all((s, r) in subj and (o, r) in obj and (s, o, r) not in known for r in real)
        assert len(real) == min(k, sum(1 for r in range(kg.num_rels) if (s, r) in subj and (o, r) in obj and (s, o, r) not in known))
    return rows


def test_train_cli_typed_and_mc_relations(tmp_path, capsys):
    from gcn_vae_amd import data, train
    from gcn_vae_amd.encoders import KGVAE
    kg = data.load_data(rc.CLI_SPEC)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt = str(tmp_path / 'm.pth')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    files = {}
    for name, seed in (('a', '5'), ('b', '5'), ('c', '6')):
        out, mc_out = str(tmp_path / f'rel_{name}.tsv'), str(tmp_path / f'mc_{name}.tsv')
        train.main(train.build_parser().parse_args([
            '-d', rc.CLI_SPEC, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1', '--mog-k', '4', '--n-flows', '2',
            '--test-mode', 'True', '--model-state-file', ckpt, '--relation-eval', '--filtered-eval', '--predict-relations', str(rc.CLI_K),
            '--relations-out', out, '--relations-typed', '--mc-samples', '3', '--mc-seed', seed, '--mc-relations', '--mc-relations-out',
            mc_out]))
        files[name] = (out, mc_out, capsys.readouterr().out)
    text = files['a'][2]
    for kind in ('raw', 'filtered', 'raw_constrained', 'filtered_constrained'):
        assert f'Relation MRR ({kind}): ' in text and f'MC relation MRR ({kind}, 3 samples): ' in text
        assert all(f'Relation Hits ({kind}) @ {h}: ' in text and f'MC relation Hits ({kind}) @ {h}: ' in text for h in (1, 3, 10))
    rows = _typed_rows(files['a'][0], kg, rc.CLI_K, 5)
    assert all(np.isfinite(float(x[4])) or int(x[3]) < 0 for x in rows)
    mc_rows = _typed_rows(files['a'][1], kg, rc.CLI_K, 6)
    assert [x[:3] for x in mc_rows] == [x[:3] for x in rows]
    for at in range(0, len(mc_rows), rc.CLI_K):
        means = [float(x[4]) for x in mc_rows[at:at + rc.CLI_K] if int(x[3]) >= 0]
        assert all(0.0 <= p <= 1.0 for p in means) and means == sorted(means, reverse=True)
    assert all(float(x[5]) >= 0 for x in mc_rows)
    assert open(files['a'][1]).read() == open(files['b'][1]).read() != open(files['c'][1]).read()


def test_transe_cli_typed_relations(tmp_path, capsys):
    from gcn_vae_amd import data, transe
    kg = data.load_data(rc.CLI_SPEC)
    ckpt, out = str(tmp_path / 't.ckpt'), str(tmp_path / 'rel.tsv')
    torch.manual_seed(0)
    transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True).save_checkpoint(ckpt)
    args = transe.build_parser().parse_args(['-d', rc.CLI_SPEC, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                             '--filtered-eval', '--relation-eval', '--predict-relations', str(rc.CLI_K), '--relations-out',
                                             out, '--relations-typed'])
    report = transe.main(args)['relations']
    text = capsys.readouterr().out
    for kind in ('raw', 'filtered', 'raw_constrained', 'filtered_constrained'):
        assert f'Relation MRR ({kind}): ' in text and 'mrr_' + kind in report
    assert report['mrr_raw_constrained'] >= report['mrr_raw'] and report['mrr_filtered_constrained'] >= report['mrr_filtered']
    rows = _typed_rows(out, kg, rc.CLI_K, 5)
    assert all(np.isfinite(float(x[4])) or int(x[3]) < 0 for x in rows)


def test_cand_argument_errors(ops):
    emb, w, s, o, target, cand, mask, filt = _case(63, 65, 16, 10)
    z = emb.unsqueeze(0).repeat(2, 1, 1)
    calls = (lambda c: ops.pair_relation_scores(emb, w, s, o, target=target, cand=c),
             lambda c: ops.pair_relation_scores_mc(z, w, s, o, target=target, cand=c),
             lambda c: ops.transe_pair_relations(emb, w, s, o, 1, target=target, cand=c))
    for call in calls:
        with pytest.raises(RuntimeError, match='cand: the gfx950 path needs a CUDA/ROCm tensor'):
            call(cand.cpu())
        with pytest.raises(TypeError, match='cand: expected a 2-D int32 / uint32 bitmask'):
            call(cand.long())
        with pytest.raises(TypeError, match='cand: expected a 2-D int32 / uint32 bitmask'):
            call(cand[0])
        with pytest.raises(ValueError, match=r'cand: need at least one set and ceil\(65 / 32\) = 3 words per set'):
            call(cand[:, :2])
        with pytest.raises(ValueError, match='cand: need 2 n = 600 rows'):
            call(cand[:-1])
        wide = torch.zeros(2 * rc.N, 5, dtype=torch.int32, device='cuda')      # a view with a longer row stride is taken as it is
        wide[:, :3] = cand
        got, want = call(wide[:, :3])[0], call(cand)[0]
        assert got[1] is None and got[3] is None and torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    with pytest.raises(ValueError, match='bias: one value per sample'):
        ops.pair_relation_scores_mc(z, w, s, o, target=target, bias=torch.zeros(3).cuda())
    with pytest.raises(RuntimeError, match='w: the gfx950 path needs a CUDA/ROCm tensor; there is no CPU fallback'):
        ops.pair_relation_scores_mc(z, w.cpu(), s, o, target=target)
