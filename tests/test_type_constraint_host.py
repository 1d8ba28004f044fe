"""Type-constrained ranking and top-k without a GPU: ranking.TypeConstraint against Python sets, the plain-torch rules
(rank_from_scores_constrained, topk_from_scores(cand=...)) against brute force, and the --type-constrain flag of both CLIs."""
import numpy as np
import pytest
import torch

from gcn_vae_amd import ranking, train, transe


def _graph(n, num_rels, count, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n, (count,), generator=gen), torch.randint(0, num_rels, (count,), generator=gen),
                        torch.randint(0, n, (count,), generator=gen)], 1)


def _python_sets(num_rels, *triplet_sets):
    sets = [set() for _ in range(2 * num_rels)]
    for t in triplet_sets:
        for s, r, o in np.asarray(t).reshape(-1, 3).tolist():
            sets[r].add(o)
            sets[num_rels + r].add(s)
    return sets


def _bits(words_row):
    """The set a row of int32 words spells out, every bit of every word read (padding bits included)."""
    out = set()
    for w, x in enumerate(words_row.tolist()):
        x &= 0xffffffff
        out |= {32 * w + b for b in range(32) if x >> b & 1}
    return out


@pytest.mark.parametrize('n', [203, 33, 64])
def test_type_constraint_against_python_sets(n):
    num_rels = 3
    a, b = _graph(n, num_rels, 150, seed=n), _graph(n, num_rels, 40, seed=n + 1)
    a[0] = torch.tensor([n - 1, 0, n - 1])                       # the last entity: the top used bit of the last word
    b = torch.cat([b, b[:7], a[:5]])                             # duplicated triplets, within and across the sets
    tc = ranking.TypeConstraint(n, num_rels, a, b.numpy())
    want = _python_sets(num_rels, a, b)
    assert tc.words.dtype == torch.int32 and tuple(tc.words.shape) == (2 * num_rels, (n + 31) // 32)
    for i in range(2 * num_rels):
        assert _bits(tc.words[i]) == want[i]                     # nothing at positions >= n either
    assert tc.sizes.tolist() == [len(x) for x in want]
    r = torch.arange(num_rels)
    assert tc.set_ids(r, 'o').dtype == torch.int32
    assert tc.set_ids(r, 'o').tolist() == [0, 1, 2] and tc.set_ids(r, 's').tolist() == [3, 4, 5]
    ent = torch.arange(n)
    for rel in range(num_rels):
        for d, sid in (('o', rel), ('s', num_rels + rel)):
            got = tc.contains(torch.full((n,), rel), ent, d)
            assert got.dtype == torch.bool and got.tolist() == [j in want[sid] for j in range(n)]
    dense = tc.mask(torch.tensor([0, 5, -1, 6]))
    assert tuple(dense.shape) == (4, n) and dense[0].tolist() == [j in want[0] for j in range(n)]
    assert dense[1].tolist() == [j in want[5] for j in range(n)] and not dense[2:].any()      # out of range: the empty set
    with pytest.raises(ValueError):
        tc.set_ids(r, 'x')


def test_type_constraint_empty_and_out_of_range():
    tc = ranking.TypeConstraint(203, 3, np.zeros((0, 3), dtype=np.int64))
    assert tuple(tc.words.shape) == (6, 7) and not tc.words.any() and tc.sizes.tolist() == [0] * 6
    tc = ranking.TypeConstraint(203, 3)
    assert tuple(tc.words.shape) == (6, 7) and not tc.words.any()
    for bad in ([[203, 0, 1]], [[1, 0, 203]], [[1, 3, 1]], [[-1, 0, 1]], [[1, -1, 1]]):
        with pytest.raises(ValueError):
            ranking.TypeConstraint(203, 3, torch.tensor(bad))
    with pytest.raises(ValueError):
        ranking.TypeConstraint(203, 3, torch.tensor([[0, 0, 1]])).contains(torch.tensor([0]), torch.tensor([203]), 'o')


def _brute(score, target, cand, listed):
    m, v = score.shape
    out = np.zeros((4, m))
    for i in range(m):
        t = score[i, target[i]]
        for j in range(v):
            if j == target[i]:
                continue
            x = score[i, j]
            c = 1.0 if not (x <= t) else (0.5 if x == t else 0.0)
            for slot, ok in enumerate((True, not listed[i, j], cand[i, j], cand[i, j] and not listed[i, j])):
                if ok:
                    out[slot, i] += c
    return out


def test_rank_rule_against_a_double_loop():
    gen = torch.Generator().manual_seed(3)
    m, v = 9, 41
    score = torch.randn(m, v, generator=gen)
    target = torch.randint(0, v, (m,), generator=gen)
    cand = torch.rand(m, v, generator=gen) < 0.4
    listed = torch.rand(m, v, generator=gen) < 0.2
    nan = float('nan')
    # row 0: ties with the target inside and outside the set, listed and not
    target[0] = 4
    score[0, [1, 2, 3, 5]] = score[0, 4].item()
    cand[0, [1, 2]], cand[0, [3, 5]] = True, False
    listed[0, [1, 3]], listed[0, [2, 5]] = True, False
    # row 1: NaN candidates inside and outside the set
    target[1] = 0
    score[1, [7, 8, 9]] = nan
    cand[1, [7, 9]], cand[1, 8] = True, False
    listed[1, 9], listed[1, [7, 8]] = True, False
    # row 2: a NaN target; row 3: a target outside its set; row 4: a target inside it; row 5: the empty set; row 6: the full set
    score[2, target[2]] = nan
    cand[3, target[3]], cand[4, target[4]] = False, True
    cand[5], cand[6] = False, True
    got = ranking.rank_from_scores_constrained(score, target, cand, listed)
    want = _brute(score.numpy(), target.tolist(), cand.numpy(), listed.numpy())
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and g.tolist() == w.tolist()
    assert got[2][5] == 0 and got[3][5] == 0                         # an empty set: rank 1
    assert got[2][2] == int(cand[2].sum()) - int(cand[2, target[2]])         # a NaN target: behind every other member
    # without a listed mask: the filtered pair is None, the others unchanged
    raw, f, raw_c, f_c = ranking.rank_from_scores_constrained(score, target, cand)
    assert f is None and f_c is None and torch.equal(raw, got[0]) and torch.equal(raw_c, got[2])


def test_all_true_mask_reproduces_the_unconstrained_rules():
    gen = torch.Generator().manual_seed(4)
    n, num_rels = 60, 4
    trip = _graph(n, num_rels, 300, seed=8)
    fi = ranking.FilterIndex(n, num_rels, trip)
    ent, rel = torch.randn(n, 12, generator=gen), torch.randn(num_rels, 12, generator=gen)
    test = trip[:25]
    ent[7] = ent[3]                                                  # exact ties
    raw_u, filt_u = transe.rank_transe_unfused(ent, rel, test, 1, True, fi, batch=25)
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    full = torch.ones(25, n, dtype=torch.bool)
    pos = 0
    for head, a, b, d in ((True, o, s, 's'), (False, s, o, 'o')):
        cand = ent.unsqueeze(0).expand(25, n, 12)
        fix, rr = ent[a].unsqueeze(1).expand_as(cand), rel[r].unsqueeze(1).expand_as(cand)
        cand, fix, rr = (torch.nn.functional.normalize(x, 2, -1) for x in (cand, fix, rr))
        dist = torch.norm(cand + (rr - fix) if head else (fix + rr) - cand, 1, -1)
        lo, hi = fi.lookup(a, r, d)
        listed = ranking._listed_mask(lo, hi, fi.entities(d), 25, n, 'cpu')
        got = ranking.rank_from_scores_constrained(-dist, b, full, listed)
        assert torch.equal(got[0], ranking.sort_and_rank(-dist, b)) and torch.equal(got[2], got[0])
        assert torch.equal(got[0], raw_u[pos:pos + 25])
        assert torch.equal(got[1], filt_u[pos:pos + 25]) and torch.equal(got[3], got[1])
        pos += 25


def test_topk_rule_with_a_candidate_mask():
    gen = torch.Generator().manual_seed(5)
    m, v, k = 6, 50, 8
    score = torch.randn(m, v, generator=gen)
    score[0, 30] = 5.0                                               # row 0's best, tied by 10 (listed) and 11
    score[0, 10], score[0, 11], score[1, 3] = score[0, 30], score[0, 30], float('nan')
    lo = torch.tensor([0, 0, 2, 2, 2, 2])
    hi = torch.tensor([2, 0, 2, 4, 4, 4])
    ent = torch.tensor([10, 20, 5, 6])
    cand = torch.rand(m, v, generator=gen) < 0.5
    cand[0, [10, 11, 30]] = True
    cand[1, 3] = True
    cand[2] = False
    cand[2, [4, 9, 17]] = True                                       # a set smaller than k
    cand[3] = False                                                  # the empty set
    cand[4] = False
    cand[4, [5, 6, 7]] = True                                        # 5 and 6 are listed: one candidate left
    # cand=None is exactly the current output
    for f in ((None, None, None), (lo, hi, ent)):
        a, b = ranking.topk_from_scores(score, k, *f), ranking.topk_from_scores(score, k, *f, cand=None)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        full = ranking.topk_from_scores(score, k, *f, cand=torch.ones(m, v, dtype=torch.bool))
        assert torch.equal(a[0], full[0]) and torch.equal(a[1].view(torch.int32), full[1].view(torch.int32))
    ids, logits = ranking.topk_from_scores(score, k, lo, hi, ent, cand=cand)
    listed = ranking._listed_mask(lo, hi, ent, m, v, 'cpu')
    for i in range(m):
        pool = [j for j in range(v) if cand[i, j] and not listed[i, j]]
        pool.sort(key=lambda j: (bool(torch.isnan(score[i, j])), -float(torch.nan_to_num(score[i, j], nan=0.0)), j))
        want = pool[:k] + [-1] * max(0, k - len(pool))
        assert ids[i].tolist() == want
        for p, j in enumerate(want):
            x = logits[i, p].item()
            assert x == float('-inf') if j < 0 else (x != x if score[i, j] != score[i, j] else x == score[i, j].item())
    assert ids[2].tolist() == sorted([4, 9, 17], key=lambda j: -score[2, j].item()) + [-1] * 5
    assert ids[3].tolist() == [-1] * k and bool((logits[3] == float('-inf')).all())
    assert ids[4].tolist() == [7] + [-1] * 7
    assert ids[0, :2].tolist() == [11, 30]                           # a listed member is no candidate; ties by lower id
    # topk_from_distances: the same rule on -distance, padded with +inf
    dist = score.abs()
    ids_d, d = transe.topk_from_distances(dist, k, lo, hi, ent, cand)
    ids_s, neg = ranking.topk_from_scores(-dist, k, lo, hi, ent, cand=cand)
    assert torch.equal(ids_d, ids_s) and bool((d[3] == float('inf')).all())
    a, b = transe.topk_from_distances(dist, k, lo, hi, ent), transe.topk_from_distances(dist, k, lo, hi, ent, None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_lib_signatures_of_the_four_entry_points():
    from gcn_vae_amd import lib
    want = {'gv_rank_scores_constrained': 23, 'gv_topk_scores_constrained': 21, 'gv_transe_rank_constrained': 19,
            'gv_transe_topk_constrained': 19}
    for name, n_args in want.items():
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args
        base = name.replace('_constrained', '_filtered' if 'rank' in name else '')
        assert len(lib.SIGNATURES[base][1]) + (6 if 'rank' in name else 4) == n_args      # + cand, ld_cand, n_sets, cand_set (+ 2 counts)


def test_type_constrain_flag_of_both_clis():
    p = train.build_parser()
    base = ['-d', 'synthetic:50:4:300:20:10:7']
    assert p.parse_args(base).type_constrain is False
    args = p.parse_args(base + ['--type-constrain', '--filtered-eval', '--test-mode', 'True'])
    assert args.type_constrain is True
    train.check_args(args)
    with pytest.raises(ValueError, match='--filtered-eval'):
        train.check_args(p.parse_args(base + ['--type-constrain', '--test-mode', 'True']))
    with pytest.raises(ValueError, match='--test-mode'):             # training never reads the sets: refused, not ignored
        train.check_args(p.parse_args(base + ['--type-constrain', '--filtered-eval']))
    p = transe.build_parser()
    assert p.parse_args(base).type_constrain is False
    args = p.parse_args(base + ['--type-constrain', '--filtered-eval'])
    assert args.type_constrain is True
    transe.check_args(args)
    with pytest.raises(ValueError, match='--filtered-eval'):
        transe.check_args(p.parse_args(base + ['--type-constrain']))
    transe.check_args(p.parse_args(base + ['--predict-topk', '5']))              # unchanged without the flag
