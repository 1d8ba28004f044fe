"""Per-entity completion for the TransE baseline on the GPU (gv_transe_entity_topk / ops.transe_entity_topk /
transe.complete_entities): the fused route against the materialised one (per relation ops.transe_queries + ops.transe_distances,
ordered by transe.complete_entities_from_distances) and against the merge over relations of transe.predict_topk -- ids equal,
distance bits equal; ops.transe_distances itself is held to the golden vectors by tests/test_gpu_transe.py, so there is no tolerance
here.  pytest -m gpu."""
import functools

import numpy as np
import pytest
import torch

from entity_typed_cases import entities as _entities, same as _same

pytestmark = pytest.mark.gpu

# (N, R, dim): N % 64 != 0; dim below, across and no multiple of the 32-column stage; a single relation
SHAPES = [(150, 3, 20), (70, 7, 37), (200, 1, 200), (130, 5, 70)]


@functools.lru_cache(maxsize=None)
def _tables(n, num_rels, dim):
    gen = torch.Generator().manual_seed(n * 31 + num_rels * 7 + dim)
    ent = (torch.randn(n, dim, generator=gen) * 0.5).cuda()
    rel = (torch.randn(num_rels, dim, generator=gen) * 0.5).cuda()
    trip = torch.stack([torch.randint(0, n, (n * num_rels // 2,), generator=gen),
                        torch.randint(0, num_rels, (n * num_rels // 2,), generator=gen),
                        torch.randint(0, n, (n * num_rels // 2,), generator=gen)], 1)
    perm = torch.randperm(n, generator=gen)
    return ent, rel, trip, perm


@pytest.mark.parametrize('filtered', [False, True])
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('norm_flag', [True, False])
@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('n,num_rels,dim', SHAPES)
def test_fused_equals_unfused_exactly(n, num_rels, dim, p_norm, norm_flag, side, filtered):
    from gcn_vae_amd import ranking, transe
    ent, rel, trip, perm = _tables(n, num_rels, dim)
    tables = (ent, rel, p_norm, norm_flag)
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda') if filtered else None
    for m in (1, 64, 65, n):
        ents = _entities(perm, m)
        for k in (1, 10, 128):
            got = transe.complete_entities(tables, ents, k, side=side, filter_index=fi)
            want = transe.complete_entities_unfused(tables, ents, k, side=side, filter_index=fi)
            assert got[0].shape == (m, k) and got[0].dtype == torch.int64 and got[1].dtype == torch.int64
            assert got[2].dtype == torch.float32
            assert _same(got, want), (m, k)
    # the list is new facts only: no known triplet, no loop
    if filtered:
        r_, other, _ = got
        a = ents.view(-1, 1).expand_as(r_)
        s, o = (a, other) if side == 's' else (other, a)
        known = {tuple(t) for t in trip.tolist()}
        listed = {t for t in zip(s.flatten().tolist(), r_.flatten().tolist(), o.flatten().tolist()) if t[1] >= 0}
        assert listed and not (listed & known) and all(x != y for x, _, y in listed)


@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('n,num_rels,dim', SHAPES)
def test_fused_equals_the_merge_of_predict_topk(n, num_rels, dim, p_norm, side):
    """The bit-for-bit claim against the existing entry point: per relation transe.predict_topk gives each query's k nearest, and
    their merge by (distance, r, x) is the entity's list (exclude_self off: predict_topk keeps the loops)."""
    from gcn_vae_amd import ranking, transe
    ent, rel, trip, perm = _tables(n, num_rels, dim)
    tables = (ent, rel, p_norm, True)
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    ents, k = _entities(perm, 65), 10
    pool = torch.zeros(65, num_rels, n, device='cuda')
    given = torch.zeros(65, num_rels, n, dtype=torch.bool, device='cuda')
    for r in range(num_rels):
        ids, dist = transe.predict_topk(tables, ents, torch.full_like(ents, r), k, direction='o' if side == 's' else 's',
                                        filter_index=fi)
        live = ids >= 0
        rows = torch.arange(65, device='cuda').view(-1, 1).expand_as(ids)
        pool[rows[live], r, ids[live]] = dist[live]
        given[rows[live], r, ids[live]] = True
    want_ids, want_dist = transe.topk_from_distances(pool.view(65, -1), k, cand=given.view(65, -1))
    got = transe.complete_entities(tables, ents, k, side=side, filter_index=fi, exclude_self=False)
    assert torch.equal(got[0] * n + got[1], want_ids) and torch.equal(got[2].view(torch.int32), want_dist.view(torch.int32))


@functools.lru_cache(maxsize=None)
def _integer_case():
    """Small-integer tables, raw (norm_flag off), L1: every distance is an exact small integer, relations 0 and 2 are the same row
    (equal distances across relations), entities 3 and 90 the same row (equal distances inside a relation, 64-entity tiles apart).
    The distances come from float64 on the CPU: dist[head][a, r, x]."""
    gen = torch.Generator().manual_seed(5)
    n, num_rels, dim = 150, 4, 6
    ent = torch.randint(-2, 3, (n, dim), generator=gen).float()
    ent[90] = ent[3]
    rel = torch.randint(-2, 3, (num_rels, dim), generator=gen).float()
    rel[2] = rel[0]
    e, r = ent.double(), rel.double()
    dist = [((e[:, None, None, :] + sign * r[None, :, None, :]) - e[None, None, :, :]).abs().sum(-1).float() for sign in (1.0, -1.0)]
    return ent.cuda(), rel.cuda(), dist


@pytest.mark.parametrize('span', [None, 1, 2, 5, 12])
def test_integer_tables_tie_across_relations_and_span_boundaries(span):
    """N = 150 is three entity tiles, so the 12 (relation, tile) pairs are cut into 12, 6, 3 and 1 spans by the override (span = 5
    cuts inside relations 1 and 3); the library's own rule gives one span here.  The order must be the rule's in every cut."""
    from gcn_vae_amd import ops, transe
    ent, rel, dist = _integer_case()
    ents = torch.tensor([7, 3, 149, 90, 3, 64, 0], device='cuda')
    for head in (False, True):
        for k in (1, 10, 128):
            for excl in (True, False):
                want = transe.complete_entities_from_distances(dist[head][ents.cpu()], ents.cpu(), k, exclude_self=excl)
                got = ops.transe_entity_topk(ents, ent, rel, k, 1, head, exclude_self=excl, span=span)
                assert _same(tuple(t.cpu() for t in got), want), (head, k, excl)
        # ties are there, every relation shows up, every distance is a whole number
        assert (want[2][:, :-1] == want[2][:, 1:]).any() and len(want[0].unique()) == 4
        assert torch.equal(want[2], want[2].round()) and float(want[2].max()) <= 4 * 6 + 2 * 6


@pytest.mark.parametrize('n,num_rels,dim', [(150, 3, 20), (130, 5, 70), (70, 7, 37)])
def test_result_does_not_depend_on_the_span_geometry(n, num_rels, dim):
    from gcn_vae_amd import ops, ranking
    ent, rel, trip, perm = _tables(n, num_rels, dim)
    lo, hi, f_ent = ranking._mine_filter(ranking.FilterIndex(n, num_rels, trip, device='cuda'), n, num_rels, ent.device)
    en, rn = ops.transe_queries(ent, norm_flag=True), ops.transe_queries(rel, norm_flag=True)
    ents = _entities(perm, 65)
    base = ops.transe_entity_topk(ents, en, rn, 128, 1, False, lo, hi, f_ent)
    assert (base[0] >= 0).any()
    for span in (1, 2, 4, 7, 10 ** 6):
        assert _same(ops.transe_entity_topk(ents, en, rn, 128, 1, False, lo, hi, f_ent, span=span), base), span


def test_padding_past_the_last_candidate():
    from gcn_vae_amd import transe
    gen = torch.Generator().manual_seed(3)
    tables = (torch.randn(5, 9, generator=gen).cuda(), torch.randn(1, 9, generator=gen).cuda(), 2, True)
    ents = torch.arange(5, device='cuda')
    rel, other, dist = transe.complete_entities(tables, ents, 10)                    # 4 candidates each: the loops are out
    assert (rel[:, :4] == 0).all() and (rel[:, 4:] == -1).all() and (other[:, 4:] == -1).all()
    assert torch.isinf(dist[:, 4:]).all() and (dist[:, 4:] > 0).all()
    assert all(sorted(other[i, :4].tolist()) == [x for x in range(5) if x != i] for i in range(5))
    assert _same((rel, other, dist), transe.complete_entities_unfused(tables, ents, 10))
    rel, _, _ = transe.complete_entities(tables, ents, 10, exclude_self=False)
    assert (rel[:, :5] == 0).all() and (rel[:, 5:] == -1).all()
    for route in (transe.complete_entities, transe.complete_entities_unfused):
        empty = route(tables, ents[:0], 10)
        assert empty[0].shape == (0, 10) and empty[1].shape == (0, 10) and empty[2].shape == (0, 10)


def test_a_relation_whose_filter_lists_every_entity_contributes_nothing():
    from gcn_vae_amd import ranking, transe
    n, num_rels, dim = 150, 3, 20
    ent, rel, _, perm = _tables(n, num_rels, dim)
    tables = (ent, rel, 1, True)
    everybody = torch.cartesian_prod(torch.arange(n), torch.tensor([1]), torch.arange(n))      # every (s, 1, o)
    fi = ranking.FilterIndex(n, num_rels, everybody, device='cuda')
    ents = _entities(perm, 70)
    for side in ('s', 'o'):
        got = transe.complete_entities(tables, ents, 128, side=side, filter_index=fi)
        assert not (got[0] == 1).any() and (got[0] >= 0).all()
        assert _same(got, transe.complete_entities_unfused(tables, ents, 128, side=side, filter_index=fi))


def test_cli_writes_the_entity_profiles(tmp_path, monkeypatch):
    from gcn_vae_amd import data, transe
    spec = 'synthetic:60:4:400:40:40'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    ckpt, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'profiles.tsv')
    model.save_checkpoint(ckpt)
    seen = []
    real = transe.complete_entities

    def spy(*args, **kwargs):
        res = real(*args, **kwargs)
        seen.append((kwargs['side'], args[1].tolist(), res))
        return res
    monkeypatch.setattr(transe, 'complete_entities', spy)
    who, k = [3, 59, 3, 0], 5
    args = transe.build_parser().parse_args(['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                             '--profile-topk', str(k), '--profile-entities', ','.join(map(str, who)),
                                             '--profile-out', out])
    transe.main(args)
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert [s for s, _, _ in seen] == ['s', 'o'] and all(e == who for _, e, _ in seen)
    padding = sum(int((res[0] < 0).sum()) for _, _, res in seen)
    assert len(rows) == 2 * len(who) * k - padding and all(len(row) == 6 for row in rows)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    at = 0
    for side, ents, res in seen:
        rel, other, dist = (t.cpu() for t in res)
        for i, a in enumerate(ents):
            for j in range(k):
                if rel[i, j] < 0:
                    continue
                e_, sd, r, x, rank, d = rows[at]
                at += 1
                assert (int(e_), sd, int(r), int(x), int(rank)) == (a, side, int(rel[i, j]), int(other[i, j]), j + 1)
                assert np.float32(d) == dist[i, j].numpy()                            # nine digits give the float32 back
                fact = (a, int(r), int(x)) if side == 's' else (int(x), int(r), a)
                assert fact not in known and int(x) != a
    assert at == len(rows) and at > 0
    # an id equal to N is refused before anything is written
    bad = transe.build_parser().parse_args(['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                            '--profile-topk', str(k), '--profile-entities', f'3,{kg.num_nodes}',
                                            '--profile-out', str(tmp_path / 'never.tsv')])
    with pytest.raises(ValueError, match='outside'):
        transe.main(bad)
    assert not (tmp_path / 'never.tsv').exists()
