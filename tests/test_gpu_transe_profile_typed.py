"""Per-entity completion among type-correct facts for the TransE baseline on the GPU (gv_transe_entity_topk_typed /
ops.transe_entity_topk_typed / transe.complete_entities(type_constraint=)): the fused sweep over the relations' member lists
against the materialised route under the same constraint, against the untyped fused kernel under an all-full constraint, and
against the merge over relations of transe.predict_topk(type_constraint=) -- ids equal, distance bits equal, no tolerance
anywhere.  pytest -m gpu."""
import functools

import numpy as np
import pytest
import torch

from entity_typed_cases import (SETTINGS, SHAPES, check_facts, constraint_of, entities, full_constraint, same, setting, tables, trap)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('kind,filtered', SETTINGS)
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('p_norm,norm_flag', [(1, True), (2, True), (2, False)])
@pytest.mark.parametrize('n,num_rels,dim', SHAPES)
def test_fused_equals_unfused_exactly(n, num_rels, dim, p_norm, norm_flag, side, kind, filtered):
    from gcn_vae_amd import transe
    ent, rel, trip, _, perm = tables(n, num_rels, dim)
    model = (ent, rel, p_norm, norm_flag)
    tc, fi, cs, co = setting(n, num_rels, dim, kind, filtered)
    for m in (1, 64, 65, n):
        ents = entities(perm, m)
        for k in (1, 10, 128):
            got = transe.complete_entities(model, ents, k, side=side, filter_index=fi, type_constraint=tc)
            want = transe.complete_entities_unfused(model, ents, k, side=side, filter_index=fi, type_constraint=tc)
            assert got[0].shape == (m, k) and got[0].dtype == torch.int64 and got[1].dtype == torch.int64
            assert got[2].dtype == torch.float32
            assert same(got, want), (m, k)
    # every fact of the last (all entities, k = 128) answer is type-correct, no loop and, under a filter, new
    known = {tuple(t) for t in trip.tolist()} if filtered else None
    assert check_facts(ents, side, got[0], got[1], cs, co, known)


@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('n,num_rels,dim', SHAPES)
def test_an_all_full_constraint_gives_the_untyped_kernels_answer(n, num_rels, dim, p_norm, side):
    """Ties the new kernel to the existing one bit for bit: with every set full the gathered tiles are the untyped kernel's."""
    from gcn_vae_amd import ranking, transe
    ent, rel, trip, _, perm = tables(n, num_rels, dim)
    model = (ent, rel, p_norm, True)
    full = full_constraint(n, num_rels)
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    for m in (65, n):
        ents = entities(perm, m)
        for k in (10, 128):
            for kw in (dict(), dict(filter_index=fi), dict(filter_index=fi, exclude_self=False)):
                got = transe.complete_entities(model, ents, k, side=side, type_constraint=full, **kw)
                assert same(got, transe.complete_entities(model, ents, k, side=side, **kw)), (m, k, sorted(kw))


@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('n,num_rels,dim', SHAPES)
def test_fused_equals_the_merge_of_predict_topk(n, num_rels, dim, p_norm, side):
    """Per relation transe.predict_topk(type_constraint=) gives the k nearest type-correct answers of the queries (a, r) with a on
    the query side of r; their merge by (distance, r, x) is the entity's list (exclude_self off: predict_topk keeps the loops)."""
    from gcn_vae_amd import transe
    ent, rel, _, _, perm = tables(n, num_rels, dim)
    model = (ent, rel, p_norm, True)
    tc, fi, cs, co = setting(n, num_rels, dim, 'lengths', True)
    ents, k = entities(perm, 65), 10
    on_query_side = (cs if side == 's' else co).cuda()
    pool = torch.zeros(65, num_rels, n, device='cuda')
    given = torch.zeros(65, num_rels, n, dtype=torch.bool, device='cuda')
    for r in range(num_rels):
        rows = torch.nonzero(on_query_side[r, ents]).flatten()
        if not rows.numel():
            continue
        ids, dist = transe.predict_topk(model, ents[rows], torch.full_like(ents[rows], r), k, direction='o' if side == 's' else 's',
                                        filter_index=fi, type_constraint=tc)
        live = ids >= 0
        at = rows.view(-1, 1).expand_as(ids)
        pool[at[live], r, ids[live]] = dist[live]
        given[at[live], r, ids[live]] = True
    want_ids, want_dist = transe.topk_from_distances(pool.view(65, -1), k, cand=given.view(65, -1))
    got = transe.complete_entities(model, ents, k, side=side, filter_index=fi, exclude_self=False, type_constraint=tc)
    gone = got[0] < 0
    assert torch.equal(torch.where(gone, got[0], got[0] * n + got[1]), want_ids)
    assert torch.equal(got[2].view(torch.int32), want_dist.view(torch.int32))
    assert given.any()


@functools.lru_cache(maxsize=None)
def _integer_case():
    """The untyped test's small-integer tables (raw, L1: every distance an exact small integer; relations 0 and 2 the same row,
    entities 3 and 90 the same row) under a constraint that keeps both twins as candidates of both relations on either side.  The
    candidate lists of side 's' (objects) and of side 'o' (subjects) are the same sets: relation 0 all but three ids (147 members,
    three tiles: the twins sit in tiles 0 and 1), relation 1 65 random members, relation 2 the even ids and 3 (76 members: the
    twins share tile 0), relation 3 30 members: 8 tiles.  Every entity is on the query side of every relation."""
    gen = torch.Generator().manual_seed(5)
    n, num_rels, dim = 150, 4, 6
    ent = torch.randint(-2, 3, (n, dim), generator=gen).float()
    ent[90] = ent[3]
    rel = torch.randint(-2, 3, (num_rels, dim), generator=gen).float()
    rel[2] = rel[0]
    e, r = ent.double(), rel.double()
    dist = [((e[:, None, None, :] + sign * r[None, :, None, :]) - e[None, None, :, :]).abs().sum(-1).float() for sign in (1.0, -1.0)]
    cand = torch.zeros(num_rels, n, dtype=torch.bool)
    cand[0] = True
    cand[0, [10, 20, 30]] = False
    cand[1, torch.randperm(n, generator=gen)[:65]] = True
    cand[2, 0::2] = True
    cand[2, 3] = True
    cand[3, torch.randperm(n, generator=gen)[:30]] = True
    return ent.cuda(), rel.cuda(), dist, cand


@pytest.mark.parametrize('span', [None, 1, 2, 5, 10 ** 6])
def test_integer_tables_tie_across_relations_and_span_boundaries(span):
    """8 tiles: span = 1 cuts after every tile (inside every list of more than 64), 2 at the relations' ends only, 5 inside relation
    2's list, 10**6 and the library's own rule not at all.  The order must be the rule's in every cut."""
    from gcn_vae_amd import ops, transe
    ent, rel, dist, cand = _integer_case()
    everybody = torch.ones_like(cand)
    ents = torch.tensor([7, 3, 149, 90, 3, 64, 0], device='cuda')
    for head in (False, True):
        cs, co = (everybody, cand) if not head else (cand, everybody)
        set_ptr, set_ids = constraint_of(cs, co).members('cuda')
        assert ops.entity_typed_plan(set_ptr, 4, 'o' if head else 's')[0].tolist() == [0, 3, 5, 7, 8]
        for k in (1, 10, 128):
            for excl in (True, False):
                want = transe.complete_entities_from_distances(dist[head][ents.cpu()], ents.cpu(), k, exclude_self=excl,
                                                               cand_query=everybody, cand_other=cand)
                got = ops.transe_entity_topk_typed(ents, ent, rel, k, 1, set_ptr, set_ids, head, exclude_self=excl, span=span)
                assert same(tuple(t.cpu() for t in got), want), (head, k, excl)
        # ties are there, every relation shows up, every distance is a whole number
        assert (want[2][:, :-1] == want[2][:, 1:]).any() and len(want[0].unique()) == 4
        assert torch.equal(want[2], want[2].round())
        for row in range(ents.numel()):                                     # the twins: relation 0 before 2, entity 3 before 90
            pairs = list(zip(want[0][row].tolist(), want[1][row].tolist()))
            twins = [p for p in pairs if p in ((0, 3), (0, 90), (2, 3), (2, 90))]
            assert twins == sorted(twins)


@pytest.mark.parametrize('n,num_rels,dim', [(150, 3, 20), (130, 5, 260), (70, 7, 37)])
def test_result_does_not_depend_on_the_span_geometry(n, num_rels, dim):
    from gcn_vae_amd import ops, ranking
    ent, rel, _, _, perm = tables(n, num_rels, dim)
    tc, fi, _, _ = setting(n, num_rels, dim, 'lengths', True)
    lo, hi, f_ent = ranking._mine_filter(fi, n, num_rels, ent.device)
    set_ptr, set_ids = tc.members('cuda')
    en, rn = ops.transe_queries(ent, norm_flag=True), ops.transe_queries(rel, norm_flag=True)
    ents = entities(perm, 65)
    base = ops.transe_entity_topk_typed(ents, en, rn, 128, 1, set_ptr, set_ids, False, lo, hi, f_ent)
    assert (base[0] >= 0).any()
    for span in (1, 2, 4, 7, 10 ** 6):
        assert same(ops.transe_entity_topk_typed(ents, en, rn, 128, 1, set_ptr, set_ids, False, lo, hi, f_ent, span=span), base), span


@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('side', ['s', 'o'])
def test_listed_ids_between_two_members_hide_only_themselves(side, p_norm):
    """The filter trap: the cursor must pass 128 listed non-members between two members (more than one window of 64) and then still
    hide the two listed members behind them."""
    from gcn_vae_amd import ranking, transe
    n, num_rels, a, cq, co, listed, remain = trap()
    model = (tables(n, 1, 200)[0], tables(150, 3, 20)[1][:2].repeat(1, 10).contiguous(), p_norm, True)
    cs, cobj = (cq, co) if side == 's' else (co, cq)
    tc = constraint_of(cs, cobj)
    trip = [(q, r, x) if side == 's' else (x, r, q) for q, r, x in listed]
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    ents = torch.tensor([a, 7, 3], device='cuda')                          # 3 is on the query side of no relation
    for excl in (True, False):
        got = transe.complete_entities(model, ents, 128, side=side, filter_index=fi, exclude_self=excl, type_constraint=tc)
        assert same(got, transe.complete_entities_unfused(model, ents, 128, side=side, filter_index=fi, exclude_self=excl,
                                                          type_constraint=tc))
        rel, other = got[0].cpu(), got[1].cpu()
        assert sorted(other[0][rel[0] == 1].tolist()) == remain                # 193 and 197 are gone, every other member is there
        assert sorted(other[0][rel[0] == 0].tolist()) == list(range(50)) and int((rel[0] < 0).sum()) == 128 - 57
        assert sorted(other[1][rel[1] == 1].tolist()) == list(range(192, 200))      # entity 7 lists member 5 only
        assert (rel[2] == -1).all()


def test_padding_and_the_lists_that_end_at_a_tile_boundary():
    from gcn_vae_amd import ops, transe
    n, num_rels = 150, 4
    model = (tables(150, 3, 20)[0], tables(70, 7, 37)[1][:4, :20].contiguous(), 2, True)
    co = torch.zeros(num_rels, n, dtype=torch.bool)
    co[0, 10:74] = True                                                     # exactly 64 candidates
    co[1, torch.arange(0, 130, 2)] = True                                   # 65
    co[3, 149] = True                                                       # 1; relation 2 has none
    cs = torch.zeros(num_rels, n, dtype=torch.bool)
    cs[:, :100] = True                                                      # entities 100 .. 149 are on the query side of nothing
    cs[2, :] = True                                                         # ... but of the relation without candidates
    tc = constraint_of(cs, co)
    ents = torch.tensor([0, 120, 12, 149, 99], device='cuda')
    got = transe.complete_entities(model, ents, 128, type_constraint=tc)
    assert same(got, transe.complete_entities_unfused(model, ents, 128, type_constraint=tc))
    rel, other, dist = (t.cpu() for t in got)
    for row in (1, 3):
        assert (rel[row] == -1).all() and (other[row] == -1).all() and (dist[row] == float('inf')).all()
    # entity 12 is a candidate of relations 0 and 1 itself: 63 + 64 + 0 + 1 candidates without its loops, exactly k
    assert [int((rel[2] == r).sum()) for r in range(num_rels)] == [63, 64, 0, 1]
    for row in (0, 4):                                                      # 129 and 130 candidates: a full list, none of relation 2
        assert (rel[row] >= 0).all() and not (rel[row] == 2).any()
    # no tile at all: every candidate list empty
    none = constraint_of(cs, torch.zeros(num_rels, n, dtype=torch.bool))
    for k in (1, 100):
        rel, other, dist = transe.complete_entities(model, ents, k, type_constraint=none)
        assert rel.shape == other.shape == dist.shape == (5, k) and rel.dtype == torch.int64
        assert (rel == -1).all() and (other == -1).all() and (dist == float('inf')).all()
    set_ptr, _ = none.members('cuda')
    assert ops.entity_typed_plan(set_ptr, num_rels, 's')[1] == 0
    for route in (transe.complete_entities, transe.complete_entities_unfused):
        empty = route(model, ents[:0], 10, type_constraint=tc)
        assert empty[0].shape == (0, 10) and empty[1].shape == (0, 10) and empty[2].shape == (0, 10)


def test_cli_writes_the_typed_entity_profiles(tmp_path, monkeypatch, capsys):
    from gcn_vae_amd import data, ranking, transe
    spec = 'synthetic:60:4:400:40:40'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=16, p_norm=1, norm_flag=True)
    ckpt, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'profiles.tsv')
    model.save_checkpoint(ckpt)
    seen = []
    real = transe.complete_entities

    def spy(*args, **kwargs):
        assert isinstance(kwargs['type_constraint'], ranking.TypeConstraint)
        res = real(*args, **kwargs)
        seen.append((kwargs['side'], args[1].tolist(), res))
        return res
    monkeypatch.setattr(transe, 'complete_entities', spy)
    who, k = [3, 59, 3, 0], 5
    args = transe.build_parser().parse_args(['-d', spec, '--gpu', '0', '--dim', '16', '--test-mode', '--checkpoint', ckpt,
                                             '--profile-topk', str(k), '--profile-typed', '--profile-entities',
                                             ','.join(map(str, who)), '--profile-out', out])
    transe.main(args)
    assert 'type-correct' in capsys.readouterr().out
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert [s for s, _, _ in seen] == ['s', 'o'] and all(e == who for _, e, _ in seen)
    padding = sum(int((res[0] < 0).sum()) for _, _, res in seen)
    assert len(rows) == 2 * len(who) * k - padding and all(len(row) == 6 for row in rows) and rows
    every = np.concatenate([kg.train, kg.valid, kg.test]).tolist()
    known = {tuple(x) for x in every}
    subjects, objects = {(r, s) for s, r, _ in every}, {(r, o) for _, r, o in every}
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
                s, o = (a, int(x)) if side == 's' else (int(x), a)
                assert (s, int(r), o) not in known and s != o
                assert (int(r), s) in subjects and (int(r), o) in objects               # type-correct
    assert at == len(rows)
