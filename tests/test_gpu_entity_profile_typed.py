"""Per-entity completion among type-correct facts on the GPU (gv_entity_topk_scores_typed / ops.entity_topk_scores_typed /
ranking.complete_entities(type_constraint=)): the fused sweep over the relations' member lists against the materialised route
under the same constraint, against the untyped fused kernel under an all-full constraint, and against the merge over relations of
ranking.predict_topk(type_constraint=) -- ids equal, logit bits equal, no tolerance anywhere.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from entity_typed_cases import (SETTINGS, SHAPES, check_facts, constraint_of, entities, full_constraint, same, setting, tables, trap)

pytestmark = pytest.mark.gpu

FLP = 0.37


@pytest.mark.parametrize('flp', [None, FLP])
@pytest.mark.parametrize('kind,filtered', SETTINGS)
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('n,num_rels,h', SHAPES)
def test_fused_equals_unfused_exactly(n, num_rels, h, side, kind, filtered, flp):
    from gcn_vae_amd import ranking
    emb, w, trip, _, perm = tables(n, num_rels, h)
    tc, fi, cs, co = setting(n, num_rels, h, kind, filtered)
    bias = None if flp is None else torch.tensor(flp, device='cuda')
    for m in (1, 64, 65, n):
        ents = entities(perm, m)
        for k in (1, 10, 128):
            got = ranking.complete_entities(emb, w, ents, k, side=side, filter_index=fi, flow_log_prob=bias, type_constraint=tc)
            want = ranking.complete_entities_unfused(emb, w, ents, k, side=side, filter_index=fi, flow_log_prob=bias, type_constraint=tc)
            assert got[0].shape == (m, k) and got[0].dtype == torch.int64 and got[2].dtype == torch.float32
            assert same(got, want), (m, k)
    # every fact of the last (all entities, k = 128) answer is type-correct, no loop and, under a filter, new
    known = {tuple(t) for t in trip.tolist()} if filtered else None
    facts = check_facts(ents, side, got[0], got[1], cs, co, known)
    assert facts


@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('n,num_rels,h', SHAPES)
def test_an_all_full_constraint_gives_the_untyped_kernels_answer(n, num_rels, h, side):
    """Ties the new kernel to the existing one bit for bit: with every set full the member lists are 0 .. N - 1, the gathered tiles
    are the untyped kernel's tiles, and the two fused routes must agree in every id and every logit bit."""
    from gcn_vae_amd import ranking
    emb, w, trip, _, perm = tables(n, num_rels, h)
    full = full_constraint(n, num_rels)
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    bias = torch.tensor(FLP, device='cuda')
    for m in (65, n):
        ents = entities(perm, m)
        for k in (10, 128):
            for kw in (dict(), dict(filter_index=fi, flow_log_prob=bias), dict(filter_index=fi, exclude_self=False)):
                got = ranking.complete_entities(emb, w, ents, k, side=side, type_constraint=full, **kw)
                assert same(got, ranking.complete_entities(emb, w, ents, k, side=side, **kw)), (m, k, sorted(kw))


@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('n,num_rels,h', SHAPES)
def test_fused_equals_the_merge_of_predict_topk(n, num_rels, h, side):
    """Per relation ranking.predict_topk(type_constraint=) gives the k best type-correct answers of the queries (a, r) with a on
    the query side of r; their merge by (logit, r, x) is the entity's list (exclude_self off: predict_topk keeps the loops)."""
    from gcn_vae_amd import ranking
    emb, w, _, _, perm = tables(n, num_rels, h)
    tc, fi, cs, co = setting(n, num_rels, h, 'lengths', True)
    ents, k = entities(perm, 65), 10
    bias = torch.tensor(FLP, device='cuda')
    on_query_side = (cs if side == 's' else co).cuda()
    pool = torch.zeros(65, num_rels, n, device='cuda')
    given = torch.zeros(65, num_rels, n, dtype=torch.bool, device='cuda')
    for r in range(num_rels):
        rows = torch.nonzero(on_query_side[r, ents]).flatten()
        if not rows.numel():
            continue
        ids, logits = ranking.predict_topk(emb, w, ents[rows], torch.full_like(ents[rows], r), k, direction='o' if side == 's' else 's',
                                           filter_index=fi, flow_log_prob=bias, type_constraint=tc)
        live = ids >= 0
        at = rows.view(-1, 1).expand_as(ids)
        pool[at[live], r, ids[live]] = logits[live]
        given[at[live], r, ids[live]] = True
    want_ids, want_logits = ranking.topk_from_scores(pool.view(65, -1), k, cand=given.view(65, -1))
    got = ranking.complete_entities(emb, w, ents, k, side=side, filter_index=fi, flow_log_prob=bias, exclude_self=False, type_constraint=tc)
    gone = got[0] < 0
    assert torch.equal(torch.where(gone, got[0], got[0] * n + got[1]), want_ids)
    assert torch.equal(got[2].view(torch.int32), want_logits.view(torch.int32))
    assert given.any()


def _dyadic_case():
    """The untyped test's integer tables -- relations 0 and 2 the same row of w, entities 3 and 90 the same row of emb -- under a
    constraint that keeps both twins as candidates of both relations.  Candidate lists (side 's'): relation 0 all but three ids
    (147 members, three tiles: the twins sit in tiles 0 and 1), relation 1 65 random members (two tiles), relation 2 the even ids
    and 3 (76 members, two tiles: the twins share tile 0), relation 3 30 members (one tile): 8 tiles."""
    gen = torch.Generator().manual_seed(5)
    n, num_rels, h = 150, 4, 6
    emb = torch.randint(-2, 3, (n, h), generator=gen).float()
    emb[90] = emb[3]
    w = torch.randint(-1, 2, (num_rels, h), generator=gen).float()
    w[2] = w[0]
    score = torch.einsum('ah,rh,xh->arx', emb.double(), w.double(), emb.double()).float()      # exact: integers below 2^24
    co = torch.zeros(num_rels, n, dtype=torch.bool)
    co[0] = True
    co[0, [10, 20, 30]] = False
    co[1, torch.randperm(n, generator=gen)[:65]] = True
    co[2, 0::2] = True
    co[2, 3] = True
    co[3, torch.randperm(n, generator=gen)[:30]] = True
    cs = torch.rand(num_rels, n, generator=gen) < 0.5
    cs[0], cs[2] = True, True
    return emb.cuda(), w.cuda(), score, cs, co


@pytest.mark.parametrize('span', [None, 1, 2, 5, 10 ** 6])
def test_dyadic_tables_tie_across_relations_and_span_boundaries(span):
    """8 tiles: span = 1 cuts after every tile (inside every list of more than 64), 2 at the relations' ends only, 5 inside relation
    2's list, 10**6 and the library's own rule not at all.  The order must be the rule's in every cut."""
    from gcn_vae_amd import ops, ranking
    emb, w, score, cs, co = _dyadic_case()
    set_ptr, set_ids = constraint_of(cs, co).members('cuda')
    assert ops.entity_typed_plan(set_ptr, 4, 's')[0].tolist() == [0, 3, 5, 7, 8]
    ents = torch.tensor([7, 3, 149, 90, 3, 64, 0], device='cuda')
    for k in (1, 10, 128):
        for excl in (True, False):
            want = ranking.complete_entities_from_scores(score[ents.cpu()], ents.cpu(), k, exclude_self=excl, cand_query=cs, cand_other=co)
            got = ops.entity_topk_scores_typed(ents, emb, w, k, set_ptr, set_ids, 's', exclude_self=excl, span=span)
            assert same(tuple(t.cpu() for t in got), want), (k, excl)
    rel, other = got[0].cpu(), got[1].cpu()
    assert (want[2][:, :-1] == want[2][:, 1:]).any() and len(rel[rel >= 0].unique()) == 4      # ties are there, every relation shows up
    # the twins, adjacent in one list and equal in value: relation 0 before relation 2, entity 3 before entity 90
    for row in range(ents.numel()):
        pairs = list(zip(rel[row].tolist(), other[row].tolist()))
        twins = [p for p in pairs if p in ((0, 3), (0, 90), (2, 3), (2, 90))]
        assert twins == sorted(twins)


@pytest.mark.parametrize('n,num_rels,h,k', [(150, 3, 20, 10), (130, 5, 260, 128), (70, 7, 37, 128)])
def test_result_does_not_depend_on_the_span_geometry(n, num_rels, h, k):
    from gcn_vae_amd import ops, ranking
    emb, w, _, _, perm = tables(n, num_rels, h)
    tc, fi, _, _ = setting(n, num_rels, h, 'lengths', True)
    lo, hi, ent = ranking._mine_filter(fi, n, num_rels, emb.device)
    set_ptr, set_ids = tc.members('cuda')
    ents = entities(perm, 65)
    base = ops.entity_topk_scores_typed(ents, emb, w, k, set_ptr, set_ids, 's', None, lo, hi, ent)
    assert (base[0] >= 0).any()
    for span in (1, 2, 4, 7, 10 ** 6):
        assert same(ops.entity_topk_scores_typed(ents, emb, w, k, set_ptr, set_ids, 's', None, lo, hi, ent, span=span), base), span


@pytest.mark.parametrize('side', ['s', 'o'])
def test_listed_ids_between_two_members_hide_only_themselves(side):
    """The filter trap: the cursor must pass 128 listed non-members between two members (more than one window of 64) and then still
    hide the two listed members behind them."""
    from gcn_vae_amd import ranking
    n, num_rels, a, cq, co, listed, remain = trap()
    emb, w = tables(n, 1, 200)[0], tables(150, 3, 20)[1][:2].repeat(1, 10).contiguous()
    cs, cobj = (cq, co) if side == 's' else (co, cq)
    tc = constraint_of(cs, cobj)
    trip = [(q, r, x) if side == 's' else (x, r, q) for q, r, x in listed]
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    ents = torch.tensor([a, 7, 3], device='cuda')                          # 3 is on the query side of no relation
    for excl in (True, False):
        got = ranking.complete_entities(emb, w, ents, 128, side=side, filter_index=fi, exclude_self=excl, type_constraint=tc)
        assert same(got, ranking.complete_entities_unfused(emb, w, ents, 128, side=side, filter_index=fi, exclude_self=excl,
                                                           type_constraint=tc))
        rel, other = got[0].cpu(), got[1].cpu()
        assert sorted(other[0][rel[0] == 1].tolist()) == remain                # 193 and 197 are gone, every other member is there
        assert sorted(other[0][rel[0] == 0].tolist()) == list(range(50)) and int((rel[0] < 0).sum()) == 128 - 57
        assert sorted(other[1][rel[1] == 1].tolist()) == list(range(192, 200))      # entity 7 lists member 5 only
        assert (rel[2] == -1).all()


def test_padding_and_the_lists_that_end_at_a_tile_boundary():
    from gcn_vae_amd import ops, ranking
    n, num_rels = 150, 4
    emb, w = tables(150, 3, 20)[0], tables(70, 7, 37)[1][:4, :20].contiguous()
    co = torch.zeros(num_rels, n, dtype=torch.bool)
    co[0, 10:74] = True                                                     # exactly 64 candidates
    co[1, torch.arange(0, 130, 2)] = True                                   # 65
    co[3, 149] = True                                                       # 1; relation 2 has none
    cs = torch.zeros(num_rels, n, dtype=torch.bool)
    cs[:, :100] = True                                                      # entities 100 .. 149 are on the query side of nothing
    cs[2, :] = True                                                         # ... but of the relation without candidates
    tc = constraint_of(cs, co)
    ents = torch.tensor([0, 120, 12, 149, 99], device='cuda')
    got = ranking.complete_entities(emb, w, ents, 128, type_constraint=tc)
    assert same(got, ranking.complete_entities_unfused(emb, w, ents, 128, type_constraint=tc))
    rel, other, logits = (t.cpu() for t in got)
    for row in (1, 3):
        assert (rel[row] == -1).all() and (other[row] == -1).all() and (logits[row] == float('-inf')).all()
    # entity 12 is a candidate of relations 0 and 1 itself: 63 + 64 + 0 + 1 candidates without its loops, exactly k
    assert [int((rel[2] == r).sum()) for r in range(num_rels)] == [63, 64, 0, 1]
    for row in (0, 4):                                                      # 129 and 130 candidates: a full list, none of relation 2
        assert (rel[row] >= 0).all() and not (rel[row] == 2).any()
    # no tile at all: every candidate list empty
    none = constraint_of(cs, torch.zeros(num_rels, n, dtype=torch.bool))
    for k in (1, 100):
        rel, other, logits = ranking.complete_entities(emb, w, ents, k, type_constraint=none)
        assert rel.shape == other.shape == logits.shape == (5, k)
        assert (rel == -1).all() and (other == -1).all() and (logits == float('-inf')).all()
    set_ptr, set_ids = none.members('cuda')
    assert ops.entity_typed_plan(set_ptr, num_rels, 's')[1] == 0 and ops.entity_typed_plan(set_ptr, num_rels, 'o')[1] > 0
    empty = ranking.complete_entities(emb, w, ents[:0], 10, type_constraint=tc)
    assert empty[0].shape == (0, 10) and empty[1].shape == (0, 10) and empty[2].shape == (0, 10)


def test_cli_writes_the_typed_entity_profiles(tmp_path, monkeypatch, capsys):
    from gcn_vae_amd import ranking, train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:60:4:400:40:40'
    kg = __import__('gcn_vae_amd.data', fromlist=['load_data']).load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt, out = str(tmp_path / 'm.pth'), str(tmp_path / 'profiles.tsv')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    seen = []
    real = ranking.complete_entities

    def spy(*args, **kwargs):
        assert isinstance(kwargs['type_constraint'], ranking.TypeConstraint)
        res = real(*args, **kwargs)
        seen.append((kwargs['side'], args[2].tolist(), res))
        return res
    monkeypatch.setattr(ranking, 'complete_entities', spy)
    who, k = [3, 59, 3, 0], 5
    args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                            '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file', ckpt,
                                            '--profile-topk', str(k), '--profile-typed', '--profile-entities', ','.join(map(str, who)),
                                            '--profile-out', out])
    train.main(args)
    assert 'type-correct' in capsys.readouterr().out
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert [s for s, _, _ in seen] == ['s', 'o'] and all(e == who for _, e, _ in seen)
    padding = sum(int((res[0] < 0).sum()) for _, _, res in seen)
    assert len(rows) == 2 * len(who) * k - padding and all(len(row) == 7 for row in rows) and rows
    every = np.concatenate([kg.train, kg.valid, kg.test]).tolist()
    known = {tuple(x) for x in every}
    subjects, objects = {(r, s) for s, r, _ in every}, {(r, o) for _, r, o in every}
    at = 0
    for side, ents, res in seen:
        rel, other, logits = (t.cpu() for t in res)
        for i, a in enumerate(ents):
            for j in range(k):
                if rel[i, j] < 0:
                    continue
                ent, sd, r, x, rank, logit, prob = rows[at]
                at += 1
                assert (int(ent), sd, int(r), int(x), int(rank)) == (a, side, int(rel[i, j]), int(other[i, j]), j + 1)
                assert np.float32(logit) == logits[i, j].numpy()                      # nine digits give the float32 back
                s, o = (a, int(x)) if side == 's' else (int(x), a)
                assert (s, int(r), o) not in known and s != o
                assert (int(r), s) in subjects and (int(r), o) in objects               # type-correct
    assert at == len(rows)
