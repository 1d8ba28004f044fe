"""Per-entity completion on the KG-VAE posterior predictive on the GPU (gv_entity_topk_scores_mc / gv_entity_topk_scores_typed_mc,
ops.entity_topk_scores{,_typed}_mc, ranking.complete_entities_mc, --mc-profile): the fused sweeps against the rule applied to the
existing Monte-Carlo scorer's own probabilities -- ids and value bits equal, no tolerance --, against each other under an all-full
constraint, under every span geometry, with duplicated samples, saturated, with NaN / inf and ids outside the table, on strided
stacks, against the materialised route within the float64 bound, and through the CLI.  pytest -m gpu."""
import numpy as np
import pytest
import torch

from entity_mc_cases import SHAPES, dense_pbar, dense_pbar_of, dyadic_case, rule, stack_of
from entity_typed_cases import SETTINGS, check_facts, constraint_of, entities, full_constraint, same, setting, tables, trap
from mine_mc_cases import C_SIG, U, pbar64, stack

pytestmark = pytest.mark.gpu

QNAN = 0x7fc00000


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. exact against the existing MC scorer ----------------------------------------------------------------------------------
@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('kind,filtered', [('untyped', False), ('untyped', True)] + SETTINGS)
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('s,n,num_rels,h', SHAPES)
def test_fused_equals_the_rule_on_the_mc_scorers_probabilities(s, n, num_rels, h, side, kind, filtered, with_bias):
    from gcn_vae_amd import ranking
    z, w, bias = stack_of(s, n, num_rels, h, with_bias)
    pbar = dense_pbar_of(s, n, num_rels, h, with_bias)
    _, _, trip, _, perm = tables(n, num_rels, h)
    if kind == 'untyped':
        fi = ranking.FilterIndex(n, num_rels, trip, device='cuda') if filtered else None
        typed, masks = {}, {}
    else:
        tc, fi, cs, co = setting(n, num_rels, h, kind, filtered)
        typed, masks = dict(type_constraint=tc), dict(cand_subj=cs, cand_obj=co)
    for m in (1, 65, n):
        ents = entities(perm, m)
        for k in (1, 10, 128):
            got = ranking.complete_entities_mc(z, w, ents, k, side=side, filter_index=fi, flow_log_probs=bias, **typed)
            assert got[0].shape == (m, k) and got[0].dtype == torch.int64 and got[2].dtype == torch.float32 and got[3].shape == (m, k)
            assert same(got[:3], rule(pbar, ents, k, side, fi, **masks)), (m, k)
            assert bool((got[3] >= 0).all()) and bool((got[3][got[0] < 0] == 0).all())
    assert bool((got[0] >= 0).any())
    if kind != 'untyped':       # every fact of the last (all entities, k = 128) answer is type-correct, no loop and, under a filter, new
        assert check_facts(ents, side, got[0], got[1], cs, co, {tuple(t) for t in trip.tolist()} if filtered else None)


# ---- 2. an all-full constraint is the untyped MC kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('s,n,num_rels,h', SHAPES)
def test_an_all_full_constraint_gives_the_untyped_mc_kernels_answer(s, n, num_rels, h, side):
    from gcn_vae_amd import ranking
    z, w, bias = stack_of(s, n, num_rels, h, True)
    _, _, trip, _, perm = tables(n, num_rels, h)
    full = full_constraint(n, num_rels)
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    for m in (65, n):
        ents = entities(perm, m)
        for k in (10, 128):
            for kw in (dict(), dict(filter_index=fi, flow_log_probs=bias), dict(filter_index=fi, exclude_self=False)):
                got = ranking.complete_entities_mc(z, w, ents, k, side=side, type_constraint=full, **kw)
                want = ranking.complete_entities_mc(z, w, ents, k, side=side, **kw)
                assert same(got[:3], want[:3]) and torch.equal(_bits(got[3]), _bits(want[3])), (m, k, sorted(kw))


# ---- 3. span invariance on tables whose ties cross relations and span cuts ----------------------------------------------------
@pytest.mark.parametrize('span', [None, 1, 2, 5, 10 ** 6])
@pytest.mark.parametrize('typed', [False, True])
def test_dyadic_stacks_tie_across_relations_and_span_boundaries(typed, span):
    """Untyped: 4 relations x 3 column tiles = 12 tiles; typed: 8 tiles (3 + 2 + 2 + 1).  span = 1 cuts after every tile, 2 and 5
    inside and between the relations, 10**6 and the library's own rule (None) not at all.  The order must be the rule's in every
    cut: equal pbar by relation, then by entity."""
    from gcn_vae_amd import ops
    z, w, cs, co = dyadic_case(3)
    pbar = dense_pbar(z, w, None)
    ents = torch.tensor([7, 3, 149, 90, 3, 64, 0], device='cuda')
    masks = dict(cand_subj=cs, cand_obj=co) if typed else {}
    if typed:
        set_ptr, set_ids = constraint_of(cs, co).members('cuda')
        assert ops.entity_typed_plan(set_ptr, 4, 's')[0].tolist() == [0, 3, 5, 7, 8]
    for k in (1, 10, 128):
        for excl in (True, False):
            want = rule(pbar, ents, k, 's', None, excl, **masks)
            if typed:
                got = ops.entity_topk_scores_typed_mc(ents, z, w, k, set_ptr, set_ids, 's', exclude_self=excl, span=span)
            else:
                got = ops.entity_topk_scores_mc(ents, z, w, k, exclude_self=excl, span=span)
            assert same(got, want), (k, excl)
    rel, other, val = got[0].cpu(), got[1].cpu(), got[2].cpu()
    assert (val[:, :-1] == val[:, 1:]).any() and len(rel[rel >= 0].unique()) == 4          # ties are there, every relation shows up
    # the twins, equal in value: relation 0 before relation 2, entity 3 before entity 90
    found = 0
    for row in range(ents.numel()):
        pairs = list(zip(rel[row].tolist(), other[row].tolist()))
        twins = [p for p in pairs if p in ((0, 3), (0, 90), (2, 3), (2, 90))]
        assert twins == sorted(twins)
        if len(twins) == 4:
            at = [pairs.index(p) for p in twins]
            assert len({int(_bits(val[row, i])) for i in at}) == 1
            found += 1
    assert found


# ---- 4. duplicated samples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('typed', [False, True])
@pytest.mark.parametrize('s,n,num_rels,h', SHAPES)
def test_the_same_sample_twice_or_four_times_gives_the_one_samples_values(s, n, num_rels, h, typed):
    """p + p = 2p, 2p + p = 3p rounds to a neighbour at most half a unit of 4p away and + p lands on 4p again (a tie goes to the
    even 4p), and 1 / S is exact: S = 2 and S = 4 copies of a table must give the one table's values bit for bit."""
    from gcn_vae_amd import ops, ranking
    z, w, _ = stack_of(s, n, num_rels, h, True)
    one = z[:1].contiguous()
    bias = torch.tensor([0.37], device='cuda')
    _, _, trip, _, perm = tables(n, num_rels, h)
    tc, fi, _, _ = setting(n, num_rels, h, 'lengths', True)
    lo, hi, ent = ranking._mine_filter(fi, n, num_rels, z.device)
    set_ptr, set_ids = tc.members('cuda')
    ents = entities(perm, 65)

    def run(stack_, b, k=10):
        if typed:
            return ops.entity_topk_scores_typed_mc(ents, stack_, w, k, set_ptr, set_ids, 's', b, lo, hi, ent)
        return ops.entity_topk_scores_mc(ents, stack_, w, k, b, lo, hi, ent)

    base = run(one, bias)
    assert bool((base[0] >= 0).any())
    assert same(run(one.repeat(2, 1, 1), bias.repeat(2)), base)
    assert same(run(one.repeat(4, 1, 1), bias.repeat(4)), base)
    assert same(run(one.repeat(4, 1, 1), bias.repeat(4), k=128), run(one, bias, k=128))
    # S = 1 against the single-sample kernel: the same ids wherever the sigmoids of neighbouring logits differ by more than the
    # device sigmoid's error allows to swap (2 C_SIG u), the k-th against the (k + 1)-th included
    k = 100
    mc = run(one, bias, k=k)
    if typed:
        single = ops.entity_topk_scores_typed(ents, one[0], w, k + 1, set_ptr, set_ids, 's', bias[0], lo, hi, ent)
    else:
        single = ops.entity_topk_scores(ents, one[0], w, k + 1, bias[0], lo, hi, ent)
    sig = torch.sigmoid(single[2].double())
    sig[single[0] < 0] = -1.0
    gap = torch.full_like(sig, float('inf'))
    gap[:, 1:] = torch.minimum(gap[:, 1:], sig[:, :-1] - sig[:, 1:])
    gap[:, :-1] = torch.minimum(gap[:, :-1], sig[:, :-1] - sig[:, 1:])
    clear = (gap[:, :k] > 2 * C_SIG * U) & (single[0][:, :k] >= 0)
    assert bool(clear.any())
    assert torch.equal(mc[0][clear], single[0][:, :k][clear]) and torch.equal(mc[1][clear], single[1][:, :k][clear])


# ---- 5. saturation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('span', [None, 1])
@pytest.mark.parametrize('typed', [False, True])
def test_saturated_candidates_tie_at_one_and_go_by_relation_then_entity(typed, span):
    """A block of 100 entities (more than a tile, fewer than two) whose logits among each other are >= 30 in every sample: pbar
    is exactly 1.0f for all of them, so the list is the first k by (relation, entity) -- 99 of relation 0, then relation 1's --
    across the column tiles' and (span = 1) every span's cut."""
    from gcn_vae_amd import ops
    n, num_rels, h, s, k = 150, 3, 20, 3, 128
    gen = torch.Generator().manual_seed(11)
    block = torch.sort(torch.randperm(n, generator=gen)[:100]).values
    sign = -torch.ones(n)
    sign[block] = 1.0
    z = torch.stack([(1.5 + 0.05 * i) * sign.view(-1, 1) * (1.0 + 0.1 * torch.rand(n, h, generator=gen)) for i in range(s)]).cuda()
    w = (1.0 + 0.1 * torch.rand(num_rels, h, generator=gen)).cuda()
    logits = torch.einsum('sah,rh,sxh->srax', z[:, block].double(), w.double(), z[:, block].double())
    assert float(logits.min()) >= 30.0
    ents = block[[0, 57, 99, 3]].cuda()
    if typed:
        full = torch.ones(num_rels, n, dtype=torch.bool)
        set_ptr, set_ids = constraint_of(full, full).members('cuda')
        rel, other, val = ops.entity_topk_scores_typed_mc(ents, z, w, k, set_ptr, set_ids, 's', span=span)
    else:
        rel, other, val = ops.entity_topk_scores_mc(ents, z, w, k, span=span)
    assert torch.equal(_bits(val), torch.full_like(_bits(val), 0x3f800000))
    for i, a in enumerate(ents.tolist()):
        want = [(r, x) for r in range(num_rels) for x in block.tolist() if x != a][:k]
        assert list(zip(rel[i].tolist(), other[i].tolist())) == want
        assert want[98][0] == 0 and want[99][0] == 1


# ---- 6. NaN, inf, ids outside the table, the filter trap ---------------------------------------------------------------------
def test_nan_in_one_sample_sorts_last_and_inf_logits_give_one():
    from gcn_vae_amd import ops
    s, n, num_rels, h = 3, 40, 2, 20
    z, w, bias, _ = stack(s, n, h, num_rels, 21)
    z, w = z.clone(), w.abs().contiguous()
    z[1, 9] = float('nan')                      # entity 9: NaN in the middle sample only
    z[:, 30] = 1e20                             # entities 30 and 31: (1e20 * w) . 1e20 overflows to +inf in every sample
    z[:, 31] = 2e20
    pbar = dense_pbar(z, w, bias)
    ents = torch.tensor([4, 9, 30, 31, 17], device='cuda')
    for typed in (False, True):
        for k in (10, 128):
            if typed:
                full = torch.ones(num_rels, n, dtype=torch.bool)
                set_ptr, set_ids = constraint_of(full, full).members('cuda')
                got = ops.entity_topk_scores_typed_mc(ents, z, w, k, set_ptr, set_ids, 's', bias)
            else:
                got = ops.entity_topk_scores_mc(ents, z, w, k, bias)
            assert same(got, rule(pbar, ents, k)), (typed, k)
    rel, other, val = (t.cpu() for t in got)
    bits = _bits(val)
    # 2 * 39 = 78 candidates per entity, fewer than k: numbers first, then the NaNs by (relation, entity), then padding
    assert list(zip(rel[0, 76:78].tolist(), other[0, 76:78].tolist())) == [(0, 9), (1, 9)]
    assert bits[0, 76:78].tolist() == [QNAN, QNAN] and not val[0, :76].isnan().any()
    assert (rel[0, 78:] == -1).all() and (other[0, 78:] == -1).all() and (val[0, 78:] == float('-inf')).all()
    # the NaN entity's own list: every candidate NaN, in (relation, entity) order
    assert bits[1, :78].tolist() == [QNAN] * 78
    assert list(zip(rel[1, :78].tolist(), other[1, :78].tolist())) == [(r, x) for r in range(num_rels) for x in range(n) if x != 9]
    # +inf logits: exactly 1.0, under every relation
    for row, x in ((2, 31), (3, 30)):
        hit = (other[row] == x) & (rel[row] >= 0)
        assert int(hit.sum()) == num_rels and bits[row][hit].tolist() == [0x3f800000] * num_rels


def test_query_entities_outside_the_table_give_padding_rows():
    """Through the C entries, as a C caller may pass them (the Python wrappers refuse such ids): -1 and N are dereferenced in no
    sample and give all-padding rows; the rows around them are the wrapper's."""
    from gcn_vae_amd import lib, ops
    s, n, num_rels, h = 3, 70, 7, 37
    z, w, bias = stack_of(s, n, num_rels, h, True)
    tc = setting(n, num_rels, h, 'lengths', False)[0]
    set_ptr, set_ids = tc.members('cuda')
    tile_ptr, n_tiles, cand_base = ops.entity_typed_plan(set_ptr, num_rels, 's')
    tile_ptr = tile_ptr.cuda()
    ents = torch.tensor([5, -1, 69, n, 0, 2 ** 31 - 1, -(2 ** 31)], dtype=torch.int32, device='cuda')
    m, k = ents.numel(), 10
    good = torch.tensor([0, 2, 4], device='cuda')
    for typed in (False, True):
        rel, other = (torch.full((m, k), 7, dtype=torch.int32, device='cuda') for _ in range(2))
        val = torch.zeros(m, k, device='cuda')
        if typed:
            ws_bytes = int(lib.load().gv_entity_topk_scores_typed_workspace_bytes(m, n_tiles, k, 0))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
            lib.call('gv_entity_topk_scores_typed_mc', ents.data_ptr(), m, z.data_ptr(), h, n * h, s, w.data_ptr(), h, bias.data_ptr(), None,
                     None, None, 0, set_ptr.data_ptr(), set_ids.data_ptr(), tile_ptr.data_ptr(), n_tiles, cand_base, 1, k, 0,
                     rel.data_ptr(), other.data_ptr(), val.data_ptr(), ws.data_ptr(), ws_bytes, n, num_rels, h, lib.stream())
            want = ops.entity_topk_scores_typed_mc(ents[good].long(), z, w, k, set_ptr, set_ids, 's', bias)
        else:
            ws_bytes = int(lib.load().gv_entity_topk_scores_workspace_bytes(m, n, num_rels, k))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
            lib.call('gv_entity_topk_scores_mc', ents.data_ptr(), m, z.data_ptr(), h, n * h, s, w.data_ptr(), h, bias.data_ptr(), None, None,
                     None, 0, 1, k, 0, rel.data_ptr(), other.data_ptr(), val.data_ptr(), ws.data_ptr(), ws_bytes, n, num_rels, h,
                     lib.stream())
            want = ops.entity_topk_scores_mc(ents[good].long(), z, w, k, bias)
        torch.cuda.synchronize()
        assert same((rel[good].long(), other[good].long(), val[good]), want), typed
        for row in (1, 3, 5, 6):
            assert (rel[row] == -1).all() and (other[row] == -1).all() and (val[row] == float('-inf')).all(), (typed, row)


@pytest.mark.parametrize('side', ['s', 'o'])
def test_listed_ids_between_two_members_hide_only_themselves_under_mc(side):
    """entity_typed_cases.trap(): the cursor must pass 128 listed non-members between two members and then still hide the two
    listed members behind them -- with the sample loop inside the tile; the untyped sweep takes the same filter."""
    from gcn_vae_amd import ranking
    n, num_rels, a, cq, co, listed, remain = trap()
    z, w, bias = stack_of(2, n, num_rels, 20, True)
    pbar = dense_pbar_of(2, n, num_rels, 20, True)
    cs, cobj = (cq, co) if side == 's' else (co, cq)
    tc = constraint_of(cs, cobj)
    trip = [(q, r, x) if side == 's' else (x, r, q) for q, r, x in listed]
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    ents = torch.tensor([a, 7, 3], device='cuda')                          # 3 is on the query side of no relation
    for excl in (True, False):
        got = ranking.complete_entities_mc(z, w, ents, 128, side=side, filter_index=fi, flow_log_probs=bias, exclude_self=excl,
                                           type_constraint=tc)
        assert same(got[:3], rule(pbar, ents, 128, side, fi, excl, cs, cobj))
        rel, other = got[0].cpu(), got[1].cpu()
        assert sorted(other[0][rel[0] == 1].tolist()) == remain                # 193 and 197 are gone, every other member is there
        assert sorted(other[0][rel[0] == 0].tolist()) == list(range(50)) and int((rel[0] < 0).sum()) == 128 - 57
        assert sorted(other[1][rel[1] == 1].tolist()) == list(range(192, 200))      # entity 7 lists member 5 only
        assert (rel[2] == -1).all() and (got[3][2] == 0).all()
        got = ranking.complete_entities_mc(z, w, ents, 128, side=side, filter_index=fi, flow_log_probs=bias, exclude_self=excl)
        assert same(got[:3], rule(pbar, ents, 128, side, fi, excl))


# ---- 7. strided stacks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s,n,num_rels,h,pad', [(3, 70, 7, 37, 5), (4, 150, 3, 20, 4), (2, 130, 5, 260, 3)])
def test_a_stack_carved_from_a_larger_buffer_gives_the_contiguous_result(s, n, num_rels, h, pad):
    from gcn_vae_amd import ops, ranking
    z, w, bias = stack_of(s, n, num_rels, h, True)
    big = torch.full((s, n + 3, h + pad), float('nan'), device='cuda')
    big[:, :n, :h] = z
    carved = big[:, :n, :h]
    assert carved.stride(0) > n * carved.stride(1) and carved.stride(1) > h and not carved.is_contiguous()
    assert ops._mine_sample_stack(carved, 'z')[0].data_ptr() == big.data_ptr()              # taken as it is, not copied
    big_w = torch.full((num_rels, h + 1), float('nan'), device='cuda')
    big_w[:, :h] = w
    _, _, trip, _, perm = tables(n, num_rels, h)
    tc, fi, _, _ = setting(n, num_rels, h, 'lengths', True)
    lo, hi, ent = ranking._mine_filter(fi, n, num_rels, z.device)
    set_ptr, set_ids = tc.members('cuda')
    ents = entities(perm, 65)
    for k in (10, 128):
        assert same(ops.entity_topk_scores_mc(ents, carved, big_w[:, :h], k, bias, lo, hi, ent), ops.entity_topk_scores_mc(ents, z, w, k, bias, lo, hi, ent))
        assert same(ops.entity_topk_scores_typed_mc(ents, carved, big_w[:, :h], k, set_ptr, set_ids, 'o', bias, lo, hi, ent),
                    ops.entity_topk_scores_typed_mc(ents, z, w, k, set_ptr, set_ids, 'o', bias, lo, hi, ent))


# ---- 8. the wrappers, fused against unfused, within the float64 bound ------------------------------------------------------------
@pytest.mark.parametrize('typed', [False, True])
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('seed', [1, 2])
@pytest.mark.parametrize('s,n,num_rels,h', [(3, 150, 3, 20), (2, 200, 5, 260)])
def test_fused_and_unfused_routes_agree_within_the_float64_bound(s, n, num_rels, h, seed, side, typed):
    """Per row the sets of facts are compared, leaving out the facts whose value lies within 2 eps of that row's k-th value (either
    route may put those on either side of the cut), eps being mine_mc_cases.pbar64's per-element bound: at most 1 % of a case's
    returned facts may be left out.  The means of the common facts agree within eps, the spreads within 1e-5 + 2 eps (the
    tolerance of tests/test_gpu_mc_rank.py).  Prints the worst |pbar - pbar64| / eps."""
    from gcn_vae_amd import ranking
    z, w, bias = stack_of(s, n, num_rels, h, True, seed=seed)
    ref, eps = _pbar64_of(s, n, num_rels, h, seed)
    _, _, trip, _, _ = tables(n, num_rels, h)
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda')
    kw = dict(side=side, filter_index=fi, flow_log_probs=bias)
    if typed:
        kw['type_constraint'] = ranking.TypeConstraint(n, num_rels, trip, device='cuda')
    ents = torch.arange(n, device='cuda')
    worst = 0.0
    for k in (10, 128):
        fused = [t.cpu().numpy() for t in ranking.complete_entities_mc(z, w, ents, k, **kw)]
        unfused = [t.cpu().numpy() for t in ranking.complete_entities_mc_unfused(z, w, ents, k, **kw)]
        returned = left_out = 0
        for a in range(n):
            rows = []
            for rel, other, mean, std in (fused, unfused):
                live = rel[a] >= 0
                r_, x_ = rel[a][live], other[a][live]
                e_ = eps[r_, a, x_]
                kth = mean[a][live][-1] if live.all() else -np.inf                        # a row that is not full holds every candidate
                near = np.abs(mean[a][live] - kth) <= 2 * e_
                rows.append({(int(r), int(x)): (float(p), float(d), float(e), bool(nr))
                             for r, x, p, d, e, nr in zip(r_, x_, mean[a][live], std[a][live], e_, near)})
            f_facts, u_facts = rows
            assert len(f_facts) == len(u_facts), (k, a)
            returned += len(f_facts)
            only_f, only_u = set(f_facts) - set(u_facts), set(u_facts) - set(f_facts)
            # a fact only one route returns lies within 2 eps of that route's k-th value: it is left out of the comparison
            assert all(f_facts[t][3] for t in only_f) and all(u_facts[t][3] for t in only_u), (k, a)
            left_out += max(len(only_f), len(only_u))
            for fact in set(f_facts) & set(u_facts):
                (fp, fd, e, _), (up, ud, _, _) = f_facts[fact], u_facts[fact]
                assert abs(fp - up) <= e and abs(fd - ud) <= 1e-5 + 2 * e, (k, a, fact)
                worst = max(worst, abs(fp - ref[fact[0], a, fact[1]]) / e)
        assert returned > 0 and left_out <= 0.01 * returned, (k, left_out, returned)
        print(f'S={s} N={n} R={num_rels} h={h} seed={seed} side={side} typed={typed} k={k}: {left_out} of {returned} facts near the cut')
    print(f'worst |pbar - pbar64| / eps = {worst:.3f}')


_PBAR64 = {}


def _pbar64_of(s, n, num_rels, h, seed):
    key = (s, n, num_rels, h, seed)
    if key not in _PBAR64:
        _PBAR64[key] = pbar64(*stack_of(s, n, num_rels, h, True, seed=seed))
    return _PBAR64[key]


# ---- 9. the CLI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('typed', [False, True])
def test_cli_writes_reproducible_mc_entity_profiles(tmp_path, typed):
    from gcn_vae_amd import data, ranking, train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:60:4:400:40:40'
    kg = data.load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0, use_cuda=True,
                            reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda().eval()
    ckpt = str(tmp_path / 'm.pth')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    who, k = [3, 59, 3, 0], 5
    texts = []
    for run in range(2):
        out, single = str(tmp_path / f'mc{run}.tsv'), str(tmp_path / f'p{run}.tsv')
        args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                                '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file', ckpt,
                                                '--mc-samples', '4', '--mc-seed', '0', '--profile-topk', str(k), '--profile-entities',
                                                ','.join(map(str, who)), '--profile-out', single, '--mc-profile', '--mc-profile-out',
                                                out] + (['--profile-typed'] if typed else []))
        train.main(args)
        texts.append(open(out).read())
    assert texts[0] == texts[1]                                                 # byte-identical for a fixed seed
    lines = [line.split('\t') for line in texts[0].splitlines()]
    assert lines and all(len(x) == 7 for x in lines)
    every = np.concatenate([kg.train, kg.valid, kg.test]).tolist()
    known = {tuple(x) for x in every}
    subjects, objects = {(r, s) for s, r, _ in every}, {(r, o) for _, r, o in every}
    # ranks run 1 .. n per (entity, side) block, in the order the entities were given, 's' blocks first
    blocks, at = [], 0
    for side in ('s', 'o'):
        for a in who:
            rank = 0
            while at < len(lines) and (int(lines[at][0]), lines[at][1]) == (a, side) and int(lines[at][4]) == rank + 1:
                rank += 1
                at += 1
            blocks.append(rank)
            assert rank <= k
    assert at == len(lines) and sum(blocks) == len(lines)
    if not typed:
        assert blocks == [k] * (2 * len(who))                                   # 4 x 60 candidates: every list is full
    for ent, side, r, x, rank, mean, std in lines:
        a, r, x, mean, std = int(ent), int(r), int(x), float(mean), float(std)
        s, o = (a, x) if side == 's' else (x, a)
        assert (s, r, o) not in known and s != o and 0 <= r < kg.num_rels and 0 <= x < kg.num_nodes
        assert 0.0 <= mean <= 1.0 and 0.0 <= std <= 0.5
        if typed:
            assert (r, s) in subjects and (r, o) in objects
    # the first five columns are --profile-out's: well-formed in both files, so they join
    plain = [line.split('\t') for line in open(str(tmp_path / 'p1.tsv')).read().splitlines()]
    assert plain and all(len(x) == 7 for x in plain)
    for row in lines + plain:
        assert row[1] in ('s', 'o') and all(v.lstrip('-').isdigit() for v in (row[0], row[2], row[3], row[4])) and int(row[4]) >= 1
    assert {(row[0], row[1]) for row in lines} <= {(row[0], row[1]) for row in plain}
    # means do not rise along a block
    at = 0
    for n_rows in blocks:
        means = [float(x[5]) for x in lines[at:at + n_rows]]
        assert means == sorted(means, reverse=True)
        at += n_rows
