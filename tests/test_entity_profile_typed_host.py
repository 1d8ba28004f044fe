"""Per-entity completion among type-correct facts, host side (no GPU), for both models: the two materialised rules under a
constraint against a brute-force Python enumeration, the tile prefix of ops.entity_typed_plan, the refusals and workspace sizes of
gv_entity_topk_scores_typed / gv_transe_entity_topk_typed before any launch, the wrappers' refusals, and --profile-typed."""
import ctypes
import itertools
import struct

import pytest
import torch

NAN, INF = float('nan'), float('inf')
N, R = 9, 3
SHAPE, NULL = -2, -1


def _bits(x):
    return struct.unpack('<I', struct.pack('<f', x))[0]


def _brute(val, entities, k, allowed_query, allowed_other, listed, exclude_self, ascending):
    """The rule, one candidate at a time.  ``allowed_query[r]`` / ``allowed_other[r]``: Python sets of the entities allowed on the
    query side / the candidate side of relation r; ``listed`` maps (entity, relation) to the ids that are no candidates there."""
    m, num_rels, n = val.shape
    pad = _bits(INF if ascending else -INF)
    rows = []
    for i, a in enumerate(entities):
        cands = []
        for r in range(num_rels):
            if a not in allowed_query[r]:
                continue
            hidden = set((listed or {}).get((a, r), ()))
            for x in range(n):
                if x not in allowed_other[r] or x in hidden or (exclude_self and x == a):
                    continue
                v = float(val[i, r, x])
                nan = v != v
                v = 0.0 if v == 0.0 else v
                cands.append((1 if nan else 0, 0.0 if nan else (v if ascending else -v), r, x, 0x7fc00000 if nan else _bits(v)))
        cands.sort(key=lambda c: c[:4])
        rows.append(cands[:k] + [(0, 0.0, -1, -1, pad)] * max(0, k - len(cands)))
    return ([[c[2] for c in row] for row in rows], [[c[3] for c in row] for row in rows], [[c[4] for c in row] for row in rows])


def _dense_filter(listed, n, num_rels):
    lo, hi, ent = [], [], []
    for a in range(n):
        for r in range(num_rels):
            lo.append(len(ent))
            ent.extend(sorted(set(listed.get((a, r), ()))))
            hi.append(len(ent))
    return torch.tensor(lo), torch.tensor(hi), torch.tensor(ent, dtype=torch.int64)


def _masks(sets):
    out = torch.zeros(len(sets), N, dtype=torch.bool)
    for r, members in enumerate(sets):
        out[r, sorted(members)] = True
    return out


# subjects / objects per relation: entity 8 is in no set; relation 1 has no object (an empty candidate list for side 's') but
# subjects; relation 2 is full on both sides
SUBJ = [{0, 1, 4}, {2, 4, 5}, set(range(N))]
OBJ = [{1, 2, 3, 7}, set(), set(range(N))]
SUBJ_NO8 = [SUBJ[0], SUBJ[1], set(range(8))]
OBJ_NO8 = [OBJ[0], OBJ[1], set(range(8))]
ENTS = [4, 8, 0, 4, 2, 7]                                                     # 4 repeated; 8 outside every set of *_NO8
LISTED = {(4, 0): [1, 5, 7], (4, 2): [0, 4, 8], (0, 0): [3], (2, 2): list(range(N)), (7, 2): [6], (2, 1): [4]}


def _values(ascending):
    gen = torch.Generator().manual_seed(11)
    val = torch.randint(0 if ascending else -4, 5, (len(ENTS), R, N), generator=gen).float() * 0.25      # ties everywhere
    val[0, 2, 3], val[2, 0, 1] = NAN, NAN
    val[0, 0, 2] = INF
    val[3] = val[0]                                                          # the repeated entity's row
    if not ascending:
        val[val == 0.0] = -0.0
        val[4, 2, 1] = 0.0
    return val


@pytest.mark.parametrize('exclude_self', [True, False])
@pytest.mark.parametrize('filtered', [False, True])
@pytest.mark.parametrize('side', ['s', 'o'])
@pytest.mark.parametrize('model', ['distmult', 'transe'])
def test_the_rules_under_a_constraint_equal_a_python_enumeration(model, side, filtered, exclude_self):
    from gcn_vae_amd import ranking, transe
    ascending = model == 'transe'
    rule = transe.complete_entities_from_distances if ascending else ranking.complete_entities_from_scores
    val = _values(ascending)
    query, other = (SUBJ_NO8, OBJ_NO8) if side == 's' else (OBJ_NO8, SUBJ_NO8)
    filt = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), _dense_filter(LISTED, N, R))) if filtered else {}
    for k in (1, 4, 128):
        rel, oth, out = rule(val, torch.tensor(ENTS), k, exclude_self=exclude_self, cand_query=_masks(query), cand_other=_masks(other),
                             **filt)
        assert rel.dtype == torch.int64 and oth.dtype == torch.int64 and out.dtype == torch.float32 and rel.shape == (len(ENTS), k)
        want = _brute(val, ENTS, k, query, other, LISTED if filtered else None, exclude_self, ascending)
        assert rel.tolist() == want[0] and oth.tolist() == want[1]
        assert [[b & 0xffffffff for b in row] for row in out.view(torch.int32).tolist()] == want[2]
        assert (rel[1] == -1).all() and (oth[1] == -1).all()                 # entity 8: on the query side of no relation
        assert torch.equal(rel[0], rel[3]) and torch.equal(oth[0], oth[3])    # the repeated entity repeats its row
    if side == 's':
        assert not (rel == 1).any()                                          # relation 1 has no candidate object
    # an id outside [0, N) is an all-padding row under a constraint
    rel, oth, out = rule(val[:2], torch.tensor([4, N]), 3, cand_query=_masks(query), cand_other=_masks(other))
    assert (rel[1] == -1).all() and (oth[1] == -1).all() and torch.isinf(out[1]).all() and (rel[0] >= 0).any()


@pytest.mark.parametrize('model', ['distmult', 'transe'])
def test_a_constraint_whose_every_set_is_full_changes_nothing(model):
    from gcn_vae_amd import ranking, transe
    ascending = model == 'transe'
    rule = transe.complete_entities_from_distances if ascending else ranking.complete_entities_from_scores
    val = _values(ascending)
    full = torch.ones(R, N, dtype=torch.bool)
    filt = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), _dense_filter(LISTED, N, R)))
    for kw in ({}, filt):
        for excl in (True, False):
            for k in (1, 5, 128):
                a = rule(val, torch.tensor(ENTS), k, exclude_self=excl, **kw)
                b = rule(val, torch.tensor(ENTS), k, exclude_self=excl, cand_query=full, cand_other=full, **kw)
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    with pytest.raises(ValueError, match='together'):
        rule(val, torch.tensor(ENTS), 3, cand_query=full)
    with pytest.raises(ValueError, match='expected bool'):
        rule(val, torch.tensor(ENTS), 3, cand_query=full[:2], cand_other=full)


def test_complete_masks_are_the_sets_of_the_constraint_seen_from_one_entity():
    from gcn_vae_amd import ranking
    trip = [[0, 0, 1], [4, 0, 7], [1, 0, 2], [2, 1, 5], [5, 1, 5]]
    tc = ranking.TypeConstraint(N, R, trip)
    cq, co = ranking.complete_masks(tc, 's')
    assert torch.equal(cq, _masks([{0, 4, 1}, {2, 5}, set()])) and torch.equal(co, _masks([{1, 7, 2}, {5}, set()]))
    oq, oo = ranking.complete_masks(tc, 'o')
    assert torch.equal(oq, co) and torch.equal(oo, cq)
    with pytest.raises(ValueError, match='side'):
        ranking.complete_masks(tc, 'x')


def test_tile_prefix_for_the_member_counts_that_matter():
    from gcn_vae_amd import ops
    counts_o, counts_s = [0, 1, 63, 64, 65, 129], [129, 65, 64, 63, 1, 0]
    ptr = torch.tensor([0] + list(itertools.accumulate(counts_o + counts_s)))
    tile_ptr, n_tiles, cand_base = ops.entity_typed_plan(ptr, 6, 's')
    assert tile_ptr.dtype == torch.int32 and tile_ptr.tolist() == [0, 0, 1, 2, 3, 5, 8] and n_tiles == 8 and cand_base == 0
    tile_ptr, n_tiles, cand_base = ops.entity_typed_plan(ptr, 6, 'o')
    assert tile_ptr.tolist() == [0, 3, 5, 6, 7, 8, 8] and n_tiles == 8 and cand_base == 6
    tile_ptr, n_tiles, _ = ops.entity_typed_plan(torch.zeros(5, dtype=torch.int64), 2, 's')
    assert tile_ptr.tolist() == [0, 0, 0] and n_tiles == 0
    with pytest.raises(ValueError, match='side'):
        ops.entity_typed_plan(ptr, 6, 'x')


def _refusals(entry, call, p):
    from gcn_vae_amd import lib

    def refused(code, text, **kw):
        rc = call(**kw)
        err = lib.last_error()
        assert rc == code, (kw, rc, err)
        assert err.startswith(entry + ':') and text in err, (kw, err)

    refused(SHAPE, 'k=0', k=0)
    refused(SHAPE, 'k=129', k=129)
    assert call(m=0, k=0) == SHAPE                                          # sizes are looked at even without queries
    refused(SHAPE, 'm=-1', m=-1)
    refused(SHAPE, 'n=0', n=0)
    refused(SHAPE, 'num_rels=0', num_rels=0)
    refused(SHAPE, 'n_filt_ent=-1', n_ent=-1, lo=p, hi=p, ent=p)
    refused(SHAPE, '31 bits', n=1 << 16, num_rels=1 << 15, cand_base=1 << 15)
    refused(SHAPE, 'span_tiles=-1', span=-1)
    refused(SHAPE, 'n_tiles=-1', n_tiles=-1)
    refused(SHAPE, 'cand_base=1', cand_base=1)
    refused(SHAPE, 'cand_base=-3', cand_base=-3)
    for given in (dict(lo=p), dict(hi=p), dict(ent=p), dict(lo=p, hi=p), dict(lo=p, ent=p), dict(hi=p, ent=p)):
        refused(NULL, 'all given or all NULL', n_ent=1, **given)
    for missing in ('ents', 'tab_a', 'tab_b', 'rel', 'other', 'val', 'ws'):
        refused(NULL, 'NULL pointer', **{missing: None})
    for missing in ('set_ptr', 'set_ids', 'tile_ptr'):
        refused(NULL, 'NULL set_ptr / set_ids / tile_ptr', **{missing: None})
    # 5 tiles, m = 4, k = 5: the library's rule makes one span (fewer than 16 tiles); span = 2 makes three
    refused(SHAPE, 'workspace of 159 bytes, 160 needed', ws_bytes=4 * 5 * 8 - 1)
    refused(SHAPE, 'workspace of 479 bytes, 480 needed', span=2, ws_bytes=3 * 4 * 5 * 8 - 1)
    refused(SHAPE, 'workspace of 159 bytes, 160 needed', n_tiles=0, ws_bytes=4 * 5 * 8 - 1)      # no tile: one span of padding
    # m == 0 returns before the pointers are looked at
    assert call(ents=None, m=0, tab_a=None, tab_b=None, rel=None, other=None, val=None, ws=None, ws_bytes=0, set_ptr=None, set_ids=None,
                tile_ptr=None) == 0


def test_distmult_entry_refuses_bad_arguments_before_any_launch():
    from gcn_vae_amd import lib
    entry = 'gv_entity_topk_scores_typed'
    fn = getattr(lib.load(), entry)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def call(ents=p, m=4, tab_a=p, ld_e=8, tab_b=p, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, set_ptr=p, set_ids=p, tile_ptr=p,
             n_tiles=5, cand_base=0, k=5, span=0, rel=p, other=p, val=p, ws=p, ws_bytes=1 << 20, n=10, num_rels=3, h=8):
        return fn(ents, m, tab_a, ld_e, tab_b, ld_w, None, lo, hi, ent, n_ent, set_ptr, set_ids, tile_ptr, n_tiles, cand_base, 1, k, span,
                  rel, other, val, ws, ws_bytes, n, num_rels, h, None)

    _refusals(entry, call, p)
    for kw, text in ((dict(h=0), 'h=0'), (dict(ld_e=7), 'leading dimension'), (dict(ld_w=7), 'leading dimension')):
        assert call(**kw) == SHAPE and lib.last_error().startswith(entry + ':') and text in lib.last_error()
    assert call(cand_base=3, ws_bytes=0) == SHAPE and 'workspace' in lib.last_error()       # cand_base = R itself passes


def test_transe_entry_refuses_bad_arguments_before_any_launch():
    from gcn_vae_amd import lib
    entry = 'gv_transe_entity_topk_typed'
    fn = getattr(lib.load(), entry)
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def call(ents=p, m=4, tab_a=p, tab_b=p, n=10, num_rels=3, dim=8, head=0, p_norm=1, lo=None, hi=None, ent=None, n_ent=0, set_ptr=p,
             set_ids=p, tile_ptr=p, n_tiles=5, cand_base=0, k=5, span=0, rel=p, other=p, val=p, ws=p, ws_bytes=1 << 20):
        return fn(ents, m, tab_a, tab_b, n, num_rels, dim, head, p_norm, lo, hi, ent, n_ent, set_ptr, set_ids, tile_ptr, n_tiles, cand_base,
                  1, k, span, rel, other, val, ws, ws_bytes, None)

    _refusals(entry, call, p)
    for kw, text in ((dict(dim=0), 'dim=0'), (dict(dim=513), 'dim=513'), (dict(p_norm=3), 'p_norm=3')):
        assert call(**kw) == SHAPE and lib.last_error().startswith(entry + ':') and text in lib.last_error()
    assert call(cand_base=3, head=1, ws_bytes=0) == SHAPE and 'workspace' in lib.last_error()


@pytest.mark.parametrize('entry', ['gv_entity_topk_scores_typed', 'gv_transe_entity_topk_typed'])
def test_workspace_bytes(entry):
    from gcn_vae_amd import lib
    ws = getattr(lib.load(), entry + '_workspace_bytes')
    for bad in ((0, 5, 5, 0), (-1, 5, 5, 0), (4, -1, 5, 0), (4, 5, 0, 0), (4, 5, 129, 0), (4, 5, 5, -1)):
        assert ws(*bad) == 0, bad
    # a given span_tiles: m * ceil(T / span_tiles) * k * 8, span_tiles capped at T; no tile at all is one span of padding
    for m, tiles, k, span in ((4, 5, 5, 1), (4, 5, 5, 2), (4, 5, 5, 100), (65, 37, 128, 4), (1, 3600, 10, 7), (3, 1, 1, 1)):
        per = min(span, tiles)
        assert ws(m, tiles, k, span) == m * ((tiles + per - 1) // per) * k * 8, (m, tiles, k, span)
    assert ws(4, 0, 5, 0) == 4 * 5 * 8 and ws(4, 0, 5, 3) == 4 * 5 * 8

    # the library's rule (k_topk.h, topk_spans_of with at most 256 spans): about 1024 workgroups, spans of at least 8 tiles
    def rule(m, tiles):
        row_tiles = (m + 63) // 64
        s = max(1, min((1024 + row_tiles - 1) // row_tiles, max(1, tiles // 8), 256))
        per = (tiles + s - 1) // s
        return (tiles + per - 1) // per

    for m, tiles, k in ((1, 3600, 100), (14541, 3600, 100), (40943, 700, 128), (65, 9, 10), (1, 17, 3)):
        assert ws(m, tiles, k, 0) == m * rule(m, tiles) * k * 8, (m, tiles, k)
    assert rule(1, 3600) > 200                                               # a single entity is spread over the chip


def _members(n, num_rels):
    from gcn_vae_amd import ranking
    return ranking.TypeConstraint(n, num_rels, [[1, 0, 2], [4, 2, 4], [3, 1, 0]]).members()


def test_wrappers_refuse_before_any_device_is_touched():
    from gcn_vae_amd import ops
    emb, w, ents = torch.zeros(10, 8), torch.zeros(3, 8), torch.tensor([4, 1, 4])
    ptr, ids = _members(10, 3)
    for call in (lambda *a, **kw: ops.entity_topk_scores_typed(ents, emb, w, *a, **kw),
                 lambda k, *a, **kw: ops.transe_entity_topk_typed(ents, emb, w, k, 1, *a, **kw)):
        for k in (0, 129):
            with pytest.raises(ValueError, match='k must lie'):
                call(k, ptr, ids)
        with pytest.raises(ValueError, match='span'):
            call(5, ptr, ids, span=0)
        with pytest.raises(RuntimeError, match='no CPU fallback'):           # valid arguments: the device check, no launch
            call(5, ptr, ids)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.entity_topk_scores_typed(torch.tensor([4, 10]), emb, w, 5, ptr, ids)
    with pytest.raises(ValueError, match='31 bits'):
        ops.entity_topk_scores_typed(ents, torch.zeros(1 << 16, 1), torch.zeros(1 << 15, 1), 5, ptr, ids)
    with pytest.raises(ValueError, match='width 513'):
        ops.transe_entity_topk_typed(ents, torch.zeros(10, 513), torch.zeros(3, 513), 5, 1, ptr, ids)
    with pytest.raises(ValueError, match='1 or 2'):
        ops.transe_entity_topk_typed(ents, emb, w, 5, 3, ptr, ids)


def test_a_constraint_built_for_other_sizes_is_refused():
    from gcn_vae_amd import ranking, transe
    emb, w, ents = torch.zeros(10, 8), torch.zeros(3, 8), torch.tensor([4, 1, 4])
    for tc in (ranking.TypeConstraint(11, 3, [[1, 0, 2]]), ranking.TypeConstraint(10, 4, [[1, 0, 2]])):
        for route in (ranking.complete_entities, ranking.complete_entities_unfused):
            with pytest.raises(ValueError, match='the TypeConstraint is for'):
                route(emb, w, ents, 5, type_constraint=tc)
        for route in (transe.complete_entities, transe.complete_entities_unfused):
            with pytest.raises(ValueError, match='the TypeConstraint is for'):
                route((emb, w, 1, True), ents, 5, type_constraint=tc)
    good = ranking.TypeConstraint(10, 3, [[1, 0, 2]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):               # the right sizes: the device check, no launch
        ranking.complete_entities(emb, w, ents, 5, type_constraint=good)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        transe.complete_entities((emb, w, 1, True), ents, 5, side='o', type_constraint=good)


def test_the_unconstrained_call_leaves_the_argument_out():
    """The default is the sentinel ranking.UNCONSTRAINED; anything that is not a TypeConstraint -- an explicit None too -- is a
    TypeError ahead of every other check, on both models and both routes."""
    from gcn_vae_amd import ranking, transe
    emb, w, ents = torch.zeros(10, 8), torch.zeros(3, 8), torch.tensor([4, 1, 4])
    calls = [lambda **kw: ranking.complete_entities(emb, w, ents, 5, **kw), lambda **kw: ranking.complete_entities_unfused(emb, w, ents, 5, **kw),
             lambda **kw: transe.complete_entities((emb, w, 1, True), ents, 5, **kw),
             lambda **kw: transe.complete_entities_unfused((emb, w, 1, True), ents, 5, **kw)]
    for call in calls:
        for bad in (None, 'typed', torch.ones(6, 10, dtype=torch.bool)):
            with pytest.raises(TypeError, match='expected a ranking.TypeConstraint'):
                call(type_constraint=bad)
        for kw in ({}, {'type_constraint': ranking.UNCONSTRAINED}):          # the plain call: on to the device check
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                call(**kw)
    assert repr(ranking.UNCONSTRAINED) == 'UNCONSTRAINED' and transe.UNCONSTRAINED is ranking.UNCONSTRAINED


def test_profile_typed_needs_profile_topk_on_both_clis():
    from gcn_vae_amd import train, transe
    p = train.build_parser()
    assert p.parse_args(['-d', 'x']).profile_typed is False
    with pytest.raises(ValueError, match='--profile-typed restricts the profiles: it needs --profile-topk'):
        train.check_args(p.parse_args(['-d', 'x', '--test-mode', 'True', '--profile-typed']))
    train.check_args(p.parse_args(['-d', 'x', '--test-mode', 'True', '--profile-typed', '--profile-topk', '10']))
    t = transe.build_parser()
    assert t.parse_args(['-d', 'x']).profile_typed is False
    with pytest.raises(ValueError, match='--profile-typed restricts the profiles: it needs --profile-topk'):
        transe.check_args(t.parse_args(['-d', 'x', '--profile-typed']))
    transe.check_args(t.parse_args(['-d', 'x', '--profile-typed', '--profile-topk', '10']))
    # --type-constrain keeps its meaning: it does not switch the typed profiles on
    assert t.parse_args(['-d', 'x', '--type-constrain', '--filtered-eval', '--profile-topk', '3']).profile_typed is False
