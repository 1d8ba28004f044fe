"""The refusals of the six per-entity ``ops`` wrappers and of the routes above them (``ranking.complete_entities{,_unfused,_mc,
_mc_unfused}``, ``transe.complete_entities{,_unfused}``), host side (no GPU): exception type and WHOLE message of every check a CPU
tensor reaches, one fault at a time, and for each adjacent pair of checks both faults at once -- the earlier check is the one that
reports.  The table was recorded from the wrappers as six separate functions, before they became one core per model; it holds for
both.  The last refusal a CPU tensor reaches is the "no CPU fallback" one of the first table; the checks behind it (the second
table's device, the member lists and their plan, the bias) need a GPU tensor and belong to the GPU modules -- here they are only
shown not to run ahead of it."""
import pytest
import torch

N, R, H = 10, 3, 8
PTR = torch.tensor([0, 1, 2, 3, 4, 5, 6])                       # 2 R + 1 entries: six sets of one member each
IDS = torch.tensor([2, 5, 1, 1, 4, 4], dtype=torch.int32)
LO, HI, ENT = torch.zeros(N * R, dtype=torch.long), torch.ones(N * R, dtype=torch.long), torch.tensor([3])
TRIPLETS = [[1, 0, 2], [4, 1, 5], [4, 2, 1]]

SIDE = "side is 's' (the entity as subject: new facts (a, r, x)) or 'o' (as object: new facts (x, r, a))"
K0 = 'k must lie in [1, 128], got 0'
NO_CPU = '{}: the gfx950 path needs a CUDA/ROCm tensor; there is no CPU fallback'
NO_CPU_GOT = '{}: the gfx950 path needs a CUDA/ROCm tensor (got Tensor on cpu); there is no CPU fallback'

# fault -> (what the call is given instead, exception, message); '{tile}' is the wrapper's word for a tile
WRAPPER_FAULTS = {
    'stack': (dict(table=torch.zeros(N, H)), TypeError, 'z: expected a 3-D (samples, entities, width) tensor with at least one sample'),
    'emb_dim': (dict(table=torch.zeros(N)), TypeError, 'emb: expected a 2-D tensor'),
    'w_dim': (dict(w=torch.zeros(R)), TypeError, 'w: expected a 2-D tensor'),
    'ents': (dict(ents=torch.tensor([1.0])), TypeError, 'ents: expected a 1-D integer tensor of entity ids'),
    'width': (dict(w=torch.zeros(R, H - 1)), ValueError, 'emb / w width mismatch'),
    'sizes': (dict(w=torch.zeros(0, H)), ValueError, 'need at least one entity, one relation and width >= 1 (n=10, num_rels=0, h=8)'),
    'bits31': (dict(table=torch.zeros(1 << 16, 1), w=torch.zeros(1 << 15, 1)), ValueError,
               'n * num_rels = 2147483648 does not fit 31 bits: a candidate (r, x) is the id r * n + x'),
    'k': (dict(k=0), ValueError, K0),
    'k_high': (dict(k=129), ValueError, 'k must lie in [1, 128], got 129'),
    'p_norm': (dict(p_norm=3), ValueError, 'p_norm must be 1 or 2, got 3'),
    'wide': (dict(table=torch.zeros(N, 513), w=torch.zeros(R, 513)), ValueError, 'en / rn: width 513 above 512'),
    'span': (dict(span=0), ValueError, 'span counts (relation, {tile} tile) pairs per workgroup: at least 1, got 0'),
    'range': (dict(ents=torch.tensor([4, N])), ValueError, 'query entities must lie in [0, 10)'),
    'range_low': (dict(ents=torch.tensor([-1, 4])), ValueError, 'query entities must lie in [0, 10)'),
    'filter': (dict(filt=(LO, None, None)), ValueError, 'filt_lo, filt_hi and filt_ent are given together or not at all'),
    'filter_rows': (dict(filt=(LO[:N], HI[:N], ENT)), ValueError, 'one filter range (filt_lo, filt_hi) per query row'),
    'filter_order': (dict(filt=(HI, LO, ENT)), ValueError, 'filter ranges must satisfy 0 <= filt_lo <= filt_hi <= 1'),
    'filter_ids': (dict(filt=(LO, HI, ENT + 7)), ValueError, 'filtered entity ids must lie in [0, 10)'),
    # behind the device check: given WITH it, they must not be the ones reported
    'members': (dict(members=(PTR[:-1], IDS)), None, None),
    'side': (dict(side='x'), None, None),
    'bias': (dict(bias=torch.zeros(5)), None, None),
    'empty': (dict(ents=torch.zeros(0, dtype=torch.long)), None, None),      # no fault: ``m == 0`` returns behind the device checks
}

# wrapper -> (its word for a tile, the order of its checks as far as a CPU tensor gets, its last refusal, the faults behind that)
DISTMULT_ORDER = ('width', 'k', 'span', 'range', 'filter')
TRANSE_ORDER = ('width', 'k', 'p_norm', 'wide', 'span', 'range', 'filter')
WRAPPERS = {
    'entity_topk_scores': ('column', DISTMULT_ORDER, NO_CPU.format('emb'), ('bias',)),
    'entity_topk_scores_typed': ('member', DISTMULT_ORDER, NO_CPU.format('emb'), ('members', 'side', 'bias')),
    'entity_topk_scores_mc': ('column', ('stack',) + DISTMULT_ORDER, NO_CPU.format('z'), ('bias',)),
    'entity_topk_scores_typed_mc': ('member', ('stack',) + DISTMULT_ORDER, NO_CPU.format('z'), ('members', 'side', 'bias')),
    'transe_entity_topk': ('entity', TRANSE_ORDER, NO_CPU_GOT.format('en'), ()),
    'transe_entity_topk_typed': ('member', TRANSE_ORDER, NO_CPU_GOT.format('en'), ('members',)),
}
OPERAND_FAULTS = ('emb_dim', 'w_dim', 'ents', 'sizes', 'bits31', 'k_high', 'range_low', 'filter_rows', 'filter_order', 'filter_ids')


def _call_wrapper(name, faults):
    from gcn_vae_amd import ops
    mc, typed, transe = name.endswith('_mc'), 'typed' in name, name.startswith('transe')
    a = dict(ents=torch.tensor([4, 1, 4]), table=torch.zeros(N, H), w=torch.zeros(R, H), k=5, p_norm=1, span=None, filt=(None, None, None),
             bias=None, members=(PTR, IDS), side='s')
    for f in faults:
        a.update(WRAPPER_FAULTS[f][0])
    if mc and 'stack' not in faults:
        a['table'] = a['table'].unsqueeze(0).repeat(2, 1, 1)
    if transe:
        return getattr(ops, name)(a['ents'], a['table'], a['w'], a['k'], a['p_norm'], *(a['members'] if typed else ()), False, *a['filt'],
                                  True, a['span'])
    return getattr(ops, name)(a['ents'], a['table'], a['w'], a['k'], *((*a['members'], a['side']) if typed else ()), a['bias'], *a['filt'],
                              True, a['span'])


def _wrapper_cases():
    cases = []
    for name, (tile, order, last, behind) in WRAPPERS.items():
        singles = order + tuple(f for f in OPERAND_FAULTS if not (f == 'emb_dim' and name.endswith('_mc')))
        for f in singles:
            cases.append((name, (f,), WRAPPER_FAULTS[f][1], WRAPPER_FAULTS[f][2].format(tile=tile)))
        for first, second in zip(order, order[1:]):                  # both faults: the earlier check reports
            cases.append((name, (first, second), WRAPPER_FAULTS[first][1], WRAPPER_FAULTS[first][2].format(tile=tile)))
        cases.append((name, (), RuntimeError, last))                    # valid arguments on the CPU: the first table's device
        cases.append((name, ('empty',), RuntimeError, last))
        if behind:
            cases.append((name, behind, RuntimeError, last))
    return cases


@pytest.mark.parametrize('name, faults, exc, message', _wrapper_cases(), ids=lambda v: '+'.join(v) if isinstance(v, tuple) else None)
def test_wrapper_refusal(name, faults, exc, message):
    with pytest.raises(Exception) as got:
        _call_wrapper(name, faults)
    assert type(got.value) is exc and str(got.value) == message


# ---- the routes above the wrappers -------------------------------------------------------------------------------------------------
ROUTE_FAULTS = {
    'constraint': (dict(type_constraint=None), TypeError,
                   'type_constraint: expected a ranking.TypeConstraint, got NoneType (leave the argument out for the unconstrained call)'),
    'side': (dict(side='x'), ValueError, SIDE),
    'k': (dict(k=0), ValueError, K0),
    'samples': (dict(table=torch.zeros(N, H)), ValueError, 'z: expected the (S, N, h) samples of KGVAE.posterior_samples, S >= 1'),
    'flps': (dict(flow_log_probs=torch.zeros(5)), ValueError, 'flow_log_probs: one value per sample (2), got 5'),
    'width': (dict(w=torch.zeros(R, H - 1)), ValueError, 'emb / w width mismatch'),
    'filter_index': (dict(filter_index=(N + 1, R)), ValueError, 'the FilterIndex is for 11 entities / 3 relations, the tables have 10 / 3'),
    'p_norm': (dict(p_norm=3), ValueError, 'p_norm must be 1 or 2, got 3'),
    'tc_sizes': (dict(type_constraint=(N + 1, R)), ValueError,
                 'the TypeConstraint is for 11 entities / 3 relations, the tables have 10 / 3'),
    'range': (dict(ents=[4, N]), ValueError, 'query entities must lie in [0, 10)'),
}
RANKING_ORDER = ('constraint', 'side', 'k', 'width', 'filter_index', 'tc_sizes')
MC_ORDER = ('constraint', 'side', 'k', 'samples', 'width', 'filter_index', 'tc_sizes')
TRANSE_ROUTE_ORDER = ('constraint', 'side', 'k', 'width', 'filter_index', 'p_norm', 'tc_sizes')
# route -> (order of its checks, further single faults, last refusal untyped, last refusal typed)
ROUTES = {
    'ranking.complete_entities': (RANKING_ORDER + ('range',), (), NO_CPU.format('emb'), NO_CPU.format('emb')),
    'ranking.complete_entities_unfused': (RANKING_ORDER, (), NO_CPU_GOT.format('a'), NO_CPU_GOT.format('a')),
    'ranking.complete_entities_mc': (MC_ORDER + ('range',), ('flps',), NO_CPU.format('z'), NO_CPU.format('z')),
    'ranking.complete_entities_mc_unfused': (MC_ORDER, ('flps',), NO_CPU_GOT.format('a'), NO_CPU_GOT.format('a')),
    'transe.complete_entities': (TRANSE_ROUTE_ORDER, (), NO_CPU_GOT.format('ent'), NO_CPU_GOT.format('ent')),
    'transe.complete_entities_unfused': (TRANSE_ROUTE_ORDER, (), NO_CPU_GOT.format('ent'), NO_CPU_GOT.format('ent')),
}


def _call_route(name, faults, typed=False):
    from gcn_vae_amd import ranking, transe
    module, fn = name.split('.')
    a = dict(table=torch.zeros(N, H), w=torch.zeros(R, H), ents=[4, 1, 4], k=5, p_norm=1, side='s')
    if typed:
        a['type_constraint'] = (N, R)
    for f in faults:
        a.update(ROUTE_FAULTS[f][0])
    if '_mc' in fn and 'samples' not in faults:
        a['table'] = a['table'].unsqueeze(0).repeat(2, 1, 1)
    kw = {key: a[key] for key in ('side', 'type_constraint', 'flow_log_probs') if key in a}
    if isinstance(kw.get('type_constraint'), tuple):
        kw['type_constraint'] = ranking.TypeConstraint(*kw['type_constraint'], TRIPLETS)
    if 'filter_index' in a:
        kw['filter_index'] = ranking.FilterIndex(*a['filter_index'], TRIPLETS)
    if module == 'transe':
        return getattr(transe, fn)((a['table'], a['w'], a['p_norm'], True), a['ents'], a['k'], **kw)
    return getattr(ranking, fn)(a['table'], a['w'], a['ents'], a['k'], **kw)


def _route_cases():
    cases = []
    for name, (order, more, last, last_typed) in ROUTES.items():
        for f in order + more:
            cases.append((name, (f,), ROUTE_FAULTS[f][1], ROUTE_FAULTS[f][2]))
        for first, second in zip(order, order[1:]):
            cases.append((name, (first, second), ROUTE_FAULTS[first][1], ROUTE_FAULTS[first][2]))
        cases.append((name, (), RuntimeError, last))
        cases.append((name, ('typed',), RuntimeError, last_typed))
    return cases


@pytest.mark.parametrize('name, faults, exc, message', _route_cases(), ids=lambda v: '+'.join(v) if isinstance(v, tuple) else None)
def test_route_refusal(name, faults, exc, message):
    typed = faults == ('typed',)
    with pytest.raises(Exception) as got:
        _call_route(name, () if typed else faults, typed)
    assert type(got.value) is exc and str(got.value) == message
