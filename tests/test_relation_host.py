"""Relation prediction, the host side (no GPU): ranking.PairFilterIndex against a brute-force dictionary, the rules the unfused
twins apply on hand-made matrices, the argument refusals of gv_pair_rel_scores / gv_transe_pair_rel and of their ops wrappers --
every text pinned, and with two faults at once the order in which they are reported --, the CLI flags and the TSV writers on a
fake route."""
import ctypes
import math

import numpy as np
import pytest
import torch

P = 'P'          # a non-NULL dummy pointer: nothing is launched, nothing reads it
M, N, R, H, K = 4, 10, 3, 8, 5
NULL, SHAPE = -1, -2

DM = [('e', P), ('ld_e', H), ('n', N), ('w', P), ('ld_w', H), ('num_rels', R), ('s', P), ('o', P), ('target', P), ('bias', None),
      ('filt_lo', P), ('filt_hi', P), ('filt_rel', P), ('n_filt_rel', 1), ('k', K), ('tgt', P), ('count_raw', P), ('count_filt', P),
      ('out_ids', P), ('out_logits', P), ('m', M), ('h', H), ('stream', None)]
TE = [('en', P), ('rn', P), ('n', N), ('num_rels', R), ('dim', H), ('p_norm', 2), ('s', P), ('o', P), ('target', P), ('filt_lo', P),
      ('filt_hi', P), ('filt_rel', P), ('n_filt_rel', 1), ('k', K), ('tgt', P), ('count_raw', P), ('count_filt', P), ('out_ids', P),
      ('out_dist', P), ('m', M), ('stream', None)]
ENTRIES = {'gv_pair_rel_scores': DM, 'gv_transe_pair_rel': TE}
NO_FILTER = {'filt_lo': None, 'filt_hi': None, 'filt_rel': None, 'count_filt': None}

# (faults, return code, the text after "<entry>: "); rows that name a parameter one entry lacks are skipped for it
REFUSALS = [
    ({'m': -1}, SHAPE, {'gv_pair_rel_scores': 'm=-1 n=10 num_rels=3 h=8 n_filt_rel=1',
                        'gv_transe_pair_rel': 'm=-1 n=10 num_rels=3 dim=8 (1..512) p_norm=2 (1 or 2) n_filt_rel=1'}),
    ({'num_rels': 0}, SHAPE, {'gv_pair_rel_scores': 'm=4 n=10 num_rels=0 h=8 n_filt_rel=1',
                              'gv_transe_pair_rel': 'm=4 n=10 num_rels=0 dim=8 (1..512) p_norm=2 (1 or 2) n_filt_rel=1'}),
    ({'dim': 513}, SHAPE, 'm=4 n=10 num_rels=3 dim=513 (1..512) p_norm=2 (1 or 2) n_filt_rel=1'),
    ({'p_norm': 3}, SHAPE, 'm=4 n=10 num_rels=3 dim=8 (1..512) p_norm=3 (1 or 2) n_filt_rel=1'),
    ({'k': 129}, SHAPE, 'k=129 outside [0, 128]'),
    ({'k': -1}, SHAPE, 'k=-1 outside [0, 128]'),
    ({'k': 0, 'target': None}, SHAPE, 'neither ranks (target) nor a top-k (k >= 1) asked for'),
    ({'ld_e': H - 1}, SHAPE, 'leading dimension too small'),
    ({'ld_w': H - 1}, SHAPE, 'leading dimension too small'),
    ({'filt_lo': None}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'filt_hi': None}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'filt_rel': None, 'filt_hi': None}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'e': None}, NULL, 'NULL pointer'), ({'en': None}, NULL, 'NULL pointer'), ({'rn': None}, NULL, 'NULL pointer'),
    ({'w': None}, NULL, 'NULL pointer'), ({'s': None}, NULL, 'NULL pointer'), ({'o': None}, NULL, 'NULL pointer'),
    ({'tgt': None}, NULL, 'NULL pointer'), ({'out_ids': None}, NULL, 'NULL pointer'),
    ({'out_logits': None}, NULL, 'NULL pointer'), ({'out_dist': None}, NULL, 'NULL pointer'),
    ({'count_filt': None}, NULL, 'a filter needs count_filt'),
    ({**NO_FILTER, 'count_filt': P}, NULL, 'count_filt needs a filter'),
    # two faults at once: the sizes, then k and what is asked for, then the leading dimensions, then the filter's arrays -- all ahead
    # of m == 0 --, then the pointers, then what comes with a filter
    ({'m': -1, 'k': 129}, SHAPE, {'gv_pair_rel_scores': 'm=-1 n=10 num_rels=3 h=8 n_filt_rel=1',
                                  'gv_transe_pair_rel': 'm=-1 n=10 num_rels=3 dim=8 (1..512) p_norm=2 (1 or 2) n_filt_rel=1'}),
    ({'k': 129, 'ld_e': H - 1}, SHAPE, 'k=129 outside [0, 128]'),
    ({'k': 129, 'filt_hi': None}, SHAPE, 'k=129 outside [0, 128]'),
    ({'k': 0, 'target': None, 'filt_lo': None}, SHAPE, 'neither ranks (target) nor a top-k (k >= 1) asked for'),
    ({'ld_w': H - 1, 'filt_hi': None}, SHAPE, 'leading dimension too small'),
    ({'m': 0, 'k': 129}, SHAPE, 'k=129 outside [0, 128]'),
    ({'m': 0, 'filt_hi': None}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'filt_hi': None, 's': None}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'s': None, 'count_filt': None}, NULL, 'NULL pointer'),
    ({'tgt': None, 'count_filt': None}, NULL, 'NULL pointer'),
]
# accepted without a launch: no pairs
EMPTY = [{'m': 0}, {'m': 0, 's': None, 'o': None, 'tgt': None, 'out_ids': None}, {'m': 0, **NO_FILTER}]


def _call(name, faults):
    from gcn_vae_amd import lib
    buf = (ctypes.c_int32 * 64)()
    args = {**dict(ENTRIES[name]), **faults}
    rc = getattr(lib.load(), name)(*[ctypes.addressof(buf) if args[p] == P else args[p] for p, _ in ENTRIES[name]])
    return rc, (lib.last_error() if rc else '')


@pytest.mark.parametrize('name', list(ENTRIES))
def test_entry_refusals_are_reported_through_the_return_code(name):
    params, seen = {p for p, _ in ENTRIES[name]}, 0
    for faults, code, text in REFUSALS:
        if not set(faults) <= params:
            continue
        text = text[name] if isinstance(text, dict) else text
        assert _call(name, faults) == (code, f'{name}: {text}'), faults
        seen += 1
    assert seen >= 25
    for faults in EMPTY:
        assert _call(name, {f: v for f, v in faults.items() if f in params}) == (0, ''), faults


def test_abi_table_lists_both_entries():
    from gcn_vae_amd import lib
    for name, params in ENTRIES.items():
        assert len(lib.SIGNATURES[name][1]) == len(params)


# ---- the ops wrappers on CPU tensors: every refusal comes before the look at the device, where the valid call ends ---------------
def _good(te):
    z = torch.zeros
    base = dict(s=torch.tensor([0, 1, 2, 9]), o=torch.tensor([9, 1, 0, 3]), target=torch.tensor([0, 1, 2, 0]), k=K,
                filt_lo=z(M, dtype=torch.long), filt_hi=torch.ones(M, dtype=torch.long), filt_rel=torch.tensor([2]))
    return {**(dict(en=z(N, H), rn=z(R, H), p_norm=2) if te else dict(emb=z(N, H), w=z(R, H))), **base}


WRAPPER_REFUSALS = [
    ({}, RuntimeError, 'there is no CPU fallback'),
    ({'TABLE': torch.zeros(H)}, TypeError, 'TABLE: expected a 2-D tensor'),
    ({'RELS': None}, TypeError, 'RELS: expected a 2-D tensor'),
    ({'s': torch.zeros(M)}, TypeError, 's: expected a 1-D integer tensor of entity ids'),
    ({'o': torch.zeros(M, 1, dtype=torch.long)}, TypeError, 'o: expected a 1-D integer tensor of entity ids'),
    ({'RELS': torch.zeros(R, H - 1)}, ValueError, 'TABLE / RELS width mismatch'),
    ({'RELS': torch.zeros(0, H)}, ValueError, 'need at least one entity, one relation and width >= 1 (n=10, num_rels=0, h=8)'),
    ({'o': torch.tensor([1, 2])}, ValueError, 'one object per subject: s and o are the two columns of the pairs'),
    ({'k': 129}, ValueError, 'k must lie in [0, 128] (0: no top-k), got 129'),
    ({'k': -1}, ValueError, 'k must lie in [0, 128] (0: no top-k), got -1'),
    ({'k': 0, 'target': None}, ValueError, 'nothing asked for: give target (ranks), k >= 1 (top-k) or both'),
    ({'s': torch.tensor([0, 1, 2, N])}, ValueError, 'pair entities must lie in [0, 10)'),
    ({'o': torch.tensor([0, -1, 2, 3])}, ValueError, 'pair entities must lie in [0, 10)'),
    ({'p_norm': 3}, ValueError, 'p_norm must be 1 or 2, got 3'),
    ({'target': torch.arange(M - 1)}, ValueError, 'one target per query row'),
    ({'target': torch.tensor([0, 1, 2, R])}, ValueError, 'targets must lie in [0, 3)'),
    ({'filt_lo': None}, ValueError, 'filt_lo, filt_hi and filt_rel are given together or not at all'),
    ({'filt_lo': torch.zeros(M - 1, dtype=torch.long)}, ValueError, 'one filter range (filt_lo, filt_hi) per query row'),
    ({'filt_hi': torch.full((M,), 2)}, ValueError, 'filter ranges must satisfy 0 <= filt_lo <= filt_hi <= 1'),
    ({'filt_rel': torch.tensor([R])}, ValueError, 'filtered relation ids must lie in [0, 3)'),
    # two at once: shapes, the pairs, k, the pairs' range, the norm, the targets, the filter
    ({'RELS': torch.zeros(R, H - 1), 'k': 129}, ValueError, 'TABLE / RELS width mismatch'),
    ({'k': 129, 's': torch.tensor([0, 1, 2, N])}, ValueError, 'k must lie in [0, 128] (0: no top-k), got 129'),
    ({'s': torch.tensor([0, 1, 2, N]), 'target': torch.tensor([0, 1, 2, R])}, ValueError, 'pair entities must lie in [0, 10)'),
    ({'target': torch.tensor([0, 1, 2, R]), 'filt_rel': torch.tensor([R])}, ValueError, 'targets must lie in [0, 3)'),
]


@pytest.mark.parametrize('te', [False, True])
def test_ops_wrapper_refusals(te):
    from gcn_vae_amd import ops
    fn = ops.transe_pair_relations if te else ops.pair_relation_scores
    table, rels = ('en', 'rn') if te else ('emb', 'w')
    for faults, exc, text in WRAPPER_REFUSALS:
        if 'p_norm' in faults and not te:
            continue
        kwargs = _good(te)
        kwargs.update({{'TABLE': table, 'RELS': rels}.get(n, n): v for n, v in faults.items()})
        text = text.replace('TABLE', table).replace('RELS', rels)
        with pytest.raises(exc) as err:
            fn(**kwargs)
        assert str(err.value) == text or (not faults and str(err.value).endswith(text)), (faults, str(err.value))
    if te:
        with pytest.raises(ValueError, match='en / rn: width 513 above 512'):
            fn(**{**_good(True), 'en': torch.zeros(N, 513), 'rn': torch.zeros(R, 513)})


def test_ids_checked_skips_the_value_reads_and_the_drivers_check_once():
    from gcn_vae_amd import ops, ranking
    ops.pair_ids_check(torch.tensor([0, N - 1]), torch.tensor([N - 1, 0]), torch.tensor([0, R - 1]), N, R)
    ops.pair_ids_check(torch.tensor([], dtype=torch.long), torch.tensor([], dtype=torch.long), None, N, R)
    for s, o, t, text in ((torch.tensor([0, N]), torch.tensor([1, 2]), None, 'pair entities must lie in [0, 10)'),
                          (torch.tensor([0, 1]), torch.tensor([-1, 2]), torch.tensor([0, 1]), 'pair entities must lie in [0, 10)'),
                          (torch.tensor([0, 1]), torch.tensor([1, 2]), torch.tensor([0, R]), 'targets must lie in [0, 3)'),
                          (torch.tensor([0, N]), torch.tensor([1, 2]), torch.tensor([0, R]), 'pair entities must lie in [0, 10)')):
        with pytest.raises(ValueError) as err:
            ops.pair_ids_check(s, o, t, N, R)
        assert str(err.value) == text
    # a caller that vouches for the ids gets the shape checks only: values out of range pass on to the look at the device
    for te in (False, True):
        fn = ops.transe_pair_relations if te else ops.pair_relation_scores
        wild = {**_good(te), 's': torch.tensor([0, 1, 2, N]), 'target': torch.tensor([0, 1, 2, R]), 'filt_rel': torch.tensor([R])}
        with pytest.raises(RuntimeError, match='there is no CPU fallback'):
            fn(**wild, ids_checked=True)
        with pytest.raises(ValueError, match='one target per query row'):
            fn(**{**wild, 'target': torch.arange(M - 1)}, ids_checked=True)
        with pytest.raises(ValueError, match='one filter range'):
            fn(**{**wild, 'filt_hi': torch.ones(M - 1, dtype=torch.long)}, ids_checked=True)
        with pytest.raises(ValueError, match='given together or not at all'):
            fn(**{**wild, 'filt_rel': None}, ids_checked=True)
    pf = ranking.PairFilterIndex(N, R, np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match='pair_filter was built for 10 entities / 3 relations, the tables hold 10 / 4'):
        ranking.rank_relations(torch.zeros(N, H), torch.zeros(R + 1, H), torch.tensor([[0, 1, 2]]), pf)
    with pytest.raises(ValueError, match='targets must lie in'):
        ranking.rank_relations(torch.zeros(N, H), torch.zeros(R, H), torch.tensor([[0, R, 2]]), pf)
    with pytest.raises(RuntimeError, match='there is no CPU fallback'):
        ranking.rank_relations(torch.zeros(N, H), torch.zeros(R, H), torch.tensor([[0, 1, 2]]), pf)


# ---- PairFilterIndex -----------------------------------------------------------------------------------------------------------------
def _brute(sets):
    known = {}
    for s, r, o in np.concatenate(sets).tolist():
        known.setdefault((s, o), set()).add(r)
    return {k: sorted(v) for k, v in known.items()}


def test_pair_filter_index_matches_a_dictionary():
    from gcn_vae_amd.ranking import PairFilterIndex
    rng = np.random.default_rng(0)
    n, num_rels = 40, 7
    train = np.stack([rng.integers(0, n, 600), rng.integers(0, num_rels, 600), rng.integers(0, n, 600)], 1)
    train[:50, 2] = train[:50, 0]                                    # s == o
    valid = np.concatenate([train[:30], train[:30], [[3, 2, 3], [3, 2, 3], [3, 0, 3]]])     # duplicates, within and across sets
    index = PairFilterIndex(n, num_rels, train, valid)
    known = _brute([train, valid])
    assert index.keys.dtype == torch.int64 and index.rel.dtype == torch.int32
    assert index.rel.numel() == sum(len(v) for v in known.values())
    pairs = sorted(known) + [(a, b) for a in range(n) for b in range(0, n, 7) if (a, b) not in known][:60]
    s, o = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    lo, hi = index.lookup(s, o)
    rel = index.relations()
    for i, pair in enumerate(pairs):
        assert rel[lo[i]:hi[i]].tolist() == known.get(pair, []), pair
    assert any(lo[i] == hi[i] for i in range(len(pairs))) and (3, 3) in known and known[(3, 3)][:2] == [0, 2]
    for bad in ([[0, 0, n]], [[-1, 0, 0]], [[0, num_rels, 0]], [[0, -1, 0]]):
        with pytest.raises(ValueError, match='out of range'):
            PairFilterIndex(n, num_rels, np.array(bad))
    empty = PairFilterIndex(n, num_rels)
    lo, hi = empty.lookup(s, o)
    assert empty.rel.numel() == 0 and bool((lo == hi).all())


def test_pair_filter_index_keys_are_int64():
    from gcn_vae_amd.ranking import PairFilterIndex
    n = 70000                                                        # s * n + o passes 2**31 (and 2**32)
    trip = np.array([[69999, 4, 69998], [69999, 1, 69998], [69999, 4, 69998], [0, 2, 69999], [46341, 0, 46341], [65536, 3, 0]])
    index = PairFilterIndex(n, 5, trip)
    assert int(index.keys.max()) == 69999 * n + 69998 > 2 ** 32
    s, o = torch.tensor([69999, 0, 46341, 65536, 69998, 8643]), torch.tensor([69998, 69999, 46341, 0, 69999, 22702])
    lo, hi = index.lookup(s, o)
    # (the last pair's key equals 69999 * n + 69998 modulo 2**32: a 32-bit key would find the first pair's relations there)
    assert (8643 * n + 22702) % 2 ** 32 == (69999 * n + 69998) % 2 ** 32
    assert [index.rel[a:b].tolist() for a, b in zip(lo.tolist(), hi.tolist())] == [[1, 4], [2], [0], [3], [], []]


# ---- the rules of the unfused twins on hand-made matrices --------------------------------------------------------------------------
def test_rank_rule_ties_listed_target_and_nan():
    from gcn_vae_amd.ranking import relation_ranks_from_scores
    nan, inf = float('nan'), float('inf')
    score = torch.tensor([[3., 1., 3., 3., 0.],        # target 0 ties with two: 0 better + 2 / 2
                          [3., 1., 3., 3., 0.],        # target 1: three better
                          [1., nan, 0., 2., 1.],       # a NaN candidate counts as better
                          [nan, 5., 1., 0., 2.],       # a NaN target ranks last
                          [1., inf, 1., -inf, 1.],     # +inf beats, ties half
                          [2., 2., 2., 2., 2.]])
    target = torch.tensor([0, 1, 0, 0, 2, 4])
    raw, none = relation_ranks_from_scores(score, target)
    assert none is None and raw.tolist() == [1.0, 3.0, 2.5, 4.0, 2.0, 2.0]
    # the filter: row 0 lists one of the ties and the TARGET itself (allowed), row 2 the NaN, row 5 everything
    lo, hi = torch.tensor([0, 2, 2, 3, 3, 3]), torch.tensor([2, 2, 3, 3, 3, 8])
    rel = torch.tensor([0, 2, 1, 0, 1, 2, 3, 4])
    raw2, filt = relation_ranks_from_scores(score, target, lo, hi, rel)
    assert torch.equal(raw, raw2) and filt.tolist() == [0.5, 3.0, 1.5, 4.0, 2.0, 0.0]


def test_topk_rule_on_relations():
    from gcn_vae_amd.ranking import topk_from_scores
    from gcn_vae_amd.transe import topk_from_distances
    nan = float('nan')
    score = torch.tensor([[1., 2., 2., nan, -0.], [0., 0., 0., 0., 0.]])
    ids, val = topk_from_scores(score, 7, torch.tensor([0, 1]), torch.tensor([1, 4]), torch.tensor([1, 0, 2, 4]))
    assert ids.tolist() == [[2, 0, 4, 3, -1, -1, -1], [1, 3, -1, -1, -1, -1, -1]]
    assert val[0, :3].tolist() == [2., 1., 0.] and math.isnan(val[0, 3]) and val[0, 4] == -math.inf
    assert math.copysign(1.0, float(val[0, 2])) == 1.0                                 # -0 reported as +0
    ids, dist = topk_from_distances(score, 7, torch.tensor([0, 1]), torch.tensor([1, 4]), torch.tensor([1, 0, 2, 4]))
    assert ids.tolist() == [[4, 0, 2, 3, -1, -1, -1], [1, 3, -1, -1, -1, -1, -1]] and dist[0, 4] == math.inf


# ---- the CLI flags and the writers ----------------------------------------------------------------------------------------------------
def test_cli_flags_and_defaults():
    from gcn_vae_amd import train, transe
    for mod, default in ((train, 'relation_predictions.tsv'), (transe, 'transe_relation_predictions.tsv')):
        a = mod.build_parser().parse_args(['-d', 'x'])
        assert (a.relation_eval, a.predict_relations, a.relations_out) == (False, 0, default)
        a = mod.build_parser().parse_args(['-d', 'x', '--relation-eval', '--predict-relations', '7', '--relations-out', 'r.tsv'])
        assert (a.relation_eval, a.predict_relations, a.relations_out) == (True, 7, 'r.tsv')
        for bad in ('129', '-1'):
            a = mod.build_parser().parse_args(['-d', 'x', '--test-mode'] + (['True'] if mod is train else []) + ['--predict-relations', bad])
            with pytest.raises(ValueError, match='--predict-relations must lie in'):
                mod.check_args(a)
    with pytest.raises(ValueError, match='--relation-eval decode a trained checkpoint'):
        train.check_args(train.build_parser().parse_args(['-d', 'x', '--relation-eval']))
    with pytest.raises(ValueError, match='--neg-rel: relation corruption is not supported'):          # queries exist, negatives do not
        transe.check_args(transe.build_parser().parse_args(['-d', 'x', '--neg-rel', '1']))


def _fake_route(k, sign):
    def route(s, o):
        ids = (s.view(-1, 1) + torch.arange(k)) % 3
        val = sign * (o.view(-1, 1).float() + torch.arange(k) / 3)
        ids[:, k - 1], val[:, k - 1] = -1, -sign * float('inf')                              # a padding slot per row
        return ids, val
    return route


def test_relation_writers_columns_padding_and_format(tmp_path, monkeypatch):
    from gcn_vae_amd import ranking, train, transe
    trip = torch.tensor([[5, 1, 7], [0, 0, 0], [5, 2, 7], [9, 1, 2]])
    k = 3
    seen = []
    monkeypatch.setattr(ranking, 'predict_relations', lambda emb, w, s, o, kk, pf, flp=None: seen.append((kk, pf, flp)) or
                        _fake_route(kk, 1.0)(s, o))
    monkeypatch.setattr(transe, 'predict_relations', lambda model, s, o, kk, pf: seen.append((kk, pf)) or _fake_route(kk, -1.0)(s, o))
    a, b = str(tmp_path / 'a.tsv'), str(tmp_path / 'b.tsv')
    assert train.write_relation_predictions(a, None, None, trip, k, 'PF', 'FLP') == 12
    assert transe.write_relation_predictions(b, None, trip.numpy(), k, 'PF') == 12
    assert seen == [(3, 'PF', 'FLP'), (3, 'PF')]
    rows_a = [line.rstrip('\n').split('\t') for line in open(a)]
    rows_b = [line.rstrip('\n').split('\t') for line in open(b)]
    assert all(len(r) == 5 for r in rows_a + rows_b)
    assert [r[:4] for r in rows_a] == [r[:4] for r in rows_b]                                 # the files join on four columns
    assert [r[:3] for r in rows_a] == [[str(s), str(o), str(p)] for s, _, o in trip.tolist() for p in range(k)]
    assert rows_a[0] == ['5', '7', '0', '2', '7'] and rows_a[1] == ['5', '7', '1', '0', f'{np.float32(7 + 1 / 3):.9g}']
    assert rows_a[1][4] == '7.33333349' and rows_b[1][4] == '-7.33333349'
    assert rows_a[2] == ['5', '7', '2', '-1', '-inf'] and rows_b[2] == ['5', '7', '2', '-1', 'inf']
    # the chunked loop gives the same file
    c = str(tmp_path / 'c.tsv')
    assert train.write_relation_lines(c, trip, _fake_route(k, 1.0), rows=3) == 12
    assert open(c).read() == open(a).read()
    assert train.write_relation_lines(c, trip[:0], _fake_route(k, 1.0)) == 0 and open(c).read() == ''
