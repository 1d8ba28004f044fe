"""Relation prediction under type sets and on the posterior predictive, the host side (no GPU): TypeConstraint.relation_words
against a brute-force set construction, the twins' constrained rank and list rules on hand-made matrices, the refusals of the four
new C entries before any launch (code, text, and with two faults at once the order), the ops wrappers on CPU tensors, every
check_args refusal of the new flags and the writers' columns."""
import ctypes

import numpy as np
import pytest
import torch

P = 'P'          # a non-NULL dummy pointer: nothing is launched, nothing reads it
M, N, R, H, K, S = 4, 10, 3, 8, 5, 3
NULL, SHAPE = -1, -2

_PAIR = [('s', P), ('o', P), ('target', P)]
_FILT = [('filt_lo', P), ('filt_hi', P), ('filt_rel', P), ('n_filt_rel', 1)]
_CAND = [('cand', P), ('ld_cand', 1), ('n_sets', 2 * N)]
_COUNTS = [('count_raw', P), ('count_filt', P)]
_COUNTS_C = [('count_raw_c', P), ('count_filt_c', P)]
_DM_TABLES = [('n', N), ('w', P), ('ld_w', H), ('num_rels', R)]
_DM_OUT = [('out_ids', P), ('out_values', P), ('m', M), ('h', H), ('stream', None)]
ENTRIES = {
    'gv_pair_rel_scores_constrained': [('e', P), ('ld_e', H)] + _DM_TABLES + _PAIR + [('bias', None)] + _FILT + _CAND + [('k', K), ('tgt', P)]
    + _COUNTS + _COUNTS_C + _DM_OUT,
    'gv_pair_rel_scores_mc': [('e', P), ('ld_e', H), ('e_stride', N * H), ('n_samples', S)] + _DM_TABLES + _PAIR + [('bias', None)] + _FILT
    + [('k', K), ('tgt', P)] + _COUNTS + _DM_OUT,
    'gv_pair_rel_scores_mc_constrained': [('e', P), ('ld_e', H), ('e_stride', N * H), ('n_samples', S)] + _DM_TABLES + _PAIR + [('bias', None)]
    + _FILT + _CAND + [('k', K), ('tgt', P)] + _COUNTS + _COUNTS_C + _DM_OUT,
    'gv_transe_pair_rel_constrained': [('en', P), ('rn', P), ('n', N), ('num_rels', R), ('dim', H), ('p_norm', 2)] + _PAIR + _FILT + _CAND
    + [('k', K), ('tgt', P)] + _COUNTS + _COUNTS_C + [('out_ids', P), ('out_values', P), ('m', M), ('stream', None)],
}
NO_FILTER = {'filt_lo': None, 'filt_hi': None, 'filt_rel': None, 'count_filt': None, 'count_filt_c': None}
CAND_SHAPE = 'n_sets={} (>= 2 n = 20) ld_cand={} (>= 1)'

# (faults, return code, the text after "<entry>: "); rows that name a parameter an entry lacks are skipped for it
REFUSALS = [
    ({'cand': None}, NULL, 'NULL cand'),
    ({'ld_cand': 0}, SHAPE, CAND_SHAPE.format(20, 0)),
    ({'n_sets': 2 * N - 1}, SHAPE, CAND_SHAPE.format(19, 1)),
    ({'n_samples': 0}, SHAPE, 'n_samples=0'),
    ({'e_stride': (N - 1) * H + H - 1}, SHAPE, 'sample stride shorter than the table it spans (e_stride=79)'),
    ({'count_filt_c': None}, NULL, 'a filter needs count_filt_c'),
    ({'count_filt': None}, NULL, 'a filter needs count_filt'),
    ({**NO_FILTER, 'count_filt_c': P}, NULL, 'count_filt_c needs a filter and targets'),
    ({'k': 129}, SHAPE, 'k=129 outside [0, 128]'),
    ({'k': 0, 'target': None}, SHAPE, 'neither ranks (target) nor a top-k (k >= 1) asked for'),
    ({'ld_e': H - 1}, SHAPE, 'leading dimension too small'),
    ({'filt_hi': None}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'s': None}, NULL, 'NULL pointer'), ({'tgt': None}, NULL, 'NULL pointer'), ({'out_values': None}, NULL, 'NULL pointer'),
    # two at once, in the neighbours' order: the sizes, k and what is asked for, the sample geometry where the leading dimensions
    # stand (n_samples, the leading dimensions, the stride), the filter's arrays, the bitmask (geometry, then the array) -- all
    # ahead of m == 0 --, then the pointers, then what comes with a filter
    ({'m': -1, 'k': 129}, SHAPE, {'gv_pair_rel_scores_constrained': 'm=-1 n=10 num_rels=3 h=8 n_filt_rel=1',
                                  'gv_pair_rel_scores_mc': 'm=-1 n=10 num_rels=3 h=8 n_filt_rel=1',
                                  'gv_pair_rel_scores_mc_constrained': 'm=-1 n=10 num_rels=3 h=8 n_filt_rel=1',
                                  'gv_transe_pair_rel_constrained': 'm=-1 n=10 num_rels=3 dim=8 (1..512) p_norm=2 (1 or 2) n_filt_rel=1'}),
    ({'k': 129, 'n_samples': 0}, SHAPE, 'k=129 outside [0, 128]'),
    ({'k': 129, 'cand': None}, SHAPE, 'k=129 outside [0, 128]'),
    ({'n_samples': 0, 'ld_e': H - 1}, SHAPE, 'n_samples=0'),
    ({'ld_e': H - 1, 'e_stride': 1}, SHAPE, 'leading dimension too small'),
    ({'e_stride': 1, 'filt_hi': None}, SHAPE, 'sample stride shorter than the table it spans (e_stride=1)'),
    ({'filt_hi': None, 'ld_cand': 0}, NULL, 'filt_lo / filt_hi / filt_rel must be all given or all NULL'),
    ({'ld_cand': 0, 'cand': None}, SHAPE, CAND_SHAPE.format(20, 0)),
    ({'m': 0, 'cand': None}, NULL, 'NULL cand'),
    ({'m': 0, 'n_samples': 0}, SHAPE, 'n_samples=0'),
    ({'cand': None, 's': None}, NULL, 'NULL cand'),
    ({'s': None, 'count_filt_c': None}, NULL, 'NULL pointer'),
    ({'count_filt': None, 'count_filt_c': None}, NULL, 'a filter needs count_filt'),
]
# accepted without a launch: no pairs (one sample needs no stride)
EMPTY = [{'m': 0}, {'m': 0, 's': None, 'o': None, 'tgt': None, 'out_ids': None, 'count_raw_c': None}, {'m': 0, **NO_FILTER},
         {'m': 0, 'n_samples': 1, 'e_stride': 0}]


def _call(name, faults):
    from gcn_vae_amd import lib
    buf = (ctypes.c_int32 * 64)()
    args = {**dict(ENTRIES[name]), **faults}
    rc = getattr(lib.load(), name)(*[ctypes.addressof(buf) if args[p] == P else args[p] for p, _ in ENTRIES[name]])
    return rc, (lib.last_error() if rc else '')


@pytest.mark.parametrize('name', list(ENTRIES))
def test_entry_refusals_come_before_any_launch(name):
    params, seen = {p for p, _ in ENTRIES[name]}, 0
    for faults, code, text in REFUSALS:
        if not set(faults) <= params:
            continue
        text = text[name] if isinstance(text, dict) else text
        assert code < 0 and _call(name, faults) == (code, f'{name}: {text}'), faults
        seen += 1
    assert seen >= 15
    for faults in EMPTY:
        assert _call(name, {f: v for f, v in faults.items() if f in params}) == (0, ''), faults


def test_abi_table_and_header_list_the_entries():
    import os
    from gcn_vae_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header, guide = open(os.path.join(root, 'include', 'gcnvae.h')).read(), open(os.path.join(root, 'INTEGRATION.md')).read()
    for name, params in ENTRIES.items():
        assert len(lib.SIGNATURES[name][1]) == len(params)
        assert f'int {name}(' in header and name in guide


# ---- TypeConstraint.relation_words ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_rels', [1, 3, 32, 33, 65])
def test_relation_words_match_a_brute_force_construction(num_rels):
    from gcn_vae_amd import ranking
    n = 41
    rng = np.random.default_rng(num_rels)
    sets = [np.stack([rng.integers(0, n, c), rng.integers(0, num_rels, c), rng.integers(0, n, c)], 1) for c in (120, 30, 0, 7)]
    sets[1][:, 1] = num_rels - 1                                         # the last relation is seen: the top used bit is set
    sets[0] = np.concatenate([sets[0], sets[0][:10]])                    # duplicate triplets are one bit
    tc = ranking.TypeConstraint(n, num_rels, *sets)
    rw = tc.relation_words()
    n_words = (num_rels + 31) // 32
    assert rw.dtype == torch.int32 and tuple(rw.shape) == (2 * n, n_words) and rw.is_contiguous() and tc.relation_words() is rw
    subj, obj = [set() for _ in range(n)], [set() for _ in range(n)]
    for s, r, o in np.concatenate(sets).tolist():
        subj[s].add(r)
        obj[o].add(r)
    want = np.zeros((2 * n, n_words), dtype=np.uint32)
    for e in range(n):
        for row, rels in ((e, subj[e]), (n + e, obj[e])):
            for r in rels:
                want[row, r >> 5] |= np.uint32(1) << np.uint32(r & 31)
    assert np.array_equal(rw.numpy().view(np.uint32), want)              # (bits from num_rels on are zero: `want` never sets one)
    # the pair's set is the AND of two rows, and pair_mask -- read off `words`, the other construction -- agrees with it
    s, o = torch.from_numpy(rng.integers(0, n, 200)), torch.from_numpy(rng.integers(0, n, 200))
    both = (rw[s] & rw[n + o]).numpy().view(np.uint32)
    dense = tc.pair_mask(s, o).numpy()
    assert dense.shape == (200, num_rels)
    for i in range(200):
        members = subj[int(s[i])] & obj[int(o[i])]
        assert set(np.nonzero(dense[i])[0].tolist()) == members
        assert {r for r in range(n_words * 32) if (both[i, r >> 5] >> np.uint32(r & 31)) & 1} == members
    # the same sets as `words`, seen from the entity
    assert int(sum(bin(int(x)).count('1') for x in want.ravel())) == int(tc.sizes.sum())
    empty = ranking.TypeConstraint(n, num_rels)
    assert not bool(empty.relation_words().any()) and not bool(empty.pair_mask(s, o).any())


# ---- the twins' rules ---------------------------------------------------------------------------------------------------------------
def test_constrained_rank_and_list_rules_on_a_hand_made_matrix():
    from gcn_vae_amd import ranking
    nan, inf = float('nan'), float('inf')
    score = torch.tensor([[0.5, 0.9, 0.5, 0.1, 0.7],      # target 0: better 1, 4; tie 2
                          [0.5, 0.9, 0.5, 0.1, 0.7],      # the same row, nothing type-correct
                          [0.2, nan, 0.3, 0.2, -inf],     # target 3: a NaN candidate counts as better
                          [1.0, 1.0, 1.0, 1.0, 1.0]])     # saturated: one tie
    target = torch.tensor([0, 0, 3, 2])
    allowed = torch.tensor([[0, 1, 1, 1, 0], [0, 0, 0, 0, 0], [1, 1, 0, 1, 1], [1, 1, 1, 0, 1]], dtype=torch.bool)
    lo, hi, rel = torch.tensor([0, 1, 1, 2]), torch.tensor([1, 1, 2, 4]), torch.tensor([1, 1, 0, 2])
    raw, filt, raw_c, filt_c = ranking.relation_ranks_from_scores(score, target, lo, hi, rel, cand_mask=allowed)
    assert raw.tolist() == [2.5, 2.5, 2.5, 2.0] and filt.tolist() == [1.5, 2.5, 1.5, 1.5]
    assert raw_c.tolist() == [1.5, 0.0, 1.5, 1.5]          # the target is never counted, allowed (rows 0, 2) or not (row 3)
    assert filt_c.tolist() == [0.5, 0.0, 0.5, 1.0]
    two = ranking.relation_ranks_from_scores(score, target, cand_mask=allowed)
    assert two[1] is None and two[3] is None and torch.equal(two[2], raw_c)
    assert len(ranking.relation_ranks_from_scores(score, target, lo, hi, rel)) == 2
    ids, val = ranking.topk_from_scores(score, 3, lo, hi, rel, cand=allowed)
    assert ids.tolist() == [[2, 3, -1], [-1, -1, -1], [0, 3, 4], [1, 4, -1]]      # allowed less listed; NaN (listed here) never shows
    assert val[1].tolist() == [-inf] * 3 and val[0, 2] == -inf and val[2, 2] == -inf and ids[2, 2] == 4
    ids, _ = ranking.topk_from_scores(score, 5, cand=allowed)
    assert ids[2].tolist() == [0, 3, 4, 1, -1]             # -inf before NaN, NaN last, then padding


def test_pair_pbar_unfused_is_the_running_sum(monkeypatch):
    from gcn_vae_amd import ranking
    z, w = torch.randn(3, 6, 4), torch.randn(5, 4)
    s, o, flp = torch.tensor([0, 5, 2]), torch.tensor([1, 5, 0]), torch.tensor([0.1, -0.2, 0.3])
    monkeypatch.setattr(ranking, 'pair_scores_unfused', lambda e, w_, s_, o_, b=None: (e[s_] * e[o_]) @ w_.T + (0 if b is None else b))
    got = ranking.pair_pbar_unfused(z, w, s, o, flp)
    want = sum(torch.sigmoid((z[i][s] * z[i][o]) @ w.T + flp[i]) for i in range(3)) * (1.0 / 3)
    assert got.shape == (3, 5) and torch.allclose(got, want, atol=1e-7)


# ---- the ops wrappers on CPU tensors --------------------------------------------------------------------------------------------------
def test_ops_wrappers_have_no_cpu_fallback_and_check_shapes_first():
    from gcn_vae_amd import ops
    z = torch.zeros
    pairs = dict(s=torch.tensor([0, 1, 2, 9]), o=torch.tensor([9, 1, 0, 3]), target=torch.tensor([0, 1, 2, 0]), k=K)
    cand = z(2 * N, 1, dtype=torch.int32)
    for fn, tables in ((ops.pair_relation_scores, dict(emb=z(N, H), w=z(R, H))), (ops.pair_relation_scores_mc, dict(z=z(S, N, H), w=z(R, H))),
                       (ops.transe_pair_relations, dict(en=z(N, H), rn=z(R, H), p_norm=1))):
        for extra in ({}, {'cand': cand}):
            with pytest.raises(RuntimeError, match='there is no CPU fallback'):
                fn(**tables, **pairs, **extra)
        with pytest.raises(ValueError, match='nothing asked for'):
            fn(**tables, **{**pairs, 'target': None, 'k': 0}, cand=cand)
        with pytest.raises(ValueError, match='pair entities must lie in'):
            fn(**tables, **{**pairs, 's': torch.tensor([0, 1, 2, N])}, cand=cand)
    mc = dict(w=z(R, H), **pairs)
    for bad in (z(N, H), z(0, N, H), None):
        with pytest.raises(TypeError, match='z: expected a 3-D'):
            ops.pair_relation_scores_mc(bad, **mc)
    with pytest.raises(ValueError, match='z / w width mismatch'):
        ops.pair_relation_scores_mc(z(S, N, H + 1), **mc)
    with pytest.raises(ValueError, match=r'k must lie in \[0, 128\]'):
        ops.pair_relation_scores_mc(z(S, N, H), **{**mc, 'k': 129})
    with pytest.raises(ValueError, match='targets must lie in'):
        ops.pair_relation_scores_mc(z(S, N, H), **{**mc, 'target': torch.tensor([0, 1, 2, R])})


def test_drivers_refuse_foreign_constraints_before_the_device():
    from gcn_vae_amd import ranking
    tc = ranking.TypeConstraint(N, R + 1, np.array([[0, 1, 2]]))
    trip = torch.tensor([[0, 1, 2]])
    for call in (lambda: ranking.rank_relations(torch.zeros(N, H), torch.zeros(R, H), trip, type_constraint=tc),
                 lambda: ranking.rank_relations_mc(torch.zeros(S, N, H), torch.zeros(R, H), trip, type_constraint=tc),
                 lambda: ranking.predict_relations_mc(torch.zeros(S, N, H), torch.zeros(R, H), trip[:, 0], trip[:, 2], 2, type_constraint=tc)):
        with pytest.raises(ValueError, match='type_constraint was built for 10 entities / 4 relations, the tables hold 10 / 3'):
            call()
    with pytest.raises(ValueError, match='z: expected the'):
        ranking.rank_relations_mc(torch.zeros(N, H), torch.zeros(R, H), trip)
    with pytest.raises(ValueError, match='flow_log_probs: one value per sample'):
        ranking.rank_relations_mc(torch.zeros(S, N, H), torch.zeros(R, H), trip, flow_log_probs=torch.zeros(S + 1))
    ok = ranking.TypeConstraint(N, R, np.array([[0, 1, 2]]))
    with pytest.raises(RuntimeError, match='there is no CPU fallback'):
        ranking.rank_relations_mc(torch.zeros(S, N, H), torch.zeros(R, H), trip, type_constraint=ok)


# ---- the CLIs -----------------------------------------------------------------------------------------------------------------------------
def test_check_args_refuses_bad_combinations_before_anything_is_loaded():
    from gcn_vae_amd import train, transe
    base = ['-d', 'nowhere', '--gpu', '0', '--test-mode', 'True', '--model-state-file', 'none.pth']

    def refused(flags, text, parser=train, head=base):
        with pytest.raises(ValueError, match=text):
            parser.check_args(parser.build_parser().parse_args(head + flags))
    refused(['--relations-typed'], '--relations-typed restricts the relation queries: it needs --relation-eval or --predict-relations')
    refused(['--mc-relations', '--relation-eval'], '--mc-relations answers the relation queries on the posterior predictive: it needs '
                                                   '--mc-samples S > 0')
    refused(['--mc-relations', '--mc-samples', '4'], '--mc-relations writes the posterior-predictive form of the relation queries: it needs '
                                                     '--relation-eval or --predict-relations')
    refused(['--mc-relations', '--mc-samples', '4', '--relations-typed'], '--relations-typed restricts the relation queries')
    refused(['--mc-relations', '--mc-samples', '4', '--relation-eval', '--model-class', 'RGCN'], '--mc-samples needs --model-class KGVAE')
    refused(['--relations-typed', '--relation-eval'], 'decode a trained checkpoint', head=['-d', 'nowhere', '--gpu', '0'])
    for flags in (['--relations-typed', '--relation-eval'], ['--relations-typed', '--predict-relations', '3'],
                  ['--mc-relations', '--mc-samples', '2', '--predict-relations', '3', '--relations-typed'],
                  ['--mc-relations', '--mc-samples', '2', '--relation-eval', '--mc-type-constrain', '--filtered-eval']):
        train.check_args(train.build_parser().parse_args(base + flags))
    args = train.build_parser().parse_args(base)
    assert args.relations_typed is False and args.mc_relations is False and args.mc_relations_out == 'mc_relation_predictions.tsv'
    te = ['-d', 'nowhere', '--gpu', '0']
    refused(['--relations-typed'], '--relations-typed restricts the relation queries: it needs --relation-eval or --predict-relations',
            transe, te)
    refused(['--relations-typed', '--relation-eval', '--neg-rel', '1'], '--neg-rel: relation corruption is not supported', transe, te)
    transe.check_args(transe.build_parser().parse_args(te + ['--relations-typed', '--predict-relations', '3']))
    assert transe.build_parser().parse_args(te).relations_typed is False


def test_writers_columns(tmp_path, monkeypatch):
    from gcn_vae_amd import ranking, train
    trip = torch.tensor([[3, 0, 4], [5, 1, 6]])
    seen = {}

    def fake_mc(z, w, s, o, k, pair_filter, flps, type_constraint=None):
        tc = type_constraint
        seen['mc'] = (pair_filter, flps, tc)
        ids = torch.tensor([[2, 0, -1], [1, -1, -1]])[:s.numel()]
        return ids, torch.tensor([[0.75, 0.5, -float('inf')], [1.0, -float('inf'), -float('inf')]]), torch.tensor([[0.125, 0.0, 0.0], [0.25, 0.0, 0.0]])

    def fake(embed, w, s, o, k, pair_filter, flp, type_constraint=None):
        tc = type_constraint
        seen['one'] = (pair_filter, flp, tc)
        return torch.tensor([[2, 0, -1], [1, -1, -1]]), torch.tensor([[1.5, -2.0, -float('inf')], [0.0, -float('inf'), -float('inf')]])
    monkeypatch.setattr(ranking, 'predict_relations_mc', fake_mc)
    monkeypatch.setattr(ranking, 'predict_relations', fake)
    mc, one = str(tmp_path / 'mc.tsv'), str(tmp_path / 'one.tsv')
    assert train.write_mc_relation_predictions(mc, None, None, trip, 3, 'PF', 'FLPS', 'TC') == 6
    assert train.write_relation_predictions(one, None, None, trip, 3, 'PF', 'FLP', 'TC') == 6
    assert seen == {'mc': ('PF', 'FLPS', 'TC'), 'one': ('PF', 'FLP', 'TC')}
    assert open(mc).read().splitlines() == ['3\t4\t0\t2\t0.75\t0.125', '3\t4\t1\t0\t0.5\t0', '3\t4\t2\t-1\t-inf\t0',
                                            '5\t6\t0\t1\t1\t0.25', '5\t6\t1\t-1\t-inf\t0', '5\t6\t2\t-1\t-inf\t0']
    rows, mc_rows = [x.split('\t') for x in open(one).read().splitlines()], [x.split('\t') for x in open(mc).read().splitlines()]
    assert [x[:3] for x in rows] == [x[:3] for x in mc_rows] and all(len(x) == 5 for x in rows)      # the files join on three columns
    assert rows[0] == ['3', '4', '0', '2', '1.5'] and rows[2] == ['3', '4', '2', '-1', '-inf']
