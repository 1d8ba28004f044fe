"""The entity queries' host-side argument refusals, pinned (no GPU): every gv_rank_scores* / gv_topk_scores* / gv_entity_topk_scores /
gv_pair_prob_std_mc / gv_transe_rank_* / gv_transe_topk* entry and its ops wrapper is called with arguments that are turned down
before any launch, and the return code with the whole text of gv_last_error_string() -- resp. the exception's type and message --
is compared with tests/golden/query_entries_host.json.  The expected values are RECORDED from the library, not reasoned out: they
say what the entries do today, including the order in which two simultaneous faults are reported, so that host code shared between
the entries cannot change any of it unnoticed.  `python tests/test_query_entries_host.py --record` rewrites the file; do that only
when an entry's contract changes on purpose, and read the diff."""
import ctypes
import itertools
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'query_entries_host.json')
P = 'P'          # a non-NULL dummy pointer (tests/test_topk_host.py's pattern: nothing is launched, nothing reads it)
M, V, H, S, K = 4, 10, 8, 2, 5

# ---- the C entries: parameter names in ABI order and one valid call (filter, candidate sets and every output given) -------------
_Q = [('q', P), ('ld_q', H), ('e', P), ('ld_e', H)]
_QMC = [('q', P), ('ld_q', H), ('q_stride', M * H), ('e', P), ('ld_e', H), ('e_stride', V * H), ('n_samples', S)]
_FILT = [('filt_lo', P), ('filt_hi', P), ('filt_ent', P), ('n_filt_ent', 1)]
_CAND = [('cand', P), ('ld_cand', 1), ('n_sets', 1), ('cand_set', P)]
_MVH = [('m', M), ('v', V), ('h', H), ('stream', None)]
_TE = [('q', P), ('m', M), ('en', P), ('v', V), ('dim', H), ('p_norm', 2)]
_TE_FILT = [('f_lo', P), ('f_hi', P), ('f_ent', P)]
_TOPK_OUT = [('k', K), ('out_ids', P), ('out_logits', P), ('workspace', P)]
_COUNTS4 = [('tgt', P), ('count_raw', P), ('count_filt', P), ('count_raw_c', P), ('count_filt_c', P)]

ENTRIES = {
    'gv_rank_scores': _Q + [('target', P), ('bias', None), ('tgt', P), ('count', P)] + _MVH,
    'gv_rank_scores_filtered': _Q + [('target', P), ('bias', None)] + _FILT + [('tgt', P), ('count_raw', P), ('count_filt', P)] + _MVH,
    'gv_rank_scores_constrained': _Q + [('target', P), ('bias', None)] + _FILT + _CAND + _COUNTS4 + _MVH,
    'gv_rank_scores_mc': _QMC + [('target', P), ('bias', None)] + _FILT + [('tgt', P), ('count_raw', P), ('count_filt', P)] + _MVH,
    'gv_rank_scores_mc_constrained': _QMC + [('target', P), ('bias', None)] + _FILT + _CAND + _COUNTS4 + _MVH,
    'gv_topk_scores': _Q + [('bias', None)] + _FILT + _TOPK_OUT + _MVH,
    'gv_topk_scores_constrained': _Q + [('bias', None)] + _FILT + _CAND + _TOPK_OUT + _MVH,
    'gv_topk_scores_mc': _QMC + [('bias', None)] + _FILT + _TOPK_OUT + _MVH,
    'gv_topk_scores_mc_constrained': _QMC + [('bias', None)] + _FILT + _CAND + _TOPK_OUT + _MVH,
    'gv_entity_topk_scores': [('ents', P), ('m', M), ('e', P), ('ld_e', H), ('w', P), ('ld_w', H), ('bias', None)] + _FILT + [
        ('exclude_self', 1), ('k', K), ('span_tiles', 0), ('out_rel', P), ('out_ent', P), ('out_logits', P), ('workspace', P),
        ('workspace_bytes', 1 << 20), ('n', V), ('num_rels', 3), ('h', H), ('stream', None)],
    'gv_pair_prob_std_mc': _QMC + [('bias', None), ('ids', P), ('k', K), ('out_std', P)] + _MVH,
    'gv_transe_rank_filtered': _TE + [('target', P)] + _TE_FILT + [('counts_raw', P), ('counts_filt', P), ('stream', None)],
    'gv_transe_rank_constrained': _TE + [('target', P)] + _TE_FILT + _CAND + [
        ('counts_raw', P), ('counts_filt', P), ('counts_raw_c', P), ('counts_filt_c', P), ('stream', None)],
    'gv_transe_topk': _TE + _FILT + _TOPK_OUT + [('stream', None)],
    'gv_transe_topk_constrained': _TE + _FILT + _CAND + _TOPK_OUT + [('stream', None)],
}

# pointers an entry takes as NULL with everything else valid: such a call would be LAUNCHED, so no row may consist of them alone
OPTIONAL = {'bias', 'stream'}
OPTIONAL_OF = {'gv_rank_scores_filtered': {'count_raw'}}
# rows of the generic table that an entry ACCEPTS, and would launch: gv_transe_rank_filtered reads "no filter" off f_lo alone (with
# f_lo NULL the other two are not looked at), the two TransE rankers take any width, gv_pair_prob_std_mc any k >= 1
LAUNCHED = {'gv_transe_rank_filtered|f_lo=None', 'gv_transe_rank_filtered|f_lo=None,f_hi=None',
            'gv_transe_rank_filtered|f_lo=None,f_ent=None', 'gv_transe_rank_filtered|dim=513', 'gv_transe_rank_constrained|dim=513',
            'gv_pair_prob_std_mc|k=129'}

# single faults, by parameter name (applied to every entry that has the parameters); PAIRED: the ones combined two at a time
SIZES = [{'m': 0}, {'m': -1}, {'v': 0}, {'n': 0}, {'h': 0}, {'dim': 0}, {'dim': 513}, {'n_filt_ent': -1}, {'num_rels': 0},
         {'p_norm': 3}, {'span_tiles': -1}, {'workspace_bytes': 8}]
K_RANGE = [{'k': 129}, {'k': 0}]
LEADING = [{'ld_q': H - 1}, {'ld_e': H - 1}, {'ld_w': H - 1}]
SAMPLES = [{'n_samples': 0}, {'q_stride': M * H - 1}, {'e_stride': V * H - 1}]
CAND_GROUP = [{'cand': None}, {'cand_set': None}, {'n_sets': 0}, {'ld_cand': 0}, {'cand': None, 'cand_set': None}]
FILTERED_COUNTS = [{'count_filt': None}, {'count_filt_c': None}, {'count_filt': None, 'count_filt_c': None}, {'counts_filt': None},
                   {'counts_filt_c': None}, {'counts_filt': None, 'counts_filt_c': None}]
PAIRED = [{'m': 0}, {'v': 0}, {'n': 0}, {'k': 129}, {'ld_q': H - 1}, {'ld_w': H - 1}, {'n_samples': 0}, {'filt_hi': None},
          {'f_hi': None}, {'cand': None}, {'n_sets': 0}, {'q': None}, {'ents': None}, {'tgt': None}, {'out_ids': None},
          {'out_std': None}, {'count_filt': None}, {'counts_filt_c': None}, {'p_norm': 3}]


def _filter_names(params):
    return [n for n in ('filt_lo', 'filt_hi', 'filt_ent', 'f_lo', 'f_hi', 'f_ent') if n in params]


def entry_rows(name):
    """The argument tuples of one entry: [(row id, {parameter: value})], each differing from the valid call in one or two faults."""
    params = dict(ENTRIES[name])
    singles = [f for f in SIZES + K_RANGE + LEADING + SAMPLES + CAND_GROUP + FILTERED_COUNTS if set(f) <= set(params)]
    filt = _filter_names(params)
    for r in (1, 2):                                        # a partly given filter, in each of the six partial combinations
        singles += [dict.fromkeys(c) for c in itertools.combinations(filt, r)]
    optional = OPTIONAL | OPTIONAL_OF.get(name, set()) | set(filt) | {'cand', 'cand_set'}
    singles += [{p: None} for p, v in ENTRIES[name] if v == P and p not in optional]      # each required pointer NULL in turn
    pairs = [f for f in PAIRED if set(f) <= set(params)]
    faults = singles + [{**a, **b} for a, b in itertools.combinations(pairs, 2)]
    rows, seen = [], set()
    for f in faults:
        rid = name + '|' + ','.join(f'{p}={f[p]}' for p, _ in ENTRIES[name] if p in f)
        if rid in seen or rid in LAUNCHED:
            continue
        seen.add(rid)
        rows.append((rid, {**params, **f}))
    return rows


WORKSPACE_ROWS = {
    'gv_topk_scores_workspace_bytes': [(0, 10, 5), (-1, 10, 5), (4, 0, 5), (4, 10, 0), (4, 10, 129), (4, 10, 5), (4, 10, 128),
                                       (65, 700, 64), (40932, 14541, 10), (1, 14541, 100), (100000, 40943, 128)],
    'gv_entity_topk_scores_workspace_bytes': [(0, 10, 3, 5), (4, 0, 3, 5), (4, 10, 0, 5), (4, 10, 3, 0), (4, 10, 3, 129),
                                              (4, 1 << 20, 1 << 12, 5), (4, 10, 3, 5), (1, 14541, 237, 10), (14541, 14541, 237, 100),
                                              (40943, 40943, 11, 128)],
    'gv_transe_topk_workspace_bytes': [(0, 10, 5), (-1, 10, 5), (1 << 31, 10, 5), (4, 0, 5), (4, 10, 0), (4, 10, 129), (4, 10, 5),
                                       (40932, 14541, 10), (1, 14541, 100), ((1 << 31) - 1, 40943, 128)],
}


# ---- the ops wrappers: one valid call on CPU tensors each, and a table of bad inputs by argument name --------------------------
def _wrappers():
    z, i64 = torch.zeros, torch.long
    filt = dict(filt_lo=z(M, dtype=i64), filt_hi=torch.ones(M, dtype=i64), filt_ent=torch.tensor([3]))
    cand = dict(cand=z(2, 1, dtype=torch.int32), cand_set=z(M, dtype=i64))
    tgt = dict(target=torch.arange(M))
    dm = dict(q=z(M, H), entities=z(V, H))
    mc = dict(q=z(S, M, H), entities=z(S, V, H), bias=z(S))
    te = dict(q=z(M, H), en=z(V, H), p_norm=2)
    return {
        'rank_scores': {**dm, **tgt},
        'rank_scores_filtered': {**dm, **tgt, **filt},
        'rank_scores_constrained': {**dm, **tgt, **cand, **filt},
        'rank_scores_mc': {**mc, **tgt, **filt},
        'rank_scores_mc_constrained': {**mc, **tgt, **cand, **filt},
        'topk_scores': {**dm, 'k': K, **filt},
        'topk_scores_constrained': {**dm, 'k': K, **cand, **filt},
        'topk_scores_mc': {**mc, 'k': K, **filt},
        'topk_scores_mc_constrained': {**mc, 'k': K, **cand, **filt},
        'entity_topk_scores': dict(ents=torch.arange(M), emb=z(V, H), w=z(3, H), k=K, filt_lo=z(3 * V, dtype=i64),
                                   filt_hi=torch.ones(3 * V, dtype=i64), filt_ent=torch.tensor([3])),
        'pair_prob_std_mc': {**mc, 'ids': z(M, K, dtype=i64)},
        'transe_rank_filtered': {**te, **tgt, **filt},
        'transe_rank_constrained': {**te, **tgt, **cand, **filt},
        'transe_topk': {**te, 'k': K, **filt},
        'transe_topk_constrained': {**te, 'k': K, **cand, **filt},
    }


def _bad_inputs(good):
    """(label, {argument: bad value}) for the arguments the wrapper has; `table` is its entity table, whatever it is called."""
    z, i64 = torch.zeros, torch.long
    table = next(n for n in ('entities', 'emb', 'en') if n in good)
    first = 'q' if 'q' in good else 'w'
    mc = good[table].dim() == 3
    lead = (S,) if mc else ()
    n_rows = good['filt_lo'].numel() if 'filt_lo' in good else 0
    bad = [
        ('valid', {}),
        ('rank', {first: z(H)}), ('rank-table', {table: z(*lead, V, H, 1)}), ('not-a-tensor', {first: None}),
        ('width', {table: z(*lead, V, H - 1)}), ('no-entities', {table: z(*lead, 0, H)}),
        ('no-width', {first: z(*lead, good[first].shape[-2], 0), table: z(*lead, V, 0)}),
        ('samples', {table: z(S + 1, V, H)} if mc else None),
        ('targets', {'target': torch.arange(M - 1)}), ('target-high', {'target': torch.tensor([0, 1, 2, V])}),
        ('target-low', {'target': torch.tensor([0, -1, 2, 3])}),
        ('k-low', {'k': 0}), ('k-high', {'k': 129}),
        ('half-filter-lo', {'filt_lo': None}), ('half-filter-ent', {'filt_ent': None}),
        ('half-filter-hi-only', {'filt_lo': None, 'filt_ent': None}),
        ('no-filter', {'filt_lo': None, 'filt_hi': None, 'filt_ent': None}),
        ('ranges', {'filt_lo': z(n_rows - 1, dtype=i64), 'filt_hi': torch.ones(n_rows - 1, dtype=i64)} if n_rows else None),
        ('unsorted', {'filt_lo': torch.ones(n_rows, dtype=i64), 'filt_hi': z(n_rows, dtype=i64)}),
        ('range-end', {'filt_hi': torch.full((n_rows,), 2, dtype=i64)}),
        ('filter-id', {'filt_ent': torch.tensor([V])}), ('filter-id-low', {'filt_ent': torch.tensor([-1])}),
        ('cand-dtype', {'cand': z(2, 1, dtype=i64)}), ('cand-shape', {'cand': z(2, dtype=torch.int32)}),
        ('cand-words', {'cand': z(2, 0, dtype=torch.int32)}), ('sets', {'cand_set': z(M - 1, dtype=i64)}),
        ('bias', {'bias': z(S + 1)} if mc else None),
        ('ents-float', {'ents': z(M)}), ('ents-high', {'ents': torch.tensor([0, V])}), ('span', {'span': 0}),
        ('ids-shape', {'ids': z(M + 1, K, dtype=i64)}), ('ids-high', {'ids': torch.full((M, K), V, dtype=i64)}),
        ('p-norm', {'p_norm': 3}),
    ]
    extra = {'span'} if 'ents' in good else set()
    bad = [(label, f) for label, f in bad if f is not None and set(f) <= set(good) | extra]
    pairs = [b for b in bad if b[0] in ('width', 'targets', 'target-high', 'k-low', 'half-filter-lo', 'unsorted', 'filter-id',
                                        'cand-dtype', 'sets', 'bias', 'ents-high', 'ids-high')]
    for (la, fa), (lb, fb) in itertools.combinations(pairs, 2):
        if not set(fa) & set(fb):
            bad.append((f'{la}+{lb}', {**fa, **fb}))
    return bad


def wrapper_rows(name):
    good = _wrappers()[name]
    return [(f'ops.{name}|{label}', {**good, **f}) for label, f in _bad_inputs(good)]


# ---- running a row ----------------------------------------------------------------------------------------------------------------
def _call_entry(name, args, dummy):
    from gcn_vae_amd import lib
    fn = getattr(lib.load(), name)
    rc = fn(*[dummy if args[p] == P else args[p] for p, _ in ENTRIES[name]])
    return [rc, lib.last_error() if rc else '']          # (a call that returns GV_OK leaves the previous call's text in place)


def _call_wrapper(name, kwargs):
    from gcn_vae_amd import ops
    try:
        getattr(ops, name)(**kwargs)
    except Exception as exc:      # noqa: BLE001  (the type is what is recorded)
        return [type(exc).__name__, str(exc)]
    return ['returned', '']


def observe():
    from gcn_vae_amd import lib
    buf = (ctypes.c_int32 * 64)()
    dummy = ctypes.addressof(buf)
    seen = {}
    for name in ENTRIES:
        for rid, args in entry_rows(name):
            seen[rid] = _call_entry(name, args, dummy)
    for name, rows in WORKSPACE_ROWS.items():
        for row in rows:
            seen[f'{name}|{",".join(map(str, row))}'] = int(getattr(lib.load(), name)(*row))
    for name in _wrappers():
        for rid, kwargs in wrapper_rows(name):
            seen[rid] = _call_wrapper(name, kwargs)
    return seen


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def observed():
    return observe()


def test_the_table_is_the_recorded_one(recorded, observed):
    assert sorted(observed) == sorted(recorded)


def test_no_recorded_row_reaches_a_launch(recorded):
    for name in ENTRIES:
        rows = {rid: v for rid, v in recorded.items() if rid.startswith(name + '|')}
        assert len(rows) > 20, name
        for rid, (rc, text) in rows.items():
            # GV_ERR_NULL or GV_ERR_SHAPE (a launch's status would be positive), or the early return of an empty query set
            assert rc in (-1, -2) or (rc == 0 and 'm=0' in rid.split('|')[1].split(',')), rid
            assert rc == 0 or text.startswith(name + ':'), rid
        assert sum(1 for rid in rows if rid.count('=') >= 2) >= 3, name                     # two faults at once


@pytest.mark.parametrize('name', list(ENTRIES))
def test_c_entry_refusals(name, recorded, observed):
    for rid, _ in entry_rows(name):
        assert observed[rid] == recorded[rid], rid


@pytest.mark.parametrize('name', list(WORKSPACE_ROWS))
def test_workspace_sizes(name, recorded, observed):
    for rid in observed:
        if rid.startswith(name + '|'):
            assert observed[rid] == recorded[rid], rid


@pytest.mark.parametrize('name', list(_wrappers()))
def test_ops_wrapper_refusals(name, recorded, observed):
    rows = wrapper_rows(name)
    assert any(observed[rid][1].endswith('there is no CPU fallback') for rid, _ in rows)       # the valid call ends there
    for rid, _ in rows:
        assert observed[rid] == recorded[rid], rid
        assert observed[rid][0] != 'returned', rid


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(GOLDEN, 'w') as out:
        json.dump(observe(), out, indent=0, sort_keys=True)
        out.write('\n')
    print(f'recorded {GOLDEN}')
