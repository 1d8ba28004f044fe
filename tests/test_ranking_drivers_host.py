"""The evaluation drivers of ranking.py and transe.py without a GPU: ``ranking.ops`` and ``transe.ops`` are replaced by a stub whose
entries state the rank rule in plain torch on materialised scores and record every call, so that the chunk loops, the truncation,
the empty results, the None pattern, the order of the ops calls, the returned dicts and the printed text are all pinned on CPU
tensors.  Every table is integer-valued (scores are exact, real ties occur); the Monte-Carlo samples are multiples of 10, so every
logit is a multiple of 100 and every per-sample probability exactly 0, 0.5 or 1, wherever it stands in a chunk.  Chunk constants
are 4: the 11 test triplets go as chunks of 4, 4, 3.  The brute-force loop is test_type_constraint_host's, the sigmoid
test_mc_rank_host's."""
import pytest
import torch

from gcn_vae_amd import ranking, transe
from test_mc_rank_host import _sig
from test_type_constraint_host import _brute

N, R, H = 23, 3, 4
KINDS = ('raw', 'filtered', 'raw_constrained', 'filtered_constrained')
_gen = torch.Generator().manual_seed(11)
EMB = torch.randint(-2, 3, (N, H), generator=_gen).float()
EMB[7] = EMB[3]                                                       # two entities that tie everywhere
W = torch.randint(-1, 3, (R, H), generator=_gen).float()
TEST = torch.tensor([[0, 0, 5], [0, 0, 9], [3, 1, 7], [3, 1, 2], [12, 2, 0], [22, 0, 1], [4, 2, 4], [9, 1, 22], [0, 0, 5], [15, 2, 7],
                     [6, 1, 3]])                                      # (0, 0) and (3, 1) queried twice, one triplet repeated
MORE = torch.tensor([[0, 0, 3], [0, 0, 7], [3, 1, 11], [5, 1, 7], [8, 1, 7], [12, 2, 19], [1, 0, 1], [20, 2, 4], [21, 2, 7]])
KNOWN = torch.cat([TEST, MORE])
FI = ranking.FilterIndex(N, R, KNOWN)
TC = ranking.TypeConstraint(N, R, KNOWN)
FLIP = torch.where(torch.arange(N) % 2 == 1, -1.0, 1.0).view(N, 1)
Z = {'same': torch.stack([10 * EMB, 10 * EMB]),                       # one sample twice: pbar ties wherever the logits tie
     'mirrored': torch.stack([10 * EMB, 10 * EMB * FLIP])}            # odd entities negated: their logits change sign
FLP = torch.tensor([100.0, -100.0])
ROWS = (4, 4, 3)


def _rule(value, target, listed=None, cand=None):
    """The rank rule written out: better is ``~(x <= tgt)``, ties count half, the target is left out of every pool."""
    tgt = value.gather(1, target.view(-1, 1))
    other = torch.ones_like(value, dtype=torch.bool).scatter_(1, target.view(-1, 1), False)
    better, equal = ~(value <= tgt) & other, (value == tgt) & other

    def rank(pool):
        return (better & pool).sum(1).float() + 0.5 * (equal & pool).sum(1).float()
    keep = None if listed is None else ~listed
    return (rank(other), None if keep is None else rank(keep), None if cand is None else rank(cand),
            None if keep is None or cand is None else rank(cand & keep))


def _pbar(z, a, r, flp):
    total = 0
    for s in range(z.shape[0]):
        total = total + torch.sigmoid((z[s][a] * W[r]) @ z[s].T + (0.0 if flp is None else flp[s]))
    return total / z.shape[0]


def _distance(ent, a, r, head):
    q = ent[a] - W[r] if head else ent[a] + W[r]
    return (q.unsqueeze(1) - ent.unsqueeze(0)).abs().sum(-1)


def _want(value_of, trip=TEST):
    """{'s': ..., 'o': ...}: ``_rule``'s four ranks of every triplet at once, the masks from Python sets of the known triplets."""
    known = {tuple(t) for t in KNOWN.tolist()}
    subj = [{s for s, r, _ in known if r == x} for x in range(R)]
    obj = [{o for _, r, o in known if r == x} for x in range(R)]
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    out = {}
    for d, a, b in (('s', o, s), ('o', s, o)):
        listed = torch.tensor([[((j, x, e) if d == 's' else (e, x, j)) in known for j in range(N)]
                               for e, x in zip(a.tolist(), r.tolist())]).reshape(-1, N)
        cand = torch.tensor([[j in (subj if d == 's' else obj)[x] for j in range(N)] for x in r.tolist()]).reshape(-1, N)
        out[d] = _rule(value_of(a, r, d), b, listed, cand)
    return out


WANT = _want(lambda a, r, d: (EMB[a] * W[r]) @ EMB.T)
WANT_TRANSE = _want(lambda a, r, d: -_distance(EMB, a, r, d == 's'))
WANT_MC = {(name, biased): _want(lambda a, r, d: _pbar(z, a, r, FLP if biased else None))
           for name, z in Z.items() for biased in (False, True)}


class StubOps:
    """What the drivers call of ``ops``, in plain torch, each call recorded as (name, rows, direction of the candidate sets,
    direction of the filter): a direction is read off the set ids and off which of the index's lists came in."""

    def __init__(self):
        self.calls = []

    def _masks(self, m, lo, hi, ent, words=None, sets=None):
        listed = None
        if ent is not None:
            listed = torch.zeros(m, N, dtype=torch.bool)
            for i in range(m):
                listed[i, ent[int(lo[i]):int(hi[i])].long()] = True
        cand = None
        if sets is not None:
            cand = torch.tensor([[bool(int(words[int(x), j >> 5]) >> (j & 31) & 1) for j in range(N)] for x in sets]).reshape(m, N)
        return listed, cand

    def _dirs(self, ent, sets=None):
        f = None if ent is None else next(d for d in 'so' if ent is FI.ent[d])
        if sets is None:
            return (f,)
        assert sets.dtype == torch.int32 and (bool((sets >= R).all()) or bool((sets < R).all()))
        return ('s' if bool((sets >= R).all()) else 'o', f)

    def _rank(self, name, value, target, lo, hi, ent, words=None, sets=None):
        self.calls.append((name, value.shape[0]) + self._dirs(ent, sets))
        return _rule(value, target, *self._masks(value.shape[0], lo, hi, ent, words, sets))

    def mul(self, a, b):
        self.calls.append(('mul', a.shape[-2]))
        return a * b

    def gemm(self, a, b, trans_b=False, precision=None):
        self.calls.append(('gemm', a.shape[0]))
        return a @ (b.T if trans_b else b)

    def rank_scores(self, q, entities, target, bias=None):
        self.calls.append(('rank_scores', q.shape[0]))
        return _rule(q @ entities.T + (0.0 if bias is None else bias), target)[0]

    def rank_scores_filtered(self, q, entities, target, filt_lo, filt_hi, filt_ent, bias=None):
        return self._rank('rank_scores_filtered', q @ entities.T + (0.0 if bias is None else bias), target, filt_lo, filt_hi,
                          filt_ent)[:2]

    def rank_scores_constrained(self, q, entities, target, cand, cand_set, filt_lo=None, filt_hi=None, filt_ent=None, bias=None):
        return self._rank('rank_scores_constrained', q @ entities.T + (0.0 if bias is None else bias), target, filt_lo, filt_hi,
                          filt_ent, cand, cand_set)

    def _mc(self, q, entities, bias):
        total = 0
        for s in range(q.shape[0]):
            total = total + torch.sigmoid(q[s] @ entities[s].T + (0.0 if bias is None else bias[s]))
        return total / q.shape[0]

    def rank_scores_mc(self, q, entities, target, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
        pbar = self._mc(q, entities, bias)
        return self._rank('rank_scores_mc', pbar, target, filt_lo, filt_hi, filt_ent)[:2] + (pbar.gather(1, target.view(-1, 1)),)

    def rank_scores_mc_constrained(self, q, entities, target, cand, cand_set, bias=None, filt_lo=None, filt_hi=None, filt_ent=None):
        pbar = self._mc(q, entities, bias)
        return self._rank('rank_scores_mc_constrained', pbar, target, filt_lo, filt_hi, filt_ent, cand, cand_set) + (
            pbar.gather(1, target.view(-1, 1)),)

    def transe_queries(self, ent, rel=None, a=None, r=None, head=False, norm_flag=True):
        assert norm_flag is False                                     # the tests rank unnormalised tables: integers throughout
        if rel is None:
            self.calls.append(('transe_queries', 'table'))
            return ent.clone()
        self.calls.append(('transe_queries', a.shape[0], 'head' if head else 'tail'))
        return ent[a] - rel[r] if head else ent[a] + rel[r]

    def transe_distances(self, q, en, p_norm):
        assert p_norm == 1
        self.calls.append(('transe_distances', q.shape[0]))
        return (q.unsqueeze(1) - en.unsqueeze(0)).abs().sum(-1)

    def transe_rank_filtered(self, q, en, target, p_norm, filt_lo=None, filt_hi=None, filt_ent=None):
        assert p_norm == 1
        raw, filt = self._rank('transe_rank_filtered', -(q.unsqueeze(1) - en.unsqueeze(0)).abs().sum(-1), target, filt_lo, filt_hi,
                               filt_ent)[:2]
        return raw, raw.clone() if filt is None else filt             # the kernel writes both counts, filter or not

    def transe_rank_constrained(self, q, en, target, p_norm, cand, cand_set, filt_lo=None, filt_hi=None, filt_ent=None):
        assert p_norm == 1
        return self._rank('transe_rank_constrained', -(q.unsqueeze(1) - en.unsqueeze(0)).abs().sum(-1), target, filt_lo, filt_hi,
                          filt_ent, cand, cand_set)


@pytest.fixture
def stub(monkeypatch):
    ops = StubOps()
    monkeypatch.setattr(ranking, 'ops', ops)
    monkeypatch.setattr(transe, 'ops', ops)
    for name in ('MAX_QUERY_ROWS', 'MC_STACK_ROWS', 'MC_UNFUSED_ROWS'):
        monkeypatch.setattr(ranking, name, 4)
    monkeypatch.setattr(transe, 'MAX_QUERY_ROWS', 4)
    return ops


def _calls(per_chunk, rows=ROWS, first=()):
    """The expected record: ``first``, then every 's' chunk, then every 'o' chunk, ``per_chunk(rows, direction)`` each."""
    return list(first) + [c for d in 'so' for m in rows for c in per_chunk(m, d)]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None and w is None) or (g.dtype == torch.float32 and torch.equal(g, w))


def _cut(want, n, kinds, width=4):
    """The first ``n`` rows of the kinds (positions in ``KINDS``) a protocol reports, None for the others of its ``width``."""
    return tuple(want[i][:n] if i in kinds else None for i in range(width))


def _dict(by_s, by_o, hits, lead=()):
    out = dict(lead)
    for kind, rs, ro in zip(KINDS, by_s, by_o):
        if rs is not None:
            ranks = torch.cat([rs, ro]) + 1
            out['mrr_' + kind] = torch.mean(1.0 / ranks.float()).item()
            out['hits_' + kind] = {hit: torch.mean((ranks <= hit).float()).item() for hit in hits}
    return out


def _lines(out, hits, mc=False):
    lines = []
    for kind in (k for k in KINDS if 'mrr_' + k in out):
        if mc:
            lines.append("MC MRR ({}, {} samples): {:.6f}".format(kind, out['n_samples'], out['mrr_' + kind]))
            lines += ["MC Hits ({}) @ {}: {:.6f}".format(kind, hit, out['hits_' + kind][hit]) for hit in hits]
        else:
            lines.append("MRR ({}): {:.6f}".format(kind, out['mrr_' + kind]))
            lines += ["Hits ({}) @ {}: {:.6f}".format(kind, hit, out['hits_' + kind][hit]) for hit in hits]
    return ''.join(line + '\n' for line in lines)


def _progress(fmt, ranks, heads):
    """The cumulative line a verbose driver prints after each of its chunks of 4, 4, 3."""
    out = ''
    for head, hi in zip(heads, (4, 8, 11)):
        x = 1.0 + ranks[:hi].float()
        out += fmt.format(*head, x.mean().item(), (1.0 / x).mean().item()) + '\n'
    return out


S_, R_, O_ = TEST[:, 0], TEST[:, 1], TEST[:, 2]
BOTH = (('s', O_, S_), ('o', S_, O_))
EMPTY = torch.zeros(0, dtype=torch.long)


# ---- the single-draw rank drivers ------------------------------------------------------------------------------------------
def test_raw_driver_fused_and_unfused(stub, capsys):
    for d, a, b in BOTH:
        for fn, second, fmt, heads in (
                (ranking.perturb_and_get_rank, 'rank_scores', "rows {} / {}: MR : {:.6f} |  MRR : {:.6f}", [(4, 11), (8, 11), (11, 11)]),
                (ranking.perturb_and_get_rank_unfused, 'gemm', "batch {} / {}: MR : {:.6f} |  MRR : {:.6f}", [(0, 3), (1, 3), (2, 3)])):
            stub.calls.clear()
            got = fn(EMB, W, a, R_, b, 11, batch_size=4, verbose=True)
            _same((got,), WANT[d][:1])
            assert stub.calls == [c for m in ROWS for c in (('mul', m), (second, m))]
            assert capsys.readouterr().out == _progress(fmt, WANT[d][0], heads)
            stub.calls.clear()
            _same((fn(EMB, W, a, R_, b, 11, batch_size=5, all_batches=False, flow_log_prob=torch.tensor(3.0)),), _cut(WANT[d], 5, {0}, 1))
            rows = (4, 1) if fn is ranking.perturb_and_get_rank else (5,)         # the unfused route chunks by batch_size
            assert stub.calls == [c for m in rows for c in (('mul', m), (second, m))]
            assert capsys.readouterr().out == ''
    empty = ranking.perturb_and_get_rank(EMB, W, EMPTY, EMPTY, EMPTY, 0)
    assert empty.dtype == torch.float32 and tuple(empty.shape) == (0,) and empty.device == EMB.device


def test_filtered_driver(stub, capsys):
    for d, a, b in BOTH:
        stub.calls.clear()
        _same(ranking.perturb_and_get_rank_filtered(EMB, W, a, R_, b, 11, FI, d, verbose=True), WANT[d][:2])
        assert stub.calls == [c for m in ROWS for c in (('mul', m), ('rank_scores_filtered', m, d))]
        assert capsys.readouterr().out == _progress("rows {} / {}: MR (filtered) : {:.6f} |  MRR (filtered) : {:.6f}", WANT[d][1],
                                                    [(4, 11), (8, 11), (11, 11)])
        _same(ranking.perturb_and_get_rank_filtered(EMB, W, a, R_, b, 11, FI, d, 5, False), _cut(WANT[d], 5, {0, 1}, 2))
        assert capsys.readouterr().out == ''
    raw, filt = ranking.perturb_and_get_rank_filtered(EMB, W, EMPTY, EMPTY, EMPTY, 0, FI, 'o')
    assert raw is not filt and raw.dtype == filt.dtype == torch.float32 and raw.shape == filt.shape == (0,)


@pytest.mark.parametrize('filtered', [True, False])
def test_constrained_driver(stub, filtered):
    fi, kinds = (FI, {0, 1, 2, 3}) if filtered else (None, {0, 2})
    for d, a, b in BOTH:
        stub.calls.clear()
        _same(ranking.perturb_and_get_rank_constrained(EMB, W, a, R_, b, 11, fi, TC, d), _cut(WANT[d], 11, kinds))
        assert stub.calls == [c for m in ROWS for c in (('mul', m), ('rank_scores_constrained', m, d, d if filtered else None))]
        _same(ranking.perturb_and_get_rank_constrained(EMB, W, a, R_, b, 11, fi, TC, d, 5, False), _cut(WANT[d], 5, kinds))
    _same(ranking.perturb_and_get_rank_constrained(EMB, W, EMPTY, EMPTY, EMPTY, 0, fi, TC, 'o'), _cut(WANT['o'], 0, kinds))


# ---- the Monte-Carlo rank drivers ------------------------------------------------------------------------------------------
def _mc_chunk(entry, fused, filtered, typed):
    if not fused:
        return lambda m, d: [('mul', m), ('gemm', m)] * 2                    # one product per sample
    return lambda m, d: [('mul', m), (entry, m) + ((d,) if typed else ()) + (d if filtered else None,)]


@pytest.mark.parametrize('sample', ['same', 'mirrored'])
@pytest.mark.parametrize('filtered', [True, False])
@pytest.mark.parametrize('fused', [True, False])
def test_mc_drivers(stub, sample, filtered, fused):
    z, want = Z[sample], WANT_MC[sample, False]
    fi = FI if filtered else None
    plain = ranking.perturb_and_get_rank_mc if fused else ranking.perturb_and_get_rank_mc_unfused
    typed = ranking.perturb_and_get_rank_mc_constrained if fused else ranking.perturb_and_get_rank_mc_constrained_unfused
    for fn, extra, kinds, entry in ((plain, (), {0, 1} if filtered else {0}, 'rank_scores_mc'),
                                    (typed, (TC,), {0, 1, 2, 3} if filtered else {0, 2}, 'rank_scores_mc_constrained')):
        width = 4 if extra else 2
        for d, a, b in BOTH:
            stub.calls.clear()
            _same(fn(z, W, a, R_, b, 11, fi, *extra, d), _cut(want[d], 11, kinds, width))
            assert stub.calls == [c for m in ROWS for c in _mc_chunk(entry, fused, filtered, bool(extra))(m, d)]
            _same(fn(z, W, a, R_, b, 11, fi, *extra, d, 5, False), _cut(want[d], 5, kinds, width))
        got = fn(z, W, EMPTY, EMPTY, EMPTY, 0, fi, *extra, 'o')
        _same(got, _cut(want['o'], 0, kinds, width))
        assert all(x is None or x.device == z.device for x in got)
        if filtered:
            assert got[0] is not got[1]


# ---- the two-direction reports ---------------------------------------------------------------------------------------------
HITS = [1, 3, 10]


def test_calc_mrr(stub, capsys):
    bias = torch.tensor(3.0)
    want = _dict(WANT['s'][:1], WANT['o'][:1], HITS)
    got = ranking.calc_mrr(EMB, W, TEST, hits=HITS, flow_log_prob=bias)
    assert isinstance(got, float) and got == want['mrr_raw']
    assert capsys.readouterr().out == _lines(want, HITS)
    assert stub.calls == _calls(lambda m, d: [('mul', m), ('rank_scores', m)])
    stub.calls.clear()
    cut = _dict(_cut(WANT['s'], 5, {0}, 1), _cut(WANT['o'], 5, {0}, 1), HITS)
    assert ranking.calc_mrr(EMB, W, TEST, hits=HITS, eval_bz=5, all_batches=False, verbose=False) == cut['mrr_raw']
    assert capsys.readouterr().out == ''
    assert stub.calls == _calls(lambda m, d: [('mul', m), ('rank_scores', m)], rows=(4, 1))


def test_calc_filtered_mrr(stub, capsys):
    want = _dict(WANT['s'][:2], WANT['o'][:2], HITS)
    got = ranking.calc_filtered_mrr(EMB, W, TEST, FI, hits=HITS, flow_log_prob=torch.tensor(3.0))
    assert got == want and list(got) == ['mrr_raw', 'hits_raw', 'mrr_filtered', 'hits_filtered']
    assert capsys.readouterr().out == _lines(want, HITS)
    assert stub.calls == _calls(lambda m, d: [('mul', m), ('rank_scores_filtered', m, d)])
    stub.calls.clear()
    cut = _dict(_cut(WANT['s'], 5, {0, 1}), _cut(WANT['o'], 5, {0, 1}), HITS)
    assert ranking.calc_filtered_mrr(EMB, W, TEST, FI, hits=HITS, eval_bz=5, all_batches=False, verbose=False) == cut
    assert capsys.readouterr().out == ''
    assert stub.calls == _calls(lambda m, d: [('mul', m), ('rank_scores_filtered', m, d)], rows=(4, 1))


@pytest.mark.parametrize('filtered', [True, False])
def test_calc_constrained_mrr(stub, capsys, filtered):
    fi, kinds = (FI, {0, 1, 2, 3}) if filtered else (None, {0, 2})
    want = _dict(_cut(WANT['s'], 11, kinds), _cut(WANT['o'], 11, kinds), HITS)
    got = ranking.calc_constrained_mrr(EMB, W, TEST, fi, TC, hits=HITS)
    assert got == want and list(got) == list(want) and len(got) == 2 * len(kinds)
    assert capsys.readouterr().out == _lines(want, HITS)
    assert stub.calls == _calls(lambda m, d: [('mul', m), ('rank_scores_constrained', m, d, d if filtered else None)])
    stub.calls.clear()
    cut = _dict(_cut(WANT['s'], 5, kinds), _cut(WANT['o'], 5, kinds), HITS)
    assert ranking.calc_constrained_mrr(EMB, W, TEST, fi, TC, hits=HITS, eval_bz=5, all_batches=False, verbose=False) == cut
    assert capsys.readouterr().out == ''
    assert [c[1] for c in stub.calls] == [4, 4, 1, 1] * 2


@pytest.mark.parametrize('sample', ['same', 'mirrored'])
@pytest.mark.parametrize('filtered', [True, False])
@pytest.mark.parametrize('fused', [True, False])
def test_calc_mc_reports(stub, capsys, sample, filtered, fused):
    z, by = Z[sample], WANT_MC[sample, True]
    fi = FI if filtered else None
    plain = ranking.calc_mc_mrr if fused else ranking.calc_mc_mrr_unfused
    typed = ranking.calc_mc_constrained_mrr if fused else ranking.calc_mc_constrained_mrr_unfused
    for fn, extra, kinds, entry in ((plain, (), {0, 1} if filtered else {0}, 'rank_scores_mc'),
                                    (typed, (TC,), {0, 1, 2, 3} if filtered else {0, 2}, 'rank_scores_mc_constrained')):
        stub.calls.clear()
        want = _dict(_cut(by['s'], 11, kinds), _cut(by['o'], 11, kinds), HITS, {'n_samples': 2})
        got = fn(z, W, TEST, fi, *extra, FLP, hits=HITS)
        assert got == want and list(got) == list(want) and list(got)[0] == 'n_samples'
        assert capsys.readouterr().out == _lines(want, HITS, mc=True)
        assert stub.calls == _calls(_mc_chunk(entry, fused, filtered, bool(extra)))
        stub.calls.clear()
        cut = _dict(_cut(by['s'], 5, kinds), _cut(by['o'], 5, kinds), HITS, {'n_samples': 2})
        assert fn(z, W, TEST, fi, *extra, FLP, hits=HITS, eval_bz=5, all_batches=False, verbose=False) == cut
        assert capsys.readouterr().out == ''
        assert stub.calls == _calls(_mc_chunk(entry, fused, filtered, bool(extra)), rows=(4, 1))
        stub.calls.clear()
        with pytest.raises(ValueError, match='per sample'):           # refused before anything is ranked
            fn(z, W, TEST, fi, *extra, torch.zeros(3), hits=HITS)
        assert stub.calls == []


# ---- the TransE rankers ----------------------------------------------------------------------------------------------------
def _transe_want(filtered):
    """All head queries, then all tail queries; without a filter the filtered positions hold their unfiltered twins."""
    pick = (0, 1, 2, 3) if filtered else (0, 0, 2, 2)
    return tuple(torch.cat([WANT_TRANSE['s'][i], WANT_TRANSE['o'][i]]) for i in pick)


@pytest.mark.parametrize('filtered', [True, False])
def test_transe_rankers(stub, filtered):
    fi, f = (FI, lambda d: d) if filtered else (None, lambda d: None)
    want = _transe_want(filtered)
    side = {'s': 'head', 'o': 'tail'}
    table = [('transe_queries', 'table')]                             # the normalised table, once per call
    _same(transe.rank_transe(EMB, W, TEST, 1, False, fi), want[:2])
    assert stub.calls == _calls(lambda m, d: [('transe_queries', m, side[d]), ('transe_rank_filtered', m, f(d))], first=table)
    stub.calls.clear()
    _same(transe.rank_transe_unfused(EMB, W, TEST, 1, False, fi, batch=4), want[:2])
    assert stub.calls == []                                           # plain torch
    _same(transe.rank_transe_constrained(EMB, W, TEST, 1, False, TC, fi), want)
    assert stub.calls == _calls(lambda m, d: [('transe_queries', m, side[d]), ('transe_rank_constrained', m, d, f(d))], first=table)
    stub.calls.clear()
    _same(transe.rank_transe_constrained_unfused(EMB, W, TEST, 1, False, TC, fi, batch=4), want)
    assert stub.calls == _calls(lambda m, d: [('transe_queries', m, side[d]), ('transe_distances', m)], first=table)
    none = torch.zeros(0, 3, dtype=torch.long)
    for fn, extra in ((transe.rank_transe, ()), (transe.rank_transe_unfused, ()), (transe.rank_transe_constrained, (TC,)),
                      (transe.rank_transe_constrained_unfused, (TC,))):
        with pytest.raises((ValueError, RuntimeError), match='non-empty list'):      # torch.cat of no chunks, as torch words it
            fn(EMB, W, none, 1, False, *extra, fi)


# ---- the one rule ----------------------------------------------------------------------------------------------------------
def test_the_single_rule_against_the_brute_force_loops():
    rule = getattr(ranking, 'mid_ranks', None)
    if rule is None:
        pytest.skip('ranking.mid_ranks is not there yet')
    gen = torch.Generator().manual_seed(5)
    m, v = 8, 37
    score = torch.randint(-3, 4, (m, v), generator=gen).float()       # ties everywhere
    target = torch.randint(0, v, (m,), generator=gen)
    cand, listed = torch.rand(m, v, generator=gen) < 0.5, torch.rand(m, v, generator=gen) < 0.3
    score[1, [2, 9, 30]] = float('nan')                               # NaN candidates, listed and members or not
    score[2, target[2]] = float('nan')                                # a NaN target ranks last
    listed[3, target[3]], cand[4, target[4]], cand[5] = True, False, False
    pbar = torch.tensor([[_sig(float(x)) for x in row] for row in score.tolist()], dtype=torch.float64)
    for value in (score, pbar):
        want = _brute(value.numpy(), target.tolist(), cand.numpy(), listed.numpy())
        full = rule(value, target, listed, cand)
        assert [x.tolist() for x in full] == want.tolist() and all(x.dtype == torch.float32 for x in full)
        _same(rule(value, target), (full[0], None, None, None))
        _same(rule(value, target, listed), (full[0], full[1], None, None))
        _same(rule(value, target, cand_mask=cand), (full[0], None, full[2], None))
        # the three public statements of the rule are thin calls of it
        assert torch.equal(ranking.sort_and_rank(value, target), full[0])
        _same(ranking.rank_from_scores_constrained(value, target, cand, listed), full)
        _same(ranking.rank_from_scores_constrained(value, target, cand), (full[0], None, full[2], None))
        _same(ranking.mc_ranks_from_probs(value, target, listed), full[:2])
        _same(ranking.mc_ranks_from_probs(value, target), (full[0], None))
        _same(full, _rule(value, target, listed, cand))               # and the stub above states the same rule
