"""Per-relation completion for the TransE baseline, the parts that need no GPU: the rule (transe.complete_relations_from_distances
against three Python loops per relation), the per-relation level walk of ops._mine_drive_by_relation with ``ascending=True`` driven
by a fake launch that plays gv_transe_mine_by_relation on a materialised distance tensor in numpy, the default ``ascending=False``
path on one fixed case, the argument checks of the wrappers and of the two entries (nothing is launched), and the command line."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mine_cases import filter_arrays
from relation_profile_cases import same
from transe_relation_profile_cases import brute_force_distances

NAN, INF = float('nan'), float('inf')


def distances(n, num_rels, dim, seed, special=True, p=1):
    gen = torch.Generator().manual_seed(seed)
    en, rn = torch.randn(n, dim, generator=gen), torch.randn(num_rels, dim, generator=gen)
    if special and n >= 8:
        en[5] = en[2]                        # exact ties, across and within subjects, and zero distances under a zero relation
        en[6] = en[2]
        en[4] = NAN                          # a NaN row (and column)
        en[7, 0] = INF                       # +inf distances; NaN against itself
    if special and num_rels >= 2:
        rn[1] = 0.0                          # d(s, 1, o) = d(o, 1, s): ties by (s, o), and exact zeros between the duplicated rows
    diff = (en.view(1, n, 1, dim) + rn.view(num_rels, 1, 1, dim)) - en.view(1, 1, n, dim)
    return diff.abs().sum(-1) if p == 1 else diff.pow(2).sum(-1).sqrt()


def random_filter(n, num_rels, seed):
    gen = torch.Generator().manual_seed(seed)
    return {(int(a), int(b), int(c)) for a, b, c in zip(torch.randint(0, n, (3 * n,), generator=gen),
                                                        torch.randint(0, num_rels, (3 * n,), generator=gen),
                                                        torch.randint(0, n, (3 * n,), generator=gen))}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,num_rels,seed', [(12, 4, 0), (9, 2, 1), (8, 1, 2), (3, 3, 3), (1, 2, 4)])
@pytest.mark.parametrize('exclude_self', [True, False])
def test_the_rule_equals_three_loops_per_relation(n, num_rels, seed, exclude_self):
    from gcn_vae_amd import transe
    dist = distances(n, num_rels, 4, seed, p=1 + seed % 2)
    if num_rels >= 3:
        dist[2] = NAN                                            # a relation with no candidate at all
    filt = random_filter(n, num_rels, seed + 100)
    orders = [None, list(range(num_rels))[::-1]] + ([[2, 0]] if num_rels >= 3 else [])
    for f in (None, filt):
        arrays = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filter_arrays(f, n, num_rels))) if f else {}
        for rels in orders:
            ids = list(range(num_rels)) if rels is None else rels
            for k in (1, 2, 5, 17, n * n + 7):                   # the last: K larger than any relation's candidates
                got = transe.complete_relations_from_distances(dist, k, relations=rels, exclude_self=exclude_self, **arrays)
                assert got[2].dtype == torch.float32 and got[0].dtype == got[1].dtype == torch.int64
                assert same(got, brute_force_distances(dist, ids, k, filt=f, exclude_self=exclude_self)), (rels, k)


def test_the_rule_on_a_hand_made_tensor():
    from gcn_vae_amd import transe
    dist = torch.tensor([[[0.0, -0.0, 1.0], [0.0, 0.0, NAN], [INF, 5.0, 0.0]],
                         [[0.0, 1.0, 1.0], [1.0, 0.0, 3.0], [NAN, 1.0, 0.0]],
                         [[NAN, NAN, NAN], [NAN, 2.0, NAN], [NAN, NAN, NAN]]])         # [r, s, o]; relation 2: only a loop
    subj, obj, d, info = transe.complete_relations_from_distances(dist, 4, relations=[1, 2, 0])
    assert subj.tolist() == [[0, 0, 1, 2], [-1, -1, -1, -1], [0, 1, 0, 2]]
    assert obj.tolist() == [[1, 2, 0, 1], [-1, -1, -1, -1], [1, 0, 2, 1]]
    assert d.tolist() == [[1.0, 1.0, 1.0, 1.0], [INF] * 4, [0.0, 0.0, 1.0, 5.0]]
    assert not bool(torch.signbit(d[2, :2]).any())                                       # a zero is reported as +0, ties by (s, o)
    assert info['count'].tolist() == [4, 0, 4]
    subj, obj, d, info = transe.complete_relations_from_distances(dist, 5, relations=[0])
    assert (subj.tolist(), obj.tolist(), d.tolist()[0][4]) == ([[0, 1, 0, 2, 2]], [[1, 0, 2, 1, 0]], INF)      # +inf is kept, and last
    assert info['count'].tolist() == [5]
    subj, obj, _, info = transe.complete_relations_from_distances(dist, 2, relations=[1])
    assert (subj.tolist(), obj.tolist(), info['count'].tolist()) == ([[0, 0]], [[1, 2]], [4])      # the tie block of the 2nd distance
    subj, obj, d, info = transe.complete_relations_from_distances(dist, 2, relations=[2, 1], exclude_self=False)
    assert (subj.tolist(), obj.tolist()) == ([[1, -1], [0, 1]], [[1, -1], [0, 1]]) and d[0].tolist() == [2.0, INF]
    assert info['count'].tolist() == [1, 3]                                              # the three loops at 0 tie at the 2nd place
    lo, hi, ent = filter_arrays({(0, 0, 1), (0, 1, 1)}, 3, 3)
    subj, obj, _, _ = transe.complete_relations_from_distances(dist, 1, filt_lo=lo, filt_hi=hi, filt_ent=ent)
    assert (subj.tolist(), obj.tolist()) == ([[1], [0], [-1]], [[0], [2], [-1]])


def test_the_typed_rule_and_its_masks():
    from gcn_vae_amd import transe
    n, num_rels = 10, 3
    dist = distances(n, num_rels, 4, 5, p=2)
    gen = torch.Generator().manual_seed(9)
    cs, co = torch.rand(num_rels, n, generator=gen) < 0.5, torch.rand(num_rels, n, generator=gen) < 0.6
    cs[1] = False                                                # an empty subject set: an all-padding row
    for k in (1, 4, 200):
        got = transe.complete_relations_from_distances(dist, k, relations=[2, 1, 0], cand_subj=cs, cand_obj=co)
        assert same(got, brute_force_distances(dist, [2, 1, 0], k, cand_subj=cs, cand_obj=co))
        assert got[0][1].tolist() == [-1] * k and got[2][1].tolist() == [INF] * k and int(got[3]['count'][1]) == 0
    with pytest.raises(ValueError, match='together'):
        transe.complete_relations_from_distances(dist, 1, cand_subj=cs)
    with pytest.raises(ValueError, match='cand_obj'):
        transe.complete_relations_from_distances(dist, 1, cand_subj=cs, cand_obj=co[:, :5])


def test_overflow_names_the_relation_and_says_at_or_below():
    from gcn_vae_amd import transe
    dist = distances(8, 3, 4, 11, special=False)
    dist[1] = 1.0                                                # 56 candidates on one value
    with pytest.raises(transe.MineOverflow) as err:
        transe.complete_relations_from_distances(dist, 3, max_results=3 * 55)
    assert err.value.count == 56 and 'relation 1' in str(err.value) and 'at or below the K-th distance' in str(err.value)
    got = transe.complete_relations_from_distances(dist, 3, max_results=3 * 56)
    assert got[3]['count'].tolist()[1] == 56 and got[0][1].tolist() == [0, 0, 0] and got[1][1].tolist() == [1, 2, 3]


# ---- the level walk ----------------------------------------------------------------------------------------------------------------
def host_keys(dist, exclude_self=True):
    """The ordered keys of -dist[r, s, o] as the kernels compute them, 0 for what is no candidate (NaN, s == o)."""
    v = -np.ascontiguousarray(dist.numpy(), dtype=np.float32) + np.float32(0.0)
    u = v.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    key[np.isnan(v)] = 0
    if exclude_self:
        key[:, np.arange(v.shape[1]), np.arange(v.shape[1])] = 0
    return key


class FakeSweep:
    """gv_transe_mine_by_relation on a materialised distance tensor, in numpy: one call is one sweep over the slots, the keys those of
    -d, a record's fourth word the bits of d.  ``log`` keeps what every sweep was asked."""

    def __init__(self, dist, exclude_self=True):
        self.dist, self.keys, self.log = dist, host_keys(dist, exclude_self), []

    def __call__(self, mode, rels32, key_min, prefix_bits, prefix, bin_bits, out, capacity, out_base, words):
        rels = rels32.numpy()
        self.log.append((mode, prefix_bits, bin_bits, rels.tolist()))
        n = self.keys.shape[1]
        for i, r in enumerate(rels):
            if r < 0:
                continue
            ks = self.keys[r].ravel()
            if mode == 1:
                ks = ks[ks != 0]
                if prefix_bits:
                    ks = ks[(ks >> (32 - prefix_bits)) == int(prefix.numpy().view(np.uint32)[i])]
                bins = (ks >> (32 - prefix_bits - bin_bits)) & ((1 << bin_bits) - 1)
                words[i << bin_bits:(i + 1) << bin_bits] += torch.from_numpy(np.bincount(bins, minlength=1 << bin_bits))
            else:
                at = np.nonzero((ks != 0) & (ks >= int(key_min.numpy().view(np.uint32)[i])))[0]
                words[i] = len(at)
                at = at[::-1]                                                    # arrival order is arbitrary
                b0, b1 = int(out_base[i]), int(out_base[i + 1])
                at = at[:max(0, min(b1, capacity) - b0)]
                bits = (self.dist[r].reshape(-1)[torch.from_numpy(at.copy())] + 0.0).view(torch.int32)
                out[b0:b0 + len(at)] = torch.stack([torch.from_numpy(at // n).int(), torch.full((len(at),), int(r)).int(),
                                                    torch.from_numpy(at % n).int(), bits], 1)


def walk(dist, rels, k, share, levels=None, **fake):
    from gcn_vae_amd import ops
    sweep = FakeSweep(dist, **fake)
    rels = torch.tensor(rels, dtype=torch.int64)
    got = ops._mine_drive_by_relation(sweep, torch.device('cpu'), dist.shape[1], rels, k, share, levels or ops.MINE_RELATION_LEVELS, 'fake',
                                      ascending=True)
    return got, sweep.log


@pytest.mark.parametrize('levels', ['by_relation', 'typed'])
def test_the_ascending_walk_finds_every_relations_own_threshold(levels):
    """Relations at scales 2^-6 .. 2^6: each one's K-th distance sits in its own first-level bin, the case ONE threshold for the
    whole graph gets wrong (it would fill the list from the shortest relation)."""
    from gcn_vae_amd import ops, transe
    levels = ops.MINE_RELATION_LEVELS if levels == 'by_relation' else ops.MINE_RELATION_TYPED_LEVELS
    dist = distances(12, 4, 4, 21, special=False) * torch.tensor([2.0 ** -6, 1.0, 2.0 ** 6, 2.0 ** 3]).view(4, 1, 1)
    dist[1, 4] = NAN
    dist[3, 2, 7] = INF
    for rels in ([0, 1, 2, 3], [3, 0, 2]):
        for k in (1, 10, 60, 500):
            for share in (k, 10 * k):
                (subj, obj, d, info), log = walk(dist, rels, k, share, levels)
                want = brute_force_distances(dist, rels, k)
                assert same((subj, obj, d, info), want), (rels, k, share)
                ref = transe.complete_relations_from_distances(dist, k, relations=rels, max_results=share * len(rels))
                assert same(ref, want)
                assert info['passes'] == len(log) <= len(levels) + 1 and [e[0] for e in log] == [1] * (len(log) - 1) + [0]
    firsts = {int(host_keys(dist)[r][host_keys(dist)[r] != 0].max()) >> 24 for r in range(4)}
    assert len(firsts) == 4                                      # the four nearest keys lie in four first-level bins


def test_slots_resolve_at_different_levels_and_sit_out_the_later_sweeps():
    n = 12
    dist = torch.zeros(3, n, n)
    dist[0] = 2.0 ** torch.arange(n * n, dtype=torch.float32).view(n, n).remainder(97.0)     # spread over many exponents
    dist[1] = 1.0 + torch.rand(n, n, generator=torch.Generator().manual_seed(3))            # all in one first-level bin
    dist[2] = NAN                                                                            # no candidate at all
    (subj, obj, d, info), log = walk(dist, [0, 1, 2], 5, 20)
    assert same((subj, obj, d, info), brute_force_distances(dist, [0, 1, 2], 5))
    hist = [e for e in log if e[0] == 1]
    assert hist[0][3] == [0, 1, 2] and len(hist) >= 2
    assert all(e[3][0] == -1 and e[3][1] == 1 and e[3][2] == -1 for e in hist[1:])      # 0 resolved at level 0, 2 is empty
    assert log[-1][0] == 0 and log[-1][3] == [0, 1, -1]                                  # the empty relation is not emitted
    assert subj[2].tolist() == [-1] * 5 and d[2].tolist() == [INF] * 5 and info['count'].tolist()[2] == 0
    (_, _, _, info), log = walk(dist, [0, 2], 5, 20)                                     # every relation resolved at level 0
    assert info['passes'] == 2 and [e[0] for e in log] == [1, 0]
    (subj, _, d, info), log = walk(dist, [2], 5, 20)                                     # nothing to emit at all
    assert subj.tolist() == [[-1] * 5] and d.tolist() == [[INF] * 5] and info['passes'] == 1 and info['count'].tolist() == [0]


def test_a_tie_larger_than_the_share_overflows_naming_the_relation():
    from gcn_vae_amd import ops
    dist = distances(9, 3, 4, 31, special=False)
    dist[2] = 0.25                                               # 72 candidates on one exact value
    sweep = FakeSweep(dist)
    with pytest.raises(ops.MineOverflow) as err:
        ops._mine_drive_by_relation(sweep, torch.device('cpu'), 9, torch.tensor([0, 2, 1]), 3, 71, ops.MINE_RELATION_LEVELS, 'fake',
                                    ascending=True)
    assert err.value.count == 72 and 'relation 2' in str(err.value) and 'at or below the K-th distance' in str(err.value)
    assert [e[0] for e in sweep.log] == [1, 1, 1, 1]             # a tie is only known at the last level; nothing was emitted
    got, log = walk(dist, [0, 2, 1], 3, 72)
    assert same(got, brute_force_distances(dist, [0, 2, 1], 3)) and got[3]['count'].tolist()[1] == 72


def test_the_default_descending_path_is_what_it_was():
    """``ascending`` left out: relation_select and the overflow text on one fixed case, the expected rows worked out by hand from
    the rule as it was before the keyword existed (logit descending, -0 as +0, then (s, o); padding -1 / -1 / -inf)."""
    from gcn_vae_amd import ops
    slot = torch.tensor([1, 0, 1, 1, 0, 1])
    s, o = torch.tensor([2, 0, 0, 1, 1, 0]), torch.tensor([0, 1, 2, 1, 0, 1])
    logits = torch.tensor([0.5, -0.0, 0.5, 2.0, 0.0, -1.0])
    subj, obj, best, count = ops.relation_select(slot, s, o, logits, torch.tensor([7, 3]), 2, 3, 10)
    assert subj.tolist() == [[0, 1], [1, 0]] and obj.tolist() == [[1, 0], [1, 2]]
    assert best.tolist() == [[0.0, 0.0], [2.0, 0.5]] and not bool(torch.signbit(best[0]).any()) and count.tolist() == [2, 3]
    subj, obj, best, count = ops.relation_select(slot, s, o, logits, torch.tensor([7, 3]), 5, 3, 10)
    assert best.tolist() == [[0.0, 0.0, -INF, -INF, -INF], [2.0, 0.5, 0.5, -1.0, -INF]] and subj[0].tolist() == [0, 1, -1, -1, -1]
    with pytest.raises(ops.MineOverflow) as err:
        ops.relation_select(slot, s, o, logits, torch.tensor([7, 3]), 2, 3, 2)
    assert 'relation 3' in str(err.value) and 'at or above the K-th logit' in str(err.value) and err.value.count == 3
    # the same candidates read as distances
    subj, obj, best, count = ops.relation_select(slot, s, o, logits, torch.tensor([7, 3]), 2, 3, 10, ascending=True)
    assert subj.tolist() == [[0, 1], [0, 0]] and obj.tolist() == [[1, 0], [1, 2]] and best.tolist() == [[0.0, 0.0], [-1.0, 0.5]]
    assert count.tolist() == [2, 3]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_bad_arguments_and_host_tensors():
    from gcn_vae_amd import ops, ranking, transe
    en, rn = torch.zeros(6, 3), torch.zeros(4, 3)
    tables = (en, rn, 1, False)
    dist = torch.zeros(4, 6, 6)
    for call in (lambda **kw: ops.transe_relation_topk(en, rn, kw.pop('k', 2), 1, **kw),
                 lambda **kw: transe.complete_relations(tables, kw.pop('k', 2), **kw),
                 lambda **kw: transe.complete_relations_unfused(tables, kw.pop('k', 2), **kw),
                 lambda **kw: transe.complete_relations_from_distances(dist, kw.pop('k', 2), **kw)):
        with pytest.raises(ValueError, match='repeated'):
            call(relations=[1, 3, 1])
        with pytest.raises(ValueError, match=r'\[0, 4\)'):
            call(relations=[0, 4])
        with pytest.raises(ValueError, match='at least one'):
            call(relations=[])
        with pytest.raises(TypeError):
            call(relations=[0.5])
        with pytest.raises(ValueError, match='k must be >= 1'):
            call(k=0)
        with pytest.raises(ValueError, match='max_results'):
            call(k=3, max_results=11)                            # 4 relations * 3
    for call in (lambda **kw: ops.transe_relation_topk(en, rn, 2, 1, **kw), lambda **kw: transe.complete_relations(tables, 2, **kw),
                 lambda **kw: transe.complete_relations_unfused(tables, 2, **kw)):
        with pytest.raises(RuntimeError, match='CUDA/ROCm'):
            call()
        with pytest.raises(RuntimeError, match='CUDA/ROCm'):
            call(relations=[2, 0])
    with pytest.raises(ValueError, match='width'):
        ops.transe_relation_topk(en, torch.zeros(4, 5), 2, 1)
    with pytest.raises(ValueError, match='together'):
        transe.complete_relations_from_distances(dist, 2, filt_lo=torch.zeros(24, dtype=torch.long))
    for call in (transe.complete_relations, transe.complete_relations_unfused):
        with pytest.raises(TypeError, match='type_constraint'):
            call(tables, 2, type_constraint=None)
        with pytest.raises(ValueError, match='FilterIndex'):
            call(tables, 2, filter_index=ranking.FilterIndex(5, 2, np.array([[0, 1, 2]])))
        with pytest.raises(ValueError, match='TypeConstraint'):
            call(tables, 2, type_constraint=ranking.TypeConstraint(5, 2, np.array([[0, 1, 2]])))
    tc = ranking.TypeConstraint(6, 4, np.array([[0, 1, 2], [3, 1, 4]]))
    set_ptr, set_ids = tc.members()
    with pytest.raises(RuntimeError, match='CUDA/ROCm'):
        ops.transe_relation_topk_typed(en, rn, 2, 1, set_ptr, set_ids)
    with pytest.raises(ValueError, match='2 R \\+ 1'):
        ops.transe_relation_topk_typed(en, rn, 2, 1, set_ptr[:-1], set_ids)


def test_the_typed_plan_takes_a_span_multiple():
    from gcn_vae_amd import ops
    sizes = torch.tensor([70, 0, 1300, 5, 65, 64, 1, 200])       # objects of r = 0..3, then subjects of r = 0..3
    set_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    rels = torch.tensor([2, 0, 1])
    assert torch.equal(ops.relation_typed_plan(set_ptr, 4, rels), ops.relation_typed_plan(set_ptr, 4, rels, multiple=1))
    units = ops.relation_typed_plan(set_ptr, 4, rels, multiple=4)
    of_two = units[units[:, 0] == 0]
    assert of_two[:, 2].tolist() == [0, 4, 8, 12, 16, 20] and of_two[:, 3].tolist() == [4, 8, 12, 16, 20, 21]      # 21 object tiles in fours
    assert set(units[:, 0].tolist()) == {0, 1}


def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entries_are_exported_and_check_their_arguments():
    """Both entries validate on the host before any launch (this runs without a GPU); every message names the entry."""
    from gcn_vae_amd import lib
    l = lib.load()
    handle = ctypes.CDLL(lib.LIB_PATH)
    header = open(os.path.join(_root(), 'include', 'gcnvae.h')).read()
    integration = open(os.path.join(_root(), 'INTEGRATION.md')).read()
    one = ctypes.c_void_p(16)            # a non-NULL address that is never dereferenced: every call below fails before a launch

    def untyped(en=one, rn=one, n=100, num_rels=3, dim=8, p=1, lo=None, hi=None, ent=None, n_ent=0, mode=0, rels=one, m=3, key_min=one,
                prefix_bits=0, prefix=one, bin_bits=8, out=one, capacity=10, out_base=one, counter=one, hist=one, ws=None, ws_bytes=0):
        return l.gv_transe_mine_by_relation(en, rn, n, num_rels, dim, p, lo, hi, ent, n_ent, 1, mode, rels, m, key_min, prefix_bits,
                                            prefix, bin_bits, out, capacity, out_base, counter, hist, ws, ws_bytes, None)

    def typed(en=one, rn=one, n=100, num_rels=3, dim=8, p=1, lo=None, hi=None, ent=None, n_ent=0, mode=0, rels=one, m=3, key_min=one,
              prefix_bits=0, prefix=one, bin_bits=8, out=one, capacity=10, out_base=one, counter=one, hist=one, units=one, n_units=5):
        return l.gv_transe_mine_typed_by_relation(en, rn, n, num_rels, dim, p, one, one, units, n_units, lo, hi, ent, n_ent, 1, mode,
                                                  rels, m, key_min, prefix_bits, prefix, bin_bits, out, capacity, out_base, counter,
                                                  hist, None)

    for name, call in (('gv_transe_mine_by_relation', untyped), ('gv_transe_mine_typed_by_relation', typed)):
        assert hasattr(handle, name) and f'int {name}(' in header and name in lib.SIGNATURES and f'`{name}`' in integration

        def refused(what, **kw):
            assert call(**kw) != 0, kw
            assert what in lib.last_error() and name + ':' in lib.last_error(), (kw, lib.last_error())
        refused('NULL', en=None)
        refused('NULL', rn=None)
        refused('NULL', rels=None)
        refused('NULL', key_min=None)
        refused('NULL', out_base=None)
        refused('NULL', counter=None)
        refused('NULL', out=None)
        refused('NULL', mode=1, hist=None)
        refused('NULL', mode=1, prefix_bits=8, prefix=None)
        assert call(mode=1, prefix=None, n=0, en=None, rn=None) == 0                    # level 0 reads no prefix; no entity: nothing to do
        refused('aligned', out=ctypes.c_void_p(8))
        refused('m=0', m=0)
        refused('m=4', m=4)                                                             # more slots than relations
        refused('mode', mode=2)
        refused('capacity', capacity=-1)
        refused('dim=0', dim=0)
        refused('dim=513', dim=513)
        refused('p_norm=3', p=3)
        refused('2^31', n=2 ** 20, num_rels=2 ** 11, m=1)
        refused('filt', lo=one)
        refused('histogram words', mode=1, m=2 ** 17, num_rels=2 ** 17, n=10, bin_bits=8)
        assert call(n=0, en=None, rn=None, out=None, counter=None, rels=None, key_min=None, out_base=None) == 0
    assert untyped(mode=1, bin_bits=9) != 0 and 'bin_bits=9 above 8' in lib.last_error()            # the 256-bin LDS histograms
    assert typed(mode=1, bin_bits=13) != 0 and 'bin_bits' in lib.last_error()
    assert untyped(lo=one, hi=one, ent=one, n_ent=5) != 0 and 'workspace' in lib.last_error()
    assert untyped(lo=one, hi=one, ent=one, n_ent=5, ws=ctypes.c_void_p(24), ws_bytes=1 << 20) != 0 and 'aligned' in lib.last_error()
    assert typed(units=ctypes.c_void_p(8)) != 0 and 'aligned' in lib.last_error()
    assert typed(n_units=-1) != 0 and 'n_units' in lib.last_error()


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_the_flags_parse_and_are_refused_in_combination(tmp_path):
    from gcn_vae_amd import transe
    p = transe.build_parser()
    a = p.parse_args(['-d', 'x', '--relation-profile-topk', '50', '--relation-profile-ids', '5,0,2', '--relation-profile-out', 'r.tsv',
                      '--relation-profile-typed'])
    assert (a.relation_profile_topk, a.relation_profile_ids, a.relation_profile_out, a.relation_profile_typed) == (50, '5,0,2', 'r.tsv', True)
    transe.check_args(a)
    d = p.parse_args(['-d', 'x'])
    assert (d.relation_profile_topk, d.relation_profile_ids, d.relation_profile_out, d.relation_profile_typed) == (None, None, None, False)
    assert transe.RELATION_PROFILE_OUT == 'transe_relation_profiles.tsv' and 'transe_relation_profiles.tsv' in p.format_help()
    assert d.profile_topk == 0 and d.complete_topk is None and d.complete_typed is False      # the existing flags as they were
    transe.check_args(d)
    base = ['-d', 'x']
    with pytest.raises(ValueError, match='--relation-profile-typed.*needs --relation-profile-topk'):
        transe.check_args(p.parse_args(base + ['--relation-profile-typed']))
    with pytest.raises(ValueError, match='--relation-profile-ids.*needs --relation-profile-topk'):
        transe.check_args(p.parse_args(base + ['--relation-profile-ids', '1']))
    with pytest.raises(ValueError, match='--relation-profile-out.*needs --relation-profile-topk'):
        transe.check_args(p.parse_args(base + ['--relation-profile-out', 'r.tsv']))
    for k in ('0', '-1'):
        with pytest.raises(ValueError, match='--relation-profile-topk.*>= 1'):
            transe.check_args(p.parse_args(base + ['--relation-profile-topk', k]))
    for bad, what in (('1,x', 'comma-separated'), ('1,-2', 'outside'), ('3,1,3', 'twice'), (',', 'names no relation')):
        with pytest.raises(ValueError, match=what):                                          # before anything is loaded
            transe.check_args(p.parse_args(base + ['--relation-profile-topk', '5', '--relation-profile-ids', bad]))
    listed = tmp_path / 'rels.txt'
    listed.write_text('3\n\n1\n')
    transe.check_args(p.parse_args(base + ['--relation-profile-topk', '5', '--relation-profile-ids', str(listed)]))
