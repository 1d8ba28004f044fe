"""Per-relation completion, the parts that need no GPU: the rule (ranking.complete_relations_from_scores against three Python loops
per relation), the per-relation level walk of ops._mine_drive_by_relation driven by a fake launch that histograms a materialised
key array in numpy, the argument checks of the wrappers and of gv_mine_scores_by_relation / gv_mine_scores_typed_by_relation
(nothing is launched), and the command-line surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mine_cases import filter_arrays
from relation_profile_cases import brute_force, same

NAN, INF = float('nan'), float('inf')


def scores(n, num_rels, h, seed, special=True):
    gen = torch.Generator().manual_seed(seed)
    emb = torch.randn(n, h, generator=gen)
    w = torch.randn(num_rels, h, generator=gen)
    if special and n >= 8:
        emb[5] = emb[2]                      # exact ties, across and within subjects
        emb[6] = emb[2]
        emb[3] = 0.0                         # +0 / -0 logits
        emb[4] = NAN                         # a NaN row (and column)
        emb[7] = 0.0
        emb[7, 0] = INF                      # +-inf logits, NaN against the zero row
    return torch.einsum('sd,rd,od->rso', emb, w, emb)


def random_filter(n, num_rels, seed):
    gen = torch.Generator().manual_seed(seed)
    return {(int(a), int(b), int(c)) for a, b, c in zip(torch.randint(0, n, (3 * n,), generator=gen),
                                                        torch.randint(0, num_rels, (3 * n,), generator=gen),
                                                        torch.randint(0, n, (3 * n,), generator=gen))}


@pytest.mark.parametrize('n,num_rels,seed', [(12, 4, 0), (9, 2, 1), (8, 1, 2), (3, 3, 3), (1, 2, 4)])
@pytest.mark.parametrize('exclude_self', [True, False])
def test_the_rule_equals_three_loops_per_relation(n, num_rels, seed, exclude_self):
    from gcn_vae_amd import ranking
    score = scores(n, num_rels, 4, seed)
    if num_rels >= 3:
        score[2] = NAN                                           # a relation with no candidate at all
    filt = random_filter(n, num_rels, seed + 100)
    orders = [None, list(range(num_rels))[::-1]] + ([[2, 0]] if num_rels >= 3 else [])
    for f in (None, filt):
        arrays = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filter_arrays(f, n, num_rels))) if f else {}
        for rels in orders:
            ids = list(range(num_rels)) if rels is None else rels
            for k in (1, 2, 5, 17, n * n + 7):                   # the last: K larger than any relation's candidates
                got = ranking.complete_relations_from_scores(score, k, relations=rels, exclude_self=exclude_self, **arrays)
                assert same(got, brute_force(score, ids, k, filt=f, exclude_self=exclude_self)), (rels, k)


def test_the_rule_on_a_hand_made_tensor():
    from gcn_vae_amd import ranking
    score = torch.tensor([[[9.0, -0.0, 1.0], [0.0, 9.0, NAN], [INF, -INF, 9.0]],
                          [[9.0, 1.0, 1.0], [1.0, 9.0, 0.0], [NAN, 1.0, 9.0]],
                          [[NAN, NAN, NAN], [NAN, 2.0, NAN], [NAN, NAN, NAN]]])        # [r, s, o]; relation 2: only a loop
    subj, obj, logits, info = ranking.complete_relations_from_scores(score, 4, relations=[1, 2, 0])
    assert subj.tolist() == [[0, 0, 1, 2], [-1, -1, -1, -1], [2, 0, 0, 1]]
    assert obj.tolist() == [[1, 2, 0, 1], [-1, -1, -1, -1], [0, 2, 1, 0]]
    assert logits.tolist() == [[1.0, 1.0, 1.0, 1.0], [-INF] * 4, [INF, 1.0, 0.0, 0.0]]
    assert not bool(torch.signbit(logits[2, 2:]).any())                                  # -0 is reported as +0, and ties by (s, o)
    assert info['count'].tolist() == [4, 0, 4]
    subj, obj, _, info = ranking.complete_relations_from_scores(score, 2, relations=[1])
    assert (subj.tolist(), obj.tolist(), info['count'].tolist()) == ([[0, 0]], [[1, 2]], [4])      # the tie block of the 2nd logit
    subj, obj, logits, info = ranking.complete_relations_from_scores(score, 2, relations=[2, 0], exclude_self=False)
    assert (subj.tolist(), obj.tolist()) == ([[1, -1], [2, 0]], [[1, -1], [0, 0]]) and logits[0].tolist() == [2.0, -INF]
    assert info['count'].tolist() == [1, 4]                                              # the three 9.0 tie at the 2nd place
    lo, hi, ent = filter_arrays({(2, 0, 0), (0, 1, 1)}, 3, 3)
    subj, obj, _, _ = ranking.complete_relations_from_scores(score, 1, filt_lo=lo, filt_hi=hi, filt_ent=ent)
    assert (subj.tolist(), obj.tolist()) == ([[0], [0], [-1]], [[2], [2], [-1]])


def test_the_typed_rule_and_its_masks():
    from gcn_vae_amd import ranking
    n, num_rels = 10, 3
    score = scores(n, num_rels, 4, 5)
    gen = torch.Generator().manual_seed(9)
    cs, co = torch.rand(num_rels, n, generator=gen) < 0.5, torch.rand(num_rels, n, generator=gen) < 0.6
    cs[1] = False                                                # an empty subject set: an all-padding row
    for k in (1, 4, 200):
        got = ranking.complete_relations_from_scores(score, k, relations=[2, 1, 0], cand_subj=cs, cand_obj=co)
        assert same(got, brute_force(score, [2, 1, 0], k, cand_subj=cs, cand_obj=co))
        assert got[0][1].tolist() == [-1] * k and int(got[3]['count'][1]) == 0
    with pytest.raises(ValueError, match='together'):
        ranking.complete_relations_from_scores(score, 1, cand_subj=cs)
    with pytest.raises(ValueError, match='cand_obj'):
        ranking.complete_relations_from_scores(score, 1, cand_subj=cs, cand_obj=co[:, :5])


def test_overflow_names_the_relation_and_carries_its_count():
    from gcn_vae_amd import ranking
    score = scores(8, 3, 4, 11, special=False)
    score[1] = 1.0                                               # 56 candidates on one value
    with pytest.raises(ranking.MineOverflow) as err:
        ranking.complete_relations_from_scores(score, 3, max_results=3 * 55)
    assert err.value.count == 56 and 'relation 1' in str(err.value) and '56' in str(err.value)
    got = ranking.complete_relations_from_scores(score, 3, max_results=3 * 56)
    assert got[3]['count'].tolist()[1] == 56 and got[0][1].tolist() == [0, 0, 0] and got[1][1].tolist() == [1, 2, 3]
    ranking.complete_relations_from_scores(score, 3, relations=[0, 2], max_results=8)      # the others fit (symmetric scores tie in pairs)


# ---- the level walk ----------------------------------------------------------------------------------------------------------------
def host_keys(val, exclude_self=True):
    """The ordered keys of val[r, s, o] as the kernels compute them, 0 for what is no candidate (NaN, s == o)."""
    v = np.ascontiguousarray(val.numpy(), dtype=np.float32) + np.float32(0.0)
    u = v.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    key[np.isnan(v)] = 0
    if exclude_self:
        key[:, np.arange(v.shape[1]), np.arange(v.shape[1])] = 0
    return key


class FakeSweep:
    """gv_mine_scores_by_relation on a materialised key array, in numpy: one call is one sweep over the slots.  ``log`` keeps what
    every sweep was asked; ``lose`` drops that many records of slot 0 in the emission (a miscounting kernel)."""

    def __init__(self, val, exclude_self=True, lose=0):
        self.val, self.keys, self.log, self.lose = val, host_keys(val, exclude_self), [], lose

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
                at = at[::-1][self.lose if i == 0 else 0:]                       # arrival order is arbitrary
                b0, b1 = int(out_base[i]), int(out_base[i + 1])
                at = at[:max(0, min(b1, capacity) - b0)]
                logits = (self.val[r].reshape(-1)[torch.from_numpy(at.copy())] + 0.0).view(torch.int32)
                out[b0:b0 + len(at)] = torch.stack([torch.from_numpy(at // n).int(), torch.full((len(at),), int(r)).int(),
                                                    torch.from_numpy(at % n).int(), logits], 1)


def walk(val, rels, k, share, levels=None, **fake):
    from gcn_vae_amd import ops
    sweep = FakeSweep(val, **fake)
    rels = torch.tensor(rels, dtype=torch.int64)
    got = ops._mine_drive_by_relation(sweep, torch.device('cpu'), val.shape[1], rels, k, share, levels or ops.MINE_RELATION_LEVELS, 'fake')
    return got, sweep.log


def test_the_level_layouts_cover_the_key():
    from gcn_vae_amd import ops
    for levels in (ops.MINE_RELATION_LEVELS, ops.MINE_RELATION_TYPED_LEVELS):
        assert sum(b for _, b in levels) == 32 and [p for p, _ in levels] == list(np.cumsum([0] + [b for _, b in levels[:-1]]))
    assert max(b for _, b in ops.MINE_RELATION_LEVELS) == 8 and ops.MINE_RELATION_TYPED_LEVELS == ops.MINE_LEVELS


@pytest.mark.parametrize('levels', ['by_relation', 'typed'])
def test_the_walk_finds_every_relations_own_threshold(levels):
    """w rows scaled by 2^-10 .. 2^10: each relation's K-th key sits in its own first-level bin, the case ONE threshold for the
    whole graph gets wrong (it would fill the list from the relation of largest scale)."""
    from gcn_vae_amd import ops, ranking
    levels = ops.MINE_RELATION_LEVELS if levels == 'by_relation' else ops.MINE_RELATION_TYPED_LEVELS
    val = scores(12, 4, 4, 21, special=False) * torch.tensor([2.0 ** -10, 1.0, 2.0 ** 10, -2.0 ** 5]).view(4, 1, 1)
    val[3] = -val[3].abs()                                       # a relation with only negative logits
    val[1, 4] = NAN
    for rels in ([0, 1, 2, 3], [3, 0, 2]):
        for k in (1, 10, 60, 500):
            for share in (k + 1, 10 * k):                        # (a symmetric score ties (s, o) with (o, s): K + 1 at the K-th)
                (subj, obj, logits, info), log = walk(val, rels, k, share, levels)
                want = brute_force(val, rels, k)
                assert same((subj, obj, logits, info), want), (rels, k, share)
                ref = ranking.complete_relations_from_scores(val, k, relations=rels, max_results=share * len(rels))
                assert same(ref, want)
                assert info['passes'] == len(log) <= len(levels) + 1 and [e[0] for e in log] == [1] * (len(log) - 1) + [0]
    firsts = {int(host_keys(val)[r][host_keys(val)[r] != 0].max()) >> 24 for r in range(4)}
    assert len(firsts) == 4                                      # the four best keys lie in four first-level bins


def test_a_resolved_relation_sits_out_the_later_sweeps():
    n = 12
    val = torch.zeros(3, n, n)
    val[0] = 2.0 ** torch.arange(n * n, dtype=torch.float32).view(n, n).remainder(97.0)      # spread over many exponents
    val[1] = 1.0 + torch.rand(n, n, generator=torch.Generator().manual_seed(3))             # all in one first-level bin
    val[2] = NAN                                                                             # no candidate at all
    (subj, obj, logits, info), log = walk(val, [0, 1, 2], 5, 20)
    assert same((subj, obj, logits, info), brute_force(val, [0, 1, 2], 5))
    hist = [e for e in log if e[0] == 1]
    assert hist[0][3] == [0, 1, 2] and len(hist) >= 2
    assert all(e[3][0] == -1 and e[3][1] == 1 and e[3][2] == -1 for e in hist[1:])      # 0 resolved at level 0, 2 is empty
    assert log[-1][0] == 0 and log[-1][3] == [0, 1, -1]                                  # the empty relation is not emitted
    assert subj[2].tolist() == [-1] * 5 and info['count'].tolist()[2] == 0
    # every relation resolved at level 0: one histogram sweep, one emission
    (_, _, _, info), log = walk(val, [0, 2], 5, 20)
    assert info['passes'] == 2 and [e[0] for e in log] == [1, 0]
    # nothing to emit at all
    (subj, _, logits, info), log = walk(val, [2], 5, 20)
    assert subj.tolist() == [[-1] * 5] and logits.tolist() == [[-INF] * 5] and info['passes'] == 1 and info['count'].tolist() == [0]


def test_a_tie_larger_than_the_share_overflows_naming_the_relation():
    from gcn_vae_amd import ops
    val = scores(9, 3, 4, 31, special=False)
    val[2] = 0.25                                                # 72 candidates on one exact value
    sweep = FakeSweep(val)
    with pytest.raises(ops.MineOverflow) as err:
        ops._mine_drive_by_relation(sweep, torch.device('cpu'), 9, torch.tensor([0, 2, 1]), 3, 71, ops.MINE_RELATION_LEVELS, 'fake')
    assert err.value.count == 72 and 'relation 2' in str(err.value)
    assert [e[0] for e in sweep.log] == [1, 1, 1, 1]             # a tie is only known at the last level; nothing was emitted
    assert all(e[3] == [-1, 2, -1] for e in sweep.log[1:])       # the other two had resolved at level 0
    got, log = walk(val, [0, 2, 1], 3, 72)
    assert same(got, brute_force(val, [0, 2, 1], 3)) and got[3]['count'].tolist()[1] == 72


def test_the_emission_is_checked_against_the_histograms():
    val = scores(9, 2, 4, 41, special=False)
    with pytest.raises(RuntimeError, match='relation 1.*emission pass found'):
        # the counter says fewer than the histograms counted
        from gcn_vae_amd import ops

        class Short(FakeSweep):
            def __call__(self, mode, *a):
                super().__call__(mode, *a)
                if mode == 0:
                    a[-1][0] -= 1
        sweep = Short(val)
        ops._mine_drive_by_relation(sweep, torch.device('cpu'), 9, torch.tensor([1, 0]), 4, 8, ops.MINE_RELATION_LEVELS, 'fake')


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_bad_arguments_and_host_tensors():
    from gcn_vae_amd import ops, ranking
    emb, w = torch.zeros(6, 3), torch.zeros(4, 3)
    score = torch.zeros(4, 6, 6)
    for call in (lambda **kw: ops.relation_topk_scores(emb, w, kw.pop('k', 2), **kw),
                 lambda **kw: ranking.complete_relations(emb, w, kw.pop('k', 2), **kw),
                 lambda **kw: ranking.complete_relations_unfused(emb, w, kw.pop('k', 2), **kw),
                 lambda **kw: ranking.complete_relations_from_scores(score, kw.pop('k', 2), **kw)):
        with pytest.raises(ValueError, match='repeated'):
            call(relations=[1, 3, 1])
        with pytest.raises(ValueError, match=r'\[0, 4\)'):
            call(relations=[0, 4])
        with pytest.raises(ValueError, match=r'\[0, 4\)'):
            call(relations=torch.tensor([-1, 2]))
        with pytest.raises(ValueError, match='at least one'):
            call(relations=[])
        with pytest.raises(TypeError):
            call(relations=[0.5])
        with pytest.raises(ValueError, match='k must be >= 1'):
            call(k=0)
        with pytest.raises(ValueError, match='max_results'):
            call(k=3, max_results=11)                            # 4 relations * 3
        with pytest.raises(ValueError, match='max_results'):
            call(max_results=0)
    for call in (ops.relation_topk_scores, ranking.complete_relations, ranking.complete_relations_unfused):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call(emb, w, 2)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call(emb, w, 2, relations=[2, 0])
    with pytest.raises(ValueError, match='width'):
        ops.relation_topk_scores(emb, torch.zeros(4, 5), 2)
    with pytest.raises(ValueError, match='together'):
        ops.relation_topk_scores(emb, w, 2, filt_lo=torch.zeros(24, dtype=torch.long))
    for call in (ranking.complete_relations, ranking.complete_relations_unfused):
        with pytest.raises(TypeError, match='type_constraint'):
            call(emb, w, 2, type_constraint=None)
        with pytest.raises(ValueError, match='FilterIndex'):
            call(emb, w, 2, filter_index=ranking.FilterIndex(5, 2, np.array([[0, 1, 2]])))
        with pytest.raises(ValueError, match='TypeConstraint'):
            call(emb, w, 2, type_constraint=ranking.TypeConstraint(5, 2, np.array([[0, 1, 2]])))
    tc = ranking.TypeConstraint(6, 4, np.array([[0, 1, 2], [3, 1, 4]]))
    set_ptr, set_ids = tc.members()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.relation_topk_scores_typed(emb, w, 2, set_ptr, set_ids)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.complete_relations(emb, w, 2, type_constraint=tc)
    with pytest.raises(ValueError, match='2 R \\+ 1'):
        ops.relation_topk_scores_typed(emb, w, 2, set_ptr[:-1], set_ids)
    assert ops.relation_ids_check(None, 3).tolist() == [0, 1, 2] and ops.relation_ids_check([2, 0], 3).tolist() == [2, 0]


def test_the_typed_plan_holds_the_chosen_relations_units_by_slot():
    from gcn_vae_amd import ops
    sizes = torch.tensor([70, 0, 130, 5, 65, 64, 1, 200])        # objects of r = 0..3, then subjects of r = 0..3
    set_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    rels = torch.tensor([2, 0, 1])
    for span in (None, 1, 2, 100):
        units = ops.relation_typed_plan(set_ptr, 4, rels, span)
        full = ops.mine_typed_plan(set_ptr, 4, span)
        assert units.dtype == torch.int32 and units.shape[1] == 4
        for slot, r in enumerate(rels.tolist()):
            mine = units[units[:, 0] == slot][:, 1:]
            pairs = {(int(u[0]), o) for u in mine for o in range(int(u[1]), int(u[2]))}
            want = {(int(u[1]), o) for u in full[full[:, 0] == r] for o in range(int(u[2]), int(u[3]))}
            assert pairs == want and len(pairs) == sum(int(u[2] - u[1]) for u in mine)      # every tile pair exactly once
        assert set(units[:, 0].tolist()) == {0, 1}               # relation 1 (slot 2) has no object: no unit; relation 3 is not asked


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gcnvae.h')).read()


def test_the_entries_are_exported_and_check_their_arguments():
    """Both entries validate on the host before any launch (this runs without a GPU); every message names the entry."""
    from gcn_vae_amd import lib
    l = lib.load()
    handle, header = ctypes.CDLL(lib.LIB_PATH), _header()
    one = ctypes.c_void_p(16)            # a non-NULL address that is never dereferenced: every call below fails before a launch
    integration = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'INTEGRATION.md')).read()

    def untyped(e=one, ld_e=8, w=one, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, mode=0, rels=one, m=3, key_min=one, prefix_bits=0,
                prefix=one, bin_bits=8, out=one, capacity=10, out_base=one, counter=one, hist=one, ws=None, ws_bytes=0, n=100,
                num_rels=3, h=8):
        return l.gv_mine_scores_by_relation(e, ld_e, w, ld_w, None, lo, hi, ent, n_ent, 1, mode, rels, m, key_min, prefix_bits, prefix,
                                            bin_bits, out, capacity, out_base, counter, hist, ws, ws_bytes, n, num_rels, h, None)

    def typed(e=one, ld_e=8, w=one, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, mode=0, rels=one, m=3, key_min=one, prefix_bits=0,
              prefix=one, bin_bits=8, out=one, capacity=10, out_base=one, counter=one, hist=one, n=100, num_rels=3, h=8, units=one,
              n_units=5, ws=None, ws_bytes=0):
        return l.gv_mine_scores_typed_by_relation(e, ld_e, w, ld_w, None, one, one, units, n_units, lo, hi, ent, n_ent, 1, mode, rels, m,
                                                  key_min, prefix_bits, prefix, bin_bits, out, capacity, out_base, counter, hist, n,
                                                  num_rels, h, None)

    for name, call in (('gv_mine_scores_by_relation', untyped), ('gv_mine_scores_typed_by_relation', typed)):
        assert hasattr(handle, name) and f'int {name}(' in header and name in lib.SIGNATURES and f'`{name}`' in integration

        def refused(what, **kw):
            assert call(**kw) != 0, kw
            assert what in lib.last_error() and name + ':' in lib.last_error(), (kw, lib.last_error())
        refused('NULL', e=None)
        refused('NULL', w=None)
        refused('NULL', rels=None)
        refused('NULL', key_min=None)
        refused('NULL', out_base=None)
        refused('NULL', counter=None)
        refused('NULL', out=None)
        refused('NULL', mode=1, hist=None)
        refused('NULL', mode=1, prefix_bits=8, prefix=None)
        assert call(mode=1, prefix=None, n=0, e=None, w=None) == 0                      # level 0 reads no prefix; no entity: nothing to do
        refused('aligned', out=ctypes.c_void_p(8))
        refused('m=0', m=0)
        refused('m=4', m=4)                                                             # more slots than relations
        refused('mode', mode=2)
        refused('capacity', capacity=-1)
        refused('leading dimension', ld_e=7)
        refused('2^31', n=2 ** 20, num_rels=2 ** 11, m=1)
        refused('filt', lo=one)
        refused('histogram words', mode=1, m=2 ** 17, num_rels=2 ** 17, n=10, bin_bits=8)
        assert call(n=0, e=None, w=None, out=None, counter=None, rels=None, key_min=None, out_base=None) == 0
    assert untyped(mode=1, bin_bits=9) != 0 and 'bin_bits=9 above 8' in lib.last_error()            # the 256-bin LDS histogram
    assert typed(mode=1, bin_bits=13) != 0 and 'bin_bits' in lib.last_error()
    assert untyped(lo=one, hi=one, ent=one, n_ent=5) != 0 and 'workspace' in lib.last_error()
    assert untyped(lo=one, hi=one, ent=one, n_ent=5, ws=ctypes.c_void_p(24), ws_bytes=1 << 20) != 0 and 'aligned' in lib.last_error()
    assert typed(units=ctypes.c_void_p(8)) != 0 and 'aligned' in lib.last_error()
    assert typed(n_units=-1) != 0 and 'n_units' in lib.last_error()


# ---- the command line -------------------------------------------------------------------------------------------------------------
def test_the_flags_parse_and_are_refused_in_combination(tmp_path):
    from gcn_vae_amd import train
    p = train.build_parser()
    a = p.parse_args(['-d', 'x', '--test-mode', 'True', '--relation-profile-topk', '50', '--relation-profile-ids', '5,0,2',
                      '--relation-profile-out', 'r.tsv', '--relation-profile-typed'])
    assert (a.relation_profile_topk, a.relation_profile_ids, a.relation_profile_out, a.relation_profile_typed) == (50, '5,0,2', 'r.tsv', True)
    train.check_args(a)
    d = p.parse_args(['-d', 'x'])
    assert (d.relation_profile_topk, d.relation_profile_ids, d.relation_profile_out, d.relation_profile_typed) == \
        (0, None, 'relation_profiles.tsv', False)
    assert d.profile_topk == 0 and d.complete_topk == 0 and d.complete_typed is False      # the existing flags as they were
    train.check_args(d)
    with pytest.raises(ValueError, match='--test-mode'):
        train.main(p.parse_args(['-d', 'synthetic:30:3:100:10:10:0', '--relation-profile-topk', '5']))
    base = ['-d', 'x', '--test-mode', 'True']
    with pytest.raises(ValueError, match='--relation-profile-typed.*needs --relation-profile-topk'):
        train.check_args(p.parse_args(base + ['--relation-profile-typed']))
    with pytest.raises(ValueError, match='--relation-profile-ids.*needs --relation-profile-topk'):
        train.check_args(p.parse_args(base + ['--relation-profile-ids', '1']))
    with pytest.raises(ValueError, match='--relation-profile-topk'):
        train.check_args(p.parse_args(base + ['--relation-profile-topk', '-1']))
    for bad, what in (('1,x', 'comma-separated'), ('1,-2', 'outside'), ('3,1,3', 'twice'), (',', 'names no relation')):
        with pytest.raises(ValueError, match=what):                                          # before anything is loaded
            train.check_args(p.parse_args(base + ['--relation-profile-topk', '5', '--relation-profile-ids', bad]))
    # an id past the dataset's relations: refused once the data is read, before the model is built or the GPU is asked for
    with pytest.raises(ValueError, match=r'relation 7 lies outside \[0, 3\)'):
        train.main(p.parse_args(['-d', 'synthetic:30:3:100:10:10:0', '--test-mode', 'True', '--relation-profile-topk', '5',
                                 '--relation-profile-ids', '1,7']))
    assert train.relation_profile_ids_arg(None) is None and train.relation_profile_ids_arg(None, 3) == [0, 1, 2]
    assert train.relation_profile_ids_arg(' 4, 0 ,2', 5) == [4, 0, 2]                        # the order asked
    listed = tmp_path / 'rels.txt'
    listed.write_text('3\n\n1\n')
    assert train.relation_profile_ids_arg(str(listed), 4) == [3, 1]
    with pytest.raises(ValueError, match=r'\[0, 3\)'):
        train.relation_profile_ids_arg(str(listed), 3)
