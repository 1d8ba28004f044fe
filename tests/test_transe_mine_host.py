"""Whole-graph TransE mining, the parts that need no GPU: the rule itself (transe.mine_from_distances against a triple Python
loop), the argument checks of gv_transe_mine (nothing is launched), and the command-line surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mine_cases import brute_force, filter_arrays, same


def distances(n, num_rels, seed):
    """L1 distances of a small table with what the rule has to get right: exact ties (duplicated rows, and values on a coarse
    grid), zeros, a NaN row and column, +inf entries."""
    gen = torch.Generator().manual_seed(seed)
    ent = torch.randint(-3, 4, (n, 3), generator=gen).float() * 0.5
    rel = torch.randint(-1, 2, (num_rels, 3), generator=gen).float() * 0.5
    rel[0] = 0.0                                # relation 0: d[s, 0, s] = 0, d symmetric
    if n >= 8:
        ent[5] = ent[2]
        ent[6] = ent[2]                         # zeros off the diagonal, ties everywhere
        ent[4] = float('nan')
        ent[7, 0] = float('inf')                # +inf against every other row, NaN (inf - inf) against itself
    q = ent[None, :, None, :] + rel[:, None, None, :]
    return (q - ent[None, None, :, :]).abs().sum(-1)


@pytest.mark.parametrize('n,num_rels,seed', [(9, 2, 0), (12, 3, 1), (8, 1, 2), (3, 3, 3), (1, 2, 4)])
@pytest.mark.parametrize('exclude_self', [True, False])
def test_mine_from_distances_equals_the_triple_loop(n, num_rels, seed, exclude_self):
    from gcn_vae_amd import transe
    dist = distances(n, num_rels, seed)
    if n >= 8:
        assert bool(torch.isnan(dist).any()) and bool(torch.isinf(dist).any()) and int((dist == 0).sum()) > n
    gen = torch.Generator().manual_seed(seed + 100)
    filt = {(int(a), int(b), int(c)) for a, b, c in zip(torch.randint(0, n, (2 * n,), generator=gen),
                                                        torch.randint(0, num_rels, (2 * n,), generator=gen),
                                                        torch.randint(0, n, (2 * n,), generator=gen))}
    for f in (None, filt):
        arrays = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filter_arrays(f, n, num_rels))) if f else {}
        total = brute_force(dist, True, k=10 ** 9, filt=f, exclude_self=exclude_self)[2]
        for k in (1, 2, 5, 17, max(total, 1), total + 7):          # the last: K larger than the number of candidates
            got = transe.mine_from_distances(dist, k=k, exclude_self=exclude_self, **arrays)
            assert same(got, brute_force(dist, True, k=k, filt=f, exclude_self=exclude_self)), k
        for t in (float('inf'), 0.0, -0.0, -1.0, 1.5, 2.0, 3.25):
            got = transe.mine_from_distances(dist, threshold=t, exclude_self=exclude_self, **arrays)
            assert same(got, brute_force(dist, True, threshold=t, filt=f, exclude_self=exclude_self)), t
        assert transe.mine_from_distances(dist, threshold=-1.0, exclude_self=exclude_self, **arrays)[0].shape == (0, 3)
        everything = transe.mine_from_distances(dist, threshold=float('inf'), exclude_self=exclude_self, **arrays)
        assert everything[0].shape[0] == total and not bool(torch.isnan(everything[1]).any())      # all but NaN, +inf included
        if n >= 8 and total:
            assert bool(torch.isinf(everything[1][-1]))                                            # ... and last


def test_the_rule_on_a_hand_made_tensor():
    from gcn_vae_amd import transe
    nan, inf = float('nan'), float('inf')
    dist = torch.tensor([[[9.0, 0.0, 1.0], [2.0, 9.0, nan], [inf, 3.0, 9.0]],
                         [[9.0, 1.0, 1.0], [1.0, 9.0, 2.0], [nan, 1.0, 9.0]]])        # [r, s, o]
    trip, d, info = transe.mine_from_distances(dist, threshold=inf)
    assert trip.tolist() == [[0, 0, 1], [0, 0, 2], [0, 1, 1], [0, 1, 2], [1, 1, 0], [2, 1, 1], [1, 0, 0], [1, 1, 2], [2, 0, 1],
                             [2, 0, 0]]
    assert d.tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 2.0, 3.0, inf] and info['count'] == 10
    trip, d, info = transe.mine_from_distances(dist, k=3)
    assert trip.tolist() == [[0, 0, 1], [0, 0, 2], [0, 1, 1]] and info['count'] == 6      # the tie block of the 3rd distance
    trip, _, info = transe.mine_from_distances(dist, k=3, exclude_self=False)
    assert trip.tolist() == [[0, 0, 1], [0, 0, 2], [0, 1, 1]] and info['count'] == 6      # the diagonal is at 9
    assert transe.mine_from_distances(dist, threshold=0.0)[0].tolist() == [[0, 0, 1]]
    assert transe.mine_from_distances(dist, threshold=-0.5)[0].shape == (0, 3)
    lo, hi, ent = filter_arrays({(0, 0, 1), (0, 1, 1)}, 3, 2)
    trip, _, _ = transe.mine_from_distances(dist, k=3, filt_lo=lo, filt_hi=hi, filt_ent=ent)
    assert trip.tolist() == [[0, 0, 2], [0, 1, 2], [1, 1, 0]]


def test_both_overflow_errors_carry_the_true_count():
    from gcn_vae_amd import ops, transe
    dist = torch.rand(2, 10, 10, generator=torch.Generator().manual_seed(7))
    want = brute_force(dist, True, threshold=0.4)[2]
    assert want > 5
    with pytest.raises(transe.MineOverflow) as err:
        transe.mine_from_distances(dist, threshold=0.4, max_results=want - 1)
    assert err.value.count == want and str(want) in str(err.value)
    assert transe.mine_from_distances(dist, threshold=0.4, max_results=want)[0].shape[0] == want
    ties = torch.ones(2, 6, 6)                                   # 60 candidates at one distance: a tie block
    with pytest.raises(transe.MineOverflow) as err:
        transe.mine_from_distances(ties, k=3, max_results=59)
    assert err.value.count == 60 and '60' in str(err.value)
    trip, d, info = transe.mine_from_distances(ties, k=3, max_results=60)
    assert trip.tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 3]] and info['count'] == 60
    assert transe.MineOverflow is ops.MineOverflow
    # the direction argument of the shared helpers: ascending for distances, descending (the default) for logits
    t = torch.tensor([[0, 0, 1], [1, 0, 0], [0, 0, 2]])
    v = torch.tensor([2.0, 1.0, 1.0])
    assert ops.mine_order(t, v, 3, 1, ascending=True)[0].tolist() == [[0, 0, 2], [1, 0, 0], [0, 0, 1]]
    assert ops.mine_order(t, v, 3, 1)[0].tolist() == [[0, 0, 1], [0, 0, 2], [1, 0, 0]]
    assert ops.mine_select(t, v, 1, 10, 3, 1, ascending=True)[2] == 2 and ops.mine_select(t, v, 1, 10, 3, 1)[2] == 1


def test_exactly_one_of_k_and_threshold():
    from gcn_vae_amd import ops, transe
    tables = (torch.zeros(4, 3), torch.zeros(2, 3), 1, True)
    for fn in (lambda **kw: transe.mine_triplets(tables, **kw), lambda **kw: transe.mine_triplets_unfused(tables, **kw),
               lambda **kw: ops.transe_mine(tables[0], tables[1], 1, **kw),
               lambda **kw: transe.mine_from_distances(torch.zeros(2, 4, 4), **kw)):
        with pytest.raises(ValueError, match='exactly one'):
            fn()
        with pytest.raises(ValueError, match='exactly one'):
            fn(k=3, threshold=0.0)
        with pytest.raises(ValueError, match='NaN'):
            fn(threshold=float('nan'))
        with pytest.raises(ValueError):
            fn(k=0)


def test_entry_points_are_exported_and_check_their_arguments():
    """gv_transe_mine validates on the host before any launch (this runs without a GPU)."""
    from gcn_vae_amd import lib, ops
    l = lib.load()
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'gv_transe_mine') and hasattr(handle, 'gv_transe_mine_workspace_bytes')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gcnvae.h')).read()
    assert 'int gv_transe_mine(' in header and 'int64_t gv_transe_mine_workspace_bytes(' in header
    assert 'gv_transe_mine' in lib.SIGNATURES and 'gv_transe_mine_workspace_bytes' in lib.SIGNATURES
    one = ctypes.c_void_p(16)            # a non-NULL address that is never dereferenced: every call below fails before a launch

    def call(en=one, rn=one, n=100, num_rels=3, dim=8, p=1, lo=None, hi=None, ent=None, n_ent=0, mode=0, prefix_bits=0, prefix=0,
             bin_bits=12, out=one, capacity=10, counter=one, hist=one, ws=None, ws_bytes=0):
        return l.gv_transe_mine(en, rn, n, num_rels, dim, p, lo, hi, ent, n_ent, 1, mode, 0, prefix_bits, prefix, bin_bits, out,
                                capacity, counter, hist, ws, ws_bytes, None)
    assert call(dim=0) != 0 and 'dim' in lib.last_error()
    assert call(dim=ops.TRANSE_MAX_DIM + 1) != 0 and 'dim' in lib.last_error()
    assert ops.TRANSE_MAX_DIM == 512
    assert call(p=3) != 0 and 'p_norm' in lib.last_error()
    assert call(p=0) != 0
    assert call(mode=1, bin_bits=13) != 0 and 'bin_bits' in lib.last_error()
    assert call(mode=1, bin_bits=0) != 0 and 'bin_bits' in lib.last_error()
    assert call(mode=1, prefix_bits=22, bin_bits=12) != 0
    assert call(mode=1, prefix_bits=12, prefix=4096, bin_bits=10) != 0
    assert call(lo=one) != 0 and 'filt' in lib.last_error()                       # the three filter arrays come together
    assert call(lo=one, hi=one, ent=one, n_ent=5) != 0 and 'workspace' in lib.last_error()
    assert call(lo=one, hi=one, ent=one, n_ent=5, ws=one, ws_bytes=8) != 0 and 'workspace' in lib.last_error()
    assert call(lo=one, hi=one, ent=one, n_ent=5, ws=ctypes.c_void_p(24), ws_bytes=1 << 20) != 0 and 'aligned' in lib.last_error()
    assert call(n=2 ** 20, num_rels=2 ** 11) != 0 and '2^31' in lib.last_error()
    assert call(num_rels=2 ** 19 + 1, n=1) != 0 and 'relations' in lib.last_error()
    assert call(en=None) != 0 and 'NULL' in lib.last_error()
    assert call(rn=None) != 0 and 'NULL' in lib.last_error()
    assert call(out=None) != 0 and 'NULL' in lib.last_error()
    assert call(out=ctypes.c_void_p(8)) != 0 and 'aligned' in lib.last_error()
    assert call(counter=None) != 0 and 'NULL' in lib.last_error()
    assert call(mode=1, hist=None) != 0 and 'NULL' in lib.last_error()
    assert call(capacity=-1) != 0 and 'capacity' in lib.last_error()
    assert call(capacity=2 ** 31) != 0 and 'capacity' in lib.last_error()
    assert call(mode=2) != 0 and 'mode' in lib.last_error()
    assert call(num_rels=0) != 0 and call(n=-1) != 0
    assert call(n=0, en=None, rn=None, out=None, counter=None) == 0                # no entities: nothing to do
    assert call(n=0, dim=0, en=None, rn=None, out=None, counter=None) != 0         # ... but the arguments are still checked
    assert l.gv_transe_mine_workspace_bytes(0, 3, 5) == 0
    assert l.gv_transe_mine_workspace_bytes(100, 3, 5) >= (4 + 5 + 5) * 4
    fb = l.gv_transe_mine_workspace_bytes(14541, 237, 310116)
    assert fb >= (2 * 228 * 228 + 1 + 310116) * 4 and fb % 16 == 0
    assert fb == l.gv_mine_scores_workspace_bytes(14541, 237, 310116)              # one re-bucketed filter for both miners


def test_the_wrappers_refuse_host_tensors_and_bad_arguments():
    from gcn_vae_amd import ops, ranking, transe
    en, rn = torch.zeros(4, 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.transe_mine(en, rn, 1, k=3)
    with pytest.raises(ValueError, match='max_results'):
        ops.transe_mine(en, rn, 1, k=3, max_results=0)
    fi = ranking.FilterIndex(5, 2, np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match='FilterIndex'):
        transe.mine_triplets((en, rn, 1, True), k=3, filter_index=fi)
    assert ops.mine_key(-0.0) == ops.mine_key(0.0) == 0x80000000                  # threshold -0 selects the zero distances
    assert ops.mine_key(-1.5) < ops.mine_key(-0.5) < ops.mine_key(-0.0) < ops.mine_key(0.25)      # key(-d): nearer = larger


def test_the_new_flags_parse_and_bad_values_are_refused():
    from gcn_vae_amd import transe
    p = transe.build_parser()
    a = p.parse_args(['-d', 'x', '--complete-topk', '50', '--complete-threshold', '7.5', '--complete-out', 'c.tsv'])
    assert (a.complete_topk, a.complete_threshold, a.complete_out) == (50, 7.5, 'c.tsv')
    transe.check_args(a)
    d = p.parse_args(['-d', 'x'])
    assert (d.complete_topk, d.complete_threshold, d.complete_out) == (None, None, 'transe_completions.tsv')
    assert d.predict_topk is None and d.predict_out == 'transe_predictions.tsv'      # the existing flags as they were
    transe.check_args(d)
    transe.check_args(p.parse_args(['-d', 'x', '--complete-threshold', '-1']))        # a negative distance: an empty file, no error
    transe.check_args(p.parse_args(['-d', 'x', '--complete-threshold', 'inf']))
    for bad in ('0', '-3'):
        with pytest.raises(ValueError, match='--complete-topk'):
            transe.check_args(p.parse_args(['-d', 'x', '--complete-topk', bad]))
    with pytest.raises(ValueError, match='--complete-threshold'):
        transe.check_args(p.parse_args(['-d', 'x', '--complete-threshold', 'nan']))
