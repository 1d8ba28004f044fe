"""Whole-graph triplet mining, the parts that need no GPU: the rule itself (ranking.mine_from_scores against a triple Python
loop), the argument checks of gv_mine_scores (nothing is launched), and the command-line surface."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from mine_cases import brute_force, filter_arrays, same


def scores(n, num_rels, h, seed, special=True):
    gen = torch.Generator().manual_seed(seed)
    emb = torch.randn(n, h, generator=gen)
    w = torch.randn(num_rels, h, generator=gen)
    if special and n >= 8:
        emb[5] = emb[2]                      # exact ties
        emb[6] = emb[2]
        emb[3] = 0.0                         # +0 / -0 logits
        emb[4] = float('nan')                # a NaN row (and column)
        emb[7] = 0.0
        emb[7, 0] = float('inf')             # +-inf logits, NaN against the zero row
    return torch.einsum('sd,rd,od->rso', emb, w, emb)


@pytest.mark.parametrize('n,num_rels,seed', [(12, 3, 0), (9, 2, 1), (8, 1, 2), (3, 3, 3), (1, 2, 4)])
@pytest.mark.parametrize('exclude_self', [True, False])
def test_mine_from_scores_equals_the_triple_loop(n, num_rels, seed, exclude_self):
    from gcn_vae_amd import ranking
    score = scores(n, num_rels, 4, seed)
    gen = torch.Generator().manual_seed(seed + 100)
    filt = {(int(a), int(b), int(c)) for a, b, c in zip(torch.randint(0, n, (2 * n,), generator=gen),
                                                        torch.randint(0, num_rels, (2 * n,), generator=gen),
                                                        torch.randint(0, n, (2 * n,), generator=gen))}
    for f in (None, filt):
        arrays = dict(zip(('filt_lo', 'filt_hi', 'filt_ent'), filter_arrays(f, n, num_rels))) if f else {}
        total = brute_force(score, False, k=10 ** 9, filt=f, exclude_self=exclude_self)[2]
        for k in (1, 2, 5, 17, max(total, 1), total + 7):          # the last: K larger than the number of candidates
            got = ranking.mine_from_scores(score, k=k, exclude_self=exclude_self, **arrays)
            assert same(got, brute_force(score, False, k=k, filt=f, exclude_self=exclude_self))
        for t in (float('inf'), float('-inf'), 0.0, -0.0, 0.7, -1.3):
            got = ranking.mine_from_scores(score, threshold=t, exclude_self=exclude_self, **arrays)
            assert same(got, brute_force(score, False, threshold=t, filt=f, exclude_self=exclude_self))
        everything = ranking.mine_from_scores(score, threshold=float('-inf'), exclude_self=exclude_self, **arrays)
        assert everything[0].shape[0] == total and not bool(torch.isnan(everything[1]).any())      # all but NaN


def test_the_rule_on_a_hand_made_tensor():
    from gcn_vae_amd import ranking
    nan, inf = float('nan'), float('inf')
    score = torch.tensor([[[9.0, -0.0, 1.0], [0.0, 9.0, nan], [inf, -inf, 9.0]],
                          [[9.0, 1.0, 1.0], [1.0, 9.0, 0.0], [nan, 1.0, 9.0]]])        # [r, s, o]
    trip, logits, info = ranking.mine_from_scores(score, threshold=-inf)
    assert trip.tolist() == [[2, 0, 0], [0, 0, 2], [0, 1, 1], [0, 1, 2], [1, 1, 0], [2, 1, 1], [0, 0, 1], [1, 0, 0], [1, 1, 2],
                             [2, 0, 1]]
    assert logits.tolist() == [inf, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, -inf] and info['count'] == 10
    assert not bool(torch.signbit(logits[6:9]).any())                                   # -0 is reported as +0
    trip, logits, info = ranking.mine_from_scores(score, k=3)
    assert trip.tolist() == [[2, 0, 0], [0, 0, 2], [0, 1, 1]] and info['count'] == 6      # the tie block of the 3rd logit
    trip, _, info = ranking.mine_from_scores(score, k=3, exclude_self=False)
    assert trip.tolist() == [[2, 0, 0], [0, 0, 0], [0, 1, 0]] and info['count'] == 7
    assert ranking.mine_from_scores(score, threshold=inf)[0].tolist() == [[2, 0, 0]]
    assert ranking.mine_from_scores(score[:, :2, :2], threshold=inf)[0].shape == (0, 3)
    lo, hi, ent = filter_arrays({(2, 0, 0), (0, 1, 1)}, 3, 2)
    trip, _, _ = ranking.mine_from_scores(score, k=3, filt_lo=lo, filt_hi=hi, filt_ent=ent)
    assert trip.tolist() == [[0, 0, 2], [0, 1, 2], [1, 1, 0]]


def test_both_overflow_errors_carry_the_true_count():
    from gcn_vae_amd import ranking
    score = scores(10, 2, 4, 7, special=False)
    want = brute_force(score, False, threshold=-0.5)[2]
    assert want > 5
    with pytest.raises(ranking.MineOverflow) as err:
        ranking.mine_from_scores(score, threshold=-0.5, max_results=want - 1)
    assert err.value.count == want and str(want) in str(err.value)
    assert ranking.mine_from_scores(score, threshold=-0.5, max_results=want)[0].shape[0] == want
    ties = torch.ones(2, 6, 6)                                   # 60 candidates on one logit value: a tie block
    with pytest.raises(ranking.MineOverflow) as err:
        ranking.mine_from_scores(ties, k=3, max_results=59)
    assert err.value.count == 60 and '60' in str(err.value)
    trip, logits, info = ranking.mine_from_scores(ties, k=3, max_results=60)
    assert trip.tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 3]] and info['count'] == 60
    assert issubclass(ranking.MineOverflow, RuntimeError)


def test_exactly_one_of_k_and_threshold():
    from gcn_vae_amd import generate, ops, ranking
    emb, w = torch.zeros(4, 3), torch.zeros(2, 3)
    for fn in (functools.partial(ranking.mine_triplets, emb, w), functools.partial(ranking.mine_triplets_unfused, emb, w),
               functools.partial(ops.mine_scores, emb, w), functools.partial(ranking.mine_from_scores, torch.zeros(2, 4, 4)),
               functools.partial(generate.sample_graph, None, 4)):
        with pytest.raises(ValueError, match='exactly one'):
            fn()
        with pytest.raises(ValueError, match='exactly one'):
            fn(k=3, threshold=0.0)
    with pytest.raises(ValueError):
        ranking.mine_from_scores(torch.zeros(2, 4, 4), threshold=float('nan'))
    with pytest.raises(ValueError):
        ranking.mine_from_scores(torch.zeros(2, 4, 4), k=0)


def test_the_host_key_is_the_order():
    from gcn_vae_amd import ops
    xs = [float('-inf'), -3.0e38, -1.5, -1e-45, -0.0, 1e-45, 2.0, 3.0e38, float('inf')]
    keys = [ops.mine_key(x) for x in xs]
    assert keys[4] == ops.mine_key(0.0) == 0x80000000 and ops.mine_key(float('nan')) == 0
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and min(keys) > 0
    assert sum(b for _, b in ops.MINE_LEVELS) == 32 and [p for p, _ in ops.MINE_LEVELS] == [0, 12, 22]


def test_entry_points_are_exported_and_check_their_arguments():
    """gv_mine_scores validates on the host before any launch (this runs without a GPU)."""
    from gcn_vae_amd import lib
    l = lib.load()
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'gv_mine_scores') and hasattr(handle, 'gv_mine_scores_workspace_bytes')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gcnvae.h')).read()
    assert 'int gv_mine_scores(' in header and 'int64_t gv_mine_scores_workspace_bytes(' in header
    assert 'gv_mine_scores' in lib.SIGNATURES and 'gv_mine_scores_workspace_bytes' in lib.SIGNATURES
    one = ctypes.c_void_p(16)            # a non-NULL address that is never dereferenced: every call below fails before a launch

    def call(e=one, ld_e=8, w=one, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, mode=0, prefix_bits=0, prefix=0, bin_bits=12,
             out=one, capacity=10, counter=one, hist=one, ws=None, ws_bytes=0, n=100, num_rels=3, h=8):
        return l.gv_mine_scores(e, ld_e, w, ld_w, None, lo, hi, ent, n_ent, 1, mode, 0, prefix_bits, prefix, bin_bits, out, capacity,
                                counter, hist, ws, ws_bytes, n, num_rels, h, None)
    assert call(e=None) != 0 and 'NULL' in lib.last_error()
    assert call(w=None) != 0 and 'NULL' in lib.last_error()
    assert call(out=None) != 0 and 'NULL' in lib.last_error()
    assert call(out=ctypes.c_void_p(8)) != 0 and 'aligned' in lib.last_error()
    assert call(counter=None) != 0 and 'NULL' in lib.last_error()
    assert call(mode=1, hist=None) != 0 and 'NULL' in lib.last_error()
    assert call(lo=one) != 0 and 'filt' in lib.last_error()                       # the three filter arrays come together
    assert call(lo=one, hi=one, ent=one, n_ent=5) != 0 and 'workspace' in lib.last_error()
    assert call(lo=one, hi=one, ent=one, n_ent=5, ws=one, ws_bytes=8) != 0 and 'workspace' in lib.last_error()
    assert call(lo=one, hi=one, ent=one, n_ent=5, ws=ctypes.c_void_p(24), ws_bytes=1 << 20) != 0 and 'aligned' in lib.last_error()
    assert call(ld_e=7) != 0 and 'leading dimension' in lib.last_error()
    assert call(ld_w=7) != 0 and 'leading dimension' in lib.last_error()
    assert call(n=2 ** 20, num_rels=2 ** 11) != 0 and '2^31' in lib.last_error()
    assert call(capacity=-1) != 0 and 'capacity' in lib.last_error()
    assert call(capacity=2 ** 31) != 0 and 'capacity' in lib.last_error()
    assert call(mode=2) != 0 and 'mode' in lib.last_error()
    assert call(mode=1, bin_bits=13) != 0 and 'bin_bits' in lib.last_error()
    assert call(mode=1, bin_bits=0) != 0
    assert call(mode=1, prefix_bits=22, bin_bits=12) != 0
    assert call(mode=1, prefix_bits=12, prefix=4096, bin_bits=10) != 0
    assert call(h=0) != 0 and call(num_rels=0) != 0 and call(n=-1) != 0
    assert call(n=0, e=None, w=None, out=None, counter=None) == 0                  # no entities: nothing to do
    assert l.gv_mine_scores_workspace_bytes(100, 3, 5) >= (4 + 5 + 5) * 4
    assert l.gv_mine_scores_workspace_bytes(0, 3, 5) == 0
    fb = l.gv_mine_scores_workspace_bytes(14541, 237, 310116)
    assert fb >= (2 * 228 * 228 + 1 + 310116) * 4 and fb % 16 == 0
    assert fb == l.gv_transe_mine_workspace_bytes(14541, 237, 310116)              # one re-bucketed filter for both miners


def test_the_wrappers_refuse_host_tensors_and_bad_arguments():
    from gcn_vae_amd import ops, ranking
    emb, w = torch.zeros(4, 3), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.mine_scores(emb, w, k=3)
    with pytest.raises(ValueError, match='width'):
        ops.mine_scores(emb, torch.zeros(2, 4), k=3)
    with pytest.raises(ValueError, match='max_results'):
        ops.mine_scores(emb, w, k=3, max_results=0)
    with pytest.raises(ValueError, match='together'):
        ops.mine_scores(emb, w, k=3, filt_lo=torch.zeros(8, dtype=torch.long))
    fi = ranking.FilterIndex(5, 2, np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match='FilterIndex'):
        ranking.mine_triplets(emb, w, k=3, filter_index=fi)


def test_the_new_flags_parse_and_are_refused_outside_test_mode():
    from gcn_vae_amd import train
    p = train.build_parser()
    a = p.parse_args(['-d', 'x', '--test-mode', 'True', '--complete-topk', '50', '--complete-threshold', '0.9', '--complete-out',
                      'c.tsv', '--sample-graph', '30', '--sample-topk', '7', '--sample-out', 's.tsv'])
    assert (a.complete_topk, a.complete_threshold, a.complete_out) == (50, 0.9, 'c.tsv')
    assert (a.sample_graph, a.sample_topk, a.sample_out) == (30, 7, 's.tsv')
    train.check_args(a)
    d = p.parse_args(['-d', 'x'])
    assert (d.complete_topk, d.complete_threshold, d.complete_out, d.sample_graph) == (0, None, 'completions.tsv', 0)
    assert d.generate is False and d.predict_topk == 0                               # the existing flags as they were
    train.check_args(d)
    for flags in (['--complete-topk', '5'], ['--complete-threshold', '0.5'], ['--sample-graph', '10']):
        with pytest.raises(ValueError, match='--test-mode'):
            train.main(p.parse_args(['-d', 'synthetic:30:3:100:10:10:0'] + flags))
    with pytest.raises(ValueError, match='probability'):
        train.check_args(p.parse_args(['-d', 'x', '--test-mode', 'True', '--complete-threshold', '1.5']))
    assert train._logit_of(0.5) == 0.0 and train._logit_of(0.0) == float('-inf') and train._logit_of(1.0) == float('inf')
