"""The constructed TransE step cases (transe_cases.py) without a GPU: every named case finds an unambiguous seed among eight, its
margin leaves 20..80 % of the pairs active in float64, and the structure the device tests rely on is really there."""
import numpy as np
import pytest
import torch

import transe_cases as tc


@pytest.mark.parametrize('param', tc.PARAMS, ids=tc.param_id)
def test_case_is_unambiguous_active_share_and_structure(param):
    (V, R, dim, B, K), (p, nf, adv, regul) = param
    c = tc.case_of(param)                                          # raises when none of the 8 seeds is usable
    assert c['amb_rows'] == 0 and c['amb_pairs'] == 0 and c['cancelled'] == 0 and 0 <= c['seed'] < tc.MAX_SEEDS
    bh, br, bt, ent, rel = c['bh'], c['br'], c['bt'], c['ent'], c['rel']
    assert ent.shape == (V, dim) and rel.shape == (R, dim) and ent.dtype == rel.dtype == torch.float32
    assert bh.numel() == br.numel() == bt.numel() == B * (1 + K)
    assert 0 <= int(bh.min()) and int(max(bh.max(), bt.max())) < V and 0 <= int(br.min()) and int(br.max()) < R
    # the hinge: 20..80 % of the pairs active in the float64 reference, the margin a positive float32
    s64 = c['out64'][0][0]
    ps, ns = s64[:B].view(1, B), s64[B:].view(K, B)
    share = float(((ps - ns) > -c['margin']).double().mean())
    assert share == c['active_share'] and 0.2 <= share <= 0.8
    assert c['margin'] > 0 and c['margin'] == float(np.float32(c['margin']))
    assert c['lr'] > 0 and np.log2(c['lr']) == round(np.log2(c['lr']))
    # layout: every negative keeps the relation and exactly one entity of its positive -- but the one identical negative
    ph, pt = bh[:B], bt[:B]
    nh, nr, nt = bh[B:].view(K, B), br[B:].view(K, B), bt[B:].view(K, B)
    assert bool((nr == br[:B]).all())
    head, tail = nh != ph, nt != pt
    assert not bool((head & tail).any())
    same = ~head & ~tail
    assert int(same.sum()) == 1 and bool(same[K - 1, B - 1])
    assert float(ns[K - 1, B - 1]) == float(ps[0, B - 1])         # ns == ps, d = 0
    if K >= 2:
        assert bool((head.any(0) & tail.any(0)).any())            # both kinds within one positive
    # the planted rows, each read by the batch
    n64 = ent.double().norm(dim=1)
    assert not bool(ent[tc.ZERO].any())
    assert abs(float(n64[tc.TINY_BELOW]) / 5e-13 - 1) < 1e-2 and abs(float(n64[tc.TINY_ABOVE]) / 2e-12 - 1) < 1e-2
    assert float(n64[tc.TINY_BELOW]) < 1e-12 < float(n64[tc.TINY_ABOVE])
    occ = tc.occurrence_ids(c)
    for row in (tc.ZERO, tc.TINY_BELOW, tc.TINY_ABOVE):
        assert bool((occ == row).any())
    assert bool((tc.corrupted_ids(c) == tc.ZERO).any()) or B * K < 4        # a corrupted side on the zero row as well
    assert int(((ph == tc.HOT) | (pt == tc.HOT)).sum()) * 4 >= B
    if B > 64:
        assert int(torch.bincount(br[:B], minlength=R).max()) > 64
        assert int(((ph == tc.HOT) | (pt == tc.HOT)).sum()) > 64 or B < 130
    touched = torch.zeros(V, dtype=torch.bool)
    touched[torch.cat([bh, bt])] = True
    assert not bool(touched[V - 1]) and bool(touched[occ].all()) and int(touched.sum()) == int(torch.unique(occ).numel())
    if not nf:
        assert float(s64.max()) < 32.0                             # raw tables: scores O(1..20), exp(-ns T) well-conditioned


def test_ambiguity_rule_flags_the_edges_and_exempts_exact_zeros():
    ent = torch.tensor([[1.0, 2.0], [0.5, -1.0], [1.5, 1.0 + 2.0 ** -22], [0.0, 0.0]])
    rel = torch.tensor([[0.5, -1.0], [0.0, 0.0]])
    bh, br, bt = torch.tensor([0, 3, 0]), torch.tensor([0, 1, 0]), torch.tensor([2, 3, 1])
    args = (ent.double(), rel.double(), ent, rel, bh, br, bt, 1, 2)
    rows, _ = tc.ambiguity(*args, 1, False, 1.0)
    # row 0: z = (0, -2^-22), inside 16 ulp of the operands' size; row 1: all-zero operands, exactly 0 in both precisions
    assert rows.tolist() == [True, False, False]
    rows, _ = tc.ambiguity(*args, 2, False, 1.0)
    assert not bool(rows.any())                                    # p = 2 has no sign branch
    # scores 2^-22, 0 and 3: the pairs (0, j) have d = 2^-22 - (0 | 3); a margin of 3 puts the second on the hinge's edge
    _, pairs = tc.ambiguity(*args, 1, False, 3.0)
    assert pairs.view(-1).tolist() == [False, True]
    _, pairs = tc.ambiguity(*args, 1, False, 3.001)
    assert not bool(pairs.any())


def test_cases_are_shared_and_cover_every_switch():
    assert tc.case_of(tc.PARAMS[5]) is tc.case_of(tc.PARAMS[5])   # one case and one reference per process
    for shape in tc.SHAPES:
        mine = [c for s, c in tc.PARAMS if s == shape]
        assert {c[0] for c in mine} == {1, 2} and {c[1] for c in mine} == {True, False}
        assert {c[2] for c in mine} == {None, 1.0} and {c[3] for c in mine} == {0.0, 0.01}
