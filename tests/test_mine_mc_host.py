"""Type-correct completion on the posterior predictive without a GPU: the rule on materialised probabilities
(ranking.mine_from_probs) on a hand-made tensor, the --mc-complete flag's refusals and the flag sets it leaves alone, the wrappers'
argument errors that need no device, and gv_mine_scores_typed_mc's host-side argument checks (return codes, nothing launched)."""
import pytest
import torch

from gcn_vae_amd import lib, ops, ranking, train


def test_mine_from_probs_on_a_hand_made_tensor():
    nan = float('nan')
    # pbar[r, s, o], two relations, three entities; the diagonal is excluded by default
    pbar = torch.tensor([[[0.9, 0.5, 1.0], [1.0, 0.1, 0.25], [0.5, nan, 0.7]],
                         [[0.2, 1.0, 0.0], [0.75, 0.3, 0.5], [1.0, 0.5, 0.4]]])
    trip, probs, info = ranking.mine_from_probs(pbar, threshold=float('-inf'))
    # value descending, then (s, r, o) ascending: the saturated 1.0s tie, as do the 0.5s; the NaN is no candidate
    want = [(0, 0, 2), (0, 1, 1), (1, 0, 0), (2, 1, 0), (1, 1, 0), (0, 0, 1), (1, 1, 2), (2, 0, 0), (2, 1, 1), (1, 0, 2), (0, 1, 2)]
    assert [tuple(x) for x in trip.tolist()] == want and info['count'] == 11
    assert probs.tolist() == [1.0, 1.0, 1.0, 1.0, 0.75, 0.5, 0.5, 0.5, 0.5, 0.25, 0.0]
    # K inside the tie at 1.0: the first K in (s, r, o) order, the count is the whole tie
    trip, probs, info = ranking.mine_from_probs(pbar, k=2)
    assert [tuple(x) for x in trip.tolist()] == want[:2] and probs.tolist() == [1.0, 1.0] and info['count'] == 4
    with pytest.raises(ranking.MineOverflow) as err:
        ranking.mine_from_probs(pbar, k=2, max_results=3)
    assert err.value.count == 4
    trip, probs, info = ranking.mine_from_probs(pbar, k=6)
    assert [tuple(x) for x in trip.tolist()] == want[:6] and info['count'] == 9          # the four 0.5s count
    # a threshold is a probability, compared as it is
    trip, probs, info = ranking.mine_from_probs(pbar, threshold=0.5)
    assert [tuple(x) for x in trip.tolist()] == want[:9] and info['count'] == 9
    assert ranking.mine_from_probs(pbar, threshold=2.0)[0].shape == (0, 3)
    with pytest.raises(ranking.MineOverflow) as err:
        ranking.mine_from_probs(pbar, threshold=0.5, max_results=8)
    assert err.value.count == 9
    # the diagonal kept, the typed rule and a filter: (0, 0, 2) listed, relation 1 without subjects
    trip, _, info = ranking.mine_from_probs(pbar, threshold=0.9, exclude_self=False)
    assert [tuple(x) for x in trip.tolist()] == [(0, 0, 2), (0, 1, 1), (1, 0, 0), (2, 1, 0), (0, 0, 0)]
    cs = torch.tensor([[True, True, False], [False, False, False]])
    co = torch.tensor([[True, False, True], [True, True, True]])
    lo, hi, ent = torch.tensor([0, 1, 1, 1, 1, 1]), torch.tensor([1, 1, 1, 1, 1, 1]), torch.tensor([2])
    trip, probs, info = ranking.mine_from_probs(pbar, k=10, cand_subj=cs, cand_obj=co, filt_lo=lo, filt_hi=hi, filt_ent=ent)
    assert [tuple(x) for x in trip.tolist()] == [(1, 0, 0), (1, 0, 2)] and probs.tolist() == [1.0, 0.25] and info['count'] == 2
    for bad in (dict(), dict(k=1, threshold=0.5), dict(k=0), dict(threshold=nan)):
        with pytest.raises(ValueError):
            ranking.mine_from_probs(pbar, **bad)


def test_mc_complete_flag_and_its_refusals():
    p = train.build_parser()
    base = ['-d', 'synthetic:50:4:300:20:10:7']
    mc = ['--mc-samples', '3', '--test-mode', 'True']
    args = p.parse_args(base)
    assert args.mc_complete is False and args.mc_complete_out == 'mc_completions.tsv'
    ok = p.parse_args(base + mc + ['--complete-topk', '50', '--complete-typed', '--mc-complete', '--mc-complete-out', 'x.tsv'])
    assert ok.mc_complete is True and ok.mc_complete_out == 'x.tsv'
    train.check_args(ok)
    train.check_args(p.parse_args(base + mc + ['--complete-threshold', '0.9', '--complete-typed', '--mc-complete']))
    with pytest.raises(ValueError, match='--mc-samples'):
        train.check_args(p.parse_args(base + ['--test-mode', 'True', '--complete-topk', '50', '--complete-typed', '--mc-complete']))
    with pytest.raises(ValueError, match='--complete-typed'):
        train.check_args(p.parse_args(base + mc + ['--complete-topk', '50', '--mc-complete']))
    with pytest.raises(ValueError, match='--complete-typed'):
        train.check_args(p.parse_args(base + mc + ['--mc-complete']))
    with pytest.raises(ValueError, match='--complete-topk or --complete-threshold'):       # no selection: --complete-typed's own refusal
        train.check_args(p.parse_args(base + mc + ['--complete-typed', '--mc-complete']))
    with pytest.raises(ValueError, match='--test-mode'):
        train.check_args(p.parse_args(base + ['--mc-samples', '3', '--complete-topk', '50', '--complete-typed', '--mc-complete']))
    with pytest.raises(ValueError, match='deterministic'):
        train.check_args(p.parse_args(base + mc + ['--model-class', 'RGCN', '--complete-topk', '50', '--complete-typed',
                                                   '--mc-complete']))


def test_flag_sets_without_mc_complete_check_as_before():
    p = train.build_parser()
    base = ['-d', 'synthetic:50:4:300:20:10:7']
    for flags in ([], ['--test-mode', 'True', '--complete-topk', '50'], ['--test-mode', 'True', '--complete-topk', '50', '--complete-typed'],
                  ['--test-mode', 'True', '--mc-samples', '3', '--complete-topk', '50'],
                  ['--test-mode', 'True', '--mc-samples', '3', '--complete-topk', '50', '--complete-typed'],
                  ['--test-mode', 'True', '--mc-samples', '3', '--complete-threshold', '0.5', '--predict-topk', '3', '--filtered-eval']):
        args = p.parse_args(base + flags)
        assert args.mc_complete is False
        train.check_args(args)
    with pytest.raises(ValueError, match='--complete-typed'):
        train.check_args(p.parse_args(base + ['--test-mode', 'True', '--complete-typed']))
    with pytest.raises(ValueError, match='--type-constrain'):
        train.check_args(p.parse_args(base + ['--mc-samples', '4', '--test-mode', 'True', '--filtered-eval', '--type-constrain']))


def test_wrapper_argument_errors_need_no_device():
    z, w = torch.zeros(2, 5, 3), torch.zeros(2, 3)
    tc = ranking.TypeConstraint(5, 2, torch.tensor([[0, 1, 2]]))
    for fn in (ranking.mine_triplets_mc, ranking.mine_triplets_mc_unfused):
        with pytest.raises(ValueError, match='type_constraint'):
            fn(z, w, k=3)
        with pytest.raises(ValueError, match='exactly one'):
            fn(z, w, type_constraint=tc)
        with pytest.raises(ValueError, match='posterior_samples'):
            fn(z[0], w, k=3, type_constraint=tc)
        with pytest.raises(ValueError, match='per sample'):
            fn(z, w, k=3, type_constraint=tc, flow_log_probs=torch.zeros(3))
        with pytest.raises(ValueError, match='TypeConstraint'):
            fn(z[:, :4], w, k=3, type_constraint=tc)
    ptr, ids = tc.members()
    with pytest.raises(TypeError, match='3-D'):
        ops.mine_scores_typed_mc(z[0], w, ptr, ids, k=3)
    with pytest.raises(ValueError, match='exactly one'):
        ops.mine_scores_typed_mc(z, w, ptr, ids)
    with pytest.raises(ValueError, match='width'):
        ops.mine_scores_typed_mc(z, w[:, :2], ptr, ids, k=3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):         # good arguments: the CPU tables are what is refused next
        ops.mine_scores_typed_mc(z, w, ptr, ids, k=3)


def test_the_c_entry_reports_bad_arguments_before_any_launch():
    """Return codes, not launches (runs without a GPU): the checks gv_mine_scores_typed makes, plus the sample geometry."""
    l = lib.load()
    one = 1 << 4                                            # any non-NULL, 16-byte aligned address: nothing is dereferenced on the host

    def mc(n=10, num_rels=2, h=4, ld_e=4, e=one, e_stride=40, n_samples=2, units=one, n_units=1, mode=0, capacity=8, out=one,
           counter=one, bin_bits=1, filt=(None, None, None)):
        return l.gv_mine_scores_typed_mc(e, ld_e, e_stride, n_samples, one, h, None, one, one, units, n_units, *filt, 0, 1, mode, 0, 0,
                                         0, bin_bits, out, capacity, counter, one, n, num_rels, h, None)

    assert mc(n=0) == 0 and mc(n=0, n_samples=1, e_stride=0) == 0               # no entity: nothing to do
    for bad in (dict(n_samples=0), dict(n_samples=-1), dict(e_stride=39), dict(e_stride=0), dict(ld_e=6, e_stride=57),
                dict(out=one + 4), dict(out=None), dict(n_units=2 ** 31), dict(n_units=-1), dict(mode=7), dict(capacity=-1),
                dict(e=None), dict(units=None), dict(units=one + 4), dict(counter=None), dict(num_rels=0), dict(h=0), dict(n=-1),
                dict(ld_e=3), dict(mode=1, bin_bits=13), dict(filt=(one, None, None))):
        assert mc(**bad) != 0, bad
        assert 'gv_mine_scores_typed_mc' in lib.last_error(), bad
    assert mc(n_samples=0) != 0 and 'n_samples' in lib.last_error()
    assert mc(e_stride=39) != 0 and 'e_stride' in lib.last_error()
    assert mc(out=one + 4) != 0 and 'aligned' in lib.last_error()
