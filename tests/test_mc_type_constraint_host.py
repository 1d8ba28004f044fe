"""The type-constrained protocol on the posterior predictive without a GPU: the --mc-type-constrain flag's defaults, acceptance and
refusals (and the standing refusal of --mc-samples with --type-constrain), the argument errors of the two ops wrappers that are
raised before any look at the device, ``ranking.rank_from_scores_constrained`` applied to a hand-made pbar (saturated ties, NaN
members and non-members, a non-member target) against mid-ranks written out by hand, and the two gv_*_mc_constrained names in
the header and the ctypes table.

The ``_unfused`` twins do NOT run on CPU tensors: their pbar comes from ``ops.gemm`` (``_mc_pbar_unfused``), which has no CPU path;
that refusal is asserted here, their values are checked on the GPU (tests/test_gpu_mc_type_constraint.py)."""
import inspect
import os
import re

import pytest
import torch

from gcn_vae_amd import lib, ops, ranking, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mc_type_constrain_flag_defaults_acceptance_and_refusals():
    p = train.build_parser()
    base = ['-d', 'synthetic:50:4:300:20:10:7']
    args = p.parse_args(base)
    assert args.mc_type_constrain is False
    train.check_args(args)
    ok = p.parse_args(base + ['--mc-samples', '4', '--mc-seed', '7', '--test-mode', 'True', '--filtered-eval', '--predict-topk', '3',
                              '--mc-type-constrain'])
    assert ok.mc_type_constrain is True and ok.type_constrain is False
    train.check_args(ok)
    with pytest.raises(ValueError, match='--mc-type-constrain.*--mc-samples'):
        train.check_args(p.parse_args(base + ['--test-mode', 'True', '--filtered-eval', '--mc-type-constrain']))
    with pytest.raises(ValueError, match='--mc-type-constrain.*--filtered-eval'):
        train.check_args(p.parse_args(base + ['--mc-samples', '4', '--test-mode', 'True', '--mc-type-constrain']))
    # the single-draw flag stays refused next to --mc-samples, with or without the new flag
    for extra in ([], ['--mc-type-constrain']):
        with pytest.raises(ValueError, match='--type-constrain'):
            train.check_args(p.parse_args(base + ['--mc-samples', '4', '--test-mode', 'True', '--filtered-eval', '--type-constrain']
                                          + extra))
    assert 'type_constraint' in inspect.signature(train.write_mc_predictions).parameters
    assert inspect.signature(train.write_mc_predictions).parameters['type_constraint'].default is None


def test_wrapper_shape_errors_are_raised_before_any_look_at_the_device():
    q, e = torch.zeros(2, 4, 8), torch.zeros(2, 50, 8)                  # CPU tensors: a device check would raise RuntimeError
    t = torch.zeros(4, dtype=torch.long)
    cand = torch.zeros(3, 2, dtype=torch.int32)
    sets = torch.zeros(4, dtype=torch.int32)
    for call in (lambda q_, e_: ops.rank_scores_mc_constrained(q_, e_, t, cand, sets),
                 lambda q_, e_: ops.topk_scores_mc_constrained(q_, e_, 3, cand, sets)):
        with pytest.raises(TypeError, match='3-D'):
            call(q[0], e[0])                                            # the single-sample operands
        with pytest.raises(ValueError, match='samples'):
            call(q, e[:1])
        with pytest.raises(ValueError, match='width'):
            call(q, e[:, :, :4])
        with pytest.raises(ValueError, match='at least one entity'):
            call(q, e[:, :0])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call(q, e)                                                  # well-formed: only now the device is looked at


def test_signatures_of_the_new_functions():
    names = list(inspect.signature(ops.rank_scores_mc_constrained).parameters)
    assert names == ['q', 'entities', 'target', 'cand', 'cand_set', 'bias', 'filt_lo', 'filt_hi', 'filt_ent']
    names = list(inspect.signature(ops.topk_scores_mc_constrained).parameters)
    assert names == ['q', 'entities', 'k', 'cand', 'cand_set', 'bias', 'filt_lo', 'filt_hi', 'filt_ent']
    for fn in (ranking.perturb_and_get_rank_mc_constrained, ranking.perturb_and_get_rank_mc_constrained_unfused):
        assert list(inspect.signature(fn).parameters) == ['z', 'w', 'a', 'r', 'b', 'test_size', 'filter_index', 'type_constraint',
                                                          'direction', 'batch_size', 'all_batches', 'flow_log_probs']
    for fn in (ranking.calc_mc_constrained_mrr, ranking.calc_mc_constrained_mrr_unfused):
        assert list(inspect.signature(fn).parameters) == ['z', 'w', 'test_triplets', 'filter_index', 'type_constraint',
                                                          'flow_log_probs', 'hits', 'eval_bz', 'all_batches', 'verbose']
    for fn in (ranking.predict_topk_mc, ranking.predict_topk_mc_unfused):
        par = inspect.signature(fn).parameters
        assert list(par)[-1] == 'type_constraint' and par['type_constraint'].default is None


def test_constrained_mid_ranks_on_a_hand_made_pbar():
    nan = float('nan')
    #                 0    1    2    3    4    5    6    7
    pbar = torch.tensor([[1.0, 1.0, 1.0, 0.5, nan, nan, 0.2, 1.0],      # target 0 (saturated), a member
                         [1.0, 1.0, 1.0, 0.5, nan, nan, 0.2, 1.0],      # target 3, NOT a member
                         [1.0, 1.0, 1.0, 0.5, nan, nan, 0.2, 1.0],      # target 4: a NaN target
                         [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])     # all saturated
    target = torch.tensor([0, 3, 4, 2])
    member = torch.tensor([[1, 1, 0, 1, 1, 0, 1, 0]] * 3 + [[1, 0, 1, 1, 1, 0, 0, 1]], dtype=torch.bool)
    listed = torch.zeros(4, 8, dtype=torch.bool)
    listed[0, 1] = True            # a saturated tie that is a member
    listed[0, 4] = True            # the NaN member
    listed[1, 5] = True            # the NaN non-member
    listed[3, 3] = True
    raw, filt, raw_c, filt_c = ranking.rank_from_scores_constrained(pbar, target, member, listed)
    # query 0, target 1.0: ties 1, 2, 7 (three halves), NaN 4, 5 above.  Members other than the target: 1 (tie), 3, 4 (NaN), 6.
    assert float(raw[0]) == 2 + 1.5 and float(filt[0]) == 1 + 1.0        # listed: the tie 1 and the NaN 4
    assert float(raw_c[0]) == 1 + 0.5                                    # NaN member 4 above, tie 1; NaN non-member 5 nowhere
    assert float(filt_c[0]) == 0.0                                       # both of them listed
    # query 1, target 0.5 (entity 3, no member): above 0, 1, 2, 7 (1.0) and NaN 4, 5.  Members: 0, 1, 4 (NaN), 6 (below).
    assert float(raw[1]) == 6.0 and float(filt[1]) == 5.0                # the listed NaN non-member leaves the filtered pool
    assert float(raw_c[1]) == 3.0 and float(filt_c[1]) == 3.0            # ... and was never in the constrained ones
    # query 2, a NaN target: last in every pool (7 others; members other than the target: 0, 1, 3, 6)
    assert float(raw[2]) == 7.0 and float(filt[2]) == 7.0 and float(raw_c[2]) == 4.0 and float(filt_c[2]) == 4.0
    # query 3, everything saturated: the middle rank of each pool.  Members other than the target 2: 0, 3, 4, 7; 3 is listed.
    assert float(raw[3]) == 3.5 and float(filt[3]) == 3.0 and float(raw_c[3]) == 2.0 and float(filt_c[3]) == 1.5
    # without a listed mask the filtered kinds are None and the others unchanged
    raw0, none1, raw_c0, none2 = ranking.rank_from_scores_constrained(pbar, target, member)
    assert none1 is None and none2 is None and torch.equal(raw0, raw) and torch.equal(raw_c0, raw_c)


def test_unfused_twins_have_no_cpu_path():
    z, w = torch.zeros(2, 6, 4), torch.zeros(3, 4)
    tc = ranking.TypeConstraint(6, 3, torch.tensor([[0, 0, 1], [2, 1, 3]]))
    one = torch.zeros(1, dtype=torch.long)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.perturb_and_get_rank_mc_constrained_unfused(z, w, one, one, one, 1, None, tc, 'o')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.calc_mc_constrained_mrr_unfused(z, w, torch.zeros(1, 3, dtype=torch.long), None, tc, verbose=False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ranking.predict_topk_mc_unfused(z, w, one, one, 2, type_constraint=tc)
    # what needs no device is refused first
    with pytest.raises(ValueError, match='per sample'):
        ranking.calc_mc_constrained_mrr(z, w, torch.zeros(1, 3, dtype=torch.long), None, tc, flow_log_probs=torch.zeros(3),
                                        verbose=False)
    with pytest.raises(ValueError, match='direction'):
        ranking.predict_topk_mc(z, w, one, one, 2, direction='x', type_constraint=tc)
    # no queries: empty results of the right kinds, no launch
    empty = torch.zeros(0, dtype=torch.long)
    out = ranking.perturb_and_get_rank_mc_constrained(z, w, empty, empty, empty, 0, None, tc, 'o')
    assert out[1] is None and out[3] is None and out[0].numel() == 0 and out[2].numel() == 0


def test_entry_points_in_the_header_and_the_ctypes_table():
    with open(os.path.join(ROOT, 'include', 'gcnvae.h')) as f:
        header = f.read()
    for name, parent in (('gv_rank_scores_mc_constrained', 'gv_rank_scores_mc'), ('gv_topk_scores_mc_constrained', 'gv_topk_scores_mc')):
        proto = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert proto is not None, name
        n_args = len(proto.group(1).split(','))
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args
        assert lib.SIGNATURES[name][1][2] is lib._L and lib.SIGNATURES[name][1][5] is lib._L      # the sample strides are 64-bit
        # the parent plus cand, ld_cand, n_sets, cand_set (and, for the ranker, the two constrained counts)
        assert n_args == len(lib.SIGNATURES[parent][1]) + (6 if 'rank' in name else 4)
