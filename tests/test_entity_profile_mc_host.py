"""Per-entity completion on the posterior predictive without a GPU: the two C entries' place in the signature table and their
host-side refusals (return codes, nothing launched), the wrappers' argument errors that need no device, the rule of the
materialised route on hand-made probabilities (ranking.complete_entities_mc_from_probs) and the --mc-profile flag checks."""
import ctypes

import pytest
import torch

from gcn_vae_amd import lib, ops, ranking, train

SHAPE, NULL = -2, -1
ENTRIES = ('gv_entity_topk_scores_mc', 'gv_entity_topk_scores_typed_mc')


def test_both_entries_are_in_the_signature_table():
    for entry, parent, n_args in ((ENTRIES[0], 'gv_entity_topk_scores', 25), (ENTRIES[1], 'gv_entity_topk_scores_typed', 30)):
        res, args = lib.SIGNATURES[entry]
        assert res is ctypes.c_int and len(args) == n_args == len(lib.SIGNATURES[parent][1]) + 2
        # e_stride (after ld_e) and workspace_bytes (fifth from the end) are the two 64-bit integers
        assert [i for i, a in enumerate(args) if a is ctypes.c_int64] == [4, n_args - 5]
        # the parent's arguments with (e_stride, n_samples) put in after ld_e
        assert args[:4] + args[6:] == lib.SIGNATURES[parent][1] and args[5] is ctypes.c_int
        assert hasattr(lib.load(), entry)


def _callers():
    l = lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def untyped(ents=p, m=4, e=p, ld_e=8, e_stride=80, n_samples=2, w=p, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, k=5, span=0, rel=p,
                other=p, val=p, ws=p, ws_bytes=1 << 20, n=10, num_rels=3, h=8, **typed):
        assert not typed
        return l.gv_entity_topk_scores_mc(ents, m, e, ld_e, e_stride, n_samples, w, ld_w, None, lo, hi, ent, n_ent, 1, k, span, rel, other,
                                          val, ws, ws_bytes, n, num_rels, h, None)

    def typed(ents=p, m=4, e=p, ld_e=8, e_stride=80, n_samples=2, w=p, ld_w=8, lo=None, hi=None, ent=None, n_ent=0, set_ptr=p, set_ids=p,
              tile_ptr=p, n_tiles=5, cand_base=0, k=5, span=0, rel=p, other=p, val=p, ws=p, ws_bytes=1 << 20, n=10, num_rels=3, h=8):
        return l.gv_entity_topk_scores_typed_mc(ents, m, e, ld_e, e_stride, n_samples, w, ld_w, None, lo, hi, ent, n_ent, set_ptr, set_ids,
                                                tile_ptr, n_tiles, cand_base, 1, k, span, rel, other, val, ws, ws_bytes, n, num_rels, h,
                                                None)
    return p, ((ENTRIES[0], untyped), (ENTRIES[1], typed))


def test_the_entries_refuse_bad_arguments_before_any_launch():
    p, callers = _callers()
    for entry, call in callers:
        assert call(m=0) == 0 and call(m=0, n_samples=1, e_stride=0) == 0           # no query entity: nothing to do
        for kw, code, text in ((dict(n_samples=0), SHAPE, 'n_samples=0'), (dict(n_samples=-3), SHAPE, 'n_samples=-3'),
                               (dict(e_stride=79), SHAPE, 'e_stride=79'), (dict(e_stride=0), SHAPE, 'e_stride=0'),
                               (dict(ld_e=12, e_stride=115), SHAPE, 'e_stride=115'),       # (n - 1) * ld_e + h = 116
                               (dict(k=0), SHAPE, 'k=0'), (dict(k=129), SHAPE, 'k=129'),
                               (dict(n=1 << 16, num_rels=1 << 15, e_stride=1 << 20), SHAPE, '31 bits'),
                               (dict(ws_bytes=4 * 5 * 8 - 1), SHAPE, 'workspace'), (dict(span=-1), SHAPE, 'span_tiles=-1'),
                               (dict(lo=p), NULL, 'all given or all NULL'), (dict(lo=p, hi=p), NULL, 'all given or all NULL'),
                               (dict(ld_e=7), SHAPE, 'leading dimension'), (dict(ld_w=7), SHAPE, 'leading dimension'),
                               (dict(h=0), SHAPE, 'h=0'), (dict(m=-1), SHAPE, 'm=-1'), (dict(e=None), NULL, 'NULL pointer'),
                               (dict(ents=None), NULL, 'NULL pointer'), (dict(val=None), NULL, 'NULL pointer')):
            assert call(**kw) == code, (entry, kw)
            assert lib.last_error().startswith(entry + ':') and text in lib.last_error(), (entry, kw, lib.last_error())
        # one sample needs no stride; the geometry is reported ahead of the filter, and the sizes ahead of the geometry
        assert call(n_samples=1, e_stride=0, ws_bytes=0) == SHAPE and 'workspace' in lib.last_error()
        assert call(n_samples=0, lo=p) == SHAPE and 'n_samples' in lib.last_error()
        assert call(n_samples=0, k=0) == SHAPE and 'k=0' in lib.last_error()
    entry, typed = callers[1]
    for kw, code, text in ((dict(cand_base=1), SHAPE, 'cand_base=1'), (dict(cand_base=-1), SHAPE, 'cand_base=-1'),
                           (dict(n_tiles=-1), SHAPE, 'n_tiles=-1'), (dict(set_ptr=None), NULL, 'NULL set_ptr'),
                           (dict(tile_ptr=None), NULL, 'NULL set_ptr')):
        assert typed(**kw) == code and lib.last_error().startswith(entry + ':') and text in lib.last_error(), kw
    assert typed(cand_base=3, ws_bytes=0) == SHAPE and 'workspace' in lib.last_error()       # cand_base = R itself passes
    assert typed(cand_base=1, n_samples=0) == SHAPE and 'cand_base' in lib.last_error()      # the sets' shape ahead of the samples


def _members(n, num_rels):
    return ranking.TypeConstraint(n, num_rels, [[1, 0, 2], [4, 2, 4], [3, 1, 0]]).members()


def test_ops_wrappers_refuse_before_any_device_is_touched():
    z, w, ents = torch.zeros(2, 10, 8), torch.zeros(3, 8), torch.tensor([4, 1, 4])
    ptr, ids = _members(10, 3)
    for call in (lambda z_, *a, **kw: ops.entity_topk_scores_mc(ents, z_, w, *a, **kw),
                 lambda z_, k, *a, **kw: ops.entity_topk_scores_typed_mc(ents, z_, w, k, ptr, ids, 's', *a, **kw)):
        for bad in (z[0], torch.zeros(0, 10, 8), [z]):
            with pytest.raises(TypeError, match='3-D'):
                call(bad, 5)
        with pytest.raises(ValueError, match='width'):
            call(z[:, :, :7], 5)
        for k in (0, 129):
            with pytest.raises(ValueError, match='k must lie'):
                call(z, k)
        with pytest.raises(ValueError, match='span'):
            call(z, 5, span=0)
        with pytest.raises(ValueError, match='together'):
            call(z, 5, None, torch.zeros(30, dtype=torch.long))
        with pytest.raises(RuntimeError, match='no CPU fallback'):           # valid arguments: the device check, no launch
            call(z, 5)
        with pytest.raises(RuntimeError, match='no CPU fallback'):           # (the per-sample bias is looked at on the device only)
            call(z, 5, torch.zeros(3))
    with pytest.raises(TypeError, match='1-D integer'):
        ops.entity_topk_scores_mc(ents.float(), z, w, 5)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.entity_topk_scores_mc(torch.tensor([4, 10]), z, w, 5)
    with pytest.raises(ValueError, match='31 bits'):
        ops.entity_topk_scores_mc(ents, torch.zeros(1, 1 << 16, 1), torch.zeros(1 << 15, 1), 5)
    with pytest.raises(ValueError, match='one value per sample'):
        ops._mc_bias_arg(torch.zeros(3), 2, 'cpu')


def test_ranking_wrappers_refuse_before_any_device_is_touched():
    z, w, ents = torch.zeros(2, 10, 8), torch.zeros(3, 8), torch.tensor([4, 1, 4])
    good = ranking.TypeConstraint(10, 3, [[1, 0, 2]])
    for route in (ranking.complete_entities_mc, ranking.complete_entities_mc_unfused):
        for bad in (None, 'typed', good.words):                                # an explicit None too: ahead of every other check
            with pytest.raises(TypeError, match='type_constraint'):
                route(z, w, ents, 5, side='x', type_constraint=bad)
        with pytest.raises(ValueError, match='side'):
            route(z, w, ents, 5, side='x')
        for k in (0, 129):
            with pytest.raises(ValueError, match='k must lie'):
                route(z, w, ents, k)
        with pytest.raises(ValueError, match='posterior_samples'):
            route(z[0], w, ents, 5)
        with pytest.raises(ValueError, match='per sample'):
            route(z, w, ents, 5, flow_log_probs=torch.zeros(3))
        with pytest.raises(ValueError, match='width'):
            route(z, w[:, :7], ents, 5)
        with pytest.raises(TypeError, match='1-D integer'):
            route(z, w, ents.float(), 5)
        for tc in (ranking.TypeConstraint(11, 3, [[1, 0, 2]]), ranking.TypeConstraint(10, 4, [[1, 0, 2]])):
            with pytest.raises(ValueError, match='the TypeConstraint is for'):
                route(z, w, ents, 5, type_constraint=tc)
    for kw in (dict(), dict(type_constraint=good), dict(side='o', type_constraint=good)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):             # the right arguments: the device check, no launch
            ranking.complete_entities_mc(z, w, ents, 5, **kw)


def test_the_materialised_rule_on_hand_made_probabilities():
    nan = float('nan')
    # probs[s, i, r, x]: two samples, the entities 2 and 0, two relations, four entities
    p0 = torch.tensor([[[1.0, 0.5, 0.9, 1.0], [0.25, 1.0, 0.1, 0.5]],
                       [[0.3, 0.5, 0.5, nan], [0.0, 0.75, 0.5, 0.5]]])
    p1 = torch.tensor([[[1.0, 0.5, 0.1, 1.0], [0.75, 1.0, 0.3, 0.0]],
                       [[0.7, 0.0, 0.5, 0.2], [0.5, 0.25, 0.5, 0.5]]])
    probs = torch.stack([p0, p1])
    pbar = (p0 + p1) * 0.5
    ents = torch.tensor([2, 0])
    rel, other, mean, std = ranking.complete_entities_mc_from_probs(pbar, probs, ents, 5)
    # entity 2 (its loops (r, 2) left out): the saturated 1.0s tie and go by relation, then entity; then the 0.5s the same way
    assert list(zip(rel[0].tolist(), other[0].tolist())) == [(0, 0), (0, 3), (1, 1), (0, 1), (1, 0)]
    assert mean[0].tolist() == [1.0, 1.0, 1.0, 0.5, 0.5]
    assert torch.allclose(std[0], torch.tensor([0.0, 0.0, 0.0, 0.0, 0.25]))
    # entity 0: 0.5 four times over -- (0, 2), (1, 1), (1, 2), (1, 3) by relation, then entity -- then 0.25; the NaN comes last
    assert list(zip(rel[1].tolist(), other[1].tolist())) == [(0, 2), (1, 1), (1, 2), (1, 3), (0, 1)]
    assert mean[1].tolist() == [0.5, 0.5, 0.5, 0.5, 0.25]
    assert torch.allclose(std[1], torch.tensor([0.0, 0.25, 0.0, 0.0, 0.25]))
    rel, other, mean, std = ranking.complete_entities_mc_from_probs(pbar, probs, ents, 7)
    assert (rel[1, 5].item(), other[1, 5].item()) == (0, 3) and mean[1, 5].isnan() and std[1, 5].isnan()      # NaN after every number
    assert rel[1, 6].item() == -1 and other[1, 6].item() == -1 and mean[1, 6].item() == float('-inf') and std[1, 6].item() == 0.0
    assert (rel[0] >= 0).sum().item() == 6 and std[0, 6].item() == 0.0                                         # padding: std 0
    # the loops kept, a filter (entity 2 lists entity 0 under relation 0) and the typed masks
    rel, other, mean, std = ranking.complete_entities_mc_from_probs(pbar, probs, ents, 3, exclude_self=False)
    assert list(zip(rel[0].tolist(), other[0].tolist())) == [(0, 0), (0, 3), (1, 1)]
    lo, hi = torch.zeros(8, dtype=torch.long), torch.zeros(8, dtype=torch.long)
    hi[2 * 2 + 0:] = 1
    lo[2 * 2 + 1:] = 1
    rel, other, mean, _ = ranking.complete_entities_mc_from_probs(pbar, probs, ents, 2, filt_lo=lo, filt_hi=hi, filt_ent=torch.tensor([0]))
    assert list(zip(rel[0].tolist(), other[0].tolist())) == [(0, 3), (1, 1)]
    cq = torch.tensor([[True, False, False, False], [True, False, True, False]])
    co = torch.tensor([[True, True, True, True], [False, False, True, True]])
    rel, other, mean, std = ranking.complete_entities_mc_from_probs(pbar, probs, ents, 3, cand_query=cq, cand_other=co)
    assert list(zip(rel[0].tolist(), other[0].tolist())) == [(1, 3), (-1, -1), (-1, -1)] and mean[0, 0].item() == 0.25
    assert abs(std[0, 0].item() - 0.25) < 1e-7 and std[0, 1:].tolist() == [0.0, 0.0]
    assert list(zip(rel[1].tolist(), other[1].tolist())) == [(0, 2), (1, 2), (1, 3)]


def test_mc_profile_flag_and_its_refusals():
    p = train.build_parser()
    base = ['-d', 'synthetic:50:4:300:20:10:7']
    mc = ['--mc-samples', '3', '--test-mode', 'True']
    args = p.parse_args(base)
    assert args.mc_profile is False and args.mc_profile_out == 'mc_profiles.tsv'
    ok = p.parse_args(base + mc + ['--profile-topk', '5', '--mc-profile', '--mc-profile-out', 'x.tsv', '--profile-entities', '3,1'])
    assert ok.mc_profile is True and ok.mc_profile_out == 'x.tsv'
    train.check_args(ok)
    train.check_args(p.parse_args(base + mc + ['--profile-topk', '5', '--profile-typed', '--mc-profile']))
    with pytest.raises(ValueError, match='--mc-profile.*--mc-samples'):
        train.check_args(p.parse_args(base + ['--test-mode', 'True', '--profile-topk', '5', '--mc-profile']))
    with pytest.raises(ValueError, match='--mc-profile.*--profile-topk'):
        train.check_args(p.parse_args(base + mc + ['--mc-profile']))
    with pytest.raises(ValueError, match='--profile-topk'):                    # --profile-typed's own refusal comes first
        train.check_args(p.parse_args(base + mc + ['--profile-typed', '--mc-profile']))
    with pytest.raises(ValueError, match='--test-mode'):
        train.check_args(p.parse_args(base + ['--mc-samples', '3', '--profile-topk', '5', '--mc-profile']))
    with pytest.raises(ValueError, match='deterministic'):
        train.check_args(p.parse_args(base + mc + ['--model-class', 'RGCN', '--profile-topk', '5', '--mc-profile']))
    with pytest.raises(ValueError, match='at most 128'):
        train.check_args(p.parse_args(base + mc + ['--profile-topk', '129', '--mc-profile']))
    # without the flag the existing flag sets check as before
    for flags in ([], ['--test-mode', 'True', '--profile-topk', '5'], mc + ['--profile-topk', '5', '--profile-typed'],
                  mc + ['--predict-topk', '3', '--filtered-eval']):
        args = p.parse_args(base + flags)
        assert args.mc_profile is False
        train.check_args(args)


def test_the_transe_cli_has_no_monte_carlo_flags():
    from gcn_vae_amd import transe
    with pytest.raises(SystemExit):
        transe.build_parser().parse_args(['-d', 'x', '--mc-profile'])
