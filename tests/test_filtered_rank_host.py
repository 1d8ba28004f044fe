"""Filtered evaluation, host side (no GPU): the FilterIndex against a set-of-triplets definition, int64 keys on graphs whose
num_nodes * num_rels passes 2**31, argument checks of gv_rank_scores_filtered before any launch, and the --filtered-eval flag."""
import ctypes

import numpy as np
import pytest
import torch


def _answers(index, a, r, d):
    lo, hi = index.lookup(torch.tensor([a]), torch.tensor([r]), d)
    return index.ent[d][int(lo[0]):int(hi[0])].tolist()


def _check_against_sets(index, trip_sets, num_nodes, num_rels):
    known = {tuple(int(x) for x in t) for ts in trip_sets for t in np.asarray(ts).reshape(-1, 3)}
    by_o, by_s = {}, {}
    for s, r, o in known:
        by_o.setdefault((s, r), set()).add(o)
        by_s.setdefault((o, r), set()).add(s)
    for d, table in (('o', by_o), ('s', by_s)):
        keys = index.keys[d]
        assert keys.dtype == torch.int64 and index.ent[d].dtype == torch.int32
        assert bool((keys[1:] >= keys[:-1]).all())
        assert index.ent[d].numel() == len(known)
        for (a, r), want in table.items():
            assert _answers(index, a, r, d) == sorted(want)
        # every query of a few random (a, r), known or not, in one batched lookup
        gen = torch.Generator().manual_seed(3)
        qa, qr = torch.randint(0, num_nodes, (200,), generator=gen), torch.randint(0, num_rels, (200,), generator=gen)
        lo, hi = index.lookup(qa, qr, d)
        for i in range(200):
            got = index.ent[d][int(lo[i]):int(hi[i])].tolist()
            assert got == sorted(table.get((int(qa[i]), int(qr[i])), ()))


def test_filter_index_on_a_hand_made_kg():
    from gcn_vae_amd import ranking
    train = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 2], [3, 1, 0], [1, 0, 0]])     # (0, 0, 2) twice
    valid = np.array([[0, 0, 4], [2, 1, 3]])
    test = np.array([[0, 0, 1], [4, 1, 3]])                                         # (0, 0, 1) also in train
    idx = ranking.FilterIndex(5, 2, train, valid, test)
    assert _answers(idx, 0, 0, 'o') == [1, 2, 4]              # the query's own target (1) is in its list
    assert _answers(idx, 3, 1, 's') == [2, 4]
    assert _answers(idx, 0, 0, 's') == [1]
    assert _answers(idx, 1, 1, 'o') == []                     # a key with no entry: an empty range
    assert _answers(idx, 4, 1, 'o') == [3]
    _check_against_sets(idx, (train, valid, test), 5, 2)


def test_filter_index_on_a_synthetic_dataset():
    from gcn_vae_amd import data, ranking
    kg = data.load_data('synthetic:300:7:4000:300:300:5')
    idx = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cpu')
    _check_against_sets(idx, (kg.train, kg.valid, kg.test), kg.num_nodes, kg.num_rels)
    # Zipf endpoints: some keys hold many answers, most hold few
    lens = torch.unique_consecutive(idx.keys['o'], return_counts=True)[1]
    assert int(lens.max()) > 10 and int(lens.min()) == 1
    # a torch tensor as input gives the same index
    again = ranking.FilterIndex(kg.num_nodes, kg.num_rels, torch.from_numpy(np.concatenate([kg.train, kg.valid, kg.test])))
    for d in ('o', 's'):
        assert torch.equal(again.keys[d], idx.keys[d]) and torch.equal(again.ent[d], idx.ent[d])


def test_filter_index_keys_do_not_overflow_int32():
    from gcn_vae_amd import ranking
    n, r = 3_000_000, 1000                      # n * r = 3e9 > 2**31
    trip = np.array([[n - 1, r - 1, 5], [n - 1, r - 1, 7], [5, r - 1, n - 1], [2_500_000, 999, 1], [2_500_000, 998, 2]])
    idx = ranking.FilterIndex(n, r, trip)
    assert int(idx.keys['o'].max()) == (n - 1) * r + r - 1 > 2 ** 31
    assert _answers(idx, n - 1, r - 1, 'o') == [5, 7]
    assert _answers(idx, n - 1, r - 1, 's') == [5]
    assert _answers(idx, 2_500_000, 999, 'o') == [1]
    assert _answers(idx, 2_500_000, 998, 'o') == [2]
    assert _answers(idx, 2_500_000, 999, 's') == []
    with pytest.raises(ValueError):
        ranking.FilterIndex(10, 2, np.array([[0, 2, 1]]))     # relation out of range


def test_filtered_ranker_validates_arguments_before_any_launch():
    from gcn_vae_amd import lib
    l = lib.load()
    fn = l.gv_rank_scores_filtered
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    # q, ld_q, e, ld_e, target, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, tgt, count_raw, count_filt, m, v, h, stream
    assert fn(None, 8, None, 8, None, None, None, None, None, 0, None, None, None, 0, 10, 8, None) == 0   # m == 0: nothing to do
    assert fn(p, 8, p, 8, p, None, None, p, p, 1, p, None, p, 4, 10, 8, None) != 0
    assert 'NULL' in lib.last_error() and 'filter' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, None, p, 1, p, None, p, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, p, None, 1, p, None, p, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, p, p, 1, p, None, None, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(None, 8, p, 8, p, None, p, p, p, 1, p, None, p, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, p, p, 1, p, None, p, -1, 10, 8, None) != 0 and 'm=-1' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, p, p, 1, p, None, p, 4, 0, 8, None) != 0 and 'v=0' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, p, p, 1, p, None, p, 4, 10, 0, None) != 0 and 'h=0' in lib.last_error()
    assert fn(p, 8, p, 8, p, None, p, p, p, -1, p, None, p, 4, 10, 8, None) != 0 and 'n_filt_ent=-1' in lib.last_error()
    assert fn(p, 7, p, 8, p, None, p, p, p, 1, p, None, p, 4, 10, 8, None) != 0 and 'leading dimension' in lib.last_error()
    assert fn(p, 8, p, 4, p, None, p, p, p, 1, p, None, p, 4, 10, 8, None) != 0 and 'leading dimension' in lib.last_error()


def test_train_parser_has_filtered_eval_off_by_default():
    from gcn_vae_amd import train
    p = train.build_parser()
    base = p.parse_args(['-d', 'FB15k-237-synthetic'])
    assert base.filtered_eval is False
    on = p.parse_args(['-d', 'FB15k-237-synthetic', '--filtered-eval', '--gpu', '0'])
    assert on.filtered_eval is True and on.gpu == 0
    # every other flag parses as before, with or without the new one
    argv = ['-d', 'x', '--dropout', '0.1', '--n-hidden', '16', '--gpu', '0', '--lr', '0.01', '--n-bases', '4', '--n-layers', '3',
            '--n-epochs', '5', '--eval-batch-size', '7', '--regularization', '0.5', '--kl-param', '0.2', '--mmd-param', '1',
            '--mog-k', '3', '--n-flows', '2', '--grad-norm', '2', '--graph-batch-size', '100', '--graph-split-size', '0.4',
            '--negative-sample', '3', '--evaluate-every', '9', '--edge-sampler', 'neighbor', '--test-mode', 'True',
            '--model-state-file', 'm.pth', '--model-class', 'RGCN', '--load', 'True', '--generate', 'True', '--bf16',
            '--graph-step', '--device-sampler']
    a, b = vars(p.parse_args(argv)), vars(p.parse_args(argv + ['--filtered-eval']))
    assert b.pop('filtered_eval') is True and a.pop('filtered_eval') is False and a == b
    assert a['n_hidden'] == 16 and a['test_mode'] is True and a['edge_sampler'] == 'neighbor' and a['bf16'] and a['device_sampler']
