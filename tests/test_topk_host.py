"""Top-k link prediction, host side (no GPU): the order and padding rules of ranking.topk_from_scores on hand-written score
matrices, argument checks of ops.topk_scores / gv_topk_scores before any launch, and the --predict-topk / --predict-out flags."""
import ctypes

import pytest
import torch

NAN, INF = float('nan'), float('inf')


def _topk(rows, k, lists=None):
    from gcn_vae_amd import ranking
    score = torch.tensor(rows, dtype=torch.float32)
    if lists is None:
        return ranking.topk_from_scores(score, k)
    lens = torch.tensor([len(x) for x in lists])
    hi = torch.cumsum(lens, 0)
    ent = torch.tensor(sum(lists, []), dtype=torch.int64)
    return ranking.topk_from_scores(score, k, hi - lens, hi, ent)


def test_ties_go_by_id():
    ids, logits = _topk([[1.0, 3.0, 2.0, 3.0, 3.0], [5.0, 5.0, 5.0, 5.0, 5.0]], 4)
    assert ids.dtype == torch.int64 and logits.dtype == torch.float32
    assert ids.tolist() == [[1, 3, 4, 2], [0, 1, 2, 3]]
    assert logits.tolist() == [[3.0, 3.0, 3.0, 2.0], [5.0] * 4]


def test_signed_zeros_tie():
    ids, logits = _topk([[-0.0, 0.0, -1.0, -0.0, 0.5]], 5)
    assert ids.tolist() == [[4, 0, 1, 3, 2]]
    assert [str(x) for x in logits[0].tolist()] == ['0.5', '0.0', '0.0', '0.0', '-1.0']    # -0 reported as +0


def test_nan_last_and_after_minus_inf():
    ids, logits = _topk([[NAN, -INF, 2.0, NAN, INF, -3.0]], 6)
    assert ids.tolist() == [[4, 2, 5, 1, 0, 3]]
    got = logits[0].tolist()
    assert got[:4] == [INF, 2.0, -3.0, -INF] and all(x != x for x in got[4:])
    # every NaN comes out as the one quiet NaN
    odd = torch.tensor([[0.0, 1.0]]).view(torch.int32)
    odd[0, 0] = 0x7fa00001                                  # a signalling-pattern NaN
    from gcn_vae_amd import ranking
    _, lg = ranking.topk_from_scores(odd.view(torch.float32), 2)
    assert lg.view(torch.int32)[0, 1].item() == 0x7fc00000


def test_padding_when_fewer_candidates_than_k():
    ids, logits = _topk([[1.0, 2.0, 0.5]], 5)                # v < k
    assert ids.tolist() == [[1, 0, 2, -1, -1]]
    assert logits.tolist() == [[2.0, 1.0, 0.5, -INF, -INF]]
    # the filter leaves fewer than k: rows 0 and 1 list 3 resp. 4 of the 4 entities, row 2 none
    ids, logits = _topk([[4.0, 3.0, 2.0, 1.0], [1.0, 2.0, 3.0, 4.0], [NAN, 1.0, 1.0, -INF]], 3, [[0, 1, 3], [0, 1, 2, 3], []])
    assert ids.tolist() == [[2, -1, -1], [-1, -1, -1], [1, 2, 3]]
    assert logits[:2].tolist() == [[2.0, -INF, -INF], [-INF, -INF, -INF]]
    assert logits[2].tolist() == [1.0, 1.0, -INF]


def test_filter_removes_listed_ids_only():
    ids, _ = _topk([[9.0, 8.0, 7.0, 6.0, 5.0]] * 2, 2, [[0, 2], [4]])
    assert ids.tolist() == [[1, 3], [0, 1]]


def test_topk_scores_rejects_bad_arguments_before_any_launch():
    from gcn_vae_amd import ops
    q, e = torch.zeros(4, 8), torch.zeros(10, 8)
    lo, hi, ent = torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.long), torch.tensor([3])
    for k in (0, 129):
        with pytest.raises(ValueError, match='k must lie'):
            ops.topk_scores(q, e, k)
    with pytest.raises(ValueError, match='width'):
        ops.topk_scores(q, torch.zeros(10, 7), 5)
    with pytest.raises(ValueError, match='together'):
        ops.topk_scores(q, e, 5, None, lo, hi, None)
    with pytest.raises(ValueError, match='together'):
        ops.topk_scores(q, e, 5, None, None, None, ent)
    with pytest.raises(ValueError, match='one filter range'):
        ops.topk_scores(q, e, 5, None, lo[:3], hi[:3], ent)
    with pytest.raises(ValueError, match='filt_lo <= filt_hi'):
        ops.topk_scores(q, e, 5, None, hi, lo, ent)                  # inverted
    with pytest.raises(ValueError, match='filt_lo <= filt_hi'):
        ops.topk_scores(q, e, 5, None, lo, hi + 1, ent)              # past the end of the list
    with pytest.raises(ValueError, match='filt_lo <= filt_hi'):
        ops.topk_scores(q, e, 5, None, lo - 1, hi, ent)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.topk_scores(q, e, 5, None, lo, hi, ent + 7)              # id out of [0, v)
    with pytest.raises(ValueError, match=r'\[0, 10\)'):
        ops.topk_scores(q, e, 5, None, lo, hi, ent - 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):        # valid arguments: the device check, still no launch
        ops.topk_scores(q, e, 5, None, lo, hi, ent)


def test_c_entry_validates_arguments_before_any_launch():
    from gcn_vae_amd import lib
    l = lib.load()
    fn = l.gv_topk_scores
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    # q, ld_q, e, ld_e, bias, filt_lo, filt_hi, filt_ent, n_filt_ent, k, out_ids, out_logits, workspace, m, v, h, stream
    assert fn(None, 8, None, 8, None, None, None, None, 0, 5, None, None, None, 0, 10, 8, None) == 0    # m == 0
    assert fn(p, 8, p, 8, None, None, None, None, 0, 0, p, p, p, 4, 10, 8, None) != 0 and 'k=0' in lib.last_error()
    assert fn(p, 8, p, 8, None, None, None, None, 0, 129, p, p, p, 4, 10, 8, None) != 0 and 'k=129' in lib.last_error()
    assert fn(p, 8, p, 8, None, p, None, p, 1, 5, p, p, p, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(p, 8, p, 8, None, None, None, p, 1, 5, p, p, p, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(None, 8, p, 8, None, None, None, None, 0, 5, p, p, p, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(p, 8, p, 8, None, None, None, None, 0, 5, p, p, None, 4, 10, 8, None) != 0 and 'NULL' in lib.last_error()
    assert fn(p, 8, p, 8, None, None, None, None, 0, 5, p, p, p, -1, 10, 8, None) != 0 and 'm=-1' in lib.last_error()
    assert fn(p, 8, p, 8, None, None, None, None, 0, 5, p, p, p, 4, 0, 8, None) != 0 and 'v=0' in lib.last_error()
    assert fn(p, 8, p, 8, None, None, None, None, 0, 5, p, p, p, 4, 10, 0, None) != 0 and 'h=0' in lib.last_error()
    assert fn(p, 8, p, 8, None, p, p, p, -1, 5, p, p, p, 4, 10, 8, None) != 0 and 'n_filt_ent=-1' in lib.last_error()
    assert fn(p, 7, p, 8, None, None, None, None, 0, 5, p, p, p, 4, 10, 8, None) != 0 and 'leading dimension' in lib.last_error()
    ws = l.gv_topk_scores_workspace_bytes
    assert ws(0, 10, 5) == 0 and ws(4, 10, 0) == 0 and ws(4, 10, 129) == 0
    assert ws(4, 10, 5) == 4 * 5 * 8                                   # one span of one tile
    big = ws(40932, 14541, 10)
    assert big >= 40932 * 10 * 8 and big % (40932 * 10 * 8) == 0


def test_parser_has_predict_topk_and_keeps_every_other_default():
    from gcn_vae_amd import train
    p = train.build_parser()
    base = p.parse_args(['-d', 'FB15k-237-synthetic'])
    assert base.predict_topk == 0 and base.predict_out == 'predictions.tsv'
    on = p.parse_args(['-d', 'x', '--test-mode', 'True', '--predict-topk', '10', '--predict-out', 'p.tsv'])
    assert on.predict_topk == 10 and on.predict_out == 'p.tsv' and on.test_mode is True
    ref = dict(dropout=0.2, n_hidden=500, gpu=-1, lr=1e-3, n_bases=100, n_layers=2, n_epochs=1e5, eval_batch_size=400,
               regularization=0.01, kl_param=1e-5, mmd_param=0, mog_k=10, n_flows=0, grad_norm=1.0, graph_batch_size=20000,
               graph_split_size=0.5, negative_sample=10, evaluate_every=200, edge_sampler='uniform', test_mode=False,
               model_state_file='model_state.pth', model_class='KGVAE', load=False, generate=False, bf16=False,
               graph_step=False, device_sampler=False, filtered_eval=False)
    got = vars(base)
    for k, v in ref.items():
        assert got[k] == v, k
