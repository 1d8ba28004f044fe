"""Monte-Carlo posterior-predictive ranking without a GPU: the definitions on materialised values (ranking.mc_mean_prob,
ranking.mc_ranks_from_probs) against a brute-force float64 loop and hand-computed cases, the --mc-samples flag's refusals, the
argument errors of KGVAE.posterior_samples that need no device, and the three gv_*_mc names in the header and the ctypes table."""
import math
import os
import re

import pytest
import torch

from gcn_vae_amd import lib, ranking, train
from gcn_vae_amd.encoders import KGVAE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


def test_mean_prob_and_ranks_against_a_brute_force_float64_loop():
    gen = torch.Generator().manual_seed(3)
    n_samples, n, h, n_rel, m = 3, 30, 5, 4, 12
    z = torch.randn(n_samples, n, h, generator=gen, dtype=torch.float64)
    w = torch.randn(n_rel, h, generator=gen, dtype=torch.float64)
    flp = torch.randn(n_samples, generator=gen, dtype=torch.float64)
    a = torch.randint(0, n, (m,), generator=gen)
    r = torch.randint(0, n_rel, (m,), generator=gen)
    b = torch.randint(0, n, (m,), generator=gen)
    listed = torch.rand(m, n, generator=gen) < 0.2
    listed[0, b[0]] = True                                            # a query that lists its own target
    for bias in (None, flp):
        pbar = ranking.mc_mean_prob(z, w, a, r, bias)
        assert pbar.dtype == torch.float64 and tuple(pbar.shape) == (m, n)
        want = torch.zeros(m, n, dtype=torch.float64)
        for i in range(m):
            for j in range(n):
                acc = 0.0
                for s in range(n_samples):
                    dot = sum(float(z[s, a[i], c]) * float(w[r[i], c]) * float(z[s, j, c]) for c in range(h))
                    acc += _sig(dot + (float(bias[s]) if bias is not None else 0.0))
                want[i, j] = acc / n_samples
        assert float((pbar - want).abs().max()) < 1e-14
        raw, filt = ranking.mc_ranks_from_probs(pbar, b, listed)
        for i in range(m):
            t = int(b[i])
            others = [j for j in range(n) if j != t]
            assert float(raw[i]) == sum(want[i, j] > want[i, t] for j in others)      # (no ties among random float64 values)
            assert float(filt[i]) == sum(want[i, j] > want[i, t] for j in others if not listed[i, j])
        assert ranking.mc_ranks_from_probs(pbar, b)[1] is None
    # float32 in, float32 out
    assert ranking.mc_mean_prob(z.float(), w.float(), a, r, flp.float()).dtype == torch.float32


def test_hand_computed_one_dimensional_cases():
    # h = 1, the query entity's value and the relation weight are 1: logit_s[j] = z[s, j]
    inf = float('inf')
    z = torch.tensor([[[1.0], [0.0], [2.0], [0.0], [-inf], [inf], [3.0]],
                      [[1.0], [2.0], [0.0], [2.0], [inf], [inf], [float('nan')]]], dtype=torch.float64)
    z[:, 0] = 1.0
    w = torch.ones(1, 1, dtype=torch.float64)
    a, r = torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long)
    pbar = ranking.mc_mean_prob(z, w, a, r)
    s0, s1, s2 = _sig(0.0), _sig(1.0), _sig(2.0)
    want = [s1, (s0 + s2) / 2, (s2 + s0) / 2, (s0 + s2) / 2, 0.5, 1.0]
    assert pbar[0, :6].tolist() == pytest.approx(want, abs=1e-15)
    assert pbar[0, 4].item() == 0.5 and pbar[0, 5].item() == 1.0      # -inf -> 0, +inf -> 1 in a sample
    assert math.isnan(pbar[0, 6].item())                               # a NaN in any sample makes pbar NaN
    assert pbar[0, 1].item() == pbar[0, 3].item()                      # the same two terms in the same order: an exact tie
    target = torch.tensor([1, 1, 6, 0])
    listed = torch.zeros(4, 7, dtype=torch.bool)
    listed[1, 3] = True                                                # query 1 lists the tie
    listed[1, 6] = True                                                # ... and the NaN candidate
    listed[3, 0] = True                                                # query 3 lists its own target: still ranked
    raw, filt = ranking.mc_ranks_from_probs(pbar, target, listed)
    # target 1 (0.5 (s0 + s2) = 0.690): above it 0 (s1 = 0.731), 5 (1.0) and the NaN; entities 3 and 2 (the same terms, for 2 in
    # the other order) tie; entity 2's vote is taken from the values themselves
    a2, e2 = float(pbar[0, 2] > pbar[0, 1]), float(pbar[0, 2] == pbar[0, 1])
    assert float(raw[0]) == 3 + a2 + 0.5 * (1 + e2)
    assert float(filt[0]) == float(raw[0])                             # nothing listed for query 0
    assert float(raw[1]) == float(raw[0]) and float(filt[1]) == 2 + a2 + 0.5 * e2      # the tie and the NaN left out
    assert float(raw[2]) == 6.0 and float(filt[2]) == 6.0              # a NaN target ranks last
    # target 0 (0.731): above it 5 (1.0) and the NaN only
    assert float(raw[3]) == 2.0 and float(filt[3]) == 2.0


def test_mc_samples_flag_and_its_refusals():
    p = train.build_parser()
    base = ['-d', 'synthetic:50:4:300:20:10:7']
    args = p.parse_args(base)
    assert args.mc_samples == 0 and args.mc_seed == 0 and args.mc_predict_out == 'mc_predictions.tsv'
    train.check_args(args)
    ok = p.parse_args(base + ['--mc-samples', '4', '--mc-seed', '7', '--test-mode', 'True', '--filtered-eval', '--predict-topk', '3'])
    assert ok.mc_samples == 4 and ok.mc_seed == 7
    train.check_args(ok)
    with pytest.raises(ValueError, match='--test-mode'):
        train.check_args(p.parse_args(base + ['--mc-samples', '4']))
    with pytest.raises(ValueError, match='deterministic'):
        train.check_args(p.parse_args(base + ['--mc-samples', '4', '--test-mode', 'True', '--model-class', 'RGCN']))
    with pytest.raises(ValueError, match='--type-constrain'):
        train.check_args(p.parse_args(base + ['--mc-samples', '4', '--test-mode', 'True', '--filtered-eval', '--type-constrain']))
    with pytest.raises(ValueError, match='--mc-samples'):
        train.check_args(p.parse_args(base + ['--mc-samples', '-1', '--test-mode', 'True']))


def test_posterior_samples_argument_errors_need_no_device():
    enc = KGVAE(30, 8, 8, 6, num_bases=2, k=2, n_flows=1)
    none = (None, None, None, None)
    enc.eval()
    with pytest.raises(ValueError, match='n_samples'):
        enc.posterior_samples(*none, 0)
    enc.train()
    with pytest.raises(RuntimeError, match='eval'):
        enc.posterior_samples(*none, 2)
    enc.eval()
    enc.row_part = object()
    with pytest.raises(NotImplementedError):
        enc.posterior_samples(*none, 2)


def test_mc_argument_errors_of_the_ranking_layer():
    z = torch.zeros(2, 5, 3)
    w = torch.zeros(1, 3)
    with pytest.raises(ValueError, match='per sample'):
        ranking.calc_mc_mrr(z, w, torch.zeros(1, 3, dtype=torch.long), flow_log_probs=torch.zeros(3), verbose=False)
    with pytest.raises(ValueError, match='posterior_samples'):
        ranking.calc_mc_mrr(z[0], w, torch.zeros(1, 3, dtype=torch.long), verbose=False)
    with pytest.raises(ValueError, match='direction'):
        ranking.predict_topk_mc(z, w, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), 2, direction='x')


def test_entry_points_in_the_header_and_the_ctypes_table():
    with open(os.path.join(ROOT, 'include', 'gcnvae.h')) as f:
        header = f.read()
    want = {'gv_rank_scores_mc': 20, 'gv_topk_scores_mc': 20, 'gv_pair_prob_std_mc': 15}
    for name, n_args in want.items():
        proto = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header)
        assert proto is not None, name
        assert len(proto.group(1).split(',')) == n_args
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args
        # the two sample strides are 64-bit
        assert lib.SIGNATURES[name][1][2] is lib._L and lib.SIGNATURES[name][1][5] is lib._L
    # the single-sample filtered ranker plus q_stride, e_stride, n_samples
    assert len(lib.SIGNATURES['gv_rank_scores_filtered'][1]) + 3 == want['gv_rank_scores_mc']
    assert len(lib.SIGNATURES['gv_topk_scores'][1]) + 3 == want['gv_topk_scores_mc']
