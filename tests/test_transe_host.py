"""TransE host rules (no GPU): the plain-torch step against the reference fixture, the model's keys and seeded init, the
sampler's mappings, the CLI defaults of baselines/transe/main.py and argument refusals."""
import os

import numpy as np
import pytest
import torch

from gcn_vae_amd import ops, transe

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'transe.npz'))
CASES = ['p1_norm', 'p1_raw', 'p2_norm', 'p2_raw', 'adv', 'regul', 'tie']


def case(tag):
    cfg = GOLD[f'{tag}.cfg']
    B, K, p, nf = int(cfg[0]), int(cfg[1]), int(cfg[2]), bool(cfg[3])
    return dict(ent=torch.from_numpy(GOLD[f'{tag}.ent']), rel=torch.from_numpy(GOLD[f'{tag}.rel']),
                bh=torch.from_numpy(GOLD[f'{tag}.bh']), br=torch.from_numpy(GOLD[f'{tag}.br']), bt=torch.from_numpy(GOLD[f'{tag}.bt']),
                B=B, K=K, p=p, nf=nf, margin=float(cfg[4]), adv=float(cfg[5]) or None, regul=float(cfg[6]), lr=float(cfg[7]))


@pytest.mark.parametrize('tag', CASES)
def test_unfused_step_equals_reference_fixture(tag):
    c = case(tag)
    score, loss, g_ent, g_rel = transe.step_unfused(c['ent'], c['rel'], c['bh'], c['br'], c['bt'], c['B'], c['p'], c['nf'],
                                                    c['margin'], c['adv'], c['regul'])
    torch.testing.assert_close(score, torch.from_numpy(GOLD[f'{tag}.score']), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(loss, torch.tensor(float(GOLD[f'{tag}.loss'])), rtol=1e-6, atol=1e-6)
    assert_rows_close(g_ent, torch.from_numpy(GOLD[f'{tag}.g_ent']), 'g_ent')
    assert_rows_close(g_rel, torch.from_numpy(GOLD[f'{tag}.g_rel']), 'g_rel')


def assert_rows_close(got, ref, what, tol=1e-5):
    """|got - ref| <= tol * (max |ref| of the row + 1e-6) elementwise.  Row-wise: under norm_flag the all-zero entity row's
    gradient is gy / 1e-12 (~1e11); a tensor-wide scale would leave the other rows unchecked."""
    err = (got.double() - ref.double()).abs()
    bound = tol * (ref.double().abs().amax(dim=1, keepdim=True) + 1e-6)
    assert bool((err <= bound).all()), f'{what}: worst excess {float((err - bound).max()):.3e}'


@pytest.mark.parametrize('tag', ['p1_norm', 'p2_norm', 'adv', 'regul'])
def test_row_bound_sees_ordinary_rows_next_to_the_zero_row(tag):
    c = case(tag)
    _, _, g_ent, _ = transe.step_unfused(c['ent'], c['rel'], c['bh'], c['br'], c['bt'], c['B'], c['p'], c['nf'], c['margin'],
                                         c['adv'], c['regul'])
    ref = torch.from_numpy(GOLD[f'{tag}.g_ent'])
    assert float(ref[0].abs().max()) > 1e9 and float(ref[1:].abs().max()) < 10     # the zero row dwarfs the others
    assert_rows_close(g_ent, ref, 'g_ent')
    zeroed = g_ent.clone()
    zeroed[1:] = 0.0
    scaled = g_ent.clone()
    scaled[1:] *= 1.01
    for bad in (zeroed, scaled, -3 * g_ent):
        with pytest.raises(AssertionError):
            assert_rows_close(bad, ref, 'perturbed g_ent')


def test_tie_and_zero_row_in_fixture():
    c = case('tie')
    s = torch.from_numpy(GOLD['tie.score'])
    assert float(s[0] - s[c['B']]) == -c['margin']             # an exact hinge tie at pair (0, 0)
    assert float(s[1]) == 0.0                                  # a zero difference (positive 1)
    assert not GOLD['p1_norm.ent'][0].any() and GOLD['p1_norm.bh'][0] == 0


def test_state_dict_keys_and_seeded_init():
    torch.manual_seed(0)
    m = transe.TransE(12, 4, dim=16, p_norm=1, norm_flag=True)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD['state_keys']]
    assert torch.equal(sd['ent_embeddings.weight'], torch.from_numpy(GOLD['seed.ent']))
    assert torch.equal(sd['rel_embeddings.weight'], torch.from_numpy(GOLD['seed.rel']))
    m2 = transe.TransE(12, 4, dim=16)
    m2.load_state_dict(sd)                                     # a reference checkpoint's dict loads


def test_model_refuses_margin_epsilon_and_p():
    with pytest.raises(ValueError):
        transe.TransE(5, 2, margin=1.0)
    with pytest.raises(ValueError):
        transe.TransE(5, 2, epsilon=1.0)
    with pytest.raises(ValueError):
        transe.TransE(5, 2, p_norm=3)


@pytest.mark.parametrize('seed', range(5))
def test_nth_unlisted_equals_brute_force(seed):
    rs = np.random.RandomState(seed)
    v = rs.randint(1, 40)
    for k in [0, 1, v // 2, v - 1, v]:
        listed = np.sort(rs.choice(v, size=k, replace=False))
        free = [e for e in range(v) if e not in set(listed.tolist())]
        assert [transe.nth_unlisted(listed, u) for u in range(v - k)] == free
    assert transe.nth_unlisted(np.arange(v), 0) == v            # k == V: nothing left below V


def test_map_draw_range():
    assert transe.map_draw(0, 7) == 0 and transe.map_draw(0xFFFFFFFF, 7) == 6


def test_bern_probabilities():
    # relation 0: one head, three tails (1-to-N): tph 3, hpt 1 -> head corrupted with 3/4; relation 1: N-to-1 -> 1/4
    train = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 3], [1, 1, 9], [2, 1, 9], [3, 1, 9]])
    p = transe.bern_head_prob(train, 3)
    assert p.dtype == torch.float32
    assert float(p[0]) == 0.75 and float(p[1]) == 0.25 and float(p[2]) == 0.5


def test_sample_from_draws_layout_and_filter():
    train = np.array([[0, 0, 1], [0, 0, 2], [3, 1, 4]])
    tf = transe.TrainFilter(train, 6, 2, 'cpu')
    draws = np.zeros((2, 2 + 3), dtype=np.uint32)
    draws[:, 2:] = [0, 0x80000000, 0xFFFFFFFF]
    bh, br, bt = transe.sample_from_draws(draws, train, 6, 2, 3, None, tf)
    # word 0 -> triple 0, the tail replaced; (0, 0, ?) knows tails {1, 2}: the 4 free tails are 0, 3, 4, 5
    assert (bh == 0).all() and (br == 0).all()
    assert bt.tolist() == [1, 1, 0, 0, 4, 4, 5, 5]
    bh, br, bt = transe.sample_from_draws(draws, train, 6, 2, 3, None, None)
    assert bt.tolist() == [1, 1, 0, 0, 3, 3, 5, 5]             # unfiltered: onto all 6


def test_cli_defaults_match_main_py():
    a = transe.build_parser().parse_args(['-d', 'FB15k-237-synthetic'])
    assert (a.dim, a.p_norm, a.norm_flag, a.margin, a.nbatches, a.neg_ent, a.bern_flag, a.filter_flag, a.train_times, a.alpha,
            a.opt_method, a.neg_rel) == (200, 1, 1, 5.0, 100, 25, 1, 1, 1000, 1.0, 'sgd', 0)


@pytest.mark.parametrize('extra', [['--opt-method', 'adam'], ['--neg-rel', '1'], ['--p-norm', '3'], ['--adv-temperature', '0'],
                                   ['--dim', '1000']])
def test_cli_refuses_unsupported(extra):
    a = transe.build_parser().parse_args(['-d', 'x'] + extra)
    with pytest.raises(ValueError):
        transe.main(a)


def test_ops_argument_checks_raise_before_launch():
    cpu = torch.zeros(4, 8)
    i = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.transe_step(cpu, cpu, i, i, i, 4, 1, 1, True, 1.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.transe_distances(cpu, cpu, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.transe_rank_filtered(cpu, cpu, torch.zeros(4, dtype=torch.long), 2)
    with pytest.raises(ValueError):
        ops._p_norm(3)
