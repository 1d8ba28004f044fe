"""The TransE optimisers' host side (no GPU): the CLI's --optimizer / --weight-decay / --lr-decay and their refusals, the argument
checks of ops.transe_apply_opt, and transe.apply_unfused (index_add_ + a real torch.optim step) against a hand-written float64
statement of the four rules gv_transe_apply_opt implements -- which pins that those rules are torch's."""
import pytest
import torch

import transe_opt_cases as oc
from gcn_vae_amd import ops, transe


def parse(*extra):
    return transe.build_parser().parse_args(['-d', 'x', *extra])


def test_new_flags_parse_with_sgd_defaults():
    a = parse()
    assert (a.optimizer, a.weight_decay, a.lr_decay, a.opt_method, a.alpha) == ('sgd', 0.0, 0.0, 'sgd', 1.0)
    transe.check_args(a)
    a = parse('--optimizer', 'Adagrad', '--weight-decay', '0.01', '--lr-decay', '0.05', '--alpha', '0.5')
    assert (a.optimizer, a.weight_decay, a.lr_decay, a.alpha) == ('Adagrad', 0.01, 0.05, 0.5)
    transe.check_args(a)
    for name in ('sgd', 'adagrad', 'adadelta', 'adam', 'ADAM'):
        transe.check_args(parse('--optimizer', name, '--weight-decay', '0.1'))


@pytest.mark.parametrize('extra, match', [
    (['--optimizer', 'rmsprop'], '--optimizer'),
    (['--weight-decay', '-0.1'], '--weight-decay'),
    (['--optimizer', 'adagrad', '--lr-decay', '-1'], '--lr-decay'),
    (['--lr-decay', '0.1'], 'adagrad'),
    (['--optimizer', 'adam', '--lr-decay', '0.1'], 'adagrad'),
    (['--optimizer', 'adam', '--alpha', '-1'], '--alpha'),
    (['--opt-method', 'adam'], '--optimizer'),
    (['--opt-method', 'Adagrad', '--optimizer', 'adagrad'], '--optimizer'),
])
def test_check_args_refuses(extra, match):
    with pytest.raises(ValueError, match=match):
        transe.check_args(parse(*extra))
    with pytest.raises(ValueError, match=match):
        transe.main(parse(*extra))


def test_make_optimizer_builds_the_reference_trainers_choice():
    p = [torch.zeros(2, 3, requires_grad=True)]
    for name, cls in (('SGD', torch.optim.SGD), ('adagrad', torch.optim.Adagrad), ('Adadelta', torch.optim.Adadelta),
                      ('adam', torch.optim.Adam)):
        opt = transe.make_optimizer(p, name, 0.25, 0.01, 0.05 if cls is torch.optim.Adagrad else 0.0)
        assert type(opt) is cls and opt.defaults['lr'] == 0.25 and opt.defaults['weight_decay'] == 0.01
    assert transe.make_optimizer(p, 'adagrad', 1.0, 0.0, 0.05).defaults['lr_decay'] == 0.05
    with pytest.raises(ValueError, match='opt_method'):
        transe.make_optimizer(p, 'lion')


def apply_args(n_ent=6, n_rel=3, dim=8, state_shape=None):
    ent, rel = torch.zeros(n_ent, dim), torch.zeros(n_rel, dim)
    order = [dict(n=4, n_seg=n_ent), dict(n=2, n_seg=n_rel)]
    state = ops.TransEOptState(*(state_shape or (n_ent, n_rel, dim)), 'cpu')
    return (ent, rel, torch.zeros(4, dim), torch.zeros(2, dim), order), (torch.zeros(2), 5.0, torch.zeros(1)), state


def test_apply_opt_argument_checks_raise_before_launch():
    head, tail, state = apply_args()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.transe_apply_opt(*head, 'adam', 0.01, *tail, state=state)
    for bad in ('rmsprop', 3, None):
        with pytest.raises(ValueError, match='method'):
            ops.transe_apply_opt(*head, bad, 0.01, *tail, state=state)
    for kw in (dict(lr=-1.0), dict(lr=float('nan')), dict(weight_decay=-0.1), dict(lr_decay=-0.1)):
        args = dict(lr=0.01, weight_decay=0.0, lr_decay=0.0)
        args.update(kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.transe_apply_opt(*head, 'adagrad', args.pop('lr'), *tail, state=state, **args)
    with pytest.raises(ValueError, match='lr_decay'):
        ops.transe_apply_opt(*head, 'adam', 0.01, *tail, state=state, lr_decay=0.1)
    with pytest.raises(TypeError, match='state'):
        ops.transe_apply_opt(*head, 'adam', 0.01, *tail, state=None)
    for shape, what in (((7, 3, 8), r'state\.ent'), ((6, 4, 8), r'state\.rel'), ((6, 3, 9), r'state\.ent')):
        with pytest.raises(ValueError, match=what):
            ops.transe_apply_opt(*head, 'adam', 0.01, *tail, state=apply_args(state_shape=shape)[2])
    assert int(state.t) == 0                      # nothing ran: the step number did not move


def test_state_holder_zero_snapshot_restore_in_place():
    st = ops.TransEOptState(4, 2, 3, 'cpu')
    assert [tuple(x.shape) for x in st.tensors()] == [(4, 3), (4, 3), (2, 3), (2, 3), (1,)] and st.t.dtype == torch.int64
    ptrs = [x.data_ptr() for x in st.tensors()]
    for i, x in enumerate(st.tensors()):
        x.fill_(i + 1)
    snap = st.snapshot()
    st.zero_()
    assert all(float(x.abs().sum()) == 0 for x in st.tensors())
    st.restore(snap)
    assert [float(x.reshape(-1)[0]) for x in st.tensors()] == [1, 2, 3, 4, 5]
    assert [x.data_ptr() for x in st.tensors()] == ptrs


def test_trainer_refuses_bad_optimiser_arguments_before_touching_the_device():
    for kw, match in ((dict(opt_method='lion'), 'opt_method'), (dict(weight_decay=-1.0), 'weight_decay'),
                      (dict(opt_method='adam', lr_decay=0.1), 'lr_decay'), (dict(opt_method='adam', alpha=-1.0), 'alpha')):
        with pytest.raises(ValueError, match=match):
            transe.DeviceTrainer(None, None, **kw)


@pytest.mark.parametrize('method', oc.METHODS)
def test_apply_unfused_float64_equals_the_hand_statement(method):
    """Three steps with weight_decay = 0.01 (and lr_decay = 0.05 for Adagrad): tables and state to 1e-12 relative -- a handful of
    float64 operations an element.  And without either, so that a rule that only differs through them is pinned too."""
    c = oc.make_case(*oc.SHAPES[1])
    for wd, ld in ((0.01, 0.05 if method == 'adagrad' else 0.0), (0.0, 0.0)):
        got = oc.unfused_steps(c, method, wd, ld, torch.float64)
        want = oc.hand_steps(c, method, wd, ld, torch.float64)
        for step, (g, w) in enumerate(zip(got, want), 1):
            pairs = [('ent', g[0], w[0]), ('rel', g[1], w[1])]
            for i in range(len(oc.STATE_KEYS[method])):
                pairs += [(f'ent state {i}', g[2][i], w[2][i]), (f'rel state {i}', g[3][i], w[3][i])]
            for what, a, b in pairs:
                assert a.dtype == torch.float64
                err = (a - b).abs()
                assert bool((err <= 1e-12 * b.abs().clamp_min(1e-300)).all()), f'{method} wd={wd} step {step} {what}: {float(err.max()):.3e}'
        assert not torch.equal(got[-1][0], c['ent'].double())


def test_the_wrong_variants_differ_from_torch():
    """The three broken rules of ``hand_step`` are not torch's: each leaves the hand statement's agreement with torch.optim."""
    c = oc.make_case(*oc.SHAPES[1])
    for method, wrong in (('adam', 'adam_no_bias_correction'), ('adagrad', 'adagrad_no_lr_decay'), ('adadelta', 'adadelta_eps_outside')):
        ld = 0.05 if method == 'adagrad' else 0.0
        good = oc.unfused_steps(c, method, 0.01, ld, torch.float64)[-1][0]
        bad = oc.hand_steps(c, method, 0.01, ld, torch.float64, wrong)[-1][0]
        assert float((good - bad).abs().max()) > 1e-3


def test_apply_unfused_keeps_dtype_and_takes_int32_ids():
    c = oc.make_case(*oc.SHAPES[0])
    st = c['steps'][0]
    ent, rel = c['ent'].clone(), c['rel'].clone()
    opt = transe.make_optimizer([ent, rel], 'sgd', 0.5)
    transe.apply_unfused(ent, rel, st['g_ent'], st['occ_ent'].int(), st['g_rel'], st['occ_rel'].int(), opt)
    assert ent.dtype == torch.float32
    want = c['ent'] - 0.5 * oc.dense_grad(st['g_ent'], st['occ_ent'], c['n_ent'])
    assert torch.equal(ent, want)                 # dyadic rows: the sums are exact in any order
    assert torch.equal(ent[0], c['ent'][0]) and not torch.equal(ent[3], c['ent'][3])
