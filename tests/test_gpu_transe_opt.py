"""gv_transe_apply_opt (ops.transe_apply_opt) and the trainer's optimisers on the device.

a. The entry point alone against float64, on transe_opt_cases' constructed occurrence rows (exact row sums: only the rule is under
   test) at widths 1 / 65 / 200 / 512, a partly filled last workgroup, runs of 70 and of 1, rows without occurrences, a row of
   2^-40 gradients and 66..70 loss partials; every method with and without weight decay (Adagrad: and lr_decay), tables and both
   state arrays after step 1 (slack 1e-5) and step 3 (1e-4) under test_gpu_transe.bound_of: |device - float32 CPU| <=
   4 |float32 CPU - float64| + slack * (row max of |float64|), both references transe.apply_unfused on the CPU.
b. torch's dense semantics: which rows keep their bits, which move, decay or shrink.
c. The bound rejects Adam without bias correction, Adagrad without lr_decay and Adadelta with eps outside the roots.
d. SGD without decay through the new entry point is gv_transe_apply, bit for bit.
e. / f. The trainer: runs and eager vs captured bit-identical (tables, state, step number, epoch loss); one step equals the
   recomputation of its own batch through the three ops.
g. The CLI with --optimizer.

Every comparison of (a) prints its share of the bound (pytest -s, lines "RATIO ...").  Measured worst |device - float32 CPU| /
bound on an MI355X over the four shapes, tables and both state arrays of both tables, (step 1, step 3):

  method     weight_decay 0             weight_decay 0.01 (Adagrad: lr_decay 0.05)
             tables        state        tables        state
  sgd        0.000 0.000   --           0.000 0.000   --
  adagrad    0.000 0.005   0.000 0.000  0.000 0.010   0.000 0.000
  adadelta   0.007 0.001   0.045 0.006  0.008 0.001   0.045 0.007
  adam       0.001 0.001   0.012 0.009  0.033 0.002   0.012 0.067
"""
import numpy as np
import pytest
import torch

import transe_cases as tc
import transe_opt_cases as oc
from gcn_vae_amd import ops, transe
from test_gpu_transe import DEV, assert_bound, bound_of, small_trainer

pytestmark = pytest.mark.gpu


def held(got, fix, f64, what, slack, tag):
    bound = bound_of(fix.double(), f64.double(), slack)
    print(f'RATIO {tag} {what}: {tc.worst_ratio(got, fix, bound):.3f}')
    assert_bound(got, fix, f64, what, slack)


class Applier:
    """The device side of one case: tables, state and buffers, ``step(i)`` applies the case's i-th gradient set."""

    def __init__(self, c, method, wd=0.0, lr_decay=0.0, lr=None):
        self.c, self.method, self.wd, self.ld = c, method, wd, lr_decay
        self.lr = oc.LR[method] if lr is None else lr
        self.ent, self.rel = c['ent'].to(DEV).contiguous().clone(), c['rel'].to(DEV).contiguous().clone()
        self.state = ops.TransEOptState(c['n_ent'], c['n_rel'], c['dim'], DEV)
        self.order = ops.TransEOrder(c['n_occ_e'], c['n_ent'], c['B'], c['n_rel'], DEV)
        self.loss = torch.zeros(1, device=DEV)
        self.acc = torch.zeros(1, dtype=torch.float64, device=DEV)

    def step(self, i):
        st = self.c['steps'][i]
        parts = self.order.build(st['occ_ent'].to(device=DEV, dtype=torch.int32), st['occ_rel'].to(device=DEV, dtype=torch.int32))
        ops.transe_apply_opt(self.ent, self.rel, st['g_ent'].to(DEV), st['g_rel'].to(DEV), parts, self.method, self.lr,
                             st['loss_part'].to(DEV), self.c['margin'], self.loss, self.acc, state=self.state,
                             weight_decay=self.wd, lr_decay=self.ld)
        torch.cuda.synchronize()
        return self


def setting_id(s):
    return f'wd{s[0]:g}-lrdecay{s[1]:g}'


@pytest.mark.parametrize('setting', oc.SETTINGS, ids=setting_id)
@pytest.mark.parametrize('method', oc.METHODS)
@pytest.mark.parametrize('shape', oc.SHAPES, ids=lambda s: f'V{s[0]}-R{s[1]}-dim{s[2]}')
def test_apply_opt_matches_float64(shape, method, setting):
    c = oc.make_case(*shape)
    fix, f64 = oc.references(shape, method, setting)
    a = Applier(c, method, setting[0], setting[1] if method == 'adagrad' else 0.0)
    tag = f'dim{shape[2]}-{method}-{setting_id(setting)}'
    total = 0.0
    for i in range(oc.STEPS):
        a.step(i)
        total += float(c['steps'][i]['loss_part'].double().sum()) + c['margin']
        assert float(a.loss) == float(c['steps'][i]['loss_part'].double().sum()) + c['margin']       # dyadic partials: exact
        if i not in (0, oc.STEPS - 1):
            continue
        slack, when = (1e-5, 'step 1') if i == 0 else (1e-4, f'step {oc.STEPS}')
        held(a.ent, fix[i][0], f64[i][0], f'ent after {when}', slack, tag)
        held(a.rel, fix[i][1], f64[i][1], f'rel after {when}', slack, tag)
        for k in range(2):          # a state array torch does not keep is zero in the references: the device left it alone
            held(a.state.ent[k], fix[i][2][k], f64[i][2][k], f'ent state {k} after {when}', slack, tag)
            held(a.state.rel[k], fix[i][3][k], f64[i][3][k], f'rel state {k} after {when}', slack, tag)
    assert int(a.state.t) == oc.STEPS and float(a.acc) == total
    assert not torch.equal(a.ent.cpu(), c['ent'])
    if setting[0] == 0 and method in ('sgd', 'adagrad'):     # rows without occurrences were not written
        assert torch.equal(a.ent.cpu()[[0, -1]], c['ent'][[0, -1]]) and torch.equal(a.rel.cpu()[2], c['rel'][2])


def semantics_case():
    """10 entities, 3 relations, dim 65; entity 2 and relation 1 are touched in step 1 only, entity 9 and relation 2 never.
    Table entries lie in +-[0.5, 1.5]: a decayed entry keeps its sign."""
    rs = np.random.RandomState(11)
    n_ent, n_rel, dim, n_occ, B = 10, 3, 65, 12, 5
    sign = lambda *s: torch.from_numpy(((rs.rand(*s) + 0.5) * np.where(rs.rand(*s) < 0.5, -1.0, 1.0)).astype(np.float32))  # noqa: E731
    c = dict(n_ent=n_ent, n_rel=n_rel, dim=dim, n_occ_e=n_occ, B=B, margin=1.0, ent=sign(n_ent, dim), rel=sign(n_rel, dim), steps=[])
    for occ_e, occ_r in (([2, 2, 2, 0, 1, 3, 4, 5, 6, 7, 8, 0], [1, 1, 0, 0, 0]), ([0, 0, 1, 3, 3, 4, 5, 6, 7, 8, 8, 1], [0, 0, 0, 0, 0])):
        c['steps'].append(dict(occ_ent=torch.tensor(occ_e), occ_rel=torch.tensor(occ_r), g_ent=oc.dyadic(rs, n_occ, dim),
                               g_rel=oc.dyadic(rs, B, dim), loss_part=oc.dyadic(rs, B)))
    return c


@pytest.mark.parametrize('method', oc.METHODS)
def test_rows_touched_in_step_one_only(method):
    c = semantics_case()
    a = Applier(c, method).step(0)
    rows = lambda: [x[2].clone() for x in (a.ent, *a.state.ent)] + [x[1].clone() for x in (a.rel, *a.state.rel)]  # noqa: E731
    p1, s1, s2, rp1, rs1, rs2 = rows()
    assert not torch.equal(p1.cpu(), c['ent'][2]) and not torch.equal(rp1.cpu(), c['rel'][1])
    a.step(1)
    q1, t1, t2, rq1, rt1, rt2 = rows()
    if method in ('sgd', 'adagrad'):          # the identity: not written
        for x, y in ((p1, q1), (s1, t1), (s2, t2), (rp1, rq1), (rs1, rt1), (rs2, rt2)):
            assert torch.equal(x, y)
    elif method == 'adam':        # g = 0, but the first moment still moves every element it is non-zero in; both moments decay
        live_e, live_r = s1 != 0, rs1 != 0
        assert int(live_e.sum()) > 0.9 * c['dim'] and int(live_r.sum()) > 0.9 * c['dim']
        assert bool((q1 != p1)[live_e].all()) and bool((rq1 != rp1)[live_r].all())
        torch.testing.assert_close(t1, s1 * 0.9, rtol=2 ** -20, atol=0)
        torch.testing.assert_close(t2, s2 * 0.999, rtol=2 ** -20, atol=0)
    else:                         # adadelta: d = 0 -- the parameter stays, both averages decay by rho
        assert torch.equal(q1, p1) and torch.equal(rq1, rp1)
        assert float(s1.abs().max()) > 0 and float(s2.abs().max()) > 0
        for new, old in ((t1, s1), (t2, s2), (rt1, rs1), (rt2, rs2)):
            torch.testing.assert_close(new, old * 0.9, rtol=2 ** -20, atol=0)
    # never touched, no decay: the parameter keeps its bits under every method
    assert torch.equal(a.ent[9].cpu(), c['ent'][9]) and torch.equal(a.rel[2].cpu(), c['rel'][2])


@pytest.mark.parametrize('method', oc.METHODS)
def test_weight_decay_shrinks_rows_that_are_never_touched(method):
    c = semantics_case()
    a = Applier(c, method, wd=0.1, lr=0.01)
    for i in range(2):
        before = (a.ent[9].clone(), a.rel[2].clone())
        a.step(i)
        for new, old in zip((a.ent[9], a.rel[2]), before):
            assert bool((new.abs() < old.abs()).all()) and bool((new.sign() == old.sign()).all())


@pytest.mark.parametrize('method, wrong', [('adam', 'adam_no_bias_correction'), ('adagrad', 'adagrad_no_lr_decay'),
                                           ('adadelta', 'adadelta_eps_outside')])
def test_bound_rejects_a_wrong_rule(method, wrong):
    """On test (a)'s inputs and bound, the three-step tables of a rule that is wrong in one detail fail, the right rule's pass
    (float32 hand statements stand in for a device: what is shown is that the bound tells them apart)."""
    shape, setting = oc.SHAPES[1], oc.SETTINGS[1]
    c = oc.make_case(*shape)
    fix, f64 = oc.references(shape, method, setting)
    ld = setting[1] if method == 'adagrad' else 0.0
    good = oc.hand_steps(c, method, setting[0], ld, torch.float32)
    bad = oc.hand_steps(c, method, setting[0], ld, torch.float32, wrong)
    for which, what in ((0, 'ent'), (1, 'rel')):
        assert_bound(good[-1][which], fix[-1][which], f64[-1][which], what, 1e-4)
        with pytest.raises(AssertionError):
            assert_bound(bad[-1][which], fix[-1][which], f64[-1][which], f'{wrong} {what}', 1e-4)


def test_sgd_without_decay_is_transe_apply_bit_for_bit():
    c = tc.case_of(((211, 2, 200, 130, 2), tc.COMBOS[0]))
    B, K = c['B'], c['K']
    ids = tuple(c[k].to(device=DEV, dtype=torch.int32).contiguous() for k in ('bh', 'br', 'bt'))
    tabs = [[c['ent'].to(DEV).contiguous().clone(), c['rel'].to(DEV).contiguous().clone()] for _ in range(2)]
    order = ops.TransEOrder((2 + K) * B, c['V'], B, c['R'], DEV)
    occ = torch.empty((2 + K) * B, dtype=torch.int32, device=DEV)
    loss = [torch.zeros(1, device=DEV) for _ in range(2)]
    acc = [torch.zeros(1, dtype=torch.float64, device=DEV) for _ in range(2)]
    state = ops.TransEOptState(c['V'], c['R'], c['dim'], DEV)
    for _ in range(2):
        g_ent, g_rel, part = ops.transe_step(*tabs[0], *ids, B, K, c['p'], c['nf'], c['margin'], c['adv'], c['regul'], occ_ent=occ)
        parts = order.build(occ, ids[1][:B])
        ops.transe_apply(*tabs[0], g_ent, g_rel, parts, c['lr'], part, c['margin'], loss[0], acc[0])
        ops.transe_apply_opt(*tabs[1], g_ent, g_rel, parts, 'SGD', c['lr'], part, c['margin'], loss[1], acc[1], state=state)
        torch.cuda.synchronize()
        for x, y in zip(tabs[0] + [loss[0], acc[0]], tabs[1] + [loss[1], acc[1]]):
            assert torch.equal(x, y)
    assert not torch.equal(tabs[1][0].cpu(), c['ent']) and int(state.t) == 2
    assert all(float(x.abs().sum()) == 0 for x in (*state.ent, *state.rel))


TRAINERS = [('sgd', dict(weight_decay=0.01)), ('adagrad', dict(alpha=0.1, lr_decay=0.05)), ('adadelta', dict()),
            ('adam', dict(alpha=0.01)), ('adam', dict(alpha=0.01, weight_decay=0.01))]


def trainer_result(method, kw, graph, steps=5):
    _, model, tr = small_trainer(graph=graph, opt_method=method, **kw)
    tr.epoch_loss.zero_()                      # as epoch() does (the warm-up step of capture() has added to it)
    for _ in range(steps):
        tr.step()
    torch.cuda.synchronize()
    return [tr.ent, tr.rel, *tr.opt_state.tensors(), tr.epoch_loss, tr.loss]


@pytest.mark.parametrize('method, kw', TRAINERS, ids=[f'{m}-{"-".join(k)}' for m, k in TRAINERS])
def test_trainer_runs_are_bit_identical_eager_and_captured(method, kw):
    """With Adam this fails if the step number is baked into the capture, or if capture() forgets to restore the state."""
    first = trainer_result(method, kw, False)
    for graph in (False, True):
        other = trainer_result(method, kw, graph)
        for i, (x, y) in enumerate(zip(first, other)):
            assert torch.equal(x, y), f'{"captured" if graph else "second eager"} run: tensor {i} differs'
    assert int(first[6]) == 5 and float(first[7]) > 0


def test_trainer_plain_sgd_keeps_gv_transe_apply():
    _, _, tr = small_trainer()
    assert tr.opt_state is None and tr.opt_method == 'sgd'
    _, _, tr = small_trainer(opt_method='SGD')
    assert tr.opt_state is None


@pytest.mark.parametrize('method, kw', TRAINERS[1:], ids=[f'{m}-{"-".join(k)}' for m, k in TRAINERS[1:]])
def test_trainer_step_is_the_three_ops_on_its_own_batch(method, kw):
    _, model, tr = small_trainer(opt_method=method, **kw)
    ent, rel = tr.ent.clone(), tr.rel.clone()
    start = ent.clone()
    tr.step()
    B, K = tr.batch, tr.neg_ent
    occ = torch.empty((2 + K) * B, dtype=torch.int32, device=DEV)
    g_ent, g_rel, part = ops.transe_step(ent, rel, tr.bh, tr.br, tr.bt, B, K, model.p_norm, model.norm_flag, tr.margin, tr.adv, tr.regul,
                                         occ_ent=occ)
    parts = ops.TransEOrder((2 + K) * B, model.ent_tot, B, model.rel_tot, DEV).build(occ, tr.br[:B])
    state = ops.TransEOptState(model.ent_tot, model.rel_tot, model.dim, DEV)
    loss = torch.zeros(1, device=DEV)
    ops.transe_apply_opt(ent, rel, g_ent, g_rel, parts, method, tr.alpha, part, tr.margin, loss, state=state,
                         weight_decay=tr.weight_decay, lr_decay=tr.lr_decay)
    torch.cuda.synchronize()
    for x, y in zip([ent, rel, loss, *state.tensors()], [tr.ent, tr.rel, tr.loss, *tr.opt_state.tensors()]):
        assert torch.equal(x, y)
    assert int(state.t) == 1 and not torch.equal(ent, start)


@pytest.mark.parametrize('extra', [['--optimizer', 'adagrad'], ['--optimizer', 'adam', '--alpha', '0.01', '--graph-step']],
                         ids=['adagrad', 'adam-captured'])
def test_cli_trains_with_an_optimizer(extra, tmp_path, capsys):
    args = transe.build_parser().parse_args(['-d', 'synthetic:300:6:4000:200:200', '--train-times', '2', '--nbatches', '10', '--dim', '48',
                                             '--seed', '0', '--checkpoint', str(tmp_path / 'transe.ckpt')] + extra)
    out = transe.main(args)
    printed = capsys.readouterr().out
    assert 'Epoch 1 | loss:' in printed
    assert np.isfinite(out['mrr_raw']) and np.isfinite(out['mr_raw']) and all(np.isfinite(v) for v in out['hits_raw'].values())
    assert 0 < out['mrr_raw'] <= 1
