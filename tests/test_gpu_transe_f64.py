"""The fused TransE step (gv_transe_step + TransEOrder + gv_transe_apply) and gv_transe_queries against float64 at the shapes that
select the kernels' paths: widths 1 / 63 / 64 / 65 / 200 / 500 / 512 (which of the 8 register slots of 64 columns are live and
where the k < dim guard falls), batches of 4 .. 257 positives (1 .. 65 workgroups, a partly filled last one), K = 1 .. 4, long
occurrence runs, both norms, norm_flag on and off, with and without self-adversarial weights and the regulariser.

The cases and their references come from transe_cases.py (constructed, screened for float32-ambiguous branches, shared by every
test here and never modified).  The bound is test_gpu_transe.bound_of's: |device - float32 CPU| <= 4 |float32 CPU - float64| +
slack * (row max of |float64|), where both references are transe.step_unfused, slack 1e-5 for the first step's score, loss and
gradients and 1e-4 for the tables after three SGD steps.

Measured worst |device - float32 CPU| / bound over the four (p, norm_flag, adv, regul) combinations of each shape on an MI355X:

  (V, R, dim, B, K)        score   loss    g_ent   g_rel   ent3    rel3
  (50, 5, 1, 5, 1)         0.000   0.009   0.137   0.008   0.009   0.001
  (97, 7, 63, 5, 2)        0.029   0.084   0.086   0.049   0.004   0.001
  (97, 7, 64, 4, 3)        0.023   0.067   0.082   0.060   0.006   0.003
  (97, 7, 65, 7, 3)        0.027   0.076   0.029   0.047   0.003   0.003
  (211, 2, 200, 130, 2)    0.045   0.046   0.230   0.067   0.008   0.008
  (64, 3, 500, 9, 4)       0.060   0.110   0.164   0.081   0.023   0.016
  (64, 3, 512, 9, 4)       0.057   0.133   0.169   0.071   0.020   0.021
  (30, 2, 128, 257, 1)     0.043   0.018   0.106   0.075   0.010   0.008

The epoch accumulator used 0.006 (dim 200) and 0.017 (B = 257) of its bound, the trainer's step 0.009 (loss) and 0.002 (tables)
with 1 ambiguous positive of 400, the queries at most 0.16 of theirs.  Every test prints its ratios (pytest -s, lines "RATIO ...").
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transe_cases as tc
from gcn_vae_amd import ops
from test_gpu_transe import DEV, assert_bound, bound_of, device_steps, small_trainer

pytestmark = pytest.mark.gpu


def held(got, fix, f64, what, slack=1e-5, tag=''):
    """assert_bound, after printing how much of the bound the device used (read with pytest -s)."""
    bound = bound_of(fix.double(), f64.double(), slack)
    print(f'RATIO {tag} {what}: {tc.worst_ratio(got, fix, bound):.3f}')
    assert_bound(got, fix, f64, what, slack)


def references(c, step=0):
    return c['out32'][step], c['out64'][step]


@pytest.mark.parametrize('param', tc.PARAMS, ids=tc.param_id)
def test_step_matches_float64(param):
    c, tag = tc.case_of(param), tc.param_id(param)
    (score, loss, ge, gr), ent3, rel3 = device_steps(c, tc.STEPS)
    (s32, l32, ge32, gr32), (s64, l64, ge64, gr64) = references(c)
    held(score, s32, s64, 'score', tag=tag)
    held(loss.reshape(()), l32, l64, 'loss', tag=tag)
    held(ge, ge32, ge64, 'g_ent', tag=tag)
    held(gr, gr32, gr64, 'g_rel', tag=tag)
    held(ent3, c['tab32'][tc.STEPS][0], c['tab64'][tc.STEPS][0], 'ent after 3 steps', 1e-4, tag)
    held(rel3, c['tab32'][tc.STEPS][1], c['tab64'][tc.STEPS][1], 'rel after 3 steps', 1e-4, tag)


def one_step(c, ent=None, rel=None):
    """gv_transe_step alone: (g_ent rows, g_rel rows, loss_part, occ_ent) and the device tables and ids it ran on."""
    ent = (c['ent'] if ent is None else ent).to(DEV).contiguous().clone()
    rel = (c['rel'] if rel is None else rel).to(DEV).contiguous().clone()
    B, K = c['B'], c['K']
    ids = tuple(c[k].to(device=DEV, dtype=torch.int32).contiguous() for k in ('bh', 'br', 'bt'))
    occ = torch.full(((2 + K) * B,), -1, dtype=torch.int32, device=DEV)
    g_ent, g_rel, part = ops.transe_step(ent, rel, *ids, B, K, c['p'], c['nf'], c['margin'], c['adv'], c['regul'], occ_ent=occ)
    return (g_ent, g_rel, part, occ), ent, rel, ids


@pytest.mark.parametrize('param', tc.PARAMS, ids=tc.param_id)
def test_occurrence_rows_carry_their_ids_and_add_up_to_the_gradient(param):
    """One gradient row per occurrence, [h of b | t of b | corrupted side of (j, b)] and [r of b]: the ids are exactly those, and
    the rows' float64 index_add is the table gradient (the same bound, without the device's ordered reduction)."""
    c, tag = tc.case_of(param), tc.param_id(param)
    (g_ent, g_rel, part, occ), _, _, _ = one_step(c)
    assert torch.equal(occ.cpu().long(), tc.occurrence_ids(c))
    (_, l32, ge32, gr32), (_, l64, ge64, gr64) = references(c)
    ge = torch.zeros(c['V'], c['dim'], dtype=torch.float64).index_add_(0, tc.occurrence_ids(c), g_ent.cpu().double())
    gr = torch.zeros(c['R'], c['dim'], dtype=torch.float64).index_add_(0, c['br'][:c['B']], g_rel.cpu().double())
    held(ge, ge32, ge64, 'index_add of the g_ent rows', tag=tag)
    held(gr, gr32, gr64, 'index_add of the g_rel rows', tag=tag)
    held(part.cpu().double().sum() + c['margin'], l32, l64, 'loss_part.sum() + margin', tag=tag)


@pytest.mark.parametrize('param', [p for p in tc.PARAMS if p[0] in (tc.SHAPES[1], tc.SHAPES[4])], ids=tc.param_id)
def test_rows_without_an_occurrence_keep_their_bits(param):
    c = tc.case_of(param)
    _, ent3, rel3 = device_steps(c, tc.STEPS)
    free_e = torch.ones(c['V'], dtype=torch.bool)
    free_e[tc.occurrence_ids(c)] = False
    free_r = torch.ones(c['R'], dtype=torch.bool)
    free_r[c['br']] = False
    assert int(free_e.sum()) > 0 and (int(free_r.sum()) > 0 or c['B'] > c['R'])       # B = 5 on R = 7 leaves relations free
    assert torch.equal(ent3.cpu()[free_e], c['ent'][free_e]) and torch.equal(rel3.cpu()[free_r], c['rel'][free_r])
    assert not torch.equal(ent3.cpu()[~free_e], c['ent'][~free_e])


@pytest.mark.parametrize('param', [p for p in tc.PARAMS if p[0] in (tc.SHAPES[4], tc.SHAPES[7])], ids=tc.param_id)
def test_loss_and_epoch_accumulator(param):
    """loss_out[0] = loss_part.sum() + margin (B > 64: the loss wave's strided loop runs more than once), and the float64 epoch
    accumulator after three steps is the sum of the three losses, within the sum of their bounds."""
    c, tag = tc.case_of(param), tc.param_id(param)
    B, K = c['B'], c['K']
    order = ops.TransEOrder((2 + K) * B, c['V'], B, c['R'], DEV)
    loss = torch.zeros(1, device=DEV)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    ent = rel = None
    total32 = total64 = total_bound = 0.0
    for s in range(tc.STEPS):
        (g_ent, g_rel, part, occ), ent, rel, ids = one_step(c, ent, rel)
        ops.transe_apply(ent, rel, g_ent, g_rel, order.build(occ, ids[1][:B]), c['lr'], part, c['margin'], loss, acc)
        l32, l64 = c['out32'][s][1], c['out64'][s][1]
        held(loss.reshape(()), l32, l64, f'loss_out of step {s}', tag=tag)
        held(part.cpu().double().sum() + c['margin'], l32, l64, f'loss_part.sum() + margin of step {s}', tag=tag)
        total32, total64 = total32 + float(l32.double()), total64 + float(l64)
        total_bound += float(bound_of(l32.double(), l64, 1e-5))
    err = abs(float(acc) - total32)
    print(f'RATIO {tag} epoch_acc: {err / total_bound:.3f}')
    assert err <= total_bound, f'epoch_acc {float(acc)!r} vs {total32!r} (float64 {total64!r}): {err:.3e} > {total_bound:.3e}'


@pytest.mark.parametrize('param', [p for p in tc.PARAMS if p[0][2] in (200, 512)], ids=tc.param_id)
def test_bound_bites_at_width(param):
    """At the workload's width and at GV_TRANSE_MAX_DIM the bound sees a 1 % change of one ordinary g_ent row, and the loss of
    the columns of the row's last live register slot (192..199 of 200; 448..511 of 512: a dropped slot)."""
    c = tc.case_of(param)
    (_, _, ge, _), _, _ = device_steps(c, 1)
    (_, _, ge32, _), (_, _, ge64, _) = references(c)
    assert_bound(ge, ge32, ge64, 'g_ent')
    first = tc.HOT + 1                                            # past the zero, the two tiny and the hot rows
    row = int(ge64[first:].abs().amax(1).argmax()) + first
    cols = slice(192, 200) if c['dim'] == 200 else slice(448, 512)
    assert float(ge64[row, cols].abs().max()) > 1e-3 * float(ge64[row].abs().max())      # the slot holds a share of the row
    scaled, dropped = ge.clone(), ge.clone()
    scaled[row] *= 1.01
    dropped[row, cols] = 0.0
    for bad, what in ((scaled, 'scaled row'), (dropped, 'dropped slot')):
        with pytest.raises(AssertionError):
            assert_bound(bad, ge32, ge64, what)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'captured'])
def test_trainer_step_matches_float64_replay_of_its_batch(graph):
    """One DeviceTrainer step at the workload's width (dim 200, 400 positives, 5 negatives each, sampled on the device), eager and
    as a captured graph's replay: the batch is read back and replayed through float64 step_unfused and ent - alpha * g.  A
    sampled batch is not screened, so the positives with a float32-ambiguous branch (transe_cases.ambiguity) are found in
    float64 and the table rows they touch left out: at most 2 % of the positives, or the test fails."""
    _, model, tr = small_trainer(graph=graph, dim=200, neg_ent=5)
    start = (model.ent_embeddings.weight.detach().cpu().clone(), model.rel_embeddings.weight.detach().cpu().clone())
    tr.step()
    torch.cuda.synchronize()
    B, K = tr.batch, tr.neg_ent
    c = dict(ent=start[0], rel=start[1], bh=tr.bh.cpu().long(), br=tr.br.cpu().long(), bt=tr.bt.cpu().long(), B=B, K=K,
             p=model.p_norm, nf=model.norm_flag, margin=tr.margin, adv=tr.adv, regul=tr.regul, lr=tr.alpha)
    out32, tab32 = tc.run_steps(c, torch.float32, 1)
    out64, tab64 = tc.run_steps(c, torch.float64, 1)
    rows, pairs = tc.ambiguity(tab64[0][0], tab64[0][1], tab32[0][0], tab32[0][1], c['bh'], c['br'], c['bt'], B, model.dim,
                               c['p'], c['nf'], c['margin'])
    amb = rows.view(1 + K, B).any(0) | pairs.any(0)
    print(f'RATIO trainer-{"captured" if graph else "eager"} ambiguous positives: {int(amb.sum())} of {B}')
    assert int(amb.sum()) <= 0.02 * B
    keep_e = torch.ones(model.ent_tot, dtype=torch.bool)
    keep_r = torch.ones(model.rel_tot, dtype=torch.bool)
    keep_e[torch.cat([c['bh'].view(1 + K, B)[:, amb].reshape(-1), c['bt'].view(1 + K, B)[:, amb].reshape(-1)])] = False
    keep_r[c['br'][:B][amb]] = False
    tag = f'trainer-{"captured" if graph else "eager"}'
    held(tr.loss.reshape(()), out32[0][1], out64[0][1], 'loss', tag=tag)
    held(tr.ent.cpu()[keep_e], tab32[1][0][keep_e], tab64[1][0][keep_e], 'ent after the step', 1e-4, tag)
    held(tr.rel.cpu()[keep_r], tab32[1][1][keep_r], tab64[1][1][keep_r], 'rel after the step', 1e-4, tag)
    assert not torch.equal(tr.ent.cpu(), start[0])


@pytest.mark.parametrize('norm_flag', [True, False], ids=['norm', 'raw'])
@pytest.mark.parametrize('dim', [1, 63, 64, 65, 200, 512])
def test_queries_match_float64_of_the_host_tables(dim, norm_flag):
    """gv_transe_queries' three forms against float64 F.normalize(ent[a]) +- F.normalize(rel[r]) of the HOST tables, to a few ulps
    of a division and an add: 8 * 2^-23 * (|n(e)| + |n(r)|) + 1e-30 per element."""
    V, R = 41, 5
    ent, rel = tc.special_tables(V, R, dim, 1.0, np.random.RandomState(dim))
    a = torch.tensor([tc.ZERO, tc.TINY_BELOW, tc.TINY_ABOVE, 7, 40, 3, 3, 19, 22, 8, 1, 30, 11])      # 13 queries: 4 blocks, one wave in the last
    r = torch.tensor([0, 1, 2, 3, 4, 0, 4, 2, 2, 1, 3, 0, 1])
    n = (lambda x: F.normalize(x, 2, -1)) if norm_flag else (lambda x: x)
    ne, nr = n(ent.double()), n(rel.double())
    dev_ent, dev_rel = ent.to(DEV), rel.to(DEV)
    forms = (('table', ops.transe_queries(dev_ent, norm_flag=norm_flag), ne, torch.zeros_like(ne), 1.0),
             ('tail', ops.transe_queries(dev_ent, dev_rel, a, r, head=False, norm_flag=norm_flag), ne[a], nr[r], 1.0),
             ('head', ops.transe_queries(dev_ent, dev_rel, a, r, head=True, norm_flag=norm_flag), ne[a], nr[r], -1.0))
    for what, got, e, rr, sign in forms:
        bound = 8 * tc.ULP * (e.abs() + rr.abs()) + 1e-30
        err = (got.cpu().double() - (e + sign * rr)).abs()
        print(f'RATIO queries-dim{dim}-{"norm" if norm_flag else "raw"} {what}: {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all()), f'{what}: worst excess {float((err - bound).max()):.3e} (max err {float(err.max()):.3e})'
    if norm_flag:       # the planted rows did what they are there for: 0, x / 1e-12 (norm 0.5) and a unit row
        norms = forms[0][1].cpu().double().norm(dim=1)
        assert float(norms[tc.ZERO]) == 0.0 and abs(float(norms[tc.TINY_BELOW]) - 0.5) < 1e-2 and abs(float(norms[tc.TINY_ABOVE]) - 1) < 1e-5
