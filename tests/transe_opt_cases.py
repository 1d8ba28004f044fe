"""Constructed inputs and references for the TransE optimiser tests (test_transe_opt_host.py without a GPU,
test_gpu_transe_opt.py on the device).

``hand_step`` is a hand-written statement of the four update rules of gv_transe_apply_opt (torch.optim's SGD, Adagrad, Adadelta and
Adam at torch's defaults, coupled weight decay) in whatever dtype its tensors have; its ``wrong`` argument states three broken
variants that a useful bound must reject.

``make_case`` builds what the apply entry point alone reads: two tables, and per step a fresh set of occurrence gradient rows with
their ids.  Every gradient value is a multiple of 2^-10 in [-1, 1] (one planted row: 2^-40 in every column), so a row's sum of up to
a few hundred occurrences is exact in float32 in any order: only the update rule is under test, and no float32-ambiguous sign of a
tiny gradient can arise.  Planted in every step's ids:
  * entity 0 and the last entity, relation 2: no occurrence;
  * entity 3: LONG (> 64) occurrences; entity 5 and relation 4: exactly one;
  * entity 7: one occurrence whose gradient is 2^-40 in every column (the eps terms decide its update);
  * B > 64 relation occurrences (and loss partials: the loss wave's strided loop runs twice).
``references`` runs ``transe.apply_unfused`` (index_add_ + a real torch.optim step) on the CPU in float32 (the fixture) and float64
(the truth) and records tables and optimiser state after every step.  Cached: the tests of a process share one case and its
references, and none changes them.
"""
import functools

import numpy as np
import torch

from gcn_vae_amd import transe

STEPS = 3
LONG = 70
TINY = 2.0 ** -40
# (n_ent, n_rel, dim, n_occ_e, B): n_ent + n_rel is no multiple of 4 (the last workgroup of rows is partly filled)
SHAPES = [
    (37, 6, 1, 150, 70),       # one live lane
    (37, 6, 65, 150, 70),      # two trips of the lane loop, the second with one lane
    (41, 5, 200, 180, 70),     # the workload's width: four trips, the guard inside the last
    (21, 5, 512, 120, 66),     # GV_TRANSE_MAX_DIM: eight full trips
]
LR = {'sgd': 0.5, 'adagrad': 0.5, 'adadelta': 1.0, 'adam': 0.01}
# (weight_decay, lr_decay of Adagrad)
SETTINGS = [(0.0, 0.0), (0.01, 0.05)]
METHODS = ('sgd', 'adagrad', 'adadelta', 'adam')
STATE_KEYS = {'sgd': (), 'adagrad': ('sum',), 'adadelta': ('square_avg', 'acc_delta'), 'adam': ('exp_avg', 'exp_avg_sq')}


def hand_step(method, p, g, s1, s2, t, lr, wd=0.0, lr_decay=0.0, wrong=None):
    """One step of ``method`` on parameter ``p`` with dense gradient ``g`` and state (s1, s2) at the 1-based step ``t``, out of
    place: returns (p, s1, s2).  ``wrong``: 'adam_no_bias_correction', 'adagrad_no_lr_decay' or 'adadelta_eps_outside'."""
    g = g + wd * p
    if method == 'sgd':
        return p - lr * g, s1, s2
    if method == 'adagrad':
        clr = lr if wrong == 'adagrad_no_lr_decay' else lr / (1 + (t - 1) * lr_decay)
        s1 = s1 + g * g
        return p - clr * g / (s1.sqrt() + 1e-10), s1, s2
    if method == 'adadelta':
        rho, eps = 0.9, 1e-6
        s1 = rho * s1 + (1 - rho) * g * g
        if wrong == 'adadelta_eps_outside':
            d = (s2.sqrt() + eps) / (s1.sqrt() + eps) * g
        else:
            d = (s2 + eps).sqrt() / (s1 + eps).sqrt() * g
        s2 = rho * s2 + (1 - rho) * d * d
        return p - lr * d, s1, s2
    if method == 'adam':
        b1, b2, eps = 0.9, 0.999, 1e-8
        bc1, bc2 = (1.0, 1.0) if wrong == 'adam_no_bias_correction' else (1 - b1 ** t, 1 - b2 ** t)
        s1 = s1 + (1 - b1) * (g - s1)
        s2 = b2 * s2 + (1 - b2) * g * g
        return p - (lr / bc1) * s1 / (s2.sqrt() / bc2 ** 0.5 + eps), s1, s2
    raise ValueError(method)


def dense_grad(rows, occ, n):
    return torch.zeros(n, rows.shape[1], dtype=rows.dtype).index_add_(0, occ, rows)


def hand_steps(c, method, wd, lr_decay, dtype, wrong=None):
    """The case's STEPS steps by ``hand_step`` in ``dtype``: [(ent, rel, (s1_ent, s2_ent), (s1_rel, s2_rel))] after each step."""
    ent, rel = c['ent'].to(dtype), c['rel'].to(dtype)
    se, sr = (torch.zeros_like(ent), torch.zeros_like(ent)), (torch.zeros_like(rel), torch.zeros_like(rel))
    out = []
    for t, st in enumerate(c['steps'], 1):
        ent, *se = hand_step(method, ent, dense_grad(st['g_ent'].to(dtype), st['occ_ent'], c['n_ent']), *se, t, LR[method], wd, lr_decay, wrong)
        rel, *sr = hand_step(method, rel, dense_grad(st['g_rel'].to(dtype), st['occ_rel'], c['n_rel']), *sr, t, LR[method], wd, lr_decay, wrong)
        out.append((ent, rel, tuple(se), tuple(sr)))
    return out


def dyadic(rs, *shape):
    return torch.from_numpy((rs.randint(-1024, 1025, shape) / 1024.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def make_case(n_ent, n_rel, dim, n_occ_e, B, seed=0):
    rs = np.random.RandomState(seed + dim)
    c = dict(n_ent=n_ent, n_rel=n_rel, dim=dim, n_occ_e=n_occ_e, B=B, margin=5.0,
             ent=torch.from_numpy(rs.standard_normal((n_ent, dim)).astype(np.float32)),
             rel=torch.from_numpy(rs.standard_normal((n_rel, dim)).astype(np.float32)), steps=[])
    free_e = np.array([e for e in range(1, n_ent - 1) if e not in (3, 5, 7)])
    free_r = np.array([r for r in range(n_rel) if r not in (2, 4)])
    for _ in range(STEPS):
        occ_e = np.concatenate([np.full(LONG, 3), [5, 7], free_e[rs.randint(0, len(free_e), n_occ_e - LONG - 2)]])
        perm = rs.permutation(n_occ_e)
        occ_e = occ_e[perm]
        g_ent = dyadic(rs, n_occ_e, dim)
        g_ent[int(np.nonzero(occ_e == 7)[0][0])] = TINY
        occ_r = np.concatenate([[4], free_r[rs.randint(0, len(free_r), B - 1)]])[rs.permutation(B)]
        c['steps'].append(dict(occ_ent=torch.from_numpy(occ_e.astype(np.int64)), g_ent=g_ent,
                               occ_rel=torch.from_numpy(occ_r.astype(np.int64)), g_rel=dyadic(rs, B, dim),
                               loss_part=dyadic(rs, B)))
    return c


def unfused_steps(c, method, wd, lr_decay, dtype):
    """The case's STEPS steps by ``transe.apply_unfused`` + ``transe.make_optimizer`` on the CPU in ``dtype``, in the layout of
    ``hand_steps`` (a state torch does not keep is a zero array)."""
    ent, rel = c['ent'].to(dtype).clone(), c['rel'].to(dtype).clone()
    opt = transe.make_optimizer([ent, rel], method, LR[method], wd, lr_decay)
    out = []
    for st in c['steps']:
        transe.apply_unfused(ent, rel, st['g_ent'], st['occ_ent'], st['g_rel'], st['occ_rel'], opt)
        states = []
        for p in (ent, rel):
            s = [opt.state[p][k].clone() for k in STATE_KEYS[method]]
            states.append(tuple(s + [torch.zeros_like(p)] * (2 - len(s))))
        out.append((ent.clone(), rel.clone(), states[0], states[1]))
    return out


@functools.lru_cache(maxsize=None)
def references(shape, method, setting):
    """(float32 fixture, float64 truth) of ``unfused_steps`` for one shape, method and (weight_decay, lr_decay) setting."""
    c = make_case(*shape)
    wd, ld = setting[0], setting[1] if method == 'adagrad' else 0.0
    return unfused_steps(c, method, wd, ld, torch.float32), unfused_steps(c, method, wd, ld, torch.float64)
