"""gv_clip_adam_step / gv_adam_step (k_gradsq_part + k_adam), optim.FlatAdam and distributed.ShardedFlatAdam on the device,
beyond a one-block arena.  Inputs, references and the bound are flat_adam_cases' (its docstring says why the references take the
float32-rounded hyperparameters): |device - float32 CPU| <= 4 |float32 CPU - float64| + slack * max |float64|, slack 1e-5 after
step 1 and 1e-4 after step 3, both references torch.optim.Adam + clip_grad_norm_ on the CPU.

1. The entry points against float64 at n = 1, 63, 257, 4097, 300*4096+1 and 4194304+4096+3 (one partial with idle threads; two
   partials; 301 partials = the second trip of k_adam's partial loop; past the 1024-partial and the 2048-block caps with a ragged
   tail), lr 1e-2 and 1e-3, in four forms: gv_clip_adam_step; gv_adam_step with a sumsq of gv_mean_sq (the sharded route), without
   a sumsq, and after the weight decay's gv_axpby.  Also the norm within 1 % of max_norm, step counters preset to 999 and 99 999,
   and zero gradients after a non-zero one.
2. The norm counts every element once: twelve powers of two whose squares occupy disjoint bits, sumsq bit for bit.
3. The norm's accuracy on a dense arena under a bound derived from the code (``chain_length``).
4. Through FlatAdam and ShardedFlatAdam with parameter sizes that are no multiples of 64: every parameter and its moment slices
   under the bound, the padding exactly 0, grad_norm() under (3)'s bound.
5. Degenerate gradients.  6. Non-finite gradients, pinned.  7. The bound rejects three wrong rules on the device's own inputs.

Every comparison of (1), (3) and (4) prints its share of its bound (pytest -s, lines "RATIO ...").  Measured worst
|device - float32 CPU| / bound on an MI355X, (step 1, step 3):

                                                   p             exp_avg       exp_avg_sq
  (1) six sizes x two lr, gv_clip_adam_step        0.008 0.085   0.000 0.198   0.000 0.221
      gv_mean_sq + gv_adam_step                    0.008 0.085   0.000 0.198   0.000 0.221
      gv_adam_step without a sumsq                 0.008 0.017   0.000 0.001   0.000 0.000
      gv_axpby + gv_adam_step (weight decay)       0.239 0.019   0.010 0.001   0.018 0.000
      clip edge, preset t, zero gradients (both)   0.012 0.008   0.000 0.001   0.000 0.002
  (4) FlatAdam and ShardedFlatAdam (the same)      0.010 0.022   0.000 0.097   0.000 0.140

and the worst |sumsq - float64| / sumsq as a share of chain_length's bound: 0.060 (gv_clip_adam_step, n = 257) and 0.054
(gv_mean_sq) over every step of (1); 0.041 / 0.046 at n = 300*4096+1 and 0.018 / 0.017 at n = 4194304+4096+3 in (3); grad_norm()
in (4): 0.023.  No comparison came near its bound and (6) found the behaviour read off the code: the kernel was not changed.
"""
import numpy as np
import pytest
import torch

import flat_adam_cases as fc
from gcn_vae_amd import lib
from gcn_vae_amd.lib import ptr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
U = 2.0 ** -24
FORMS = ('clip', 'mean_sq', 'plain', 'decay')


def case_of(n, lr, form, **kw):
    if form in ('clip', 'mean_sq'):
        return fc.arena_case(n, lr, **kw)
    return fc.arena_case(n, lr, max_norm=None, weight_decay=fc.WEIGHT_DECAY if form == 'decay' else 0.0, **kw)


def chain_length(n, route):
    """The longest chain of float32 roundings between one g[i]^2 and the published sum of squares, read off the code.

    First pass (k_gradsq_part for gv_clip_adam_step, k_sumsq_part for gv_mean_sq): nb = min(1024, ceil(n / 4096)) blocks of 256
    threads; a thread runs ceil(n / (256 nb)) trips of acc = fmaf(g, g, acc), one rounding each (the product is exact inside the
    fma).  wave_sum: four DPP adds inside a row of 16 (row16_sum), then (r0 + r16) + (r32 + r48): 6.  The block's four waves:
    (s0 + s1) + (s2 + s3) in k_gradsq_part: 2; s0 + s1 + s2 + s3 in block_sum_256: 3.  Second pass (the head of k_adam, or
    k_final_sum): ceil(nb / 256) trips of acc += part[i], the same wave_sum, the same block sum.  gv_mean_sq's scale is 1: exact.
    Every term is non-negative, so with k such roundings |sum - exact| / exact <= (1 + u)^k - 1 <= k u / (1 - k u), u = 2^-24."""
    nb = min(1024, -(-n // 4096))
    trips, part_trips, wave = -(-n // (256 * nb)), -(-nb // 256), 4 + 2
    block = 2 if route == 'clip' else 3
    return (trips + wave + block) + (part_trips + wave + block)


def sumsq_bound(n, route):
    k = chain_length(n, route)
    return k * U / (1 - k * U)


def test_chain_length_is_what_the_docstring_derives():
    assert chain_length(1, 'clip') == (1 + 6 + 2) + (1 + 6 + 2)
    assert chain_length(300 * 4096 + 1, 'clip') == (16 + 6 + 2) + (2 + 6 + 2)          # 301 blocks, 77 056 floats a trip
    assert chain_length(4198403, 'clip') == (17 + 6 + 2) + (4 + 6 + 2)                 # 1024 blocks, 262 144 floats a trip
    assert chain_length(4198403, 'mean_sq') == (17 + 6 + 3) + (4 + 6 + 3)


class Arena:
    """The device side of one direct-call case: the test's own tensors, ``step(i)`` applies the case's i-th gradient."""

    def __init__(self, case, form):
        self.case, self.form = case, form
        p0, self.grads = fc.make_case(case)
        self.n = p0.numel()
        self.p = p0.to(DEV)
        self.g, self.m, self.v = (torch.zeros(self.n, device=DEV) for _ in range(3))
        self.ws = torch.zeros(1024, device=DEV)
        self.sumsq = torch.full((), -1.0, device=DEV)
        self.step_t = torch.full((), float(case.t0), device=DEV)
        self.hyp = (float(case.lr), fc.BETAS[0], fc.BETAS[1], fc.EPS)

    def step(self, i):
        """Apply gradient i; returns the gradient arena as the Adam launch was given it."""
        self.g.copy_(self.grads[i])
        max_norm, st = float(self.case.max_norm or 0.0), lib.stream()
        if self.form == 'clip':
            given = self.g.clone()
            lib.call('gv_clip_adam_step', ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), self.n, ptr(self.ws), ptr(self.sumsq),
                     max_norm, *self.hyp, ptr(self.step_t), 1, st)
        else:
            self.step_t += 1
            sumsq = None
            if self.form == 'mean_sq':
                sumsq = self.sumsq
                lib.call('gv_mean_sq', ptr(self.g), self.n, 1.0, ptr(sumsq), ptr(self.ws), 0, st)
            elif self.form == 'decay':
                lib.call('gv_axpby', self.n, None, self.case.weight_decay, ptr(self.p), 1.0, ptr(self.g), st)
            given = self.g.clone()
            lib.call('gv_adam_step', ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), self.n, ptr(sumsq), max_norm, *self.hyp,
                     ptr(self.step_t), st)
        torch.cuda.synchronize()
        return given


def held(got, fix, f64, what, slack, tag):
    print(f'RATIO {tag} {what}: {fc.worst_ratio(got, fix, f64, slack):.3f}')
    fc.assert_bound(got, fix, f64, f'{tag} {what}', slack)


def sumsq_held(got, norm64, n, route, tag):
    exact = float(norm64) ** 2
    err = abs(float(got) - exact)
    if exact == 0.0:
        assert float(got) == 0.0, f'{tag}: sumsq {float(got)} of an all-zero gradient'
        return
    print(f'RATIO {tag} sumsq: {err / exact / sumsq_bound(n, route):.3f}')
    assert err <= sumsq_bound(n, route) * exact, f'{tag}: sumsq {float(got)!r} vs {exact!r}'


def run_arena(case, form, tag):
    fix, f64 = fc.references(case)
    a = Arena(case, form)
    for i in range(fc.STEPS):
        given = a.step(i)
        if form == 'clip':
            assert not a.g.any(), f'{tag}: the gradient arena is not cleared after step {i + 1}'
        else:
            assert torch.equal(a.g, given), f'{tag}: gv_adam_step wrote the gradient arena in step {i + 1}'
        if form in ('clip', 'mean_sq'):
            sumsq_held(a.sumsq, f64[i]['norm'], a.n, form, f'{tag} step {i + 1}')
        if i + 1 in fc.SLACK:
            for key, what in (('p', 'p'), ('m', 'exp_avg'), ('v', 'exp_avg_sq')):
                held(getattr(a, key), fix[i][key][0], f64[i][key][0], f'{what} after step {i + 1}', fc.SLACK[i + 1], tag)
    assert float(a.step_t) == case.t0 + fc.STEPS
    assert not torch.equal(a.p.cpu(), fc.make_case(case)[0])
    return a


# the forms that share a reference run one after the other: the cache of references holds a few cases only
@pytest.mark.parametrize('n, lr, form', [(n, lr, f) for n in fc.SIZES for lr in fc.LRS for f in FORMS],
                         ids=lambda x: str(x))
def test_entry_points_match_float64(n, lr, form):
    run_arena(case_of(n, lr, form), form, f'n{n}-lr{lr:g}-{form}')


EXTRA = {'edge-4097': dict(n=4097, lr=1e-2, kind='edge'), 'edge-257': dict(n=257, lr=1e-3, kind='edge'),
         't999': dict(n=4097, lr=1e-3, t0=999), 't99999': dict(n=4097, lr=1e-2, t0=99999),
         'zero-after': dict(n=4097, lr=1e-2, kind=(1e-6, 0.0, 0.0))}


@pytest.mark.parametrize('form', FORMS[:2])
@pytest.mark.parametrize('name', EXTRA)
def test_clip_edge_large_step_numbers_and_zero_gradients_match_float64(name, form):
    """The norm within 1 % on each side of max_norm; powf(beta, t) at t = 1000.. and 100 000.. (moments zero, as the references'
    preset state); two all-zero gradients after a non-zero one."""
    run_arena(case_of(form=form, **EXTRA[name]), form, f'{name}-{form}')


POSITIONS = (0, 63, 64, 255, 256, 4095, 4096, 262143, 262144, 4194303, 4194304)


@pytest.mark.parametrize('n', [4198403, 300 * 4096 + 1])
def test_norm_counts_every_element_once(n):
    """g = 2^-j at the j-th of the positions that fit (lane, wave, block, first-trip and cap boundaries, and n - 1), zero
    elsewhere: the squares 4^-j occupy disjoint bits, 23 at the most, so their float32 sum is exact in any order -- at twelve
    positions (4 - 4^-11) / 3.  A dropped or doubled position is a wrong bit."""
    pos = [i for i in POSITIONS if i < n - 1] + [n - 1]
    g0 = torch.zeros(n)
    g0[pos] = torch.tensor([2.0 ** -j for j in range(len(pos))])
    want = torch.tensor(sum(4.0 ** -j for j in range(len(pos))), dtype=torch.float32)
    assert float(want.double()) == sum(4.0 ** -j for j in range(len(pos)))           # representable: nothing was rounded
    if n == 4198403:
        assert len(pos) == 12 and float(want.double()) == (4 - 4.0 ** -11) / 3
    p, g, m, v = torch.zeros(n, device=DEV), g0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws, step_t = torch.zeros(1024, device=DEV), torch.zeros((), device=DEV)
    out = [torch.full((), -1.0, device=DEV) for _ in range(2)]
    lib.call('gv_mean_sq', ptr(g), n, 1.0, ptr(out[0]), ptr(ws), 0, lib.stream())
    lib.call('gv_clip_adam_step', ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(ws), ptr(out[1]), 1.0, 1e-3, *fc.BETAS, fc.EPS, ptr(step_t), 1,
             lib.stream())
    torch.cuda.synchronize()
    for o, what in zip(out, ('gv_mean_sq', 'gv_clip_adam_step')):
        assert int(o.cpu().view(torch.int32)) == int(want.view(torch.int32)), f'{what}: {float(o)!r} for {float(want)!r}'
    assert int((v.cpu() != 0).sum()) == len(pos) and not g.any()


@pytest.mark.parametrize('n', fc.SIZES[-2:])
def test_norm_of_a_dense_arena_is_within_the_derived_bound(n):
    """Random gradients (the scale-3 step of the size's case) against the float64 sum of the same float32 values, both routes,
    under ``chain_length``'s k u / (1 - k u); the float64 sum's own error (~1e-16 a term) is nothing beside it."""
    case = fc.arena_case(n, 1e-2)
    g0 = fc.make_case(case)[1][1]
    exact = float((g0.double() ** 2).sum())
    p, g, m, v = torch.zeros(n, device=DEV), g0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws, step_t = torch.zeros(1024, device=DEV), torch.zeros((), device=DEV)
    out = [torch.full((), -1.0, device=DEV) for _ in range(2)]
    lib.call('gv_mean_sq', ptr(g), n, 1.0, ptr(out[0]), ptr(ws), 0, lib.stream())
    lib.call('gv_clip_adam_step', ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(ws), ptr(out[1]), 1.0, 1e-3, *fc.BETAS, fc.EPS, ptr(step_t), 1,
             lib.stream())
    torch.cuda.synchronize()
    assert exact > 8 * n
    for o, route in zip(out, ('mean_sq', 'clip')):
        sumsq_held(o, exact ** 0.5, n, route, f'dense n{n} {route}')


SHAPES = ((37, 5), (4100,), (3, 4, 5), (1,), (300, 4099))       # no numel is a multiple of 64; padded: 1 234 240 floats, 302 partials


def make_opt(route, params, lr):
    from gcn_vae_amd import distributed as gdist
    from gcn_vae_amd.optim import FlatAdam
    if route == 'sharded':
        return gdist.ShardedFlatAdam(params, lr=lr, max_grad_norm=fc.MAX_NORM)
    return FlatAdam(params, lr=lr, max_grad_norm=fc.MAX_NORM if route == 'flat' else None)


def feed(opt, params, grads):
    opt.zero_grad()
    for p, gp in zip(params, grads):
        p.grad.copy_(gp.to(DEV))
    opt.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize('lr', fc.LRS)
@pytest.mark.parametrize('route', ['flat', 'sharded'])
def test_flat_adam_parameters_moments_padding_and_norm(route, lr):
    case = fc.Case(SHAPES, lr, fc.MAX_NORM, 0.0, 'scales', 0)
    fix, f64 = fc.references(case)
    p0, grads = fc.make_case(case)
    params = [torch.nn.Parameter(x.to(DEV)) for x in fc.split(p0, SHAPES)]
    opt = make_opt(route, params, lr)
    try:
        assert opt.total == 1234240 and opt.total % 4096 != 0
        pad = torch.ones(opt.total, dtype=torch.bool, device=DEV)
        for p in params:
            pad[opt.offsets[p]:opt.offsets[p] + p.numel()] = False
        assert int(pad.sum()) == opt.total - p0.numel()
        tag = f'{route}-lr{lr:g}'
        rel = sumsq_bound(opt.total, 'clip' if route == 'flat' else 'mean_sq')
        for i in range(fc.STEPS):
            feed(opt, params, fc.split(grads[i], SHAPES))
            assert not opt.flat_g.any()
            # sqrt halves the relative error of sumsq and adds one rounding: k u / 2 + u <= k u
            norm, want = float(opt.grad_norm()), float(f64[i]['norm'])
            print(f'RATIO {tag} grad_norm after step {i + 1}: {abs(norm - want) / want / rel:.3f}')
            assert abs(norm - want) <= rel * want
            for arena in (opt.flat_p, opt.exp_avg, opt.exp_avg_sq):
                assert not arena[pad].any(), f'{tag}: padding written in step {i + 1}'
            if i + 1 not in fc.SLACK:
                continue
            for j, p in enumerate(params):
                o, n = opt.offsets[p], p.numel()
                for got, key, what in ((p, 'p', 'p'), (opt.exp_avg[o:o + n], 'm', 'exp_avg'), (opt.exp_avg_sq[o:o + n], 'v', 'exp_avg_sq')):
                    held(got, fix[i][key][j], f64[i][key][j], f'{what}[{j}] after step {i + 1}', fc.SLACK[i + 1], tag)
        assert float(opt.step_t) == fc.STEPS
    finally:
        opt.close()


@pytest.mark.parametrize('form', FORMS[:2])
@pytest.mark.parametrize('n', [4097, 300 * 4096 + 1])
def test_all_zero_gradient_at_step_one_changes_nothing(n, form):
    case = fc.arena_case(n, 1e-2, kind=(0.0, 0.0, 0.0))
    a = Arena(case, form)
    a.step(0)
    assert torch.equal(a.p.cpu(), fc.make_case(case)[0])                   # p - lr * 0 / (0 + eps): the same bits
    assert not a.m.any() and not a.v.any() and float(a.sumsq) == 0.0 and float(a.step_t) == 1
    assert bool(torch.isfinite(a.p).all())


@pytest.mark.parametrize('form', FORMS[:2])
def test_zero_gradient_after_a_step_still_moves_the_parameters(form):
    """As torch does: the first moment lives on.  (The values are held to the references in the 'zero-after' case above.)"""
    a = Arena(case_of(form=form, **EXTRA['zero-after']), form)
    a.step(0)
    p1, m1, v1 = a.p.clone(), a.m.clone(), a.v.clone()
    a.step(1)
    live = m1 != 0
    assert int(live.sum()) > 0.99 * a.n and bool((a.p != p1)[live].all()) and bool(((a.p < p1) == (m1 > 0))[live].all())
    assert bool((a.m.abs() < m1.abs())[live].all()) and bool((a.v < v1)[live].all()) and float(a.sumsq) == 0.0


BAD_N, BAD_AT = 3 * 4096 + 1, 5000          # four partials of 1024 floats a trip: index 5000 is read in a later trip


@pytest.mark.parametrize('bad', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('route', ['flat', 'sharded'])
def test_non_finite_gradient_is_visible_and_stays_in_its_element(route, bad):
    """PINNED, not endorsed (optim.py's docstring states it).  One non-finite gradient element after one ordinary step:
      * grad_norm() is non-finite (NaN for a NaN, inf for an inf), so a driver can see it;
      * NaN: fminf(1, NaN) = 1, so the step runs UNCLIPPED: every other element is, bit for bit, a FlatAdam without
        max_grad_norm on the same gradient, and only the element itself turns NaN (p and both moments).  torch's
        clip_grad_norm_ multiplies every gradient by the NaN coefficient and loses every parameter;
      * inf: the coefficient is max_norm / inf = 0, so every other element sees a zero gradient (bit for bit the same optimiser
        fed zeros: the parameters still move by their first moment) and the element itself is inf * 0 = NaN.  torch does the same.
    """
    case = fc.arena_case(BAD_N, 1e-2)
    p0, grads = fc.make_case(case)
    nan = bad != bad
    g2, g2_twin = grads[1].clone(), grads[1].clone()
    assert float(g2.norm()) > 100 * fc.MAX_NORM                   # a clip, had there been one, would have shown
    g2[BAD_AT] = bad
    g2_twin[BAD_AT] = 0.0
    if not nan:
        g2_twin.zero_()
    pa, pb = ([torch.nn.Parameter(p0.to(DEV))] for _ in range(2))
    opt, twin = make_opt(route, pa, 1e-2), make_opt('plain' if nan else route, pb, 1e-2)
    try:
        for o, ps in ((opt, pa), (twin, pb)):
            feed(o, ps, [grads[0]])                   # clip idle: coefficient 1 in every route
        assert torch.equal(pa[0], pb[0]) and not torch.equal(pa[0].cpu(), p0)
        feed(opt, pa, [g2])
        feed(twin, pb, [g2_twin])
        norm = float(opt.grad_norm())
        assert norm != norm if nan else norm == float('inf')
        others = torch.ones(BAD_N, dtype=torch.bool, device=DEV)
        others[BAD_AT] = False
        for mine, theirs, what in ((pa[0], pb[0], 'p'), (opt.exp_avg[:BAD_N], twin.exp_avg[:BAD_N], 'exp_avg'),
                                   (opt.exp_avg_sq[:BAD_N], twin.exp_avg_sq[:BAD_N], 'exp_avg_sq')):
            assert bool(torch.isnan(mine[BAD_AT])), f'{what}[{BAD_AT}] = {float(mine[BAD_AT])}'
            assert bool(torch.isfinite(mine[others]).all()) and torch.equal(mine[others], theirs[others]), what
        assert not torch.equal(pa[0][others], p0.to(DEV)[others])
        for o in (opt, twin):
            assert not o.flat_p[BAD_N:].any() and not o.exp_avg[BAD_N:].any() and not o.exp_avg_sq[BAD_N:].any()
    finally:
        opt.close()
        twin.close()


@pytest.mark.parametrize('wrong', fc.WRONG)
@pytest.mark.parametrize('lr', fc.LRS)
def test_bound_rejects_a_wrong_rule(lr, wrong):
    """On test (1)'s inputs, references and bound, the three-step parameters of a rule that is wrong in one detail fail and the
    right rule's pass (float32 hand statements stand in for a device: what is shown is that the bound tells them apart)."""
    case = fc.arena_case(4097, lr)
    fix, f64 = fc.references(case)
    good, bad = fc.hand_steps(case, torch.float32), fc.hand_steps(case, torch.float32, wrong)
    ref = (fix[-1]['p'][0], f64[-1]['p'][0])
    fc.assert_bound(good[-1][0], *ref, 'p', fc.SLACK[fc.STEPS])
    with pytest.raises(AssertionError):
        fc.assert_bound(bad[-1][0], *ref, f'{wrong} p', fc.SLACK[fc.STEPS])
    assert fc.worst_ratio(bad[-1][0], *ref, fc.SLACK[fc.STEPS]) > 100
