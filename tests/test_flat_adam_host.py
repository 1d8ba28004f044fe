"""The flat clip+Adam tests' own footing (no GPU): the hand statement of flat_adam_cases is torch's rule; the bound of
test_gpu_flat_adam.py rejects three rules that are wrong in one detail; a float32 restatement of k_adam stays under half of that
bound on every case, so the inputs leave room for a correct kernel; and the same restatement with beta2 as the double 0.999 does
not, which is why the references take the float32-rounded hyperparameters."""
import numpy as np
import pytest
import torch

import flat_adam_cases as fc

HOST_SIZES = [n for n in fc.SIZES if n <= 300 * 4096 + 1]
EXTRA = [fc.arena_case(4097, 1e-2, kind='edge'), fc.arena_case(257, 1e-3, kind='edge'),
         fc.arena_case(4097, 1e-3, t0=999), fc.arena_case(4097, 1e-2, t0=99999),
         fc.arena_case(4097, 1e-2, kind=(1e-6, 0.0, 0.0))]


def kinds(n, lr):
    """The three references a size is held to on the device: clipped, plain, weight decay."""
    return [fc.arena_case(n, lr), fc.arena_case(n, lr, max_norm=None), fc.arena_case(n, lr, max_norm=None, weight_decay=fc.WEIGHT_DECAY)]


def case_id(c):
    return f'n{fc.numel(c.shapes[0])}-lr{c.lr:g}-clip{c.max_norm}-wd{c.weight_decay:g}-{c.kind}-t{c.t0}'


def test_rounded_hyperparameters_are_what_the_abi_passes():
    assert fc.r32(0.999) == 0.9990000128746033 and abs((1 - fc.r32(0.999)) / 1e-3 - 1) > 1.2e-5
    # 1 - float32(beta) is a float32 again: the kernel's 1.f - b and the references' 1 - beta (a double) are one number
    for b in fc.BETAS:
        assert float(np.float32(1) - np.float32(b)) == 1 - fc.r32(b)


def test_case_inputs_are_what_the_docstring_says():
    c = fc.arena_case(4097, 1e-2)
    p0, grads = fc.make_case(c)
    assert p0.dtype == torch.float32 and 0.005 < float(p0.abs().mean()) < 0.012
    for g, scale in zip(grads, fc.SCALES):
        assert float(g[7]) == 2.0 ** -40 and float(g[9]) == 2.0 ** -27 and float(g[11]) == -2.0 ** -27
        assert 0.9 * scale * 64 < float(g.double().norm()) < 1.1 * scale * 64
    for n in fc.SIZES[:4]:                       # clip idle, far active, idle: at every size, the single element included
        _, grads = fc.make_case(fc.arena_case(n, 1e-2))
        norms = [float(g.double().norm()) for g in grads]
        assert norms[0] < 0.01 * fc.MAX_NORM and norms[1] > 1.4 * fc.MAX_NORM and norms[2] < 0.01 * fc.MAX_NORM
    _, grads = fc.make_case(EXTRA[0])
    shares = [float(g.double().norm()) / fc.MAX_NORM for g in grads]
    # (planting the three tiny values takes three of the 4097 random ones out of the norm: 1e-3 of it at the most)
    assert all(abs(s / e - 1) < 2e-3 for s, e in zip(shares, fc.EDGE)) and 0.99 < shares[0] < 1 < shares[1] < 1.01
    _, grads = fc.make_case(EXTRA[4])
    assert float(grads[0].abs().max()) > 0 and not grads[1].any() and not grads[2].any()


def test_references_do_not_share_storage_with_the_case():
    c = fc.arena_case(257, 1e-2)
    p0 = fc.make_case(c)[0].clone()
    fix, f64 = fc.references(c)
    assert torch.equal(fc.make_case(c)[0], p0)                      # the float32 run stepped a copy
    assert fix[0]['p'][0].dtype == torch.float32 and f64[0]['p'][0].dtype == torch.float64
    assert not torch.equal(fix[-1]['p'][0], p0)


@pytest.mark.parametrize('case', kinds(4097, 1e-2) + kinds(63, 1e-3) + EXTRA, ids=case_id)
def test_hand_step_float64_equals_torch(case):
    """Parameters and both moments after every step to 1e-12: a handful of float64 operations an element.  The second moment
    is a sum of non-negative terms and is held element by element, the 2^-80 of the planted gradient included; a parameter or a
    first moment can cancel to nothing (p crosses zero, 0.9 m meets -0.1 g), so these are held to 1e-12 of the tensor's largest."""
    _, f64 = fc.references(case)
    want = fc.hand_steps(case, torch.float64)
    for step, (ref, w) in enumerate(zip(f64, want), 1):
        for what, a, b in (('p', ref['p'][0], w[0]), ('exp_avg', ref['m'][0], w[1]), ('exp_avg_sq', ref['v'][0], w[2])):
            assert a.dtype == b.dtype == torch.float64
            err = (a - b).abs()
            scale = a.abs() if what == 'exp_avg_sq' else a.abs().max()
            assert bool((err <= 1e-12 * scale.clamp_min(1e-300)).all()), f'step {step} {what}: {float(err.max()):.3e}'
    assert not torch.equal(f64[-1]['p'][0], fc.make_case(case)[0].double())


@pytest.mark.parametrize('wrong', fc.WRONG)
@pytest.mark.parametrize('lr', fc.LRS)
def test_bound_rejects_the_wrong_variants(lr, wrong):
    """float32 hand statements stand in for a device.  The right rule passes; each wrong one exceeds the bound on the parameters
    after step 3 by a wide factor (measured here, asserted at 100: no_bias_correction and eps_inside_root are above 500)."""
    case = fc.arena_case(4097, lr)
    fix, f64 = fc.references(case)
    good = fc.hand_steps(case, torch.float32)
    bad = fc.hand_steps(case, torch.float32, wrong)
    slack = fc.SLACK[fc.STEPS]
    assert fc.worst_ratio(good[-1][0], fix[-1]['p'][0], f64[-1]['p'][0], slack) < 0.5
    ratio = fc.worst_ratio(bad[-1][0], fix[-1]['p'][0], f64[-1]['p'][0], slack)
    print(f'RATIO wrong {wrong} lr{lr:g} p after step {fc.STEPS}: {ratio:.1f}')
    assert ratio > 100


def test_torch_clip_spreads_a_nan_and_turns_an_inf_into_zero_gradients():
    """What optim.py's docstring sets the kernel's pinned behaviour against (test_gpu_flat_adam.py pins the kernel's)."""
    for bad, rest in ((float('nan'), float('nan')), (float('inf'), 0.0)):
        p = torch.nn.Parameter(torch.ones(4))
        p.grad = torch.tensor([1.0, bad, -2.0, 3.0])
        norm = torch.nn.utils.clip_grad_norm_([p], 1.0)
        assert not bool(torch.isfinite(norm)) and bool(torch.isnan(p.grad[1]))
        others = p.grad[[0, 2, 3]]
        assert bool(torch.isnan(others).all()) if rest != rest else bool((others == 0).all())


ROOM = [c for n in HOST_SIZES for lr in fc.LRS for c in kinds(n, lr)] + EXTRA


@pytest.mark.parametrize('case', ROOM, ids=case_id)
def test_kernel_restatement_leaves_half_the_bound(case):
    fix, f64 = fc.references(case)
    got = fc.kernel_restatement(case)
    for step in sorted(fc.SLACK):
        for k, what in enumerate(('p', 'm', 'v')):
            ratio = fc.worst_ratio(got[step - 1][k], fix[step - 1][what][0], f64[step - 1][what][0], fc.SLACK[step])
            print(f'RATIO restatement {case_id(case)} {what} after step {step}: {ratio:.3f}')
            assert ratio < 0.5, f'{what} after step {step}: {ratio:.3f} of the bound'


def test_unrounded_beta2_exceeds_the_bound_on_the_second_moment():
    """A kernel fed beta2 = 0.999 as a double differs from one fed the ABI's float by 1.3e-5 of exp_avg_sq at step 1, which the
    1e-5 slack refuses: held to references on 0.999 the kernel would fail for its ABI and not for an error."""
    case = fc.arena_case(4097, 1e-2)
    fix, f64 = fc.references(case)
    got = fc.kernel_restatement(case, b2_exact=True)
    assert fc.worst_ratio(got[0][2], fix[0]['v'][0], f64[0]['v'][0], fc.SLACK[1]) > 1.2
    assert fc.worst_ratio(got[0][1], fix[0]['m'][0], f64[0]['m'][0], fc.SLACK[1]) < 0.5     # beta1 is not involved
