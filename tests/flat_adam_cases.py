"""Constructed inputs and references for the flat clip+Adam tests (test_flat_adam_host.py without a GPU, test_gpu_flat_adam.py
on the device): gv_clip_adam_step / gv_adam_step (k_gradsq_part and k_adam of csrc/k_elem.hip), optim.FlatAdam and
distributed.ShardedFlatAdam.

``hand_step`` is a hand-written statement of ``clip_grad_norm_`` + ``torch.optim.Adam`` over one arena in whatever dtype its
tensors have (clip coefficient min(1, max_norm / (norm + 1e-6)); coupled weight decay g += wd * p when there is no clip; bias
correction; eps outside the root); its ``wrong`` argument states three broken variants that a useful bound must reject.

``make_case`` builds the inputs.  Parameters are 0.01 * randn, so an update of size lr (1e-2 or 1e-3) is visible against |p|.
A case runs STEPS steps whose gradients are ``scale * randn`` with the scales (1e-6, 3.0, 1e-6): clip idle, clip far active, clip
idle with history ('edge': the norm set to 0.995 / 1.005 / 0.995 of max_norm; a scale of 0 is an all-zero gradient).  Every
non-zero gradient carries 2^-40 at index 7 and +-2^-27 at indices 9 and 11 (|g| ~ eps = 1e-8: only these see where eps sits).
A case may start from a preset step counter ``t0`` (moments zero), which holds powf(beta, t) at large t to the references.

``references`` runs real ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.Adam`` on the CPU in float32 (the fixture) and float64
(the truth) and records parameters, both moments and the float64 pre-clip norm after every step.  The C ABI takes lr, the betas,
eps and max_norm as ``float``: the kernel is a self-consistent Adam with beta2 = float32(0.999) = 0.99900001287..., whose
1 - beta2 = 0.00099998713 is 1.3e-5 below 0.001 -- more than the step-1 bound allows on exp_avg_sq (``kernel_restatement`` with
``b2_exact=True`` shows it).  That is the ABI and no error, so both references get the float32-rounded values, as Python floats.

``kernel_restatement`` is k_adam's arithmetic in float32 numpy, in the kernel's order of operations: the proof, without a device,
that these inputs leave room for a correct kernel under ``bound_of``.
"""
import collections
import functools

import numpy as np
import torch

STEPS = 3
MAX_NORM = 1.0
WEIGHT_DECAY = 5e-4
BETAS = (0.9, 0.999)
EPS = 1e-8
LRS = (1e-2, 1e-3)
SCALES = (1e-6, 3.0, 1e-6)
EDGE = (0.995, 1.005, 0.995)         # 'edge': the gradient norm as a share of max_norm
# one partial with idle threads | two partials, the second with one element | 301 partials: the second trip of k_adam's
# partial loop | past the 1024-partial cap and the 2048-block cap, with a ragged tail
SIZES = (1, 63, 257, 4097, 300 * 4096 + 1, 4194304 + 4096 + 3)
SLACK = {1: 1e-5, STEPS: 1e-4}       # the project's numbers for its other optimisers (test_gpu_transe_opt.py)
WRONG = ('no_bias_correction', 'eps_inside_root', 'clip_after_moments')

# shapes: the parameter tensors (one 1-D tensor for a direct ABI call); kind: 'scales', 'edge' or a tuple of three scales
Case = collections.namedtuple('Case', 'shapes lr max_norm weight_decay kind t0')


def arena_case(n, lr, max_norm=MAX_NORM, weight_decay=0.0, kind='scales', t0=0):
    return Case(((n,),), lr, max_norm, weight_decay, kind, t0)


def r32(x):
    """The hyperparameter as the kernel receives it (the ABI's float), as a Python float."""
    return float(np.float32(x))


def bound_of(fix, f64, slack):
    """4 |fixture - float64| + slack * (max |float64| of the element's ROW; of the whole tensor below 2-D): test_gpu_transe's,
    verbatim.  The callers here pass flattened tensors: the scale is per parameter tensor, or per arena for a direct call."""
    scale = f64.abs().amax(dim=-1, keepdim=True) if f64.dim() >= 2 else f64.abs().max()
    return 4 * (fix - f64).abs() + slack * (scale + 1e-30)


def as_f64(x):
    return torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)).double().reshape(-1)


def worst_ratio(got, fix, f64, slack):
    """max |got - fixture| / bound_of: how much of the bound ``got`` uses (above 1: it fails)."""
    got, fix, f64 = as_f64(got), as_f64(fix), as_f64(f64)
    return float(((got - fix).abs() / bound_of(fix, f64, slack)).max())


def assert_bound(got, fix, f64, what, slack):
    got, fix, f64 = as_f64(got), as_f64(fix), as_f64(f64)
    bound = bound_of(fix, f64, slack)
    err = (got - fix).abs()
    assert bool((err <= bound).all()), f'{what}: worst excess {float((err - bound).max()):.3e} (max err {float(err.max()):.3e})'


def numel(shape):
    return int(np.prod(shape))


@functools.lru_cache(maxsize=4)
def make_case(case):
    """(p0, [g_1 .. g_STEPS]): float32 tensors of the case's total length (the parameters one after another, unpadded)."""
    n = sum(numel(s) for s in case.shapes)
    rs = np.random.RandomState(n % 9973 + 17)
    p0 = torch.from_numpy((0.01 * rs.standard_normal(n)).astype(np.float32))
    grads = []
    for i in range(STEPS):
        g = rs.standard_normal(n)
        if n == 1:
            g = np.sign(g) * (0.5 + np.abs(g))          # one element: keep |g| off zero, so that scale 3 still clips
        if case.kind == 'edge':
            g *= EDGE[i] * case.max_norm / np.sqrt((g * g).sum())
        else:
            g *= (SCALES if case.kind == 'scales' else case.kind)[i]
        g = g.astype(np.float32)
        if g.any():
            for idx, val in ((7, 2.0 ** -40), (9, 2.0 ** -27), (11, -2.0 ** -27)):
                if idx < n:
                    g[idx] = val
        grads.append(torch.from_numpy(g))
    return p0, grads


def split(flat, shapes):
    """The unpadded flat tensor cut into the case's parameter tensors (copies)."""
    out, o = [], 0
    for s in shapes:
        out.append(flat[o:o + numel(s)].clone().reshape(s))
        o += numel(s)
    return out


def torch_steps(case, dtype):
    """The case's steps by clip_grad_norm_ + torch.optim.Adam on the CPU in ``dtype`` with the float32-rounded hyperparameters:
    [dict(p=[..], m=[..], v=[..], norm=pre-clip total norm in ``dtype``)] after each step, one tensor per parameter."""
    p0, grads = make_case(case)
    # clone BEFORE wrapping: .to(float32) of a float32 tensor is the tensor itself, and the float32 run would step p0 in place
    params = [torch.nn.Parameter(x.clone().to(dtype)) for x in split(p0, case.shapes)]
    opt = torch.optim.Adam(params, lr=r32(case.lr), betas=(r32(BETAS[0]), r32(BETAS[1])), eps=r32(EPS),
                           weight_decay=r32(case.weight_decay), foreach=False)
    if case.t0:
        for p in params:
            opt.state[p] = dict(step=torch.tensor(float(case.t0)), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    out = []
    for g in grads:
        for p, gp in zip(params, split(g, case.shapes)):
            p.grad = gp.to(dtype)
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
        if case.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(params, r32(case.max_norm))
        opt.step()
        out.append(dict(p=[p.detach().clone() for p in params], m=[opt.state[p]['exp_avg'].clone() for p in params],
                        v=[opt.state[p]['exp_avg_sq'].clone() for p in params], norm=norm.clone()))
    assert all(int(opt.state[p]['step']) == case.t0 + STEPS for p in params)
    return out


@functools.lru_cache(maxsize=2)
def references(case):
    """(float32 fixture, float64 truth) of ``torch_steps``.  Cached: the tests that share a case share its references, and none
    changes them."""
    return torch_steps(case, torch.float32), torch_steps(case, torch.float64)


def hand_step(p, g, m, v, t, lr, b1, b2, eps, max_norm, weight_decay, wrong=None):
    """One clip + Adam step over one arena at the 1-based step ``t``, out of place, in the dtype of the tensors: returns
    (p, m, v).  ``wrong``: one of WRONG."""
    clip = 1.0
    if max_norm is not None:
        clip = torch.clamp(max_norm / ((g * g).sum().sqrt() + 1e-6), max=1.0)
    elif weight_decay:
        g = g + weight_decay * p
    gm = g if wrong == 'clip_after_moments' else g * clip
    bc1, bc2 = (1.0, 1.0) if wrong == 'no_bias_correction' else (1 - b1 ** t, 1 - b2 ** t)
    m = b1 * m + (1 - b1) * gm
    v = b2 * v + (1 - b2) * gm * gm
    if wrong == 'eps_inside_root':
        denom = (v / bc2 + eps).sqrt()
    else:
        denom = v.sqrt() / bc2 ** 0.5 + eps
    upd = (lr / bc1) * m / denom
    if wrong == 'clip_after_moments':
        upd = upd * clip
    return p - upd, m, v


def hand_steps(case, dtype, wrong=None):
    """A one-tensor case's steps by ``hand_step`` in ``dtype`` with the float32-rounded hyperparameters: [(p, m, v)]."""
    p0, grads = make_case(case)
    p = p0.clone().to(dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for i, g in enumerate(grads, 1):
        p, m, v = hand_step(p, g.to(dtype), m, v, case.t0 + i, r32(case.lr), r32(BETAS[0]), r32(BETAS[1]), r32(EPS),
                            None if case.max_norm is None else r32(case.max_norm), r32(case.weight_decay), wrong)
        out.append((p, m, v))
    return out


def kernel_restatement(case, b2_exact=False):
    """A one-tensor case's steps in k_adam's float32 arithmetic and order of operations (the axpby of the weight decay in front,
    the sum of squares by numpy's float32 sum): [(p, m, v)] as float32 numpy arrays.  ``b2_exact``: beta2 reaches the second moment
    as the double 0.999 instead of the ABI's float -- what the references would have to assume, were they given 0.999."""
    f = np.float32
    p0, grads = make_case(case)
    p = p0.numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    lr, b1, b2, eps = f(case.lr), f(BETAS[0]), f(BETAS[1]), f(EPS)
    out = []
    for i, g in enumerate(grads, 1):
        g = g.numpy()
        clip = f(1)
        if case.max_norm is not None:
            tot = (g * g).sum(dtype=f)
            clip = min(f(1), f(case.max_norm) / (np.sqrt(tot) + f(1e-6)))
        elif case.weight_decay:
            g = f(case.weight_decay) * p + f(1) * g
        t = f(case.t0 + i)
        bc1, bc2 = f(1) - np.power(b1, t), f(1) - np.power(b2, t)
        step_size, inv_sqrt_bc2 = lr / bc1, f(1) / np.sqrt(bc2)
        gi = g * clip
        m = b1 * m + (f(1) - b1) * gi
        if b2_exact:
            v = (BETAS[1] * v.astype(np.float64) + (1 - BETAS[1]) * (gi * gi).astype(np.float64)).astype(f)
        else:
            v = b2 * v + (f(1) - b2) * gi * gi
        p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
        assert p.dtype == m.dtype == v.dtype == f
        out.append((p, m, v))
    return out
