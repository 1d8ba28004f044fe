"""Constructed inputs, float64 references, bounds and float32 restatements for the MMD pair and the prior sampler
(test_mmd_host.py without a GPU, test_gpu_mmd.py on the device): gv_mmd_fwd / gv_mmd_bwd (k_mmd_fwd<4|16>, k_mmd_fwd_g<4|8>,
k_mmd_bwd<4|16>, k_mmd_bwd_g<4> of csrc/k_loss.hip) and gv_prior_sample_fwd / gv_prior_sample_bwd.

    K(a, b) = exp(-|a - b|^2 / h^2),    mmd = sum Kxx / sx^2 + sum Kyy / sy^2 - 2 sum Kxy / (sx sy)
    d mmd / d a = sum_j t_j,   t_j = c_j K_j (a - b_j),   c_same = g (-2 / h^2) 2 / n_same^2,  c_other = g (-2 / h^2) (-2) / (sx sy)

with g = gscale * gmmd, j over the rows of a's own set and then over the other set's.

INPUTS.  ``make_case(sx, sy, h, scale, seed)``: x = randn, y = 0.7 randn + 0.1.  Scale 'n' leaves them so: the exponents e = d^2 / h^2
are about 2 / h and K is about 1 (the regime training is in); the 0.1 offset of y keeps the two sets' means apart, which is what
the gradient is made of there.  Scale 'w' multiplies both by 0.7 sqrt(h): the exponents then lie around 0.5 (yy), 0.7 (xy) and 1.0
(xx), K is far from 1, and a wrong exponent or a dropped expf is visible.  sx != sy except in the single-row case (1 / sx^2,
1 / sy^2 and 1 / (sx sy) are one number at sx = sy).

REFERENCES.  Float64 from the fp32 inputs: the per-block forward partials in gv_mmd_fwd's workspace layout (x rows, then y rows),
the value, both gradients element by element, and -- ``indexed_reference`` -- what every row of a pre-filled gy must end at when y
is rows ``pick`` (with repeats) of a taller matrix.

BOUND (u = 2^-24), per output element, from a count of the roundings in k_mmd_*:

    u sum_j |t_j| (N + 12 + (h + 4) e_j)

  (h + 4) e_j   the exponent: h differences (1 rounding each, 2 on the square), a sum of h non-negative squares in any order (fma
                chains of 4 or 16 a lane, then a 16- or 64-lane tree: at most h - 1 roundings), 1 / (h h) (h h is exact up to
                1024^2; the division rounds once) and the product d^2 * inv: at most (h + 3) u relative on e, which is an
                ABSOLUTE error of (h + 3) u e on the argument of expf, hence relative on K.
  12            the rest of one term: g = gscale * gmmd (1), g * (-2 inv) (1; the 2s are exact), inv again as a factor (1), the
                division by n n or sx sy (1; the integer product is exact), expf at 2 ulp = 4 u (HIP documents 1 ulp; the build
                passes no -fgpu-approx-transcendentals, see _build.py), cf * expf (1), a - b_j (1): 10.  A forward term wt * K_j
                has wt (1), expf (4), the product (1): 6.  12 leaves two to spare.
  N             a float32 sum of N terms in ANY order is within (N - 1) u sum |t_j|; the fma accumulations, the adds across a
                wave's four groups and across the 16 waves are that sum.  N = n_same + n_other for a gradient element, the
                block's own term count for a forward partial (sx + sy for an x row, sy for a y row), where t_j = wt K_j.

The VALUE is held to the float64 sum of the fp32 partials the kernel stored (themselves bound-checked): (sx + sy) u sum |partial|
+ u |sum| (k_final_sum adds sx + sy numbers in some order and rounds the scaled result).  On the INDEXED path an element that m
positions of ``pick`` name gets m atomic adds: m u (|prefill| + sum |contribution|) on top of the contributions' own bounds.

``restate`` is the kernels' arithmetic in float32 torch; ``wrong`` states rules that are off in one detail (WRONG).

PRIOR SAMPLER.  z_pre = [mu; raw] (2k, h), eps (s, h), s = k * repeat:  out_r = mu_j + eps_r sd_j,  sd = sqrt(softplus(raw) + 1e-8),
j = r % k.  Forward bound u (|out| + 8 |eps sd|): expf (2 u), log1pf (2 u; it does not amplify the error of its argument), + 1e-8f
(1) -> 5 u on the variance, halved by the root, + sqrtf (1) = 3.5 u on sd, the product (1): 4.5, counted as 8 (which also covers
1e-8f against 1e-8 and softplus against the raw value above 20: 1e-8 relative at the most); the final add rounds out.  Backward:
mu half (s / k) u sum_r |g_r| (a sum of s / k terms); raw half (s / k + 12) u sum_r |g_r eps_r| f with f = 0.5 / sd * (raw > 20 ?
1 : sigmoid(raw)), the factor the kernel applies: a product per term (1), the sum (s / k), sd (3.5), the division (1), the sigmoid
(expf 2 u damped by expf / (1 + expf) <= 1, the add, the division: 4), the last product (1): 10.5, counted as 12.  Accumulating
adds u |prefill + value|.  Raw values -30, -5, 0, 19.99, 20.01 and 50 are planted in row k of z_pre (component 0).
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
SCALES = ('n', 'w')
# what the backward is called with at each scale: (gscale, gmmd); gmmd None = the NULL pointer
GRAD_ARGS = {'n': (1.0, None), 'w': (0.37, 1.3)}

# (sx, sy, h).  Row-of-16 forms (128 partner rows a trip, 64 groups): counts 1, 63, 65, 129, 130 at h = 4, 200, 256 (g<4>) and 260,
# 512 (forward g<8>, backward <16>).  Lane-per-column forms (forward 64 a trip with tails at +16, +32, +48; backward 32 a trip):
# counts 1, 17, 33, 49, 65 at h = 30, 6 (<4>) and 258, 516, 1024 (<16>).
FORM_SHAPES = ((1, 1, 4), (63, 130, 4), (65, 129, 200), (129, 65, 200), (130, 63, 256), (130, 1, 260), (65, 129, 512),
               (17, 33, 30), (33, 17, 30), (49, 65, 6), (65, 1, 30), (17, 33, 258), (33, 49, 516), (65, 17, 1024))
INDEX_SHAPES = ((40, 200), (33, 258))          # (sx, h): y is 300 rows, pick 70 positions
INDEX_ROWS, INDEX_PICKS = 300, 70
INSTANCES = ('k_mmd_fwd_g<4>', 'k_mmd_fwd_g<8>', 'k_mmd_fwd<4>', 'k_mmd_fwd<16>', 'k_mmd_bwd_g<4>', 'k_mmd_bwd<4>', 'k_mmd_bwd<16>')
WRONG = ('k_is_one', 'cross_weight', 'drop_last_same', 'drop_last_other', 'index_off_by_one', 'store_not_add', 'gscale_dropped')

SAMPLER_SHAPES = ((1, 4, 1), (10, 200, 20), (3, 258, 7), (4, 1024, 2))       # (k, h, repeat)
PLANT = (19.99, 20.01, -30.0, 0.0, -5.0, 50.0)
SAMPLER_WRONG = ('no_threshold', 'sigmoid_dropped', 'eps_dropped', 'stride_k_wrong')


def r32(v):
    """A scalar as the ABI's ``float`` carries it, as a Python float."""
    return float(np.float32(v))


def dispatch(h, aligned=True, rows16=True):
    """The kernel instantiations gv_mmd_fwd and gv_mmd_bwd launch (csrc/k_loss.hip), restated: ``aligned`` = every operand on a
    16-byte boundary, ``rows16`` = GV_MMD_ROWS16 unset or non-zero."""
    al = rows16 and aligned and h % 4 == 0
    if al and h <= 256:
        fwd = 'k_mmd_fwd_g<4>'
    elif al and h <= 512:
        fwd = 'k_mmd_fwd_g<8>'
    else:
        fwd = 'k_mmd_fwd<4>' if h <= 256 else 'k_mmd_fwd<16>'
    if al and h <= 256:
        bwd = 'k_mmd_bwd_g<4>'
    else:
        bwd = 'k_mmd_bwd<4>' if h <= 256 else 'k_mmd_bwd<16>'
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def make_case(sx, sy, h, scale='n', seed=None):
    gen = torch.Generator().manual_seed(7 * sx + 3 * sy + h if seed is None else seed)
    x = torch.randn(sx, h, generator=gen)
    y = torch.randn(sy, h, generator=gen) * 0.7 + 0.1
    if scale == 'w':
        f = torch.tensor(0.7 * float(np.sqrt(h)), dtype=torch.float32)
        x, y = x * f, y * f
    return x, y


@functools.lru_cache(maxsize=None)
def make_index_case(sx, h, scale='n'):
    """(x, y of INDEX_ROWS rows, pick, prefill): ``pick`` has INDEX_PICKS positions over 38 distinct rows -- row 5 is named three
    times, row 11 by the first and the last position, 29 rows twice -- none of them the last row (so that 'index_off_by_one' stays in bounds)."""
    x, y = make_case(sx, INDEX_ROWS, h, scale, seed=1000 + sx + h)
    gen = torch.Generator().manual_seed(h)
    rows = torch.randperm(INDEX_ROWS - 1, generator=gen)[:40]
    rows = rows[(rows != 5) & (rows != 11)][:36]
    inner = torch.cat([rows, rows[:29], torch.tensor([5, 5, 5])])
    inner = inner[torch.randperm(inner.numel(), generator=gen)]
    pick = torch.cat([torch.tensor([11]), inner, torch.tensor([11])]).to(torch.int64)
    assert pick.numel() == INDEX_PICKS
    prefill = torch.randn(INDEX_ROWS, h, generator=gen)
    return x, y, pick, prefill


# ---- float64 / float32 building blocks (one code path, the dtype of the operands decides) ------------------------------------
def _chunks(n, per_row):
    step = max(1, (1 << 22) // max(1, per_row))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def sqdist(a, b):
    """|a_i - b_j|^2 as the sum of the squared differences (never the |a|^2 + |b|^2 - 2 ab form)."""
    out = a.new_empty(a.shape[0], b.shape[0])
    for r0, r1 in _chunks(a.shape[0], b.shape[0] * a.shape[1]):
        d = a[r0:r1, None, :] - b[None]
        out[r0:r1] = (d * d).sum(-1)
    return out


def contract(a, b, c, w=None):
    """sum_j c_ij (a_i - b_j)  and, with ``w``, sum_j |c_ij| |a_i - b_j| and sum_j |c_ij| w_ij |a_i - b_j|  (each (rows of a, h))."""
    out = a.new_zeros(a.shape)
    asum, wsum = (a.new_zeros(a.shape), a.new_zeros(a.shape)) if w is not None else (None, None)
    for r0, r1 in _chunks(a.shape[0], b.shape[0] * a.shape[1]):
        d = a[r0:r1, None, :] - b[None]
        out[r0:r1] = (c[r0:r1, :, None] * d).sum(1)
        if w is not None:
            d = d.abs_()
            ca = c[r0:r1].abs()
            asum[r0:r1] = (ca[:, :, None] * d).sum(1)
            wsum[r0:r1] = ((ca * w[r0:r1])[:, :, None] * d).sum(1)
    return out, asum, wsum


def grad_scale(gscale, gmmd):
    return r32(gscale) * (1.0 if gmmd is None else r32(gmmd))


def references(x, y, gscale=1.0, gmmd=None):
    """Float64 references and bounds for dense x (sx, h), y (sy, h): dict(partials, partials_bound, mmd, gx, gx_bound, gy, gy_bound,
    gx_abs, gy_abs (sum_j |t_j|), exponents=(exx, eyy, exy))."""
    x, y = x.double(), y.double()
    (sx, h), sy = x.shape, y.shape[0]
    h2 = float(h) * float(h)
    exx, eyy, exy = sqdist(x, x) / h2, sqdist(y, y) / h2, sqdist(x, y) / h2
    kxx, kyy, kxy = torch.exp(-exx), torch.exp(-eyy), torch.exp(-exy)
    n = sx + sy

    def wt(e, terms):
        return terms + 12 + (h + 4) * e
    px = kxx.sum(1) / sx ** 2 - 2 * kxy.sum(1) / (sx * sy)
    py = kyy.sum(1) / sy ** 2
    bx = U * ((kxx * wt(exx, n)).sum(1) / sx ** 2 + 2 * (kxy * wt(exy, n)).sum(1) / (sx * sy))
    by = U * (kyy * wt(eyy, sy)).sum(1) / sy ** 2
    g = grad_scale(gscale, gmmd)
    base = g * (-2.0 / h2)
    c_xx, c_yy, c_xy = base * 2 / sx ** 2, base * 2 / sy ** 2, base * (-2) / (sx * sy)
    gx_s, ax_s, wx_s = contract(x, x, c_xx * kxx, wt(exx, n))
    gx_o, ax_o, wx_o = contract(x, y, c_xy * kxy, wt(exy, n))
    gy_s, ay_s, wy_s = contract(y, y, c_yy * kyy, wt(eyy, n))
    gy_o, ay_o, wy_o = contract(y, x, c_xy * kxy.t(), wt(exy.t(), n))
    partials = torch.cat([px, py])
    return dict(partials=partials, partials_bound=torch.cat([bx, by]), mmd=partials.sum(), gx=gx_s + gx_o,
                gx_bound=U * (wx_s + wx_o), gy=gy_s + gy_o, gy_bound=U * (wy_s + wy_o), gx_abs=ax_s + ax_o, gy_abs=ay_s + ay_o,
                exponents=(exx, eyy, exy))


@functools.lru_cache(maxsize=None)
def case_references(sx, sy, h, scale):
    """``references`` of ``make_case(sx, sy, h, scale)`` at the scale's GRAD_ARGS.  Cached and shared: nobody changes them."""
    return references(*make_case(sx, sy, h, scale), *GRAD_ARGS[scale])


def value_reference(stored_partials):
    """(float64 sum of the fp32 partials the kernel stored, its bound): what the output scalar is held to."""
    p = stored_partials.detach().double().cpu().reshape(-1)
    ref = p.sum()
    return ref, p.numel() * U * p.abs().sum() + U * ref.abs()


def value_bound_from_reference(ref):
    """For a value whose partials cannot be read back (inside the loss head): the partials' own bounds, the sum of sx + sy
    numbers that are within those bounds of the float64 partials, and the result's rounding."""
    p, b = ref['partials'], ref['partials_bound']
    return b.sum() + p.numel() * U * (p.abs() + b).sum() + U * ref['mmd'].abs()


def indexed_reference(x, y, pick, prefill, gscale=1.0, gmmd=None):
    """y is rows ``pick`` of the taller ``y``; gy is pre-filled.  dict(dense=references on y[pick], gy=(rows of y, h) final values,
    gy_bound, gy_adds=the share of gy_bound that is the m atomic adds' own roundings, picked=(rows,) bool)."""
    dense = references(x, y[pick], gscale, gmmd)
    gy = prefill.double().clone()
    gy.index_add_(0, pick, dense['gy'])
    bound = torch.zeros_like(gy).index_add_(0, pick, dense['gy_bound'])
    mass = prefill.double().abs().index_add_(0, pick, dense['gy'].abs())
    count = torch.bincount(pick, minlength=y.shape[0]).double()
    picked = count > 0
    adds = count[:, None] * U * mass
    return dict(dense=dense, gy=gy, gy_bound=bound + adds, gy_adds=adds, picked=picked)


@functools.lru_cache(maxsize=None)
def index_case_references(sx, h, scale, gscale=0.37, gmmd=1.3):
    x, y, pick, prefill = make_index_case(sx, h, scale)
    return indexed_reference(x, y, pick, prefill, gscale, gmmd)


def restate(x, y, pick=None, prefill=None, gscale=1.0, gmmd=None, wrong=None):
    """k_mmd_fwd* / k_mmd_bwd* in float32 torch: the same expressions per element, torch's summation order.  Returns
    dict(partials, mmd, gx, gy); with ``pick`` gy has y's rows and starts from ``prefill``.  ``wrong``: one of WRONG."""
    f32 = torch.float32
    assert x.dtype == f32 and y.dtype == f32
    t = functools.partial(torch.tensor, dtype=f32)
    idx = pick
    if pick is not None and wrong == 'index_off_by_one':
        idx = (pick + 1) % y.shape[0]
    ys = y if pick is None else y[idx]
    (sx, h), sy = x.shape, ys.shape[0]
    inv = t(1.0) / (t(float(h)) * t(float(h)))

    def kern(a, b):
        d2 = sqdist(a, b)
        return torch.ones_like(d2) if wrong == 'k_is_one' else torch.exp(-d2 * inv)

    def keep(k, is_same):
        if (wrong == 'drop_last_same' and is_same) or (wrong == 'drop_last_other' and not is_same):
            k = k.clone()
            k[:, -1] = 0
        return k
    kxx, kyy, kxy = kern(x, x), kern(ys, ys), kern(x, ys)
    nxx, nyy, nxy = t(float(sx)) * t(float(sx)), t(float(sy)) * t(float(sy)), t(float(sx)) * t(float(sy))
    w_xx, w_yy = t(1.0) / nxx, t(1.0) / nyy
    w_xy = t(-2.0) / (nxx if wrong == 'cross_weight' else nxy)
    px = (w_xx * keep(kxx, True)).sum(1) + (w_xy * keep(kxy, False)).sum(1)
    py = (w_yy * keep(kyy, True)).sum(1)
    partials = torch.cat([px, py])
    g = (t(1.0) if wrong == 'gscale_dropped' else t(gscale)) * (t(1.0) if gmmd is None else t(gmmd))
    base = g * (t(-2.0) * inv)
    c_xx, c_yy = base * t(2.0) / nxx, base * t(2.0) / nyy
    c_xy_x = base * t(-2.0) / (nxx if wrong == 'cross_weight' else nxy)
    c_xy_y = base * t(-2.0) / (nyy if wrong == 'cross_weight' else nxy)
    gx = contract(x, x, c_xx * keep(kxx, True))[0] + contract(x, ys, c_xy_x * keep(kxy, False))[0]
    gyd = contract(ys, ys, c_yy * keep(kyy, True))[0] + contract(ys, x, c_xy_y * keep(kxy.t(), False))[0]
    if pick is None:
        gy = gyd
    else:
        gy = prefill.clone()
        for p, r in enumerate(idx.tolist()):
            gy[r] = (prefill[r] if wrong == 'store_not_add' else gy[r]) + gyd[p]
    assert partials.dtype == gx.dtype == gy.dtype == f32
    return dict(partials=partials, mmd=partials.sum(), gx=gx, gy=gy)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (0 where the error is 0)."""
    got, ref, bound = (torch.as_tensor(v).detach().double().cpu().reshape(-1) for v in (got, ref, bound))
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def worst_ratio_after_adds(got, ref, bound, adds):
    """max (|got - ref| - adds)+ / (bound - adds): what is left of the error once the final adds have been granted their
    roundings in full, against what is left of the bound."""
    got, ref, bound, adds = (torch.as_tensor(v).detach().double().cpu().reshape(-1) for v in (got, ref, bound, adds))
    err = ((got - ref).abs() - adds).clamp_min(0)
    r = torch.where(err == 0, torch.zeros_like(err), err / (bound - adds).clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def share_above(ref, bound):
    """The share of the elements on which an all-zero output would exceed the bound."""
    return float((ref.abs() > bound).double().mean())


# ---- the prior sampler -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampler_case(k, h, repeat):
    """(z_pre (2k, h), eps (s, h), g (s, h), prefill (2k, h)) with PLANT in the first columns of component 0's raw row."""
    gen = torch.Generator().manual_seed(100 * k + h + repeat)
    z_pre = torch.cat([torch.randn(k, h, generator=gen) * 0.5, torch.randn(k, h, generator=gen)])
    n_plant = min(h, len(PLANT))
    z_pre[k, :n_plant] = torch.tensor(PLANT[:n_plant])
    s = k * repeat
    eps, g = torch.randn(s, h, generator=gen), torch.randn(s, h, generator=gen) * 0.3
    prefill = torch.randn(2 * k, h, generator=gen)
    return z_pre, eps, g, prefill


def _factor(raw, sd):
    """0.5 / sd * (raw > 20 ? 1 : sigmoid(raw)): the derivative of sqrt(softplus(raw) + 1e-8) as the kernel applies it."""
    return 0.5 / sd * torch.where(raw > 20, torch.ones_like(raw), torch.sigmoid(raw))


def sampler_reference(z_pre, eps, g=None, prefill=None):
    """Float64: dict(out, out_bound, out_adds, sd, factor[, gz, gz_bound, gz_adds]); ``prefill``: the gradient is accumulated into
    it.  ``*_adds`` is the share of the bound that is the ONE rounding of the last add (u |result|): a statement about a single
    IEEE operation that a correct kernel can use up entirely."""
    z, e = z_pre.double(), eps.double()
    k, h, s = z.shape[0] // 2, z.shape[1], e.shape[0]
    mu, raw = z[:k], z[k:]
    sd = torch.sqrt(torch.nn.functional.softplus(raw) + 1e-8)
    rep = s // k
    spread = e * sd.repeat(rep, 1)
    out = mu.repeat(rep, 1) + spread
    res = dict(out=out, out_bound=U * (out.abs() + 8 * spread.abs()), out_adds=U * out.abs(), sd=sd, factor=_factor(raw, sd))
    if g is not None:
        g = g.double()
        gm, am = g.view(rep, k, h).sum(0), g.abs().view(rep, k, h).sum(0)
        ge = g * e
        gs, as_ = ge.view(rep, k, h).sum(0), ge.abs().view(rep, k, h).sum(0)
        gz = torch.cat([gm, gs * res['factor']])
        bound = torch.cat([rep * U * am, (rep + 12) * U * as_ * res['factor']])
        res['gz_abs'] = torch.cat([am, as_ * res['factor']])
        adds = torch.zeros_like(gz)
        if prefill is not None:
            gz = gz + prefill.double()
            adds = U * gz.abs()
        res.update(gz=gz, gz_bound=bound + adds, gz_adds=adds)
    return res


def sampler_restate(z_pre, eps, g, prefill=None, wrong=None):
    """k_prior_sample_fwd / _bwd in float32 torch: (out, gz).  ``wrong``: one of SAMPLER_WRONG."""
    f32 = torch.float32
    k, h, s = z_pre.shape[0] // 2, z_pre.shape[1], eps.shape[0]
    mu, raw = z_pre[:k], z_pre[k:]
    v = torch.where(raw > 20, raw, torch.log1p(torch.exp(raw))) + torch.tensor(1e-8, dtype=f32)
    sd = torch.sqrt(v)
    r = torch.arange(s)
    comp = torch.clamp(r % (k + 1), max=k - 1) if wrong == 'stride_k_wrong' else r % k
    e_fwd = torch.ones_like(eps) if wrong == 'eps_dropped' else eps
    out = mu[comp] + e_fwd * sd[comp]
    gm, gs = torch.zeros(k, h), torch.zeros(k, h)
    for j in range(k):
        rows = range(j, s, k + 1) if wrong == 'stride_k_wrong' else range(j, s, k)
        for row in rows:
            gm[j] = gm[j] + g[row]
            gs[j] = gs[j] + (g[row] if wrong == 'eps_dropped' else g[row] * eps[row])
    sig = 1.0 / (1.0 + torch.exp(-raw))
    if wrong == 'sigmoid_dropped':
        sig = torch.ones_like(raw)
    elif wrong != 'no_threshold':
        sig = torch.where(raw > 20, torch.ones_like(raw), sig)
    gr = gs * 0.5 / sd * sig
    gz = torch.cat([gm, gr])
    if prefill is not None:
        gz = prefill + gz
    assert out.dtype == gz.dtype == f32
    return out, gz


def composed_bound(samp, mmd_bound, eps):
    """z_pre's gradient through ops.prior_sample -> ops.mmd: the sampler's backward bound at the float64 g (``samp`` =
    sampler_reference(..., g=g64)) plus the MMD gradient's own bound on g pushed through the sampler's sums:
    sum_r bound_r for the mu half, sum_r bound_r |eps_r| * factor for the raw half."""
    k, h = samp['sd'].shape
    rep = eps.shape[0] // k
    b = mmd_bound.double()
    through = torch.cat([b.view(rep, k, h).sum(0), (b * eps.double().abs()).view(rep, k, h).sum(0) * samp['factor']])
    return samp['gz_bound'] + through
