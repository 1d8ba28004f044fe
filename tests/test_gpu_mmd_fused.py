"""The one-sweep MMD (csrc/k_loss.hip: gv_mmd_fwd_grad, the same row workgroups inside gv_distmult_bce_fwd_grad_mmd, and the
backward's gv_mmd_grad_finish) against the float64 references and the element-wise bounds of tests/mmd_cases.py (u = 2**-24).

The sweep computes a gradient row at upstream 1 and the finishing launch scales it: per term the coefficient is (-2 inv) 2 / n n
(inv 1, the division 1), expf (4), cf * expf (1), a - b (1), and behind the sum gg (1) and gg * row (1): ten roundings, what
k_mmd_bwd_g spends (mmd_cases counts 12), and a sum of N terms in another fixed order.  The bounds hold unchanged.

    sweep     every aligned width of mc.FORM_SHAPES (h <= 256: four float4 columns a lane; 260 and 512: eight) and (200, 200, 200),
              natural and wide inputs, into NaN-filled outputs: partials, the value (gv_loss_combine over the stored partials),
              gx (= g_pri), gy, z_pre's gradient stored and accumulated, gmmd a device scalar or NULL, gscale 1 and 0.37 -- and
              each against the separate launches (gv_mmd_fwd, gv_mmd_bwd, gv_prior_sample_bwd) within the sum of both bounds.
    indexed   y = rows ``pick`` (with repeats) of a 300-row matrix, the rows ADDED into a pre-filled gy: picked rows inside the
              bound, every other row bit-identical.
    combined  the DistMult outputs of gv_distmult_bce_fwd_grad_mmd are torch.equal to gv_distmult_bce_fwd_grad's at the shapes of
              tests/test_gpu_distmult_rows.py, with an MMD problem of (7, 130, 16) riding along (held to its own bounds).
    head      ops.loss_head on the hand-off route and with its own KL pass, h = 8 and 200, 300 nodes: against GV_MMD_FUSED=0
              within the summed bounds (plus the roundings of the adds that land the MMD part in a larger KL or decoder
              value: stated where they are added); both routes and the kl_w = 0 one captured and replayed; the sampler's backward
              silent for a claimed link and raising for a foreign gradient.

Every comparison prints RATIO <what> <largest |got - ref| / bound>."""
import functools

import pytest
import torch

import mmd_cases as mc
import test_gpu_distmult_rows as dr

gpu = pytest.mark.gpu
U = mc.U
SWEEP_SHAPES = tuple(s for s in mc.FORM_SHAPES if s[2] % 4 == 0 and s[2] <= 512) + ((200, 200, 200),)
SWEEP_CASES = [(sx, sy, h, s) for sx, sy, h in SWEEP_SHAPES for s in mc.SCALES]


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def ratio(what, got, ref, bound):
    got = torch.as_tensor(got).detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f'{what}: not finite (something was not written)'
    worst = mc.worst_ratio(got, ref, bound)
    print(f'RATIO {what} {worst:.3f}')
    assert worst <= 1.0, f'{what}: largest |got - ref| / bound = {worst}'


def nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def components(sx):
    """A mixture size whose repeats make exactly sx prior rows (the finishing launch needs whole repeats)."""
    return next(k for k in (10, 9, 5, 3, 1) if sx % k == 0)


def value_of(ops, part, sx, sy):
    """The MMD value as the loss head gets it: gv_loss_combine's sum of the stored partials (scal[3])."""
    lib, ptr = ops.lib, ops.ptr
    ws, scal, loss = torch.zeros(2048, device='cuda'), nan(4), nan(1)
    lib.call('gv_loss_combine', ptr(ws), 1, None, 0, 0, None, 0, 4, 0, ptr(part), sx, sy, 0.0, 0.0, 1.0, ptr(scal), ptr(loss), None,
             lib.stream())
    return scal[3:4]


def launch_new(ops, x, y, pick, gy0, gscale, gmmd, z_pre, eps, gz0):
    """gv_mmd_fwd_grad + gv_mmd_grad_finish; everything they write starts as NaN, except a pre-filled gy / gz_pre.  CPU tensors."""
    lib, ptr = ops.lib, ops.ptr
    (sx, h), sy = x.shape, (y.shape[0] if pick is None else pick.numel())
    xd, yd, pd = x.cuda(), y.cuda(), (None if pick is None else pick.cuda())
    zd, ed = z_pre.cuda(), eps.cuda()
    part, gx_u, gy_u = nan(sx + sy), nan(sx, h), nan(sy, h)
    lib.call('gv_mmd_fwd_grad', ptr(xd), ptr(yd), ptr(pd), sx, sy, h, ptr(part), ptr(gx_u), ptr(gy_u), lib.stream())
    value = value_of(ops, part, sx, sy)
    gy = nan(sy, h) if gy0 is None else gy0.cuda()
    gz = nan(*z_pre.shape) if gz0 is None else gz0.cuda()
    g_pri = nan(sx, h)
    g = None if gmmd is None else torch.tensor([gmmd], device='cuda')
    lib.call('gv_mmd_grad_finish', ptr(gx_u), ptr(gy_u), ptr(pd), sx, sy, h, ptr(g), gscale, ptr(gy), ptr(g_pri), ptr(zd), ptr(ed),
             ptr(gz), 0 if gz0 is None else 1, z_pre.shape[0] // 2, lib.stream())
    torch.cuda.synchronize()
    return dict(partials=part.cpu(), value=value.cpu(), gx=g_pri.cpu(), gy=gy.cpu(), gz=gz.cpu())


def launch_old(ops, x, y, pick, gy0, gscale, gmmd, z_pre, eps, gz0):
    """The separate launches on the same inputs: gv_mmd_fwd, gv_mmd_bwd, gv_prior_sample_bwd."""
    lib, ptr = ops.lib, ops.ptr
    (sx, h), sy = x.shape, (y.shape[0] if pick is None else pick.numel())
    xd, yd, pd = x.cuda(), y.cuda(), (None if pick is None else pick.cuda())
    zd, ed = z_pre.cuda(), eps.cuda()
    part, out, gx = nan(sx + sy), nan(1), nan(sx, h)
    lib.call('gv_mmd_fwd', ptr(xd), ptr(yd), ptr(pd), sx, sy, h, ptr(out), ptr(part), lib.stream())
    gy = nan(sy, h) if gy0 is None else gy0.cuda()
    gz = nan(*z_pre.shape) if gz0 is None else gz0.cuda()
    g = None if gmmd is None else torch.tensor([gmmd], device='cuda')
    lib.call('gv_mmd_bwd', ptr(xd), ptr(yd), ptr(pd), sx, sy, h, ptr(g), gscale, ptr(gx), ptr(gy), lib.stream())
    lib.call('gv_prior_sample_bwd', ptr(zd), ptr(ed), ptr(gx), ptr(gz), 0 if gz0 is None else 1, sx,
             z_pre.shape[0] // 2, h, lib.stream())
    torch.cuda.synchronize()
    return dict(partials=part.cpu(), value=out.cpu(), gx=gx.cpu(), gy=gy.cpu(), gz=gz.cpu())


def check_against_float64(tag, got, ref, samp, gz_bound, gy_ref=None, gy_bound=None):
    ratio(f'{tag} partials', got['partials'], ref['partials'], ref['partials_bound'])
    vref, vbound = mc.value_reference(got['partials'])
    ratio(f'{tag} value', got['value'], vref, vbound)
    ratio(f'{tag} gx', got['gx'], ref['gx'], ref['gx_bound'])
    if gy_ref is None:
        ratio(f'{tag} gy', got['gy'], ref['gy'], ref['gy_bound'])
    else:
        ratio(f'{tag} gy picked rows', got['gy'], gy_ref, gy_bound)
    ratio(f'{tag} g z_pre', got['gz'], samp['gz'], gz_bound)


# ---- the sweep and the finishing launch ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('sx,sy,h,scale', SWEEP_CASES)
def test_sweep_and_finish_over_shapes(ops, sx, sy, h, scale):
    """Dense y.  Scale 'n' runs gscale = 1 with gmmd == NULL and a stored z_pre gradient; scale 'w' gscale = 0.37 with a device
    gmmd = 1.3 and a z_pre gradient accumulated into a prefill."""
    x, y = mc.make_case(sx, sy, h, scale)
    ref = mc.case_references(sx, sy, h, scale)
    gscale, gmmd = mc.GRAD_ARGS[scale]
    k = components(sx)
    z_pre, eps, _, prefill = mc.sampler_case(k, h, sx // k)
    gz0 = prefill if scale == 'w' else None
    samp = mc.sampler_reference(z_pre, eps, ref['gx'], gz0)
    gz_bound = mc.composed_bound(samp, ref['gx_bound'], eps)
    new = launch_new(ops, x, y, None, None, gscale, gmmd, z_pre, eps, gz0)
    tag = f'sweep {sx}x{sy}x{h} {scale}'
    check_against_float64(tag, new, ref, samp, gz_bound)
    old = launch_old(ops, x, y, None, None, gscale, gmmd, z_pre, eps, gz0)
    vb = mc.value_bound_from_reference(ref)
    for what, bound in (('partials', ref['partials_bound']), ('value', vb), ('gx', ref['gx_bound']), ('gy', ref['gy_bound']),
                        ('gz', gz_bound)):
        ratio(f'{tag} {what} against the separate launches', new[what], old[what].double(), 2 * bound)


@gpu
@pytest.mark.parametrize('scale,prefilled,gmmd', [('n', True, 1.3), ('w', True, 1.3), ('w', True, None), ('n', False, None)])
def test_indexed_rows_added_into_a_prefilled_gradient(ops, scale, prefilled, gmmd):
    """y of 300 rows, 70 positions over 38 rows (one named three times), gscale = 0.37, into a randn prefill and into zeros:
    picked rows inside the bound, every other row bit-identical to the prefill."""
    sx, h = 40, 200
    x, y, pick, prefill = mc.make_index_case(sx, h, scale)
    if not prefilled:
        prefill = torch.zeros_like(prefill)
    ref = mc.indexed_reference(x, y, pick, prefill, 0.37, gmmd)
    k = components(sx)
    z_pre, eps, _, _ = mc.sampler_case(k, h, sx // k)
    samp = mc.sampler_reference(z_pre, eps, ref['dense']['gx'])
    gz_bound = mc.composed_bound(samp, ref['dense']['gx_bound'], eps)
    new = launch_new(ops, x, y, pick, prefill, 0.37, gmmd, z_pre, eps, None)
    picked = ref['picked']
    tag = f'indexed {sx}x{mc.INDEX_PICKS}x{h} {scale} prefill={prefilled} gmmd={gmmd}'
    assert torch.equal(new['gy'][~picked], prefill[~picked]), f'{tag}: a row that no index names was written'
    rows = dict(new, gy=new['gy'][picked])
    check_against_float64(tag, rows, ref['dense'], samp, gz_bound, ref['gy'][picked], ref['gy_bound'][picked])
    old = launch_old(ops, x, y, pick, prefill, 0.37, gmmd, z_pre, eps, None)
    assert torch.equal(old['gy'][~picked], new['gy'][~picked])
    ratio(f'{tag} gy against the separate launches', new['gy'][picked], old['gy'][picked].double(), 2 * ref['gy_bound'][picked])
    ratio(f'{tag} gx against the separate launches', new['gx'], old['gx'].double(), 2 * ref['dense']['gx_bound'])


@gpu
def test_shapes_outside_the_rule_are_refused(ops):
    """h % 4 != 0, h > 512 (> 256 inside the DistMult launch is refused by the same rule) and sx + sy > 1024 launch nothing."""
    lib, ptr = ops.lib, ops.ptr
    for sx, sy, h in ((4, 4, 6), (4, 4, 516), (1000, 25, 4)):
        x, y = torch.zeros(sx, h, device='cuda'), torch.zeros(sy, h, device='cuda')
        part, gx_u, gy_u = nan(sx + sy), nan(sx, h), nan(sy, h)
        with pytest.raises(RuntimeError, match='gv_mmd_fwd_grad: sx='):
            lib.call('gv_mmd_fwd_grad', ptr(x), ptr(y), None, sx, sy, h, ptr(part), ptr(gx_u), ptr(gy_u), lib.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(part).all()) and bool(torch.isnan(gx_u).all()) and bool(torch.isnan(gy_u).all())


# ---- inside the DistMult forward launch ------------------------------------------------------------------------------------------
MMD_BESIDE = (7, 130, 16)


@gpu
@pytest.mark.parametrize('flavour', dr.FLAVOURS)
@pytest.mark.parametrize('h', dr.WIDTHS)
def test_distmult_outputs_of_the_combined_launch_are_bit_identical(ops, h, flavour):
    lib, ptr = ops.lib, ops.ptr
    e32, w32, trip, y32 = dr.problem(h)
    idx = dr.make_index(ops, trip, flavour)
    seg, T = idx.rel, dr.T
    e, w, labels, bias = e32.cuda(), w32.cuda(), y32.cuda(), torch.tensor(0.3, device='cuda')
    n_coef = 2 * T if idx.pos3 is not None else T
    sx, sy, mh = MMD_BESIDE
    x, y = mc.make_case(sx, sy, mh, 'w')
    xd, yd = x.cuda(), y.cuda()

    def run(combined):
        fill = lambda *shape: torch.full(shape, -7.0, device='cuda')     # noqa: E731  (slots no item owns keep the fill)
        out = dict(score=fill(T), delta=fill(n_coef), u=fill(dr.N_REL, h), partial=fill(max(seg.n_slots, 1), h), ws=fill(2048))
        args = (ptr(seg.items), seg.n_items, ptr(idx.rel_s), ptr(idx.rel_o), ptr(idx.rel_tid), ptr(e), h, ptr(w), h, ptr(labels),
                ptr(bias), ptr(idx.pos3), ptr(out['score']), ptr(out['delta']), ptr(out['u']), ptr(out['partial']), ptr(out['ws']),
                T, h)
        if combined:
            out.update(part=nan(sx + sy), gx_u=nan(sx, mh), gy_u=nan(sy, mh))
            lib.call('gv_distmult_bce_fwd_grad_mmd', *args, ptr(xd), ptr(yd), None, sx, sy, mh, ptr(out['part']), ptr(out['gx_u']),
                     ptr(out['gy_u']), lib.stream())
        else:
            lib.call('gv_distmult_bce_fwd_grad', *args, lib.stream())
        torch.cuda.synchronize()
        return out
    alone, both = run(False), run(True)
    for name in ('score', 'delta', 'u', 'partial', 'ws'):
        assert torch.equal(alone[name], both[name]), f'{name} differs between the two launches (h={h}, {flavour})'
    assert bool((alone['score'] != -7.0).all())
    ref = mc.references(x, y)
    tag = f'combined h={h} {flavour} mmd {sx}x{sy}x{mh}'
    ratio(f'{tag} partials', both['part'], ref['partials'], ref['partials_bound'])
    ratio(f'{tag} gx_u', both['gx_u'], ref['gx'], ref['gx_bound'])
    ratio(f'{tag} gy_u', both['gy_u'], ref['gy'], ref['gy_bound'])


# ---- through the loss head -------------------------------------------------------------------------------------------------------
N_NODES, N_LIVE, N_TRIP, N_REL, K_MIX, REPEAT, N_PICK = 300, 150, 256, 4, 4, 10, 50
MMD_W, UPSTREAM, REG_W, KL_W = 0.6, 1.7, 0.01, 1e-2


@functools.lru_cache(maxsize=None)
def head_problem(h, repeats=True):
    """300 nodes; the triplets touch nodes [0, 150) only, ``pick`` (50 positions over 30 rows, or 50 distinct rows) draws from
    [150, 300); the prior rows are ops.prior_sample's of a 4-component mixture, 10 repeats."""
    gen = torch.Generator().manual_seed(57 * h + repeats)
    trip = torch.stack([torch.randint(0, N_LIVE, (N_TRIP,), generator=gen), torch.randint(0, N_REL, (N_TRIP,), generator=gen),
                        torch.randint(0, N_LIVE, (N_TRIP,), generator=gen)], 1)
    rows = N_LIVE + torch.randperm(N_NODES - N_LIVE, generator=gen)
    if repeats:
        pick = torch.cat([rows[:30], rows[:18], rows[3:5]])
        pick = pick[torch.randperm(pick.numel(), generator=gen)]
    else:
        pick = rows[:N_PICK].clone()
    return dict(trip=trip, labels=(torch.rand(N_TRIP, generator=gen) > 0.5).float(), w_rel=torch.randn(N_REL, h, generator=gen) * 0.3,
                z=torch.randn(N_NODES, h, generator=gen), pick=pick.to(torch.int64), h2=torch.randn(N_NODES, 2 * h, generator=gen),
                eps=torch.randn(N_NODES, h, generator=gen), z_pre=torch.randn(2 * K_MIX, h, generator=gen) * 0.5,
                eps_pri=torch.randn(K_MIX * REPEAT, h, generator=gen),
                keep=(torch.rand(N_NODES, 2 * h, generator=gen) >= 0.2).to(torch.uint8),
                m=torch.randn(N_NODES, h, generator=gen) * 0.5, v=torch.rand(N_NODES, h, generator=gen) + 0.2)


def record_calls(monkeypatch, ops):
    names, real = [], ops.lib.call

    def call(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(ops.lib, 'call', call)
    return names


def run_head(ops, p, route, extra_consumer=False):
    """One forward + backward of ops.loss_head with z_pri = ops.prior_sample(z_pre, eps_pri).  ``route``: 'link' = ops.reparam with
    an EpilogueLink and kl_w > 0 (training's default); 'own' = kl_w > 0 with a flow log-probability (the head's own KL passes,
    the MMD rows added on the side stream).  Returns CPU tensors."""
    dev = {k: p[k].cuda() for k in ('trip', 'labels', 'pick', 'eps', 'eps_pri')}
    z_pre = p['z_pre'].cuda().requires_grad_()
    w_rel = p['w_rel'].cuda().requires_grad_()
    tidx = ops.TripletIndex(dev['trip'], N_NODES, N_REL, sync_free=True)
    seen, seen_z, leaves = [], [], {}
    if route == 'link':
        h2 = p['h2'].cuda().requires_grad_()
        epi = ops.EpilogueLink(p['keep'].cuda(), 1.25, True, None, 2 * p['z'].shape[1])
        z, m, v = ops.reparam(h2, dev['eps'], z_pre, epi)
        z.register_hook(lambda g: seen_z.append(g.detach().clone()))
        flp = None
        leaves['h2'] = h2
    else:
        z, m, v = (p[k].cuda().requires_grad_() for k in ('z', 'm', 'v'))
        flp = torch.tensor(-0.4, device='cuda')
        leaves.update(z=z, m=m, v=v)
    z_pri = ops.prior_sample(z_pre, dev['eps_pri'])
    z_pri.register_hook(lambda g: seen.append(g.detach().clone()))
    loss, pred, kl, mmd = ops.loss_head(z, m, v, w_rel, z_pre, flp, z_pri, dev['pick'], dev['labels'], tidx, REG_W, KL_W, MMD_W, False)
    total = loss * UPSTREAM
    if extra_consumer:
        total = total + z_pri.sum()
    total.backward()
    torch.cuda.synchronize()
    out = dict(loss=loss, mmd=mmd, z_pre=z_pre.grad, w_rel=w_rel.grad, z_values=z, z_pri=z_pri,
               g_pri=seen[0], **{f'g_{k}': t.grad for k, t in leaves.items()})
    assert len(seen) == 1, 'the hook on z_pri did not fire exactly once'
    if route == 'link':
        assert len(seen_z) == 1, 'the hook on z did not fire exactly once'
        out['g_z'] = seen_z[0]
    return {k: v.detach().cpu() for k, v in out.items()}


@gpu
@pytest.mark.parametrize('route', ['link', 'own'])
@pytest.mark.parametrize('h', [8, 200])
def test_head_against_the_switch_off_route(ops, monkeypatch, h, route):
    """Both routes on the same inputs.  Everything but the MMD term is the same launches on the same bits, so: w_rel's gradient and
    every row of dL/dz that no pick names are bit-identical; picked rows, z_pri's gradient, the value and the loss differ by at
    most the two routes' MMD bounds (plus the roundings of the adds that land them: (count + 1) u |value| per route); z_pre's
    gradient by the sampler's composed bounds (plus 2 u |value| for the adds into KL's part); dL/dh2 (hand-off route: mean half
    = dL/dz, raw half = dL/dz eps 0.5 / sd sigmoid(raw), both plus KL's part) by the picked rows' bound carried through those
    two factors, 4 u |value| on top."""
    p = head_problem(h)
    names = record_calls(monkeypatch, ops)
    new = run_head(ops, p, route)
    new_names = list(names)
    del names[:]
    monkeypatch.setattr(ops, 'MMD_FUSED', False)
    old = run_head(ops, p, route)
    old_names = list(names)
    monkeypatch.undo()
    # the launches: the sampler's backward and both MMD launches are gone on the new route
    assert new_names.count('gv_distmult_bce_fwd_grad_mmd') == 1 and new_names.count('gv_mmd_grad_finish') == 1
    assert not {'gv_mmd_fwd', 'gv_mmd_bwd', 'gv_prior_sample_bwd', 'gv_distmult_bce_fwd_grad'} & set(new_names)
    assert old_names.count('gv_mmd_fwd') == 1 and old_names.count('gv_mmd_bwd') == 1 and old_names.count('gv_prior_sample_bwd') == 1
    assert not {'gv_distmult_bce_fwd_grad_mmd', 'gv_mmd_grad_finish'} & set(old_names)
    assert len(new_names) == len(old_names) - 2
    assert torch.equal(new['z_values'], old['z_values']) and torch.equal(new['z_pri'], old['z_pri'])
    tag = f'head {route} h={h}'
    zero = torch.zeros(N_NODES, h)
    ref = mc.indexed_reference(new['z_pri'], new['z_values'], p['pick'], zero, MMD_W, UPSTREAM)
    dense, picked = ref['dense'], ref['picked']
    count = torch.bincount(p['pick'], minlength=N_NODES).double()[:, None]
    assert torch.equal(new['w_rel'], old['w_rel'])
    vb = mc.value_bound_from_reference(dense)
    ratio(f'{tag} mmd', new['mmd'], old['mmd'].double(), 2 * vb)
    ratio(f'{tag} mmd against float64', new['mmd'], dense['mmd'], vb)
    ratio(f'{tag} loss', new['loss'], old['loss'].double(), 2 * mc.r32(MMD_W) * vb + 4 * U * old['loss'].double().abs())
    ratio(f'{tag} dz_pri', new['g_pri'], old['g_pri'].double(), 2 * dense['gx_bound'])
    ratio(f'{tag} dz_pri against float64', new['g_pri'], dense['gx'], dense['gx_bound'])
    g_new, g_old = new['g_z'], old['g_z']      # (hand-off route: what the head returns for z, caught by a hook; else z.grad)
    assert torch.equal(g_new[~picked], g_old[~picked]), f'{tag}: a row of dL/dz that no pick names differs'
    row_bound = 2 * ref['gy_bound'] + 2 * (count + 1) * U * g_old.double().abs()
    ratio(f'{tag} dz picked rows', g_new[picked], g_old[picked].double(), row_bound[picked])
    eps_pri = p['eps_pri']
    samp = mc.sampler_reference(p['z_pre'], eps_pri, dense['gx'])
    zb = 2 * mc.composed_bound(samp, dense['gx_bound'], eps_pri) + 4 * U * old['z_pre'].double().abs()
    ratio(f'{tag} dz_pre', new['z_pre'], old['z_pre'].double(), zb)
    if route == 'link':
        raw = p['h2'][:, h:].double()
        sd = torch.sqrt(torch.nn.functional.softplus(raw) + 1e-8)
        factor = p['eps'].double().abs() * 0.5 / sd * torch.sigmoid(raw)
        hb = torch.cat([row_bound, row_bound * factor], 1) * 1.25 + 4 * U * old['g_h2'].double().abs()      # (keep scale 1.25)
        assert torch.equal(new['g_h2'][~picked], old['g_h2'][~picked])
        ratio(f'{tag} dh2 picked rows', new['g_h2'][picked], old['g_h2'][picked].double(), hb[picked])
    else:
        assert torch.equal(new['g_m'], old['g_m']) and torch.equal(new['g_v'], old['g_v'])


@gpu
@pytest.mark.parametrize('route', ['link', 'own', 'nokl'])
@pytest.mark.parametrize('h', [8, 200])
def test_head_captured_and_replayed(ops, h, route):
    """One step -- ops.prior_sample, the route's own way to z, ops.loss_head, backward -- captured in a graph on a side stream and
    replayed twice: the loss and every gradient carry the eager bits.
        link   ops.reparam with an EpilogueLink, kl_w > 0: gv_mmd_grad_finish on the main stream behind bdd_aggregate (training's route)
        own    kl_w > 0 with a flow log-probability: on side stream 1 behind gv_kl_bwd, z_pre's gradient next to KL's
        nokl   kl_w = 0: on side stream 1 behind the regulariser's gv_axpby
    The pick has no repeats (two float atomics on one address have no fixed order; the repeats are held to the bound above)."""
    p = head_problem(h, repeats=False)
    assert p['pick'].unique().numel() == p['pick'].numel()
    dev = {k: p[k].cuda() for k in ('trip', 'labels', 'pick', 'eps', 'eps_pri', 'keep')}
    names = {'link': ('h2', 'z_pre', 'w_rel'), 'own': ('z', 'm', 'v', 'z_pre', 'w_rel'), 'nokl': ('z', 'z_pre', 'w_rel')}[route]
    leaf = {k: p[k].cuda().requires_grad_() for k in names}
    params = list(leaf.values())
    for t in params:
        t.grad = torch.zeros_like(t)
    flp = torch.tensor(-0.4, device='cuda') if route == 'own' else None
    tidx = ops.TripletIndex(dev['trip'], N_NODES, N_REL, sync_free=True)
    links, calls = [], []
    real = ops.lib.call

    def call(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    def step():
        for t in params:
            t.grad.zero_()
        z_pre, w_rel = leaf['z_pre'], leaf['w_rel']
        z_pri = ops.prior_sample(z_pre, dev['eps_pri'])
        links.append(z_pri._gv_prior_link)
        if route == 'link':
            epi = ops.EpilogueLink(dev['keep'], 1.25, True, None, 2 * h)
            z, m, v = ops.reparam(leaf['h2'], dev['eps'], z_pre, epi)
            head = (z, m, v, w_rel, z_pre, None)
        elif route == 'own':
            head = (leaf['z'], leaf['m'], leaf['v'], w_rel, z_pre, flp)
        else:
            head = (leaf['z'], None, None, w_rel, None, None)
        loss, _, _, _ = ops.loss_head(*head, z_pri, dev['pick'], dev['labels'], tidx, REG_W, 0.0 if route == 'nokl' else KL_W, MMD_W,
                                      False)
        (loss * UPSTREAM).backward()
        return loss

    def snapshot(loss):
        torch.cuda.synchronize()
        return [loss.detach().clone().cpu()] + [t.grad.clone().cpu() for t in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ops.lib.call = call
    try:
        with torch.cuda.stream(side):
            eager = snapshot(step())
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        del calls[:]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = step()
    finally:
        ops.lib.call = real
    assert all(link is not None and link.claimed for link in links)
    # what was captured is the new route, on the route's own KL launches
    assert calls.count('gv_distmult_bce_fwd_grad_mmd') == 1 and calls.count('gv_mmd_grad_finish') == 1
    assert not {'gv_mmd_fwd', 'gv_mmd_bwd', 'gv_prior_sample_bwd'} & set(calls)
    assert ('gv_kl_bwd' in calls) == (route == 'own') and ('gv_reparam_kl_fwd' in calls) == (route == 'link')
    if route == 'link':
        assert 'gv_kl_fwd' not in calls and any(n in calls for n in ('gv_reparam_kl_bwd_fold', 'gv_reparam_kl_bwd'))
    runs = []
    for _ in range(2):
        graph.replay()
        runs.append(snapshot(out))
    for name, a, b, c in zip(('loss',) + names, eager, runs[0], runs[1]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b) and torch.equal(b, c), f'{name}: a replay differs from the eager run ({route}, h={h})'
    for name, g in zip(names, runs[1][1:]):
        assert float(g.abs().max()) > 0, f'{name} received no gradient'


@gpu
def test_sampler_backward_raises_on_a_foreign_gradient(ops, monkeypatch):
    """z_pri has a second consumer: the gradient arriving at the sampler is autograd's sum, not the buffer the loss head recorded,
    and z_pre's share of the extra term would be lost -- the sampler's backward raises instead of returning the folded result."""
    p = head_problem(8)
    with pytest.raises(RuntimeError, match='ops.PriorLink'):
        run_head(ops, p, 'own', extra_consumer=True)
    torch.cuda.synchronize()
