"""gv_mmd_fwd / gv_mmd_bwd and gv_prior_sample_fwd / _bwd (csrc/k_loss.hip) against float64, element by element, inside the
derived bounds of tests/mmd_cases.py (its docstring counts the roundings; tests/test_mmd_host.py proves without a device that
the bounds leave a correct kernel half of their room, reject rules that are wrong in one detail and reject an all-zero
gradient on 99 % of the elements).  u = 2**-24.

    forms     every kernel instantiation at the row counts its loop strides make interesting (mc.FORM_SHAPES), natural and
              wide inputs, through the C ABI into NaN-filled outputs: the per-block partials, the value (against the float64 sum
              of the stored partials), both gradients.  GV_MMD_ROWS16=0 is read once per process: the lane-per-column forms at
              the aligned widths run in one child process (tests/workers/mmd_knob_worker.py).
    unaligned an operand 4 bytes into its allocation sends h = 200 to the lane-per-column forms.
    indexed   y = rows ``pick`` (with repeats) of a 300-row matrix read in place, the gradient ADDED into a pre-filled gy with
              atomics: picked rows inside the bound, every other row bit-identical to the prefill.
    sampler   forward and backward, stored and accumulated, and ops.prior_sample feeding ops.mmd.
    head      the three ways _LossHead reaches gv_mmd_bwd, on inputs whose decoder and regulariser gradients are exactly zero on
              the rows MMD touches.

Every comparison prints RATIO <what> <largest |got - ref| / bound>."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import mmd_cases as mc

gpu = pytest.mark.gpu
U = mc.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = 'GV_MMD_ROWS16'
RATIOS = {}
FORM_CASES = [(sx, sy, h, s) for sx, sy, h in mc.FORM_SHAPES for s in mc.SCALES]
ALIGNED_WIDTH_CASES = [c for c in FORM_CASES if c[2] % 4 == 0 and c[2] <= 512]


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture
def default_forms():
    """The tests that speak of the default dispatch (a row of 16 lanes per partner row wherever it applies)."""
    assert os.environ.get(KNOB) is None, f'{KNOB} is set: this process runs other kernels than these tests name'


def ratio(what, got, ref, bound):
    got = torch.as_tensor(got).detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f'{what}: not finite (something was not written)'
    worst = mc.worst_ratio(got, ref, bound)
    print(f'RATIO {what} {worst:.3f}')
    RATIOS[what] = worst
    assert worst <= 1.0, f'{what}: largest |got - ref| / bound = {worst}'


def nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def placed(t, offset=0):
    """A device copy of ``t`` that starts ``offset`` floats into its (512-byte aligned) allocation."""
    buf = torch.empty(t.numel() + 4, device='cuda')
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view


def launch(ops, x, y, pick, gy0, gscale, gmmd, offsets=(0, 0, 0, 0)):
    """gv_mmd_fwd without an output scalar (the loss head's call: partials only), again with one, then gv_mmd_bwd; everything the
    kernels write starts as NaN, except a pre-filled gy.  Returns CPU tensors (partials, value, gx, gy)."""
    lib, ptr = ops.lib, ops.ptr
    (sx, h), sy = x.shape, (y.shape[0] if pick is None else pick.numel())
    xd, yd = placed(x, offsets[0]), placed(y, offsets[1])
    pd = None if pick is None else pick.cuda()
    ws, ws2, out = nan(sx + sy), nan(sx + sy), nan(1)
    lib.call('gv_mmd_fwd', ptr(xd), ptr(yd), ptr(pd), sx, sy, h, None, ptr(ws), lib.stream())
    lib.call('gv_mmd_fwd', ptr(xd), ptr(yd), ptr(pd), sx, sy, h, ptr(out), ptr(ws2), lib.stream())
    gx = placed(nan(sx, h), offsets[2])
    gy = placed(nan(sy, h) if gy0 is None else gy0, offsets[3])
    g = None if gmmd is None else torch.tensor([gmmd], device='cuda')
    lib.call('gv_mmd_bwd', ptr(xd), ptr(yd), ptr(pd), sx, sy, h, ptr(g), gscale, ptr(gx), ptr(gy), lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(ws.cpu(), ws2.cpu()), 'the partials depend on whether an output scalar is asked for'
    return ws.cpu(), out.cpu(), gx.cpu(), gy.cpu()


def check_forward(tag, partials, value, ref):
    ratio(f'{tag} partials', partials, ref['partials'], ref['partials_bound'])
    vref, vbound = mc.value_reference(partials)
    ratio(f'{tag} value', value, vref, vbound)


def check_dense(ops, tag, sx, sy, h, scale, offsets=(0, 0, 0, 0)):
    x, y = mc.make_case(sx, sy, h, scale)
    ref = mc.case_references(sx, sy, h, scale)
    partials, value, gx, gy = launch(ops, x, y, None, None, *mc.GRAD_ARGS[scale], offsets)
    check_forward(tag, partials, value, ref)
    ratio(f'{tag} gx', gx, ref['gx'], ref['gx_bound'])
    ratio(f'{tag} gy', gy, ref['gy'], ref['gy_bound'])


# ---- every kernel form -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('sx,sy,h,scale', FORM_CASES)
def test_forms_over_shapes(ops, default_forms, sx, sy, h, scale):
    fwd, bwd = mc.dispatch(h)
    check_dense(ops, f'{fwd} {bwd} {sx}x{sy}x{h} {scale}', sx, sy, h, scale)


@gpu
@pytest.mark.parametrize('which,scale', [('x', 'w'), ('y', 'w'), ('x', 'n'), ('y', 'n'), ('gx', 'n'), ('gy', 'w')])
def test_unaligned_base_takes_the_lane_per_column_forms(ops, default_forms, which, scale):
    """h = 200 is an aligned width; x or y (forward and backward) or a gradient (backward) 4 bytes into its allocation fails
    aligned16 and must run k_mmd_fwd<4> / k_mmd_bwd<4>, which load and store single floats."""
    offsets = tuple(int(which == name) for name in ('x', 'y', 'gx', 'gy'))
    assert mc.dispatch(200, aligned=False) == ('k_mmd_fwd<4>', 'k_mmd_bwd<4>')
    check_dense(ops, f'unaligned {which} 65x129x200 {scale}', 65, 129, 200, scale, offsets)


@gpu
def test_static_knob_in_a_child_process(ops, default_forms):
    """GV_MMD_ROWS16=0: the aligned widths on the lane-per-column kernels (h = 260 and 512 are then the only aligned route to
    k_mmd_fwd<16>), in ONE child process started once; a failing child fails the test and nothing is started after it."""
    worker = os.path.join(ROOT, 'tests', 'workers', 'mmd_knob_worker.py')
    out = subprocess.run([sys.executable, worker], cwd=ROOT, env=dict(os.environ, **{KNOB: '0'}), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, f'exit {out.returncode}\n{out.stdout[-3000:]}\n{out.stderr[-3000:]}'
    assert f'{len(ALIGNED_WIDTH_CASES) + 1} cases checked' in out.stdout, out.stdout[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith('{')][-1]
    got = json.loads(line)
    assert len(got) >= 4 * len(ALIGNED_WIDTH_CASES)
    for what, r in got.items():
        print(f'RATIO {KNOB}=0 {what} {r:.3f}')
        RATIOS[f'{KNOB}=0 {what}'] = r
        assert r <= 1.0


# ---- the indexed path ----------------------------------------------------------------------------------------------------------
def check_indexed(ops, tag, sx, h, scale, prefilled, gmmd):
    x, y, pick, prefill = mc.make_index_case(sx, h, scale)
    if prefilled:
        ref = mc.index_case_references(sx, h, scale, 0.37, gmmd)
    else:
        prefill = torch.zeros_like(prefill)
        ref = mc.indexed_reference(x, y, pick, prefill, 0.37, gmmd)
    partials, value, gx, gy = launch(ops, x, y, pick, prefill, 0.37, gmmd)
    check_forward(tag, partials, value, ref['dense'])
    ratio(f'{tag} gx', gx, ref['dense']['gx'], ref['dense']['gx_bound'])
    picked = ref['picked']
    assert torch.equal(gy[~picked], prefill[~picked]), f'{tag}: a row that no index names was written'
    ratio(f'{tag} gy picked rows', gy[picked], ref['gy'][picked], ref['gy_bound'][picked])


@gpu
@pytest.mark.parametrize('sx,h,scale,prefilled,gmmd', [
    (40, 200, 'n', True, 1.3), (40, 200, 'w', True, 1.3), (33, 258, 'n', True, 1.3), (33, 258, 'w', True, 1.3),
    (40, 200, 'w', True, None), (40, 200, 'n', False, None), (33, 258, 'n', False, 1.3)])
def test_indexed_rows_read_in_place_and_added_with_atomics(ops, default_forms, sx, h, scale, prefilled, gmmd):
    """y of 300 rows, 70 positions over 38 rows (one named three times, one by the first and the last position), gscale = 0.37,
    a device gmmd = 1.3 or NULL, into a randn prefill and into zeros (the loss head's own case, where the bound is the
    contributions' alone)."""
    fwd, bwd = mc.dispatch(h)
    check_indexed(ops, f'indexed {fwd} {bwd} {sx}x{mc.INDEX_PICKS}x{h} {scale} prefill={prefilled} gmmd={gmmd}', sx, h, scale,
                  prefilled, gmmd)


@gpu
def test_more_blocks_than_partial_slots_are_refused(ops):
    """sx + sy = 1025 > the 1024 partial slots: gv_mmd_fwd raises on its argument check and launches nothing."""
    lib, ptr = ops.lib, ops.ptr
    x, y = torch.zeros(1000, 4, device='cuda'), torch.zeros(25, 4, device='cuda')
    ws, out = nan(1025), nan(1)
    with pytest.raises(RuntimeError, match='gv_mmd_fwd: sx=1000 sy=25 h=4'):
        lib.call('gv_mmd_fwd', ptr(x), ptr(y), None, 1000, 25, 4, ptr(out), ptr(ws), lib.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()) and bool(torch.isnan(out).all())


# ---- the prior sampler -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('k,h,repeat', mc.SAMPLER_SHAPES)
def test_prior_sampler_forward_and_backward(ops, k, h, repeat, accumulate):
    lib, ptr = ops.lib, ops.ptr
    z_pre, eps, g, prefill = mc.sampler_case(k, h, repeat)
    ref = mc.sampler_reference(z_pre, eps, g, prefill if accumulate else None)
    zd, ed, gd = z_pre.cuda(), eps.cuda(), g.cuda()
    s = eps.shape[0]
    out = nan(s, h)
    gz = prefill.cuda() if accumulate else nan(2 * k, h)
    lib.call('gv_prior_sample_fwd', ptr(zd), ptr(ed), ptr(out), s, k, h, lib.stream())
    lib.call('gv_prior_sample_bwd', ptr(zd), ptr(ed), ptr(gd), ptr(gz), 1 if accumulate else 0, s, k, h, lib.stream())
    torch.cuda.synchronize()
    tag = f'sampler k={k} h={h} repeat={repeat} accumulate={accumulate}'
    ratio(f'{tag} out', out, ref['out'], ref['out_bound'])
    ratio(f'{tag} gz', gz, ref['gz'], ref['gz_bound'])


@gpu
@pytest.mark.parametrize('k,h,repeat,sy', [(10, 200, 20, 150), (3, 258, 7, 17)])
def test_prior_sample_feeding_mmd(ops, default_forms, k, h, repeat, sy):
    """ops.prior_sample -> ops.mmd -> backward with an upstream 1.3.  The sampler's output is held to its float64 reference; the
    MMD references are then taken at the fp32 sample the device stored (a bound-checked intermediate), and z_pre's gradient is
    held to the float64 sampler backward of the float64 MMD gradient, inside mc.composed_bound."""
    z_pre, eps, _, _ = mc.sampler_case(k, h, repeat)
    y = torch.randn(sy, h, generator=torch.Generator().manual_seed(sy)) * 0.8
    zg, yg = z_pre.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    xg = ops.prior_sample(zg, eps.cuda())
    mg = ops.mmd(xg, yg)
    (mg * 1.3).backward()
    torch.cuda.synchronize()
    tag = f'composed k={k} h={h} repeat={repeat} sy={sy}'
    fwd = mc.sampler_reference(z_pre, eps)
    ratio(f'{tag} sample', xg, fwd['out'], fwd['out_bound'])
    ref = mc.references(xg.detach().cpu(), y, 1.0, 1.3)
    ratio(f'{tag} value', mg, ref['mmd'], mc.value_bound_from_reference(ref))
    ratio(f'{tag} gy', yg.grad, ref['gy'], ref['gy_bound'])
    samp = mc.sampler_reference(z_pre, eps, ref['gx'])
    ratio(f'{tag} g z_pre', zg.grad, samp['gz'], mc.composed_bound(samp, ref['gx_bound'], eps))


# ---- through the loss head -------------------------------------------------------------------------------------------------------
N_NODES, N_LIVE, N_PRI, N_TRIP, N_REL, K_MIX = 96, 48, 40, 64, 4, 4
MMD_W, UPSTREAM = 0.6, 1.7


@functools.lru_cache(maxsize=None)
def head_problem(h, repeats=True):
    """z of 96 rows; the triplets touch nodes [0, 48) only and ``pick`` (50 positions over 30 rows, or 40 distinct rows) draws
    from [48, 96) only: with reg_w = 0 the decoder's and the regulariser's gradients on the picked rows are exactly zero."""
    gen = torch.Generator().manual_seed(31 * h + repeats)
    trip = torch.stack([torch.randint(0, N_LIVE, (N_TRIP,), generator=gen), torch.randint(0, N_REL, (N_TRIP,), generator=gen),
                        torch.randint(0, N_LIVE, (N_TRIP,), generator=gen)], 1)
    labels = (torch.rand(N_TRIP, generator=gen) > 0.5).float()
    w_rel = torch.randn(N_REL, h, generator=gen) * 0.3
    z = torch.randn(N_NODES, h, generator=gen)
    z_pri = torch.randn(N_PRI, h, generator=gen) * 0.7 + 0.1
    rows = N_LIVE + torch.randperm(N_NODES - N_LIVE, generator=gen)
    if repeats:
        pick = torch.cat([rows[:30], rows[:18], rows[3:5]])
        pick = pick[torch.randperm(pick.numel(), generator=gen)]
    else:
        pick = rows[:40].clone()
    h2 = torch.randn(N_NODES, 2 * h, generator=gen)
    eps = torch.randn(N_NODES, h, generator=gen)
    z_pre = torch.randn(2 * K_MIX, h, generator=gen) * 0.5
    keep = (torch.rand(N_NODES, 2 * h, generator=gen) >= 0.2).to(torch.uint8)
    m, v = torch.randn(N_NODES, h, generator=gen) * 0.5, torch.rand(N_NODES, h, generator=gen) + 0.2
    assert int(trip[:, [0, 2]].max()) < N_LIVE <= int(pick.min())
    return dict(trip=trip, labels=labels, w_rel=w_rel, z=z, z_pri=z_pri, pick=pick.to(torch.int64), h2=h2, eps=eps, z_pre=z_pre,
                keep=keep, m=m, v=v)


def record_calls(monkeypatch, ops):
    names, real = [], ops.lib.call

    def call(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(ops.lib, 'call', call)
    return names


def check_head_rows(tag, p, z_values, got_rows, got_pri, prefill_rows=None):
    """Rows [48, 96) of dL/dz and z_pri's gradient against the indexed reference at gscale = mmd_w, upstream 1.7, on the fp32 z
    the head read; ``prefill_rows``: what those rows hold besides MMD (fp32 bits, all 96 rows), which costs one more rounding."""
    prefill = torch.zeros_like(z_values) if prefill_rows is None else prefill_rows
    ref = mc.indexed_reference(p['z_pri'], z_values, p['pick'], prefill, MMD_W, UPSTREAM)
    picked = ref['picked'].clone()
    assert not bool(picked[:N_LIVE].any())
    idle = ~picked
    idle[:N_LIVE] = False
    if prefill_rows is None:
        assert bool((got_rows[idle] == 0).all()), f'{tag}: an unpicked row of [48, 96) is not exactly zero'
    else:
        assert torch.equal(got_rows[idle], prefill_rows[idle]), f'{tag}: an unpicked row of [48, 96) moved'
    bound = ref['gy_bound'] + (0.0 if prefill_rows is None else U * ref['gy'].abs())
    ratio(f'{tag} dz picked rows', got_rows[picked], ref['gy'][picked], bound[picked])
    ratio(f'{tag} dz_pri', got_pri, ref['dense']['gx'], ref['dense']['gx_bound'])
    return ref


def run_head(ops, p, z, z_mean, z_sigma, z_pre, flp, kl_w, mmd_w):
    dev = {k: p[k].cuda() for k in ('trip', 'labels', 'pick')}
    z_pri = p['z_pri'].cuda().requires_grad_()
    w_rel = p['w_rel'].cuda().requires_grad_()
    tidx = ops.TripletIndex(dev['trip'], N_NODES, N_REL, sync_free=True)
    loss, pred, _, mmd = ops.loss_head(z, z_mean, z_sigma, w_rel, z_pre, flp, z_pri if mmd_w > 0 else None,
                                       dev['pick'] if mmd_w > 0 else None, dev['labels'], tidx, 0.0, kl_w, mmd_w, False)
    (loss * UPSTREAM).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), pred.detach().cpu(), mmd.detach().cpu(), z_pri.grad


@gpu
@pytest.mark.parametrize('h', [8, 200])
def test_head_without_kl_adds_the_rows_into_the_regulariser_buffer(ops, default_forms, monkeypatch, h):
    """(a) kl_w = 0, z a leaf: gv_mmd_bwd runs on side stream 1 behind the regulariser's axpby (reg_w = 0: zeros) and adds into
    gz, which the decoder's gather-aggregate takes as its addend."""
    p = head_problem(h)
    names = record_calls(monkeypatch, ops)
    z = p['z'].cuda().requires_grad_()
    loss, pred, mmd, g_pri = run_head(ops, p, z, None, None, None, None, 0.0, MMD_W)
    monkeypatch.undo()
    assert names.count('gv_mmd_bwd') == 1 and names.count('gv_mmd_fwd') == 1 and 'gv_kl_bwd' not in names
    ref = check_head_rows(f'head (a) h={h}', p, p['z'], z.grad.cpu(), g_pri.cpu())
    ratio(f'head (a) h={h} mmd', mmd, ref['dense']['mmd'], mc.value_bound_from_reference(ref['dense']))
    # loss = pred + 0 * reg + fl(mmd_w * mmd): two roundings, neither term larger than the loss (both are positive)
    ratio(f'head (a) h={h} loss - pred', loss.double() - pred.double(), mc.r32(MMD_W) * mmd.double(), 2 * U * loss.double().abs())


@gpu
@pytest.mark.parametrize('h', [8, 200])
def test_head_on_the_link_route_adds_the_rows_after_the_decoder(ops, default_forms, monkeypatch, h):
    """(b) ops.reparam with an EpilogueLink and kl_w > 0 (training's default route): KL's part of dL/dz travels through the link,
    and what _LossHead.backward returns for z -- the decoder's gradient with the MMD rows added by gv_mmd_bwd on the main stream
    -- is caught by a hook on z."""
    p = head_problem(h)
    names = record_calls(monkeypatch, ops)
    h2, z_pre = p['h2'].cuda().requires_grad_(), p['z_pre'].cuda().requires_grad_()
    epi = ops.EpilogueLink(p['keep'].cuda(), 1.25, True, None, 2 * h)
    z, m, v = ops.reparam(h2, p['eps'].cuda(), z_pre, epi)
    seen = []
    z.register_hook(lambda g: seen.append(g.detach().clone()))
    _, _, mmd, g_pri = run_head(ops, p, z, m, v, z_pre, None, 1e-2, MMD_W)
    monkeypatch.undo()
    assert len(seen) == 1, 'the hook on z did not fire exactly once'
    assert names.count('gv_mmd_bwd') == 1
    assert 'gv_kl_fwd' not in names and 'gv_kl_bwd' not in names, 'the loss head did not take the hand-off'
    assert any(n in names for n in ('gv_reparam_kl_bwd_fold', 'gv_reparam_kl_bwd'))
    assert bool(torch.isfinite(h2.grad).all()) and bool(torch.isfinite(z_pre.grad).all())
    z_values = z.detach().cpu()
    ref = check_head_rows(f'head (b) h={h}', p, z_values, seen[0].cpu(), g_pri.cpu())
    ratio(f'head (b) h={h} mmd', mmd, ref['dense']['mmd'], mc.value_bound_from_reference(ref['dense']))


@gpu
@pytest.mark.parametrize('h', [8, 200])
def test_head_with_its_own_kl_adds_the_rows_behind_the_kl_sweep(ops, default_forms, monkeypatch, h):
    """(c) kl_w > 0 without the link (a flow log-probability is given): gv_kl_bwd writes gz on side stream 1 and gv_mmd_bwd adds
    into it behind it.  The KL part of rows [48, 96) is taken, as fp32 bits, from the same step at mmd_w = 0."""
    p = head_problem(h)
    flp = torch.tensor(-0.4, device='cuda')
    runs = {}
    for mmd_w in (0.0, MMD_W):
        names = record_calls(monkeypatch, ops)
        z, m, v = (p[k].cuda().requires_grad_() for k in ('z', 'm', 'v'))
        z_pre = p['z_pre'].cuda().requires_grad_()
        _, _, mmd, g_pri = run_head(ops, p, z, m, v, z_pre, flp, 1e-2, mmd_w)
        monkeypatch.undo()
        assert names.count('gv_kl_bwd') == 1 and names.count('gv_mmd_bwd') == (1 if mmd_w > 0 else 0)
        runs[mmd_w] = (z.grad.cpu(), g_pri, mmd)
    kl_rows, with_mmd = runs[0.0][0], runs[MMD_W]
    assert bool(torch.isfinite(kl_rows).all()) and float(kl_rows[N_LIVE:].abs().max()) > 0
    ref = check_head_rows(f'head (c) h={h}', p, p['z'], with_mmd[0], with_mmd[1].cpu(), prefill_rows=kl_rows)
    ratio(f'head (c) h={h} mmd', with_mmd[2], ref['dense']['mmd'], mc.value_bound_from_reference(ref['dense']))


@gpu
def test_head_without_kl_captured_and_replayed(ops, default_forms):
    """Route (a) at h = 200 captured in a graph on a side stream and replayed twice gives the eager bits.  The indexed rows are
    float atomics: with a repeated index the order in which two contributions land on one address is not fixed, and float
    addition does not commute with a third term in between -- so this ONE bit-equality check uses a pick WITHOUT repeats (every
    address gets a single add onto a zero), and the repeats are held to the bound by the tests above."""
    h = 200
    p = head_problem(h, repeats=False)
    assert p['pick'].unique().numel() == p['pick'].numel()
    dev = {k: p[k].cuda() for k in ('trip', 'labels', 'pick')}
    params = [p[k].cuda().requires_grad_() for k in ('z', 'z_pri', 'w_rel')]
    z, z_pri, w_rel = params
    for t in params:
        t.grad = torch.zeros_like(t)
    tidx = ops.TripletIndex(dev['trip'], N_NODES, N_REL, sync_free=True)

    def step():
        for t in params:
            t.grad.zero_()
        loss, _, _, _ = ops.loss_head(z, None, None, w_rel, None, None, z_pri, dev['pick'], dev['labels'], tidx, 0.0, 0.0, MMD_W, False)
        (loss * UPSTREAM).backward()
        return loss

    def snapshot(loss):
        torch.cuda.synchronize()
        return [loss.detach().clone().cpu()] + [t.grad.clone().cpu() for t in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = snapshot(step())
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    runs = []
    for _ in range(2):
        graph.replay()
        runs.append(snapshot(out))
    for a, b, c in zip(eager, runs[0], runs[1]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(b, c)
    check_head_rows('head (a) h=200 captured', p, p['z'], runs[1][1], runs[1][2])
