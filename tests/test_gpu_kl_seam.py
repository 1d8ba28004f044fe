"""The seam between the encoder's second layer and the loss head on the reparameterisation/KL hand-off route
(csrc/k_loss.hip: gv_reparam_kl_fwd's sum z^2 partials + gv_loss_combine_fold; gv_reparam_kl_bwd_fold = the KL backward sweep that
also masks dL/dh2 with layer 2's keep mask and sums its bias gradient) against the three launches it replaces (GV_KL_SEAM_FOLD=0:
gv_mean_sq2, gv_rgcn_epilogue_bwd, gv_colsum_finish).

What is compared with what (u = 2**-24):

    rows      the masked dL/dh2 rows are keep ? value * scale : 0 of the SAME fp32 value on both routes: bit-identical.
    g_zpre    the mixture gradient's slice partials are the same values added in the same order: bit-identical.
    bias      column sums of those rows.  Reference: the float64 sum of the (bit-checked) fp32 rows, mask applied as in
              k_epilogue_bwd_colsum.  A float32 sum of n terms in ANY order is within n u sum|g| of it; an accumulated target adds
              one rounding of the result, u |prefill + sum|.
    reg       scal[1] = mean z^2 + mean w_rel^2.  Reference: float64 means of the fp32 z the same sweep stored (its bits are held
              to the separate reparameterisation by tests/test_gpu_model.py) and of w_rel.  Each half is a sum of N non-negative
              terms (one product rounding each) in any order, then one scaling and the final add:
              (n h + 4) u mean z^2 + (numel w + 4) u mean w^2.

The references are never taken from the fold under test.  Every comparison prints RATIO <what> <largest |got - ref| / bound>.

Shapes: h = 4 (one lane live), 200 (50 of 64 lanes), 256 (a full wave), 260 and 500 (two column tiles, the second with 1 and 61
lanes); n = 1, 15, 37 (fewer rows than the 256 row slices: empty slices; 15 and 37 are no multiple of the 16 rows of a workgroup
round), 1000 (several rounds per slice); k = 1 and 10 folded.  h = 6 and k = 12 are outside the float4-column backward's rule
(ops.kl_seam_fold_ok) and must run the separate launches and still be right."""
import functools

import pytest
import torch

gpu = pytest.mark.gpu
U = 2.0 ** -24
P_DROP = 0.2
SCALE = float(torch.tensor(1.0 / (1.0 - P_DROP), dtype=torch.float32))
HS, NS = (4, 200, 256, 260, 500), (1, 15, 37, 1000)


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def ratio(what, got, ref, bound):
    got, ref, bound = got.double().cpu().reshape(-1), ref.double().cpu().reshape(-1), bound.double().cpu().reshape(-1)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), what
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(r.max()) if r.numel() else 0.0
    print(f'RATIO {what} {worst:.3f}')
    assert worst <= 1.0, f'{what}: largest |got - ref| / bound = {worst}'


@functools.lru_cache(maxsize=None)
def problem(n, h, k, mask='p'):
    gen = torch.Generator().manual_seed(1000 * n + 10 * h + k)
    h2 = torch.randn(n, 2 * h, generator=gen)
    if h >= 4:
        h2[0, h:h + 4] = torch.tensor([25.0, -30.0, 19.99, 20.01])           # softplus threshold on both sides
    eps = torch.randn(n, h, generator=gen)
    z_pre = torch.randn(2 * k, h, generator=gen) * 0.5
    gz_up = torch.randn(n, h, generator=gen) * 1e-2
    keep = {'p': (torch.rand(n, 2 * h, generator=gen) >= P_DROP), 'zeros': torch.zeros(n, 2 * h, dtype=torch.bool),
            'ones': torch.ones(n, 2 * h, dtype=torch.bool), None: None}[mask]
    prefill = torch.randn(2 * h, generator=gen)
    return h2, eps, z_pre, gz_up, None if keep is None else keep.to(torch.uint8), prefill


def kl_forward(ops, h2, eps, z_pre):
    """gv_reparam_kl_fwd into a NaN-filled workspace (nothing read that was not written)."""
    lib, ptr = ops.lib, ops.ptr
    n, h, k = h2.shape[0], h2.shape[1] // 2, z_pre.shape[0] // 2
    ws = torch.full((int(lib.load().gv_kl_workspace_bytes(n, h, k)) // 4,), float('nan'), device='cuda')
    z, v, m = (torch.empty(n, h, device='cuda') for _ in range(3))
    resp = torch.empty(n, k, device='cuda')
    lib.call('gv_reparam_kl_fwd', ptr(h2), ptr(eps), ptr(z_pre), ptr(z), ptr(v), ptr(m), ptr(resp), ptr(ws), n, h, k, lib.stream())
    return z, v, m, resp, ws


def seam_backward(ops, n, h, k, mask, accumulate, with_gz):
    """Both routes of the backward on the same forward state: (rows, bias, g_zpre) folded and separate, the keep mask, the prefill."""
    lib, ptr = ops.lib, ops.ptr
    h2, eps, z_pre, gz_up, keep, prefill = (None if t is None else t.cuda() for t in problem(n, h, k, mask))
    z, v, _, resp, ws = kl_forward(ops, h2, eps, z_pre)
    gkl = torch.tensor([1.3], device='cuda')
    gz = gz_up if with_gz else None
    scale = SCALE if keep is not None else 1.0
    out = {}
    for route in ('separate', 'folded'):
        gh2, gzp = torch.full_like(h2, float('nan')), torch.full_like(z_pre, float('nan'))
        bias = prefill.clone() if accumulate else torch.full((2 * h,), float('nan'), device='cuda')
        if route == 'folded':
            lib.call('gv_reparam_kl_bwd_fold', ptr(z), ptr(h2), ptr(v), ptr(eps), ptr(z_pre), ptr(resp), ptr(gkl), 0.01, 1e-4, ptr(gz),
                     ptr(gh2), ptr(gzp), 0, ptr(keep), scale, ptr(bias), 1 if accumulate else 0, ptr(ws), n, h, k, lib.stream())
            rows = gh2
        else:
            lib.call('gv_reparam_kl_bwd', ptr(z), ptr(h2), ptr(v), ptr(eps), ptr(z_pre), ptr(resp), ptr(gkl), 0.01, 1e-4, ptr(gz),
                     ptr(gh2), ptr(gzp), 0, ptr(ws), n, h, k, lib.stream())
            rows = ops.epilogue_bwd(None, gh2, ops.ACT_NONE, keep, scale, colsum_out=bias, colsum_accumulate=accumulate)
        torch.cuda.synchronize()
        out[route] = (rows.cpu(), bias.cpu(), gzp.cpu(), gh2.cpu())
    return out, keep, prefill.cpu()


def check_seam(tag, out, keep, prefill, n, accumulate):
    rows_s, bias_s, gzp_s, raw = out['separate']
    rows_f, bias_f, gzp_f, _ = out['folded']
    assert torch.isfinite(rows_f).all() and torch.equal(rows_f, rows_s), f'{tag}: masked rows differ'
    assert torch.equal(gzp_f, gzp_s), f'{tag}: g_zpre differs'
    # the mask rule itself, on the separate route's unmasked rows (float32: the same single multiply)
    want = raw if keep is None else torch.where(keep.cpu() != 0, raw * torch.tensor(SCALE), torch.zeros(()))
    assert torch.equal(rows_f, want), f'{tag}: rows are not keep ? value * scale : 0'
    g64 = rows_s.double()
    ref, bound = g64.sum(0), n * U * g64.abs().sum(0)
    if accumulate:
        ref = ref + prefill.double()
        bound = bound + U * ref.abs()
    ratio(f'{tag} bias folded', bias_f, ref, bound)
    ratio(f'{tag} bias separate', bias_s, ref, bound)


@gpu
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('h', HS)
def test_backward_fold_over_shapes(ops, n, h):
    """Every (n, h) of the module docstring at k = 10 with a p = 0.2 keep mask, an upstream gz and a fresh bias gradient."""
    out, keep, prefill = seam_backward(ops, n, h, 10, 'p', False, True)
    check_seam(f'n={n} h={h} k=10', out, keep, prefill, n, False)


@gpu
@pytest.mark.parametrize('n,h,k,mask,accumulate,with_gz', [
    (37, 200, 1, 'p', False, True), (1000, 260, 1, 'p', True, False), (15, 4, 1, None, True, True),
    (37, 200, 10, None, False, True), (1000, 200, 10, None, True, False),
    (37, 200, 10, 'zeros', True, True), (37, 260, 10, 'ones', False, False), (1000, 500, 10, 'zeros', False, True),
    (1000, 200, 10, 'p', True, True), (15, 256, 10, 'p', True, False), (1, 4, 10, 'ones', True, False)])
def test_backward_fold_variants(ops, n, h, k, mask, accumulate, with_gz):
    """k = 1, no keep mask (dropout off: rows unmasked, bias still summed), all-zero and all-one masks, the bias gradient
    accumulated into a pre-filled slot, no upstream gz."""
    out, keep, prefill = seam_backward(ops, n, h, k, mask, accumulate, with_gz)
    check_seam(f'n={n} h={h} k={k} mask={mask} acc={accumulate} gz={with_gz}', out, keep, prefill, n, accumulate)


@gpu
def test_fold_entry_point_refuses_what_the_column_form_does_not_cover(ops):
    """h % 4 != 0 and k > 10: gv_reparam_kl_bwd_fold fails loudly and launches nothing (the host must not ask)."""
    lib, ptr = ops.lib, ops.ptr
    for n, h, k in ((15, 6, 10), (15, 8, 12)):
        h2, eps, z_pre, gz_up, keep, _ = (t.cuda() for t in problem(n, h, k, 'p'))
        z, v, _, resp, ws = kl_forward(ops, h2, eps, z_pre)
        gh2, gzp, bias = torch.zeros_like(h2), torch.zeros_like(z_pre), torch.zeros(2 * h, device='cuda')
        gkl = torch.tensor([1.0], device='cuda')
        with pytest.raises(RuntimeError, match='float4-column'):
            lib.call('gv_reparam_kl_bwd_fold', ptr(z), ptr(h2), ptr(v), ptr(eps), ptr(z_pre), ptr(resp), ptr(gkl), 0.01, 1e-4, None,
                     ptr(gh2), ptr(gzp), 0, ptr(keep), SCALE, ptr(bias), 0, ptr(ws), n, h, k, lib.stream())
        torch.cuda.synchronize()
        assert float(gh2.abs().sum()) == 0.0 and float(bias.abs().sum()) == 0.0


@gpu
@pytest.mark.parametrize('n,h,k', [(1, 4, 1), (15, 6, 10), (37, 200, 10), (1000, 256, 10), (1000, 260, 10), (37, 500, 1), (1000, 500, 10)])
def test_regulariser_from_the_forward_sweep(ops, n, h, k):
    """scal[1] of gv_loss_combine_fold (sum z^2 from the three forward forms: four nodes per wave, float4 columns, lane per
    column at h = 6; w_rel^2 summed by the combine block) and of the separate gv_mean_sq2 route, against float64."""
    lib, ptr = ops.lib, ops.ptr
    h2, eps, z_pre, *_ = (None if t is None else t.cuda() for t in problem(n, h, k, None))
    z, _, _, _, ws = kl_forward(ops, h2, eps, z_pre)
    w_rel = torch.randn(8, h, generator=torch.Generator().manual_seed(h)).cuda() * 0.4
    ws_pred = torch.zeros(2048, device='cuda')
    z64, w64 = z.double().cpu(), w_rel.double().cpu()
    ref_z, ref_w = z64.pow(2).mean(), w64.pow(2).mean()
    ref, bound = ref_z + ref_w, (n * h + 4) * U * ref_z + (w64.numel() + 4) * U * ref_w
    scal, loss = torch.full((4,), float('nan'), device='cuda'), torch.empty((), device='cuda')
    lib.call('gv_loss_combine_fold', ptr(ws_pred), 16, ptr(w_rel), z.numel(), w_rel.numel(), ptr(ws), n, h, k, None, 0, 0, 0.5, 0.0,
             0.0, ptr(scal), ptr(loss), lib.stream())
    ratio(f'n={n} h={h} reg folded', scal[1], ref, bound)
    ratio(f'n={n} h={h} loss = reg_w * reg', loss, 0.5 * ref, 0.5 * bound + U * 0.5 * ref)
    ws2 = torch.empty(1024, device='cuda')
    lib.call('gv_mean_sq2', ptr(z), z.numel(), 1.0 / z.numel(), ptr(w_rel), w_rel.numel(), 1.0 / w_rel.numel(), None, ptr(ws2), None,
             n, lib.stream())
    scal2 = torch.full((4,), float('nan'), device='cuda')
    lib.call('gv_loss_combine', ptr(ws_pred), 16, ptr(ws2), z.numel(), w_rel.numel(), None, n, h, 0, None, 0, 0, 0.5, 0.0, 0.0,
             ptr(scal2), ptr(loss), None, lib.stream())
    ratio(f'n={n} h={h} reg separate', scal2[1], ref, bound)


def record_calls(monkeypatch, ops):
    names, real = [], ops.lib.call

    def call(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(ops.lib, 'call', call)
    return names


def head_step(ops, monkeypatch, fold, n, h, k, bias_target=None, extra_consumer=False, with_keep=True):
    """ops.reparam + ops.loss_head on a leaf h2 with a hand-made EpilogueLink standing for the layer: returns the names of the
    launches, whether the backward folded, (rows, bias, ...) as the layer's backward would have them, (loss, kl) and the loss's
    regulariser bound reg_w * ((n h + 4) u mean z^2 + (numel w + 4) u mean w^2) + u |loss| from float64."""
    monkeypatch.setattr(ops, 'KL_SEAM_FOLD', fold)
    names = record_calls(monkeypatch, ops)
    h2, eps, z_pre, _, keep, _ = (None if t is None else t.cuda() for t in problem(n, h, k, 'p' if with_keep else None))
    gen = torch.Generator().manual_seed(7)
    T, R = 64, 4
    trip = torch.stack([torch.randint(0, n, (T,), generator=gen), torch.randint(0, R, (T,), generator=gen),
                        torch.randint(0, n, (T,), generator=gen)], 1).cuda()
    labels = (torch.rand(T, generator=gen) > 0.5).float().cuda()
    w_rel = (torch.randn(R, h, generator=gen) * 0.3).cuda().requires_grad_()
    h2, z_pre = h2.requires_grad_(), z_pre.requires_grad_()
    scale = SCALE if keep is not None else 1.0
    epi = ops.EpilogueLink(keep, scale, True, bias_target, 2 * h)
    z, m, v = ops.reparam(h2, eps, z_pre, epi)
    tidx = ops.TripletIndex(trip, n, R, sync_free=True)
    loss, _, kl, _ = ops.loss_head(z, m, v, w_rel, z_pre, None, None, None, labels, tidx, 0.01, 1e-2, 0.0, False)
    total = loss + (m * 0.001).sum() if extra_consumer else loss
    total.backward()
    folded = epi.buf is not None            # (h2 is a leaf here: its .grad is a copy of the recorded buffer)
    if folded:
        rows = h2.grad
        bias = bias_target if bias_target is not None else epi.grad_bias
    else:
        bias = bias_target if bias_target is not None else torch.empty(2 * h, device='cuda')
        rows = ops.epilogue_bwd(None, h2.grad, ops.ACT_NONE, keep, scale, colsum_out=bias, colsum_accumulate=bias_target is not None)
    torch.cuda.synchronize()
    monkeypatch.undo()
    z64, w64 = z.detach().double().cpu(), w_rel.detach().double().cpu()
    reg_bound = 0.01 * ((n * h + 4) * U * z64.pow(2).mean() + (w64.numel() + 4) * U * w64.pow(2).mean()) + U * loss.detach().double().abs().cpu()
    return names, folded, (rows.cpu(), bias.cpu(), z_pre.grad.cpu(), w_rel.grad.cpu()), (loss.detach().cpu(), kl.detach().cpu()), reg_bound


FOLD_CALLS = ('gv_reparam_kl_bwd_fold', 'gv_loss_combine_fold')
SEPARATE_CALLS = ('gv_mean_sq2', 'gv_reparam_kl_bwd', 'gv_loss_combine')


@gpu
@pytest.mark.parametrize('n,h,k,slot', [(37, 200, 10, False), (37, 200, 10, True), (1000, 260, 1, True), (15, 4, 10, False)])
def test_hand_off_through_reparam_and_loss_head(ops, monkeypatch, n, h, k, slot):
    """The Python route: with the switch on the two fold entry points run and none of the three launches; rows, z_pre's and
    w_rel's gradients carry the switch-off route's bits, the bias gradient (fresh, or added into a pre-filled direct slot) and
    the loss stay inside their bounds."""
    prefill = problem(n, h, k)[5]
    names_f, was_f, (rows_f, bias_f, gzp_f, gw_f), (loss_f, kl_f), rb = head_step(ops, monkeypatch, True, n, h, k, prefill.clone().cuda() if slot else None)
    names_s, was_s, (rows_s, bias_s, gzp_s, gw_s), (loss_s, kl_s), _ = head_step(ops, monkeypatch, False, n, h, k, prefill.clone().cuda() if slot else None)
    assert was_f and not was_s
    assert all(c in names_f for c in FOLD_CALLS) and not any(c in names_f for c in SEPARATE_CALLS + ('gv_rgcn_epilogue_bwd', 'gv_colsum_finish'))
    assert all(c in names_s for c in SEPARATE_CALLS) and not any(c in names_s for c in FOLD_CALLS)
    assert torch.equal(rows_f, rows_s) and torch.equal(gzp_f, gzp_s) and torch.equal(gw_f, gw_s) and torch.equal(kl_f, kl_s)
    g64 = rows_s.double()
    ref = g64.sum(0) + (prefill.double() if slot else 0.0)
    bound = n * U * g64.abs().sum(0) + (U * ref.abs() if slot else 0.0)
    ratio(f'ops n={n} h={h} k={k} slot={slot} bias folded', bias_f, ref, bound)
    ratio(f'ops n={n} h={h} k={k} slot={slot} bias separate', bias_s, ref, bound)
    # the two losses differ by the regulariser's summation order alone: each is within its bound of the exact value
    ratio(f'ops n={n} h={h} k={k} loss folded vs separate', loss_f, loss_s, 2 * rb)


@gpu
@pytest.mark.parametrize('n,h,k,extra', [(15, 6, 10, False), (37, 8, 12, False), (37, 200, 10, True)])
def test_unfolded_routes_stay_right(ops, monkeypatch, n, h, k, extra):
    """h = 6 (h % 4 != 0), k = 12 (> 10 components) and another consumer of z_mean (gm arrives): the backward is NOT folded even
    with the switch on -- the plain gv_reparam_kl_bwd runs and the layer's own epilogue pass does the mask and the bias -- and
    gives the switch-off route's bits.  The forward's sum z^2 fold does not depend on the backward's rule."""
    names_f, was_f, res_f, (loss_f, kl_f), rb = head_step(ops, monkeypatch, True, n, h, k, extra_consumer=extra)
    names_s, was_s, res_s, (loss_s, kl_s), _ = head_step(ops, monkeypatch, False, n, h, k, extra_consumer=extra)
    assert not was_f and not was_s
    assert 'gv_reparam_kl_bwd' in names_f and 'gv_reparam_kl_bwd_fold' not in names_f and 'gv_loss_combine_fold' in names_f
    for a, b in zip(res_f, res_s):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(kl_f, kl_s)
    ratio(f'unfolded n={n} h={h} k={k} loss', loss_f, loss_s, 2 * rb)


def tiny_link_predict(ops, dropout):
    import numpy as np
    from gcn_vae_amd import sampling
    from gcn_vae_amd.data import synthetic_kg
    from gcn_vae_amd.encoders import KGVAE
    from gcn_vae_amd.layers import RelGraphConv
    from gcn_vae_amd.train import LinkPredict
    data = synthetic_kg(60, 3, 400, seed=0)
    adj, deg = sampling.get_adj_and_degrees(data.num_nodes, data.train)
    np.random.seed(0)
    g, node_id, etype, node_norm, samples, labels = sampling.generate_sampled_graph_and_labels(
        data.train, 200, 0.5, data.num_rels, adj, deg, 4, 'uniform')
    torch.manual_seed(0)
    net = LinkPredict(KGVAE, data.num_nodes, 8, data.num_rels, num_bases=4, num_hidden_layers=2, dropout=dropout, use_cuda=True,
                      reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=0).cuda().train()
    net.static_batch = True
    n = len(node_id)
    gen = torch.Generator().manual_seed(1)
    net.encoder.eps_override = torch.randn(n, 8, generator=gen).cuda()
    if dropout > 0:
        for mod in net.modules():
            if isinstance(mod, RelGraphConv):
                mod.keep_mask_override = (torch.rand(n, mod.out_feat, generator=gen) >= dropout).to(torch.uint8).cuda()
    nid, et = torch.from_numpy(node_id).view(-1, 1).cuda(), torch.from_numpy(etype).cuda()
    en = sampling.node_norm_to_edge_norm(g, torch.from_numpy(node_norm).view(-1, 1)).cuda()
    st, lt = torch.from_numpy(samples).cuda(), torch.from_numpy(labels).cuda()
    return net, (g, nid, et, en, st, lt), n


@gpu
@pytest.mark.parametrize('dropout', [0.2, 0.0])
def test_full_step_eager_and_captured(ops, monkeypatch, dropout):
    """One LinkPredict step on a 60-node, 3-relation graph at h = 8: loss and every parameter gradient, folded against switch-off
    -- everything but layer 2's bias gradient and the loss carries the same bits; those two stay inside the bounds of the module
    docstring -- and the folded step captured and replayed twice as a graph gives the eager folded bits."""
    results, g_rows = {}, {}
    for fold in (False, True):
        monkeypatch.setattr(ops, 'KL_SEAM_FOLD', fold)
        names = record_calls(monkeypatch, ops)
        net, (g, nid, et, en, st, lt), n = tiny_link_predict(ops, dropout)
        params = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
        for _, p in params:
            p.grad = torch.zeros_like(p)

        def step():
            for _, p in params:
                p.grad.zero_()
            loss, pred, _, _ = net.get_loss(g, net(g, nid, et, en), st, lt)
            loss.backward()
            return loss

        def snapshot(loss):
            torch.cuda.synchronize()
            return [loss.detach().clone().cpu()] + [p.grad.clone().cpu() for _, p in params]

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = snapshot(step())
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if fold:
            assert all(c in names for c in FOLD_CALLS) and 'gv_mean_sq2' not in names and 'gv_colsum_finish' in names
            assert names.count('gv_rgcn_epilogue_bwd') == names.count('gv_reparam_kl_bwd_fold')      # layer 1's only
        else:
            assert not any(c in names for c in FOLD_CALLS) and 'gv_mean_sq2' in names
            assert names.count('gv_rgcn_epilogue_bwd') == 2 * names.count('gv_reparam_kl_bwd')
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = step()
        runs = []
        for _ in range(2):
            graph.replay()
            runs.append(snapshot(out))
        for a, b, c in zip(eager, runs[0], runs[1]):
            assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(b, c)
        results[fold] = eager
        monkeypatch.undo()
        if not fold:      # the rows layer 2's epilogue gradient sees on the separate route, for the bias bound
            h2_seen = []
            enc = net.encoder
            inner = enc.rconv_layer_2.forward

            def layer_2_with_hook(*a, **k):
                h = inner(*a, **k)
                h.register_hook(lambda gr: h2_seen.append(gr.detach().clone()))
                return h
            enc.rconv_layer_2.forward = layer_2_with_hook
            monkeypatch.setattr(ops, 'KL_SEAM_FOLD', False)
            with torch.cuda.stream(side):
                embed = net(g, nid, et, en)
                loss, _, _, _ = net.get_loss(g, embed, st, lt)
                loss.backward()
            torch.cuda.synchronize()
            monkeypatch.undo()
            keep = enc.rconv_layer_2.keep_mask_override
            raw = h2_seen[0].cpu()
            g_rows['rows'] = raw if keep is None else torch.where(keep.cpu() != 0, raw * torch.tensor(SCALE), torch.zeros(()))
            z64, w64 = embed.detach().double().cpu(), net.w_relation.detach().double().cpu()
            g_rows['reg'] = 0.01 * ((z64.numel() + 4) * U * z64.pow(2).mean() + (w64.numel() + 4) * U * w64.pow(2).mean())
            g_rows['n'] = n
    names_p = [k for k, p in net.named_parameters() if p.requires_grad]
    g64 = g_rows['rows'].double()
    for name, a, b in zip(['loss'] + names_p, results[False], results[True]):
        if name == 'loss':
            ratio(f'step dropout={dropout} loss', b, a, 2 * (g_rows['reg'] + U * a.double().abs()))
        elif name.endswith('rconv_layer_2.h_bias'):
            bound = g_rows['n'] * U * g64.abs().sum(0)
            ratio(f'step dropout={dropout} {name} folded', b, g64.sum(0), bound)
            ratio(f'step dropout={dropout} {name} separate', a, g64.sum(0), bound)
        else:
            assert torch.equal(a, b), name
