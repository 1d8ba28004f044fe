"""The finisher kinds among the riders (csrc/k_riders.h, gv_gemm_f32_riders_fin, ops.RiderBox): the prior sampler of get_mmd on a
forward self-loop product, the KL backward's finishing launch and the bias column sums of an epilogue backward on the backward's
dL/dx = g @ loop_weight^T.

Everything here is an EQUALITY.  The prior sampler's rider IS its kernel's body.  The two slice sums run as 256-thread workgroups
inside the product, 1024-thread blocks alone: both form the same 64 slice-group sums with the same function and add them in the
same order, and share the store expressions -- so every output of the combined launch must carry the bits of gv_gemm_f32 +
gv_prior_sample_fwd + gv_kl_bwd_mix_final + gv_colsum_finish launched one after the other.  No tolerance anywhere."""
import ctypes
import itertools
import random

import pytest
import torch

gpu = pytest.mark.gpu
pytestmark = gpu

GV_ERR_SHAPE = -2
KINDS = ('prior', 'klfin', 'colsum')
# the product of the issue: a partial row tile, a partial column tile and a K tail; and a single tile, which every kind outnumbers
RAGGED, ONE_TILE = (130, 40, 72), (1, 1, 1)


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as o
    o.lib.load()
    return o


def guard(t, fill):
    """A copy of ``t`` followed by 4 guard elements (a write past the end shows)."""
    out = torch.full((t.numel() + 4,), float('nan')).cuda()
    if fill:
        out[:t.numel()] = t.reshape(-1)
    return out


def launch_pair(ops, shape, trans_b, kinds, slices=37, accumulate=0, kl_bias=True, kl_kh=(3, 8), alias=None):
    """Both routes on the same inputs: {'rc', 'riders': outputs of the combined launch, 'separate': of the separate launches}."""
    l = ops.lib.load()
    ptr, st = ops.ptr, ops.lib.stream()
    m, n, k = shape
    gen = torch.Generator().manual_seed(m * 1000 + n * 10 + k + slices)
    a = torch.randn(m, k, generator=gen).cuda()
    b = (torch.randn(n, k, generator=gen) if trans_b else torch.randn(k, n, generator=gen)).cuda()
    bias = torch.randn(n, generator=gen).cuda()
    c0 = torch.randn(m, n, generator=gen).cuda()
    # prior sampler: 40 samples of 3 components x 8 columns (320 elements: two workgroups, the second partial)
    pk, ph, ps = 3, 8, 40
    z_pre = torch.randn(2 * pk, ph, generator=gen).cuda() * 3
    z_pre[pk, 0] = 25.0                                         # the linear branch of the softplus
    eps = torch.randn(ps, ph, generator=gen).cuda()
    # KL finisher: 3 components, h = 8: (2 * 3 + 2) * 8 = 64 columns with the bias sums (4 workgroups: padded to 8), 48 without
    kk, kh = kl_kh
    cols = (2 * kk + (2 if kl_bias else 0)) * kh
    kl_part = torch.randn(slices, cols, generator=gen).cuda()
    kl_zpre = torch.randn(2 * kk, kh, generator=gen).cuda() * 3
    kl_zpre[kk, 1] = 25.0
    gkl = torch.tensor([0.7]).cuda()
    gz0, gb0 = torch.randn(2 * kk * kh, generator=gen).cuda(), torch.randn(2 * kh, generator=gen).cuda()
    # column sums: 40 columns (3 workgroups, the last partial)
    cn = 40
    cs_part = torch.randn(slices, cn, generator=gen).cuda()
    cs0 = torch.randn(cn, generator=gen).cuda()
    outs = {}
    for route in ('riders', 'separate'):
        c = c0.clone()
        res = {'c': c}
        f = ops._RidersFin()
        if 'prior' in kinds:
            res['z_pri'] = guard(eps, False)
            f.prior_z_pre, f.prior_eps, f.prior_out = z_pre.data_ptr(), eps.data_ptr(), res['z_pri'].data_ptr()
            f.prior_s, f.prior_k, f.prior_h = ps, pk, ph
        if 'klfin' in kinds:
            res['g_zpre'] = guard(gz0, accumulate)
            f.kl_part, f.kl_slices, f.kl_z_pre, f.kl_gkl = kl_part.data_ptr(), slices, kl_zpre.data_ptr(), gkl.data_ptr()
            f.kl_g_zpre, f.kl_gscale, f.kl_n, f.kl_h, f.kl_k = res['g_zpre'].data_ptr(), 0.3, 1000, kh, kk
            f.kl_accumulate = f.kl_accumulate_bias = accumulate
            if kl_bias:
                res['g_bias'] = guard(gb0, accumulate)
                f.kl_g_bias = res['g_bias'].data_ptr()
        if 'colsum' in kinds:
            res['colsum'] = guard(cs0, accumulate)
            f.cs_part, f.cs_out, f.cs_n, f.cs_slices, f.cs_accumulate = cs_part.data_ptr(), res['colsum'].data_ptr(), cn, slices, accumulate
        if alias is not None and route == 'riders':
            alias(f, a, b, c)
        gemm_args = (0, trans_b, m, n, k, ptr(a), k, ptr(b), k if trans_b else n, ptr(c), n, ptr(bias), 0, accumulate, 1, None, None, 0)
        if route == 'riders':
            outs['rc'] = l.gv_gemm_f32_riders_fin(*gemm_args, None, ctypes.addressof(f), st)
        else:
            assert l.gv_gemm_f32(*gemm_args, st) == 0                   # the plain product: the tiles must be undisturbed
            if 'prior' in kinds:
                assert l.gv_prior_sample_fwd(ptr(z_pre), ptr(eps), ptr(res['z_pri']), ps, pk, ph, st) == 0
            if 'klfin' in kinds:
                assert l.gv_kl_bwd_mix_final(ptr(kl_part), slices, ptr(kl_zpre), ptr(gkl), 0.3, ptr(res['g_zpre']), accumulate,
                                             ptr(res['g_bias']) if kl_bias else None, accumulate, 1000, kh, kk, st) == 0
            if 'colsum' in kinds:
                assert l.gv_colsum_finish(ptr(cs_part), cn, slices, ptr(res['colsum']), accumulate, st) == 0
        torch.cuda.synchronize()
        outs[route] = res
    return outs


def assert_same(outs):
    assert outs['rc'] == 0, outs['rc']
    got, want = outs['riders'], outs['separate']
    assert sorted(got) == sorted(want)
    for name in want:      # bit patterns: the NaN guards compare equal too
        assert torch.equal(got[name].view(torch.int32), want[name].view(torch.int32)), name
        body = want[name] if name == 'c' else want[name][:-4]
        assert bool(torch.isfinite(body).all()), name
        assert name == 'c' or bool(torch.isnan(got[name][-4:]).all()), name


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('trans_b', [0, 1])
@pytest.mark.parametrize('shape', [RAGGED, ONE_TILE])
def test_one_kind_alone(ops, shape, trans_b, kind):
    """Each kind by itself (2, 4 and 3 workgroups: each count is padded to 8 in front of the tiles) on the ragged product and on a
    single tile, which every kind outnumbers -- on A @ B and on A @ B^T; 37 slices: 27 of the 64 slice groups are empty."""
    assert_same(launch_pair(ops, shape, trans_b, (kind,)))


@pytest.mark.parametrize('slices', [1, 37, 130, 250, 256])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_all_kinds_together_over_slice_counts(ops, slices, accumulate):
    """The three kinds in one launch of the backward's product, stored and accumulated, over partial counts that leave slice groups
    empty (1, 37), leave a group a tail behind its 4-wide steps (130: 3 per group) or a short last group (250: 4 per group, 2 in group
    62), and the KL backward's own 256."""
    assert_same(launch_pair(ops, RAGGED, 1, KINDS, slices=slices, accumulate=accumulate))


def test_kl_finisher_without_bias_columns_and_at_model_width(ops):
    assert_same(launch_pair(ops, RAGGED, 1, ('klfin',), kl_bias=False))                       # 48 columns: 3 workgroups
    assert_same(launch_pair(ops, RAGGED, 1, ('klfin',), slices=256, kl_kh=(10, 200)))        # 4 400 columns: 275 workgroups, 3 tiles


def test_no_finisher_is_the_plain_entry(ops):
    assert_same(launch_pair(ops, RAGGED, 1, ()))
    assert_same(launch_pair(ops, RAGGED, 0, ()))


def test_overlap_with_a_product_operand_is_refused_and_launches_nothing(ops):
    def colsum_into_c(f, a, b, c):
        f.cs_out = c.data_ptr() + 16

    outs = launch_pair(ops, RAGGED, 1, ('colsum',), alias=colsum_into_c)
    assert outs['rc'] == GV_ERR_SHAPE and 'overlaps' in ops.lib.last_error()
    assert bool(torch.isnan(outs['riders']['colsum']).all())            # nothing was launched: the job's own buffer is untouched

    def zpre_grad_into_a(f, a, b, c):
        f.kl_g_zpre = a.data_ptr()

    outs = launch_pair(ops, RAGGED, 1, ('klfin',), alias=zpre_grad_into_a)
    assert outs['rc'] == GV_ERR_SHAPE and bool(torch.isnan(outs['riders']['g_bias']).all())

    def samples_into_b(f, a, b, c):
        f.prior_out = b.data_ptr()

    outs = launch_pair(ops, RAGGED, 0, ('prior',), alias=samples_into_b)
    assert outs['rc'] == GV_ERR_SHAPE

    def partials_in_c(f, a, b, c):             # a rider INPUT that the product writes
        f.cs_part = c.data_ptr()

    outs = launch_pair(ops, RAGGED, 1, ('colsum',), slices=4, alias=partials_in_c)
    assert outs['rc'] == GV_ERR_SHAPE and bool(torch.isnan(outs['riders']['colsum']).all())


# ---- model level ---------------------------------------------------------------------------------------------------
def small_model(ops):
    """~350 nodes (get_mmd picks 200 posterior rows), 4 relations (8 directed), h_dim 16 over 8 bases, dropout 0.2, all four loss
    terms on; 60 triplets."""
    import numpy as np
    from gcn_vae_amd import sampling
    from gcn_vae_amd.data import synthetic_kg
    from gcn_vae_amd.encoders import KGVAE
    from gcn_vae_amd.train import LinkPredict
    data = synthetic_kg(400, 4, 4000, seed=0)
    adj, deg = sampling.get_adj_and_degrees(data.num_nodes, data.train)
    np.random.seed(0)
    g, node_id, etype, node_norm, samples, labels = sampling.generate_sampled_graph_and_labels(
        data.train, 2000, 0.5, data.num_rels, adj, deg, 1, 'uniform')
    assert len(node_id) >= 200
    samples, labels = samples[:60], labels[:60]
    torch.manual_seed(0)
    saved, ops._rng_streams = ops._rng_streams, itertools.count(7000)      # (process-unique Philox stream ids: the same for both models)
    try:
        net = LinkPredict(KGVAE, data.num_nodes, 16, data.num_rels, num_bases=8, num_hidden_layers=2, dropout=0.2, use_cuda=True,
                          reg_param=0.01, kl_param=1e-3, mmd_param=1e-2, k=4, n_flows=0).cuda().train()
    finally:
        ops._rng_streams = saved
    net.static_batch = True
    nid, et = torch.from_numpy(node_id).view(-1, 1).cuda(), torch.from_numpy(etype).cuda()
    en = sampling.node_norm_to_edge_norm(g, torch.from_numpy(node_norm).view(-1, 1)).cuda()
    st, lt = torch.from_numpy(samples).cuda(), torch.from_numpy(labels).cuda()
    return net, (g, nid, et, en, st, lt)


def set_tick(ops, tick):
    rng = ops.device_rng(torch.device('cuda', torch.cuda.current_device()))
    rng._sync_seed()
    rng.state.copy_(torch.tensor([rng._seed, tick], dtype=torch.int64))
    rng._used.clear()
    torch.cuda.synchronize()


def one_step(ops, monkeypatch, live=False):
    """One training step at tick 3; returns (launch names in order, boxes made, tensors to compare)."""
    from gcn_vae_amd.optim import FlatAdam
    net, (g, nid, et, en, st, lt) = small_model(ops)
    params = [p for p in net.parameters() if p.requires_grad]
    opt = FlatAdam(params, lr=1e-3, max_grad_norm=1.0)
    set_tick(ops, 3)
    random.seed(0)                                      # get_mmd's posterior row pick
    names, boxes = [], []
    real_call, real_box = ops.lib.call, ops.RiderBox

    def call(name, *args, **kw):
        names.append(name)
        return real_call(name, *args, **kw)

    class CountedBox(real_box):
        __slots__ = ()

        def __init__(self):
            super().__init__()
            boxes.append(self)

    monkeypatch.setattr(ops.lib, 'call', call)
    monkeypatch.setattr(ops, 'RiderBox', CountedBox)
    opt.zero_grad()
    ctx = ops.live_rows(torch.tensor([nid.shape[0]], dtype=torch.int32).cuda(), nid.shape[0]) if live else ops.live_rows(None, 0)
    with ctx:
        z = net(g, nid, et, en)
        loss = net.get_loss(g, z, st, lt)[0]
        loss.backward()
    grads = [p.grad.detach().clone() for p in params]
    opt.step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return names, boxes, [loss.detach().clone(), z.detach().clone()] + grads + [p.detach().clone() for p in params]


ALONE = ('gv_prior_sample_fwd', 'gv_kl_bwd_mix_final', 'gv_colsum_finish', 'gv_reparam_kl_bwd_fold')


def test_training_step_with_and_without_the_route(ops, monkeypatch):
    """One training step from the same seed and tick with the route on and with GV_GEMM_RIDERS=0: the finishers ride on three products
    (layer 2's forward, both layers' dL/dx) and none is launched alone; every gradient and the weights after one FlatAdam step are
    bitwise those of the separate launches, which make no box in the backward."""
    monkeypatch.setattr(ops, 'GEMM_RIDERS', True)
    names, boxes, on = one_step(ops, monkeypatch)
    assert names.count('gv_gemm_f32_riders_fin') == 3 and 'gv_reparam_kl_bwd_fold_sweep' in names
    assert not [n for n in names if n in ALONE]
    assert sorted(b.rode for b in boxes) == [('colsum',), ('klfin',), ('mix', 'pack', 'prior'), ('rng',)]
    monkeypatch.setattr(ops, 'GEMM_RIDERS', False)
    names, boxes, off = one_step(ops, monkeypatch)
    assert len(boxes) == 2 and all(b.done and b.rode == () for b in boxes)        # the forward's two, launched stand-alone
    assert not [n for n in names if n.startswith('gv_gemm_f32_riders') or n == 'gv_reparam_kl_bwd_fold_sweep']
    assert all(n in names for n in ('gv_prior_sample_fwd', 'gv_colsum_finish', 'gv_reparam_kl_bwd_fold'))
    assert len(on) == len(off) > 10
    for a, b in zip(on, off):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)


def test_one_kind_switched_alone(ops, monkeypatch):
    """GV_GEMM_RIDER_KINDS: with only 'klfin' allowed, the forward's kinds and the other finishers are launched alone where they stood."""
    monkeypatch.setattr(ops, 'GEMM_RIDERS', True)
    monkeypatch.setattr(ops, 'GEMM_RIDER_KINDS', {'klfin'})
    names, boxes, _ = one_step(ops, monkeypatch)
    assert names.count('gv_gemm_f32_riders_fin') == 1                 # (the forward's boxes go through gv_gemm_f32_riders, empty)
    assert all(n in names for n in ('gv_rng_fill', 'gv_kl_mix', 'gv_prior_sample_fwd', 'gv_colsum_finish', 'gv_reparam_kl_bwd_fold_sweep'))
    assert sorted(b.rode for b in boxes) == [(), (), ('klfin',)]


def test_static_shape_batch_step_makes_no_boxes(ops, monkeypatch):
    """Inside a static-shape batch step (ops.live_rows) the products count live rows and carry nothing: no box is made, forward or
    backward, and every small launch stands where it stood."""
    monkeypatch.setattr(ops, 'GEMM_RIDERS', True)
    names, boxes, _ = one_step(ops, monkeypatch, live=True)
    assert boxes == []
    assert not [n for n in names if n.startswith('gv_gemm_f32_riders') or n == 'gv_reparam_kl_bwd_fold_sweep']
    assert all(n in names for n in ('gv_prior_sample_fwd', 'gv_colsum_finish', 'gv_reparam_kl_bwd_fold', 'gv_gemm_f32_live_rows'))
