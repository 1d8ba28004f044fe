"""Riders on the fp32 self-loop product (csrc/k_riders.h, gv_gemm_f32_riders, ops.RiderBox): the forward's random draws, a layer's
lane-packed weights and the KL mixture table as extra workgroups of the product's launch.

Everything here is an EQUALITY: the riders' bodies are the stand-alone kernels' bodies, Philox is counter-based -- (group in job,
stream, tick) -- and the tile workgroups run the plain kernel's body with the plain kernel's tile order, so every output of the
combined launch must carry the bits of gv_gemm_f32 + gv_rng_fill + gv_rgcn_bdd_pack_weight(_pair) + gv_kl_mix launched one after the
other with the same {seed, tick}.  No tolerance anywhere."""
import ctypes
import itertools

import pytest
import torch

gpu = pytest.mark.gpu
pytestmark = gpu

SEED, TICK = 0x1234_5678_9ABC, 7
MASK, NORMAL = 0, 1
P_DROP = 0.2
GV_ERR_SHAPE = -2


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as o
    o.lib.load()
    return o


def rng_state():
    return torch.tensor([SEED, TICK], dtype=torch.int64).cuda()


def rng_buffers(spec):
    """[(kind, n)] -> [(tensor, kind, p, stream)]; a guard element behind each buffer shows a write past its end."""
    jobs = []
    for i, (kind, n) in enumerate(spec):
        if kind == MASK:
            t = torch.full((n + 4,), 0xEE, dtype=torch.uint8).cuda()
        else:
            t = torch.full((n + 4,), float('nan'), dtype=torch.float32).cuda()
        jobs.append((t, n, kind, P_DROP, 100 + i))
    return jobs


def smallest_pack_shape(ops, blk_in, blk_out, transpose_w):
    for nb in range(1, 129):
        if ops.pack_supported(nb, blk_in, blk_out, transpose_w):
            return nb
    raise AssertionError(f'no packed kernel for {blk_in}x{blk_out} trans={transpose_w}')


EIGHT = [(MASK, 1), (MASK, 3), (MASK, 5), (MASK, 1027), (NORMAL, 2), (NORMAL, 1026), (MASK, 64), (NORMAL, 4)]


def launch_pair(ops, shape, act, accumulate, rng_spec, pack, mix, split_k=1, alias_c=None):
    """Both routes on the same inputs: (rc, outputs of the combined launch, outputs of the separate launches)."""
    l = ops.lib.load()
    ptr, st = ops.ptr, ops.lib.stream()
    m, n, k = shape
    gen = torch.Generator().manual_seed(m * 1000 + n * 10 + k)
    a = torch.randn(m, k, generator=gen).cuda()
    b = torch.randn(k, n, generator=gen).cuda()
    bias = torch.randn(n, generator=gen).cuda()
    c0 = torch.randn(m, n, generator=gen).cuda()
    state = rng_state()
    outs = {}
    for route in ('riders', 'separate'):
        c = c0.clone()
        jobs = rng_buffers(rng_spec)
        d = ops._Riders()
        res = {'c': c}
        if jobs:
            d.rng_state, d.rng_jobs = state.data_ptr(), len(jobs)
            for i, (t, cnt, kind, p, stream) in enumerate(jobs):
                d.rng_ptr[i], d.rng_count[i], d.rng_kind[i], d.rng_drop_p[i], d.rng_stream[i] = t.data_ptr(), cnt, kind, p, stream
                res[f'rng{i}'] = t
        if pack is not None:
            nb, bi, bo, trans, pair = pack
            w = torch.randn(3, nb * bi * bo, generator=torch.Generator().manual_seed(5)).cuda()
            packed = torch.full_like(w, float('nan'))
            packed2 = torch.full_like(w, float('nan')) if pair else None
            d.pack_weight, d.packed, d.packed_pair = w.data_ptr(), packed.data_ptr(), (packed2.data_ptr() if pair else None)
            d.pack_rels, d.pack_bases, d.pack_blk_in, d.pack_blk_out, d.pack_transpose = 3, nb, bi, bo, 1 if trans else 0
            res['packed'] = packed
            if pair:
                res['packed2'] = packed2
        if mix is not None:
            mk, mh = mix
            z_pre = torch.randn(2 * mk, mh, generator=torch.Generator().manual_seed(6)).cuda() * 3
            z_pre[mk, 0] = 25.0                                   # the linear branch of the softplus
            table = torch.full((3 * mk * mh + 4,), float('nan')).cuda()
            d.mix_z_pre, d.mix, d.mix_k, d.mix_h = z_pre.data_ptr(), table.data_ptr(), mk, mh
            res['mix'] = table
        if alias_c is not None and route == 'riders':
            alias_c(d, c)
        ws_bytes = int(l.gv_gemm_workspace_bytes(m, n, k, split_k)) if split_k > 1 else 0
        ws = torch.empty(max(ws_bytes // 4, 1)).cuda()
        gemm_args = (0, 0, m, n, k, ptr(a), k, ptr(b), n, ptr(c), n, ptr(bias), act, accumulate, split_k, None,
                     ptr(ws) if split_k > 1 else None, ws_bytes)
        if route == 'riders':
            rc = l.gv_gemm_f32_riders(*gemm_args, ctypes.addressof(d), st)
            outs['rc'] = rc
        else:
            assert l.gv_gemm_f32(*gemm_args, st) == 0
            if jobs:
                nj = len(jobs)
                assert l.gv_rng_fill(state.data_ptr(), nj, (ctypes.c_void_p * nj)(*[j[0].data_ptr() for j in jobs]),
                                     (ctypes.c_int64 * nj)(*[j[1] for j in jobs]), (ctypes.c_int32 * nj)(*[j[2] for j in jobs]),
                                     (ctypes.c_float * nj)(*[j[3] for j in jobs]), (ctypes.c_uint32 * nj)(*[j[4] for j in jobs]),
                                     st) == 0
            if pack is not None:
                if pair:
                    assert l.gv_rgcn_bdd_pack_weight_pair(ptr(w), 3, nb, bi, bo, ptr(packed), ptr(packed2), st) == 0
                else:
                    assert l.gv_rgcn_bdd_pack_weight(ptr(w), 3, nb, bi, bo, 1 if trans else 0, ptr(packed), st) == 0
            if mix is not None:
                assert l.gv_kl_mix(ptr(z_pre), mk, mh, ptr(table), st) == 0
        torch.cuda.synchronize()
        outs[route] = res
    return outs


def assert_same(outs):
    assert outs['rc'] == 0, outs['rc']
    got, want = outs['riders'], outs['separate']
    assert sorted(got) == sorted(want)
    for name in want:
        g, w = got[name], want[name]
        if g.dtype == torch.float32:       # bit patterns: the NaN guards compare equal too
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g, w), name


@pytest.mark.parametrize('shape', [(1, 1, 1), (65, 72, 40), (513, 130, 24)])
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_all_rider_kinds_on_every_product_shape(ops, shape, act, accumulate):
    """Eight RNG jobs (masks of 1, 3, 5 and 1027 elements at p = 0.2, normals of 2 and 1026), the 2 x 4 weight pair of the smallest
    supported shape with 3 relation types and the (10, 200) mixture table on: one tile; 2 x 2 ragged tiles with a k tail; 9 row
    tiles (the XCD remap branch with riders present) -- with bias, act none / ReLU, accumulate 0 / 1."""
    nb = smallest_pack_shape(ops, 2, 4, False)
    assert ops.pack_supported(nb, 4, 2, True)
    outs = launch_pair(ops, shape, act, accumulate, EIGHT, (nb, 2, 4, False, True), (10, 200))
    assert_same(outs)
    for i, (kind, n) in enumerate(EIGHT):     # every element drawn, nothing behind the end
        t = outs['riders'][f'rng{i}']
        if kind == MASK:
            assert int(t[:n].max()) <= 1 and bool((t[n:] == 0xEE).all())
        else:
            assert bool(torch.isfinite(t[:n]).all()) and bool(torch.isnan(t[n:]).all())
    keep = outs['riders']['rng3'][:1027].float().mean()
    assert 0.7 < float(keep) < 0.9
    assert bool(torch.isfinite(outs['riders']['mix'][:6000]).all()) and bool(torch.isnan(outs['riders']['mix'][6000:]).all())


@pytest.mark.parametrize('spec', [[(MASK, 1)], [(MASK, 3)], [(MASK, 5)], [(MASK, 1027)], [(NORMAL, 2)], [(NORMAL, 1026)]])
def test_one_rng_job_alone(ops, spec):
    assert_same(launch_pair(ops, (65, 72, 40), 0, 0, spec, None, None))


def test_pack_4x2_transposed_alone_and_mix_1x4(ops):
    """The smallest 4 x 2 shape (the transposed, backward-x kind; no forward 4 x 2 kernel exists) with 3 relation types, the single
    2 x 4 layout without its pair, and the (1, 4) mixture table."""
    nb = smallest_pack_shape(ops, 4, 2, True)
    assert_same(launch_pair(ops, (65, 72, 40), 1, 0, [], (nb, 4, 2, True, False), (1, 4)))
    nb = smallest_pack_shape(ops, 2, 4, False)
    assert_same(launch_pair(ops, (65, 72, 40), 0, 1, [], (nb, 2, 4, False, False), None))
    assert_same(launch_pair(ops, (1, 1, 1), 0, 0, [], None, (1, 4)))


def test_far_more_and_far_fewer_rider_blocks_than_tiles(ops):
    many = [(MASK, 1027), (NORMAL, 1027), (MASK, 1027), (NORMAL, 1026)]
    assert_same(launch_pair(ops, (1, 1, 1), 0, 0, many, None, (10, 200)))            # 1 tile, a dozen rider workgroups
    assert_same(launch_pair(ops, (513, 130, 24), 1, 1, [(MASK, 1)], None, None))      # 27 tiles, 1 rider workgroup


def test_no_riders_is_the_plain_entry(ops):
    """An empty description and a NULL one: gv_gemm_f32 itself -- split-K, which the riders' kernel does not have, included."""
    assert_same(launch_pair(ops, (65, 72, 40), 1, 1, [], None, None))
    assert_same(launch_pair(ops, (65, 72, 200), 0, 0, [], None, None, split_k=2))
    l, ptr = ops.lib.load(), ops.ptr
    a, b = torch.randn(65, 40).cuda(), torch.randn(40, 72).cuda()
    c1, c2 = torch.empty(65, 72).cuda(), torch.empty(65, 72).cuda()
    assert l.gv_gemm_f32_riders(0, 0, 65, 72, 40, ptr(a), 40, ptr(b), 72, ptr(c1), 72, None, 0, 0, 1, None, None, 0, None, None) == 0
    assert l.gv_gemm_f32(0, 0, 65, 72, 40, ptr(a), 40, ptr(b), 72, ptr(c2), 72, None, 0, 0, 1, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(c1, c2)


def test_refusals_launch_nothing(ops):
    def mask_into_c(d, c):
        d.rng_ptr[0] = c.data_ptr() + 16

    outs = launch_pair(ops, (65, 72, 40), 0, 1, [(MASK, 64)], None, None, alias_c=mask_into_c)
    assert outs['rc'] == GV_ERR_SHAPE and 'operand' in ops.lib.last_error()
    assert bool((outs['riders']['rng0'] == 0xEE).all())             # nothing was launched: the job's own buffer is untouched

    def mix_into_c(d, c):
        d.mix = c.data_ptr()

    outs = launch_pair(ops, (65, 72, 40), 0, 1, [], None, (1, 4), alias_c=mix_into_c)
    assert outs['rc'] == GV_ERR_SHAPE
    outs = launch_pair(ops, (65, 72, 200), 0, 0, [(MASK, 64)], None, None, split_k=2)
    assert outs['rc'] == GV_ERR_SHAPE and 'split' in ops.lib.last_error()
    assert bool((outs['riders']['rng0'] == 0xEE).all())


# ---- model level ---------------------------------------------------------------------------------------------------
def tiny_model(ops):
    """~70 nodes, 4 relations (8 directed: num_bases = 8 needs at least 8 relation types), ~300 directed edges; h_dim 16 over 8 bases: 2 x 2 blocks in layer 1, 2 x 4 in layer 2
    (the packed route); dropout 0.2; 40 triplets."""
    import numpy as np
    from gcn_vae_amd import sampling
    from gcn_vae_amd.data import synthetic_kg
    from gcn_vae_amd.encoders import KGVAE
    from gcn_vae_amd.train import LinkPredict
    data = synthetic_kg(70, 4, 600, seed=0)
    adj, deg = sampling.get_adj_and_degrees(data.num_nodes, data.train)
    np.random.seed(0)
    g, node_id, etype, node_norm, samples, labels = sampling.generate_sampled_graph_and_labels(
        data.train, 300, 0.5, data.num_rels, adj, deg, 1, 'uniform')
    samples, labels = samples[:40], labels[:40]
    torch.manual_seed(0)
    # a module takes process-unique Philox stream ids at construction: two models draw the same numbers only from the same ids
    saved, ops._rng_streams = ops._rng_streams, itertools.count(5000)
    try:
        net = LinkPredict(KGVAE, data.num_nodes, 16, data.num_rels, num_bases=8, num_hidden_layers=2, dropout=0.2, use_cuda=True,
                          reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=0).cuda().train()
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
    return rng


def test_training_step_with_and_without_the_route(ops, monkeypatch):
    """One training step from the same seed and tick with the route on and with GV_GEMM_RIDERS=0: loss, z, both keep masks, every
    parameter gradient and the weights after one FlatAdam step."""
    from gcn_vae_amd.optim import FlatAdam
    seen = {}
    for route in (True, False):
        monkeypatch.setattr(ops, 'GEMM_RIDERS', route)
        net, (g, nid, et, en, st, lt) = tiny_model(ops)
        params = [p for p in net.parameters() if p.requires_grad]
        opt = FlatAdam(params, lr=1e-3, max_grad_norm=1.0)
        set_tick(ops, 3)
        opt.zero_grad()
        z = net(g, nid, et, en)
        box1, box2 = net.encoder._rider_boxes
        assert box1.done and box2.done
        assert len(box1.rng[1]) == 3 and box2.mix is not None and box2.pack is not None and box2.pack[6] is not None
        assert box1.rode == (('rng',) if route else ()) and box2.rode == (('mix', 'pack') if route else ())
        loss = net.get_loss(g, z, st, lt)[0]
        loss.backward()
        grads = [p.grad.detach().clone() for p in params]
        opt.step()
        torch.cuda.synchronize()
        seen[route] = ([loss.detach().clone(), z.detach().clone()] + [t.clone() for t, _, _, _ in box1.rng[1]] + grads +
                       [p.detach().clone() for p in params])
        monkeypatch.undo()
    assert len(seen[True]) == len(seen[False]) > 10
    for a, b in zip(seen[True], seen[False]):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    keep1 = seen[True][2]
    assert keep1.dtype == torch.uint8 and 0.6 < float(keep1.float().mean()) < 0.95


def test_captured_step_draws_fresh_numbers_and_equals_eager(ops):
    """The step (forward, loss, backward; fixed weights) captured once and replayed twice: each replay draws at a fresh tick -- the
    keep masks differ -- and equals the eager step run at that tick."""
    net, (g, nid, et, en, st, lt) = tiny_model(ops)
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.zeros_like(p)

    def step():
        for p in params:
            p.grad.zero_()
        z = net(g, nid, et, en)
        loss = net.get_loss(g, z, st, lt)[0]
        loss.backward()
        box1, box2 = net.encoder._rider_boxes
        assert box1.rode == ('rng',) and box2.rode == ('mix', 'pack')
        return [loss, z] + [t for t, _, _, _ in box1.rng[1]]

    def snapshot(out):
        torch.cuda.synchronize()
        return [t.detach().clone() for t in out] + [p.grad.clone() for p in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    set_tick(ops, 0)
    with torch.cuda.stream(side):
        step()                                      # tick 0 -> 1
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    runs = []
    for _ in range(2):                              # ticks 2 and 3
        graph.replay()
        runs.append(snapshot(out))
    assert not torch.equal(runs[0][2], runs[1][2]) and not torch.equal(runs[0][3], runs[1][3])      # both layers' keep masks
    set_tick(ops, 1)
    with torch.cuda.stream(side):
        for replayed in runs:
            eager = snapshot(step())
            assert len(eager) == len(replayed)
            for a, b in zip(eager, replayed):
                assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    torch.cuda.current_stream().wait_stream(side)
