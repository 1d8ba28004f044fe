"""The fused DistMult head (csrc/k_loss.hip: gv_distmult_bce_fwd_grad + gv_distmult_grad_finish, taken by ops.loss_head and
ops.distmult_bce) and the separate sweeps it replaces, against a float64 CPU computation of the same formulas
(oracle.kgvae.distmult_score, torch's binary_cross_entropy_with_logits, the regulariser):

    x_t    = sum_c e[s_t,c] w[r_t,c] e[o_t,c] + b                 loss = mean_t bce(x_t, y_t) + reg (mean e^2 + mean w^2)
    delta_t = sigmoid(x_t) - y_t                                   G = upstream gradient (1 or 1.7), d_t = (G/T) delta_t
    dW[r,c] = sum_{t in r} d_t e[s_t,c] e[o_t,c] + G (2 reg / numel(w)) w[r,c]
    dE[n,c] = sum_{(t, other) incident to n} d_t e[other,c] w[r_t,c] + G (2 reg / numel(e)) e[n,c]
    db      = sum_t d_t

Bounds (u = 2**-24; a sum of k float32 terms in ANY order, each term carrying a few roundings of its own, is off by at most
(term count) u (sum of |terms|); a derivative bound carries an input error through):

    E_x[t]    = (h + 2) u (sum_c |e_s w_r e_o| + |b|)
    E_d[t]    = E_x[t] / 4 + 4 u             (|sigmoid'| <= 1/4; exp, the division and the subtraction on values <= 1)
    loss      : mean_t E_x[t]  (|bce'| <= 1)  + (T + 8) u mean_t |bce_t|  + (numel + 4) u reg mean sq, for e and for w
    dW[r,c]   : (G/T) sum_{t in r} |e_s e_o| E_d[t]  + (n_r + h) u (G/T) sum_{t in r} |delta_t e_s e_o|  + 4 u |regulariser term|
    dE[n,c]   : (G/T) sum_inc |e_other w_r| E_d[t]   + (deg_n + h) u (G/T) sum_inc |delta_t e_other w_r| + 4 u |regulariser term|
    db        : (G/T) sum_t E_d[t] + (T + 4) u (G/T) sum_t |delta_t|

n_r: the relation's triplet count, deg_n: the entity's incidence count.  A relation with no triplet has the regulariser's term
alone inside 4 u of it; its row is written (no stale memory: the buffers are pre-filled with NaN where the test can reach them).
Every comparison prints RATIO <what> <largest |got - ref| / bound>.

Shapes: 13 entities, 5 relations, T = 77 cut into by-relation items of 16: relation 0 empty, 1 one triplet, 2 forty (three
slices: split items, slots, the ordered slot sum), 3 twenty-five (two slices), 4 eleven.  One triplet has s == o, one has a
score beyond +-20 (sigmoid saturates).  h = 200 (lanes 50-63 idle), 16, 4 (one lane); 10 and 260 are outside the fused sweep's
rule (ops.distmult_fused_ok) and must run the separate sweeps inside the same bounds."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import kgvae as okg

gpu = pytest.mark.gpu
U = 2.0 ** -24
N_ENT, N_REL, T, CHUNK_REL, REG = 13, 5, 77, 16, 0.01
REL_COUNTS = (0, 1, 40, 25, 11)
SAT = 76            # the saturating triplet (entities 11, 12 belong to it alone); triplet 0 has s == o
FUSED_H, DECLINED_H = (200, 16, 4), (10, 260)
G_UP = float(torch.tensor(1.7, dtype=torch.float32))


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def problem(h, labels_kind='mixed'):
    gen = torch.Generator().manual_seed(100 + h)
    e = torch.randn(N_ENT, h, generator=gen) * 0.7
    w = torch.randn(N_REL, h, generator=gen) * 0.7
    rel = torch.cat([torch.full((c,), r) for r, c in enumerate(REL_COUNTS)])
    rel = rel[torch.randperm(T, generator=gen)]
    s = torch.randint(0, 11, (T,), generator=gen)
    o = torch.randint(0, 11, (T,), generator=gen)
    o[0] = s[0]
    s[SAT], o[SAT] = 11, 12
    r_sat = int(rel[SAT])
    w[r_sat] = torch.where(w[r_sat].abs() < 0.6, torch.where(w[r_sat] < 0, -0.6, 0.6), w[r_sat])
    e[11] = 3.0
    e[12] = 3.0 * torch.sign(w[r_sat])
    trip = torch.stack([s, rel, o], 1).contiguous()
    y = {'mixed': (torch.rand(T, generator=gen) < 0.4).float(), 'zeros': torch.zeros(T), 'ones': torch.ones(T)}[labels_kind]
    assert sorted(torch.bincount(rel, minlength=N_REL).tolist()) == sorted(REL_COUNTS)
    return e, w, trip, y


@functools.lru_cache(maxsize=None)
def reference(h, labels_kind, bias, g_up):
    """float64 values, gradients and the bounds of the module docstring; computed once per case, never modified."""
    e32, w32, trip, y32 = problem(h, labels_kind)
    e, w, y = e32.double().requires_grad_(), w32.double().requires_grad_(), y32.double()
    b = torch.tensor(0.3 if bias else 0.0, dtype=torch.float64, requires_grad=True)
    x = okg.distmult_score(e, w, trip) + b
    bce = F.binary_cross_entropy_with_logits(x, y, reduction='none')
    pred = bce.mean()
    loss = pred + REG * (e.pow(2).mean() + w.pow(2).mean())
    (loss * g_up).backward()
    ed, wd, xd = e.detach(), w.detach(), x.detach()
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    assert abs(float(xd[SAT])) > 20.0
    E_x = (h + 2) * U * ((ed[s] * wd[r] * ed[o]).abs().sum(1) + abs(float(b.detach())))
    E_d = E_x / 4 + 4 * U
    delta = torch.sigmoid(xd) - y
    gt = g_up / T
    b_pred = E_x.mean() + (T + 8) * U * bce.detach().abs().mean()
    b_loss = b_pred + (ed.numel() + 4) * U * REG * ed.pow(2).mean() + (wd.numel() + 4) * U * REG * wd.pow(2).mean()
    p = (ed[s] * ed[o]).abs()
    n_r = torch.bincount(r, minlength=N_REL).double()
    b_w = torch.zeros(N_REL, h, dtype=torch.float64).index_add_(0, r, gt * p * (E_d[:, None] + (n_r[r][:, None] + h) * U * delta.abs()[:, None]))
    b_w += 4 * U * (g_up * 2 * REG / wd.numel() * wd).abs()
    ent, oth = torch.cat([s, o]), torch.cat([o, s])
    deg = torch.bincount(ent, minlength=N_ENT).double()
    q = (ed[oth] * wd[torch.cat([r, r])]).abs()
    E_d2, d2 = torch.cat([E_d, E_d]), torch.cat([delta, delta]).abs()
    b_e = torch.zeros(N_ENT, h, dtype=torch.float64).index_add_(0, ent, gt * q * (E_d2[:, None] + (deg[ent][:, None] + h) * U * d2[:, None]))
    b_e += 4 * U * (g_up * 2 * REG / ed.numel() * ed).abs()
    b_b = gt * E_d.sum() + (T + 4) * U * gt * delta.abs().sum()
    return dict(score=xd, pred=pred.detach(), loss=loss.detach(), g_e=e.grad, g_w=w.grad, g_b=b.grad, delta=delta,
                b_score=E_x, b_pred=b_pred, b_loss=b_loss, b_e=b_e, b_w=b_w, b_b=b_b)


def make_index(ops, trip, flavour):
    if flavour == 'locality':
        idx = ops.TripletIndex(trip.cuda(), N_ENT, N_REL, chunk_rel=CHUNK_REL, locality=True)
        assert idx.pos3 is not None and idx.fwd_order is not None and idx.rel.n_fix == 2
    else:
        idx = ops.TripletIndex(trip.to(torch.int32).cuda(), N_ENT, N_REL, chunk_rel=CHUNK_REL, sync_free=True)
        assert idx.pos3 is None and not idx.rel.exact
    return idx


def record_calls(monkeypatch, ops):
    names, real = [], ops.lib.call

    def call(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(ops.lib, 'call', call)
    return names


def run_head(ops, h, flavour, labels_kind='mixed', bias=True, g_up=G_UP, arena=None, twice=False, idx=None):
    """One loss_head forward + backward on the GPU; returns the outputs and gradients (CPU float64)."""
    e32, w32, trip, y = problem(h, labels_kind)
    e, w = e32.cuda().requires_grad_(), w32.cuda().requires_grad_()
    b = torch.tensor(0.3, device='cuda', requires_grad=True) if bias else None
    idx = make_index(ops, trip, flavour) if idx is None else idx
    if arena is not None:
        ops.DIRECT_GRAD[w.data_ptr()] = arena
    try:
        loss, pred, _, _ = ops.loss_head(e, None, None, w, None, b, None, None, y.cuda(), idx, REG, 0.0, 0.0, True)
        up = loss * g_up if g_up != 1.0 else loss
        up.backward(retain_graph=twice)
        first = None
        if twice:
            first = (e.grad.clone(), w.grad.clone(), b.grad.clone())
            e.grad = w.grad = b.grad = None
            up.backward()
    finally:
        ops.DIRECT_GRAD.pop(w.data_ptr(), None)
    torch.cuda.synchronize()
    out = dict(loss=loss.detach().double().cpu(), pred=pred.detach().double().cpu(), g_e=e.grad.double().cpu(),
               g_w=None if arena is not None else w.grad.double().cpu(), g_b=b.grad.double().cpu() if bias else None, first=first,
               raw=(e.grad, None if arena is not None else w.grad))
    return out


def scores_of(ops, h, flavour, labels_kind='mixed', bias=True, grad=True):
    """(loss, score) of ops.distmult_bce -- the entry that hands the scores out."""
    e32, w32, trip, y = problem(h, labels_kind)
    e, w = e32.cuda().requires_grad_(grad), w32.cuda().requires_grad_(grad)
    b = torch.tensor(0.3, device='cuda') if bias else None
    loss, score = ops.distmult_bce(e, w, b, y.cuda(), make_index(ops, trip, flavour))
    return loss.detach().double().cpu(), score.detach().double().cpu()


def within(tag, got, ref, bound):
    ratio = float(((got - ref).abs() / bound).max())
    print(f'RATIO {tag} {ratio:.4f}')
    assert torch.isfinite(got).all(), f'{tag}: non-finite values'
    assert ratio <= 1.0, f'{tag}: |got - ref| is {ratio:.3f} of the bound'
    return ratio


def check_against_reference(tag, out, ref):
    within(f'{tag} loss', out['loss'], ref['loss'], ref['b_loss'])
    within(f'{tag} predict_loss', out['pred'], ref['pred'], ref['b_pred'])
    within(f'{tag} grad_z', out['g_e'], ref['g_e'], ref['b_e'])
    if out['g_w'] is not None:
        within(f'{tag} grad_w', out['g_w'], ref['g_w'], ref['b_w'])
    if out['g_b'] is not None:
        within(f'{tag} grad_bias', out['g_b'], ref['g_b'], ref['b_b'])


@gpu
@pytest.mark.parametrize('flavour', ['locality', 'native'])
@pytest.mark.parametrize('h', FUSED_H + DECLINED_H)
def test_head_inside_the_float64_bounds(ops, monkeypatch, h, flavour):
    """Bias, upstream gradient 1.7, mixed labels, at every width and both index flavours; the widths the rule declines run the
    separate sweeps, the others the fused pair and none of the launches it replaces."""
    names = record_calls(monkeypatch, ops)
    out = run_head(ops, h, flavour)
    fused = h in FUSED_H
    assert ('gv_distmult_bce_fwd_grad' in names) == fused and ('gv_distmult_grad_finish' in names) == fused
    assert ('gv_bce_grad' in names) == (not fused) and ('gv_rgcn_bdd_grad_weight' in names) == (not fused)
    assert ('gv_distmult_bce_fwd' in names) == (not fused)
    ref = reference(h, 'mixed', True, G_UP)
    check_against_reference(f'head h={h} {flavour}', out, ref)
    empty = REL_COUNTS.index(0)          # the relation without a triplet: the regulariser's term alone
    term = G_UP * 2 * REG / (N_REL * h) * problem(h)[1][empty].double()
    within(f'head h={h} {flavour} empty relation row', out['g_w'][empty], term, 4 * U * term.abs())
    loss, score = scores_of(ops, h, flavour)
    within(f'scores h={h} {flavour}', score, ref['score'], ref['b_score'])
    within(f'distmult_bce loss h={h} {flavour}', loss, ref['pred'], ref['b_pred'])


@gpu
@pytest.mark.parametrize('labels_kind,bias,g_up', [('zeros', True, 1.0), ('ones', False, G_UP), ('mixed', False, 1.0)])
@pytest.mark.parametrize('h', [200, 4])
def test_head_variants(ops, h, labels_kind, bias, g_up):
    out = run_head(ops, h, 'locality', labels_kind, bias, g_up)
    check_against_reference(f'variant h={h} {labels_kind} bias={bias} g={g_up:.1f}', out, reference(h, labels_kind, bias, g_up))


@gpu
@pytest.mark.parametrize('flavour', ['locality', 'native'])
def test_relation_gradient_accumulates_into_the_arena_slot(ops, monkeypatch, flavour):
    """ops.DIRECT_GRAD (the optimiser's gradient arena): the finishing launch adds into the slot, every row once -- the empty
    relation's and the split ones' too."""
    h = 16
    names = record_calls(monkeypatch, ops)
    gen = torch.Generator().manual_seed(3)
    before = torch.randn(N_REL, h, generator=gen)
    arena = before.cuda()
    out = run_head(ops, h, flavour, arena=arena)
    assert 'gv_distmult_grad_finish' in names
    ref = reference(h, 'mixed', True, G_UP)
    got = arena.double().cpu() - before.double()
    within(f'arena grad_w {flavour}', got, ref['g_w'], ref['b_w'] + U * (before.double().abs() + ref['g_w'].abs()))
    check_against_reference(f'arena {flavour}', out, ref)


@gpu
@pytest.mark.parametrize('flavour', ['locality', 'native'])
@pytest.mark.parametrize('h', FUSED_H)
def test_fused_against_the_separate_sweeps(ops, monkeypatch, h, flavour):
    """Same inputs down both paths: everything inside the sum of the two paths' bounds (twice the bound: both meet the same
    one), and the entity-side launch is the same launch on the same coefficients wherever delta has the same bits."""
    idx = make_index(ops, problem(h)[2], flavour)
    new = run_head(ops, h, flavour, idx=idx)
    new_scores = scores_of(ops, h, flavour)
    monkeypatch.setattr(ops, 'DISTMULT_FUSED', False)
    names = record_calls(monkeypatch, ops)
    old = run_head(ops, h, flavour, idx=idx)
    old_scores = scores_of(ops, h, flavour)
    assert 'gv_bce_grad' in names and 'gv_distmult_bce_fwd_grad' not in names
    ref = reference(h, 'mixed', True, G_UP)
    for key, bound in (('loss', 'b_loss'), ('pred', 'b_pred'), ('g_e', 'b_e'), ('g_w', 'b_w'), ('g_b', 'b_b')):
        within(f'fused-vs-old {key} h={h} {flavour}', new[key], old[key], 2 * ref[bound])
    within(f'fused-vs-old scores h={h} {flavour}', new_scores[1], old_scores[1], 2 * ref['b_score'])
    if torch.equal(new_scores[1], old_scores[1]):       # same scores -> the same (g/T) (sigmoid - y) bits -> the same launch
        assert torch.equal(new['raw'][0], old['raw'][0])


@gpu
@pytest.mark.parametrize('flavour', ['locality', 'native'])
@pytest.mark.parametrize('h', [200, 4])
def test_entry_points_write_every_row_of_nan_filled_buffers(ops, h, flavour):
    """The two entry points called directly on NaN-filled outputs (non-accumulating): every score, every coefficient and every
    relation row -- the empty relation's, the one-triplet relation's, the split ones' -- is written, and inside the bounds."""
    e32, w32, trip, y = problem(h)
    idx = make_index(ops, trip, flavour)
    e, w, seg = e32.cuda(), w32.cuda(), idx.rel
    nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')     # noqa: E731
    n_coef = 2 * T if idx.pos3 is not None else T
    score, delta, u, partial, g_w, d_out, dbias = nan(T), nan(n_coef), nan(N_REL, h), nan(seg.n_slots, h), nan(N_REL, h), nan(n_coef), nan(1)
    ws = torch.zeros(2048, device='cuda')
    bias, g = torch.tensor(0.3, device='cuda'), torch.tensor([G_UP], device='cuda')
    ptr, call = ops.lib.ptr, ops.lib.call
    call('gv_distmult_bce_fwd_grad', ptr(seg.items), seg.n_items, ptr(idx.rel_s), ptr(idx.rel_o), ptr(idx.rel_tid), ptr(e), h,
         ptr(w), h, ptr(y.cuda()), ptr(bias), ptr(idx.pos3), ptr(score), ptr(delta), ptr(u), ptr(partial), ptr(ws), T, h, ops.lib.stream())
    call('gv_distmult_grad_finish', ptr(g), ptr(u), ptr(partial), ptr(seg.fix), seg.n_fix, ptr(seg.rowptr), seg.chunk, N_REL, h,
         ptr(w), h, 2 * REG / w.numel(), ptr(g_w), h, 0, ptr(delta), ptr(d_out), n_coef, ptr(ws), ptr(dbias), T, ops.lib.stream())
    torch.cuda.synchronize()
    ref = reference(h, 'mixed', True, G_UP)
    tag = f'direct h={h} {flavour}'
    within(f'{tag} scores', score.double().cpu(), ref['score'], ref['b_score'])
    within(f'{tag} grad_w', g_w.double().cpu(), ref['g_w'], ref['b_w'])
    within(f'{tag} grad_bias', dbias.double().cpu()[0], ref['g_b'], ref['b_b'])
    empty = REL_COUNTS.index(0)
    term = G_UP * 2 * REG / (N_REL * h) * w32[empty].double()
    within(f'{tag} empty relation row', g_w[empty].double().cpu(), term, 4 * U * term.abs())
    assert torch.isfinite(d_out).all() and torch.isfinite(delta).all()
    E_d = ref['b_score'] / 4 + 4 * U
    if idx.pos3 is None:
        within(f'{tag} delta', delta.double().cpu(), ref['delta'], E_d)
    else:
        pos = idx.pos3.long().cpu()
        for k in (0, 1):
            within(f'{tag} delta (incidence side {k})', delta.double().cpu()[pos[:, k]], ref['delta'], E_d)
    pred = ws[:5].double().sum().cpu() / T               # red_blocks(77, 16) = 5 partial sums
    within(f'{tag} predict_loss partials', pred, ref['pred'], ref['b_pred'])


@gpu
@pytest.mark.parametrize('flavour', ['locality', 'native'])
def test_backward_twice_over_a_retained_graph(ops, flavour):
    out = run_head(ops, 16, flavour, twice=True)
    g_e1, g_w1, g_b1 = out['first']
    assert torch.equal(g_e1, out['raw'][0]) and torch.equal(g_w1, out['raw'][1])
    assert torch.equal(g_b1.double().cpu(), out['g_b'])
    check_against_reference(f'second backward {flavour}', out, reference(16, 'mixed', True, G_UP))


@gpu
def test_no_grad_forward_takes_the_plain_scorer(ops, monkeypatch):
    h = 16
    names = record_calls(monkeypatch, ops)
    e32, w32, trip, y = problem(h)
    idx = make_index(ops, trip, 'locality')
    b = torch.tensor(0.3, device='cuda')
    with torch.no_grad():
        loss, pred, _, _ = ops.loss_head(e32.cuda().requires_grad_(), None, None, w32.cuda().requires_grad_(), None, b, None,
                                         None, y.cuda(), idx, REG, 0.0, 0.0, True)
        loss2, score = ops.distmult_bce(e32.cuda(), w32.cuda(), b, y.cuda(), idx)
    assert 'gv_distmult_bce_fwd' in names and 'gv_distmult_bce_fwd_grad' not in names
    ref = reference(h, 'mixed', True, G_UP)
    within('no-grad loss', loss.double().cpu(), ref['loss'], ref['b_loss'])
    within('no-grad predict_loss', pred.double().cpu(), ref['pred'], ref['b_pred'])
    within('no-grad distmult_bce loss', loss2.double().cpu(), ref['pred'], ref['b_pred'])
    within('no-grad scores', score.double().cpu(), ref['score'], ref['b_score'])


@gpu
def test_captured_step_replays_the_eager_bits(ops, monkeypatch):
    """A tiny LinkPredict on a fixed batch: forward, loss head, backward captured as one graph; two replays give identical bits,
    equal to the eager step's.  The fused pair is what the capture records."""
    import numpy as np
    from gcn_vae_amd import sampling
    from gcn_vae_amd.data import synthetic_kg
    from gcn_vae_amd.encoders import KGVAE
    from gcn_vae_amd.train import LinkPredict

    data = synthetic_kg(300, 6, 1500, seed=0)
    adj, deg = sampling.get_adj_and_degrees(data.num_nodes, data.train)
    np.random.seed(0)
    g, node_id, etype, node_norm, samples, labels = sampling.generate_sampled_graph_and_labels(
        data.train, 400, 0.5, data.num_rels, adj, deg, 4, 'uniform')
    torch.manual_seed(0)
    net = LinkPredict(KGVAE, data.num_nodes, 16, data.num_rels, num_bases=4, num_hidden_layers=2, dropout=0.0, use_cuda=True,
                      reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=0).cuda().train()
    net.static_batch = True
    net.encoder.eps_override = torch.randn(len(node_id), 16, generator=torch.Generator().manual_seed(1)).cuda()
    nid, et = torch.from_numpy(node_id).view(-1, 1).cuda(), torch.from_numpy(etype).cuda()
    en = sampling.node_norm_to_edge_norm(g, torch.from_numpy(node_norm).view(-1, 1)).cuda()
    st, lt = torch.from_numpy(samples).cuda(), torch.from_numpy(labels).cuda()
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.zeros_like(p)
    names = record_calls(monkeypatch, ops)

    def step():
        for p in params:
            p.grad.zero_()
        loss, pred, _, _ = net.get_loss(g, net(g, nid, et, en), st, lt)
        loss.backward()
        return loss, pred

    def snapshot(loss, pred):
        torch.cuda.synchronize()
        return [loss.detach().clone(), pred.detach().clone()] + [p.grad.clone() for p in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = snapshot(*step())
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert 'gv_distmult_bce_fwd_grad' in names and 'gv_distmult_grad_finish' in names and 'gv_bce_grad' not in names
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    runs = []
    for _ in range(2):
        graph.replay()
        runs.append(snapshot(*out))
    assert all(torch.isfinite(t).all() for t in eager)
    for a, b, c in zip(eager, runs[0], runs[1]):
        assert torch.equal(a, b) and torch.equal(b, c)
