"""The 16-lane-row form of the fused DistMult forward (csrc/k_loss.hip: k_distmult_rows behind gv_distmult_bce_fwd_grad) at the
edges of its layout, against a float64 CPU computation of the same formulas (oracle.kgvae.distmult_score, torch's
binary_cross_entropy_with_logits, the regulariser):

    x_t    = sum_c e[s_t,c] w[r_t,c] e[o_t,c] + b                 loss = mean_t bce(x_t, y_t) + reg (mean e^2 + mean w^2)
    delta_t = sigmoid(x_t) - y_t                                   G = upstream gradient 1.7, d_t = (G/T) delta_t
    dW[r,c] = sum_{t in r} d_t e[s_t,c] e[o_t,c] + G (2 reg / numel(w)) w[r,c]
    dE[n,c] = sum_{(t, other) incident to n} d_t e[other,c] w[r_t,c] + G (2 reg / numel(e)) e[n,c]
    db      = sum_t d_t

Bounds, as in tests/test_gpu_distmult_fused.py (u = 2**-24; a sum of k float32 terms in ANY order, each term carrying a few
roundings of its own, is off by at most (term count) u (sum of |terms|); a derivative bound carries an input error through):

    E_x[t]    = (h + 2) u (sum_c |e_s w_r e_o| + |b|)
    E_d[t]    = E_x[t] / 4 + 4 u             (|sigmoid'| <= 1/4; exp, the division and the subtraction on values <= 1)
    loss      : mean_t E_x[t]  (|bce'| <= 1)  + (T + 8) u mean_t |bce_t|  + (numel + 4) u reg mean sq, for e and for w
    dW[r,c]   : (G/T) sum_{t in r} |e_s e_o| E_d[t]  + (n_r + h) u (G/T) sum_{t in r} |delta_t e_s e_o|  + 4 u |regulariser term|
    dE[n,c]   : (G/T) sum_inc |e_other w_r| E_d[t]   + (deg_n + h) u (G/T) sum_inc |delta_t e_other w_r| + 4 u |regulariser term|
    db        : (G/T) sum_t E_d[t] + (T + 4) u (G/T) sum_t |delta_t|

They hold for any summation order, so for the row form's (columns in lane order, the row butterfly, triplets == q (mod 4) of a
batch in row q, rows added (0 + 1) + (2 + 3)).  Every comparison prints RATIO <what> <largest |got - ref| / bound>.

Shapes: 13 entities (entity 12 in no triplet), 13 relations cut into by-relation items of 80, so a wave's 64-triplet batches
come full, followed by a second one, and short: relation counts 0, 1, 2, 3, 4, 5 (a step with three shadow rows), 7, 8, 9, 63,
64, 65 (a second batch of one triplet) and 150 (a split item with two slots, 80 + 70).  T = 381.  Triplet 0 has s == o, the last
one a score beyond +-20.  Widths: 4 (one lane of a row), 60, 64 (group 0 full), 68 (one lane of group 1), 200 and 256."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import kgvae as okg

gpu = pytest.mark.gpu
U = 2.0 ** -24
REL_COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 150)
N_ENT, N_REL, T, CHUNK_REL, REG = 13, len(REL_COUNTS), sum(REL_COUNTS), 80, 0.01
SAT = T - 1         # the saturating triplet (entities 10, 11 belong to it alone); triplet 0 has s == o; entity 12 is unreferenced
WIDTHS = (4, 60, 64, 68, 200, 256)
FLAVOURS = ('locality', 'native')
G_UP = float(torch.tensor(1.7, dtype=torch.float32))


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def problem(h):
    gen = torch.Generator().manual_seed(300 + h)
    e = torch.randn(N_ENT, h, generator=gen) * 0.7
    w = torch.randn(N_REL, h, generator=gen) * 0.7
    rel = torch.cat([torch.full((c,), r) for r, c in enumerate(REL_COUNTS)])
    rel = rel[torch.randperm(T, generator=gen)]
    s = torch.randint(0, 10, (T,), generator=gen)
    o = torch.randint(0, 10, (T,), generator=gen)
    o[0] = s[0]
    s[SAT], o[SAT] = 10, 11
    r_sat = int(rel[SAT])
    w[r_sat] = torch.where(w[r_sat].abs() < 0.6, torch.where(w[r_sat] < 0, -0.6, 0.6), w[r_sat])
    e[10] = 3.0
    e[11] = 3.0 * torch.sign(w[r_sat])
    trip = torch.stack([s, rel, o], 1).contiguous()
    y = (torch.rand(T, generator=gen) < 0.4).float()
    assert torch.bincount(rel, minlength=N_REL).tolist() == list(REL_COUNTS)
    assert 12 not in s.tolist() + o.tolist()
    return e, w, trip, y


@functools.lru_cache(maxsize=None)
def reference(h):
    """float64 values, gradients and the bounds of the module docstring (bias 0.3, upstream gradient G_UP); computed once per
    width, never modified."""
    e32, w32, trip, y32 = problem(h)
    e, w, y = e32.double().requires_grad_(), w32.double().requires_grad_(), y32.double()
    b = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    x = okg.distmult_score(e, w, trip) + b
    bce = F.binary_cross_entropy_with_logits(x, y, reduction='none')
    pred = bce.mean()
    loss = pred + REG * (e.pow(2).mean() + w.pow(2).mean())
    (loss * G_UP).backward()
    ed, wd, xd = e.detach(), w.detach(), x.detach()
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    assert abs(float(xd[SAT])) > 20.0
    E_x = (h + 2) * U * ((ed[s] * wd[r] * ed[o]).abs().sum(1) + abs(float(b.detach())))
    E_d = E_x / 4 + 4 * U
    delta = torch.sigmoid(xd) - y
    gt = G_UP / T
    b_pred = E_x.mean() + (T + 8) * U * bce.detach().abs().mean()
    b_loss = b_pred + (ed.numel() + 4) * U * REG * ed.pow(2).mean() + (wd.numel() + 4) * U * REG * wd.pow(2).mean()
    p = (ed[s] * ed[o]).abs()
    n_r = torch.bincount(r, minlength=N_REL).double()
    b_w = torch.zeros(N_REL, h, dtype=torch.float64).index_add_(0, r, gt * p * (E_d[:, None] + (n_r[r][:, None] + h) * U * delta.abs()[:, None]))
    b_w += 4 * U * (G_UP * 2 * REG / wd.numel() * wd).abs()
    ent, oth = torch.cat([s, o]), torch.cat([o, s])
    deg = torch.bincount(ent, minlength=N_ENT).double()
    q = (ed[oth] * wd[torch.cat([r, r])]).abs()
    E_d2, d2 = torch.cat([E_d, E_d]), torch.cat([delta, delta]).abs()
    b_e = torch.zeros(N_ENT, h, dtype=torch.float64).index_add_(0, ent, gt * q * (E_d2[:, None] + (deg[ent][:, None] + h) * U * d2[:, None]))
    b_e += 4 * U * (G_UP * 2 * REG / ed.numel() * ed).abs()
    b_b = gt * E_d.sum() + (T + 4) * U * gt * delta.abs().sum()
    return dict(score=xd, pred=pred.detach(), loss=loss.detach(), g_e=e.grad, g_w=w.grad, g_b=b.grad, delta=delta,
                b_score=E_x, b_delta=E_d, b_pred=b_pred, b_loss=b_loss, b_e=b_e, b_w=b_w, b_b=b_b)


def make_index(ops, trip, flavour):
    if flavour == 'locality':
        idx = ops.TripletIndex(trip.cuda(), N_ENT, N_REL, chunk_rel=CHUNK_REL, locality=True)
        assert idx.pos3 is not None and idx.rel.exact and idx.rel.n_fix == 1 and idx.rel.n_slots == 2
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


def run_head(ops, h, flavour, arena=None, idx=None):
    """One loss_head forward + backward on the GPU; returns the outputs and gradients (CPU float64)."""
    e32, w32, trip, y = problem(h)
    e, w = e32.cuda().requires_grad_(), w32.cuda().requires_grad_()
    b = torch.tensor(0.3, device='cuda', requires_grad=True)
    idx = make_index(ops, trip, flavour) if idx is None else idx
    if arena is not None:
        ops.DIRECT_GRAD[w.data_ptr()] = arena
    try:
        loss, pred, _, _ = ops.loss_head(e, None, None, w, None, b, None, None, y.cuda(), idx, REG, 0.0, 0.0, True)
        (loss * G_UP).backward()
    finally:
        ops.DIRECT_GRAD.pop(w.data_ptr(), None)
    torch.cuda.synchronize()
    return dict(loss=loss.detach().double().cpu(), pred=pred.detach().double().cpu(), g_e=e.grad.double().cpu(),
                g_w=None if arena is not None else w.grad.double().cpu(), g_b=b.grad.double().cpu())


def scores_of(ops, h, flavour, idx=None):
    """(loss, score) of ops.distmult_bce -- the entry that hands the scores out."""
    e32, w32, trip, y = problem(h)
    e, w = e32.cuda().requires_grad_(), w32.cuda().requires_grad_()
    idx = make_index(ops, trip, flavour) if idx is None else idx
    loss, score = ops.distmult_bce(e, w, torch.tensor(0.3, device='cuda'), y.cuda(), idx)
    return loss.detach().double().cpu(), score.detach().double().cpu()


def run_direct(ops, h, flavour, e32=None):
    """The two entry points called directly on NaN-filled outputs (non-accumulating); returns the raw device tensors."""
    e0, w32, trip, y = problem(h)
    idx = make_index(ops, trip, flavour)
    e, w, seg = (e0 if e32 is None else e32).cuda(), w32.cuda(), idx.rel
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
    n_part = (T + 15) // 16                 # red_blocks(381, 16) partial sums of the BCE terms
    return dict(score=score, delta=delta, g_w=g_w, d_out=d_out, dbias=dbias, pred=ws[:n_part].double().sum().cpu() / T,
                pos=None if idx.pos3 is None else idx.pos3.long().cpu())


def within(tag, got, ref, bound):
    ratio = float(((got - ref).abs() / bound).max())
    print(f'RATIO {tag} {ratio:.4f}')
    assert torch.isfinite(got).all(), f'{tag}: non-finite values'
    assert ratio <= 1.0, f'{tag}: |got - ref| is {ratio:.3f} of the bound'
    return ratio


def check_direct(tag, out, ref):
    within(f'{tag} scores', out['score'].double().cpu(), ref['score'], ref['b_score'])
    within(f'{tag} grad_w', out['g_w'].double().cpu(), ref['g_w'], ref['b_w'])
    within(f'{tag} grad_bias', out['dbias'].double().cpu()[0], ref['g_b'], ref['b_b'])
    within(f'{tag} predict_loss partials', out['pred'], ref['pred'], ref['b_pred'])
    assert torch.isfinite(out['d_out']).all() and torch.isfinite(out['delta']).all()
    delta = out['delta'].double().cpu()
    if out['pos'] is None:
        within(f'{tag} delta', delta, ref['delta'], ref['b_delta'])
    else:
        for k in (0, 1):
            within(f'{tag} delta (incidence side {k})', delta[out['pos'][:, k]], ref['delta'], ref['b_delta'])


@gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('h', WIDTHS)
def test_head_inside_the_float64_bounds(ops, monkeypatch, h, flavour):
    """Loss, predict_loss, entity / relation / bias gradient and the scores, through ops.loss_head and ops.distmult_bce."""
    names = record_calls(monkeypatch, ops)
    out = run_head(ops, h, flavour)
    assert 'gv_distmult_bce_fwd_grad' in names and 'gv_distmult_grad_finish' in names and 'gv_bce_grad' not in names
    ref = reference(h)
    tag = f'rows head h={h} {flavour}'
    within(f'{tag} loss', out['loss'], ref['loss'], ref['b_loss'])
    within(f'{tag} predict_loss', out['pred'], ref['pred'], ref['b_pred'])
    within(f'{tag} grad_z', out['g_e'], ref['g_e'], ref['b_e'])
    within(f'{tag} grad_w', out['g_w'], ref['g_w'], ref['b_w'])
    within(f'{tag} grad_bias', out['g_b'], ref['g_b'], ref['b_b'])
    empty = REL_COUNTS.index(0)          # the relation without a triplet: the regulariser's term alone
    term = G_UP * 2 * REG / (N_REL * h) * problem(h)[1][empty].double()
    within(f'{tag} empty relation row', out['g_w'][empty], term, 4 * U * term.abs())
    loss, score = scores_of(ops, h, flavour)
    within(f'rows scores h={h} {flavour}', score, ref['score'], ref['b_score'])
    within(f'rows distmult_bce loss h={h} {flavour}', loss, ref['pred'], ref['b_pred'])


@gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('h', [68, 200])
def test_relation_gradient_accumulates_into_a_prefilled_slot(ops, h, flavour):
    """ops.DIRECT_GRAD (the optimiser's gradient arena): the finishing launch adds into the slot, every row once -- the empty
    relation's and the split one's too."""
    before = torch.randn(N_REL, h, generator=torch.Generator().manual_seed(3))
    arena = before.cuda()
    run_head(ops, h, flavour, arena=arena)
    ref = reference(h)
    got = arena.double().cpu() - before.double()
    within(f'rows arena grad_w h={h} {flavour}', got, ref['g_w'], ref['b_w'] + U * (before.double().abs() + ref['g_w'].abs()))


@gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('h', WIDTHS)
def test_entry_points_write_every_row_of_nan_filled_buffers(ops, h, flavour):
    """Every score, every coefficient and every relation row -- the empty relation's, the short ones', the split one's -- is
    written and inside the bounds; a second run gives the same bits."""
    ref = reference(h)
    out = run_direct(ops, h, flavour)
    check_direct(f'rows direct h={h} {flavour}', out, ref)
    again = run_direct(ops, h, flavour)
    for key in ('score', 'delta', 'g_w', 'd_out', 'dbias'):
        assert torch.equal(out[key], again[key]), f'{key}: two runs differ'
    assert torch.equal(out['pred'], again['pred'])


@gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('h', [4, 68, 200])
def test_an_unreferenced_entity_row_of_nan_reaches_nothing(ops, h, flavour):
    """Entity 12 is in no triplet: with its embedding row NaN every output stays finite and equal to the clean run's bits -- a
    shadow row (or a lane of a group past h) reads only what its batch's triplets read."""
    e32 = problem(h)[0].clone()
    e32[12] = float('nan')
    out, clean = run_direct(ops, h, flavour, e32=e32), run_direct(ops, h, flavour)
    check_direct(f'rows nan-row h={h} {flavour}', out, reference(h))
    for key in ('score', 'delta', 'g_w', 'd_out', 'dbias'):
        assert torch.isfinite(out[key]).all() and torch.equal(out[key], clean[key]), key


@gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('h', WIDTHS)
def test_fused_against_the_separate_sweeps(ops, monkeypatch, h, flavour):
    """Same inputs down both paths (GV_DISTMULT_FUSED=0 is ops.DISTMULT_FUSED False): everything inside the sum of the two
    paths' bounds (twice the bound: both meet the same one)."""
    idx = make_index(ops, problem(h)[2], flavour)
    new = run_head(ops, h, flavour, idx=idx)
    new_scores = scores_of(ops, h, flavour, idx=idx)
    monkeypatch.setattr(ops, 'DISTMULT_FUSED', False)
    names = record_calls(monkeypatch, ops)
    old = run_head(ops, h, flavour, idx=idx)
    old_scores = scores_of(ops, h, flavour, idx=idx)
    assert 'gv_bce_grad' in names and 'gv_distmult_bce_fwd_grad' not in names
    ref = reference(h)
    for key, bound in (('loss', 'b_loss'), ('pred', 'b_pred'), ('g_e', 'b_e'), ('g_w', 'b_w'), ('g_b', 'b_b')):
        within(f'rows fused-vs-separate {key} h={h} {flavour}', new[key], old[key], 2 * ref[bound])
    within(f'rows fused-vs-separate scores h={h} {flavour}', new_scores[1], old_scores[1], 2 * ref['b_score'])
