"""TransE on the device: the fused step against the reference fixture (tolerances from a float64 recomputation), the hinge
tie and zero row, determinism (run to run, eager vs captured), the sampler's rules, the fused ranker against sort_and_rank on
the materialised distances, and a seeded CLI run."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gcn_vae_amd import ops, transe
from gcn_vae_amd.ranking import FilterIndex, sort_and_rank

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'transe.npz'))
CASES = ['p1_norm', 'p1_raw', 'p2_norm', 'p2_raw', 'adv', 'regul', 'tie']
DEV = torch.device('cuda', 0)


def case(tag):
    cfg = GOLD[f'{tag}.cfg']
    return dict(ent=torch.from_numpy(GOLD[f'{tag}.ent']), rel=torch.from_numpy(GOLD[f'{tag}.rel']),
                bh=torch.from_numpy(GOLD[f'{tag}.bh']), br=torch.from_numpy(GOLD[f'{tag}.br']), bt=torch.from_numpy(GOLD[f'{tag}.bt']),
                B=int(cfg[0]), K=int(cfg[1]), p=int(cfg[2]), nf=bool(cfg[3]), margin=float(cfg[4]), adv=float(cfg[5]) or None,
                regul=float(cfg[6]), lr=float(cfg[7]))


def device_steps(c, steps, ent=None, rel=None):
    """(score, loss, g_ent, g_rel) of the first step and the tables after ``steps`` SGD steps, all on the device path."""
    ent = (c['ent'] if ent is None else ent).to(DEV).contiguous().clone()
    rel = (c['rel'] if rel is None else rel).to(DEV).contiguous().clone()
    B, K = c['B'], c['K']
    bh, br, bt = (c[k].to(device=DEV, dtype=torch.int32).contiguous() for k in ('bh', 'br', 'bt'))
    order = ops.TransEOrder((2 + K) * B, ent.shape[0], B, rel.shape[0], DEV)
    occ = torch.empty((2 + K) * B, dtype=torch.int32, device=DEV)
    score = torch.empty(B * (1 + K), device=DEV)
    loss = torch.zeros(1, device=DEV)
    first = None
    for s in range(steps):
        g_ent, g_rel, part = ops.transe_step(ent, rel, bh, br, bt, B, K, c['p'], c['nf'], c['margin'], c['adv'], c['regul'],
                                             score=score, occ_ent=occ)
        parts = order.build(occ, br[:B])
        if s == 0:
            ge, gr = torch.zeros_like(ent), torch.zeros_like(rel)       # p += -(-1) * g on zero tables: the summed gradient
            ops.transe_apply(ge, gr, g_ent, g_rel, parts, -1.0, part, c['margin'], loss)
            first = (score.clone(), loss.clone(), ge, gr)
        ops.transe_apply(ent, rel, g_ent, g_rel, parts, c['lr'], part, c['margin'], loss)
    torch.cuda.synchronize()
    return first, ent, rel


def f64_reference(c, steps):
    ent, rel = c['ent'].double(), c['rel'].double()
    first = None
    for s in range(steps):
        out = transe.step_unfused(ent, rel, c['bh'], c['br'], c['bt'], c['B'], c['p'], c['nf'], c['margin'], c['adv'], c['regul'])
        if s == 0:
            first = out
        ent, rel = ent - c['lr'] * out[2], rel - c['lr'] * out[3]
    return first, ent, rel


def bound_of(fix, f64, slack):
    """4 |fixture - float64| + slack * (max |float64| of the element's ROW; of the whole tensor below 2-D).  Per row: under
    norm_flag the all-zero entity row gets gy / 1e-12 (~1e11), and a tensor-wide scale would let every other row pass unchecked."""
    scale = f64.abs().amax(dim=-1, keepdim=True) if f64.dim() >= 2 else f64.abs().max()
    return 4 * (fix - f64).abs() + slack * (scale + 1e-30)


def assert_bound(got, fix, f64, what, slack=1e-5):
    """|device - fixture| within bound_of (float32 work vs float32 reference rounding)."""
    got, fix, f64 = got.detach().cpu().double(), torch.as_tensor(np.asarray(fix)).double(), f64.detach().cpu().double()
    bound = bound_of(fix, f64, slack)
    err = (got - fix).abs()
    assert bool((err <= bound).all()), f'{what}: worst excess {float((err - bound).max()):.3e} (max err {float(err.max()):.3e})'


@pytest.mark.parametrize('tag', CASES)
def test_step_matches_fixture(tag):
    c = case(tag)
    (score, loss, ge, gr), ent3, rel3 = device_steps(c, 3)
    (s64, l64, ge64, gr64), ent64, rel64 = f64_reference(c, 3)
    assert_bound(score, GOLD[f'{tag}.score'], s64, 'score')
    assert_bound(loss.reshape(()), GOLD[f'{tag}.loss'], l64, 'loss')
    assert_bound(ge, GOLD[f'{tag}.g_ent'], ge64, 'g_ent')
    assert_bound(gr, GOLD[f'{tag}.g_rel'], gr64, 'g_rel')
    assert_bound(ent3, GOLD[f'{tag}.ent3'], ent64, 'ent after 3 steps', slack=1e-4)
    assert_bound(rel3, GOLD[f'{tag}.rel3'], rel64, 'rel after 3 steps', slack=1e-4)


def test_hinge_tie_and_zero_difference_exact():
    c = case('tie')
    (score, loss, ge, gr), _, _ = device_steps(c, 1)
    (_, l64, ge64, gr64), _, _ = f64_reference(c, 1)
    # dyadic tables: every score of this case is exact in float32, so the device scores are the fixture's bits, the pair
    # (0, 0) ties the hinge exactly and positive 1 has a zero difference
    assert torch.equal(score.cpu(), torch.from_numpy(GOLD['tie.score']))
    assert float(score[0] - score[c['B']]) == -c['margin'] and float(score[1]) == 0.0
    # the half gradient at the tie and the zero norm gradient at the zero difference (float64 takes the same branches)
    assert_bound(ge, GOLD['tie.g_ent'], ge64, 'tie g_ent', slack=1e-6)
    assert_bound(gr, GOLD['tie.g_rel'], gr64, 'tie g_rel', slack=1e-6)
    assert_bound(loss.reshape(()), GOLD['tie.loss'], l64, 'tie loss', slack=1e-6)


@pytest.mark.parametrize('tag', ['p1_norm', 'adv'])
def test_bound_rejects_a_perturbed_entity_gradient(tag):
    """The parity bound compares the ordinary entity rows next to the ~1e11 zero row: a 1 % change of one of them fails."""
    c = case(tag)
    (_, _, ge, _), _, _ = device_steps(c, 1)
    (_, _, ge64, _), _, _ = f64_reference(c, 1)
    assert_bound(ge, GOLD[f'{tag}.g_ent'], ge64, 'g_ent')
    row = int(ge[1:].abs().amax(1).argmax()) + 1
    bad = ge.clone()
    bad[row] *= 1.01
    with pytest.raises(AssertionError):
        assert_bound(bad, GOLD[f'{tag}.g_ent'], ge64, 'perturbed g_ent')


def test_zero_row_gradient_matches_fixture():
    for tag in ('p1_norm', 'p2_norm', 'p1_raw'):
        c = case(tag)
        (_, _, ge, _), _, _ = device_steps(c, 1)
        (_, _, ge64, _), _, _ = f64_reference(c, 1)
        assert_bound(ge[0], GOLD[f'{tag}.g_ent'][0], ge64[0], f'{tag} zero row')


def small_trainer(seed=0, graph=False, **kw):
    from gcn_vae_amd.data import synthetic_kg
    data = synthetic_kg(300, 6, 4000, 200, 200, seed=1)
    torch.manual_seed(seed)
    model = transe.TransE(data.num_nodes, data.num_rels, dim=kw.pop('dim', 48), p_norm=kw.pop('p_norm', 1)).to(DEV)
    tr = transe.DeviceTrainer(model, data.train, nbatches=kw.pop('nbatches', 10), neg_ent=kw.pop('neg_ent', 5), device=DEV, **kw)
    tr.rng.state.copy_(torch.tensor([1234, 0], dtype=torch.int64))
    tr.rng._seed = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF
    tr.stream_id = 4242                          # a fixed draw stream: the trainers below sample the same batches
    if graph:
        tr.capture()
    return data, model, tr


def test_step_bit_identical_runs_and_eager_vs_captured():
    _, m1, t1 = small_trainer()
    start = m1.ent_embeddings.weight.detach().clone()
    for _ in range(6):
        t1.step()
    _, m2, t2 = small_trainer()
    for _ in range(6):
        t2.step()
    _, m3, t3 = small_trainer(graph=True)        # capture restores the tables and the RNG after its warm-up step
    assert torch.equal(m3.ent_embeddings.weight, start)
    for _ in range(6):
        t3.step()
    torch.cuda.synchronize()
    for m in (m2, m3):
        assert torch.equal(m.ent_embeddings.weight, m1.ent_embeddings.weight)
        assert torch.equal(m.rel_embeddings.weight, m1.rel_embeddings.weight)
    assert not torch.equal(m1.ent_embeddings.weight, start)


def test_untouched_rows_unchanged():
    data, m, t = small_trainer(nbatches=400, neg_ent=2)      # 10 positives a step: most rows stay untouched
    start = m.ent_embeddings.weight.detach().clone()
    seen = torch.zeros(data.num_nodes, dtype=torch.bool, device=DEV)
    for _ in range(2):
        t.step()
        seen[t.occ_ent.long()] = True
    torch.cuda.synchronize()
    untouched = ~seen
    assert int(untouched.sum()) > 0
    assert torch.equal(m.ent_embeddings.weight[untouched], start[untouched])


def test_sampler_rules_and_host_mapping():
    from gcn_vae_amd.data import synthetic_kg
    data = synthetic_kg(400, 5, 20000, seed=3)
    train = data.train
    tf = transe.TrainFilter(train, data.num_nodes, data.num_rels, DEV)
    p_head = transe.bern_head_prob(train, data.num_rels).to(DEV)
    rng = ops.DeviceRNG(DEV)
    rng.state.copy_(torch.tensor([99, 7], dtype=torch.int64))
    tr32 = torch.as_tensor(train, dtype=torch.int32).to(DEV).contiguous()
    B, K = 20000, 4
    draws = torch.empty(B * (K + 2), dtype=torch.int32, device=DEV)
    bh, br, bt = ops.transe_sample(rng.state, 77, tr32, data.num_nodes, B, K, p_head, tf.tuple(), draws=draws)
    bh, br, bt = bh.cpu().numpy(), br.cpu().numpy(), bt.cpu().numpy()
    d = draws.cpu().numpy().view(np.uint32).reshape(B, K + 2)
    hh, hr, ht = transe.sample_from_draws(d, train, data.num_nodes, B, K, p_head.cpu(), tf)
    assert (hh == bh).all() and (hr == br).all() and (ht == bt).all()
    known = set(map(tuple, np.asarray(train).tolist()))
    ph, pr, pt = bh[:B], br[:B], bt[:B]
    assert all((int(a), int(b), int(c)) in known for a, b, c in zip(ph, pr, pt))
    head_count = np.zeros(data.num_rels)
    total = np.zeros(data.num_rels)
    for j in range(K):
        nh, nr, nt = bh[B * (j + 1):B * (j + 2)], br[B * (j + 1):B * (j + 2)], bt[B * (j + 1):B * (j + 2)]
        assert (nr == pr).all()
        changed_h, changed_t = nh != ph, nt != pt
        assert not (changed_h & changed_t).any() and (changed_h | changed_t).all()      # exactly one side replaced
        assert not any((int(a), int(b), int(c)) in known for a, b, c in zip(nh, nr, nt))
        if j == 0:
            np.add.at(head_count, pr, changed_h)
            np.add.at(total, pr, 1)
    p = p_head.cpu().numpy().astype(np.float64)
    for r in range(data.num_rels):
        if total[r] >= 200:       # 5-sigma binomial bound around tph / (tph + hpt)
            share = head_count[r] / total[r]
            assert abs(share - p[r]) <= 5 * np.sqrt(p[r] * (1 - p[r]) / total[r]) + 1.0 / total[r], (r, share, p[r])


def ranker_case(p_norm, seed):
    g = torch.Generator().manual_seed(seed)
    v, dim, m = 300, 40, 200
    ent = torch.randn(v, dim, generator=g)
    ent[10:20] = ent[0:10]                          # duplicated rows: exact ties
    ent[25] = float('nan')                          # a NaN row
    rel = torch.randn(7, dim, generator=g)
    trip = torch.stack([torch.randint(0, v, (m,), generator=g), torch.randint(0, 7, (m,), generator=g),
                        torch.randint(0, v, (m,), generator=g)], 1)
    trip[:5, 2] = trip[5:10, 2] = 3                 # shared targets; target 25 is NaN for a few queries
    trip[10:13, 0] = 25
    extra = torch.stack([trip[:, 0], trip[:, 1], torch.randint(0, v, (m,), generator=g)], 1)
    return ent.to(DEV), rel.to(DEV), trip, FilterIndex(v, 7, trip, extra, device=DEV)


@pytest.mark.parametrize('p_norm', [1, 2])
@pytest.mark.parametrize('head', [False, True])
def test_fused_ranks_equal_sort_and_rank_on_distances(p_norm, head):
    ent, rel, trip, fi = ranker_case(p_norm, 5 + p_norm)
    s, r, o = (trip[:, i].to(DEV) for i in range(3))
    a, b, d = (o, s, 's') if head else (s, o, 'o')
    en = ops.transe_queries(ent)
    q = ops.transe_queries(ent, rel, a, r, head=head)
    dist = ops.transe_distances(q, en, p_norm)
    lo, hi = fi.lookup(a, r, d)
    raw, filt = ops.transe_rank_filtered(q, en, b, p_norm, lo, hi, fi.entities(d, DEV))
    assert torch.equal(raw, sort_and_rank(-dist, b))
    from gcn_vae_amd.ranking import _listed_mask
    listed = _listed_mask(lo, hi, fi.entities(d), q.shape[0], en.shape[0], DEV)
    sc, tg = -dist, -dist.gather(1, b.view(-1, 1))
    keep = ~listed
    keep[torch.arange(q.shape[0], device=DEV), b] = False
    ref_f = ((~(sc <= tg)) & keep).sum(1).float() + 0.5 * ((sc == tg) & keep).sum(1).float()
    assert torch.equal(filt, ref_f)
    assert bool((filt <= raw).all())
    # distances within a float64 bound of the same formula, queries and table formed in float64 from the HOST tables (the
    # device's normalised queries are part of what is checked)
    e64, r64 = F.normalize(ent.cpu().double(), 2, -1), F.normalize(rel.cpu().double(), 2, -1)
    q64 = e64[a.cpu()] - r64[r.cpu()] if head else e64[a.cpu()] + r64[r.cpu()]
    d64 = torch.cdist(q64, e64, p=p_norm, compute_mode='donot_use_mm_for_euclid_dist')
    fin = torch.isfinite(d64)
    assert int(fin.sum()) > 0.9 * fin.numel()
    assert bool(((dist.cpu().double() - d64).abs()[fin] <= 1e-5 * (d64[fin] + 1)).all())


def test_full_size_fused_agrees_with_unfused():
    from gcn_vae_amd.data import load_data
    data = load_data('FB15k-237-synthetic')
    torch.manual_seed(0)
    model = transe.TransE(data.num_nodes, data.num_rels, dim=200).to(DEV)
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=DEV)
    sub = torch.as_tensor(np.asarray(data.test)[:256], dtype=torch.long)
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    rf, ff = transe.rank_transe(ent, rel, sub, 1, True, fi)
    ru, fu = transe.rank_transe_unfused(ent, rel, sub, 1, True, fi)
    # different normalisation / summation rounding: ranks may move by near-ties only
    assert float((rf - ru).abs().mean()) < 0.5 and float((ff - fu).abs().mean()) < 0.5
    assert abs(float((1 / (rf + 1)).mean() - (1 / (ru + 1)).mean())) < 1e-3


def test_training_lowers_loss_and_raises_train_mrr():
    data, model, tr = small_trainer(dim=32, nbatches=10, neg_ent=5)
    sub = np.asarray(data.train)[:300]
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, device=DEV)
    before = transe.evaluate(model, sub, fi, verbose=False)['mrr_filtered']
    losses = [tr.epoch() for _ in range(15)]
    after = transe.evaluate(model, sub, fi, verbose=False)['mrr_filtered']
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert after > before + 0.02, (before, after)


def test_cli_seeded_run_and_test_mode(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    ck = str(tmp_path / 'transe.ckpt')
    base = [sys.executable, '-m', 'gcn_vae_amd.transe', '-d', 'synthetic:300:6:4000:200:200:1', '--gpu', '0', '--seed', '0',
            '--dim', '32', '--nbatches', '10', '--neg-ent', '5', '--filtered-eval', '--checkpoint', ck]
    r = subprocess.run(['timeout', '-k', '10', '600'] + base + ['--train-times', '5', '--graph-step'], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(x) for x in re.findall(r'Epoch \d+ \| loss: ([0-9.eE+-]+)', r.stdout)]
    assert len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert 'MRR (filtered)' in r.stdout and 'Hits (raw) @ 10' in r.stdout
    sd = torch.load(ck, map_location='cpu')
    assert list(sd.keys()) == [str(k) for k in GOLD['state_keys']]
    r2 = subprocess.run(['timeout', '-k', '10', '600'] + base + ['--test-mode'], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    last = lambda out: re.findall(r'MRR \(filtered\): ([0-9.]+)', out)[-1]  # noqa: E731
    assert last(r2.stdout) == last(r.stdout)


def test_ops_reject_bad_arguments_before_launch():
    c = case('p1_norm')
    ent, rel = c['ent'].to(DEV).contiguous(), c['rel'].to(DEV).contiguous()
    B, K = c['B'], c['K']
    bh, br, bt = (c[k].to(device=DEV, dtype=torch.int32).contiguous() for k in ('bh', 'br', 'bt'))
    bad = bt.clone()
    bad[-1] = ent.shape[0]
    with pytest.raises(ValueError, match='bt'):
        ops.transe_step(ent, rel, bh, br, bad, B, K, 1, True, 5.0)
    g_ent, g_rel, part = ops.transe_step(ent, rel, bh, br, bt, B, K, 1, True, 5.0)
    order = ops.TransEOrder((2 + K) * B, ent.shape[0], B, rel.shape[0], DEV)
    loss = torch.zeros(1, device=DEV)
    with pytest.raises(ValueError, match='g_ent'):
        ops.transe_apply(ent, rel, g_ent[:-1], g_rel, order.parts, 1.0, part, 5.0, loss)
    with pytest.raises(ValueError, match='orderings'):
        ops.transe_apply(ent[:-1].contiguous(), rel, g_ent, g_rel, order.parts, 1.0, part, 5.0, loss)
    with pytest.raises(TypeError):
        ops.transe_apply(ent, rel, g_ent, g_rel, order.parts, 1.0, part, 5.0, loss, torch.zeros(1, device=DEV))
    train = torch.tensor([[0, 0, 1], [2, 3, 4]], dtype=torch.int32, device=DEV)
    rng = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match='p_head'):
        ops.transe_sample(rng, 1, train, 12, 2, 1, p_head=torch.full((2,), 0.5, device=DEV))
    with pytest.raises(ValueError, match='train'):
        ops.transe_sample(rng, 1, train, 3, 2, 1)


def test_evaluate_reports_filtered_only_with_a_filter(capsys):
    data, model, _ = small_trainer(dim=16)
    out = transe.evaluate(model, np.asarray(data.test)[:50])
    printed = capsys.readouterr().out
    assert 'mrr_filtered' not in out and 'filtered' not in printed and 'MRR (raw)' in printed
    fi = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=DEV)
    out = transe.evaluate(model, np.asarray(data.test)[:50], fi)
    assert 'MRR (filtered)' in capsys.readouterr().out and out['mrr_filtered'] >= out['mrr_raw']
