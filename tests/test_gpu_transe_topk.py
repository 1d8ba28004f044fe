"""TransE top-k link prediction on the GPU (gv_transe_topk / ops.transe_topk / transe.predict_topk) against the rule stated on
materialised distances: the same te_tile() distances (ops.transe_distances), ordered by transe.topk_from_distances.  pytest -m gpu."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def transe():
    from gcn_vae_amd import transe as _transe
    return _transe


def _lists(m, v, gen, kinds):
    """Per-query sorted unique entity lists of the given kinds, packed into (lo, hi, ent)."""
    out = []
    for i in range(m):
        k = kinds[i % len(kinds)]
        if k == 'empty':
            e = np.zeros(0, dtype=np.int64)
        elif k == 'few':
            e = np.unique(torch.randint(0, v, (5,), generator=gen).numpy())
        elif k == 'straddle':          # across a 64-column tile boundary
            c = 64 * int(torch.randint(1, max(2, v // 64), (1,), generator=gen))
            e = np.arange(max(0, c - 3), min(v, c + 3))
        elif k == 'window':            # one whole 64-column window
            c = 64 * int(torch.randint(0, max(1, v // 64), (1,), generator=gen))
            e = np.arange(c, min(v, c + 64))
        elif k == 'long':              # all entities but two: fewer than k candidates left
            e = np.sort(torch.randperm(v, generator=gen)[:max(0, v - 2)].numpy())
        elif k == 'shared':            # placeholder: pointed at row 1's range below
            e = np.zeros(0, dtype=np.int64)
        else:
            raise ValueError(k)
        out.append(e)
    lens = np.array([len(e) for e in out], dtype=np.int64)
    hi = np.cumsum(lens)
    lo = hi - lens
    if 'shared' in kinds:              # rows of kind 'shared' all point at row 1's range
        for i in range(m):
            if kinds[i % len(kinds)] == 'shared' and m > 1:
                lo[i], hi[i] = lo[1], hi[1]
    ent = np.concatenate(out) if lens.sum() else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(ent).cuda()


KINDS = ['empty', 'few', 'straddle', 'window', 'long', 'shared', 'few']


def _expected(ops, transe, q, en, k, p, lo=None, hi=None, ent=None):
    return transe.topk_from_distances(ops.transe_distances(q, en, p), k, lo, hi, ent)


def _same(a, b):
    """Bit-for-bit equality of (ids, distances) pairs."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# every m of {1, 37, 64, 129, 300}, v of {1, 7, 90, 777, 3001, 14541}, dim of {1, 5, 32, 37, 200, 512} and k of {1, 10, 64, 128}
SHAPES = [(1, 1, 1, 1), (37, 7, 5, 10), (64, 90, 32, 128), (129, 777, 200, 64), (300, 3001, 37, 10), (300, 14541, 200, 10),
          (37, 14541, 512, 128), (64, 3001, 512, 64), (129, 90, 1, 1), (1, 777, 37, 128), (129, 3001, 5, 1), (64, 7, 32, 64)]


@pytest.mark.parametrize('p', [1, 2])
@pytest.mark.parametrize('m,v,dim,k', SHAPES)
def test_topk_equals_the_definition(ops, transe, m, v, dim, k, p):
    gen = torch.Generator().manual_seed(m * 7 + v + dim + k + p)
    en = (torch.randn(v, dim, generator=gen) * 0.5).cuda()
    q = torch.randn(m, dim, generator=gen).cuda()
    got = ops.transe_topk(q, en, k, p)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (m, k) and got[1].shape == (m, k)
    assert _same(got, _expected(ops, transe, q, en, k, p))
    lo, hi, ent = _lists(m, v, gen, KINDS)
    got = ops.transe_topk(q, en, k, p, lo, hi, ent)
    assert _same(got, _expected(ops, transe, q, en, k, p, lo, hi, ent))
    if v < k:
        assert bool((got[0][:, v:] == -1).all()) and bool((got[1][:, v:] == float('inf')).all())
    assert ops.transe_topk(q[:0], en, k, p)[0].shape == (0, k)


@pytest.mark.parametrize('p', [1, 2])
def test_ties_nan_inf_and_zero(ops, transe, p):
    dim, v = 8, 1300                                         # 21 column tiles: two spans
    gen = torch.Generator().manual_seed(p)
    en = torch.randn(v, dim, generator=gen).cuda()
    for j in (7, 70, 130, 200, 299, 1000, 1299):             # exact ties across tiles and spans
        en[j] = en[3]
    en[10] = float('nan')
    en[250] = float('nan')
    en[40, 0] = float('inf')
    en[41, 0] = float('-inf')
    q = torch.stack([en[3], -en[3], en[5], en[6]]).clone()   # q[0] equals an entity (and its duplicates): distance +0
    q[2, 0] = float('inf')                                   # inf - inf: NaN against entity 40, +inf against the others
    for k in (1, 10, 64, 128):
        got = ops.transe_topk(q, en, k, p)
        want = _expected(ops, transe, q, en, k, p)
        assert torch.equal(got[0], want[0])
        assert _same(got, want)
    ids, dist = ops.transe_topk(q, en, 128, p)
    assert ids[0, :8].tolist() == [3, 7, 70, 130, 200, 299, 1000, 1299]       # the exact ties, by id across tiles and spans
    assert dist[0, :8].view(torch.int32).tolist() == [0] * 8                   # +0
    assert all(len(set(row)) == 128 for row in ids.tolist())
    # +inf before NaN, NaN by id, every NaN the one quiet NaN
    ids, dist = ops.transe_topk(q, en, 128, p, *_all_but(v, [5, 10, 40, 41, 250, 900]))
    assert ids[3, :6].tolist()[2:] == [40, 41, 10, 250] and set(ids[3, :2].tolist()) == {5, 900}
    assert dist[3, 2:4].tolist() == [float('inf')] * 2 and dist[3, 4:6].view(torch.int32).tolist() == [0x7fc00000] * 2
    assert ids[3, 6:].tolist() == [-1] * 122 and bool((dist[3, 6:] == float('inf')).all())
    assert ids[2, :6].tolist() == [5, 41, 900, 10, 40, 250]                    # q[2]: +inf to 5, 41, 900; NaN to 10, 40, 250
    # an all-equal table: ids in order, padded past v
    same = torch.ones(100, dim, device=DEV)
    ids, dist = ops.transe_topk(torch.ones(1, dim, device=DEV), same, 128, p)
    assert ids[0].tolist() == list(range(100)) + [-1] * 28
    assert dist[0, :100].view(torch.int32).tolist() == [0] * 100 and bool((dist[0, 100:] == float('inf')).all())


def _all_but(v, keep):
    """A filter that lists every entity except ``keep``, the same for each of 4 rows."""
    ent = torch.tensor([j for j in range(v) if j not in keep], device=DEV)
    return (torch.zeros(4, dtype=torch.long, device=DEV), torch.full((4,), ent.numel(), dtype=torch.long, device=DEV), ent)


def test_two_runs_are_bit_identical(ops):
    gen = torch.Generator().manual_seed(3)
    en, q = torch.randn(5000, 100, generator=gen).cuda(), torch.randn(300, 100, generator=gen).cuda()
    lo, hi, ent = _lists(300, 5000, gen, KINDS)
    for p in (1, 2):
        a = ops.transe_topk(q, en, 100, p, lo, hi, ent)
        b = ops.transe_topk(q, en, 100, p, lo, hi, ent)
        assert _same(a, b)


@pytest.mark.parametrize('p', [1, 2])
def test_crosscheck_with_the_ranker(ops, transe, p):
    """Where the first k + 1 filtered distances of a row are tie-free (judged on the materialised distances), the entity at
    position p has filtered rank p from gv_transe_rank_filtered with the same filter."""
    gen = torch.Generator().manual_seed(11 + p)
    m, v, dim, k = 150, 2500, 64, 40
    en = torch.randn(v, dim, generator=gen).cuda()
    q = torch.randn(m, dim, generator=gen).cuda()
    lo, hi, ent = _lists(m, v, gen, ['empty', 'few', 'straddle', 'window', 'few'])
    _, d_ref = _expected(ops, transe, q, en, k + 1, p, lo, hi, ent)
    ok = (d_ref[:, 1:] > d_ref[:, :-1]).all(1)                # a tie could only sit next to its equal in the order
    assert int(ok.sum()) >= m * 0.8
    ids, _ = ops.transe_topk(q, en, k + 1, p, lo, hi, ent)
    for pos in range(k):
        _, filt = ops.transe_rank_filtered(q[ok], en, ids[ok, pos], p, lo[ok], hi[ok], ent)
        assert bool((filt == pos).all())


def _fb_split():
    from gcn_vae_amd import data
    return data.load_data('FB15k-237-synthetic')


def test_hits_at_10_equals_membership_in_the_top_10(transe):
    """Filtered Hits@10 from rank_transe equals the share of queries whose target is among predict_topk(k=10) with the same
    filter, in both directions (queries whose target is not in their own filter list)."""
    from gcn_vae_amd import ranking
    kg = _fb_split()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, device=DEV)
    torch.manual_seed(6)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=200).to(DEV)
    tr = transe.DeviceTrainer(model, kg.train, device=DEV)
    for _ in range(2):
        tr.epoch()
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    trip = torch.from_numpy(np.asarray(kg.test)).long().to(DEV)
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    n = trip.shape[0]
    _, filt = transe.rank_transe(ent, rel, trip, model.p_norm, model.norm_flag, fi)        # head queries, then tail queries
    for a, b, d, ranks in ((o, s, 's', filt[:n]), (s, o, 'o', filt[n:])):
        lo, hi = fi.lookup(a, r, d)
        listed = ranking._listed_mask(lo, hi, fi.entities(d), n, kg.num_nodes, DEV)[torch.arange(n, device=DEV), b]
        keep = ~listed
        ids, _ = transe.predict_topk(model, a, r, 10, direction=d, filter_index=fi)
        hit_rank = ((ranks[keep] + 1) <= 10).float().mean().item()
        hit_topk = (ids[keep] == b[keep].view(-1, 1)).any(1).float().mean().item()
        assert hit_rank == hit_topk and hit_rank > 0


@pytest.mark.parametrize('p', [1, 2])
def test_full_fb15k237_size_against_the_unfused_path(transe, p):
    """40 932 queries (both directions of the FB15k-237-sized test split) x 14 541 entities, dim 200, k = 10, filtered with the
    synthetic dataset's train + valid + test triplets: the fused path equals the materialised one exactly."""
    from gcn_vae_amd import ranking
    kg = _fb_split()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device=DEV)
    torch.manual_seed(5)
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=200, p_norm=p).to(DEV)
    trip = torch.from_numpy(np.asarray(kg.test)).long().to(DEV)
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    total = 0
    for a_, d in ((s, 'o'), (o, 's')):
        got = transe.predict_topk(model, a_, r, 10, direction=d, filter_index=fi)
        want = transe.predict_topk_unfused(model, a_, r, 10, direction=d, filter_index=fi)
        assert _same(got, want)
        total += got[0].shape[0]
    assert total == 40932


def test_cli_writes_the_filtered_predictions(transe, tmp_path):
    from gcn_vae_amd import data, ranking
    spec = 'synthetic:300:6:4000:200:200:1'
    env = dict(os.environ, PYTHONPATH=ROOT)
    ck, out = str(tmp_path / 'transe.ckpt'), str(tmp_path / 'pred.tsv')
    base = [sys.executable, '-m', 'gcn_vae_amd.transe', '-d', spec, '--gpu', '0', '--seed', '0', '--dim', '32', '--nbatches', '10',
            '--neg-ent', '5', '--filtered-eval', '--checkpoint', ck]

    def run(extra):
        r = subprocess.run(['timeout', '-k', '10', '600'] + base + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout

    trained = run(['--train-times', '2', '--predict-topk', '5', '--predict-out', out])
    assert len(re.findall(r'Epoch \d+ \| loss', trained)) == 2
    kg = data.load_data(spec)
    n_test = len(kg.test)
    assert f'wrote {2 * n_test * 5} predictions' in trained
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert len(rows) == 2 * n_test * 5
    model = transe.TransE(kg.num_nodes, kg.num_rels, dim=32)
    model.load_checkpoint(ck)
    model = model.to(DEV)
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device=DEV)
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    test = torch.as_tensor(np.asarray(kg.test), dtype=torch.long)
    for j, (d, col) in enumerate((('o', 0), ('s', 2))):
        a, r = test[:, col], test[:, 1]
        ids, dist = transe.predict_topk(model, a, r, 5, direction=d, filter_index=fi)
        block = rows[j * n_test * 5:(j + 1) * n_test * 5]
        assert all(x[0] == d for x in block)
        assert [int(x[4]) for x in block] == ids.reshape(-1).tolist()
        assert [int(x[3]) for x in block] == list(range(5)) * n_test
        assert [int(x[1]) for x in block[::5]] == a.tolist() and [int(x[2]) for x in block[::5]] == r.tolist()
        # nine significant digits round-trip a float32
        assert np.array_equal(np.array([float(x[5]) for x in block], dtype=np.float32), dist.reshape(-1).cpu().numpy())
        for x in block:                                     # new facts only
            qa, rel, e = int(x[1]), int(x[2]), int(x[4])
            assert e == -1 or ((qa, rel, e) if d == 'o' else (e, rel, qa)) not in known
    # without the flag: no file, and the output of a flagged run less its last line
    os.remove(out)
    plain = run(['--test-mode'])
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / 'transe_predictions.tsv'))
    flagged = run(['--test-mode', '--predict-topk', '5', '--predict-out', out])
    assert os.path.exists(out) and [line.rstrip('\n').split('\t') for line in open(out)] == rows
    lines = flagged.splitlines()
    assert lines[-1].startswith('wrote ') and lines[:-1] == plain.splitlines() and 'MRR (filtered)' in plain


def test_bad_arguments_raise_before_any_launch(ops):
    gen = torch.Generator().manual_seed(0)
    q, en = torch.randn(6, 16, generator=gen).cuda(), torch.randn(40, 16, generator=gen).cuda()
    lo, hi, ent = _lists(6, 40, gen, ['few'])
    for k in (0, 129):
        with pytest.raises(ValueError, match='k must lie'):
            ops.transe_topk(q, en, k, 1)
    with pytest.raises(ValueError, match='p_norm'):
        ops.transe_topk(q, en, 5, 3)
    wide = torch.zeros(4, 513, device=DEV)
    with pytest.raises(ValueError, match='dim'):
        ops.transe_topk(wide, wide, 5, 1)
    with pytest.raises(ValueError, match='contiguous'):
        ops.transe_topk(q[:, ::2], en[:, ::2], 5, 1)
    with pytest.raises(ValueError, match='contiguous'):
        ops.transe_topk(q, en.t().contiguous().t(), 5, 1)
    with pytest.raises(ValueError, match='width'):
        ops.transe_topk(q, en[:, :8].contiguous(), 5, 1)
    for f in ((lo, None, None), (lo, hi, None), (None, hi, ent), (None, None, ent)):
        with pytest.raises(ValueError, match='together'):
            ops.transe_topk(q, en, 5, 1, *f)
    with pytest.raises(ValueError, match='one filter range'):
        ops.transe_topk(q, en, 5, 1, lo[:-1], hi[:-1], ent)
    with pytest.raises(ValueError, match='filter ranges'):
        ops.transe_topk(q, en, 5, 1, lo, hi + 1000, ent)
    with pytest.raises(ValueError, match='entity ids'):
        ops.transe_topk(q, en, 5, 1, lo, hi, ent + 40)
    with pytest.raises(RuntimeError):
        ops.transe_topk(q.cpu(), en.cpu(), 5, 1)
