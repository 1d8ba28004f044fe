"""Top-k link prediction on the GPU (gv_topk_scores / ops.topk_scores / ranking.predict_topk) against the rule stated on
materialised logits: the same f32 MFMA product (ops.gemm), ordered by ranking.topk_from_scores.  pytest -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


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


def _expected(ops, q, emb, k, bias=None, lo=None, hi=None, ent=None):
    from gcn_vae_amd import ranking
    score = ops.gemm(q, emb, trans_b=True, precision='f32')
    if bias is not None:
        score = score + bias
    return ranking.topk_from_scores(score, k, lo, hi, ent)


def _same(a, b):
    """Bit-for-bit equality of (ids, logits) pairs."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


KINDS = ['empty', 'few', 'straddle', 'window', 'long', 'shared', 'few']


@pytest.mark.parametrize('m,v,h,k,flp', [(64, 128, 16, 10, None), (37, 1000, 37, 1, 0.25), (129, 777, 200, 64, None),
                                         (70, 5000, 37, 100, -1.5), (5, 90, 8, 128, None), (200, 3001, 200, 128, 3.0),
                                         (3, 7, 5, 10, None), (1, 1, 1, 1, 0.5), (300, 14541, 200, 10, None)])
def test_topk_equals_the_definition(ops, m, v, h, k, flp):
    gen = torch.Generator().manual_seed(m * 7 + v + h + k)
    emb = (torch.randn(v, h, generator=gen) * 0.5).cuda()
    q = torch.randn(m, h, generator=gen).cuda()
    bias = None if flp is None else torch.tensor(flp, device='cuda')
    got = ops.topk_scores(q, emb, k, bias)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[0].shape == (m, k)
    assert _same(got, _expected(ops, q, emb, k, bias))
    lo, hi, ent = _lists(m, v, gen, KINDS)
    got = ops.topk_scores(q, emb, k, bias, lo, hi, ent)
    assert _same(got, _expected(ops, q, emb, k, bias, lo, hi, ent))
    if v < k:
        assert bool((got[0][:, v:] == -1).all()) and bool((got[1][:, v:] == float('-inf')).all())


def test_row_and_width_stride(ops):
    gen = torch.Generator().manual_seed(9)
    base_q, base_e = torch.randn(90, 50, generator=gen).cuda(), torch.randn(300, 50, generator=gen).cuda()
    q, emb = base_q[::2, 3:40], base_e[:, 5:42]              # non-contiguous rows, odd width
    assert _same(ops.topk_scores(q, emb, 17), _expected(ops, q.contiguous(), emb.contiguous(), 17))
    assert ops.topk_scores(q[:0], emb, 5)[0].shape == (0, 5)


def test_ties_nan_inf_and_signed_zero(ops):
    h, v = 8, 1300                                           # 21 column tiles: two spans
    gen = torch.Generator().manual_seed(0)
    emb = torch.randn(v, h, generator=gen).cuda()
    for j in (7, 70, 130, 200, 299, 1000, 1299):             # exact ties across tiles and spans
        emb[j] = emb[3]
    emb[10] = float('nan')
    emb[250] = float('nan')
    emb[20] = 0.0                                            # logit +0 (or -0: q . 0 with negative q entries)
    emb[21] = -0.0
    q = torch.stack([emb[3], -emb[3], torch.zeros(h, device='cuda'), emb[5]]).clone()
    q[2, 0] = 1.0
    emb[40] = 0.0
    emb[40, 0] = float('inf')                                # logit +inf for q[2], nan for q with a 0 there
    emb[41] = 0.0
    emb[41, 0] = float('-inf')
    for k in (1, 10, 64, 128):
        got = ops.topk_scores(q, emb, k)
        want = _expected(ops, q, emb, k)
        assert torch.equal(got[0], want[0])
        assert torch.equal(torch.nan_to_num(got[1], nan=7.0), torch.nan_to_num(want[1], nan=7.0))
        assert _same(got, want)
    # the rule itself: every entity once, NaN last, ties by id, -0 == +0
    ids, logits = ops.topk_scores(q, emb, 128)
    assert ids[2, 0] == 40 and logits[2, 0] == float('inf')             # +inf first
    row0 = ids[0].tolist()
    at = row0.index(3)
    assert row0[at:at + 8] == [3, 7, 70, 130, 200, 299, 1000, 1299]                # the exact ties of q . e_3, by id across tiles
    assert all(len(set(row)) == 128 for row in ids.tolist())
    # all-equal scores: ids in order, padded past v
    same = torch.ones(v, h, device='cuda')
    ids, logits = ops.topk_scores(torch.ones(1, h, device='cuda'), same[:100], 128)
    assert ids[0].tolist() == list(range(100)) + [-1] * 28
    assert bool((logits[0, :100] == h).all()) and bool((logits[0, 100:] == float('-inf')).all())
    # NaN candidates come after -inf ones, and among themselves by id
    e2 = torch.zeros(6, 1, device='cuda')
    e2[:, 0] = torch.tensor([float('nan'), float('-inf'), 1.0, float('nan'), -0.0, 0.0])
    ids, logits = ops.topk_scores(torch.ones(1, 1, device='cuda'), e2, 8)
    assert ids[0].tolist() == [2, 4, 5, 1, 0, 3, -1, -1]


def test_crosscheck_with_the_rankers(ops):
    """Where the first k + 1 logits of a row are tie-free, the entity at position p has raw rank p (gv_rank_scores) and, with the
    same filter, filtered rank p (gv_rank_scores_filtered)."""
    gen = torch.Generator().manual_seed(11)
    m, v, h, k = 150, 2500, 64, 40
    emb = torch.randn(v, h, generator=gen).cuda()
    q = torch.randn(m, h, generator=gen).cuda()
    bias = torch.tensor(0.75, device='cuda')
    lo, hi, ent = _lists(m, v, gen, ['empty', 'few', 'straddle', 'window', 'few'])
    ids_raw, lg_raw = ops.topk_scores(q, emb, k + 1, bias)
    ids_f, lg_f = ops.topk_scores(q, emb, k + 1, bias, lo, hi, ent)
    ok_raw = (lg_raw[:, 1:] < lg_raw[:, :-1]).all(1)          # a tie could only sit next to its equal in the order
    ok_f = (lg_f[:, 1:] < lg_f[:, :-1]).all(1)
    assert int(ok_raw.sum()) > m * 0.8 and int(ok_f.sum()) > m * 0.8
    for p in range(k):
        raw = ops.rank_scores(q, emb, ids_raw[:, p], bias)
        assert bool((raw[ok_raw] == p).all())
        _, filt = ops.rank_scores_filtered(q, emb, ids_f[:, p], lo, hi, ent, bias)
        assert bool((filt[ok_f] == p).all())


def _fb_split():
    from gcn_vae_amd import data
    return data.load_data('FB15k-237-synthetic')


def test_hits_at_10_equals_membership_in_the_top_10():
    """Filtered Hits@10 from perturb_and_get_rank_filtered equals the fraction of queries whose target is among
    predict_topk(k=10) with the same filter, in both directions (queries whose target is not in their own filter list)."""
    from gcn_vae_amd import ranking
    kg = _fb_split()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, device='cuda')
    gen = torch.Generator().manual_seed(6)
    v, h = kg.num_nodes, 200
    emb = (torch.randn(v, h, generator=gen) * 0.3).cuda()
    w = torch.randn(kg.num_rels, h, generator=gen).cuda()
    trip = torch.from_numpy(kg.test).cuda()
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    flp = torch.tensor(-0.5, device='cuda')
    for a, b, d in ((o, s, 's'), (s, o, 'o')):
        lo, hi = fi.lookup(a, r, d)
        ent = fi.entities(d, 'cuda').long()
        listed = torch.zeros(len(b), dtype=torch.bool, device='cuda')
        for i in torch.nonzero(hi > lo).flatten().tolist():
            listed[i] = bool((ent[int(lo[i]):int(hi[i])] == b[i]).any())
        keep = ~listed
        _, filt = ranking.perturb_and_get_rank_filtered(emb, w, a, r, b, len(b), fi, d, flow_log_prob=flp)
        ids, _ = ranking.predict_topk(emb, w, a, r, 10, direction=d, filter_index=fi, flow_log_prob=flp)
        hit_rank = ((filt[keep] + 1) <= 10).float().mean().item()
        hit_topk = (ids[keep] == b[keep].view(-1, 1)).any(1).float().mean().item()
        assert hit_rank == hit_topk and hit_rank > 0


def test_cli_writes_the_filtered_predictions(tmp_path, monkeypatch):
    from gcn_vae_amd import ranking, train
    from gcn_vae_amd.encoders import KGVAE
    spec = 'synthetic:300:7:2000:100:80:3'
    kg = __import__('gcn_vae_amd.data', fromlist=['load_data']).load_data(spec)
    torch.manual_seed(0)
    net = train.LinkPredict(KGVAE, kg.num_nodes, 16, kg.num_rels, num_bases=4, num_hidden_layers=1, dropout=0.0,
                            use_cuda=True, reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda()
    ckpt, out = str(tmp_path / 'm.pth'), str(tmp_path / 'pred.tsv')
    torch.save({'state_dict': train.host_state_dict(net), 'epoch': 0}, ckpt)
    seen = []
    real = ranking.predict_topk

    def spy(embed, w, a, r, k, direction='o', filter_index=None, flow_log_prob=None):
        seen.append((embed.detach().clone(), w.detach().clone(), a, r, direction, flow_log_prob))
        return real(embed, w, a, r, k, direction, filter_index, flow_log_prob)
    monkeypatch.setattr(ranking, 'predict_topk', spy)
    args = train.build_parser().parse_args(['-d', spec, '--gpu', '0', '--n-hidden', '16', '--n-bases', '4', '--n-layers', '1',
                                            '--mog-k', '4', '--n-flows', '2', '--test-mode', 'True', '--model-state-file',
                                            ckpt, '--predict-topk', '5', '--predict-out', out])
    train.main(args)
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    n_test = len(kg.test)
    assert len(rows) == 2 * n_test * 5 and len(seen) == 2
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    for j, (embed, w, a, r, d, flp) in enumerate(seen):
        ids, logits = real(embed, w, a, r, 5, d, fi, flp)
        block = rows[j * n_test * 5:(j + 1) * n_test * 5]
        assert all(x[0] == d for x in block)
        assert [int(x[4]) for x in block] == ids.reshape(-1).tolist()
        assert [int(x[3]) for x in block] == list(range(5)) * n_test
        assert [int(x[1]) for x in block[::5]] == a.tolist() and [int(x[2]) for x in block[::5]] == r.tolist()
        assert np.allclose([float(x[5]) for x in block], logits.reshape(-1).cpu().numpy(), rtol=1e-7, atol=0)
        for x in block:                                     # new facts only
            qa, rel, e = int(x[1]), int(x[2]), int(x[4])
            assert e == -1 or ((qa, rel, e) if d == 'o' else (e, rel, qa)) not in known


def test_full_fb15k237_size_against_the_unfused_path():
    """40 932 queries (both directions of the FB15k-237-sized test split) x 14 541 entities, h = 200, k = 10, filtered with the
    synthetic dataset's train + valid + test triplets: the fused path equals the materialised one exactly."""
    from gcn_vae_amd import ranking
    kg = _fb_split()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    gen = torch.Generator().manual_seed(5)
    v, h = kg.num_nodes, 200
    emb = (torch.randn(v, h, generator=gen) * 0.3).cuda()
    w = torch.randn(kg.num_rels, h, generator=gen).cuda()
    trip = torch.from_numpy(kg.test).cuda()
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    flp = torch.tensor(0.3, device='cuda')
    got, want = [], []
    for a_, d in ((s, 'o'), (o, 's')):
        got.append(ranking.predict_topk(emb, w, a_, r, 10, direction=d, filter_index=fi, flow_log_prob=flp))
        want.append(ranking.predict_topk_unfused(emb, w, a_, r, 10, direction=d, filter_index=fi, flow_log_prob=flp))
    assert sum(x[0].shape[0] for x in got) == 40932
    for g_, w_ in zip(got, want):
        assert _same(g_, w_)
