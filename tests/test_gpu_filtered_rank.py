"""Filtered ranks on the GPU (gv_rank_scores_filtered / ops.rank_scores_filtered / ranking.calc_filtered_mrr) against the
definition on materialised logits: the same f32 MFMA product (ops.gemm), masked in torch with the filter sets, mid-rank ties.
pytest -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from gcn_vae_amd import ops as _ops
    return _ops


def _filter_mask(lo, hi, ent, m, v):
    """Dense (m, v) bool: True where entity j is listed in query i's range."""
    lo, hi, ent = lo.long().cuda(), hi.long().cuda(), ent.long().cuda()
    lens = hi - lo
    total = int(lens.sum())
    mask = torch.zeros(m, v, dtype=torch.bool, device='cuda')
    if total:
        rows = torch.repeat_interleave(torch.arange(m, device='cuda'), lens)
        first = torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
        idx = torch.repeat_interleave(lo, lens) + torch.arange(total, device='cuda') - first
        mask[rows, ent[idx]] = True
    return mask


def _by_definition(ops, q, emb, target, lo, hi, ent, bias=None, score=None):
    """(raw, filtered, #filtered better, #filtered equal) from materialised logits."""
    if score is None:
        score = ops.gemm(q, emb, trans_b=True, precision='f32')
        if bias is not None:
            score = score + bias
    m, v = score.shape
    t = target.view(-1, 1).long()
    tgt = score.gather(1, t)
    other = torch.ones_like(score, dtype=torch.bool).scatter_(1, t, False)
    better = (~(score <= tgt)) & other
    equal = (score == tgt) & other
    f = _filter_mask(lo, hi, ent, m, v)
    raw = better.sum(1).float() + 0.5 * equal.sum(1).float()
    filt = (better & ~f).sum(1).float() + 0.5 * (equal & ~f).sum(1).float()
    return raw, filt, (better & f).sum(1), (equal & f).sum(1)


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
        elif k == 'long':              # more than 5 000 entries (or most of a small entity set)
            e = np.unique(torch.randint(0, v, (min(6000, v),), generator=gen).numpy())
            if v > 6000:
                e = np.unique(np.concatenate([e, np.arange(0, v, 2)]))[:max(5001, len(e))]
        else:
            raise ValueError(k)
        out.append(e)
    lens = np.array([len(e) for e in out], dtype=np.int64)
    hi = np.cumsum(lens)
    ent = np.concatenate(out) if lens.sum() else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(hi - lens).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(ent).cuda()


@pytest.mark.parametrize('m,v,h,flp', [(64, 128, 8, None), (37, 1000, 200, 0.25), (129, 777, 500, None), (200, 6400, 200, -1.5),
                                       (1, 5, 8, None), (70, 7000, 8, 3.0)])
def test_filtered_ranks_equal_the_definition(ops, m, v, h, flp):
    gen = torch.Generator().manual_seed(m * 13 + v + h)
    emb = (torch.randn(v, h, generator=gen) * 0.5).cuda()
    q = torch.randn(m, h, generator=gen).cuda()
    target = torch.randint(0, v, (m,), generator=gen).cuda()
    lo, hi, ent = _lists(m, v, gen, ['empty', 'few', 'straddle', 'window', 'long', 'few'])
    # a few queries list their own target
    for i in range(0, m, 5):
        if int(hi[i]) > int(lo[i]):
            target[i] = ent[int(lo[i])]
    bias = None if flp is None else torch.tensor(flp, device='cuda')
    raw, filt = ops.rank_scores_filtered(q, emb, target, lo, hi, ent, bias)
    w_raw, w_filt, n_fb, n_fe = _by_definition(ops, q, emb, target, lo, hi, ent, bias)
    assert raw.dtype == torch.float32 and filt.dtype == torch.float32
    assert torch.equal(raw, w_raw) and torch.equal(filt, w_filt)
    # the raw output is gv_rank_scores' own, bit for bit
    assert torch.equal(raw, ops.rank_scores(q, emb, target, bias))
    # removal is monotone and exact
    assert bool((filt <= raw).all())
    assert torch.equal(raw - filt, n_fb.float() + 0.5 * n_fe.float())


def test_shared_ranges_and_empty_filter(ops):
    gen = torch.Generator().manual_seed(2)
    m, v, h = 300, 2000, 200
    emb = torch.randn(v, h, generator=gen).cuda()
    q = torch.randn(m, h, generator=gen).cuda()
    target = torch.randint(0, v, (m,), generator=gen).cuda()
    # no filter at all: filtered == raw == gv_rank_scores
    z = torch.zeros(m, dtype=torch.int64, device='cuda')
    raw, filt = ops.rank_scores_filtered(q, emb, target, z, z, torch.zeros(0, dtype=torch.int64, device='cuda'))
    assert torch.equal(raw, filt) and torch.equal(raw, ops.rank_scores(q, emb, target))
    # every query shares one list of 900 entities
    ent = torch.from_numpy(np.unique(torch.randint(0, v, (900,), generator=gen).numpy())).cuda()
    lo, hi = z.clone(), torch.full((m,), ent.numel(), dtype=torch.int64, device='cuda')
    raw, filt = ops.rank_scores_filtered(q, emb, target, lo, hi, ent)
    _, w_filt, _, _ = _by_definition(ops, q, emb, target, lo, hi, ent)
    assert torch.equal(filt, w_filt)
    with pytest.raises(ValueError):
        ops.rank_scores_filtered(q, emb, target, lo, hi + 1, ent)                 # range past the end of the list
    with pytest.raises(ValueError):
        ops.rank_scores_filtered(q, emb, target, lo, hi, ent + v)                 # ids out of [0, v)
    with pytest.raises(ValueError):
        ops.rank_scores_filtered(q, emb, target, lo[:-1], hi[:-1], ent)           # one range per query


def test_ties_and_nan(ops):
    h, v = 8, 130
    emb = torch.randn(v, h, generator=torch.Generator().manual_seed(0)).cuda()
    emb[7] = emb[3]
    emb[129] = emb[3]
    emb[100] = emb[3]
    q = emb[[3, 3, 3]].clone()
    target = torch.tensor([3, 3, 7], device='cuda')
    # query 0: entity 7 (a tie) filtered; query 1: nothing filtered; query 2: 3 and 100 (ties) filtered, 129 not
    lists = [[7], [], [3, 100]]
    lens = torch.tensor([len(x) for x in lists], device='cuda')
    hi = torch.cumsum(lens, 0)
    lo = hi - lens
    ent = torch.tensor(sum(lists, []), device='cuda')
    raw, filt = ops.rank_scores_filtered(q, emb, target, lo, hi, ent)
    score = ops.gemm(q, emb, trans_b=True, precision='f32')
    better = [int((score[i] > score[i, int(target[i])]).sum()) for i in range(3)]
    assert float(raw[0]) == better[0] + 1.5 and float(filt[0]) == better[0] + 1.0
    assert float(filt[1]) == float(raw[1]) == better[1] + 1.5
    assert float(raw[2]) == better[2] + 1.5 and float(filt[2]) == better[2] + 0.5
    # NaN: a filtered NaN candidate counts nowhere, an unfiltered one counts as better
    bad = emb.clone()
    bad[10] = float('nan')
    bad[20] = float('nan')
    ent_nan = torch.tensor([10], device='cuda')
    one = torch.zeros(1, dtype=torch.int64, device='cuda')
    qq = emb[[3]].clone()
    t3 = torch.tensor([3], device='cuda')
    raw, filt = ops.rank_scores_filtered(qq, bad, t3, one, one + 1, ent_nan)
    sc = ops.gemm(qq, bad, trans_b=True, precision='f32')[0]
    b = int((sc > sc[3]).sum())
    assert float(raw[0]) == b + 2 + 1.5 and float(filt[0]) == b + 1 + 1.5
    # a NaN target ranks last among the candidates that count
    bad_t = emb.clone()
    bad_t[3] = float('nan')
    ent5 = torch.tensor([0, 1, 2, 3, 4], device='cuda')
    raw, filt = ops.rank_scores_filtered(qq, bad_t, t3, one, one + 5, ent5)
    assert float(raw[0]) == v - 1 and float(filt[0]) == v - 1 - 4
    # all-equal scores: the middle rank of the candidates that count
    same = torch.ones(v, h, device='cuda')
    tq = torch.tensor([0, 64], device='cuda')
    lo2, hi2 = torch.tensor([0, 0], device='cuda'), torch.tensor([10, 10], device='cuda')
    raw, filt = ops.rank_scores_filtered(torch.ones(2, h, device='cuda'), same, tq, lo2, hi2, torch.arange(10, device='cuda'))
    assert torch.equal(raw.cpu(), torch.full((2,), (v - 1) / 2.0))
    assert float(filt[0]) == (v - 10) / 2.0 and float(filt[1]) == (v - 1 - 10) / 2.0


def test_tiny_hand_computed_case(ops):
    # one-dimensional embeddings: score(i, j) = q_i * e_j, so the scores are the entity values themselves for q = 1
    e = torch.tensor([[5.0], [3.0], [9.0], [3.0], [1.0], [7.0]], device='cuda')
    q = torch.tensor([[1.0]], device='cuda')
    target = torch.tensor([1], device='cuda')                  # score 3: better 5, 9, 7; tie 3 (entity 3)
    lo, hi = torch.tensor([0], device='cuda'), torch.tensor([2], device='cuda')
    raw, filt = ops.rank_scores_filtered(q, e, target, lo, hi, torch.tensor([2, 3], device='cuda'))   # 9 and the tie filtered
    assert float(raw[0]) == 3.5 and float(filt[0]) == 2.0


def test_full_fb15k237_size_against_the_materialised_path(ops):
    """The whole FB15k-237-sized test split in both directions (2 x 20 466 queries x 14 541 entities, h = 200), the filter from a
    Zipf-skewed synthetic dataset (train + valid + test): every raw and filtered rank equals the materialised definition."""
    from gcn_vae_amd import data, ranking
    kg = data.load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    gen = torch.Generator().manual_seed(5)
    v, h = kg.num_nodes, 200
    emb = (torch.randn(v, h, generator=gen) * 0.3).cuda()
    w = torch.randn(kg.num_rels, h, generator=gen).cuda()
    trip = torch.from_numpy(kg.test).cuda()
    s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
    longest = 0
    for a, b, d in ((o, s, 's'), (s, o, 'o')):
        raw, filt = ranking.perturb_and_get_rank_filtered(emb, w, a, r, b, len(b), fi, d)
        lo, hi = fi.lookup(a, r, d)
        longest = max(longest, int((hi - lo).max()))
        ent = fi.entities(d, 'cuda')
        for c in range(0, len(b), 4096):
            sl = slice(c, c + 4096)
            q = ops.mul(emb[a[sl]].contiguous(), w[r[sl]].contiguous())
            w_raw, w_filt, _, _ = _by_definition(ops, q, emb, b[sl], lo[sl], hi[sl], ent)
            assert torch.equal(raw[sl], w_raw) and torch.equal(filt[sl], w_filt)
        assert torch.equal(raw, ranking.perturb_and_get_rank(emb, w, a, r, b, len(b)))
        assert bool((filt <= raw).all()) and bool((filt < raw).any())
    assert longest > 32                  # Zipf-skewed list lengths (most keys hold one answer)


def test_calc_filtered_mrr_end_to_end():
    """Real encoder embeddings of a seeded synthetic KG: raw MRR equals calc_mrr, filtered MRR / Hits agree with a float64 CPU
    restatement, filtered >= raw."""
    from gcn_vae_amd import ranking, sampling
    from gcn_vae_amd.data import synthetic_kg
    from gcn_vae_amd.encoders import KGVAE
    from gcn_vae_amd.train import LinkPredict
    kg = synthetic_kg(400, 9, 3000, 200, 300, seed=4)
    torch.manual_seed(0)
    net = LinkPredict(KGVAE, kg.num_nodes, 32, kg.num_rels, num_bases=4, num_hidden_layers=2, dropout=0.0, use_cuda=True,
                      reg_param=0.01, kl_param=1e-3, mmd_param=0.0, k=4, n_flows=2).cuda().eval()
    graph, rel, norm = sampling.build_test_graph(kg.num_nodes, kg.num_rels, kg.train)
    node_id = torch.arange(kg.num_nodes, device='cuda').view(-1, 1)
    enorm = sampling.node_norm_to_edge_norm(graph, torch.from_numpy(norm).view(-1, 1)).cuda()
    with torch.no_grad():
        embed = net(graph, node_id, torch.from_numpy(rel).cuda(), enorm)
    flp = net.encoder.get_flow_log_prob()
    test = torch.from_numpy(kg.test).cuda()
    fi = ranking.FilterIndex(kg.num_nodes, kg.num_rels, kg.train, kg.valid, kg.test, device='cuda')
    out = ranking.calc_filtered_mrr(embed, net.w_relation, test, fi, hits=[1, 3, 10], eval_bz=50, flow_log_prob=flp,
                                    verbose=False)
    assert out['mrr_raw'] == ranking.calc_mrr(embed, net.w_relation, test, hits=[1, 3, 10], eval_bz=50, flow_log_prob=flp,
                                              verbose=False)
    # float64 restatement on the host from the known-triplet sets
    e64, w64 = embed.detach().cpu().double(), net.w_relation.detach().cpu().double()
    f64 = float(flp.detach().cpu().reshape(-1)[0]) if isinstance(flp, torch.Tensor) else 0.0
    known = {tuple(x) for x in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    ranks = []
    ties = 0
    for s_, r_, o_ in kg.test.tolist():
        for a, b, side in ((o_, s_, 's'), (s_, o_, 'o')):
            sc = (e64[a] * w64[r_]) @ e64.T + f64
            keep = torch.ones(kg.num_nodes, dtype=torch.bool)
            for j in range(kg.num_nodes):
                if (side == 'o' and (s_, r_, j) in known) or (side == 's' and (j, r_, o_) in known):
                    keep[j] = False
            keep[b] = False
            ties += int((sc[keep] == sc[b]).sum())
            ranks.append(1 + int((sc[keep] > sc[b]).sum()))
    assert ties == 0
    rk = torch.tensor(ranks, dtype=torch.float64)
    assert abs(out['mrr_filtered'] - float((1.0 / rk).mean())) < 1e-6
    for k in (1, 3, 10):
        assert abs(out['hits_filtered'][k] - float((rk <= k).double().mean())) < 1e-6
    assert out['mrr_filtered'] >= out['mrr_raw']
    assert all(out['hits_filtered'][k] >= out['hits_raw'][k] for k in (1, 3, 10))
