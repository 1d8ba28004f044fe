"""The selection epilogue the four top-k span kernels share (csrc/k_topk.h: topk_span_clear / topk_span_select / topk_span_hand_on),
at the two places the other top-k tests leave out: k = 65, the first k with two list registers per lane (list position 64 is lane 0
of the second register; k = 64 beside it is the last with one), and m = 17 query rows, a row tile whose second wave owns one row and
whose last two own none.  Every route is held to the project's torch rule on materialised values -- ids equal, value bits equal, no
tolerance -- with a filter whose lists put entries inside and across the 64-column windows.  pytest -m gpu."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, V, N, R, H = 17, 130, 70, 2, 8


def _pack_lists(lists):
    lens = np.array([len(e) for e in lists], dtype=np.int64)
    hi = np.cumsum(lens)
    ent = np.concatenate([np.asarray(e, dtype=np.int64) for e in lists])
    return torch.from_numpy(hi - lens).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(ent).cuda()


def _row_lists(rows, v, rng):
    """One sorted unique list per row: a few ids inside every 64-column window of [0, v), and on every second row the ids on both
    sides of each window boundary; row 3 lists nothing."""
    out = []
    for i in range(rows):
        ids = set(rng.choice(v, size=6, replace=False).tolist()) | {c + j for c in range(0, v, 64) for j in (1, 40) if c + j < v}
        if i % 2 == 0:
            ids |= {c + j for c in range(64, v, 64) for j in (-2, -1, 0, 1) if c + j < v}
        out.append(sorted(ids) if i != 3 else [])
    return out


def _bits(member):
    """(n_sets, v) bool -> int32 words, entity j = bit j & 31 of word j >> 5."""
    n_sets, v = member.shape
    pad = torch.zeros(n_sets, (v + 31) // 32 * 32, dtype=torch.int64)
    pad[:, :v] = member
    words = (pad.view(n_sets, -1, 32) << torch.arange(32)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(route):
    """(call, want): call(k) runs the fused route, want(k) the torch rule on the route's materialised values (made once here)."""
    from gcn_vae_amd import ops, ranking, transe
    gen = torch.Generator().manual_seed(65)
    rng = np.random.default_rng(17)
    if route in ('topk_scores', 'topk_scores_constrained', 'topk_scores_mc', 'transe_topk'):
        lo, hi, ent = _pack_lists(_row_lists(M, V, rng))
        e = (torch.randn(2, V, H, generator=gen) * 0.6).cuda()
        q = (torch.randn(2, M, H, generator=gen) * 0.6).cuda()
        if route == 'transe_topk':
            dist = ops.transe_distances(q[0], e[0], 1)
            return (lambda k: ops.transe_topk(q[0], e[0], k, 1, lo, hi, ent),
                    lambda k: transe.topk_from_distances(dist, k, lo, hi, ent))
        if route == 'topk_scores_mc':
            bias = torch.tensor([0.3, -0.2], device='cuda')
            # pbar[i, j] as the device computes it: the ranker's own value of target j for query i (tests/test_gpu_mc_rank.py holds
            # it equal to the selector's), one query row per (i, j)
            every = torch.arange(V, device='cuda').repeat(M)
            pbar = ops.rank_scores_mc(q.repeat_interleave(V, dim=1), e, every, bias)[2].view(M, V)
            return (lambda k: ops.topk_scores_mc(q, e, k, bias, lo, hi, ent),
                    lambda k: ranking.topk_from_scores(pbar, k, lo, hi, ent))
        bias = torch.tensor(0.37, device='cuda')
        score = ops.gemm(q[0], e[0], trans_b=True, precision='f32') + bias
        if route == 'topk_scores':
            return (lambda k: ops.topk_scores(q[0], e[0], k, bias, lo, hi, ent),
                    lambda k: ranking.topk_from_scores(score, k, lo, hi, ent))
        member = torch.ones(2, V, dtype=torch.bool)           # set 0: 87 members (more than k), set 1: 43 (pads at either k)
        member[0, ::3] = False
        member[1, 1::3] = member[1, 2::3] = False
        sets = (torch.arange(M) % 2).cuda()
        words, cand = _bits(member).cuda(), member.cuda()[sets]
        return (lambda k: ops.topk_scores_constrained(q[0], e[0], k, words, sets, bias, lo, hi, ent),
                lambda k: ranking.topk_from_scores(score, k, lo, hi, ent, cand=cand))
    # the per-entity routes: 17 query entities out of order and with a repeat, one filter range per key a * R + r
    lo, hi, ent = _pack_lists(_row_lists(N * R, N, rng))
    ents = torch.randperm(N, generator=gen)[:M]
    ents[9] = ents[0]
    ents = ents.cuda()
    emb = (torch.randn(N, H, generator=gen) * 0.6).cuda()
    w = torch.randn(R, H, generator=gen).cuda()
    if route == 'entity_topk_scores':
        ea = emb[ents].contiguous()
        score = torch.stack([ops.gemm(ops.mul(ea, w[r].expand_as(ea).contiguous()), emb, trans_b=True, precision='f32')
                             for r in range(R)], dim=1)
        return (lambda k: ops.entity_topk_scores(ents, emb, w, k, None, lo, hi, ent, span=1),
                lambda k: ranking.complete_entities_from_scores(score, ents, k, filt_lo=lo, filt_hi=hi, filt_ent=ent))
    assert route == 'transe_entity_topk'
    dist = torch.stack([ops.transe_distances(ops.transe_queries(emb, w, ents, torch.full_like(ents, r), norm_flag=False), emb, 1)
                        for r in range(R)], dim=1)
    return (lambda k: ops.transe_entity_topk(ents, emb, w, k, 1, False, lo, hi, ent, span=1),
            lambda k: transe.complete_entities_from_distances(dist, ents, k, filt_lo=lo, filt_hi=hi, filt_ent=ent))


@pytest.mark.parametrize('k', [64, 65])
@pytest.mark.parametrize('route', ['topk_scores', 'topk_scores_constrained', 'topk_scores_mc', 'transe_topk', 'entity_topk_scores',
                                   'transe_entity_topk'])
def test_k_64_and_65_on_17_rows_equal_the_torch_rule_exactly(route, k):
    call, rule = _case(route)
    got, want = call(k), rule(k)
    assert len(got) == len(want) and got[0].shape == (M, k)
    for g, x in zip(got[:-1], want[:-1]):
        assert g.dtype == torch.int64 and torch.equal(g, x.to(g.device))
    assert torch.equal(got[-1].view(torch.int32), want[-1].to(got[-1].device).view(torch.int32))
    full = (got[0] >= 0).all(dim=1)                           # list position k - 1 is taken on the rows with k candidates or more
    assert bool(full.any()) and (route != 'topk_scores_constrained' or not bool(full.all()))
