"""What the tests of per-entity completion on the posterior predictive share (test_gpu_entity_profile_mc.py): sample stacks, the
dense posterior-predictive probabilities of every (a, r, x) taken from the existing Monte-Carlo scorer's own tile, the rule applied
to them, and the integer tables whose ties cross relations and span cuts."""
import functools

import torch

from entity_typed_cases import pack
from mine_mc_cases import pbar_from_topk, stack

SHAPES = [(3, 70, 7, 37), (2, 128, 3, 20), (4, 150, 3, 20), (2, 130, 5, 260)]      # (S, N, R, h)


@functools.lru_cache(maxsize=None)
def stack_of(s, n, num_rels, h, with_bias, seed=None):
    """(z (S, N, h), w (R, h), bias (S,) or None) on the GPU; left unchanged by every test."""
    z, w, bias, _ = stack(s, n, h, num_rels, s * 1000 + n * 31 + num_rels * 7 + h if seed is None else seed, bias=with_bias)
    return z, w, bias


def dense_pbar(z, w, bias):
    """pbar[r, a, x] (R, N, N) on the GPU, every value from the existing MC scorer's tile, for the query z_s[a] * w[r] at entity x:
    gv_topk_scores_mc with k = N up to 128 entities, else gv_topk_scores_mc_constrained over candidate blocks of at most 128 ids
    (its pbar is the unconstrained entry's, bit for bit)."""
    from gcn_vae_amd import ops, ranking
    n, num_rels = z.shape[1], w.shape[0]
    if n <= 128:
        return pbar_from_topk(ops, ranking, z, w, bias)
    a = torch.arange(n, device=z.device).repeat_interleave(num_rels)
    r = torch.arange(num_rels, device=z.device).repeat(n)
    q = ranking._mc_queries(z, w, a, r)
    blocks = (n + 127) // 128
    member = torch.zeros(blocks, n, dtype=torch.bool)
    for b in range(blocks):
        member[b, 128 * b:128 * (b + 1)] = True
    words = pack(member).cuda()
    dense = torch.empty(n * num_rels, n, device=z.device)
    seen = torch.zeros(n * num_rels, n, dtype=torch.bool, device=z.device)
    for b in range(blocks):
        ids, prob = ops.topk_scores_mc_constrained(q, z, 128, words, torch.full((n * num_rels,), b, device=z.device), bias)
        live = ids >= 0
        rows = torch.arange(n * num_rels, device=z.device).view(-1, 1).expand_as(ids)
        dense[rows[live], ids[live]] = prob[live]
        seen[rows[live], ids[live]] = True
    assert bool(seen.all())
    return dense.view(n, num_rels, n).permute(1, 0, 2).contiguous()


@functools.lru_cache(maxsize=None)
def dense_pbar_of(s, n, num_rels, h, with_bias):
    return dense_pbar(*stack_of(s, n, num_rels, h, with_bias))


def rule(pbar, ents, k, side='s', filter_index=None, exclude_self=True, cand_subj=None, cand_obj=None):
    """``ranking.complete_entities_from_scores`` on the dense pbar[r, a, x], for the query entities ``ents`` on ``side``: the filter
    of the other direction, and with the masks (bool (R, N), CPU) the typed rule seen from that side."""
    from gcn_vae_amd import ranking
    n, num_rels = pbar.shape[1], pbar.shape[0]
    lo, hi, ent = ranking._mine_filter(filter_index, n, num_rels, pbar.device, 'o' if side == 's' else 's')
    masks = {}
    if cand_subj is not None:
        cq, co = (cand_subj, cand_obj) if side == 's' else (cand_obj, cand_subj)
        masks = dict(cand_query=cq.to(pbar.device), cand_other=co.to(pbar.device))
    inside = ents.clamp(0, n - 1)
    return ranking.complete_entities_from_scores(pbar[:, inside].permute(1, 0, 2), ents, k, filt_lo=lo, filt_hi=hi, filt_ent=ent,
                                                 exclude_self=exclude_self, **masks)


def dyadic_case(n_samples):
    """The single-sample tests' integer tables -- relations 0 and 2 the same row of w, entities 3 and 90 the same row of every
    sample's table -- stacked ``n_samples`` times with a small integer perturbation per sample: every logit is an exact small
    integer, so equal logit tuples give equal pbar bits and the twins tie across relations, column tiles and span cuts.  The
    typed case keeps both twins as candidates of both relations: relation 0 all but three ids (147 members, three tiles),
    relation 1 65 random members (two tiles), relation 2 the even ids and 3 (76 members, two tiles), relation 3 30 members (one
    tile): 8 tiles.  Returns (z, w, cand_subj, cand_obj)."""
    gen = torch.Generator().manual_seed(5)
    n, num_rels, h = 150, 4, 6
    emb = torch.randint(-2, 3, (n, h), generator=gen).float()
    w = torch.randint(-1, 2, (num_rels, h), generator=gen).float()
    w[2] = w[0]
    co = torch.zeros(num_rels, n, dtype=torch.bool)
    co[0] = True
    co[0, [10, 20, 30]] = False
    co[1, torch.randperm(n, generator=gen)[:65]] = True
    co[2, 0::2] = True
    co[2, 3] = True
    co[3, torch.randperm(n, generator=gen)[:30]] = True
    cs = torch.rand(num_rels, n, generator=gen) < 0.5
    cs[0], cs[2] = True, True
    z = emb.unsqueeze(0) + torch.randint(-1, 2, (n_samples, n, h), generator=gen).float()
    z[:, 90] = z[:, 3]
    return z.cuda(), w.cuda(), cs, co
