"""What the tests of the Monte-Carlo typed miner share (test_gpu_mine_typed_mc.py): sample stacks, the posterior-predictive
probabilities of every (s, r, o) taken from the rankers' own tile (ops.topk_scores_mc with k = n), the float64 reference with its
per-element bound, the host rule applied to emitted values, and a raw call of the C entry."""
import numpy as np
import torch

U = 2.0 ** -24
C_SIG = 4.0                # tests/test_gpu_mc_rank.py: twice the device sigmoid's largest measured error, rounded up


def stack(s, n, h, num_rels, seed, scale=None, bias=True):
    """(z (S, n, h), w (R, h), bias (S,) or None) on the GPU: samples scattered around one base table."""
    gen = torch.Generator().manual_seed(seed)
    scale = 0.8 * h ** -0.25 if scale is None else scale
    base = scale * torch.randn(n, h, generator=gen)
    z = base.unsqueeze(0) + 0.5 * scale * torch.randn(s, n, h, generator=gen)
    w = torch.randn(num_rels, h, generator=gen)
    b = 0.5 * torch.randn(s, generator=gen) if bias else None
    return z.cuda(), w.cuda(), (None if b is None else b.cuda()), gen


def pbar_from_topk(ops, ranking, z, w, bias):
    """pbar[r, s, o] (R, n, n) for n <= 128, every value from gv_topk_scores_mc's tile: k = n returns all n probabilities of each of
    the n * R queries z_s[a] * w[r]."""
    n, num_rels = z.shape[1], w.shape[0]
    a = torch.arange(n, device=z.device).repeat_interleave(num_rels)
    r = torch.arange(num_rels, device=z.device).repeat(n)
    ids, prob = ops.topk_scores_mc(ranking._mc_queries(z, w, a, r), z, n, bias)
    assert int(ids.min()) >= 0
    dense = torch.empty(n * num_rels, n, device=z.device).scatter_(1, ids, prob)
    return dense.view(n, num_rels, n).permute(1, 0, 2).contiguous()


def pbar64(z, w, bias):
    """(pbar, eps), float64 numpy (R, n, n): the definition on the fp32 inputs (the query's one fp32 multiply included) and the bound
    eps = mean_s(gamma (|q_s| . |e_s| + |bias_s|) / 4) + C_SIG u + S u, gamma = (h + 2) u."""
    z32, w32 = z.cpu().numpy(), w.cpu().numpy()
    s, n, h = z32.shape
    b = np.zeros(s) if bias is None else bias.cpu().numpy().astype(np.float64)
    total, mag = np.zeros((w32.shape[0], n, n)), np.zeros((w32.shape[0], n, n))
    for i in range(s):
        e64 = z32[i].astype(np.float64)
        for r in range(w32.shape[0]):
            q64 = (z32[i] * w32[r][None]).astype(np.float64)
            with np.errstate(over='ignore'):
                total[r] += 1.0 / (1.0 + np.exp(-(q64 @ e64.T + b[i])))
            mag[r] += np.abs(q64) @ np.abs(e64).T + abs(b[i])
    return total / s, (h + 2) * U * (mag / s) / 4 + C_SIG * U + s * U


def dense_of(got, n, num_rels):
    """A route's emitted (triplets, values) as val[r, s, o] with NaN wherever nothing was emitted: the host rule on it, with no
    filter and the diagonal kept, selects among the kernel's own candidates at the kernel's own values."""
    val = torch.full((num_rels, n, n), float('nan'), device=got[0].device)
    val[got[0][:, 1], got[0][:, 0], got[0][:, 2]] = got[1]
    return val


def candidates(cs, co, filt, exclude_self):
    """The definition's candidate mask [r, s, o] (CPU bool) before any look at the values."""
    num_rels, n = cs.shape
    cand = cs[:, :, None] & co[:, None, :]
    if exclude_self:
        cand &= ~torch.eye(n, dtype=torch.bool)[None]
    if filt is not None:
        lo, hi, ent = (t.cpu() for t in filt)
        for key in range(n * num_rels):
            cand[key % num_rels, key // num_rels, ent[lo[key]:hi[key]]] = False
    return cand


def emit_through_the_c_entry(ops, z, w, set_ptr, set_ids, capacity):
    """gv_mine_scores_typed_mc called as C callers call it -- nothing between the lists and the kernel -- in EMIT mode at key 1
    (every candidate): (triplets, values) in the rule's order, and the count."""
    from gcn_vae_amd import lib
    s, n, h = z.shape
    num_rels = w.shape[0]
    units = ops.mine_typed_plan(set_ptr, num_rels)
    out = torch.empty(capacity, 4, dtype=torch.int32, device=z.device)
    counter = torch.zeros(1, dtype=torch.int64, device=z.device)
    lib.call('gv_mine_scores_typed_mc', z.data_ptr(), h, n * h, s, w.data_ptr(), h, None, set_ptr.data_ptr(), set_ids.data_ptr(),
             units.data_ptr(), units.shape[0], None, None, None, 0, 1, 0, 1, 0, 0, 1, out.data_ptr(), capacity, counter.data_ptr(),
             counter.data_ptr(), n, num_rels, h, lib.stream())
    count = int(counter[0])
    rec = out[:min(count, capacity)]
    return ops.mine_order(rec[:, :3].long(), rec[:, 3].contiguous().view(torch.float32), n, num_rels) + ({'count': count},)
