"""What the per-entity completion benches share (entity_profile_bench.py, entity_profile_typed_bench.py, entity_profile_mc_bench.py,
transe_bench.py --profile): the two dataset shapes, the comparison of two routes' answers, the alternated timing of routes, and
the torch merge of per-query answers over each entity's relations."""
import statistics
import time

import torch

SHAPES = {'fb': ('FB15k-237-synthetic', 200), 'wn18rr': ('WN18RR-synthetic', 200)}


def same(a, b):
    """Two (rel, other, values, ...) answers: the ids equal, the values equal bit for bit."""
    return all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def time_routes(routes, reps):
    """(each route's answer from its warm-up, each route's median of ``reps`` synchronised timed regions in ms), alternated."""
    outs = {nm: fn() for nm, fn in routes}                                   # warm-up of every route
    torch.cuda.synchronize()
    times = {nm: [] for nm, _ in routes}
    for _ in range(reps):                                                    # alternated
        for nm, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[nm].append(time.perf_counter() - t0)
    return outs, {nm: statistics.median(v) * 1e3 for nm, v in times.items()}


def merge_member_queries(rows, rels, ids, values, m, n, num_rels, k, ascending):
    """The (Q, k) answers of the member queries (rows[q], rels[q]) -- row-major, relations ascending inside a row -- into each
    entity's k best (r, x): by value, then relation, then entity.  Padded to the largest number of relations an entity has."""
    dev = ids.device
    count = torch.bincount(rows, minlength=m)
    width = int(count.max()) if rows.numel() else 0
    cid = torch.full((m, max(width, 1), k), num_rels * n, dtype=torch.long, device=dev)
    val = torch.full((m, max(width, 1), k), float('inf') if ascending else float('-inf'), dtype=torch.float32, device=dev)
    if rows.numel():
        slot = torch.arange(rows.numel(), device=dev) - (torch.cumsum(count, 0) - count)[rows]
        cid[rows, slot] = _candidate_ids(rels, ids, n, num_rels)
        val[rows, slot] = values
    return _merge_slots(cid.view(m, -1), val.view(m, -1), n, num_rels, k, ascending)


def merge_all_queries(ids, values, m, n, num_rels, k, ascending):
    """``merge_member_queries`` for the (m * R, k) answers of ALL queries (a, r), a-major: every pair is a member query, so an
    entity's slots are a view of the answers as they come (no count, no scatter: they cost a single-entity call a quarter more)."""
    rels = torch.arange(num_rels, device=ids.device).repeat(m)
    return _merge_slots(_candidate_ids(rels, ids, n, num_rels).view(m, -1), values.reshape(m, -1), n, num_rels, k, ascending)


def _candidate_ids(rels, ids, n, num_rels):
    """r * N + x of every answer, the id past every candidate's (R * N) in the padding slots."""
    return torch.where(ids < 0, torch.full_like(ids, num_rels * n), rels.view(-1, 1) * n + ids)


def _merge_slots(cid, val, n, num_rels, k, ascending):
    """Each row's k best of its slots (candidate id, value): by value, then id -- relation first, then entity."""
    m, gone_id, worst = cid.shape[0], num_rels * n, float('inf') if ascending else float('-inf')
    by_id = torch.argsort(cid, dim=1, stable=True)
    order = by_id.gather(1, torch.argsort(val.gather(1, by_id), dim=1, descending=not ascending, stable=True)[:, :k])
    if order.shape[1] < k:                                                   # fewer than k slots in all: pad
        pad = torch.zeros(m, k - order.shape[1], dtype=torch.long, device=cid.device)
        best = torch.cat([cid.gather(1, order), pad + gone_id], 1)
        out = torch.cat([val.gather(1, order), pad.float() + worst], 1)
    else:
        best, out = cid.gather(1, order), val.gather(1, order)
    gone = best >= gone_id
    return torch.where(gone, -1, best // n), torch.where(gone, -1, best % n), torch.where(gone, torch.full_like(out, worst), out)
