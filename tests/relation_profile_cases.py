"""What the two per-relation completion test files share (test_relation_profile_host.py without a GPU, test_gpu_relation_profile.py
with one): the rule as three Python loops per relation and exact comparison of a route's rows with it."""
import math

import torch


def brute_force(val, rels, k, filt=None, exclude_self=True, cand_subj=None, cand_obj=None):
    """For each relation of ``rels`` its candidates of val[r, s, o] in the rule's order -- logit descending, -0 == +0, then (s, o)
    -- by three Python loops; ``filt`` a set of (s, r, o), ``cand_subj`` / ``cand_obj`` bool (R, N).  Returns (subj (m, k), obj
    (m, k), logits (m, k), count [m]) padded with -1 / -1 / -inf."""
    n, m = val.shape[1], len(rels)
    subj, obj = torch.full((m, k), -1, dtype=torch.int64), torch.full((m, k), -1, dtype=torch.int64)
    logits, count = torch.full((m, k), float('-inf')), torch.zeros(m, dtype=torch.int64)
    for i, r in enumerate(rels):
        cands = []
        for s in range(n):
            for o in range(n):
                x = float(val[r, s, o])
                if math.isnan(x) or (exclude_self and s == o) or (filt and (s, r, o) in filt):
                    continue
                if cand_subj is not None and not (bool(cand_subj[r, s]) and bool(cand_obj[r, o])):
                    continue
                cands.append((-(x + 0.0), s, o))
        cands.sort()
        count[i] = len(cands) if len(cands) <= k else sum(1 for c in cands if c[0] <= cands[k - 1][0])
        for j, (x, s, o) in enumerate(cands[:k]):
            subj[i, j], obj[i, j], logits[i, j] = s, o, -x + 0.0
    return subj, obj, logits, count


def same(got, want):
    """A route's (subj, obj, logits, info) against brute_force's (subj, obj, logits, count): ids, value bit patterns, counts."""
    return (torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
            and torch.equal(got[2].cpu().view(torch.int32), want[2].view(torch.int32)) and torch.equal(got[3]['count'].cpu(), want[3]))


def same_rows(a, b, rows_a=None, rows_b=None):
    """Two routes' results equal bit for bit, optionally on chosen rows of each."""
    pick = lambda t, rows: t.cpu() if rows is None else t.cpu()[rows]
    return (all(torch.equal(pick(x, rows_a), pick(y, rows_b)) for x, y in zip(a[:2], b[:2]))
            and torch.equal(pick(a[2], rows_a).view(torch.int32), pick(b[2], rows_b).view(torch.int32))
            and torch.equal(pick(a[3]['count'], rows_a), pick(b[3]['count'], rows_b)))
