"""What the four mining test files share (test_mine_host.py, test_transe_mine_host.py without a GPU; test_gpu_mine.py,
test_gpu_transe_mine.py with one): the rule as three Python loops, filters as (lo, hi, ent) arrays, and exact comparison."""
import math

import numpy as np
import torch


def brute_force(val, ascending, k=None, threshold=None, filt=None, exclude_self=True):
    """Every candidate of val[r, s, o] in the rule's total order -- value descending, or ``ascending`` (distances), -0 == +0, then
    (s, r, o) -- by three Python loops; ``filt`` a set of (s, r, o)."""
    num_rels, n = val.shape[0], val.shape[1]
    sign = 1.0 if ascending else -1.0
    cands = []
    for s in range(n):
        for r in range(num_rels):
            for o in range(n):
                x = float(val[r, s, o])
                if math.isnan(x) or (exclude_self and s == o) or (filt and (s, r, o) in filt):
                    continue
                cands.append((sign * (x + 0.0), s, r, o))
    cands.sort()
    if threshold is not None:
        cands = [c for c in cands if c[0] <= sign * threshold]
        count = len(cands)
    else:
        count = len(cands) if len(cands) <= k else sum(1 for c in cands if c[0] <= cands[k - 1][0])
        cands = cands[:k]
    trip = torch.tensor([c[1:] for c in cands], dtype=torch.int64).reshape(-1, 3)
    values = torch.tensor([sign * c[0] + 0.0 for c in cands], dtype=torch.float32)
    return trip, values, count


def filter_arrays(filt, n, num_rels):
    """(lo, hi, ent) over the keys s * R + r of a set of (s, r, o)."""
    lists = [[] for _ in range(n * num_rels)]
    for s, r, o in sorted(filt):
        lists[s * num_rels + r].append(o)
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    hi = np.cumsum(lens)
    ent = np.array([o for x in lists for o in x], dtype=np.int64)
    return torch.from_numpy(hi - lens), torch.from_numpy(hi), torch.from_numpy(ent)


def same(got, want):
    """A route's (triplets, values, info) against brute_force's (triplets, values, count), values as bit patterns."""
    return (torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            and got[2]['count'] == want[2])


def _same(a, b):
    """Bit-for-bit equality of (triplets, values) and of the reported counts."""
    return (torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
            and a[2]['count'] == b[2]['count'])


def _lists(keys, v, gen, dense):
    """Sorted unique object lists per key s * R + r, packed into (lo, hi, ent): empty, few, straddling a 64-column tile edge, a
    whole 64-column window, all but two.  ``dense``: every key gets a kind in turn, otherwise most keys stay empty."""
    cycle = ['empty', 'few', 'straddle', 'window', 'long', 'few', 'empty']
    sparse = {0: 'few', 3: 'few', 7: 'straddle', 13: 'window', 29: 'long'}
    out = []
    for i in range(keys):
        kind = cycle[i % len(cycle)] if dense else sparse.get(i % 41, 'empty')
        if kind == 'empty':
            e = np.zeros(0, dtype=np.int64)
        elif kind == 'few':
            e = np.unique(torch.randint(0, v, (5,), generator=gen).numpy())
        elif kind == 'straddle':
            c = 64 * int(torch.randint(1, max(2, v // 64), (1,), generator=gen))
            e = np.arange(max(0, min(v, c) - 3), min(v, c + 3))
        elif kind == 'window':
            c = 64 * int(torch.randint(0, max(1, v // 64), (1,), generator=gen))
            e = np.arange(c, min(v, c + 64))
        else:
            e = np.sort(torch.randperm(v, generator=gen)[:max(0, v - 2)].numpy())
        out.append(e)
    lens = np.array([len(e) for e in out], dtype=np.int64)
    hi = np.cumsum(lens)
    ent = np.concatenate(out) if lens.sum() else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(hi - lens).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(ent).cuda()
