"""What the two type-constrained mining GPU test files share: member lists with the lengths that matter (0, 1, 63, 64, 65, n), the
typed oracle -- mine_cases.brute_force with the known and the type-incorrect triplets as its excluded set, run ONCE per setting
for the whole ordered candidate list, from which every k and every threshold is read off -- and the checks against it."""
import numpy as np
import torch

from mine_cases import brute_force

# (subject members, object members) per relation, clipped to n; relation 0 has both sets full
LENGTHS = [(None, None), (63, 65), (64, 1), (0, 64), (65, 63), (1, None)]


def member_masks(n, num_rels, gen, lengths=LENGTHS):
    """(cand_subj, cand_obj) bool (R, n) on the CPU: random members of the listed counts, scattered over the whole id range."""
    cs, co = torch.zeros(num_rels, n, dtype=torch.bool), torch.zeros(num_rels, n, dtype=torch.bool)
    for r in range(num_rels):
        for mask, want in zip((cs, co), lengths[r % len(lengths)]):
            mask[r, torch.randperm(n, generator=gen)[:n if want is None else min(want, n)]] = True
    return cs, co


def member_lists(cs, co):
    """(ptr int64 [2 R + 1], ids int32) on the GPU: sets 0 .. R - 1 the objects, R .. 2 R - 1 the subjects, ascending."""
    dense = torch.cat([co, cs])
    ptr = torch.zeros(dense.shape[0] + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(dense.sum(1), 0)
    return ptr.cuda(), torch.nonzero(dense)[:, 1].to(torch.int32).cuda()


def excluded(cs, co, filt=None):
    """The oracle's excluded set: type-incorrect triplets, plus the listed ones of filt = (lo, hi, ent) over keys s * R + r."""
    num_rels = cs.shape[0]
    r, s, o = np.nonzero(~(cs[:, :, None] & co[:, None, :]).numpy())
    out = set(zip(s.tolist(), r.tolist(), o.tolist()))
    if filt is not None:
        lo, hi, ent = (t.cpu().tolist() for t in filt)
        for key, (a, b) in enumerate(zip(lo, hi)):
            out.update((key // num_rels, key % num_rels, x) for x in ent[a:b])
    return out


class Oracle:
    """brute_force's whole ordered candidate list for one setting; ``k`` / ``threshold`` read off it by the rule."""

    def __init__(self, val, ascending, excl, exclude_self):
        self.ascending = ascending
        inf = float('inf') if ascending else float('-inf')
        self.trip, self.values, _ = brute_force(val.cpu().numpy(), ascending, threshold=inf, filt=excl, exclude_self=exclude_self)

    def __len__(self):
        return self.values.numel()

    def _within(self, bound):
        return int((self.values <= bound).sum() if self.ascending else (self.values >= bound).sum())

    def top(self, k):
        if len(self) <= k:
            return self.trip, self.values, len(self)
        return self.trip[:k], self.values[:k], self._within(self.values[k - 1])

    def cut(self, threshold):
        m = self._within(threshold)
        return self.trip[:m], self.values[:m], m


def agrees(got, want):
    """A route's (triplets, values, info) against the oracle's (triplets, values, count), values as bit patterns."""
    return (torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu().view(torch.int32), want[1].view(torch.int32))
            and got[2]['count'] == want[2])


def check_against(oracle, mine, ks=(1, 10), thresholds=()):
    """``mine(k=...)`` / ``mine(threshold=...)`` against the oracle: k in {1, 10, more than the candidates}, the given thresholds
    and two read off the list."""
    for k in tuple(ks) + (len(oracle) + 5,):
        assert agrees(mine(k=k), oracle.top(k)), ('k', k)
    cuts = list(thresholds)
    if len(oracle):
        cuts += [float(oracle.values[len(oracle) // 2]), float(oracle.values[min(len(oracle) - 1, 100)])]
    for t in cuts:
        got = mine(threshold=t)
        assert agrees(got, oracle.cut(t)), ('threshold', t)
        assert got[2]['passes'] <= 1
