"""Shapes, pairs and relation filters shared by tests/test_gpu_relation.py and tests/test_gpu_transe_relation.py."""
import numpy as np
import torch

N = 300          # entities

# every m of {1, 63, 64, 65, 130} (partial and several row tiles), num_rels of {1, 11, 64, 65, 130, 237} (one partial tile, an exact
# tile, a tile boundary, several tiles), h of {7, 16, 24, 200} (200 is no multiple of the 16-wide k-chunk) and k of {1, 10, 128}
SHAPES = [(1, 1, 7, 1), (63, 11, 16, 10), (64, 64, 24, 128), (65, 65, 200, 10), (130, 130, 7, 128), (130, 237, 200, 10),
          (1, 237, 24, 128), (65, 11, 200, 1), (63, 130, 16, 1), (64, 1, 16, 10)]

KINDS = ['empty', 'few', 'straddle', 'window', 'long', 'target', 'shared', 'few']


def pairs(m, gen):
    """(s, o): repeats, s == o, id 0 and id N - 1 among them."""
    s, o = torch.randint(0, N, (m,), generator=gen), torch.randint(0, N, (m,), generator=gen)
    fixed = [(0, N - 1), (N - 1, 0), (5, 5), (0, N - 1), (N - 1, N - 1), (0, 0)]
    for i, (a, b) in enumerate(fixed[:m]):
        s[(i * 11) % m], o[(i * 11) % m] = a, b
    return s.cuda(), o.cuda()


def relation_lists(m, num_rels, target, gen, kinds=KINDS):
    """Per-pair sorted unique relation lists of the given kinds, cycled over the rows, packed into (lo, hi, rel) on the device."""
    out = []
    for i in range(m):
        kind = kinds[i % len(kinds)]
        if kind in ('empty', 'shared'):            # 'shared': pointed at row 1's range below
            e = np.zeros(0, dtype=np.int64)
        elif kind == 'few':
            e = np.unique(torch.randint(0, num_rels, (5,), generator=gen).numpy())
        elif kind == 'straddle':                   # across a 64-relation tile boundary (when there is one)
            c = 64 * int(torch.randint(1, max(2, num_rels // 64 + 1), (1,), generator=gen))
            e = np.arange(max(0, min(c, num_rels) - 3), min(num_rels, c + 3))
        elif kind == 'window':                     # one whole 64-relation window
            c = 64 * int(torch.randint(0, max(1, num_rels // 64), (1,), generator=gen))
            e = np.arange(c, min(num_rels, c + 64))
        elif kind == 'long':                       # all relations but two: fewer than k left
            e = np.sort(torch.randperm(num_rels, generator=gen)[:max(0, num_rels - 2)].numpy())
        elif kind == 'target':                     # the target itself is listed, among a few
            e = np.unique(np.append(torch.randint(0, num_rels, (3,), generator=gen).numpy(), int(target[i])))
        else:
            raise ValueError(kind)
        out.append(e)
    lens = np.array([len(e) for e in out], dtype=np.int64)
    hi = np.cumsum(lens)
    lo = hi - lens
    for i in range(m):
        if kinds[i % len(kinds)] == 'shared' and m > 1:
            lo[i], hi[i] = lo[1], hi[1]
    rel = np.concatenate(out) if lens.sum() else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda(), torch.from_numpy(rel).cuda()


def same_values(a, b):
    """Bit-for-bit equality of two float32 tensors."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_lists(a, b):
    """Bit-for-bit equality of (ids, values) pairs."""
    return torch.equal(a[0], b[0]) and same_values(a[1], b[1])


def gamma(j):
    u = 2.0 ** -24
    return j * u / (1.0 - j * u)


# ---- the CLIs' end-to-end cases: one data set, so that the two models' files have the same key columns ---------------------------
CLI_SPEC, CLI_K = 'synthetic:300:11:2000:100:120:3', 5


def check_relation_tsv(path, kg, k):
    """The file of --predict-relations, either model's: k lines per test triplet, in order, ``subject  object  position  relation
    value``.  The first three columns are fixed by the test split alone, so the two models' files join line by line on (subject,
    object, position), with a relation id -- or the padding's -1 -- in the fourth column of both: that is the join on the first
    four columns.  Inside a block the relations are distinct, none is a known relation of the pair, and padding comes last.
    Returns the rows."""
    rows = [line.rstrip('\n').split('\t') for line in open(path)]
    known = {(s, o, r) for s, r, o in np.concatenate([kg.train, kg.valid, kg.test]).tolist()}
    assert len(rows) == k * len(kg.test) and all(len(x) == 5 for x in rows)
    assert [x[:3] for x in rows] == [[str(s), str(o), str(p)] for s, _, o in kg.test.tolist() for p in range(k)]
    for at in range(0, len(rows), k):
        block = [int(x[3]) for x in rows[at:at + k]]
        real = [r for r in block if r >= 0]
        s, o = int(rows[at][0]), int(rows[at][1])
        assert block == real + [-1] * (k - len(real)) and len(set(real)) == len(real)
        assert all(0 <= r < kg.num_rels and (s, o, r) not in known for r in real)
        assert len(real) == min(k, kg.num_rels - sum(1 for r in range(kg.num_rels) if (s, o, r) in known))
    return rows
