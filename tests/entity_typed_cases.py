"""What the two typed per-entity GPU test files share: the untyped tests' shapes, tables and query entities, TypeConstraints with
the member counts of mine_typed_cases.LENGTHS (or built from triplets), the settings that pair a constraint with a filter, the
filter trap and the Python-set check of a returned list."""
import functools

import torch

from mine_typed_cases import LENGTHS, member_masks

SHAPES = [(150, 3, 20), (70, 7, 37), (200, 1, 200), (130, 5, 260)]      # (N, R, h): the untyped tests'
# (constraint, filtered): 'lengths' -- member counts 0 / 1 / 63 / 64 / 65 / full scattered over the ids, unrelated to the filter's
# triplets; 'same' -- constraint and filter from one triplet set (every listed id is a member); 'other' -- from two different sets
SETTINGS = [('lengths', False), ('lengths', True), ('same', True), ('other', True)]


def same(a, b):
    """Bit-for-bit equality of (rel, other, values) triples."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def pack(member):
    """(n_sets, n) bool -> int32 words (n_sets, ceil(n / 32)), entity j = bit j & 31 of word j >> 5."""
    n_sets, n = member.shape
    w = (n + 31) // 32
    pad = torch.zeros(n_sets, w * 32, dtype=torch.long)
    pad[:, :n] = member.long()
    words = (pad.view(n_sets, w, 32) << torch.arange(32)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def constraint_of(cand_subj, cand_obj):
    """A ranking.TypeConstraint on the GPU with exactly these members (bool (R, n) each): sets 0 .. R - 1 the objects, R .. 2 R - 1
    the subjects.  (Triplets cannot say 'subjects but no object'; the member counts that matter need it.)"""
    from gcn_vae_amd import ranking
    num_rels, n = cand_subj.shape
    tc = ranking.TypeConstraint(n, num_rels, device='cuda')
    dense = torch.cat([cand_obj, cand_subj])
    tc.words = pack(dense).cuda()
    tc.sizes = dense.sum(1).cuda()
    return tc


@functools.lru_cache(maxsize=None)
def tables(n, num_rels, h):
    """(emb, w) on the GPU, two triplet sets and a permutation of the entities on the CPU."""
    gen = torch.Generator().manual_seed(n * 31 + num_rels * 7 + h)
    emb = (torch.randn(n, h, generator=gen) * 0.5).cuda()
    w = torch.randn(num_rels, h, generator=gen).cuda()

    def triplets():
        return torch.stack([torch.randint(0, n, (n * num_rels // 2,), generator=gen),
                            torch.randint(0, num_rels, (n * num_rels // 2,), generator=gen),
                            torch.randint(0, n, (n * num_rels // 2,), generator=gen)], 1)
    return emb, w, triplets(), triplets(), torch.randperm(n, generator=gen)


def entities(perm, m):
    """m query entities: out of order, and with a repeat as soon as there are three."""
    ents = perm[:m].clone()
    if m >= 3:
        ents[m // 2] = ents[0]
    return ents.cuda()


@functools.lru_cache(maxsize=None)
def setting(n, num_rels, h, kind, filtered):
    """(type_constraint, filter_index or None, cand_subj, cand_obj) of one of SETTINGS; the masks on the CPU."""
    from gcn_vae_amd import ranking
    _, _, trip, trip2, _ = tables(n, num_rels, h)
    if kind == 'lengths':
        lengths = LENGTHS if num_rels > 1 else LENGTHS[1:]                    # a single relation: 63 subjects, 65 objects
        cs, co = member_masks(n, num_rels, torch.Generator().manual_seed(n + num_rels), lengths)
        tc = constraint_of(cs, co)
    else:
        tc = ranking.TypeConstraint(n, num_rels, trip if kind == 'same' else trip2, device='cuda')
        co, cs = tc.mask(torch.arange(num_rels)).cpu(), tc.mask(torch.arange(num_rels, 2 * num_rels)).cpu()
    fi = ranking.FilterIndex(n, num_rels, trip, device='cuda') if filtered else None
    return tc, fi, cs, co


def full_constraint(n, num_rels):
    return constraint_of(torch.ones(num_rels, n, dtype=torch.bool), torch.ones(num_rels, n, dtype=torch.bool))


def check_facts(ents, side, rel, other, cs, co, known=None):
    """Every returned fact is type-correct, not a loop and (with ``known``, a set of (s, r, o)) new; returns the facts."""
    a = ents.cpu().view(-1, 1).expand_as(rel)
    s, o = (a, other.cpu()) if side == 's' else (other.cpu(), a)
    facts = [t for t in zip(s.flatten().tolist(), rel.cpu().flatten().tolist(), o.flatten().tolist()) if t[1] >= 0]
    assert all(cs[r, x] and co[r, y] for x, r, y in facts)
    assert all(x != y for x, _, y in facts)
    if known is not None:
        assert not (set(facts) & known)
    return facts


def trap():
    """N = 200, two relations.  Relation 1's candidates: entity 5 and the entities 192 .. 199; the query entity 100 (on the query
    side of both relations) lists, under relation 1, the 128 non-members 64 .. 191 -- two windows of 64 between two members -- and
    the members 193 and 197.  Relation 0's candidates are the entities 0 .. 49, and 100 lists nothing there: 57 candidates in all,
    fewer than k = 128, so every one that is not hidden must come back.  Returns (n, R, query entity, cand_query, cand_other, listed
    triplets as (query entity, r, other), the members of relation 1 that must come back)."""
    n, num_rels, a = 200, 2, 100
    cq = torch.zeros(num_rels, n, dtype=torch.bool)
    cq[:, [a, 7]] = True
    co = torch.zeros(num_rels, n, dtype=torch.bool)
    co[0, :50] = True
    co[1, [5] + list(range(192, 200))] = True
    hidden = list(range(64, 192)) + [193, 197]
    listed = [(a, 1, x) for x in hidden] + [(7, 1, 5), (7, 0, 20)]
    return n, num_rels, a, cq, co, listed, [5, 192, 194, 195, 196, 198, 199]
