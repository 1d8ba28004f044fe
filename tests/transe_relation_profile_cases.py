"""What the two TransE per-relation completion test files share (test_transe_relation_profile_host.py without a GPU,
test_gpu_transe_relation_profile.py with one): the rule on distances as three Python loops per relation, and tables whose relations
live at scales 2^-6 .. 2^6."""
import numpy as np
import torch

from relation_profile_cases import brute_force


def brute_force_distances(dist, rels, k, filt=None, exclude_self=True, cand_subj=None, cand_obj=None):
    """For each relation of ``rels`` its candidates of dist[r, s, o] in the rule's order -- distance ascending, then (s, o) -- by
    relation_profile_cases' three Python loops on -dist: NaN dropped, +inf kept and last, a zero reported as +0.  Returns (subj
    (m, k), obj (m, k), dist (m, k), count [m]) padded with -1 / -1 / +inf."""
    subj, obj, neg, count = brute_force(-dist, rels, k, filt=filt, exclude_self=exclude_self, cand_subj=cand_subj, cand_obj=cand_obj)
    return subj, obj, 0.0 - neg, count


def scaled_tables(n, num_rels, dim, seed):
    """(en, rn, gen) on the CPU, to be passed un-normalised: entity rows of length 2^-10 and relation rows of EXACT scale -- unit
    rows times 1.5 * 2^e, e spread evenly over [-6, 6] -- so that a relation's distances all lie close to the length of its own
    translation vector.  The first histogram level has 8 bits, two binades a bin: relations whose exponents differ by two or more
    have their K-th distances in different first-level bins (the tests assert it on the distances they use), and ONE threshold for
    the whole graph serves the shortest relation only."""
    gen = torch.Generator().manual_seed(seed)
    en = torch.randn(n, dim, generator=gen)
    en = en / en.norm(dim=1, keepdim=True) * 2.0 ** -10
    rn = torch.randn(num_rels, dim, generator=gen)
    rn = rn / rn.norm(dim=1, keepdim=True)
    exps = torch.linspace(-6, 6, num_rels) if num_rels > 1 else torch.zeros(1)
    return en, rn * (1.5 * 2.0 ** exps).view(-1, 1), gen


def first_level_bins(dist_kth):
    """The first-level (8-bit) histogram bin of the key of -d for each distance of a float32 tensor: sign and the upper seven exponent
    bits."""
    u = (-dist_kth.detach().cpu().to(torch.float32)).numpy().view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    return (key >> 24).tolist()
