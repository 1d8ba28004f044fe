"""Raw-MRR evaluation with the reference's function names (kgvae/utils.py:180-221, :293-314).

The reference scores a batch against every entity by materialising a (h, Eb, V) outer-product
tensor and summing over h, adds ``flow_log_prob``, applies a sigmoid, sorts every row and looks the
target up.  Here ``ops.rank_scores`` (gv_rank_scores) forms (e_a * w_r) @ E^T + flow_log_prob tile by tile on the
f32 MFMA and counts, per query, the entities that beat the target -- the score matrix is never stored and
thousands of queries go through one launch.  Ranking is done on the LOGITS: the sigmoid is monotone, so tie-free
ranks equal the reference's sort-and-find, but it saturates (every candidate at 1.0f once the logits are large --
likely with ``flow_log_prob`` added to all of them), where the reference's rank is wherever ``torch.sort`` happens
to leave the target inside the tie block.  Ties are counted explicitly: rank = #better + #equal / 2 (the expected
position in such a block; ranks are floats), and a NaN target score (diverged run) ranks LAST -- never the
optimistic rank 1 that would make ``main`` keep a broken checkpoint as "best".
``perturb_and_get_rank_unfused`` keeps the materialised form (one GEMM + torch ops) as the in-repo cross-check.

Filtered evaluation (the protocol of published FB15k-237 / WN18RR figures; the reference reports raw ranks only,
kgvae/link_predict.py:7): a ``FilterIndex`` of the dataset's known triplets lists, per query, the OTHER true answers, and
``ops.rank_scores_filtered`` (gv_rank_scores_filtered) leaves them out of the count in the same launch that gives the raw
rank.  ``calc_filtered_mrr`` reports both.

Link prediction (what the reference's ``--generate`` demo did with an argmax, kgvae/utils.py:245-288): ``predict_topk`` returns
the k best entities of each query, optionally filtered by a ``FilterIndex``, from ``ops.topk_scores`` (gv_topk_scores: the same
logits, a selection epilogue instead of a count).  ``topk_from_scores`` states the order on a materialised score matrix.

Type-constrained evaluation and prediction (the second protocol of the reference's baseline tester,
baselines/transe/tester.py:70-91): a ``TypeConstraint`` holds, per relation and side, the bitmask of the entities seen there;
``ops.rank_scores_constrained`` ranks the target among those only -- raw, filtered and both constrained counts from one launch
pair -- and ``predict_topk(type_constraint=...)`` proposes members only.  ``rank_from_scores_constrained`` and
``topk_from_scores(cand=...)`` state the rules on a materialised score matrix.

Completion (no query list: which triplets are missing from the graph?): ``mine_triplets`` selects globally among all N x R x N
triplets -- the K most confident new ones, or all above a threshold -- from ``ops.mine_scores`` (gv_mine_scores: subject and
object tiles of the entity table stay in LDS while the relations are walked over them).  ``mine_from_scores`` states the rule on
a materialised (R, N, N) tensor; ``mine_triplets_unfused`` is the per-relation GEMM cross-check.

Per-entity completion (what is this entity missing? -- the question of the reference's ``--generate`` ego-net demo,
kgvae/utils.py:224-288): ``complete_entities`` returns each entity's k best new facts over ALL relations at once, the entity as
subject or as object, from ``ops.entity_topk_scores`` (gv_entity_topk_scores: one sorted list per entity while the relations are
walked, at ``predict_topk``'s logits).  ``complete_entities_from_scores`` states the rule on a materialised (m, R, N) tensor;
``complete_entities_unfused`` is the per-relation GEMM cross-check.

Monte-Carlo posterior predictive (the encoder is variational: one draw of the latents gives one of many possible rankings):
with S samples from ``KGVAE.posterior_samples``, ``calc_mc_mrr`` ranks and ``predict_topk_mc`` selects on
``pbar = mean_s sigmoid(logit_s)`` -- ``ops.rank_scores_mc`` / ``ops.topk_scores_mc`` loop over the samples around the same
score tile and keep pbar in registers -- and ``predict_topk_mc`` adds each proposal's spread over the samples.  pbar is a
probability, so it saturates and ties are real; they share the mid-rank.  ``mc_mean_prob`` / ``mc_ranks_from_probs`` state the
rule on materialised values; the ``*_mc_unfused`` routes are the per-sample GEMM cross-check.  ``mine_triplets_mc`` mines the
type-correct triplets on pbar, and ``complete_entities_mc`` is per-entity completion on it, typed or not
(``ops.entity_topk_scores_mc`` / ``ops.entity_topk_scores_typed_mc``: the sample loop inside each (relation, tile), one selection
per tile), with the mean and the spread of every returned fact; ``complete_entities_mc_from_probs`` states its rule on
materialised probabilities and ``complete_entities_mc_unfused`` is the cross-check.

Relation prediction (how are two entities related? -- the query is a pair (s, ?, o), the candidates are the relations):
``rank_relations`` / ``calc_relation_mrr`` rank the true relation among all relations, raw and -- with a ``PairFilterIndex`` of the
pairs' known relations -- filtered, and ``predict_relations`` proposes the k best new ones, from ``ops.pair_relation_scores``
(gv_pair_rel_scores: one launch, the product row e_s * e_o formed while it is staged, every relation tile walked by the workgroup
that owns the pairs).  ``relation_ranks_from_scores`` / ``topk_from_scores`` state the rules on a materialised (m, R) matrix; the
``*_unfused`` routes are the GEMM cross-check.  With a ``type_constraint`` the three also answer among the pair's TYPE-CORRECT
relations (s seen as subject of r and o as its object: the AND of two rows of ``TypeConstraint.relation_words``; four rank kinds),
and ``rank_relations_mc`` / ``calc_relation_mc_mrr`` / ``predict_relations_mc`` answer on the posterior predictive
(``ops.pair_relation_scores_mc``: the sample loop around each relation tile; ``predict_relations_mc`` adds the spread), typed or
not; ``pair_pbar_unfused`` is their materialised side.
"""
import torch

from . import ops


def mid_ranks(value, target, listed_mask=None, cand_mask=None):
    """The rank rule, once, on a materialised (m, v) matrix of values, higher is better (logits, probabilities, -distances), in
    plain torch: a candidate is better when ``~(value <= tgt)`` -- a NaN candidate or a NaN target never ranks the target well --,
    ties count half and the target itself is left out of every pool, member or not.  The pools: all entities; those not in
    ``listed_mask``; the members of ``cand_mask``; the members not listed (both masks dense (m, v) bools on ``value``'s device).
    Returns (raw, filtered, raw_constrained, filtered_constrained), 0-based float mid-ranks, None where a pool's mask is missing."""
    tgt = value.gather(1, target.view(-1, 1))
    other = torch.ones_like(value, dtype=torch.bool).scatter_(1, target.view(-1, 1), False)
    better, equal = (~(value <= tgt)) & other, (value == tgt) & other

    def rank(pool=None):
        b, e = (better, equal) if pool is None else (better & pool, equal & pool)
        return b.sum(dim=1).float() + 0.5 * e.sum(dim=1).float()
    keep = None if listed_mask is None else ~listed_mask
    return (rank(), None if keep is None else rank(keep), None if cand_mask is None else rank(cand_mask),
            None if keep is None or cand_mask is None else rank(cand_mask & keep))


def sort_and_rank(score, target):
    """0-based mid-rank of ``target`` in every row of a materialised (logit) score matrix; NaN never ranks well."""
    return mid_ranks(score, target)[0]


MAX_QUERY_ROWS = 16384      # queries per gv_rank_scores launch (bounds the (rows, h) query matrix, nothing else)


def _n_ranked(test_size, batch_size, all_batches):
    """How many queries a protocol ranks: all of them, or with ``all_batches=False`` the first batch only."""
    return min(test_size, batch_size) if all_batches is False else test_size


def _rank_chunks(n, step, a, r, b, filter_index, direction, device, n_kinds, rank_chunk, progress=None):
    """The chunk loop of every rank driver, once: the first ``n`` queries (a, r) with targets ``b`` go ``step`` at a time through
    ``rank_chunk(a, r, b, f_lo, f_hi, ent)`` -- the chunk's slices and its filter ranges into ``ent``, all three None without a
    ``filter_index`` --, which returns the chunk's ``n_kinds`` ranks in ``CONSTRAINED_KINDS``' order.  Returns one tensor per kind
    (empty float32 on ``device`` when there is nothing to rank); a filtered kind is None when the protocol has no filter.
    ``progress(hi, chunks)``, when given, is called after every chunk with the per-kind lists so far."""
    ent = filter_index.entities(direction, device) if filter_index is not None else None
    chunks = [[] for _ in range(n_kinds)]
    for lo in range(0, n, step):
        sl = slice(lo, min(n, lo + step))
        f_lo, f_hi = filter_index.lookup(a[sl], r[sl], direction) if filter_index is not None else (None, None)
        for acc, x in zip(chunks, rank_chunk(a[sl], r[sl], b[sl], f_lo, f_hi, ent)):
            acc.append(x)
        if progress is not None:
            progress(sl.stop, chunks)
    out = []
    for kind, x in enumerate(chunks):
        if filter_index is None and kind % 2:                 # a filtered kind of a protocol without a filter
            out.append(None)
        else:
            out.append(torch.cat(x) if x else torch.zeros(0, dtype=torch.float32, device=device))
    return tuple(out)


def _print_progress(head, label, ranks):
    x = 1.0 + torch.cat(ranks).float()
    print("{}: MR{} : {:.6f} |  MRR{} : {:.6f}".format(head, label, x.mean().item(), label, (1.0 / x).mean().item()))


def _queries(emb, w, a, r):
    """q = e_a * w_r of a chunk of queries."""
    return ops.mul(emb[a].contiguous(), w[r].contiguous())


def perturb_and_get_rank(embedding, w, a, r, b, test_size, batch_size=100, all_batches=True, flow_log_prob=None,
                         verbose=False):
    """Ranks of ``b`` for the queries (a, r).  ``batch_size`` only matters with ``all_batches=False`` (the reference's
    quick validation scores the first batch only, kgvae/utils.py:183-186): the fused scorer has no (h, Eb, V) tensor to bound."""
    n = _n_ranked(test_size, batch_size, all_batches)
    emb, wd = embedding.detach().contiguous(), w.detach()

    def rank_chunk(a, r, b, f_lo, f_hi, ent):
        return (ops.rank_scores(_queries(emb, wd, a, r), emb, b, flow_log_prob),)
    progress = (lambda hi, chunks: _print_progress("rows {} / {}".format(hi, n), "", chunks[0])) if verbose else None
    return _rank_chunks(n, MAX_QUERY_ROWS, a, r, b, None, None, emb.device, 1, rank_chunk, progress)[0]


def perturb_and_get_rank_unfused(embedding, w, a, r, b, test_size, batch_size=100, all_batches=True, flow_log_prob=None,
                                 verbose=False):
    n = _n_ranked(test_size, batch_size, all_batches)
    emb, wd = embedding.detach().contiguous(), w.detach()

    def rank_chunk(a, r, b, f_lo, f_hi, ent):
        score = ops.gemm(_queries(emb, wd, a, r), emb, trans_b=True)                  # (Eb, V)
        if flow_log_prob is not None:
            score = score + flow_log_prob
        return (sort_and_rank(score, b),)                         # on the logits (see the module docstring)
    n_batch = (n + batch_size - 1) // batch_size
    progress = None
    if verbose:
        progress = lambda hi, chunks: _print_progress("batch {} / {}".format((hi - 1) // batch_size, n_batch), "", chunks[0])
    return _rank_chunks(n, batch_size, a, r, b, None, None, emb.device, 1, rank_chunk, progress)[0]


class FilterIndex:
    """The known true answers of every (entity, relation) query in both directions, built once per dataset:
      'o'  object query (s, r, ?):  key s * num_rels + r -> the sorted unique objects o with (s, r, o) known
      's'  subject query (?, r, o): key o * num_rels + r -> the sorted unique subjects s with (s, r, o) known
    Keys are int64 (num_nodes * num_rels passes 2**31 on large graphs).  Per direction ``keys[d]`` (int64) and ``ent[d]`` (int32)
    are parallel arrays sorted by (key, entity): the answers of one key are a contiguous run of ``ent[d]``, which is exactly the
    (filt_lo, filt_hi, filt_ent) form ``ops.rank_scores_filtered`` takes.  Built with torch ops on ``device`` (CPU works too)."""

    def __init__(self, num_nodes, num_rels, *triplet_sets, device='cpu'):
        self.num_nodes, self.num_rels, self.device = int(num_nodes), int(num_rels), torch.device(device)
        parts = [torch.as_tensor(t).to(device=self.device, dtype=torch.long).reshape(-1, 3) for t in triplet_sets]
        trip = torch.cat(parts) if parts else torch.zeros(0, 3, dtype=torch.long, device=self.device)
        if trip.numel() and (int(trip[:, [0, 2]].min()) < 0 or int(trip[:, [0, 2]].max()) >= self.num_nodes
                             or int(trip[:, 1].min()) < 0 or int(trip[:, 1].max()) >= self.num_rels):
            raise ValueError('triplets out of range of num_nodes / num_rels')
        s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
        self.keys, self.ent = {}, {}
        for d, a, e in (('o', s, o), ('s', o, s)):
            key = a * self.num_rels + r
            order = torch.argsort(e, stable=True)
            order = order[torch.argsort(key[order], stable=True)]           # by (key, entity)
            k, x = key[order], e[order]
            keep = torch.ones_like(k, dtype=torch.bool)
            if k.numel() > 1:
                keep[1:] = (k[1:] != k[:-1]) | (x[1:] != x[:-1])              # duplicate triplets once
            self.keys[d], self.ent[d] = k[keep].contiguous(), x[keep].to(torch.int32).contiguous()
        if max(self.ent['o'].numel(), 1) >= 2 ** 31:
            raise ValueError('more than 2**31 - 1 distinct triplets')

    def lookup(self, a, r, direction):
        """(lo, hi): the range of ``ent[direction]`` holding the known answers of each query (a[i], r[i]), on ``a``'s device."""
        keys = self.keys[direction]
        q = a.to(device=self.device, dtype=torch.long) * self.num_rels + r.to(device=self.device, dtype=torch.long)
        lo = torch.searchsorted(keys, q, right=False)
        hi = torch.searchsorted(keys, q, right=True)
        return lo.to(a.device), hi.to(a.device)

    def entities(self, direction, device=None):
        return self.ent[direction] if device is None else self.ent[direction].to(device)


class TypeConstraint:
    """Per relation and side, the set of entities seen there in the given triplet sets, as one bitmask:
      set r             (direction 'o'): the entities seen as OBJECT of relation r   -- the candidates of a query (s, r, ?)
      set num_rels + r  (direction 's'): the entities seen as SUBJECT of relation r  -- the candidates of a query (?, r, o)
    ``words`` is int32 (2 * num_rels, W), W = ceil(num_nodes / 32): entity j is bit j & 31 of word j >> 5; bits at positions
    >= num_nodes are zero.  ``sizes`` (int64 [2 * num_rels]) counts the members.  Built with torch ops on ``device``."""

    def __init__(self, num_nodes, num_rels, *triplet_sets, device='cpu'):
        self.num_nodes, self.num_rels, self.device = int(num_nodes), int(num_rels), torch.device(device)
        parts = [torch.as_tensor(t).to(device=self.device, dtype=torch.long).reshape(-1, 3) for t in triplet_sets]
        trip = torch.cat(parts) if parts else torch.zeros(0, 3, dtype=torch.long, device=self.device)
        if trip.numel() and (int(trip[:, [0, 2]].min()) < 0 or int(trip[:, [0, 2]].max()) >= self.num_nodes
                             or int(trip[:, 1].min()) < 0 or int(trip[:, 1].max()) >= self.num_rels):
            raise ValueError('triplets out of range of num_nodes / num_rels')
        s, r, o = trip[:, 0], trip[:, 1], trip[:, 2]
        n_sets, n_words = 2 * self.num_rels, (self.num_nodes + 31) // 32
        # distinct (set, entity) pairs: each is one bit, so summing the bits of a word is OR-ing them
        pair = torch.unique(torch.cat([r * self.num_nodes + o, (self.num_rels + r) * self.num_nodes + s]))
        set_id, ent = pair // max(self.num_nodes, 1), pair % max(self.num_nodes, 1)
        self._pairs, self._relation_words = (set_id, ent), None              # (relation_words is built from them on first use)
        words = torch.zeros(n_sets * n_words, dtype=torch.long, device=self.device)
        words.index_add_(0, set_id * n_words + (ent >> 5), torch.ones_like(ent) << (ent & 31))
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)          # the uint32 bit pattern, held as int32
        self.words = words.to(torch.int32).view(n_sets, n_words).contiguous()
        self.sizes = torch.bincount(set_id, minlength=n_sets)

    def relation_words(self, device=None):
        """The sets seen from an entity: int32 (2 * num_nodes, ceil(num_rels / 32)), row e the relations entity e was SUBJECT of,
        row num_nodes + e those it was OBJECT of; relation r is bit r & 31 of word r >> 5, bits from num_rels on are zero.  The
        type-correct relations of a pair (s, o) are the AND of rows s and num_nodes + o -- what ``ops.pair_relation_scores(cand=)``
        reads, two words per side per 64-relation tile.  Built once, with torch ops, from the distinct (set, entity) pairs
        ``words`` is built from."""
        if self._relation_words is None:
            set_id, ent = self._pairs
            n_words = (self.num_rels + 31) // 32
            rel = set_id % max(self.num_rels, 1)
            row = torch.where(set_id >= self.num_rels, ent, self.num_nodes + ent)      # set R + r: subjects of r; set r: its objects
            words = torch.zeros(2 * self.num_nodes * n_words, dtype=torch.long, device=self.device)
            words.index_add_(0, row * n_words + (rel >> 5), torch.ones_like(rel) << (rel & 31))
            words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)      # the uint32 bit pattern, held as int32
            self._relation_words = words.to(torch.int32).view(2 * self.num_nodes, n_words).contiguous()
        return self._relation_words if device is None else self._relation_words.to(device)

    def pair_mask(self, s, o, device=None):
        """Dense (m, num_rels) bool: relation r is type-correct for the pair (s[i], o[i]) -- s[i] was seen as subject of r and
        o[i] as object of r.  Read off ``words`` (not ``relation_words``): the materialised twins' side of the cross-check."""
        s, o = (torch.as_tensor(t).to(device=self.device, dtype=torch.long).reshape(-1) for t in (s, o))
        rel = torch.arange(self.num_rels, device=self.device).view(1, -1)
        subj = (self.words[self.num_rels + rel, (s >> 5).view(-1, 1)] >> (s & 31).view(-1, 1)) & 1
        obj = (self.words[rel, (o >> 5).view(-1, 1)] >> (o & 31).view(-1, 1)) & 1
        dense = (subj & obj).bool()
        return dense if device is None else dense.to(device)

    def set_ids(self, r, direction):
        """int32 set id of each relation ``r[i]``: r for 'o' (object candidates), num_rels + r for 's' (subject candidates)."""
        if direction not in ('o', 's'):
            raise ValueError("direction is 'o' (queries (a, r, ?)) or 's' (queries (?, r, a))")
        r = torch.as_tensor(r)
        return (r + (self.num_rels if direction == 's' else 0)).to(torch.int32)

    def mask(self, set_ids, device=None):
        """Dense (m, num_nodes) bool of the members of each listed set; an id outside [0, 2 * num_rels) is the empty set."""
        ids = torch.as_tensor(set_ids).to(device=self.device, dtype=torch.long).reshape(-1)
        ok = (ids >= 0) & (ids < self.words.shape[0])
        rows = self.words[ids.clamp(0, max(self.words.shape[0] - 1, 0))] if self.words.shape[0] else self.words.new_zeros(ids.numel(), 0)
        ent = torch.arange(self.num_nodes, device=self.device)
        dense = ((rows[:, ent >> 5] >> (ent & 31)) & 1).bool() & ok.view(-1, 1)
        return dense if device is None else dense.to(device)

    def members(self, device=None):
        """Every set as a list: ``(ptr int64 [2 * num_rels + 1], ids int32 [total])``, set j's members ascending in
        ``ids[ptr[j]:ptr[j + 1]]`` -- the form the type-constrained miners take (``ops.mine_scores_typed``).  Torch ops on ``words``."""
        dense = self.mask(torch.arange(self.words.shape[0], device=self.device))
        ptr = torch.zeros(dense.shape[0] + 1, dtype=torch.int64, device=self.device)
        ptr[1:] = torch.cumsum(dense.sum(1), 0)
        ids = torch.nonzero(dense)[:, 1].to(torch.int32).contiguous()          # row-major: by set, then ascending entity
        return (ptr, ids) if device is None else (ptr.to(device), ids.to(device))

    def contains(self, r, entities, direction):
        """bool: is ``entities[i]`` a member of the ``direction`` set of relation ``r[i]``?  (On ``entities``' device.)"""
        entities = torch.as_tensor(entities)
        e = entities.to(device=self.device, dtype=torch.long)
        ids = self.set_ids(torch.as_tensor(r).to(self.device), direction).long()
        if e.numel() and (int(e.min()) < 0 or int(e.max()) >= self.num_nodes or int(ids.min()) < 0
                          or int(ids.max()) >= self.words.shape[0]):
            raise ValueError('entities / relations out of range of num_nodes / num_rels')
        return (((self.words[ids, e >> 5] >> (e & 31)) & 1).bool()).to(entities.device)


def rank_from_scores_constrained(score, target, cand_mask, listed_mask=None):
    """The rule of ``ops.rank_scores_constrained`` on a materialised (m, v) logit matrix, in plain torch (any device):
    ``sort_and_rank``'s predicates (NaN never optimistic, ties half) counted over four candidate pools, the target left out of
    every one whether or not it is a member: all entities; those not in ``listed_mask``; the members of ``cand_mask``; the
    members not listed.  Both masks are dense (m, v) bools.  Returns (raw, filtered, raw_constrained, filtered_constrained),
    0-based float mid-ranks; the two filtered ones are None without ``listed_mask``."""
    return mid_ranks(score, target, None if listed_mask is None else listed_mask.to(score.device), cand_mask.to(score.device))


def perturb_and_get_rank_constrained(embedding, w, a, r, b, test_size, filter_index, type_constraint, direction, batch_size=100,
                                     all_batches=True, flow_log_prob=None):
    """(raw, filtered, raw_constrained, filtered_constrained) ranks of ``b`` for the queries (a, r):
    ``perturb_and_get_rank_filtered`` plus the ranks among the ``direction`` type set of each query's relation only.
    ``filter_index`` may be None: the two filtered ranks are then None."""
    n = _n_ranked(test_size, batch_size, all_batches)
    emb, wd = embedding.detach().contiguous(), w.detach()
    words = type_constraint.words.to(emb.device)

    def rank_chunk(a, r, b, f_lo, f_hi, ent):
        return ops.rank_scores_constrained(_queries(emb, wd, a, r), emb, b, words, type_constraint.set_ids(r, direction), f_lo, f_hi,
                                           ent, flow_log_prob)
    return _rank_chunks(n, MAX_QUERY_ROWS, a, r, b, filter_index, direction, emb.device, 4, rank_chunk)


CONSTRAINED_KINDS = ('raw', 'filtered', 'raw_constrained', 'filtered_constrained')
MRR_LINES = ("MRR ({0}): {1:.6f}", "Hits ({0}) @ {1}: {2:.6f}")
MC_MRR_LINES = ("MC MRR ({0}, {n_samples} samples): {1:.6f}", "MC Hits ({0}) @ {1}: {2:.6f}")


def _on_device(embedding, w, flow_log_prob):
    """The reference validates with the model "on the CPU" (kgvae/link_predict.py:239-251): whatever side the caller's tensors
    are on, the scorer runs where the embedding is."""
    if isinstance(flow_log_prob, torch.Tensor):
        flow_log_prob = flow_log_prob.to(embedding.device)
    return w.to(embedding.device), flow_log_prob


def _both_directions(table, test_triplets, eval_bz, all_batches, rank):
    """The two query sets of a test split, on ``table``'s device: ``rank(a, r, b, n, direction)`` for the subjects given
    (o, r), then for the objects given (s, r); ``n`` is already cut to the first batch with ``all_batches=False``."""
    test_triplets = test_triplets.to(table.device)
    s, r, o = test_triplets[:, 0], test_triplets[:, 1], test_triplets[:, 2]
    n = _n_ranked(test_triplets.shape[0], eval_bz, all_batches)
    return rank(o, r, s, n, 's'), rank(s, r, o, n, 'o')


def _report(by_s, by_o, kinds, hits, verbose, lines, lead={}):
    """MRR and Hits@k of every kind over both directions: ``by_s`` / ``by_o`` hold the 0-based ranks of the first ``len(by_s)``
    of ``kinds``, one tensor each (None: not reported).  Returns ``lead``'s entries, then ``mrr_<kind>`` and
    ``hits_<kind>: {k: v}``; ``verbose`` prints them with the two format strings ``lines``."""
    out = dict(lead)
    for kind, rs, ro in zip(kinds, by_s, by_o):
        if rs is None:                                    # no filter_index: the filtered kinds are not reported
            continue
        ranks = torch.cat([rs, ro]) + 1
        out['mrr_' + kind] = torch.mean(1.0 / ranks.float()).item()
        out['hits_' + kind] = {hit: torch.mean((ranks <= hit).float()).item() for hit in hits}
    if verbose:
        for kind in (k for k in kinds if 'mrr_' + k in out):
            print(lines[0].format(kind, out['mrr_' + kind], **lead))
            for hit in hits:
                print(lines[1].format(kind, hit, out['hits_' + kind][hit]))
    return out


def calc_constrained_mrr(embedding, w, test_triplets, filter_index, type_constraint, hits=[1, 3, 10], eval_bz=100,
                         all_batches=True, flow_log_prob=None, verbose=True):
    """The four-way report of the type-constrained protocol over both directions: ``mrr_<kind>`` and ``hits_<kind>: {k: v}`` for
    raw, filtered, raw_constrained and filtered_constrained.  The first two equal ``calc_filtered_mrr``'s values."""
    with torch.no_grad():
        w, flow_log_prob = _on_device(embedding, w, flow_log_prob)
        by_s, by_o = _both_directions(embedding, test_triplets, eval_bz, all_batches, lambda a, r, b, n, d:
                                      perturb_and_get_rank_constrained(embedding, w, a, r, b, n, filter_index, type_constraint, d,
                                                                       eval_bz, all_batches, flow_log_prob))
        return _report(by_s, by_o, CONSTRAINED_KINDS, hits, verbose, MRR_LINES)


def perturb_and_get_rank_filtered(embedding, w, a, r, b, test_size, filter_index, direction, batch_size=100, all_batches=True,
                                  flow_log_prob=None, verbose=False):
    """(raw, filtered) ranks of ``b`` for the queries (a, r): ``perturb_and_get_rank`` with the known answers of each query left
    out of the filtered count.  ``direction`` 'o' when ``b`` are objects (queries (s, r, ?)), 's' when they are subjects."""
    n = _n_ranked(test_size, batch_size, all_batches)
    emb, wd = embedding.detach().contiguous(), w.detach()

    def rank_chunk(a, r, b, f_lo, f_hi, ent):
        return ops.rank_scores_filtered(_queries(emb, wd, a, r), emb, b, f_lo, f_hi, ent, flow_log_prob)
    progress = (lambda hi, chunks: _print_progress("rows {} / {}".format(hi, n), " (filtered)", chunks[1])) if verbose else None
    return _rank_chunks(n, MAX_QUERY_ROWS, a, r, b, filter_index, direction, emb.device, 2, rank_chunk, progress)


def calc_filtered_mrr(embedding, w, test_triplets, filter_index, hits=[1, 3, 10], eval_bz=100, all_batches=True,
                      flow_log_prob=None, verbose=True):
    """Raw and filtered MRR / Hits@k over both directions, from one scorer launch pair per chunk of queries.  Returns
    ``{'mrr_raw', 'mrr_filtered', 'hits_raw': {k: v}, 'hits_filtered': {k: v}}``; ``mrr_raw`` equals ``calc_mrr``'s value."""
    with torch.no_grad():
        w, flow_log_prob = _on_device(embedding, w, flow_log_prob)
        by_s, by_o = _both_directions(embedding, test_triplets, eval_bz, all_batches, lambda a, r, b, n, d:
                                      perturb_and_get_rank_filtered(embedding, w, a, r, b, n, filter_index, d, eval_bz, all_batches,
                                                                    flow_log_prob))
        return _report(by_s, by_o, CONSTRAINED_KINDS[:2], hits, verbose, MRR_LINES)


def _listed_mask(filt_lo, filt_hi, filt_ent, m, v, device):
    """Dense (m, v) bool: True where entity j is listed in row i's filter range."""
    lo, hi, ent = (t.reshape(-1).to(device=device, dtype=torch.long) for t in (filt_lo, filt_hi, filt_ent))
    lens = hi - lo
    total = int(lens.sum()) if m else 0
    mask = torch.zeros(m, v, dtype=torch.bool, device=device)
    if total:
        rows = torch.repeat_interleave(torch.arange(m, device=device), lens)
        first = torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
        idx = torch.repeat_interleave(lo, lens) + torch.arange(total, device=device) - first
        mask[rows, ent[idx]] = True
    return mask


def topk_from_scores(score, k, filt_lo=None, filt_hi=None, filt_ent=None, cand=None):
    """The top-k rule of ``ops.topk_scores`` on a materialised (m, v) logit matrix, in plain torch (any device): the ids listed
    in ``filt_ent[filt_lo[i]:filt_hi[i]]`` are no candidates of row i, nor are the columns where ``cand`` -- a dense (m, v) bool
    of allowed columns, the rule of ``ops.topk_scores_constrained`` -- is False; candidates go by logit descending, equal logits (-0 and
    +0 alike) by lower id, NaN after every other value (-inf included) and by id among themselves.  Returns ``(ids int64 (m, k),
    logits float32 (m, k))``, padded with id -1 / logit -inf past a row's last candidate; -0 is reported as +0 and every NaN
    as the one quiet NaN."""
    m, v = score.shape
    k = int(k)
    val = score.to(torch.float32) + 0.0                             # -0 -> +0
    nan = torch.isnan(val)
    val = torch.where(nan, torch.full_like(val, float('nan')), val)
    tier = nan.to(torch.int8)                                       # 0 a number, 1 NaN, 2 no candidate
    if filt_lo is not None:
        tier = torch.where(_listed_mask(filt_lo, filt_hi, filt_ent, m, v, val.device), torch.full_like(tier, 2), tier)
    if cand is not None:
        tier = torch.where(cand.to(val.device), tier, torch.full_like(tier, 2))
    by_logit = torch.argsort(torch.where(nan, torch.full_like(val, float('-inf')), val), dim=1, descending=True, stable=True)
    order = by_logit.gather(1, torch.argsort(tier.gather(1, by_logit), dim=1, stable=True))[:, :k]
    ids, logits = order.clone(), val.gather(1, order)
    gone = tier.gather(1, order) == 2
    ids[gone], logits[gone] = -1, float('-inf')
    if order.shape[1] < k:
        ids = torch.cat([ids, ids.new_full((m, k - order.shape[1]), -1)], 1)
        logits = torch.cat([logits, logits.new_full((m, k - order.shape[1]), float('-inf'))], 1)
    return ids, logits


def _predict_topk(embedding, w, a, r, k, direction, filter_index, select, type_constraint=None):
    if direction not in ('o', 's'):
        raise ValueError("direction is 'o' (queries (a, r, ?)) or 's' (queries (?, r, a))")
    emb = embedding.detach().contiguous()
    wd = w.detach()
    ent = filter_index.entities(direction, emb.device) if filter_index is not None else None
    ids, logits = [], []
    for lo in range(0, a.shape[0], MAX_QUERY_ROWS):
        hi = min(a.shape[0], lo + MAX_QUERY_ROWS)
        q = _queries(emb, wd, a[lo:hi], r[lo:hi])
        f_lo, f_hi = filter_index.lookup(a[lo:hi], r[lo:hi], direction) if filter_index is not None else (None, None)
        if type_constraint is None:
            i, l = select(q, emb, f_lo, f_hi, ent)
        else:
            i, l = select(q, emb, f_lo, f_hi, ent, type_constraint.set_ids(r[lo:hi], direction))
        ids.append(i)
        logits.append(l)
    if not ids:
        return (torch.zeros(0, k, dtype=torch.int64, device=emb.device),
                torch.zeros(0, k, dtype=torch.float32, device=emb.device))
    return torch.cat(ids), torch.cat(logits)


def predict_topk(embedding, w, a, r, k, direction='o', filter_index=None, flow_log_prob=None, type_constraint=None):
    """Link prediction: the ``k`` most likely entities of every query, ``direction`` 'o' for (a[i], r[i], ?) and 's' for
    (?, r[i], a[i]), scored as ``perturb_and_get_rank`` scores them (q = e_a * w_r, logit = q . e_j + flow_log_prob).  With a
    ``FilterIndex`` the query's known answers are left out (new facts only).  One fused launch pair per ``MAX_QUERY_ROWS``
    queries (ops.topk_scores); returns ``(ids int64 (n, k), logits float32 (n, k))`` in the order of ``topk_from_scores``.
    With a ``TypeConstraint`` only the members of the relation's ``direction`` type set are proposed
    (ops.topk_scores_constrained); rows with fewer than k such candidates are padded."""
    words = type_constraint.words.to(embedding.device) if type_constraint is not None else None

    def select(q, emb, f_lo, f_hi, ent, sets=None):
        if sets is None:
            return ops.topk_scores(q, emb, k, flow_log_prob, f_lo, f_hi, ent)
        return ops.topk_scores_constrained(q, emb, k, words, sets, flow_log_prob, f_lo, f_hi, ent)
    return _predict_topk(embedding, w, a, r, k, direction, filter_index, select, type_constraint)


def predict_topk_unfused(embedding, w, a, r, k, direction='o', filter_index=None, flow_log_prob=None, type_constraint=None):
    """``predict_topk`` from materialised logits (one GEMM + ``topk_from_scores`` per chunk): the in-repo cross-check and the
    bench's baseline."""
    def select(q, emb, f_lo, f_hi, ent, sets=None):
        score = ops.gemm(q, emb, trans_b=True, precision='f32')
        if flow_log_prob is not None:
            score = score + flow_log_prob
        return topk_from_scores(score, k, f_lo, f_hi, ent, None if sets is None else type_constraint.mask(sets, score.device))
    return _predict_topk(embedding, w, a, r, k, direction, filter_index, select, type_constraint)


# ---- Monte-Carlo posterior-predictive ranking and top-k --------------------------------------------------------------------
MC_STACK_ROWS = 4096        # queries per MC launch: bounds the (S, rows, h) query stack
MC_UNFUSED_ROWS = 1024      # queries per chunk of the materialised cross-check: bounds its (rows, v) matrices


def mc_mean_prob(z, w, a, r, flow_log_probs=None):
    """The posterior-predictive probability on materialised values, in the tensors' dtype (any device):
    ``pbar[i, j] = (sum_s sigmoid((z[s, a_i] * w[r_i]) . z[s, j] + flow_log_probs[s])) / S`` for the samples ``z`` (S, N, h),
    summed in ascending s.  Returns (len(a), N)."""
    total = None
    for s in range(z.shape[0]):
        logit = (z[s][a] * w[r]) @ z[s].T
        if flow_log_probs is not None:
            logit = logit + flow_log_probs[s]
        p = torch.sigmoid(logit)
        total = p if total is None else total + p
    return total / z.shape[0]


def mc_ranks_from_probs(pbar, target, listed_mask=None):
    """The rank rule of ``ops.rank_scores_mc`` on a materialised (m, v) matrix of probabilities: ``sort_and_rank``'s predicates
    (a NaN candidate or a NaN target counts as better, ties count half), the target itself left out; the filtered rank also
    leaves out the candidates of ``listed_mask`` (dense (m, v) bool), NaN ones included.  Returns ``(raw, filtered)``, 0-based
    float mid-ranks; ``filtered`` is None without a mask."""
    return mid_ranks(pbar, target.to(pbar.device), None if listed_mask is None else listed_mask.to(pbar.device))[:2]


def _mc_args(z, w, flow_log_probs):
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] < 1:
        raise ValueError('z: expected the (S, N, h) samples of KGVAE.posterior_samples, S >= 1')
    z = z.detach().contiguous()
    flp = None
    if flow_log_probs is not None:
        flp = torch.as_tensor(flow_log_probs).detach().reshape(-1).to(device=z.device, dtype=torch.float32)
        if flp.numel() != z.shape[0]:
            raise ValueError(f'flow_log_probs: one value per sample ({z.shape[0]}), got {flp.numel()}')
    return z, w.detach().to(z.device), flp


def _mc_queries(z, w, a, r):
    """Q_s = z_s[a] * w[r] for every sample, as one (S, rows, h) stack."""
    return ops.mul(z[:, a].contiguous(), w[r].unsqueeze(0).expand(z.shape[0], -1, -1).contiguous())


def _mc_pbar_unfused(z, w, a, r, flp):
    """pbar of a chunk of queries from one fp32 GEMM per sample (ops.gemm) + torch: (rows, N) float32."""
    total = None
    for s in range(z.shape[0]):
        score = ops.gemm(ops.mul(z[s][a].contiguous(), w[r].contiguous()), z[s], trans_b=True, precision='f32')
        if flp is not None:
            score = score + flp[s]
        p = torch.sigmoid(score)
        total = p if total is None else total + p
    return total * (1.0 / z.shape[0])


def _perturb_and_get_rank_mc(z, w, a, r, b, n, filter_index, direction, flp, fused, type_constraint=None):
    """The Monte-Carlo rank driver, fused or materialised: (raw, filtered), or with a ``type_constraint`` the four kinds."""
    words = type_constraint.words.to(z.device) if fused and type_constraint is not None else None

    def rank_chunk(a, r, b, f_lo, f_hi, ent):
        sets = type_constraint.set_ids(r, direction) if type_constraint is not None else None
        if fused:
            if sets is None:
                return ops.rank_scores_mc(_mc_queries(z, w, a, r), z, b, flp, f_lo, f_hi, ent)[:2]
            return ops.rank_scores_mc_constrained(_mc_queries(z, w, a, r), z, b, words, sets, flp, f_lo, f_hi, ent)[:4]
        pbar = _mc_pbar_unfused(z, w, a, r, flp)
        listed = None if ent is None else _listed_mask(f_lo, f_hi, ent, pbar.shape[0], pbar.shape[1], pbar.device)
        if sets is None:
            return mc_ranks_from_probs(pbar, b, listed)
        return rank_from_scores_constrained(pbar, b.to(pbar.device), type_constraint.mask(sets, pbar.device), listed)
    return _rank_chunks(n, MC_STACK_ROWS if fused else MC_UNFUSED_ROWS, a, r, b, filter_index, direction, z.device,
                        2 if type_constraint is None else 4, rank_chunk)


def perturb_and_get_rank_mc(z, w, a, r, b, test_size, filter_index=None, direction='o', batch_size=100, all_batches=True,
                            flow_log_probs=None):
    """(raw, filtered) posterior-predictive ranks of ``b`` for the queries (a, r) under the samples ``z`` (S, N, h): one fused
    launch pair per ``MC_STACK_ROWS`` queries (ops.rank_scores_mc).  ``filtered`` is None without a ``filter_index``."""
    z, w, flp = _mc_args(z, w, flow_log_probs)
    return _perturb_and_get_rank_mc(z, w, a, r, b, _n_ranked(test_size, batch_size, all_batches), filter_index, direction, flp, True)


def perturb_and_get_rank_mc_unfused(z, w, a, r, b, test_size, filter_index=None, direction='o', batch_size=100, all_batches=True,
                                    flow_log_probs=None):
    """``perturb_and_get_rank_mc`` from materialised probabilities (S GEMMs, sigmoids and a running sum per chunk, then
    ``mc_ranks_from_probs``): the in-repo cross-check and the bench's baseline."""
    z, w, flp = _mc_args(z, w, flow_log_probs)
    return _perturb_and_get_rank_mc(z, w, a, r, b, _n_ranked(test_size, batch_size, all_batches), filter_index, direction, flp, False)


def _calc_mc_mrr(z, w, test_triplets, filter_index, flow_log_probs, hits, eval_bz, all_batches, verbose, fused, type_constraint=None):
    with torch.no_grad():
        z, w, flp = _mc_args(z, w, flow_log_probs)
        by_s, by_o = _both_directions(z, test_triplets, eval_bz, all_batches, lambda a, r, b, n, d:
                                      _perturb_and_get_rank_mc(z, w, a, r, b, n, filter_index, d, flp, fused, type_constraint))
        return _report(by_s, by_o, CONSTRAINED_KINDS, hits, verbose, MC_MRR_LINES, {'n_samples': int(z.shape[0])})


def calc_mc_mrr(z, w, test_triplets, filter_index=None, flow_log_probs=None, hits=[1, 3, 10], eval_bz=100, all_batches=True,
                verbose=True):
    """Posterior-predictive MRR / Hits@k over both directions from the samples ``z`` (S, N, h) of ``KGVAE.posterior_samples``
    (``flow_log_probs``: its second result): every test triplet is ranked on ``pbar = mean_s sigmoid(logit_s)``.  Returns
    ``{'mrr_raw', 'hits_raw': {k: v}, 'n_samples'}`` and with a ``FilterIndex`` also ``'mrr_filtered'``, ``'hits_filtered'``, in
    the shape of ``calc_filtered_mrr``'s result.  For a fixed seed of the samples the figures are reproducible."""
    return _calc_mc_mrr(z, w, test_triplets, filter_index, flow_log_probs, hits, eval_bz, all_batches, verbose, True)


def calc_mc_mrr_unfused(z, w, test_triplets, filter_index=None, flow_log_probs=None, hits=[1, 3, 10], eval_bz=100,
                        all_batches=True, verbose=True):
    """``calc_mc_mrr`` on the materialised route (``perturb_and_get_rank_mc_unfused``)."""
    return _calc_mc_mrr(z, w, test_triplets, filter_index, flow_log_probs, hits, eval_bz, all_batches, verbose, False)


def perturb_and_get_rank_mc_constrained(z, w, a, r, b, test_size, filter_index, type_constraint, direction, batch_size=100,
                                        all_batches=True, flow_log_probs=None):
    """(raw, filtered, raw_constrained, filtered_constrained) posterior-predictive ranks of ``b`` for the queries (a, r) under the
    samples ``z`` (S, N, h): ``perturb_and_get_rank_mc`` plus the ranks among the ``direction`` type set of each query's relation
    only, all four on the same pbar (ops.rank_scores_mc_constrained, one fused launch pair per ``MC_STACK_ROWS`` queries).
    ``filter_index`` may be None: the two filtered ranks are then None."""
    z, w, flp = _mc_args(z, w, flow_log_probs)
    return _perturb_and_get_rank_mc(z, w, a, r, b, _n_ranked(test_size, batch_size, all_batches), filter_index, direction, flp, True,
                                    type_constraint)


def perturb_and_get_rank_mc_constrained_unfused(z, w, a, r, b, test_size, filter_index, type_constraint, direction, batch_size=100,
                                                all_batches=True, flow_log_probs=None):
    """``perturb_and_get_rank_mc_constrained`` from materialised probabilities (``_mc_pbar_unfused``, then
    ``rank_from_scores_constrained`` applied to pbar -- its predicates are the MC rule already): the in-repo cross-check and the
    bench's baseline."""
    z, w, flp = _mc_args(z, w, flow_log_probs)
    return _perturb_and_get_rank_mc(z, w, a, r, b, _n_ranked(test_size, batch_size, all_batches), filter_index, direction, flp, False,
                                    type_constraint)


def calc_mc_constrained_mrr(z, w, test_triplets, filter_index, type_constraint, flow_log_probs=None, hits=[1, 3, 10], eval_bz=100,
                            all_batches=True, verbose=True):
    """The four-way report of the type-constrained protocol on the posterior predictive, over both directions: ``n_samples`` and
    ``mrr_<kind>`` / ``hits_<kind>: {k: v}`` for the kinds of ``CONSTRAINED_KINDS`` (the filtered ones only with a
    ``FilterIndex``).  Every kind ranks on ``calc_mc_mrr``'s pbar: the raw and filtered figures equal its values."""
    return _calc_mc_mrr(z, w, test_triplets, filter_index, flow_log_probs, hits, eval_bz, all_batches, verbose, True, type_constraint)


def calc_mc_constrained_mrr_unfused(z, w, test_triplets, filter_index, type_constraint, flow_log_probs=None, hits=[1, 3, 10],
                                    eval_bz=100, all_batches=True, verbose=True):
    """``calc_mc_constrained_mrr`` on the materialised route (``perturb_and_get_rank_mc_constrained_unfused``)."""
    return _calc_mc_mrr(z, w, test_triplets, filter_index, flow_log_probs, hits, eval_bz, all_batches, verbose, False, type_constraint)


def _predict_topk_mc(z, w, a, r, k, direction, filter_index, flow_log_probs, fused, type_constraint=None):
    if direction not in ('o', 's'):
        raise ValueError("direction is 'o' (queries (a, r, ?)) or 's' (queries (?, r, a))")
    z, w, flp = _mc_args(z, w, flow_log_probs)
    ent = filter_index.entities(direction, z.device) if filter_index is not None else None
    words = type_constraint.words.to(z.device) if fused and type_constraint is not None else None
    ids, mean, std = [], [], []
    step = MC_STACK_ROWS if fused else MC_UNFUSED_ROWS
    for lo in range(0, a.shape[0], step):
        sl = slice(lo, min(a.shape[0], lo + step))
        f_lo, f_hi = filter_index.lookup(a[sl], r[sl], direction) if filter_index is not None else (None, None)
        sets = type_constraint.set_ids(r[sl], direction) if type_constraint is not None else None
        if fused:
            q = _mc_queries(z, w, a[sl], r[sl])
            if sets is None:
                i, p = ops.topk_scores_mc(q, z, k, flp, f_lo, f_hi, ent)
            else:
                i, p = ops.topk_scores_mc_constrained(q, z, k, words, sets, flp, f_lo, f_hi, ent)
            sd = ops.pair_prob_std_mc(q, z, i, flp)
        else:
            pbar = _mc_pbar_unfused(z, w, a[sl], r[sl], flp)
            i, p = topk_from_scores(pbar, k, f_lo, f_hi, ent, cand=None if sets is None else type_constraint.mask(sets, pbar.device))
            pick = i.clamp(min=0)
            ps = []
            for s in range(z.shape[0]):        # the selected pairs' probability in every sample, from the same GEMMs
                score = ops.gemm(ops.mul(z[s][a[sl]].contiguous(), w[r[sl]].contiguous()), z[s], trans_b=True, precision='f32')
                ps.append(torch.sigmoid(score if flp is None else score + flp[s]).gather(1, pick))
            sd = torch.stack(ps).std(dim=0, unbiased=False)
            sd[i < 0] = 0.0
        ids.append(i)
        mean.append(p)
        std.append(sd)
    if not ids:
        f32 = dict(dtype=torch.float32, device=z.device)
        return torch.zeros(0, k, dtype=torch.int64, device=z.device), torch.zeros(0, k, **f32), torch.zeros(0, k, **f32)
    return torch.cat(ids), torch.cat(mean), torch.cat(std)


def predict_topk_mc(z, w, a, r, k, direction='o', filter_index=None, flow_log_probs=None, type_constraint=None):
    """Posterior-predictive link prediction from the samples ``z`` (S, N, h): the ``k`` entities of highest
    ``pbar = mean_s sigmoid(logit_s)`` for every query (``direction`` and ``filter_index`` as ``predict_topk`` takes them), and
    how sure the model is of each: returns ``(ids int64 (n, k), prob_mean float32 (n, k), prob_std float32 (n, k))``,
    ``prob_std`` the population standard deviation of the pair's probability over the samples.  Rows with fewer than k
    candidates are padded with id -1, mean -inf, std 0.  One fused launch pair plus the spread kernel per ``MC_STACK_ROWS``
    queries (ops.topk_scores_mc, ops.pair_prob_std_mc).  With a ``TypeConstraint`` only the members of the relation's
    ``direction`` type set are proposed (ops.topk_scores_mc_constrained); the spread is computed as before, on the selected ids."""
    return _predict_topk_mc(z, w, a, r, k, direction, filter_index, flow_log_probs, True, type_constraint)


def predict_topk_mc_unfused(z, w, a, r, k, direction='o', filter_index=None, flow_log_probs=None, type_constraint=None):
    """``predict_topk_mc`` from materialised probabilities (S GEMMs per chunk + ``topk_from_scores``): the in-repo cross-check
    and the bench's baseline."""
    return _predict_topk_mc(z, w, a, r, k, direction, filter_index, flow_log_probs, False, type_constraint)


MineOverflow = ops.MineOverflow


def _mine_args(k, threshold, max_results):
    if (k is None) == (threshold is None):
        raise ValueError('give exactly one of k and threshold')
    if k is not None and int(k) < 1:
        raise ValueError(f'k must be >= 1, got {k}')
    if threshold is not None and float(threshold) != float(threshold):
        raise ValueError('threshold is NaN')
    if int(max_results) < 1:
        raise ValueError(f'max_results must be >= 1, got {max_results}')


def _mine_from_values(val, ascending, *, k=None, threshold=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                     max_results=ops.MINE_MAX_RESULTS, cand_subj=None, cand_obj=None):
    """The mining rule, once, on a materialised tensor ``val[r, s, o]`` (R, N, N) in plain torch: logits, largest first, or
    (``ascending``) distances, smallest first.  ``mine_from_scores`` and ``transe.mine_from_distances`` state it for each.
    ``cand_subj`` / ``cand_obj`` (dense bool (R, N), each optional): the typed rule -- (s, r, o) is a candidate only when
    ``cand_subj[r, s]`` and ``cand_obj[r, o]``; everything else is unchanged."""
    _mine_args(k, threshold, max_results)
    num_rels, n = val.shape[0], val.shape[1]
    val = val.to(torch.float32) + 0.0
    within = torch.le if ascending else torch.ge          # at the bound or better
    cand = ~torch.isnan(val)
    for name, side, shape in (('cand_subj', cand_subj, (num_rels, n, 1)), ('cand_obj', cand_obj, (num_rels, 1, n))):
        if side is not None:
            if side.dtype != torch.bool or tuple(side.shape) != (num_rels, n):
                raise ValueError(f'{name}: expected a bool ({num_rels}, {n}) mask')
            cand &= side.to(val.device).view(shape)
    if exclude_self:
        cand &= ~torch.eye(n, dtype=torch.bool, device=val.device).unsqueeze(0)
    if filt_lo is not None and n:
        listed = _listed_mask(filt_lo, filt_hi, filt_ent, n * num_rels, n, val.device)      # rows: key s * R + r
        cand &= ~listed.view(n, num_rels, n).permute(1, 0, 2)
    if k is not None:
        vals = val[cand]
        if vals.numel() > int(k):
            cand &= within(val, torch.topk(vals, int(k), largest=not ascending).values[-1])
    else:
        cand &= within(val, float(threshold))
    r, s, o = torch.nonzero(cand, as_tuple=True)
    return _mine_finish(torch.stack([s, r, o], 1), val[cand], {'passes': 0}, k, threshold, max_results, n, num_rels, ascending)


def _mine_finish(trip, values, info, k, threshold, max_results, n, num_rels, ascending):
    """The end of both host routes: the candidates at the bound or better into the rule's order, counted, capped."""
    if k is not None:
        trip, values, info['count'] = ops.mine_select(trip, values, int(k), int(max_results), n, num_rels, ascending)
        return trip, values, info
    info['count'] = int(values.numel())
    if info['count'] > int(max_results):
        raise MineOverflow(info['count'], max_results, f'threshold {float(threshold)}')
    return ops.mine_order(trip, values, n, num_rels, ascending) + (info,)


def mine_from_scores(score, *, k=None, threshold=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                     max_results=ops.MINE_MAX_RESULTS, cand_subj=None, cand_obj=None):
    """The mining rule of ``ops.mine_scores`` on a materialised tensor ``score[r, s, o]`` (R, N, N), in plain torch (any device,
    CPU included).  Candidates: every (s, r, o), less ``filt_ent[filt_lo[s * R + r]:filt_hi[s * R + r]]`` as objects of (s, r),
    less s == o when ``exclude_self``, less NaN logits.  Order, a strict total one: logit descending with -0 == +0, then
    (s, r, o) ascending.  ``threshold=t`` selects every candidate with logit >= t, ``k=K`` the first K (fewer if fewer exist).
    Returns ``(triplets int64 (n, 3), logits float32 (n,), info)`` in that order, -0 reported as +0; ``info['count']`` is the
    number of candidates at or above the threshold (top-K: at or above the K-th logit's exact value; all, when fewer than K
    exist).  More than ``max_results`` of those raise ``MineOverflow`` carrying the count: nothing is truncated silently.
    ``cand_subj`` / ``cand_obj`` (bool (R, N)): the typed rule of ``ops.mine_scores_typed``, s among ``cand_subj[r]`` and o among
    ``cand_obj[r]`` (``TypeConstraint.mask`` of sets R + r and r)."""
    return _mine_from_values(score, False, k=k, threshold=threshold, filt_lo=filt_lo, filt_hi=filt_hi, filt_ent=filt_ent,
                            exclude_self=exclude_self, max_results=max_results, cand_subj=cand_subj, cand_obj=cand_obj)


def _mine_filter(filter_index, n, num_rels, device, direction='o'):
    """(lo, hi, ent) of ALL N * R object-query keys s * R + r: one searchsorted over the index (``direction`` 's': the subject-query
    keys o * R + r and their known subjects)."""
    if filter_index is None:
        return None, None, None
    if filter_index.num_nodes != n or filter_index.num_rels != num_rels:
        raise ValueError(f'the FilterIndex is for {filter_index.num_nodes} entities / {filter_index.num_rels} relations, the tables '
                         f'have {n} / {num_rels}')
    a = torch.arange(n, device=device).repeat_interleave(num_rels)
    r = torch.arange(num_rels, device=device).repeat(n)
    lo, hi = filter_index.lookup(a, r, direction)
    return lo, hi, filter_index.entities(direction, device)


def _mine_members_sizes(type_constraint, n, num_rels):
    """A ``TypeConstraint`` built for other sizes than the tables' is refused."""
    if type_constraint.num_nodes != n or type_constraint.num_rels != num_rels:
        raise ValueError(f'the TypeConstraint is for {type_constraint.num_nodes} entities / {type_constraint.num_rels} relations, the '
                         f'tables have {n} / {num_rels}')


def _mine_members(type_constraint, n, num_rels, device):
    """(ptr, ids) of ``TypeConstraint.members`` on ``device`` for tables of these sizes."""
    _mine_members_sizes(type_constraint, n, num_rels)
    return type_constraint.members(device)


def _mine_bias(flow_log_prob, device):
    if flow_log_prob is None:
        return None
    return torch.as_tensor(flow_log_prob, dtype=torch.float32).detach().to(device).reshape(1)


def mine_triplets(embedding, w, *, k=None, threshold=None, filter_index=None, flow_log_prob=None, exclude_self=True,
                  max_results=ops.MINE_MAX_RESULTS, type_constraint=None):
    """Knowledge-graph completion: among ALL triplets (s, r, o), scored as every scorer here scores them (logit =
    (e_s * w_r) . e_o + flow_log_prob), the ``k`` most confident ones or every one with logit >= ``threshold`` (a probability p
    is the logit log(p / (1 - p))); with a ``FilterIndex`` the known triplets are left out (new facts only).  One fused sweep
    per pass (ops.mine_scores); returns ``(triplets int64 (n, 3), logits float32 (n,), info)`` in the order of
    ``mine_from_scores``, and raises ``MineOverflow`` rather than truncating.  With a ``type_constraint`` (TypeConstraint) only
    type-correct triplets are candidates -- s seen as subject of r, o seen as object of r -- at the same logits, from the sweep
    over each relation's member lists (ops.mine_scores_typed)."""
    _mine_args(k, threshold, max_results)
    emb = embedding.detach()
    wd = w.detach().to(emb.device)
    lo, hi, ent = _mine_filter(filter_index, emb.shape[0], wd.shape[0], emb.device)
    if type_constraint is not None:
        set_ptr, set_ids = _mine_members(type_constraint, emb.shape[0], wd.shape[0], emb.device)
        return ops.mine_scores_typed(emb, wd, set_ptr, set_ids, threshold=threshold, k=k, bias=_mine_bias(flow_log_prob, emb.device),
                                     filt_lo=lo, filt_hi=hi, filt_ent=ent, exclude_self=exclude_self, max_results=max_results)
    return ops.mine_scores(emb, wd, threshold=threshold, k=k, bias=_mine_bias(flow_log_prob, emb.device), filt_lo=lo, filt_hi=hi,
                           filt_ent=ent, exclude_self=exclude_self, max_results=max_results)


def _mine_unfused(values_of, ascending, n, num_rels, device, *, k, threshold, filt, exclude_self, max_results, members=None):
    """The unfused route of both models, one relation at a time: ``values_of(r)`` is relation r's (N, N) values (logits, or
    distances when ``ascending``), ``filt`` the (lo, hi, ent) of ``_mine_filter``; torch selection, a running K-th value pruning
    the pool.  With ``members`` = (ptr, ids) of ``TypeConstraint.members`` the typed route: ``values_of(r, subj, obj)`` is the
    (|subj|, |obj|) block of relation r's member lists, selected the same way, local indices mapped back through the lists."""
    lo, hi, ent = filt
    k = None if k is None else int(k)
    bound = None if k is not None else float(threshold)
    within = torch.le if ascending else torch.ge          # at the bound or better
    pool_t, pool_v, held = [], [], 0
    typed = members is not None
    diag = torch.eye(n, dtype=torch.bool, device=device) if exclude_self and not typed else None
    if typed:
        set_ptr, set_ids = members[0].tolist(), members[1].to(device).long()

    def prune():
        nonlocal pool_t, pool_v, held, bound
        t, v = torch.cat(pool_t), torch.cat(pool_v)
        if v.numel() > k:
            bound = float(torch.topk(v, k, largest=not ascending).values[-1])
            keep = within(v, bound)
            t, v = t[keep], v[keep]
        pool_t, pool_v, held = [t], [v], v.numel()

    for r in range(num_rels if n else 0):
        if typed:
            subj, obj = set_ids[set_ptr[num_rels + r]:set_ptr[num_rels + r + 1]], set_ids[set_ptr[r]:set_ptr[r + 1]]
            if not subj.numel() or not obj.numel():
                continue
            val = values_of(r, subj, obj)
            f_lo, f_hi = (lo[r::num_rels][subj], hi[r::num_rels][subj]) if lo is not None else (None, None)
        else:
            val = values_of(r)
            f_lo, f_hi = (lo[r::num_rels], hi[r::num_rels]) if lo is not None else (None, None)
        cand = ~torch.isnan(val)
        if diag is not None:
            cand &= ~diag
        elif exclude_self:
            cand &= subj.view(-1, 1) != obj.view(1, -1)
        if lo is not None:
            listed = _listed_mask(f_lo, f_hi, ent, val.shape[0], n, device)
            cand &= ~(listed[:, obj] if typed else listed)
        if bound is not None:
            cand &= within(val, bound)
        if k is not None and bound is None:           # no bound yet: this relation's own K-th value
            vals = val[cand]
            if vals.numel() > k:
                cand &= within(val, torch.topk(vals, k, largest=not ascending).values[-1])
        s, o = torch.nonzero(cand, as_tuple=True)
        if typed:
            s, o = subj[s], obj[o]
        pool_t.append(torch.stack([s, torch.full_like(s, r), o], 1))
        pool_v.append(val[cand])
        held += s.numel()
        if k is not None and held > max(4 * k, 1 << 20):
            prune()
    trip = torch.cat(pool_t) if pool_t else torch.zeros(0, 3, dtype=torch.int64, device=device)
    values = torch.cat(pool_v) if pool_v else torch.zeros(0, dtype=torch.float32, device=device)
    return _mine_finish(trip, values, {'passes': num_rels}, k, threshold, max_results, n, num_rels, ascending)


def mine_triplets_unfused(embedding, w, *, k=None, threshold=None, filter_index=None, flow_log_prob=None, exclude_self=True,
                          max_results=ops.MINE_MAX_RESULTS, type_constraint=None):
    """``mine_triplets`` from materialised logits, one relation at a time (``ops.mul`` + ``ops.gemm`` + torch selection, a running
    K-th logit pruning the pool): the in-repo cross-check and the bench's baseline, never a fallback.  With a ``type_constraint``
    the relation's subject and object members are ``index_select``-ed first and the GEMM is (|subjects|, h) x (h, |objects|)."""
    _mine_args(k, threshold, max_results)
    emb = embedding.detach().contiguous()
    wd = w.detach().to(emb.device).contiguous()
    n, num_rels = emb.shape[0], wd.shape[0]
    filt = _mine_filter(filter_index, n, num_rels, emb.device)
    bias = _mine_bias(flow_log_prob, emb.device)
    members = None if type_constraint is None else _mine_members(type_constraint, n, num_rels, emb.device)

    def logits_of(r, subj=None, obj=None):
        a, b = (emb, emb) if subj is None else (emb.index_select(0, subj), emb.index_select(0, obj))
        val = ops.gemm(ops.mul(a, wd[r].expand_as(a).contiguous()), b, trans_b=True, precision='f32')
        if bias is not None:
            val = val + bias
        return val + 0.0

    return _mine_unfused(logits_of, False, n, num_rels, emb.device, k=k, threshold=threshold, filt=filt, exclude_self=exclude_self,
                        max_results=max_results, members=members)


# ---- per-entity completion: what is this entity missing? ------------------------------------------------------------------------
COMPLETE_UNFUSED_ELEMS = 1 << 26      # logits per chunk of the materialised cross-check: bounds its (rows, R, N) tensor


def complete_entities_from_scores(score, entities, k, *, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                                  cand_query=None, cand_other=None):
    """The rule of ``ops.entity_topk_scores`` on a materialised (m, R, N) logit tensor, in plain torch (any device): row i belongs
    to entity ``entities[i]``, its candidates are all (r, x) less the ids ``filt_ent[filt_lo[a * R + r]:filt_hi[a * R + r]]``
    under relation r (the dense per-key ranges of ``_mine_filter``) and less ``x == a`` with ``exclude_self``; they go by logit
    descending, equal logits (-0 and +0 alike) by relation, then by entity, NaN after every other value.  Returns ``(rel int64
    (m, k), other int64 (m, k), logits float32 (m, k))``, padded with -1 / -1 / -inf; -0 is reported as +0 and every NaN as the
    one quiet NaN.  ``topk_from_scores`` on the (m, R * N) view: the id r * N + x already says relation first, then entity.
    ``cand_query`` / ``cand_other`` (bool (R, N), given together): the typed rule of ``ops.entity_topk_scores_typed`` -- (r, x) is
    a candidate of entity a only with ``cand_query[r, a]`` and ``cand_other[r, x]`` (``complete_masks`` makes them of a
    ``TypeConstraint``); an entity outside [0, N) then has no candidate at all."""
    m, num_rels, n = score.shape
    ents = torch.as_tensor(entities, dtype=torch.long, device=score.device).reshape(-1)
    if ents.numel() != m:
        raise ValueError('one query entity per row of the score tensor')
    allowed = torch.ones(m, num_rels, n, dtype=torch.bool, device=score.device)
    if (cand_query is None) != (cand_other is None):
        raise ValueError('cand_query and cand_other are given together or not at all')
    if cand_query is not None:
        cq, co = (torch.as_tensor(c, dtype=torch.bool, device=score.device) for c in (cand_query, cand_other))
        if tuple(cq.shape) != (num_rels, n) or tuple(co.shape) != (num_rels, n):
            raise ValueError(f'cand_query / cand_other: expected bool ({num_rels}, {n})')
        inside = (ents >= 0) & (ents < n)
        ents = ents.clamp(0, n - 1)                  # an entity outside the table: every candidate is denied here
        allowed &= (cq[:, ents].t() & inside.view(-1, 1)).view(m, num_rels, 1) & co.view(1, num_rels, n)
    if filt_lo is not None:
        keys = (ents.view(-1, 1) * num_rels + torch.arange(num_rels, device=score.device)).reshape(-1)
        lo, hi = filt_lo.reshape(-1).to(score.device)[keys], filt_hi.reshape(-1).to(score.device)[keys]
        allowed &= ~_listed_mask(lo, hi, filt_ent.to(score.device), m * num_rels, n, score.device).view(m, num_rels, n)
    if exclude_self and m:
        allowed[torch.arange(m, device=score.device), :, ents] = False
    ids, logits = topk_from_scores(score.reshape(m, num_rels * n), k, cand=allowed.view(m, num_rels * n))
    gone = ids < 0
    return torch.where(gone, ids, ids // n), torch.where(gone, ids, ids % n), logits


class _Unconstrained:
    """The default of ``complete_entities(type_constraint=)``: no constraint was given."""

    def __repr__(self):
        return 'UNCONSTRAINED'


UNCONSTRAINED = _Unconstrained()


def _complete_constraint(type_constraint):
    """The ``type_constraint`` argument of the per-entity routes: None when it was left at its default ``UNCONSTRAINED``, else the
    ``TypeConstraint`` given.  Anything else is a TypeError -- an explicit None too: the unconstrained call is the one that does not
    name the argument, as it was before the argument existed."""
    if type_constraint is UNCONSTRAINED:
        return None
    if not isinstance(type_constraint, TypeConstraint):
        raise TypeError(f'type_constraint: expected a ranking.TypeConstraint, got {type(type_constraint).__name__} (leave the argument '
                        f'out for the unconstrained call)')
    return type_constraint


def _complete_side(side):
    """The one refusal of a per-entity route's ``side``."""
    if side not in ('s', 'o'):
        raise ValueError("side is 's' (the entity as subject: new facts (a, r, x)) or 'o' (as object: new facts (x, r, a))")


def complete_masks(type_constraint, side, device=None):
    """``(cand_query, cand_other)``, bool (R, N) each, of a ``TypeConstraint`` for per-entity completion on ``side``: 's' (facts
    (a, r, x)) asks a among the subjects of r (set R + r) and x among its objects (set r); 'o' (facts (x, r, a)) the other way
    round -- ``mine_triplets(type_constraint=)``'s definition of type-correct, seen from one entity."""
    _complete_side(side)
    num_rels = type_constraint.num_rels
    obj = type_constraint.mask(torch.arange(num_rels), device)
    subj = type_constraint.mask(torch.arange(num_rels, 2 * num_rels), device)
    return (subj, obj) if side == 's' else (obj, subj)


def _complete_args(embedding, w, entities, k, side, filter_index):
    """What the two routes of ``complete_entities`` check and prepare alike: (emb, w, entities, k, (lo, hi, ent))."""
    _complete_side(side)
    k = ops._topk_arg(k)
    emb = embedding.detach()
    wd = w.detach().to(emb.device)
    ents, filt = _complete_queries(emb, wd, entities, side, filter_index)
    return emb, wd, ents, k, filt


def _complete_queries(table, w, entities, side, filter_index, mc=False):
    """The second half of every per-entity route's preparation, once side and k stand and the model's tables are at hand (``mc``:
    ``table`` is the sample stack): the entities on the tables' device, checked with the operands' shapes, and the filter.  Returns
    (entities, (lo, hi, ent))."""
    ents = torch.as_tensor(entities, device=table.device).reshape(-1)
    (ops._entity_topk_mc_operands if mc else ops._entity_topk_operands)(ents, table, w)
    # the entity as subject asks for objects: the filter of the object queries (a, r, ?), and the other way round
    return ents, _mine_filter(filter_index, table.shape[-2], w.shape[0], table.device, 'o' if side == 's' else 's')


def _complete_mask_args(type_constraint, side, n, num_rels, device):
    """The typed rule of the ``*_unfused`` routes as the keywords by which ``complete_entities_from_scores`` takes it: the masks of
    ``complete_masks``, refused when the constraint was built for other sizes than the tables'; {} without a constraint."""
    if type_constraint is None:
        return {}
    _mine_members_sizes(type_constraint, n, num_rels)
    return dict(zip(('cand_query', 'cand_other'), complete_masks(type_constraint, side, device)))


def _complete_unfused(chunk, ents, rows, k, n_values=1):
    """The chunk loop of the three ``*_unfused`` routes: ``chunk(part)`` is (rel, other, values...) of ``rows`` entities at a time
    (int64 ids), the results concatenated; without entities the empty result, int64 / int64 and ``n_values`` float32 (0, k)."""
    out = [chunk(ents[at:at + rows].long()) for at in range(0, ents.numel(), rows)]
    if not out:
        i64 = torch.zeros(0, k, dtype=torch.int64, device=ents.device)
        return (i64, i64.clone()) + tuple(torch.zeros(0, k, dtype=torch.float32, device=ents.device) for _ in range(n_values))
    return tuple(torch.cat(t) for t in zip(*out))


def complete_entities(embedding, w, entities, k, *, side='s', filter_index=None, flow_log_prob=None, exclude_self=True,
                      type_constraint=UNCONSTRAINED):
    """What is this entity missing?  For every entity ``a`` of ``entities`` (any order, repeats allowed) the ``k`` most likely new
    facts around it over ALL relations at once: ``side='s'`` the facts (a, r, x), ``side='o'`` the facts (x, r, a), scored as
    ``predict_topk`` scores the queries (a, r) in that direction (logit = (e_a * w_r) . e_x + flow_log_prob: the query entity's row
    carries w_r on both sides).  With a ``FilterIndex`` the known facts are left out -- direction 'o' for ``side='s'``, 's' for
    ``side='o'`` -- and with ``exclude_self`` the loops (a, r, a).  One fused launch pair (ops.entity_topk_scores) keeps one list
    per entity while the relations are walked.  Returns ``(rel int64 (m, k), other int64 (m, k), logits float32 (m, k))`` in the
    order of ``complete_entities_from_scores``: best first, ties by relation, then by entity; rows with fewer than k candidates
    end in -1 / -1 / -inf.  1 <= k <= 128.  With a ``type_constraint`` (TypeConstraint) only type-correct facts are candidates --
    the entity seen on its side of r and the other entity seen on the other side, ``mine_triplets(type_constraint=)``'s rule --
    at the same logits, from the sweep over the relations' member lists (ops.entity_topk_scores_typed); the filter and the
    constraint are independent and may come from different triplet sets.  An entity on its side of no relation gets an
    all-padding row.  The unconstrained call leaves the argument out; an explicit None is a TypeError."""
    type_constraint = _complete_constraint(type_constraint)
    emb, wd, ents, k, (lo, hi, ent) = _complete_args(embedding, w, entities, k, side, filter_index)
    if type_constraint is not None:
        set_ptr, set_ids = _mine_members(type_constraint, emb.shape[0], wd.shape[0], emb.device)
        return ops.entity_topk_scores_typed(ents, emb, wd, k, set_ptr, set_ids, side, _mine_bias(flow_log_prob, emb.device), lo, hi, ent,
                                            exclude_self)
    return ops.entity_topk_scores(ents, emb, wd, k, _mine_bias(flow_log_prob, emb.device), lo, hi, ent, exclude_self)


def complete_entities_unfused(embedding, w, entities, k, *, side='s', filter_index=None, flow_log_prob=None, exclude_self=True,
                              type_constraint=UNCONSTRAINED):
    """``complete_entities`` from materialised logits: per relation ``ops.mul`` + ``ops.gemm`` into a (rows, R, N) tensor, then
    ``complete_entities_from_scores``, ``COMPLETE_UNFUSED_ELEMS`` logits at a time.  The in-repo cross-check and the bench's
    baseline, never a fallback.  With a ``type_constraint`` the same logits under the masks of ``complete_masks``."""
    type_constraint = _complete_constraint(type_constraint)
    emb, wd, ents, k, (lo, hi, ent) = _complete_args(embedding, w, entities, k, side, filter_index)
    emb, wd = emb.contiguous(), wd.contiguous()
    n, num_rels = emb.shape[0], wd.shape[0]
    masks = _complete_mask_args(type_constraint, side, n, num_rels, emb.device)
    bias = _mine_bias(flow_log_prob, emb.device)

    def chunk(part):
        ea = emb[part].contiguous()
        score = torch.stack([ops.gemm(ops.mul(ea, wd[r].expand_as(ea).contiguous()), emb, trans_b=True, precision='f32')
                             for r in range(num_rels)], dim=1)
        if bias is not None:
            score = score + bias
        return complete_entities_from_scores(score, part, k, filt_lo=lo, filt_hi=hi, filt_ent=ent, exclude_self=exclude_self, **masks)

    return _complete_unfused(chunk, ents, max(1, COMPLETE_UNFUSED_ELEMS // (n * num_rels)), k)


# ---- per-relation completion: which pairs belong to this relation? -----------------------------------------------------------------
def _relation_pairs(val, r, num_rels, k, filt, exclude_self, subj_ok=None, obj_ok=None, ascending=False):
    """Relation r's candidates at or above its K-th logit, ``(s, o, logits)``, from its (N, N) logits ``val``: all pairs less NaN,
    less the typed rule's misses (``subj_ok`` / ``obj_ok`` bool [N]), less s == o under ``exclude_self``, less the filter's
    objects of (s, r) (``filt`` = the (lo, hi, ent) of ``_mine_filter``).  ``ascending``: ``val`` holds distances (transe.py) and
    the candidates at or below the K-th smallest are kept."""
    n = val.shape[0]
    val = val.to(torch.float32) + 0.0
    cand = ~torch.isnan(val)
    if subj_ok is not None:
        cand &= subj_ok.view(n, 1) & obj_ok.view(1, n)
    if exclude_self:
        cand &= ~torch.eye(n, dtype=torch.bool, device=val.device)
    lo, hi, ent = filt
    if lo is not None and n:
        dev = val.device
        cand &= ~_listed_mask(lo.reshape(-1).to(dev)[r::num_rels], hi.reshape(-1).to(dev)[r::num_rels], ent.to(dev), n, n, dev)
    vals = val[cand]
    if vals.numel() > k:
        kth = torch.topk(vals, k, largest=not ascending).values[-1]
        cand &= (val <= kth) if ascending else (val >= kth)
    s, o = torch.nonzero(cand, as_tuple=True)
    return s, o, val[cand]


def _relation_rows(pairs_of, rels, k, n, share, ascending=False):
    """The end of the host routes (transe.py's with ``ascending``): ``pairs_of(i, r)`` is the ``_relation_pairs`` of slot i,
    ``ops.relation_select`` the rest."""
    dev = rels.device
    parts = [pairs_of(i, r) for i, r in enumerate(rels.tolist())]
    slot = torch.cat([torch.full_like(p[0], i) for i, p in enumerate(parts)])
    subj, obj, logits, count = ops.relation_select(slot, torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]),
                                                   torch.cat([p[2] for p in parts]), rels, k, n, share, ascending)
    return subj, obj, logits, {'count': count.to(dev), 'passes': len(parts)}


def _relation_masks(cand_subj, cand_obj, num_rels, n, device):
    """The typed rule's dense masks, bool (R, N) each, given together or not at all."""
    if (cand_subj is None) != (cand_obj is None):
        raise ValueError('cand_subj and cand_obj are given together or not at all')
    if cand_subj is None:
        return None, None
    masks = tuple(torch.as_tensor(c, device=device) for c in (cand_subj, cand_obj))
    for name, c in zip(('cand_subj', 'cand_obj'), masks):
        if c.dtype != torch.bool or tuple(c.shape) != (num_rels, n):
            raise ValueError(f'{name}: expected a bool ({num_rels}, {n}) mask')
    return masks


def complete_relations_from_scores(score, k, *, relations=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                                   cand_subj=None, cand_obj=None, max_results=ops.MINE_MAX_RESULTS):
    """The rule of ``ops.relation_topk_scores`` on a materialised tensor ``score[r, s, o]`` (R, N, N), in plain torch (any device,
    CPU included): for each relation r of ``relations`` (unique ids in [0, R), any order; None: all) the ``k`` candidates (s, o)
    of largest logit.  Candidates: every (s, o), less ``filt_ent[filt_lo[s * R + r]:filt_hi[s * R + r]]`` as objects of (s, r),
    less s == o when ``exclude_self``, less NaN logits, and with ``cand_subj`` / ``cand_obj`` (bool (R, N), together) only s among
    ``cand_subj[r]`` and o among ``cand_obj[r]``.  Order inside a relation: ``mine_from_scores``' restricted to it -- logit
    descending with -0 == +0, then (s, o) ascending.  Returns ``(subj int64 (m, k), obj int64 (m, k), logits float32 (m, k),
    info)``, row i for ``relations[i]``, rows with fewer than k candidates ending in -1 / -1 / -inf, -0 reported as +0;
    ``info['count']`` int64 [m] is each relation's candidates at or above its K-th logit's exact value (all, when fewer than K
    exist).  ``m * k <= max_results``; a relation whose count exceeds its share ``max_results // m`` raises ``MineOverflow``
    naming it: nothing is truncated silently."""
    num_rels, n = score.shape[0], score.shape[1]
    rels = ops.relation_ids_check(relations, num_rels).to(score.device)
    k, max_results, share = ops._relation_args(k, rels.numel(), max_results)
    ops._mine_sizes(n, num_rels, filt_lo, filt_hi, filt_ent)
    subj_ok, obj_ok = _relation_masks(cand_subj, cand_obj, num_rels, n, score.device)
    filt = (filt_lo, filt_hi, filt_ent)

    def pairs_of(i, r):
        return _relation_pairs(score[r], r, num_rels, k, filt, exclude_self, *((subj_ok[r], obj_ok[r]) if subj_ok is not None else ()))

    return _relation_rows(pairs_of, rels, k, n, share)


def _relation_setup(embedding, w, filter_index, flow_log_prob, type_constraint):
    """What the two routes of ``complete_relations`` prepare alike: (emb, w, (lo, hi, ent), bias, the constraint or None)."""
    type_constraint = _complete_constraint(type_constraint)
    emb = embedding.detach()
    wd = w.detach().to(emb.device)
    filt = _mine_filter(filter_index, emb.shape[0], wd.shape[0], emb.device)
    if type_constraint is not None:
        _mine_members_sizes(type_constraint, emb.shape[0], wd.shape[0])
    return emb, wd, filt, _mine_bias(flow_log_prob, emb.device), type_constraint


def complete_relations(embedding, w, k, *, relations=None, filter_index=None, flow_log_prob=None, exclude_self=True,
                       type_constraint=UNCONSTRAINED, max_results=ops.MINE_MAX_RESULTS):
    """Which pairs belong to this relation?  For every relation r of ``relations`` (unique ids, any order; default: every relation)
    its OWN ``k`` most confident new facts (s, r, o), scored as every scorer here scores them (logit = (e_s * w_r) . e_o +
    flow_log_prob); with a ``FilterIndex`` the known triplets are left out.  ``mine_triplets`` cannot answer this: its one
    threshold for the whole graph compares relations by the scale of their ``w`` rows.  Here every relation has its own
    threshold, found for all of them in the same few fused sweeps (ops.relation_topk_scores), and a handful of relations cost
    their share of a sweep.  Returns ``(subj int64 (m, k), obj int64 (m, k), logits float32 (m, k), info)`` in the order of
    ``complete_relations_from_scores``: row i for ``relations[i]``, best first, ties by (s, o), short rows padded with -1 / -1 /
    -inf; ``info['count']`` int64 [m], ``info['passes']``.  ``k >= 1`` and ``m * k <= max_results``; ``MineOverflow`` (naming the
    relation) rather than a truncated list.  With a ``type_constraint`` (TypeConstraint) only type-correct pairs are candidates --
    ``mine_triplets(type_constraint=)``'s rule on the same member lists, at the same logits (ops.relation_topk_scores_typed).  The
    unconstrained call leaves the argument out; an explicit None is a TypeError."""
    emb, wd, (lo, hi, ent), bias, type_constraint = _relation_setup(embedding, w, filter_index, flow_log_prob, type_constraint)
    rule = dict(relations=relations, bias=bias, filt_lo=lo, filt_hi=hi, filt_ent=ent, exclude_self=exclude_self, max_results=max_results)
    if type_constraint is not None:
        set_ptr, set_ids = type_constraint.members(emb.device)
        return ops.relation_topk_scores_typed(emb, wd, k, set_ptr, set_ids, **rule)
    return ops.relation_topk_scores(emb, wd, k, **rule)


def complete_relations_unfused(embedding, w, k, *, relations=None, filter_index=None, flow_log_prob=None, exclude_self=True,
                               type_constraint=UNCONSTRAINED, max_results=ops.MINE_MAX_RESULTS):
    """``complete_relations`` from materialised logits, one relation at a time: ``ops.gemm(ops.mul(E, w[r]), E^T)`` (+ bias), then
    the rule of ``complete_relations_from_scores``.  The in-repo cross-check and the bench's comparator, never a fallback."""
    emb, wd, filt, bias, type_constraint = _relation_setup(embedding, w, filter_index, flow_log_prob, type_constraint)
    emb, wd = emb.contiguous(), wd.contiguous()
    n, num_rels = emb.shape[0], wd.shape[0]
    rels = ops.relation_ids_check(relations, num_rels).to(emb.device)
    k, max_results, share = ops._relation_args(k, rels.numel(), max_results)
    masks = None
    if type_constraint is not None:
        masks = (type_constraint.mask(torch.arange(num_rels, 2 * num_rels), emb.device), type_constraint.mask(torch.arange(num_rels), emb.device))

    def pairs_of(i, r):
        val = ops.gemm(ops.mul(emb, wd[r].expand_as(emb).contiguous()), emb, trans_b=True, precision='f32')
        if bias is not None:
            val = val + bias
        return _relation_pairs(val, r, num_rels, k, filt, exclude_self, *((masks[0][r], masks[1][r]) if masks else ()))

    return _relation_rows(pairs_of, rels, k, n, share)


# ---- type-correct completions on the Monte-Carlo posterior predictive ---------------------------------------------------------
MC_MINE_STACK_BYTES = 64 << 20      # bytes of the (S, chunk, h) query stack behind the spread of the mined triplets


def mine_from_probs(pbar, *, k=None, threshold=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                    max_results=ops.MINE_MAX_RESULTS, cand_subj=None, cand_obj=None):
    """The mining rule of ``ops.mine_scores_typed_mc`` on a materialised tensor of posterior-predictive probabilities
    ``pbar[r, s, o]`` (R, N, N), in plain torch: ``mine_from_scores``' rule with the probability as the value -- candidates less
    the listed, less s == o, less NaN; pbar descending, then (s, r, o) ascending; ``threshold`` a probability; ``count`` and
    ``MineOverflow`` at the exact K-th value, which for a saturated pbar (1.0f) is a real tie."""
    return _mine_from_values(pbar, False, k=k, threshold=threshold, filt_lo=filt_lo, filt_hi=filt_hi, filt_ent=filt_ent,
                             exclude_self=exclude_self, max_results=max_results, cand_subj=cand_subj, cand_obj=cand_obj)


def _mine_mc_setup(z, w, k, threshold, max_results, filter_index, flow_log_probs, type_constraint):
    _mine_args(k, threshold, max_results)
    if type_constraint is None:
        raise ValueError('mine_triplets_mc needs a type_constraint: only the sweep over the relations\' member lists has a '
                         'Monte-Carlo form.  The unconstrained sweep keeps its two tiles of ONE table in LDS across all '
                         'relations; looping it over samples would restage both per (relation, sample), so it was not built')
    z, wd, flp = _mc_args(z, w, flow_log_probs)
    n, num_rels = z.shape[1], wd.shape[0]
    return z, wd, flp, n, num_rels, _mine_filter(filter_index, n, num_rels, z.device), _mine_members(type_constraint, n, num_rels,
                                                                                                    z.device)


def mine_triplets_mc(z, w, *, k=None, threshold=None, filter_index=None, flow_log_probs=None, exclude_self=True,
                     max_results=ops.MINE_MAX_RESULTS, type_constraint=None):
    """Type-correct knowledge-graph completion on the posterior predictive of the samples ``z`` (S, N, h) of
    ``KGVAE.posterior_samples`` (``flow_log_probs``: its second result): among the type-correct triplets (``type_constraint``,
    required) the ``k`` of highest ``pbar = mean_s sigmoid(logit_s)`` or every one with pbar >= ``threshold`` (a probability),
    the known ones of ``filter_index`` left out.  One fused sweep per pass (ops.mine_scores_typed_mc); for a fixed seed of the
    samples the result is reproducible.  Returns ``(triplets int64 (n, 3), probs float32 (n,), std float32 (n,), info)`` in the
    order of ``mine_from_probs``; ``std`` is the population standard deviation over the samples of each returned triplet's
    probability (ops.pair_prob_std_mc, fed in chunks whose query stack stays under ``MC_MINE_STACK_BYTES``).  Raises
    ``MineOverflow`` rather than truncating -- also when a saturated tie at pbar == 1.0f exceeds ``max_results``."""
    z, wd, flp, n, num_rels, (lo, hi, ent), (set_ptr, set_ids) = _mine_mc_setup(z, w, k, threshold, max_results, filter_index,
                                                                                flow_log_probs, type_constraint)
    trip, probs, info = ops.mine_scores_typed_mc(z, wd, set_ptr, set_ids, threshold=threshold, k=k, bias=flp, filt_lo=lo, filt_hi=hi,
                                                 filt_ent=ent, exclude_self=exclude_self, max_results=max_results)
    rows = max(1, MC_MINE_STACK_BYTES // (z.shape[0] * z.shape[2] * 4))
    std = [ops.pair_prob_std_mc(_mc_queries(z, wd, trip[i:i + rows, 0], trip[i:i + rows, 1]), z, trip[i:i + rows, 2:3], flp)[:, 0]
           for i in range(0, trip.shape[0], rows)]
    return trip, probs, (torch.cat(std) if std else torch.zeros(0, dtype=torch.float32, device=z.device)), info


def mine_triplets_mc_unfused(z, w, *, k=None, threshold=None, filter_index=None, flow_log_probs=None, exclude_self=True,
                             max_results=ops.MINE_MAX_RESULTS, type_constraint=None):
    """``mine_triplets_mc`` from materialised probabilities, one relation at a time: per sample the relation's subject and object
    members are ``index_select``-ed, ``ops.mul`` + ``ops.gemm`` give the block of logits, torch the sigmoid and the running mean;
    then torch selection with a running K-th value (``_mine_unfused``).  The spread comes from the selected triplets' per-sample
    probabilities in torch.  The in-repo cross-check and the bench's comparator, never a fallback."""
    z, wd, flp, n, num_rels, filt, members = _mine_mc_setup(z, w, k, threshold, max_results, filter_index, flow_log_probs,
                                                            type_constraint)
    wd = wd.contiguous()
    n_samples = z.shape[0]

    def pbar_of(r, subj, obj):
        total = None
        for s in range(n_samples):
            a, b = z[s].index_select(0, subj), z[s].index_select(0, obj)
            logit = ops.gemm(ops.mul(a, wd[r].expand_as(a).contiguous()), b, trans_b=True, precision='f32')
            p = torch.sigmoid(logit if flp is None else logit + flp[s])
            total = p if total is None else total + p
        return total * (1.0 / n_samples)

    trip, probs, info = _mine_unfused(pbar_of, False, n, num_rels, z.device, k=k, threshold=threshold, filt=filt,
                                      exclude_self=exclude_self, max_results=max_results, members=members)
    std, rows = [], max(1, MC_MINE_STACK_BYTES // (n_samples * z.shape[2] * 4))
    for i in range(0, trip.shape[0], rows):
        s_, r_, o_ = trip[i:i + rows].unbind(1)
        logit = (z[:, s_] * wd[r_] * z[:, o_]).sum(-1)
        std.append(torch.sigmoid(logit if flp is None else logit + flp.view(-1, 1)).std(dim=0, unbiased=False))
    return trip, probs, (torch.cat(std) if std else torch.zeros(0, dtype=torch.float32, device=z.device)), info


# ---- per-entity completion on the Monte-Carlo posterior predictive, typed or not -------------------------------------------------
def _complete_mc_args(z, w, entities, k, side, filter_index, flow_log_probs):
    """What the two routes of ``complete_entities_mc`` check and prepare alike: (z, w, flp, entities, k, (lo, hi, ent))."""
    _complete_side(side)
    k = ops._topk_arg(k)
    z, wd, flp = _mc_args(z, w, flow_log_probs)
    ents, filt = _complete_queries(z, wd, entities, side, filter_index, mc=True)
    return z, wd, flp, ents, k, filt


def _complete_mc_rows(z):
    """Returned facts per chunk of the spread's query stack: its (S, rows, h) floats stay under ``MC_MINE_STACK_BYTES``."""
    return max(1, MC_MINE_STACK_BYTES // (z.shape[0] * z.shape[2] * 4))


def complete_entities_mc(z, w, entities, k, *, side='s', filter_index=None, flow_log_probs=None, exclude_self=True,
                         type_constraint=UNCONSTRAINED):
    """``complete_entities`` on the posterior predictive of the samples ``z`` (S, N, h) of ``KGVAE.posterior_samples``
    (``flow_log_probs``: its second result): each entity's ``k`` new facts of highest ``pbar = mean_s sigmoid(logit_s)`` over ALL
    relations, reproducible for a fixed seed of the samples.  Sides, the filter's direction, ``exclude_self`` and the constraint
    (left out: unconstrained; an explicit None is a TypeError) are ``complete_entities``'.  One fused launch pair
    (ops.entity_topk_scores_mc, or ops.entity_topk_scores_typed_mc with a ``type_constraint``) loops the samples around each score
    tile and selects once per tile.  Returns ``(rel int64 (m, k), other int64 (m, k), prob_mean float32 (m, k), prob_std float32
    (m, k))``: pbar descending, ties -- real ones, pbar saturates -- by relation, then by entity; rows with fewer than k
    candidates end in -1 / -1 / -inf / 0.  ``prob_std`` is the population standard deviation over the samples of each returned
    fact's probability (ops.pair_prob_std_mc, fed as ``mine_triplets_mc`` feeds it, in chunks whose query stack stays under
    ``MC_MINE_STACK_BYTES``)."""
    type_constraint = _complete_constraint(type_constraint)
    z, wd, flp, ents, k, (lo, hi, ent) = _complete_mc_args(z, w, entities, k, side, filter_index, flow_log_probs)
    if type_constraint is not None:
        set_ptr, set_ids = _mine_members(type_constraint, z.shape[1], wd.shape[0], z.device)
        rel, other, mean = ops.entity_topk_scores_typed_mc(ents, z, wd, k, set_ptr, set_ids, side, flp, lo, hi, ent, exclude_self)
    else:
        rel, other, mean = ops.entity_topk_scores_mc(ents, z, wd, k, flp, lo, hi, ent, exclude_self)
    # the spread: one query row (a, r) per returned fact, its one candidate the other entity; a padding slot (other -1) gives 0
    a = ents.long().view(-1, 1).expand(-1, k).reshape(-1)
    r, x = rel.reshape(-1).clamp(min=0), other.reshape(-1, 1)
    rows = _complete_mc_rows(z)
    std = [ops.pair_prob_std_mc(_mc_queries(z, wd, a[i:i + rows], r[i:i + rows]), z, x[i:i + rows], flp)[:, 0]
           for i in range(0, a.numel(), rows)]
    std = torch.cat(std) if std else torch.zeros(0, dtype=torch.float32, device=z.device)
    return rel, other, mean, std.view(-1, k)


def complete_entities_mc_from_probs(pbar, probs, entities, k, **rule):
    """The host rule of ``complete_entities_mc_unfused`` on materialised values (any device): ``pbar`` (m, R, N) the mean
    probabilities, ``probs`` (S, m, R, N) the per-sample ones; ``complete_entities_from_scores`` (``rule``: its filter, ``exclude_self``
    and masks) selects on pbar, and the spread is the population standard deviation of the selected facts' per-sample
    probabilities, 0 in the padding slots.  Returns ``(rel, other, prob_mean, prob_std)``."""
    rel, other, mean = complete_entities_from_scores(pbar, entities, k, **rule)
    m, num_rels, n = pbar.shape
    gone = rel < 0
    flat = (rel.clamp(min=0) * n + other.clamp(min=0)).unsqueeze(0).expand(probs.shape[0], -1, -1)
    picked = probs.reshape(probs.shape[0], m, num_rels * n).gather(2, flat)
    std = picked.std(dim=0, unbiased=False).to(torch.float32)
    return rel, other, mean, torch.where(gone, torch.zeros_like(std), std)


def complete_entities_mc_unfused(z, w, entities, k, *, side='s', filter_index=None, flow_log_probs=None, exclude_self=True,
                                 type_constraint=UNCONSTRAINED):
    """``complete_entities_mc`` from materialised probabilities: per sample and relation ``ops.mul`` + ``ops.gemm`` give the logits,
    torch the sigmoid and the running mean, then ``complete_entities_from_scores`` on the (rows, R, N) probabilities,
    ``COMPLETE_UNFUSED_ELEMS`` values per sample at a time; the spread comes from the selected facts' per-sample probabilities
    (``complete_entities_mc_from_probs``).  The in-repo cross-check and the bench's comparator, never a fallback."""
    type_constraint = _complete_constraint(type_constraint)
    z, wd, flp, ents, k, (lo, hi, ent) = _complete_mc_args(z, w, entities, k, side, filter_index, flow_log_probs)
    wd = wd.contiguous()
    n_samples, n, num_rels = z.shape[0], z.shape[1], wd.shape[0]
    masks = _complete_mask_args(type_constraint, side, n, num_rels, z.device)

    def chunk(part):
        probs, total = [], None
        for s in range(n_samples):
            ea = z[s][part].contiguous()
            logit = torch.stack([ops.gemm(ops.mul(ea, wd[r].expand_as(ea).contiguous()), z[s], trans_b=True, precision='f32')
                                 for r in range(num_rels)], dim=1)
            p = torch.sigmoid(logit if flp is None else logit + flp[s])
            probs.append(p)
            total = p if total is None else total + p
        return complete_entities_mc_from_probs(total * (1.0 / n_samples), torch.stack(probs), part, k, filt_lo=lo, filt_hi=hi,
                                               filt_ent=ent, exclude_self=exclude_self, **masks)

    return _complete_unfused(chunk, ents, max(1, COMPLETE_UNFUSED_ELEMS // (n * num_rels * (n_samples + 1))), k, n_values=2)


def calc_mrr(embedding, w, test_triplets, hits=[], eval_bz=100, all_batches=True, flow_log_prob=None,
             verbose=True):
    with torch.no_grad():
        w, flow_log_prob = _on_device(embedding, w, flow_log_prob)
        by_s, by_o = _both_directions(embedding, test_triplets, eval_bz, all_batches, lambda a, r, b, n, d:
                                      (perturb_and_get_rank(embedding, w, a, r, b, n, eval_bz, all_batches, flow_log_prob),))
        # Hits@k are printed, never returned: not computed when nothing is printed
        return _report(by_s, by_o, CONSTRAINED_KINDS[:1], hits if verbose else (), verbose, MRR_LINES)['mrr_raw']


# ---- relation prediction: the query is an entity pair (s, ?, o), the candidates are the relations -----------------------------
RELATION_MRR_LINES = ("Relation MRR ({0}): {1:.6f}", "Relation Hits ({0}) @ {1}: {2:.6f}")


class PairFilterIndex:
    """The known relations of every entity pair, built once per dataset: key ``s * num_nodes + o`` (int64: num_nodes ** 2 passes
    2**31 from 46 341 entities on) -> the sorted unique relations r with (s, r, o) known.  ``keys`` (int64) and ``rel`` (int32) are
    parallel arrays sorted by (key, relation), duplicate triplets once: the relations of one pair are a contiguous run of ``rel``,
    which is the (filt_lo, filt_hi, filt_rel) form ``ops.pair_relation_scores`` takes.  Built with torch ops on ``device``."""

    def __init__(self, num_nodes, num_rels, *triplet_sets, device='cpu'):
        self.num_nodes, self.num_rels, self.device = int(num_nodes), int(num_rels), torch.device(device)
        parts = [torch.as_tensor(t).to(device=self.device, dtype=torch.long).reshape(-1, 3) for t in triplet_sets]
        trip = torch.cat(parts) if parts else torch.zeros(0, 3, dtype=torch.long, device=self.device)
        if trip.numel() and (int(trip[:, [0, 2]].min()) < 0 or int(trip[:, [0, 2]].max()) >= self.num_nodes
                             or int(trip[:, 1].min()) < 0 or int(trip[:, 1].max()) >= self.num_rels):
            raise ValueError('triplets out of range of num_nodes / num_rels')
        key, r = trip[:, 0] * self.num_nodes + trip[:, 2], trip[:, 1]
        order = torch.argsort(r, stable=True)
        order = order[torch.argsort(key[order], stable=True)]               # by (key, relation)
        k, x = key[order], r[order]
        keep = torch.ones_like(k, dtype=torch.bool)
        if k.numel() > 1:
            keep[1:] = (k[1:] != k[:-1]) | (x[1:] != x[:-1])                  # duplicate triplets once
        self.keys, self.rel = k[keep].contiguous(), x[keep].to(torch.int32).contiguous()
        if max(self.rel.numel(), 1) >= 2 ** 31:
            raise ValueError('more than 2**31 - 1 distinct triplets')

    def lookup(self, s, o):
        """(lo, hi): the range of ``rel`` holding the known relations of each pair (s[i], o[i]), on ``s``'s device."""
        q = s.to(device=self.device, dtype=torch.long) * self.num_nodes + o.to(device=self.device, dtype=torch.long)
        lo = torch.searchsorted(self.keys, q, right=False)
        hi = torch.searchsorted(self.keys, q, right=True)
        return lo.to(s.device), hi.to(s.device)

    def relations(self, device=None):
        return self.rel if device is None else self.rel.to(device)


def _pair_checked(s, o, target, n, num_rels, pair_filter):
    """The id checks of a whole query set, once (``ops.pair_ids_check``: one device-to-host read), so that no chunk repeats them;
    a ``pair_filter`` vouches for its ranges only when it was built for these sizes."""
    if pair_filter is not None and (pair_filter.num_nodes != n or pair_filter.num_rels != num_rels):
        raise ValueError(f'pair_filter was built for {pair_filter.num_nodes} entities / {pair_filter.num_rels} relations, the tables '
                         f'hold {n} / {num_rels}')
    ops.pair_ids_check(s, o, target, n, num_rels)


def _pair_chunks(s, o, pair_filter, device, step):
    """The chunk loop of the pair queries, once: ``(slice, filt_lo, filt_hi, filt_rel)`` for every ``step`` pairs, the filter's
    three None without a ``pair_filter``."""
    rel = pair_filter.relations(device) if pair_filter is not None else None
    for lo in range(0, s.shape[0], step):
        sl = slice(lo, min(s.shape[0], lo + step))
        f_lo, f_hi = pair_filter.lookup(s[sl], o[sl]) if pair_filter is not None else (None, None)
        yield sl, f_lo, f_hi, rel


def pair_scores_unfused(emb, w, s, o, flow_log_prob=None):
    """The materialised (m, R) logits of the pairs: one product of the gathered rows, one fp32 GEMM against the relation table."""
    score = ops.gemm(ops.mul(emb[s].contiguous(), emb[o].contiguous()), w, trans_b=True, precision='f32')
    return score if flow_log_prob is None else score + flow_log_prob


def relation_ranks_from_scores(score, target, filt_lo=None, filt_hi=None, filt_rel=None, cand_mask=None):
    """The rank rule of ``ops.pair_relation_scores`` on a materialised (m, R) matrix, higher is better, in plain torch (any
    device): ``mid_ranks`` with the relations ``filt_rel[filt_lo[i]:filt_hi[i]]`` left out of the filtered count (a listed target
    is allowed: the target is left out of every pool anyway).  Returns (raw, filtered or None); with ``cand_mask`` (dense (m, R)
    bool of the type-correct relations, ``TypeConstraint.pair_mask``) the four kinds of ``mid_ranks``."""
    listed = None if filt_lo is None else _listed_mask(filt_lo, filt_hi, filt_rel, score.shape[0], score.shape[1], score.device)
    if cand_mask is None:
        return mid_ranks(score, target.to(score.device), listed)[:2]
    return mid_ranks(score, target.to(score.device), listed, cand_mask.to(score.device))


def _pair_cat(parts, width, dtype, device):
    return torch.cat(parts) if parts else torch.zeros((0,) + width, dtype=dtype, device=device)


def pair_pbar_unfused(z, w, s, o, flow_log_probs=None):
    """The materialised (m, R) posterior-predictive probabilities of the pairs: ``pair_scores_unfused`` per sample, a sigmoid and
    a running sum in ascending sample order, times 1 / S."""
    total = None
    for i in range(z.shape[0]):
        p = torch.sigmoid(pair_scores_unfused(z[i], w, s, o, None if flow_log_probs is None else flow_log_probs[i]))
        total = p if total is None else total + p
    return total * (1.0 / z.shape[0])


def _pair_tables(table, w, flow, mc):
    """The operands of a relation driver on the table's device: (table, w, bias) -- with ``mc`` the (S, N, h) samples and one
    bias per sample (``_mc_args``), else the embedding and the scalar flow_log_prob."""
    if mc:
        return _mc_args(table, w, flow)
    emb = table.detach().contiguous()
    return (emb,) + _on_device(emb, w.detach(), flow)


def _pair_type_checked(type_constraint, n, num_rels):
    if type_constraint is not None and (type_constraint.num_nodes != n or type_constraint.num_rels != num_rels):
        raise ValueError(f'type_constraint was built for {type_constraint.num_nodes} entities / {type_constraint.num_rels} relations, '
                         f'the tables hold {n} / {num_rels}')


def _rank_relations(table, w, triplets, pair_filter, flow, fused, type_constraint=None, mc=False):
    """The relation rank driver, fused or materialised, single-draw or (``mc``) posterior-predictive: (raw, filtered or None), with
    a ``type_constraint`` the four kinds (the filtered ones None without a ``pair_filter``)."""
    tab, wd, flow = _pair_tables(table, w, flow, mc)
    dev = tab.device
    triplets = triplets.to(dev)
    s, r, o = triplets[:, 0], triplets[:, 1], triplets[:, 2]
    _pair_checked(s, o, r, tab.shape[-2], wd.shape[0], pair_filter)
    _pair_type_checked(type_constraint, tab.shape[-2], wd.shape[0])
    cand = type_constraint.relation_words(dev) if fused and type_constraint is not None else None
    n_kinds = 2 if type_constraint is None else 4
    kinds = [[] for _ in range(n_kinds)]
    for sl, f_lo, f_hi, rel in _pair_chunks(s, o, pair_filter, dev, MAX_QUERY_ROWS):
        if fused:
            score = ops.pair_relation_scores_mc if mc else ops.pair_relation_scores
            ranks = score(tab, wd, s[sl], o[sl], target=r[sl], bias=flow, filt_lo=f_lo, filt_hi=f_hi, filt_rel=rel, cand=cand,
                          ids_checked=True)[0]
        else:
            value = pair_pbar_unfused(tab, wd, s[sl], o[sl], flow) if mc else pair_scores_unfused(tab, wd, s[sl], o[sl], flow)
            mask = None if type_constraint is None else type_constraint.pair_mask(s[sl], o[sl], dev)
            ranks = relation_ranks_from_scores(value, r[sl], f_lo, f_hi, rel, mask)
        for kind, part in zip(kinds, ranks):
            kind.append(part)
    return tuple(None if pair_filter is None and i % 2 else _pair_cat(kind, (), torch.float32, dev) for i, kind in enumerate(kinds))


def rank_relations(embedding, w, triplets, pair_filter=None, flow_log_prob=None, type_constraint=None):
    """Relation prediction, ranks: for every triplet (s, r, o) the 0-based mid-rank of r among ALL relations under ``logit =
    (e_s * e_o) . w_r + flow_log_prob`` -- DistMult's score of the triplet, read as a function of the relation -- raw and, with a
    ``PairFilterIndex``, with the other known relations of the pair left out.  One launch per ``MAX_QUERY_ROWS`` pairs
    (ops.pair_relation_scores).  Returns ``(raw, filtered or None)``; with a ``TypeConstraint`` ``(raw, filtered, raw_constrained,
    filtered_constrained)``, the last two among the pair's type-correct relations only (s seen as subject of r and o as object
    of r), the first two unchanged."""
    return _rank_relations(embedding, w, triplets, pair_filter, flow_log_prob, True, type_constraint)


def rank_relations_unfused(embedding, w, triplets, pair_filter=None, flow_log_prob=None, type_constraint=None):
    """``rank_relations`` from materialised logits (``pair_scores_unfused`` + ``mid_ranks``): the in-repo cross-check and the
    bench's comparator, never a fallback."""
    return _rank_relations(embedding, w, triplets, pair_filter, flow_log_prob, False, type_constraint)


def rank_relations_mc(z, w, triplets, pair_filter=None, flow_log_probs=None, type_constraint=None):
    """``rank_relations`` on the posterior predictive of the samples ``z`` (S, N, h) of ``KGVAE.posterior_samples``
    (``flow_log_probs``: its second result): every triplet's relation is ranked on ``pbar[r] = mean_s sigmoid((z_s[s] * z_s[o]) .
    w_r + flow_log_probs[s])`` (ops.pair_relation_scores_mc, one launch per ``MAX_QUERY_ROWS`` pairs).  Mid-ranks: pbar saturates,
    so ties are real.  Reproducible for a seed of the samples."""
    return _rank_relations(z, w, triplets, pair_filter, flow_log_probs, True, type_constraint, mc=True)


def rank_relations_mc_unfused(z, w, triplets, pair_filter=None, flow_log_probs=None, type_constraint=None):
    """``rank_relations_mc`` from materialised probabilities (``pair_pbar_unfused`` + ``mid_ranks``): cross-check and comparator."""
    return _rank_relations(z, w, triplets, pair_filter, flow_log_probs, False, type_constraint, mc=True)


RELATION_MC_MRR_LINES = ("MC relation MRR ({0}, {n_samples} samples): {1:.6f}", "MC relation Hits ({0}) @ {1}: {2:.6f}")


def _calc_relation_mrr(rank, table, w, test_triplets, pair_filter, hits, flow, verbose, type_constraint=None, mc=False):
    with torch.no_grad():
        ranks = rank(table, w, test_triplets, pair_filter, flow, type_constraint)
        none = [None if r is None else r.new_zeros(0) for r in ranks]      # one direction: nothing on _report's other side
        if mc:
            return _report(list(ranks), none, CONSTRAINED_KINDS, hits, verbose, RELATION_MC_MRR_LINES, {'n_samples': int(table.shape[0])})
        return _report(list(ranks), none, CONSTRAINED_KINDS, hits, verbose, RELATION_MRR_LINES)


def calc_relation_mrr(embedding, w, test_triplets, pair_filter=None, hits=[1, 3, 10], flow_log_prob=None, verbose=True,
                      type_constraint=None):
    """The relation-prediction report over the test triplets (one direction: there is one relation slot): ``mrr_raw`` and
    ``hits_raw: {k: v}``, and with a ``PairFilterIndex`` ``mrr_filtered`` / ``hits_filtered``; with a ``TypeConstraint`` also the
    ``_constrained`` kinds of ``CONSTRAINED_KINDS``."""
    return _calc_relation_mrr(rank_relations, embedding, w, test_triplets, pair_filter, hits, flow_log_prob, verbose, type_constraint)


def calc_relation_mrr_unfused(embedding, w, test_triplets, pair_filter=None, hits=[1, 3, 10], flow_log_prob=None, verbose=True,
                              type_constraint=None):
    return _calc_relation_mrr(rank_relations_unfused, embedding, w, test_triplets, pair_filter, hits, flow_log_prob, verbose,
                              type_constraint)


def calc_relation_mc_mrr(z, w, test_triplets, pair_filter=None, flow_log_probs=None, hits=[1, 3, 10], verbose=True, type_constraint=None):
    """``calc_relation_mrr`` on the posterior predictive (``rank_relations_mc``): ``n_samples``, then the same keys."""
    return _calc_relation_mrr(rank_relations_mc, z, w, test_triplets, pair_filter, hits, flow_log_probs, verbose, type_constraint, mc=True)


def calc_relation_mc_mrr_unfused(z, w, test_triplets, pair_filter=None, flow_log_probs=None, hits=[1, 3, 10], verbose=True,
                                 type_constraint=None):
    return _calc_relation_mrr(rank_relations_mc_unfused, z, w, test_triplets, pair_filter, hits, flow_log_probs, verbose, type_constraint,
                              mc=True)


def _pair_prob_std(z, w, s, o, ids, flp, fused):
    """The spread of each proposed relation's probability over the samples, (n, k): fused, ``ops.pair_prob_std_mc`` on the stacks
    ``mul(z[:, s], z[:, o])`` and ``w`` repeated per sample (a real copy: the entry refuses a zero stride), ``MC_STACK_ROWS`` pairs
    at a time; else from the materialised per-sample probabilities.  Padding ids give 0."""
    if fused:
        ws = w.unsqueeze(0).repeat(z.shape[0], 1, 1)
        parts = [ops.pair_prob_std_mc(ops.mul(z[:, s[lo:lo + MC_STACK_ROWS]].contiguous(), z[:, o[lo:lo + MC_STACK_ROWS]].contiguous()), ws,
                                      ids[lo:lo + MC_STACK_ROWS], flp) for lo in range(0, s.shape[0], MC_STACK_ROWS)]
        return _pair_cat(parts, (ids.shape[1],), torch.float32, z.device)
    pick = ids.clamp(min=0)
    ps = [torch.sigmoid(pair_scores_unfused(z[i], w, s, o, None if flp is None else flp[i])).gather(1, pick) for i in range(z.shape[0])]
    sd = torch.stack(ps).std(dim=0, unbiased=False)
    sd[ids < 0] = 0.0
    return sd


def _predict_relations(table, w, s, o, k, pair_filter, flow, fused, type_constraint=None, mc=False):
    tab, wd, flow = _pair_tables(table, w, flow, mc)
    dev = tab.device
    s, o = s.to(dev), o.to(dev)
    _pair_checked(s, o, None, tab.shape[-2], wd.shape[0], pair_filter)
    _pair_type_checked(type_constraint, tab.shape[-2], wd.shape[0])
    cand = type_constraint.relation_words(dev) if fused and type_constraint is not None else None
    ids, values, std = [], [], []
    for sl, f_lo, f_hi, rel in _pair_chunks(s, o, pair_filter, dev, MAX_QUERY_ROWS):
        if fused:
            score = ops.pair_relation_scores_mc if mc else ops.pair_relation_scores
            i, l = score(tab, wd, s[sl], o[sl], k=k, bias=flow, filt_lo=f_lo, filt_hi=f_hi, filt_rel=rel, cand=cand, ids_checked=True)[1]
        else:
            value = pair_pbar_unfused(tab, wd, s[sl], o[sl], flow) if mc else pair_scores_unfused(tab, wd, s[sl], o[sl], flow)
            mask = None if type_constraint is None else type_constraint.pair_mask(s[sl], o[sl], dev)
            i, l = topk_from_scores(value, k, f_lo, f_hi, rel, cand=mask)
        ids.append(i)
        values.append(l)
        if mc:
            std.append(_pair_prob_std(tab, wd, s[sl], o[sl], i, flow, fused))
    out = _pair_cat(ids, (int(k),), torch.int64, dev), _pair_cat(values, (int(k),), torch.float32, dev)
    return out + (_pair_cat(std, (int(k),), torch.float32, dev),) if mc else out


def predict_relations(embedding, w, s, o, k, pair_filter=None, flow_log_prob=None, type_constraint=None):
    """Relation prediction, proposals: the ``k`` most plausible relations between ``s[i]`` and ``o[i]`` at ``rank_relations``'
    logits, the pair's known relations (``pair_filter``) left out -- with a ``TypeConstraint`` among the pair's type-correct
    relations only.  Returns ``(ids int64 (n, k), logits float32 (n, k))`` in the order of ``topk_from_scores``, padded with
    -1 / -inf when fewer than k relations are left."""
    return _predict_relations(embedding, w, s, o, k, pair_filter, flow_log_prob, True, type_constraint)


def predict_relations_unfused(embedding, w, s, o, k, pair_filter=None, flow_log_prob=None, type_constraint=None):
    """``predict_relations`` from materialised logits (``pair_scores_unfused`` + ``topk_from_scores``): cross-check and comparator."""
    return _predict_relations(embedding, w, s, o, k, pair_filter, flow_log_prob, False, type_constraint)


def predict_relations_mc(z, w, s, o, k, pair_filter=None, flow_log_probs=None, type_constraint=None):
    """``predict_relations`` on the posterior predictive of the samples ``z`` (S, N, h): the ``k`` relations of highest ``pbar``
    (``rank_relations_mc``'s value) and how sure the model is of each.  Returns ``(ids int64 (n, k), prob_mean float32 (n, k),
    prob_std float32 (n, k))``, ``prob_std`` the population standard deviation of the relation's probability over the samples
    (ops.pair_prob_std_mc on the proposed ids); padding is -1 / -inf / 0."""
    return _predict_relations(z, w, s, o, k, pair_filter, flow_log_probs, True, type_constraint, mc=True)


def predict_relations_mc_unfused(z, w, s, o, k, pair_filter=None, flow_log_probs=None, type_constraint=None):
    """``predict_relations_mc`` from materialised probabilities (``pair_pbar_unfused`` + ``topk_from_scores``)."""
    return _predict_relations(z, w, s, o, k, pair_filter, flow_log_probs, False, type_constraint, mc=True)
