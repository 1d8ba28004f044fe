"""TransE, the baseline of Table 2 next to R-GCN and GCN-VAE (baselines/transe: OpenKE's TransE, MarginLoss, NegativeSampling,
Trainer and main.py), trained and evaluated on the device.

Model and loss keep the reference's semantics, class names and state-dict keys (``zero_const``, ``pi_const``,
``ent_embeddings.weight``, ``rel_embeddings.weight``) and its xavier-uniform initialisation, so a seeded model starts from the
reference's tables and a reference checkpoint loads.  Every training row is scored in OpenKE's 'normal' mode,
``||n(h) + n(r) - n(t)||_p`` with ``n = F.normalize`` under ``norm_flag``; the loss is ``mean(max(p - n, -margin)) + margin``
(self-adversarial: detached ``softmax(-n * T)`` weights summed over each positive's negatives) plus ``regul_rate`` times the mean
of the squares of the raw batch rows.  The ``margin`` / ``epsilon`` model arguments (a different score, ``margin - d``, and a
uniform init) are not used by main.py and are refused.

Negative sampler (OpenKE's library is not part of the reference; this is the rule implemented):
  * a batch of ``B = len(train) // nbatches`` positives is drawn uniformly with replacement (OpenKE's 'normal' mode) and
    ``neg_ent`` negatives per positive, laid out as the B positives, then ``neg_ent`` blocks of B;
  * with ``bern_flag`` the head is corrupted with probability ``tph / (tph + hpt)`` of the positive's relation (Wang et al. 2014;
    tph: triples per distinct head, hpt: triples per distinct tail), the tail otherwise; without it always the tail;
  * with ``filter_flag`` the replacement is uniform over the entities that form NO known training triple with the kept pair:
    a draw ``u`` in ``[0, V - k)`` maps to the u-th entity absent from the k known answers of ``FilterIndex(train)``
    (``nth_unlisted``); with ``k == V`` or without the filter the draw is uniform over all V entities;
  * relations are never corrupted (``neg_rel = 0``).
The draws are Philox4x32-10 keyed by the device RNG's {seed, tick} (include/gcnvae.h, gv_transe_sample), so a captured step
samples anew at every replay.

Device path (k_transe.hip): one sampler launch, one fused forward / loss / backward launch writing a gradient row per occurrence,
two gv_build_csr orderings of the occurrences, and one launch that sums each touched row's occurrences in a fixed order and applies
``p += -lr * g`` (rows without occurrences are not written, as torch's dense SGD leaves them).  No float atomics: a step is
bit-identical run to run and eager vs captured.  The loss stays on the device; the per-epoch sum is read once per epoch.

Optimisers: the reference Trainer's ``opt_method`` / ``alpha`` / ``weight_decay`` / ``lr_decay`` (torch.optim's SGD, Adagrad,
Adadelta, Adam at torch's defaults) are ``DeviceTrainer(opt_method=..., weight_decay=..., lr_decay=...)`` and the CLI's
``--optimizer`` / ``--weight-decay`` / ``--lr-decay`` (``--opt-method`` itself stays at sgd).  Plain SGD keeps the launch above;
every other choice replaces it by ``ops.transe_apply_opt`` (gv_transe_apply_opt): the same ordered per-row sum, then the chosen
rule, with the state (two arrays per table, ``ops.TransEOptState``) and the step number on the device -- the step number is
advanced on the stream inside the step, so a captured graph's replays see it grow.  Semantics are torch's dense ones: Adadelta,
Adam and any weight decay update every row of both tables at every step, SGD and Adagrad without decay only the touched rows.
``apply_unfused`` states the update with ``index_add_`` and a real ``torch.optim`` step.  Checkpoints are the model's state dict,
as in the reference: the optimiser state is not saved, and a resumed run starts it from zero.

Evaluation: raw and filtered MRR, MR and Hits@1/3/10 over both directions, filter = train + valid + test.  Ranks are exactly
``ranking.sort_and_rank(-distance, target)``: tail queries ``q = n(h) + n(r)``, head queries ``q = n(t) - n(r)``, both
``||q - n(E_j)||_p`` (``h' + (r - t)`` and ``h' - (t - r)`` round alike), from ``ops.transe_rank_filtered``, which never stores
the distance matrix.  The ``*_unfused`` functions are the plain-torch statement of the same rules: the in-repo cross-check and
the bench's comparator, never a fallback.

Link prediction: ``predict_topk`` names the ``k`` nearest entities of every query, (a, r, ?) or (?, r, a), with the query's known
answers left out when a ``FilterIndex`` is given -- the same queries, table and distances as the ranker, selected by
``ops.transe_topk`` (gv_transe_topk) without the distance matrix.  ``topk_from_distances`` states the order on a materialised
matrix: distance ascending, ties by lower id, NaN last.  ``--predict-topk K --predict-out FILE`` writes both directions of the
test split (filter: train + valid + test) in train.py's prediction TSV layout, the distance in place of the logit.

Completion: ``mine_triplets`` selects among ALL N x R x N triplets the K nearest new ones, or all within a distance -- the
distances of ``predict_topk(direction='o')``, the reference's 'normal' mode (h + r) - t -- from ``ops.transe_mine``
(gv_transe_mine: subject and object tiles of the normalised table stay in LDS while the relations are walked over them).
``mine_from_distances`` states the rule on a materialised (R, N, N) tensor; ``mine_triplets_unfused`` is the per-relation
cross-check.  ``--complete-topk K`` / ``--complete-threshold D`` write them to ``--complete-out`` in train.py's layout.  With a
``type_constraint`` (``--complete-typed``) only type-correct triplets are mined, by ``ops.transe_mine_typed``
(gv_transe_mine_typed: by relation, over that relation's subject and object member lists).

Per-entity completion: ``complete_entities`` answers "what is this entity missing?" -- an entity's ``k`` nearest new facts over
ALL relations, as subject (``side='s'``) or as object (``side='o'``), at ``predict_topk``'s distances, from ``ops.transe_entity_topk``
(gv_transe_entity_topk: one sorted list per entity while the relations are walked; no (entity x relation) query matrix).
``complete_entities_from_distances`` states the rule on a materialised (m, R, N) tensor; ``complete_entities_unfused`` is the
per-relation cross-check.  ``--profile-topk K --profile-entities IDS|FILE --profile-out FILE`` write both sides in train.py's
profile layout, the distance in place of the logit and probability.  With a ``type_constraint`` (``--profile-typed``) only
type-correct facts are candidates, from ``ops.transe_entity_topk_typed`` (gv_transe_entity_topk_typed: the relations' candidate
member lists are walked, rows gathered through the ids).

Per-relation completion: ``complete_relations`` answers "which pairs belong to this relation?" -- every relation's OWN k nearest new
facts, at ``predict_topk(direction='o')``'s distances, from ``ops.transe_relation_topk`` (gv_transe_mine_by_relation: the miner's
loop order over the chosen relations, each with its own threshold, prefix, early-exit bound, histogram, counter and output segment,
so all lists come from the same few sweeps).  ``complete_relations_from_distances`` states the rule on a materialised (R, N, N)
tensor; ``complete_relations_unfused`` is the per-relation cross-check.  ``--relation-profile-topk K --relation-profile-ids IDS|FILE
--relation-profile-out FILE`` write ``s r o rank distance`` in train.py's relation-profile layout; with a ``type_constraint``
(``--relation-profile-typed``) only type-correct pairs are candidates (gv_transe_mine_typed_by_relation).  There is no Monte-Carlo
form: TransE has no posterior.

Relation prediction: ``rank_relations`` / ``evaluate_relations`` rank the true relation of every pair (s, ?, o) among all relations
at distance ``||(n(o) - n(s)) - n(r)||_p`` -- in exact arithmetic the triplet's distance, though not ``predict_topk``'s bit pattern
for it: the operands are associated differently --, raw and with a ``ranking.PairFilterIndex`` filtered, and
``predict_relations`` proposes the k nearest new relations of a pair, from ``ops.transe_pair_relations`` (gv_transe_pair_rel: one
launch, the query row formed while it is staged, every relation tile walked by the workgroup that owns the pairs).  The
``*_unfused`` twins (``ops.transe_distances`` + ``topk_from_distances``) are the cross-check.  With a ``type_constraint``
(``--relations-typed``) the three also answer among the pair's type-correct relations (gv_transe_pair_rel_constrained: the AND of two
rows of ``TypeConstraint.relation_words``; the keys get ``_constrained``).  ``--relation-eval`` adds the report
(with ``--filtered-eval`` the filtered figures too), ``--predict-relations K --relations-out FILE`` write train.py's relation TSV
layout, the distance in place of the logit.  Relation-corrupted training negatives (``--neg-rel``) stay refused.

    python -m gcn_vae_amd.transe -d FB15k-237-synthetic --gpu 0 --train-times 5 --filtered-eval
    python -m gcn_vae_amd.transe -d FB15k-237-synthetic --gpu 0 --train-times 5 --predict-topk 10 --predict-out transe.tsv
    python -m gcn_vae_amd.transe -d FB15k-237-synthetic --gpu 0 --train-times 5 --optimizer adam --alpha 0.001 --graph-step
"""
import argparse
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ranking import (FilterIndex, MineOverflow, TypeConstraint, _listed_mask, _mine_args, _mine_filter, _mine_from_values, _mine_members,
                      UNCONSTRAINED, _complete_constraint, _complete_mask_args, _complete_queries, _complete_side, _complete_unfused,
                      _mine_unfused, complete_entities_from_scores, mid_ranks, rank_from_scores_constrained, topk_from_scores,
                      PairFilterIndex, _pair_cat, _pair_checked, _pair_chunks, relation_ranks_from_scores, _relation_masks,
                      _relation_pairs, _relation_rows)
from .train import profile_entities_arg, relation_profile_ids_arg, write_profile_lines, write_relation_lines


# ------------------------------------------------------------------------------------------------
# model and loss (the reference's modules)
# ------------------------------------------------------------------------------------------------
class BaseModule(nn.Module):
    def __init__(self):
        super().__init__()
        self.zero_const = nn.Parameter(torch.Tensor([0]))
        self.zero_const.requires_grad = False
        self.pi_const = nn.Parameter(torch.Tensor([3.14159265358979323846]))
        self.pi_const.requires_grad = False

    def load_checkpoint(self, path):
        self.load_state_dict(torch.load(path, map_location='cpu'))
        self.eval()

    def save_checkpoint(self, path):
        torch.save(self.state_dict(), path)


class TransE(BaseModule):
    def __init__(self, ent_tot, rel_tot, dim=100, p_norm=1, norm_flag=True, margin=None, epsilon=None):
        super().__init__()
        if margin is not None or epsilon is not None:
            raise ValueError('TransE(margin=..., epsilon=...) selects the reference\'s margin - d score and uniform init, which '
                             'main.py never uses: not supported (pass the margin to MarginLoss)')
        if p_norm not in (1, 2):
            raise ValueError(f'p_norm must be 1 or 2, got {p_norm}')
        self.ent_tot, self.rel_tot, self.dim, self.p_norm, self.norm_flag = ent_tot, rel_tot, dim, p_norm, norm_flag
        self.margin, self.epsilon, self.margin_flag = None, None, False
        self.ent_embeddings = nn.Embedding(ent_tot, dim)
        self.rel_embeddings = nn.Embedding(rel_tot, dim)
        nn.init.xavier_uniform_(self.ent_embeddings.weight.data)
        nn.init.xavier_uniform_(self.rel_embeddings.weight.data)

    def _calc(self, h, t, r, mode):
        return score_rule(h, r, t, self.p_norm, self.norm_flag, mode)

    def forward(self, data):
        h = self.ent_embeddings(data['batch_h'])
        t = self.ent_embeddings(data['batch_t'])
        r = self.rel_embeddings(data['batch_r'])
        return self._calc(h, t, r, data['mode'])

    def regularization(self, data):
        h = self.ent_embeddings(data['batch_h'])
        t = self.ent_embeddings(data['batch_t'])
        r = self.rel_embeddings(data['batch_r'])
        return (torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2)) / 3

    def predict(self, data):
        return self.forward(data).cpu().data.numpy()


def score_rule(h, r, t, p_norm, norm_flag, mode='normal'):
    """The reference's TransE._calc in plain torch."""
    if norm_flag:
        h, r, t = F.normalize(h, 2, -1), F.normalize(r, 2, -1), F.normalize(t, 2, -1)
    if mode != 'normal':
        h = h.view(-1, r.shape[0], h.shape[-1])
        t = t.view(-1, r.shape[0], t.shape[-1])
        r = r.view(-1, r.shape[0], r.shape[-1])
    score = h + (r - t) if mode == 'head_batch' else (h + r) - t
    return torch.norm(score, p_norm, -1).flatten()


class MarginLoss(BaseModule):
    def __init__(self, adv_temperature=None, margin=6.0):
        super().__init__()
        self.margin = nn.Parameter(torch.Tensor([margin]))
        self.margin.requires_grad = False
        if adv_temperature is not None:
            self.adv_temperature = nn.Parameter(torch.Tensor([adv_temperature]))
            self.adv_temperature.requires_grad = False
            self.adv_flag = True
        else:
            self.adv_flag = False

    def get_weights(self, n_score):
        return F.softmax(-n_score * self.adv_temperature, dim=-1).detach()

    def forward(self, p_score, n_score):
        if self.adv_flag:
            return (self.get_weights(n_score) * torch.max(p_score - n_score, -self.margin)).sum(dim=-1).mean() + self.margin
        return (torch.max(p_score - n_score, -self.margin)).mean() + self.margin


class NegativeSampling(BaseModule):
    def __init__(self, model=None, loss=None, batch_size=256, regul_rate=0.0):
        super().__init__()
        self.model, self.loss, self.batch_size, self.regul_rate = model, loss, batch_size, regul_rate

    def _get_positive_score(self, score):
        return score[:self.batch_size].view(-1, self.batch_size).permute(1, 0)

    def _get_negative_score(self, score):
        return score[self.batch_size:].view(-1, self.batch_size).permute(1, 0)

    def forward(self, data):
        score = self.model(data)
        loss_res = self.loss(self._get_positive_score(score), self._get_negative_score(score))
        if self.regul_rate != 0:
            loss_res += self.regul_rate * self.model.regularization(data)
        return loss_res


def step_unfused(ent, rel, bh, br, bt, batch, p_norm, norm_flag, margin, adv_temperature=None, regul_rate=0.0):
    """One training step's scores, loss and table gradients by torch autograd on (ent, rel) (any device): the reference's
    NegativeSampling(TransE, MarginLoss) forward and backward.  Returns (score, loss, g_ent, g_rel)."""
    e = ent.detach().clone().requires_grad_(True)
    r = rel.detach().clone().requires_grad_(True)
    bh, br, bt = (x.to(device=ent.device, dtype=torch.long) for x in (bh, br, bt))
    score = score_rule(e[bh], r[br], e[bt], p_norm, norm_flag)
    loss_fn = MarginLoss(adv_temperature, margin).to(ent.device)
    p = score[:batch].view(-1, batch).permute(1, 0)
    n = score[batch:].view(-1, batch).permute(1, 0)
    loss = loss_fn(p, n)
    if regul_rate != 0:
        h_, t_, r_ = e[bh], e[bt], r[br]
        loss = loss + regul_rate * ((torch.mean(h_ ** 2) + torch.mean(t_ ** 2) + torch.mean(r_ ** 2)) / 3)
    loss.backward()
    return score.detach(), loss.detach().reshape(()), e.grad, r.grad


# ------------------------------------------------------------------------------------------------
# negative sampling rules (host statements of gv_transe_sample)
# ------------------------------------------------------------------------------------------------
def bern_head_prob(train, num_rels):
    """Per relation tph / (tph + hpt): the probability that the head is the corrupted side (OpenKE's bern mode)."""
    t = torch.as_tensor(np.asarray(train), dtype=torch.long).reshape(-1, 3)
    out = torch.full((num_rels,), 0.5, dtype=torch.float64)
    for rr in torch.unique(t[:, 1]).tolist():
        sel = t[t[:, 1] == rr]
        n = float(sel.shape[0])
        tph = n / float(torch.unique(sel[:, 0]).numel())
        hpt = n / float(torch.unique(sel[:, 2]).numel())
        out[rr] = tph / (tph + hpt)
    return out.to(torch.float32)


def nth_unlisted(listed, u):
    """The u-th (0-based) integer >= 0 not in the sorted unique list ``listed``: u + #{j : listed[j] - j <= u} (binary search)."""
    lo, hi = 0, len(listed)
    while lo < hi:
        m = (lo + hi) // 2
        if int(listed[m]) - m <= u:
            lo = m + 1
        else:
            hi = m
    return u + lo


def map_draw(word, n):
    """A uint32 draw onto [0, n): multiply-shift (the sampler's rule)."""
    return (int(word) * int(n)) >> 32


class TrainFilter:
    """The FilterIndex(train) runs of every training triple, both directions, as gv_transe_sample reads them: f_lo / f_hi
    [2 n_train] (slot 2i: the known tails of (h, r); 2i + 1: the known heads of (t, r)) into ent['o'] / ent['s']."""

    def __init__(self, train, num_nodes, num_rels, device):
        train = torch.as_tensor(np.asarray(train), dtype=torch.long).reshape(-1, 3)
        self.index = FilterIndex(num_nodes, num_rels, train)
        lo_o, hi_o = self.index.lookup(train[:, 0], train[:, 1], 'o')
        lo_s, hi_s = self.index.lookup(train[:, 2], train[:, 1], 's')
        i32 = dict(dtype=torch.int32, device=device)
        self.f_lo = torch.stack([lo_o, lo_s], 1).reshape(-1).to(**i32).contiguous()
        self.f_hi = torch.stack([hi_o, hi_s], 1).reshape(-1).to(**i32).contiguous()
        self.ent_o = self.index.entities('o', device).contiguous()
        self.ent_s = self.index.entities('s', device).contiguous()

    def tuple(self):
        return (self.f_lo, self.f_hi, self.ent_o, self.ent_s)


def sample_from_draws(draws, train, num_nodes, batch, neg_ent, p_head=None, train_filter=None):
    """The batch gv_transe_sample makes from its raw words (``draws`` [batch, neg_ent + 2] uint32), restated on the host."""
    train = np.asarray(train).reshape(-1, 3)
    d = np.asarray(draws, dtype=np.int64) & 0xFFFFFFFF
    n = batch * (1 + neg_ent)
    bh, br, bt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    f_lo = f_hi = None
    if train_filter is not None:
        f_lo, f_hi = train_filter.f_lo.cpu().numpy(), train_filter.f_hi.cpu().numpy()
        ents = {0: train_filter.ent_o.cpu().numpy(), 1: train_filter.ent_s.cpu().numpy()}
    ph = None if p_head is None else np.asarray(p_head.cpu() if isinstance(p_head, torch.Tensor) else p_head, np.float32)
    for b in range(batch):
        i = map_draw(d[b, 0], len(train))
        h, r, t = (int(x) for x in train[i])
        head = bool(ph is not None and np.float32((d[b, 1] >> 8) * np.float32(1.0 / 16777216.0)) < ph[r])
        bh[b], br[b], bt[b] = h, r, t
        listed = None
        if f_lo is not None:
            slot = 2 * i + int(head)
            listed = ents[int(head)][f_lo[slot]:f_hi[slot]]
            if len(listed) >= num_nodes:
                listed = None
        for j in range(neg_ent):
            w = d[b, 2 + j]
            u = map_draw(w, num_nodes - (len(listed) if listed is not None else 0))
            if listed is not None:
                u = nth_unlisted(listed, u)
            o = batch * (j + 1) + b
            bh[o], br[o], bt[o] = (u, r, t) if head else (h, r, u)
    return bh, br, bt


# ------------------------------------------------------------------------------------------------
# device trainer
# ------------------------------------------------------------------------------------------------
OPT_METHODS = ('sgd', 'adagrad', 'adadelta', 'adam')


def make_optimizer(params, opt_method='sgd', alpha=1.0, weight_decay=0.0, lr_decay=0.0):
    """The ``torch.optim`` optimiser the reference's Trainer builds from ``opt_method`` (case-insensitive), ``alpha``,
    ``weight_decay`` and, for Adagrad only, ``lr_decay``; everything else at torch's defaults.  What ``apply_unfused`` steps."""
    name = str(opt_method).lower()
    if name == 'adagrad':
        return torch.optim.Adagrad(params, lr=alpha, lr_decay=lr_decay, weight_decay=weight_decay)
    if name == 'adadelta':
        return torch.optim.Adadelta(params, lr=alpha, weight_decay=weight_decay)
    if name == 'adam':
        return torch.optim.Adam(params, lr=alpha, weight_decay=weight_decay)
    if name == 'sgd':
        return torch.optim.SGD(params, lr=alpha, weight_decay=weight_decay)
    raise ValueError(f'opt_method {opt_method!r}: expected one of {OPT_METHODS}')


def apply_unfused(ent, rel, g_ent_rows, occ_ent, g_rel_rows, occ_rel, optimizer):
    """The update of ``ops.transe_apply_opt`` in plain torch (any device, any dtype): the occurrence rows are ``index_add_``-ed
    into dense gradients of the two tables (row i of ``g_ent_rows`` belongs to entity ``occ_ent[i]``, row i of ``g_rel_rows`` to
    relation ``occ_rel[i]``) and ``optimizer`` -- a ``torch.optim`` optimiser over ``[ent, rel]``, e.g. ``make_optimizer`` --
    takes one step.  The tables are updated in place.  The cross-check and the bench's comparator, never a fallback."""
    for table, rows, occ in ((ent, g_ent_rows, occ_ent), (rel, g_rel_rows, occ_rel)):
        occ = occ.to(device=table.device, dtype=torch.long)
        table.grad = torch.zeros_like(table).index_add_(0, occ, rows.to(device=table.device, dtype=table.dtype))
    optimizer.step()
    return ent, rel


class DeviceTrainer:
    """TransE training on the device: ``step()`` = sample + fused step + orderings + optimiser update, ``capture()`` records one
    step as a hipGraph that ``step()`` then replays.  ``model``'s two embedding tables are updated in place.  ``opt_method``
    ('sgd', 'adagrad', 'adadelta', 'adam', case-insensitive), ``weight_decay`` and ``lr_decay`` (Adagrad only) are the reference
    Trainer's; ``alpha`` is the learning rate of every method.  The optimiser state (``opt_state``) lives on the device."""

    def __init__(self, model, train, nbatches=100, neg_ent=25, bern_flag=True, filter_flag=True, margin=5.0, alpha=1.0,
                 adv_temperature=None, regul_rate=0.0, device='cuda', opt_method='sgd', weight_decay=0.0, lr_decay=0.0):
        self.opt_method = str(opt_method).lower()
        if self.opt_method not in OPT_METHODS:
            raise ValueError(f'opt_method {opt_method!r}: expected one of {OPT_METHODS}')
        self.weight_decay, self.lr_decay = float(weight_decay), float(lr_decay)
        if not self.weight_decay >= 0 or not self.lr_decay >= 0:
            raise ValueError(f'weight_decay={weight_decay} lr_decay={lr_decay}: both must be >= 0')
        if (self.opt_method != 'sgd' or self.weight_decay != 0) and not float(alpha) >= 0:
            raise ValueError(f'alpha={alpha}: must be >= 0 with opt_method {self.opt_method!r} / weight_decay')
        if self.lr_decay != 0 and self.opt_method != 'adagrad':
            raise ValueError('lr_decay is Adagrad\'s (the reference passes it to no other optimiser)')
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.model = model
        train = np.asarray(train).reshape(-1, 3)
        self.n_train = len(train)
        self.batch = self.n_train // nbatches
        if self.batch < 1:
            raise ValueError(f'{self.n_train} training triples cannot make {nbatches} batches')
        self.nbatches, self.neg_ent = nbatches, neg_ent
        self.margin, self.alpha, self.adv, self.regul = float(margin), float(alpha), adv_temperature, float(regul_rate)
        self.ent, self.rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
        if self.ent.device != self.device:
            raise ValueError('move the model to the device first')
        if len(train) and (train[:, [0, 2]].min() < 0 or train[:, [0, 2]].max() >= model.ent_tot or train[:, 1].min() < 0
                           or train[:, 1].max() >= model.rel_tot):
            raise ValueError(f'training triples out of range of the model ({model.ent_tot} entities, {model.rel_tot} relations)')
        self.train = torch.as_tensor(train, dtype=torch.int32).to(self.device).contiguous()
        self.p_head = bern_head_prob(train, model.rel_tot).to(self.device) if bern_flag else None
        self.filt = TrainFilter(train, model.ent_tot, model.rel_tot, self.device).tuple() if filter_flag else None
        self.rng = ops.device_rng(self.device)
        self.stream_id = ops.new_rng_stream()
        B, K, dim = self.batch, neg_ent, model.dim
        i32 = dict(dtype=torch.int32, device=self.device)
        n = B * (1 + K)
        self.bh, self.br, self.bt = (torch.empty(n, **i32) for _ in range(3))
        self.grads = (torch.empty((2 + K) * B, dim, device=self.device), torch.empty(B, dim, device=self.device),
                      torch.empty(B, device=self.device))
        self.occ_ent = torch.empty((2 + K) * B, **i32)
        self.order = ops.TransEOrder((2 + K) * B, model.ent_tot, B, model.rel_tot, self.device)
        self.loss = torch.zeros(1, device=self.device)
        self.epoch_loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        # plain SGD keeps gv_transe_apply (and its bits); everything else goes through gv_transe_apply_opt with this state
        self.opt_state = None
        if self.opt_method != 'sgd' or self.weight_decay != 0:
            self.opt_state = ops.TransEOptState(model.ent_tot, model.rel_tot, dim, self.device)
        self.graph = None

    def _step(self):
        B, K = self.batch, self.neg_ent
        self.rng.tick()
        # ids, relation shares and filter runs were validated once, at construction: no read-back inside the (captured) step
        ops.transe_sample(self.rng.state, self.stream_id, self.train, self.model.ent_tot, B, K, self.p_head, self.filt,
                          self.bh, self.br, self.bt, check=False)
        g_ent, g_rel, part = ops.transe_step(self.ent, self.rel, self.bh, self.br, self.bt, B, K, self.model.p_norm,
                                             self.model.norm_flag, self.margin, self.adv, self.regul, out=self.grads,
                                             occ_ent=self.occ_ent, check=False)
        order = self.order.build(self.occ_ent, self.br[:B])
        if self.opt_state is None:
            ops.transe_apply(self.ent, self.rel, g_ent, g_rel, order, self.alpha, part, self.margin, self.loss, self.epoch_loss)
        else:
            ops.transe_apply_opt(self.ent, self.rel, g_ent, g_rel, order, self.opt_method, self.alpha, part, self.margin, self.loss,
                                 self.epoch_loss, state=self.opt_state, weight_decay=self.weight_decay, lr_decay=self.lr_decay)

    def capture(self):
        """Record one step.  A warm-up step runs first, outside capture (library load, the orderings' first launches); the tables,
        the RNG state and the optimiser state with its step number are restored after it, so a captured run takes exactly the
        steps an eager run takes, with the same draws.  The step number is advanced on the stream inside the step, so every
        replay sees the next one."""
        saved = (self.ent.clone(), self.rel.clone(), self.rng.state.clone())
        opt_saved = self.opt_state.snapshot() if self.opt_state is not None else None
        self._step()
        self.ent.copy_(saved[0])
        self.rel.copy_(saved[1])
        self.rng.state.copy_(saved[2])
        if opt_saved is not None:
            self.opt_state.restore(opt_saved)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._step()
        return self

    def step(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self._step()

    def epoch(self):
        """nbatches steps; returns the summed loss (read back once)."""
        self.epoch_loss.zero_()
        for _ in range(self.nbatches):
            self.step()
        return float(self.epoch_loss.item())


# ------------------------------------------------------------------------------------------------
# evaluation
# ------------------------------------------------------------------------------------------------
MAX_QUERY_ROWS = 16384      # queries per ranker launch


def _summary(raw, filt, hits, suffix=''):
    out = {}
    for kind, ranks in (('raw' + suffix, raw + 1), ('filtered' + suffix, filt + 1)):
        ranks = ranks.double()
        out['mrr_' + kind] = torch.mean(1.0 / ranks).item()
        out['mr_' + kind] = torch.mean(ranks).item()
        out['hits_' + kind] = {h: torch.mean((ranks <= h).double()).item() for h in hits}
    return out


def _rank_directions(ent, triplets, step, filter_index, n_kinds, rank_chunk):
    """The direction x chunk loop of the four rankers, once: all head queries (?, r, o), then all tail queries (s, r, ?), ``step``
    at a time through ``rank_chunk(head, direction, a, r, b, filt)`` -- ``filt`` the chunk's ``(filt_lo, filt_hi, filt_ent)``, three
    None without a ``filter_index`` --, which returns the chunk's ``n_kinds`` ranks, raw and filtered alternating.  A filtered one
    that comes back None (no filter) is its unfiltered twin."""
    s, r, o = (triplets[:, i].to(ent.device).long() for i in range(3))
    out = [[] for _ in range(n_kinds)]
    for head, a, b, d in ((True, o, s, 's'), (False, s, o, 'o')):
        ent_f = filter_index.entities(d, ent.device) if filter_index is not None else None
        for lo in range(0, a.numel(), step):
            sl = slice(lo, min(a.numel(), lo + step))
            filt = (*filter_index.lookup(a[sl], r[sl], d), ent_f) if filter_index is not None else (None, None, None)
            ranks = rank_chunk(head, d, a[sl], r[sl], b[sl], filt)
            for i, acc in enumerate(out):
                acc.append(ranks[i - 1] if ranks[i] is None else ranks[i])
    return tuple(torch.cat(x) for x in out)


def rank_transe(ent, rel, triplets, p_norm, norm_flag, filter_index=None):
    """(raw, filtered) 0-based ranks, head queries of every triplet then tail queries, from the fused ranker."""
    en = ops.transe_queries(ent, norm_flag=norm_flag)                     # the normalised table, once

    def rank_chunk(head, d, a, r, b, filt):
        q = ops.transe_queries(ent, rel, a, r, head=head, norm_flag=norm_flag)
        return ops.transe_rank_filtered(q, en, b, p_norm, *filt)
    return _rank_directions(ent, triplets, MAX_QUERY_ROWS, filter_index, 2, rank_chunk)


def rank_transe_unfused(ent, rel, triplets, p_norm, norm_flag, filter_index=None, batch=32):
    """``rank_transe`` in plain torch on materialised distances: the reference's head_batch / tail scores of every entity,
    ``sort_and_rank(-distance)``'s rule, the filtered count over the entities the filter does not list."""
    v = ent.shape[0]

    def rank_chunk(head, d, a, r, b, filt):
        cand = ent.unsqueeze(0).expand(a.numel(), v, ent.shape[1])
        fix = ent[a].unsqueeze(1).expand_as(cand)
        rr = rel[r].unsqueeze(1).expand_as(cand)
        if norm_flag:
            cand, fix, rr = F.normalize(cand, 2, -1), F.normalize(fix, 2, -1), F.normalize(rr, 2, -1)
        diff = cand + (rr - fix) if head else (fix + rr) - cand
        dist = torch.norm(diff, p_norm, -1)
        listed = None if filter_index is None else _listed_mask(*filt, a.numel(), v, dist.device)
        return mid_ranks(-dist, b, listed)[:2]
    return _rank_directions(ent, triplets, batch, filter_index, 2, rank_chunk)


def rank_transe_constrained(ent, rel, triplets, p_norm, norm_flag, type_constraint, filter_index=None):
    """(raw, filtered, raw_constrained, filtered_constrained) 0-based ranks in ``rank_transe``'s order (head queries of every
    triplet, then tail queries) from the fused ranker: the constrained ranks count the members of the relation's type set only
    (``ranking.TypeConstraint``: subjects of r for a head query, objects of r for a tail query).  Without a filter the two
    filtered ones equal their unfiltered twins, as ``rank_transe``'s do."""
    en = ops.transe_queries(ent, norm_flag=norm_flag)                     # the normalised table, once
    words = type_constraint.words.to(ent.device)

    def rank_chunk(head, d, a, r, b, filt):
        q = ops.transe_queries(ent, rel, a, r, head=head, norm_flag=norm_flag)
        return ops.transe_rank_constrained(q, en, b, p_norm, words, type_constraint.set_ids(r, d), *filt)
    return _rank_directions(ent, triplets, MAX_QUERY_ROWS, filter_index, 4, rank_chunk)


def rank_transe_constrained_unfused(ent, rel, triplets, p_norm, norm_flag, type_constraint, filter_index=None, batch=1024):
    """``rank_transe_constrained`` on materialised distances: ``ranking.rank_from_scores_constrained`` on
    ``-ops.transe_distances`` -- the bits the fused ranker compares -- chunk by chunk."""
    en = ops.transe_queries(ent, norm_flag=norm_flag)

    def rank_chunk(head, d, a, r, b, filt):
        q = ops.transe_queries(ent, rel, a, r, head=head, norm_flag=norm_flag)
        listed = None if filter_index is None else _listed_mask(*filt, a.numel(), ent.shape[0], ent.device)
        cand = type_constraint.mask(type_constraint.set_ids(r, d), ent.device)
        return rank_from_scores_constrained(-ops.transe_distances(q, en, p_norm), b, cand, listed)
    return _rank_directions(ent, triplets, batch, filter_index, 4, rank_chunk)


def evaluate(model, triplets, filter_index=None, hits=(1, 3, 10), unfused=False, verbose=True, type_constraint=None):
    """Raw MRR, MR and Hits@k over both directions, and the filtered ones when ``filter_index`` is given (a FilterIndex,
    train + valid + test).  Returns {'mrr_raw', 'mr_raw', 'hits_raw': {k: v}} plus the same '_filtered' keys with a filter.
    With a ``type_constraint`` (ranking.TypeConstraint) the type-constrained protocol is reported too: '_raw_constrained' keys,
    and '_filtered_constrained' ones with a filter."""
    with torch.no_grad():
        ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
        triplets = torch.as_tensor(np.asarray(triplets), dtype=torch.long).reshape(-1, 3)
        if type_constraint is None:
            fn = rank_transe_unfused if unfused else rank_transe
            raw, filt = fn(ent, rel, triplets, model.p_norm, model.norm_flag, filter_index)
            out = _summary(raw, filt, hits)
        else:
            fn = rank_transe_constrained_unfused if unfused else rank_transe_constrained
            raw, filt, raw_c, filt_c = fn(ent, rel, triplets, model.p_norm, model.norm_flag, type_constraint, filter_index)
            out = _summary(raw, filt, hits)
            out.update(_summary(raw_c, filt_c, hits, '_constrained'))
    kinds = ('raw', 'filtered') if filter_index is not None else ('raw',)
    if type_constraint is not None:
        kinds = kinds + tuple(k + '_constrained' for k in kinds)
    if filter_index is None:         # without a filter the "filtered" ranks are the raw ones: not reported
        out = {k: v for k, v in out.items() if '_filtered' not in k}
    if verbose:
        for kind in kinds:
            print('MRR ({}): {:.6f} | MR ({}): {:.3f}'.format(kind, out['mrr_' + kind], kind, out['mr_' + kind]))
            for h in hits:
                print('Hits ({}) @ {}: {:.6f}'.format(kind, h, out['hits_' + kind][h]))
    return out


# ------------------------------------------------------------------------------------------------
# link prediction
# ------------------------------------------------------------------------------------------------
def topk_from_distances(dist, k, filt_lo=None, filt_hi=None, filt_ent=None, cand=None):
    """The top-k rule of ``ops.transe_topk`` on a materialised (m, v) distance matrix, in plain torch (any device):
    ``ranking.topk_from_scores(-dist, ...)`` -- smaller distance first, equal distances by lower id, NaN after every number (+inf
    included) and by id among themselves, the ids in ``filt_ent[filt_lo[i]:filt_hi[i]]`` no candidates of row i, nor the columns
    where ``cand`` (a dense (m, v) bool of allowed columns, the rule of ``ops.transe_topk_constrained``) is False.  Returns
    ``(ids int64 (m, k), dist float32 (m, k))`` padded with id -1 / distance +inf; a reported distance is the matrix entry's bit
    pattern, except that a zero is +0 and every NaN the one quiet NaN."""
    ids, neg = topk_from_scores(-dist.to(torch.float32), k, filt_lo, filt_hi, filt_ent, cand)
    out = 0.0 - neg                                                   # -(+0) would be -0; 0 - (+0) is +0
    return ids, torch.where(torch.isnan(out), torch.full_like(out, float('nan')), out)


def _tables(model_or_tables):
    if isinstance(model_or_tables, TransE):
        m = model_or_tables
        return m.ent_embeddings.weight.data, m.rel_embeddings.weight.data, m.p_norm, m.norm_flag
    ent, rel, p_norm, norm_flag = model_or_tables
    return ent.detach(), rel.detach(), p_norm, norm_flag


def _predict_topk(model_or_tables, a, r, k, direction, filter_index, select, type_constraint=None):
    if direction not in ('o', 's'):
        raise ValueError("direction is 'o' (queries (a, r, ?)) or 's' (queries (?, r, a))")
    ent, rel, p_norm, norm_flag = _tables(model_or_tables)
    k = int(k)
    a, r = a.to(ent.device), r.to(ent.device)
    en = ops.transe_queries(ent, norm_flag=norm_flag)                     # the normalised table, once
    ent_f = filter_index.entities(direction, ent.device) if filter_index is not None else None
    ids, dist = [], []
    for lo in range(0, a.numel(), MAX_QUERY_ROWS):
        hi = min(a.numel(), lo + MAX_QUERY_ROWS)
        q = ops.transe_queries(ent, rel, a[lo:hi], r[lo:hi], head=direction == 's', norm_flag=norm_flag)
        f = (None, None, None)
        if filter_index is not None:
            f = (*filter_index.lookup(a[lo:hi], r[lo:hi], direction), ent_f)
        if type_constraint is None:
            i, d = select(q, en, p_norm, f)
        else:
            i, d = select(q, en, p_norm, f, type_constraint.set_ids(r[lo:hi], direction))
        ids.append(i)
        dist.append(d)
    if not ids:
        return (torch.zeros(0, k, dtype=torch.int64, device=ent.device), torch.zeros(0, k, dtype=torch.float32, device=ent.device))
    return torch.cat(ids), torch.cat(dist)


def predict_topk(model_or_tables, a, r, k, direction='o', filter_index=None, type_constraint=None):
    """Link prediction: the ``k`` nearest entities of every query, ``direction`` 'o' for (a[i], r[i], ?) with
    ``q = n(a) + n(r)`` and 's' for (?, r[i], a[i]) with ``q = n(a) - n(r)``, at distance ``||q - n(E_j)||_p`` -- the queries and
    distances of ``rank_transe``.  ``model_or_tables`` is a ``TransE`` or ``(ent, rel, p_norm, norm_flag)``.  With a
    ``FilterIndex`` the query's known answers are left out (new facts only).  One fused launch pair per ``MAX_QUERY_ROWS``
    queries (ops.transe_topk); returns ``(ids int64 (n, k), dist float32 (n, k))`` in the order of ``topk_from_distances``.
    With a ``ranking.TypeConstraint`` only the members of the relation's ``direction`` type set are proposed
    (ops.transe_topk_constrained)."""
    with torch.no_grad():
        if type_constraint is None:
            return _predict_topk(model_or_tables, a, r, k, direction, filter_index,
                                 lambda q, en, p, f: ops.transe_topk(q, en, k, p, *f))
        words = type_constraint.words.to(_tables(model_or_tables)[0].device)
        return _predict_topk(model_or_tables, a, r, k, direction, filter_index,
                             lambda q, en, p, f, sets: ops.transe_topk_constrained(q, en, k, p, words, sets, *f), type_constraint)


def predict_topk_unfused(model_or_tables, a, r, k, direction='o', filter_index=None, type_constraint=None):
    """``predict_topk`` from materialised distances (``ops.transe_distances`` + ``topk_from_distances`` per chunk): the in-repo
    cross-check and the bench's comparator, never a fallback."""
    with torch.no_grad():
        def select(q, en, p, f, sets=None):
            cand = None if sets is None else type_constraint.mask(sets, q.device)
            return topk_from_distances(ops.transe_distances(q, en, p), k, *f, cand)
        return _predict_topk(model_or_tables, a, r, k, direction, filter_index, select, type_constraint)


def write_predictions(path, model_or_tables, triplets, k, filter_index, type_constraint=None):
    """Top-k link predictions for both directions of every triplet, the known answers (``filter_index``) left out, as TSV in
    train.py's layout: ``direction  query_entity  relation  position  predicted_entity  distance`` -- 'o' lines answer (s, r, ?),
    's' lines (?, r, o); a query with fewer than k candidates ends in id -1, distance inf.  With a ``type_constraint`` only members of the
    relation's type set on that side are written.  Returns the number of lines written."""
    triplets = torch.as_tensor(np.asarray(triplets), dtype=torch.long).reshape(-1, 3)
    n = 0
    with open(path, 'w') as f:
        for d, a in (('o', triplets[:, 0]), ('s', triplets[:, 2])):
            r = triplets[:, 1]
            ids, dist = predict_topk(model_or_tables, a, r, k, direction=d, filter_index=filter_index, type_constraint=type_constraint)
            n += _write_rows(f, d, a.tolist(), r.tolist(), ids.tolist(), dist.tolist())
    return n


def _write_rows(f, direction, a, r, ids, values):
    for i in range(len(a)):
        head = f"{direction}\t{a[i]}\t{r[i]}\t"
        f.writelines(f"{head}{p}\t{e}\t{x:.9g}\n" for p, (e, x) in enumerate(zip(ids[i], values[i])))
    return sum(len(row) for row in ids)


# ------------------------------------------------------------------------------------------------
# relation prediction: the query is an entity pair (s, ?, o), the candidates are the relations
# ------------------------------------------------------------------------------------------------
def _pair_tables(model_or_tables):
    """(en, rn, p_norm): the two tables normalised by ``ops.transe_queries(table, norm_flag=)``, once per call."""
    ent, rel, p_norm, norm_flag = _tables(model_or_tables)
    return (ops.transe_queries(ent.contiguous(), norm_flag=norm_flag), ops.transe_queries(rel.contiguous(), norm_flag=norm_flag),
            p_norm)


def pair_distances_unfused(en, rn, s, o, p_norm):
    """The materialised (m, R) distances of the pairs: the query rows ``en[o] - en[s]`` (one fp32 subtraction per element, the
    value the fused kernel stages) against the relation table."""
    return ops.transe_distances((en[o] - en[s]).contiguous(), rn, p_norm)


def _pair_type_checked(type_constraint, n, num_rels):
    if type_constraint is not None and (type_constraint.num_nodes != n or type_constraint.num_rels != num_rels):
        raise ValueError(f'type_constraint was built for {type_constraint.num_nodes} entities / {type_constraint.num_rels} relations, '
                         f'the tables hold {n} / {num_rels}')


def _rank_relations(model_or_tables, triplets, pair_filter, fused, type_constraint=None):
    with torch.no_grad():
        en, rn, p_norm = _pair_tables(model_or_tables)
        if not isinstance(triplets, torch.Tensor):
            triplets = torch.as_tensor(np.asarray(triplets))
        triplets = triplets.to(device=en.device, dtype=torch.long).reshape(-1, 3)
        s, r, o = triplets[:, 0], triplets[:, 1], triplets[:, 2]
        _pair_checked(s, o, r, en.shape[0], rn.shape[0], pair_filter)
        _pair_type_checked(type_constraint, en.shape[0], rn.shape[0])
        cand = type_constraint.relation_words(en.device) if fused and type_constraint is not None else None
        kinds = [[] for _ in range(2 if type_constraint is None else 4)]
        for sl, f_lo, f_hi, rel in _pair_chunks(s, o, pair_filter, en.device, MAX_QUERY_ROWS):
            if fused:
                ranks = ops.transe_pair_relations(en, rn, s[sl], o[sl], p_norm, target=r[sl], filt_lo=f_lo, filt_hi=f_hi, filt_rel=rel,
                                                  cand=cand, ids_checked=True)[0]
            else:
                mask = None if type_constraint is None else type_constraint.pair_mask(s[sl], o[sl], en.device)
                ranks = relation_ranks_from_scores(-pair_distances_unfused(en, rn, s[sl], o[sl], p_norm), r[sl], f_lo, f_hi, rel, mask)
            for kind, part in zip(kinds, ranks):
                kind.append(part)
        return tuple(None if pair_filter is None and i % 2 else _pair_cat(kind, (), torch.float32, en.device)
                     for i, kind in enumerate(kinds))


def rank_relations(model_or_tables, triplets, pair_filter=None, type_constraint=None):
    """Relation prediction, ranks: for every triplet (s, r, o) the 0-based mid-rank of r among ALL relations at distance
    ``||(n(o) - n(s)) - n(r)||_p`` -- in exact arithmetic the triplet's ``||n(s) + n(r) - n(o)||``, though not the bit pattern
    ``predict_topk`` reports for it (the operands are associated differently) -- raw and, with a ``ranking.PairFilterIndex``,
    with the pair's other known relations left out.  One launch per ``MAX_QUERY_ROWS`` pairs (ops.transe_pair_relations).
    Returns ``(raw, filtered or None)``; with a ``ranking.TypeConstraint`` ``(raw, filtered, raw_constrained,
    filtered_constrained)``, the last two among the pair's type-correct relations only, the first two unchanged."""
    return _rank_relations(model_or_tables, triplets, pair_filter, True, type_constraint)


def rank_relations_unfused(model_or_tables, triplets, pair_filter=None, type_constraint=None):
    """``rank_relations`` from materialised distances (``ops.transe_distances`` + ``ranking.mid_ranks``): the in-repo cross-check
    and the bench's comparator, never a fallback."""
    return _rank_relations(model_or_tables, triplets, pair_filter, False, type_constraint)


def evaluate_relations(model_or_tables, triplets, pair_filter=None, hits=(1, 3, 10), unfused=False, verbose=True, type_constraint=None):
    """The relation-prediction report (one direction: there is one relation slot): {'mrr_raw', 'mr_raw', 'hits_raw': {k: v}} plus
    the same '_filtered' keys with a ``ranking.PairFilterIndex`` -- ``evaluate``'s key style; with a ``ranking.TypeConstraint``
    also the '_raw_constrained' keys (and '_filtered_constrained' ones with a filter)."""
    ranks = (rank_relations_unfused if unfused else rank_relations)(model_or_tables, triplets, pair_filter, type_constraint)
    raw, filt = ranks[:2]
    out = _summary(raw, raw if filt is None else filt, hits)
    kinds = ('raw', 'filtered')
    if type_constraint is not None:
        out.update(_summary(ranks[2], ranks[2] if filt is None else ranks[3], hits, '_constrained'))
        kinds = kinds + tuple(k + '_constrained' for k in kinds)
    if filt is None:
        out = {k: v for k, v in out.items() if '_filtered' not in k}
        kinds = tuple(k for k in kinds if not k.startswith('filtered'))
    if verbose:
        for kind in kinds:
            print('Relation MRR ({}): {:.6f} | MR ({}): {:.3f}'.format(kind, out['mrr_' + kind], kind, out['mr_' + kind]))
            for h in hits:
                print('Relation Hits ({}) @ {}: {:.6f}'.format(kind, h, out['hits_' + kind][h]))
    return out


def _predict_relations(model_or_tables, s, o, k, pair_filter, fused, type_constraint=None):
    with torch.no_grad():
        en, rn, p_norm = _pair_tables(model_or_tables)
        s, o = s.to(en.device), o.to(en.device)
        _pair_checked(s, o, None, en.shape[0], rn.shape[0], pair_filter)
        _pair_type_checked(type_constraint, en.shape[0], rn.shape[0])
        cand = type_constraint.relation_words(en.device) if fused and type_constraint is not None else None
        ids, dist = [], []
        for sl, f_lo, f_hi, rel in _pair_chunks(s, o, pair_filter, en.device, MAX_QUERY_ROWS):
            if fused:
                i, d = ops.transe_pair_relations(en, rn, s[sl], o[sl], p_norm, k=k, filt_lo=f_lo, filt_hi=f_hi, filt_rel=rel, cand=cand,
                                                 ids_checked=True)[1]
            else:
                mask = None if type_constraint is None else type_constraint.pair_mask(s[sl], o[sl], en.device)
                i, d = topk_from_distances(pair_distances_unfused(en, rn, s[sl], o[sl], p_norm), k, f_lo, f_hi, rel, cand=mask)
            ids.append(i)
            dist.append(d)
        return _pair_cat(ids, (int(k),), torch.int64, en.device), _pair_cat(dist, (int(k),), torch.float32, en.device)


def predict_relations(model_or_tables, s, o, k, pair_filter=None, type_constraint=None):
    """Relation prediction, proposals: the ``k`` nearest relations between ``s[i]`` and ``o[i]`` at ``rank_relations``' distances,
    the pair's known relations (``pair_filter``) left out -- with a ``ranking.TypeConstraint`` among the pair's type-correct
    relations only.  Returns ``(ids int64 (n, k), dist float32 (n, k))`` in the order of ``topk_from_distances``, padded with
    -1 / +inf when fewer than k relations are left."""
    return _predict_relations(model_or_tables, s, o, k, pair_filter, True, type_constraint)


def predict_relations_unfused(model_or_tables, s, o, k, pair_filter=None, type_constraint=None):
    """``predict_relations`` from materialised distances (``ops.transe_distances`` + ``topk_from_distances``)."""
    return _predict_relations(model_or_tables, s, o, k, pair_filter, False, type_constraint)


def write_relation_predictions(path, model_or_tables, triplets, k, pair_filter, type_constraint=None):
    """The ``k`` nearest NEW relations of every triplet's pair as TSV in train.py's layout: ``subject  object  position
    predicted_relation  distance``, one block of k lines per triplet, in order; a pair with fewer than k relations left ends in
    id -1, distance inf.  With a ``type_constraint`` only type-correct relations are written.  Returns the number of lines
    written."""
    triplets = torch.as_tensor(np.asarray(triplets), dtype=torch.long).reshape(-1, 3)
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    return write_relation_lines(path, triplets, lambda s, o: predict_relations(model_or_tables, s, o, k, pair_filter, **constrained))


# ------------------------------------------------------------------------------------------------
# completion: the whole graph's nearest new triplets
# ------------------------------------------------------------------------------------------------
def mine_from_distances(dist, *, k=None, threshold=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                        max_results=ops.MINE_MAX_RESULTS, cand_subj=None, cand_obj=None):
    """The mining rule of ``ops.transe_mine`` on a materialised tensor ``dist[r, s, o]`` (R, N, N), in plain torch (any device,
    CPU included): the counterpart of ``ranking.mine_from_scores``.  Candidates: every (s, r, o), less
    ``filt_ent[filt_lo[s * R + r]:filt_hi[s * R + r]]`` as objects of (s, r), less s == o when ``exclude_self``, less NaN
    distances (+inf is a candidate).  Order, a strict total one: distance ascending, then (s, r, o) ascending.  ``threshold=t``
    selects every candidate with d <= t, ``k=K`` the first K (fewer if fewer exist).  Returns ``(triplets int64 (n, 3), distances
    float32 (n,), info)`` in that order; ``info['count']`` is the number of candidates at or below the threshold (top-K: at or
    below the K-th distance's exact value; all, when fewer than K exist).  More than ``max_results`` of those raise
    ``MineOverflow`` carrying the count: nothing is truncated silently.  ``cand_subj`` / ``cand_obj`` (bool (R, N)): the typed rule
    of ``ops.transe_mine_typed``, as in ``ranking.mine_from_scores``."""
    return _mine_from_values(dist, True, k=k, threshold=threshold, filt_lo=filt_lo, filt_hi=filt_hi, filt_ent=filt_ent,
                            exclude_self=exclude_self, max_results=max_results, cand_subj=cand_subj, cand_obj=cand_obj)


def mine_triplets(model_or_tables, *, k=None, threshold=None, filter_index=None, exclude_self=True,
                  max_results=ops.MINE_MAX_RESULTS, type_constraint=None):
    """Knowledge-graph completion: among ALL triplets (s, r, o), at the distance ``||n(E_s) + n(R_r) - n(E_o)||_p`` of
    ``predict_topk(direction='o')``, the ``k`` nearest ones or every one with distance <= ``threshold``; with a ``FilterIndex`` the
    known triplets are left out (new facts only).  ``model_or_tables`` is a ``TransE`` or ``(ent, rel, p_norm, norm_flag)``.  One
    fused sweep per pass (ops.transe_mine); returns ``(triplets int64 (n, 3), distances float32 (n,), info)`` in the order of
    ``mine_from_distances``, and raises ``MineOverflow`` rather than truncating.  With a ``type_constraint`` (TypeConstraint) only
    type-correct triplets are candidates -- s seen as subject of r, o seen as object of r -- at the same distances, from the sweep
    over each relation's member lists (ops.transe_mine_typed)."""
    _mine_args(k, threshold, max_results)
    with torch.no_grad():
        ent, rel, p_norm, norm_flag = _tables(model_or_tables)
        rel = rel.to(ent.device)
        lo, hi, f_ent = _mine_filter(filter_index, ent.shape[0], rel.shape[0], ent.device)
        if ent.shape[0] == 0:
            en, rn = ent.contiguous(), rel.contiguous()
        else:
            en = ops.transe_queries(ent.contiguous(), norm_flag=norm_flag)             # the normalised tables, once
            rn = ops.transe_queries(rel.contiguous(), norm_flag=norm_flag)
        if type_constraint is not None:
            set_ptr, set_ids = _mine_members(type_constraint, ent.shape[0], rel.shape[0], ent.device)
            return ops.transe_mine_typed(en, rn, p_norm, set_ptr, set_ids, k=k, threshold=threshold, filt_lo=lo, filt_hi=hi,
                                         filt_ent=f_ent, exclude_self=exclude_self, max_results=max_results)
        return ops.transe_mine(en, rn, p_norm, k=k, threshold=threshold, filt_lo=lo, filt_hi=hi, filt_ent=f_ent,
                               exclude_self=exclude_self, max_results=max_results)


def mine_triplets_unfused(model_or_tables, *, k=None, threshold=None, filter_index=None, exclude_self=True,
                          max_results=ops.MINE_MAX_RESULTS, type_constraint=None):
    """``mine_triplets`` from materialised distances, one relation at a time (``ops.transe_queries`` + ``ops.transe_distances`` +
    torch selection, a running K-th distance pruning the pool): the in-repo cross-check and the bench's comparator, never a
    fallback.  With a ``type_constraint`` the queries are the relation's subject members and the table its object members."""
    _mine_args(k, threshold, max_results)
    with torch.no_grad():
        ent, rel, p_norm, norm_flag = _tables(model_or_tables)
        ent, rel = ent.contiguous(), rel.to(ent.device).contiguous()
        n, num_rels = ent.shape[0], rel.shape[0]
        filt = _mine_filter(filter_index, n, num_rels, ent.device)
        members = None if type_constraint is None else _mine_members(type_constraint, n, num_rels, ent.device)
        subjects = torch.arange(n, device=ent.device)
        en = ops.transe_queries(ent, norm_flag=norm_flag) if n else ent

        def distances_of(r, subj=None, obj=None):
            a = subjects if subj is None else subj
            q = ops.transe_queries(ent, rel, a, torch.full_like(a, r), head=False, norm_flag=norm_flag)
            return ops.transe_distances(q, en if obj is None else en.index_select(0, obj), p_norm)

        return _mine_unfused(distances_of, True, n, num_rels, ent.device, k=k, threshold=threshold, filt=filt,
                            exclude_self=exclude_self, max_results=max_results, members=members)


def write_completions(path, model_or_tables, filter_index, k=None, threshold=None, type_constraint=None):
    """The whole graph's nearest new triplets (``mine_triplets``: the ``k`` nearest, cut at distance ``threshold`` when both are
    given; the known triplets and s == o left out; with a ``type_constraint`` type-correct triplets only) as TSV in train.py's
    completion layout: ``subject  relation  object  rank  distance``.  Returns the number of lines written."""
    if k is not None:
        trip, dist, _ = mine_triplets(model_or_tables, k=k, filter_index=filter_index, type_constraint=type_constraint)
        if threshold is not None:
            keep = dist <= float(threshold)
            trip, dist = trip[keep], dist[keep]
    else:
        trip, dist, _ = mine_triplets(model_or_tables, threshold=threshold, filter_index=filter_index, type_constraint=type_constraint)
    with open(path, 'w') as f:
        f.writelines(f"{s}\t{r}\t{o}\t{i}\t{x:.9g}\n" for i, ((s, r, o), x) in enumerate(zip(trip.tolist(), dist.tolist())))
    return int(dist.numel())


# ------------------------------------------------------------------------------------------------
# per-entity completion: what is this entity missing?
# ------------------------------------------------------------------------------------------------
COMPLETE_UNFUSED_ELEMS = 1 << 26      # distances per chunk of the materialised cross-check: bounds its (rows, R, N) tensor


def complete_entities_from_distances(dist, entities, k, *, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                                     cand_query=None, cand_other=None):
    """The rule of ``ops.transe_entity_topk`` on a materialised (m, R, N) distance tensor, in plain torch (any device): row i
    belongs to entity ``entities[i]``, its candidates are all (r, x) less the ids ``filt_ent[filt_lo[a * R + r]:filt_hi[a * R +
    r]]`` under relation r (the dense per-key ranges of ``_mine_filter``) and less ``x == a`` with ``exclude_self``; they go by
    distance ascending, equal distances by relation, then by entity, NaN after every number (+inf included).  Returns ``(rel int64
    (m, k), other int64 (m, k), dist float32 (m, k))``, padded with -1 / -1 / +inf; a zero is reported as +0 and every NaN as the
    one quiet NaN.  ``topk_from_distances`` on the (m, R * N) view under the allowed mask of
    ``ranking.complete_entities_from_scores``: the id r * N + x already says relation first, then entity.  ``cand_query`` /
    ``cand_other`` (bool (R, N), ``ranking.complete_masks``): the typed rule of ``ops.transe_entity_topk_typed``, as there."""
    rel, other, neg = complete_entities_from_scores(-dist.to(torch.float32), entities, k, filt_lo=filt_lo, filt_hi=filt_hi,
                                                    filt_ent=filt_ent, exclude_self=exclude_self, cand_query=cand_query,
                                                    cand_other=cand_other)
    out = 0.0 - neg                                                   # -(+0) would be -0; 0 - (+0) is +0
    return rel, other, torch.where(torch.isnan(out), torch.full_like(out, float('nan')), out)


def _complete_args(model_or_tables, entities, k, side, filter_index):
    """What the two routes of ``complete_entities`` check and prepare alike: (ent, rel, p_norm, norm_flag, entities, k, (lo, hi,
    ent))."""
    _complete_side(side)
    k = ops._topk_arg(k)
    ent, rel, p_norm, norm_flag = _tables(model_or_tables)
    rel = rel.to(ent.device)
    ents, filt = _complete_queries(ent, rel, entities, side, filter_index)
    return ent.contiguous(), rel.contiguous(), ops._p_norm(p_norm), norm_flag, ents, k, filt


def complete_entities(model_or_tables, entities, k, *, side='s', filter_index=None, exclude_self=True, type_constraint=UNCONSTRAINED):
    """What is this entity missing?  For every entity ``a`` of ``entities`` (any order, repeats allowed) the ``k`` nearest new
    facts around it over ALL relations at once: ``side='s'`` the facts (a, r, x) at ``||n(a) + n(r) - n(x)||_p``, ``side='o'`` the
    facts (x, r, a) at ``||n(a) - n(r) - n(x)||_p`` -- the distances of ``predict_topk`` on the queries (a, r) in direction 'o' /
    's', bit for bit.  ``model_or_tables`` is a ``TransE`` or ``(ent, rel, p_norm, norm_flag)``.  With a ``FilterIndex`` the known
    facts are left out -- direction 'o' for ``side='s'``, 's' for ``side='o'`` -- and with ``exclude_self`` the loops (a, r, a).
    The normalised tables are built once and one fused launch pair (ops.transe_entity_topk) keeps one list per entity while the
    relations are walked.  Returns ``(rel int64 (m, k), other int64 (m, k), dist float32 (m, k))`` in the order of
    ``complete_entities_from_distances``: nearest first, ties by relation, then by entity; rows with fewer than k candidates end
    in -1 / -1 / +inf.  1 <= k <= 128.  With a ``type_constraint`` (TypeConstraint) only type-correct facts are candidates -- the
    entity seen on its side of r and the other entity seen on the other side, ``mine_triplets(type_constraint=)``'s rule -- at the
    same distances, from the sweep over the relations' member lists (ops.transe_entity_topk_typed); the filter and the constraint
    are independent.  An entity on its side of no relation gets an all-padding row.  The unconstrained call leaves the argument
    out; an explicit None is a TypeError, as in ``ranking.complete_entities``."""
    type_constraint = _complete_constraint(type_constraint)
    with torch.no_grad():
        ent, rel, p_norm, norm_flag, ents, k, (lo, hi, f_ent) = _complete_args(model_or_tables, entities, k, side, filter_index)
        members = None if type_constraint is None else _mine_members(type_constraint, ent.shape[0], rel.shape[0], ent.device)
        en = ops.transe_queries(ent, norm_flag=norm_flag)                 # the normalised tables, once
        rn = ops.transe_queries(rel, norm_flag=norm_flag)
        if members is not None:
            return ops.transe_entity_topk_typed(ents, en, rn, k, p_norm, members[0], members[1], side == 'o', lo, hi, f_ent, exclude_self)
        return ops.transe_entity_topk(ents, en, rn, k, p_norm, side == 'o', lo, hi, f_ent, exclude_self)


def complete_entities_unfused(model_or_tables, entities, k, *, side='s', filter_index=None, exclude_self=True,
                              type_constraint=UNCONSTRAINED):
    """``complete_entities`` from materialised distances: per relation ``ops.transe_queries`` + ``ops.transe_distances`` into a
    (rows, R, N) tensor, then ``complete_entities_from_distances``, ``COMPLETE_UNFUSED_ELEMS`` distances at a time.  The in-repo
    cross-check and the bench's comparator, never a fallback.  With a ``type_constraint`` the same distances under the masks of
    ``ranking.complete_masks``."""
    type_constraint = _complete_constraint(type_constraint)
    with torch.no_grad():
        ent, rel, p_norm, norm_flag, ents, k, (lo, hi, f_ent) = _complete_args(model_or_tables, entities, k, side, filter_index)
        n, num_rels = ent.shape[0], rel.shape[0]
        masks = _complete_mask_args(type_constraint, side, n, num_rels, ent.device)
        en = ops.transe_queries(ent, norm_flag=norm_flag)

        def chunk(part):
            dist = torch.stack([ops.transe_distances(ops.transe_queries(ent, rel, part, torch.full_like(part, r), head=side == 'o',
                                                                        norm_flag=norm_flag), en, p_norm)
                                for r in range(num_rels)], dim=1)
            return complete_entities_from_distances(dist, part, k, filt_lo=lo, filt_hi=hi, filt_ent=f_ent, exclude_self=exclude_self,
                                                    **masks)

        return _complete_unfused(chunk, ents, max(1, COMPLETE_UNFUSED_ELEMS // (n * num_rels)), k)


def write_entity_profiles(path, model_or_tables, entities, k, filter_index, type_constraint=None):
    """Per-entity completion as TSV, ``entity  side  relation  other_entity  rank  distance``: for every entity of ``entities`` its
    ``k`` nearest new facts over all relations (``complete_entities``; ``filter_index``: the known ones left out, as are loops),
    nearest first with the rank counted from 1 -- the 's' lines are the facts (entity, relation, other), then the 'o' lines the
    facts (other, relation, entity).  The first five columns are those of train.py's ``profiles.tsv``: the two files join on them.
    An entity with fewer than k candidates has fewer lines.  With a ``type_constraint`` (ranking.TypeConstraint) only type-correct
    facts are written, in the same columns.  Returns the number of lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    return write_profile_lines(path, torch.as_tensor(entities, dtype=torch.long).reshape(-1),
                               lambda part, side: complete_entities(model_or_tables, part, k, side=side, filter_index=filter_index,
                                                                    **constrained))


# ------------------------------------------------------------------------------------------------
# per-relation completion: which pairs belong to this relation?
# ------------------------------------------------------------------------------------------------
def complete_relations_from_distances(dist, k, *, relations=None, filt_lo=None, filt_hi=None, filt_ent=None, exclude_self=True,
                                      cand_subj=None, cand_obj=None, max_results=ops.MINE_MAX_RESULTS):
    """The rule of ``ops.transe_relation_topk`` on a materialised tensor ``dist[r, s, o]`` (R, N, N), in plain torch (any device,
    CPU included): the counterpart of ``ranking.complete_relations_from_scores``.  For each relation r of ``relations`` (unique
    ids in [0, R), any order; None: all) the ``k`` candidates (s, o) of smallest distance.  Candidates: every (s, o), less
    ``filt_ent[filt_lo[s * R + r]:filt_hi[s * R + r]]`` as objects of (s, r), less s == o when ``exclude_self``, less NaN
    distances (+inf is a candidate, after every finite one), and with ``cand_subj`` / ``cand_obj`` (bool (R, N), together) only s
    among ``cand_subj[r]`` and o among ``cand_obj[r]``.  Order inside a relation: ``mine_from_distances``' restricted to it --
    distance ascending, then (s, o) ascending.  Returns ``(subj int64 (m, k), obj int64 (m, k), dist float32 (m, k), info)``, row i
    for ``relations[i]``, rows with fewer than k candidates ending in -1 / -1 / +inf, a zero reported as +0; ``info['count']`` int64
    [m] is each relation's candidates at or below its K-th distance's exact value (all, when fewer than K exist).  ``m * k <=
    max_results``; a relation whose count exceeds its share ``max_results // m`` raises ``MineOverflow`` naming it."""
    num_rels, n = dist.shape[0], dist.shape[1]
    rels = ops.relation_ids_check(relations, num_rels).to(dist.device)
    k, max_results, share = ops._relation_args(k, rels.numel(), max_results)
    ops._mine_sizes(n, num_rels, filt_lo, filt_hi, filt_ent)
    subj_ok, obj_ok = _relation_masks(cand_subj, cand_obj, num_rels, n, dist.device)
    filt = (filt_lo, filt_hi, filt_ent)

    def pairs_of(i, r):
        typed = {} if subj_ok is None else dict(subj_ok=subj_ok[r], obj_ok=obj_ok[r])
        return _relation_pairs(dist[r], r, num_rels, k, filt, exclude_self, ascending=True, **typed)

    return _relation_rows(pairs_of, rels, k, n, share, ascending=True)


def _relation_setup(model_or_tables, k, relations, max_results, filter_index, type_constraint):
    """What the two routes of ``complete_relations`` check and prepare alike, before anything is asked of the device: (ent, rel,
    p_norm, norm_flag, the relations int64 [m], k, a relation's share of ``max_results``, (lo, hi, ent), the constraint's member
    lists or None, the constraint or None)."""
    type_constraint = _complete_constraint(type_constraint)
    ent, rel, p_norm, norm_flag = _tables(model_or_tables)
    ent, rel = ent.contiguous(), rel.to(ent.device).contiguous()
    rels = ops.relation_ids_check(relations, rel.shape[0]).to(ent.device)
    k, _, share = ops._relation_args(k, rels.numel(), max_results)
    filt = _mine_filter(filter_index, ent.shape[0], rel.shape[0], ent.device)
    members = None if type_constraint is None else _mine_members(type_constraint, ent.shape[0], rel.shape[0], ent.device)
    return ent, rel, ops._p_norm(p_norm), norm_flag, rels, k, share, filt, members, type_constraint


def complete_relations(model_or_tables, k, *, relations=None, filter_index=None, exclude_self=True, type_constraint=UNCONSTRAINED,
                       max_results=ops.MINE_MAX_RESULTS):
    """Which pairs belong to this relation?  For every relation r of ``relations`` (unique ids, any order; default: every relation)
    its OWN ``k`` nearest new facts (s, r, o), at the distance ``||n(E_s) + n(R_r) - n(E_o)||_p`` of ``predict_topk(direction='o')``
    bit for bit; with a ``FilterIndex`` the known triplets are left out.  ``mine_triplets`` cannot answer this: its one distance
    for the whole graph is filled by the relations with short translation vectors.  Here every relation has its own threshold,
    found for all of them in the same few fused sweeps (ops.transe_relation_topk), and a handful of relations cost their share of
    a sweep.  ``model_or_tables`` is a ``TransE`` or ``(ent, rel, p_norm, norm_flag)``; the normalised tables are built once.
    Returns ``(subj int64 (m, k), obj int64 (m, k), dist float32 (m, k), info)`` in the order of
    ``complete_relations_from_distances``: row i for ``relations[i]``, nearest first, ties by (s, o), short rows padded with -1 /
    -1 / +inf; ``info['count']`` int64 [m], ``info['passes']``.  ``k >= 1`` and ``m * k <= max_results``; ``MineOverflow`` (naming
    the relation) rather than a truncated list.  With a ``type_constraint`` (TypeConstraint) only type-correct pairs are
    candidates -- ``mine_triplets(type_constraint=)``'s rule on the same member lists, at the same distances
    (ops.transe_relation_topk_typed).  The unconstrained call leaves the argument out; an explicit None is a TypeError.  There is no
    Monte-Carlo form: TransE has no posterior."""
    with torch.no_grad():
        ent, rel, p_norm, norm_flag, rels, k, _, (lo, hi, f_ent), members, _ = \
            _relation_setup(model_or_tables, k, relations, max_results, filter_index, type_constraint)
        if ent.shape[0] == 0:
            en, rn = ent, rel
        else:
            en = ops.transe_queries(ent, norm_flag=norm_flag)             # the normalised tables, once
            rn = ops.transe_queries(rel, norm_flag=norm_flag)
        rule = dict(relations=rels, filt_lo=lo, filt_hi=hi, filt_ent=f_ent, exclude_self=exclude_self, max_results=max_results)
        if members is not None:
            return ops.transe_relation_topk_typed(en, rn, k, p_norm, members[0], members[1], **rule)
        return ops.transe_relation_topk(en, rn, k, p_norm, **rule)


def complete_relations_unfused(model_or_tables, k, *, relations=None, filter_index=None, exclude_self=True,
                               type_constraint=UNCONSTRAINED, max_results=ops.MINE_MAX_RESULTS):
    """``complete_relations`` from materialised distances, one relation at a time: ``ops.transe_queries`` +
    ``ops.transe_distances`` into an (N, N) tensor, then the rule of ``complete_relations_from_distances``.  The in-repo
    cross-check and the bench's comparator, never a fallback."""
    with torch.no_grad():
        ent, rel, p_norm, norm_flag, rels, k, share, filt, _, type_constraint = \
            _relation_setup(model_or_tables, k, relations, max_results, filter_index, type_constraint)
        n, num_rels = ent.shape[0], rel.shape[0]
        masks = None
        if type_constraint is not None:
            masks = (type_constraint.mask(torch.arange(num_rels, 2 * num_rels), ent.device),
                     type_constraint.mask(torch.arange(num_rels), ent.device))
        subjects = torch.arange(n, device=ent.device)
        en = ops.transe_queries(ent, norm_flag=norm_flag) if n else ent

        def pairs_of(i, r):
            q = ops.transe_queries(ent, rel, subjects, torch.full_like(subjects, r), head=False, norm_flag=norm_flag)
            val = ops.transe_distances(q, en, p_norm)
            typed = {} if masks is None else dict(subj_ok=masks[0][r], obj_ok=masks[1][r])
            return _relation_pairs(val, r, num_rels, k, filt, exclude_self, ascending=True, **typed)

        return _relation_rows(pairs_of, rels, k, n, share, ascending=True)


def write_relation_profiles(path, model_or_tables, relations, k, filter_index, type_constraint=None):
    """Per-relation completion as TSV, ``s  r  o  rank  distance`` (the columns of ``write_completions``, and of train.py's
    ``relation_profiles.tsv`` with the distance in place of the logit: the files join on s, r, o): for every relation of
    ``relations``, in the order given, its OWN ``k`` nearest new facts (``complete_relations``; ``filter_index``: the known ones
    left out, as are loops), nearest first with the rank counted from 1 within the relation.  A relation with fewer than k
    candidates has fewer lines: the padding is left out.  With a ``type_constraint`` (ranking.TypeConstraint) only type-correct
    facts are written.  Returns the number of lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    subj, obj, dist, _ = complete_relations(model_or_tables, k, relations=torch.as_tensor(relations, dtype=torch.long),
                                            filter_index=filter_index, **constrained)
    n_lines = 0
    with open(path, 'w') as f:
        for r, ss, os_, xs in zip(relations, subj.tolist(), obj.tolist(), dist.tolist()):
            lines = [f"{a}\t{r}\t{b}\t{i}\t{x:.9g}\n" for i, (a, b, x) in enumerate(zip(ss, os_, xs), 1) if a >= 0]
            f.writelines(lines)
            n_lines += len(lines)
    return n_lines


# ------------------------------------------------------------------------------------------------
# CLI (baselines/transe/main.py's hyperparameters as defaults)
# ------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(description='TransE baseline (OpenKE formulation) on the device')
    p.add_argument('-d', '--dataset', type=str, required=True, help='dataset (data.load_data)')
    p.add_argument('--gpu', type=int, default=0, help='device')
    p.add_argument('--dim', type=int, default=200)
    p.add_argument('--p-norm', type=int, default=1)
    p.add_argument('--norm-flag', type=int, default=1)
    p.add_argument('--margin', type=float, default=5.0)
    p.add_argument('--nbatches', type=int, default=100)
    p.add_argument('--neg-ent', type=int, default=25)
    p.add_argument('--neg-rel', type=int, default=0)
    p.add_argument('--bern-flag', type=int, default=1)
    p.add_argument('--filter-flag', type=int, default=1)
    p.add_argument('--train-times', type=int, default=1000)
    p.add_argument('--alpha', type=float, default=1.0, help='learning rate (of every --optimizer)')
    p.add_argument('--opt-method', type=str, default='sgd', help='kept at sgd: choose the optimiser with --optimizer')
    p.add_argument('--optimizer', type=str, default='sgd',
                   help='sgd, adagrad, adadelta or adam (case-insensitive): the torch.optim rule at torch\'s defaults, on the device')
    p.add_argument('--weight-decay', type=float, default=0.0, help='coupled L2 decay, g += weight_decay * p (every row, every step)')
    p.add_argument('--lr-decay', type=float, default=0.0, help='Adagrad\'s learning-rate decay (with --optimizer adagrad only)')
    p.add_argument('--adv-temperature', type=float, default=None)
    p.add_argument('--regul-rate', type=float, default=0.0)
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--checkpoint', type=str, default='transe.ckpt')
    p.add_argument('--test-mode', action='store_true', help='load --checkpoint and evaluate only')
    p.add_argument('--eval-every', type=int, default=0, help='evaluate on valid every N epochs (0: never)')
    p.add_argument('--filtered-eval', action='store_true', help='report filtered ranks as well (filter: train + valid + test)')
    p.add_argument('--type-constrain', action='store_true',
                   help='type-constrained protocol (candidates: the entities seen on that side of the relation in train + valid + '
                        'test): with --filtered-eval the evaluation reports raw, filtered, raw_constrained and '
                        'filtered_constrained; with --predict-topk only such entities are written.  It does not touch '
                        '--complete-topk / --complete-threshold, which keep writing unconstrained completions: see --complete-typed')
    p.add_argument('--graph-step', action='store_true', help='capture one step as a hipGraph and replay it')
    p.add_argument('--predict-topk', type=int, default=None,
                   help='after the final evaluation write the K (1..128) nearest new entities of both directions of every test '
                        'triplet (train + valid + test triplets filtered out) to --predict-out')
    p.add_argument('--predict-out', type=str, default='transe_predictions.tsv',
                   help='TSV written by --predict-topk: direction, query entity, relation, position, entity, distance')
    p.add_argument('--complete-topk', type=int, default=None,
                   help='after the final evaluation write the K nearest new triplets among ALL entities x relations x entities '
                        '(train + valid + test triplets and s == o left out) to --complete-out')
    p.add_argument('--complete-threshold', type=float, default=None,
                   help='as --complete-topk, every new triplet within distance D; with both, the K nearest cut at D')
    p.add_argument('--complete-out', type=str, default='transe_completions.tsv',
                   help='TSV written by --complete-topk / --complete-threshold: subject, relation, object, rank, distance')
    p.add_argument('--complete-typed', action='store_true',
                   help='with --complete-topk / --complete-threshold: mine among type-correct triplets only (the subject seen as '
                        'subject, the object seen as object of the relation in train + valid + test); needs no --filtered-eval')
    p.add_argument('--relation-eval', action='store_true',
                   help='after the final evaluation also report relation prediction over the test triplets: MRR / MR / Hits@k of the '
                        'true relation of (s, ?, o) among all relations; with --filtered-eval also with the pair\'s other known '
                        'relations (train + valid + test) left out')
    p.add_argument('--predict-relations', type=int, default=0,
                   help='after the final evaluation write the K (1..128) nearest NEW relations between subject and object of every '
                        'test triplet (the pair\'s train + valid + test relations left out) to --relations-out; 0 = off')
    p.add_argument('--relations-typed', action='store_true',
                   help='with --relation-eval / --predict-relations: also report the ranks among the TYPE-CORRECT relations of each pair '
                        '(the subject seen as subject of the relation, the object as its object, in train + valid + test) and propose '
                        'only those')
    p.add_argument('--relations-out', type=str, default='transe_relation_predictions.tsv',
                   help='TSV written by --predict-relations: subject, object, position, predicted relation, distance; the first four '
                        'columns are those of train.py\'s --relations-out')
    p.add_argument('--profile-topk', type=int, default=0,
                   help='after the final evaluation write, for every entity of --profile-entities, its K nearest NEW facts over all '
                        'relations, as subject and as object (train + valid + test triplets and loops left out), to --profile-out; '
                        '1..128, 0 = off')
    p.add_argument('--profile-entities', type=str, default=None,
                   help='the entities of --profile-topk: comma-separated ids, or a file with one id per line; default: every entity')
    p.add_argument('--profile-out', type=str, default='transe_profiles.tsv',
                   help='TSV written by --profile-topk: entity, side (s: the entity is the subject, o: the object), relation, other '
                        'entity, rank (from 1), distance; the first five columns are those of train.py\'s --profile-out')
    p.add_argument('--profile-typed', action='store_true',
                   help='with --profile-topk: write type-correct facts only (the entity seen on its side of the relation, the other '
                        'entity seen on the other side, in train + valid + test); the same columns; --type-constrain does not '
                        'constrain profiles')
    p.add_argument('--relation-profile-topk', type=int, default=None,
                   help='after the final evaluation write, for every relation of --relation-profile-ids, ITS OWN K nearest NEW facts '
                        '(train + valid + test triplets and loops left out) to --relation-profile-out -- every relation has its own '
                        'distance threshold, where --complete-topk has one for the whole graph')
    p.add_argument('--relation-profile-ids', type=str, default=None,
                   help='the relations of --relation-profile-topk: comma-separated ids, or a file with one id per line, each at most '
                        'once; default: every relation')
    p.add_argument('--relation-profile-out', type=str, default=None,
                   help='TSV written by --relation-profile-topk (default transe_relation_profiles.tsv): s, r, o, rank from 1 within '
                        'the relation, distance; relations in the order asked; joins with --complete-out and with train.py\'s '
                        '--relation-profile-out on s, r, o')
    p.add_argument('--relation-profile-typed', action='store_true',
                   help='with --relation-profile-topk: write type-correct facts only (s seen as subject of r, o seen as its object, '
                        'in train + valid + test); the same columns; --type-constrain and --complete-typed keep their meaning')
    return p


RELATION_PROFILE_OUT = 'transe_relation_profiles.tsv'      # --relation-profile-out when it is not given


def check_args(args):
    if args.opt_method.lower() != 'sgd':
        raise ValueError(f'--opt-method {args.opt_method}: only sgd is supported here; choose the optimiser with --optimizer '
                         f'{{{",".join(OPT_METHODS)}}}')
    opt = str(getattr(args, 'optimizer', 'sgd')).lower()
    if opt not in OPT_METHODS:
        raise ValueError(f'--optimizer {args.optimizer}: expected one of {", ".join(OPT_METHODS)}')
    wd, ld = getattr(args, 'weight_decay', 0.0), getattr(args, 'lr_decay', 0.0)
    if not wd >= 0:
        raise ValueError(f'--weight-decay must be >= 0, got {wd}')
    if not ld >= 0:
        raise ValueError(f'--lr-decay must be >= 0, got {ld}')
    if ld != 0 and opt != 'adagrad':
        raise ValueError('--lr-decay is Adagrad\'s learning-rate decay: it needs --optimizer adagrad')
    if (opt != 'sgd' or wd != 0) and not args.alpha >= 0:
        raise ValueError(f'--alpha must be >= 0 with --optimizer {opt} / --weight-decay, got {args.alpha}')
    if args.neg_rel != 0:
        raise ValueError('--neg-rel: relation corruption is not supported')       # (relation QUERIES exist: --relation-eval)
    if args.p_norm not in (1, 2):
        raise ValueError('--p-norm must be 1 or 2')
    if args.adv_temperature is not None and not args.adv_temperature > 0:
        raise ValueError('--adv-temperature must be > 0')
    if not 1 <= args.dim <= ops.TRANSE_MAX_DIM:
        raise ValueError(f'--dim must lie in [1, {ops.TRANSE_MAX_DIM}]')
    k = getattr(args, 'predict_topk', None)
    if k is not None and not 1 <= k <= ops.TOPK_MAX:
        raise ValueError(f'--predict-topk must lie in [1, {ops.TOPK_MAX}], got {k}')
    ck = getattr(args, 'complete_topk', None)
    if ck is not None and ck < 1:
        raise ValueError(f'--complete-topk must be >= 1, got {ck}')
    cd = getattr(args, 'complete_threshold', None)
    if cd is not None and cd != cd:
        raise ValueError('--complete-threshold is NaN')
    if getattr(args, 'complete_typed', False) and ck is None and cd is None:
        raise ValueError('--complete-typed restricts the completions: it needs --complete-topk or --complete-threshold')
    if getattr(args, 'type_constrain', False) and not getattr(args, 'filtered_eval', False):
        raise ValueError('--type-constrain needs --filtered-eval: the report is raw, filtered, raw_constrained, filtered_constrained')
    if not 0 <= getattr(args, 'profile_topk', 0) <= ops.TOPK_MAX:
        raise ValueError(f'--profile-topk keeps one list of at most {ops.TOPK_MAX} facts per entity (0 = off), got {args.profile_topk}')
    if getattr(args, 'profile_typed', False) and not getattr(args, 'profile_topk', 0) > 0:
        raise ValueError('--profile-typed restricts the profiles: it needs --profile-topk')
    if not 0 <= getattr(args, 'predict_relations', 0) <= ops.TOPK_MAX:
        raise ValueError(f'--predict-relations must lie in [1, {ops.TOPK_MAX}] (0 = off), got {args.predict_relations}')
    if getattr(args, 'relations_typed', False) and not (getattr(args, 'relation_eval', False) or getattr(args, 'predict_relations', 0) > 0):
        raise ValueError('--relations-typed restricts the relation queries: it needs --relation-eval or --predict-relations')
    rk = getattr(args, 'relation_profile_topk', None)
    if rk is not None and rk < 1:
        raise ValueError(f'--relation-profile-topk counts the facts kept per relation: it must be >= 1, got {rk}')
    if getattr(args, 'relation_profile_typed', False) and rk is None:
        raise ValueError('--relation-profile-typed restricts the per-relation lists: it needs --relation-profile-topk')
    if getattr(args, 'relation_profile_out', None) is not None and rk is None:
        raise ValueError('--relation-profile-out names the file of the per-relation lists: it needs --relation-profile-topk')
    if getattr(args, 'relation_profile_ids', None) is not None:
        if rk is None:
            raise ValueError('--relation-profile-ids chooses the relations of the per-relation lists: it needs --relation-profile-topk')
        relation_profile_ids_arg(args.relation_profile_ids)


def main(args):
    check_args(args)
    from .data import load_data
    if not torch.cuda.is_available():
        raise RuntimeError('TransE training runs on a ROCm device (no CPU fallback)')
    torch.cuda.set_device(args.gpu)
    dev = torch.device('cuda', args.gpu)
    if args.seed is not None:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
    data = load_data(args.dataset)
    who = None
    if getattr(args, 'profile_topk', 0) > 0:         # a bad id is refused before any training
        who = profile_entities_arg(getattr(args, 'profile_entities', None), data.num_nodes)
    which = None
    if getattr(args, 'relation_profile_topk', None) is not None:
        which = relation_profile_ids_arg(getattr(args, 'relation_profile_ids', None), data.num_rels)
    model = TransE(data.num_nodes, data.num_rels, dim=args.dim, p_norm=args.p_norm, norm_flag=bool(args.norm_flag))
    filt = None
    if args.filtered_eval:
        filt = FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
    types = None
    if args.type_constrain:
        types = TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
    if not args.test_mode:
        model = model.to(dev)
        tr = DeviceTrainer(model, data.train, args.nbatches, args.neg_ent, bool(args.bern_flag), bool(args.filter_flag),
                           args.margin, args.alpha, args.adv_temperature, args.regul_rate, dev,
                           opt_method=getattr(args, 'optimizer', 'sgd'), weight_decay=getattr(args, 'weight_decay', 0.0),
                           lr_decay=getattr(args, 'lr_decay', 0.0))
        if args.graph_step:
            tr.capture()
        print('Finish initializing...')
        t0 = time.time()
        for epoch in range(args.train_times):
            res = tr.epoch()
            print('Epoch %d | loss: %f' % (epoch, res))
            if args.eval_every and (epoch + 1) % args.eval_every == 0 and len(data.valid):
                evaluate(model, data.valid, filt)
        torch.cuda.synchronize()
        print('trained {} epochs in {:.2f} s'.format(args.train_times, time.time() - t0))
        model.save_checkpoint(args.checkpoint)
    model.load_checkpoint(args.checkpoint)
    model = model.to(dev)
    out = evaluate(model, data.test, filt, type_constraint=types)
    if args.predict_topk is not None:
        known = filt if filt is not None else FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        n_lines = write_predictions(args.predict_out, model, data.test, args.predict_topk, known, types)
        print(f'wrote {n_lines} predictions (top {args.predict_topk}, both directions, known triplets filtered) to {args.predict_out}')
    if args.complete_topk is not None or args.complete_threshold is not None:
        known = filt if filt is not None else FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        typed = None
        if getattr(args, 'complete_typed', False):
            typed = types if types is not None else \
                TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        n_lines = write_completions(args.complete_out, model, known, args.complete_topk, args.complete_threshold, typed)
        print(f'wrote {n_lines} completions (nearest new {"type-correct " if typed is not None else ""}triplets of the whole graph, '
              f'known triplets filtered) to {args.complete_out}')
    if getattr(args, 'relation_eval', False) or getattr(args, 'predict_relations', 0) > 0:
        pairs = PairFilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        typed = None
        if getattr(args, 'relations_typed', False):
            typed = types if types is not None else \
                TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        if getattr(args, 'relation_eval', False):
            out['relations'] = evaluate_relations(model, data.test, pairs if args.filtered_eval else None, type_constraint=typed)
        if getattr(args, 'predict_relations', 0) > 0:
            n_lines = write_relation_predictions(args.relations_out, model, data.test, args.predict_relations, pairs, typed)
            print(f'wrote {n_lines} relation predictions (nearest {args.predict_relations} {"type-correct " if typed is not None else ""}'
                  f'per test pair, known relations filtered) to {args.relations_out}')
    if who is not None:
        known = filt if filt is not None else FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        typed = None
        if getattr(args, 'profile_typed', False):
            typed = types if types is not None else \
                TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        n_lines = write_entity_profiles(args.profile_out, model, who, args.profile_topk, known, typed)
        print(f'wrote {n_lines} new {"type-correct " if typed is not None else ""}facts around {len(who)} entities (nearest '
              f'{args.profile_topk} over all relations, as subject and as object, known triplets filtered) to {args.profile_out}')
    if which is not None:
        known = filt if filt is not None else FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        typed = None
        if getattr(args, 'relation_profile_typed', False):
            typed = types if types is not None else \
                TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device=dev)
        path = args.relation_profile_out if getattr(args, 'relation_profile_out', None) is not None else RELATION_PROFILE_OUT
        n_lines = write_relation_profiles(path, model, which, args.relation_profile_topk, known, typed)
        print(f'wrote {n_lines} new {"type-correct " if typed is not None else ""}facts of {len(which)} relations (each relation\'s own '
              f'nearest {args.relation_profile_topk}, known triplets filtered) to {path}')
    return out


if __name__ == '__main__':
    main(build_parser().parse_args())
