"""Link-prediction task head and driver with the reference's names, flags and control flow
(kgvae/link_predict.py:30-326), running on the gfx950 kernels.

    python -m gcn_vae_amd.train -d FB15k-237-synthetic --n-hidden 200 --n-bases 100 --n-flows 3 \
        --mmd-param 1 --mog-k 10 --gpu 0

Differences from the reference, all forced by its own crashes or by the device:
  * defaults that crash there (``--n-flows 0`` with ``--kl-param > 0``; ``--model-class RGCN``;
    the periodic validation with ``flow_log_prob=None``) run here;
  * validation stays on the GPU (the reference flips the model to the CPU because its scorer
    materialises a (h, Eb, V) tensor; ours is one GEMM);
  * the wall-clock spans synchronise the device before reading the clock;
  * ``--gpu`` must name a ROCm device: there is no CPU path.
"""
import argparse
import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import ops, ranking, sampling
from .optim import FlatAdam
from .data import load_data
from .encoders import KGVAE, RGCN
from .sampling import node_norm_to_edge_norm


class LinkPredict(ops.StayOnDevice, nn.Module):
    def __init__(self, model_class, in_dim, h_dim, num_rels, num_bases=-1, num_hidden_layers=1, dropout=0,
                 use_cuda=True, reg_param=0, kl_param=0, mmd_param=0, k=1, n_flows=0):
        super().__init__()
        self.encoder = model_class(num_nodes=in_dim, h_dim=h_dim, out_dim=h_dim, num_rels=num_rels * 2,
                                   num_bases=num_bases, num_hidden_layers=num_hidden_layers, dropout=dropout,
                                   use_self_loop=use_cuda, use_cuda=use_cuda, k=k, n_flows=n_flows)
        self.reg_param, self.kl_param, self.mmd_param = reg_param, kl_param, mmd_param
        if kl_param > 0 and hasattr(self.encoder, 'fuse_kl_with_reparam'):
            self.encoder.fuse_kl_with_reparam = True             # get_loss will ask for KL(z): its forward pass rides on the reparameterisation
        if mmd_param > 0 and hasattr(self.encoder, 'batch_mmd_prior_with_forward'):
            self.encoder.batch_mmd_prior_with_forward = True     # get_loss will ask for MMD: batch its flow passes
        self.w_relation = nn.Parameter(torch.Tensor(num_rels, h_dim))
        self.use_cuda, self.k, self.n_flows = use_cuda, k, n_flows
        nn.init.xavier_uniform_(self.w_relation, gain=nn.init.calculate_gain('relu'))
        self._tidx_key, self._tidx = None, None

    def triplet_index(self, embedding, triplets):
        """Index of a triplet batch for the DistMult backward; cached per (storage, version)."""
        key = (triplets.data_ptr(), triplets._version, tuple(triplets.shape), embedding.shape[0])
        if key != self._tidx_key:
            # a batch that is scored once (mini-batch training) gets the sync-free index; one that is reused every step
            # (full-graph training: set ``static_batch``) gets the exact, locality-ordered one
            self._tidx = ops.TripletIndex(triplets.to(embedding.device), embedding.shape[0], self.w_relation.shape[0],
                                          sync_free=not getattr(self, 'static_batch', False))
            self._tidx_key = key
            self._tidx_keepalive = triplets
        return self._tidx

    def calc_score(self, embedding, triplets):
        return ops.distmult_score(embedding, self.w_relation, self.triplet_index(embedding, triplets))

    def forward(self, g, h, r, norm):
        return self.encoder.forward(g, h, r, norm)

    def regularization_loss(self, embedding):
        return ops.mean_sq(embedding) + ops.mean_sq(self.w_relation)

    def get_loss(self, g, embed, triplets, labels):
        """(loss, predict_loss, kl, mmd) -- the four terms of kgvae/link_predict.py:71-92 from one fused
        autograd node (ops.loss_head); calc_score / regularization_loss / get_kl / get_mmd stay available
        as separate differentiable ops with the reference's signatures."""
        enc = self.encoder
        tidx = self.triplet_index(embed, triplets)
        vae = isinstance(enc, KGVAE)
        flp = enc.get_flow_log_prob() if vae else None
        kl_w = self.kl_param if vae else 0.0
        mmd_w = self.mmd_param if vae else 0.0
        z_pri, pick = enc.mmd_inputs(embed) if mmd_w > 0 else (None, None)
        part = getattr(enc, 'row_part', None) if vae else None
        if part is not None:
            return self._get_loss_rows(part, embed, tidx, flp, kl_w, mmd_w, z_pri, pick, labels)
        loss, predict_loss, kl, mmd = ops.loss_head(
            embed, enc.z_mean if kl_w > 0 else None, enc.z_sigma if kl_w > 0 else None, self.w_relation,
            enc.z_pre.squeeze(0) if kl_w > 0 else None, flp, z_pri, pick, labels, tidx, self.reg_param, kl_w, mmd_w,
            score_bias=self.n_flows > 0, rows_dev=getattr(self, 'rows_dev', None))
        # shapes as the reference returns them: a disabled term is ``zeros(1)`` there and broadcasts the loss to (1,)
        kl = kl.reshape(()) if kl_w > 0 else kl.reshape(1)
        mmd = mmd.reshape(()) if mmd_w > 0 else mmd.reshape(1)
        if kl_w <= 0 or mmd_w <= 0:
            loss = loss.reshape(1)
        return loss, predict_loss, kl, mmd


def _get_loss_rows(self, part, embed, tidx, flp, kl_w, mmd_w, z_pri, pick, labels):
    """get_loss under the destination-row partition.  ``embed`` is z of ALL positions; the decoder, the regulariser
    and MMD run on it (on this rank's triplets / draws), KL on the rank's own rows.  Returns the rank's SHARE of

        L = mean_p(pred_p + mmd_w mmd_p) + reg_w reg + kl_w KL     (the sum of the shares over the ranks is L)

    so that plain SUMS of the ranks' gradients (reduce-scatter of dL/dz, all-reduce of the parameter arena) are exact."""
    enc = self.encoder
    head, predict_loss, _, mmd = ops.loss_head(embed, None, None, self.w_relation, None, flp, z_pri, pick, labels, tidx,
                                               self.reg_param, 0.0, mmd_w, score_bias=self.n_flows > 0,
                                               embed_rows=part.real_rows)
    kl = None
    if kl_w > 0 and part.own_rows > 0:
        kl = ops.kl_to_mixture(enc.z_own, enc.z_mean, enc.z_sigma, enc.z_pre.squeeze(0), flp)   # mean over own rows
    loss = ops.lincomb2(head, 1.0 / part.world, kl, kl_w * part.own_rows / max(part.real_rows, 1))
    kl_share = (kl.detach() * (part.own_rows / max(part.real_rows, 1))).reshape(()) if kl is not None \
        else torch.zeros(1, device=embed.device)
    return loss, predict_loss, kl_share, (mmd.reshape(()) if mmd_w > 0 else mmd.reshape(1))


LinkPredict._get_loss_rows = _get_loss_rows


def host_state_dict(model):
    """The model's state_dict with every tensor on the HOST: the reference moves the model to the CPU before it saves
    (kgvae/link_predict.py:242-246), so its checkpoints load with a plain ``torch.load`` on a box without a GPU.  HIP modules stay
    on the device under ``.cpu()`` (ops.StayOnDevice), hence the explicit copy here."""
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def _sync():
    torch.cuda.synchronize()


def write_predictions(path, embed, w, triplets, k, filter_index, flow_log_prob=None, type_constraint=None):
    """Top-k link predictions for both directions of every triplet, the known answers (``filter_index``) left out, as TSV:
    ``direction  query_entity  relation  position  predicted_entity  logit`` -- 'o' lines answer (s, r, ?), 's' lines (?, r, o);
    a query with fewer than k candidates ends in id -1, logit -inf.  With a ``type_constraint`` (ranking.TypeConstraint) only
    members of the relation's type set on that side are written.  Returns the number of lines written."""
    n = 0
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    with torch.no_grad(), open(path, 'w') as f:
        for d, a in (('o', triplets[:, 0]), ('s', triplets[:, 2])):
            r = triplets[:, 1]
            ids, logits = ranking.predict_topk(embed, w, a, r, k, direction=d, filter_index=filter_index,
                                               flow_log_prob=flow_log_prob, **constrained)
            a, r, ids, logits = a.tolist(), r.tolist(), ids.tolist(), logits.tolist()
            for i in range(len(a)):
                head = f"{d}\t{a[i]}\t{r[i]}\t"
                f.writelines(f"{head}{p}\t{e}\t{x:.9g}\n" for p, (e, x) in enumerate(zip(ids[i], logits[i])))
                n += len(ids[i])
    return n


def write_mc_predictions(path, z, w, triplets, k, filter_index, flow_log_probs=None, type_constraint=None):
    """``write_predictions`` under the posterior predictive of the samples ``z`` (S, N, h) (ranking.predict_topk_mc), as TSV:
    ``direction  query_entity  relation  position  predicted_entity  prob_mean  prob_std`` -- the mean and the population standard
    deviation over the samples of the pair's probability; a query with fewer than k candidates ends in id -1, mean -inf, std 0.
    With a ``type_constraint`` (ranking.TypeConstraint) only members of the relation's type set on that side are written.
    Returns the number of lines written."""
    n = 0
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    with torch.no_grad(), open(path, 'w') as f:
        for d, a in (('o', triplets[:, 0]), ('s', triplets[:, 2])):
            r = triplets[:, 1]
            ids, mean, std = ranking.predict_topk_mc(z, w, a, r, k, direction=d, filter_index=filter_index,
                                                     flow_log_probs=flow_log_probs, **constrained)
            a, r, ids, mean, std = a.tolist(), r.tolist(), ids.tolist(), mean.tolist(), std.tolist()
            for i in range(len(a)):
                head = f"{d}\t{a[i]}\t{r[i]}\t"
                f.writelines(f"{head}{p}\t{e}\t{x:.9g}\t{y:.9g}\n" for p, (e, x, y) in enumerate(zip(ids[i], mean[i], std[i])))
                n += len(ids[i])
    return n


PROFILE_ROWS = 4096      # entities per ranking.complete_entities call of write_entity_profiles (bounds the host-side lists)


def profile_entities_arg(spec, num_nodes):
    """The entities of ``--profile-entities``: None is every entity, else comma-separated ids or the path of a file with one id
    per line (blank lines skipped).  Ids are kept as given, in order, repeats included; one outside [0, num_nodes) is refused."""
    if spec is None:
        return list(range(num_nodes))
    if os.path.isfile(spec):
        with open(spec) as f:
            fields = [line.strip() for line in f if line.strip()]
    else:
        fields = [x.strip() for x in spec.split(',') if x.strip()]
    try:
        ids = [int(x) for x in fields]
    except ValueError:
        raise ValueError(f'--profile-entities takes comma-separated entity ids or a file with one id per line, got {spec!r}') from None
    bad = [i for i in ids if not 0 <= i < num_nodes]
    if bad:
        raise ValueError(f'--profile-entities: entity {bad[0]} lies outside [0, {num_nodes})')
    return ids


def relation_profile_ids_arg(spec, num_rels=None):
    """The relations of ``--relation-profile-ids``: None is every relation (a list only once ``num_rels`` is known), else
    comma-separated ids or the path of a file with one id per line (blank lines skipped), kept in the order given.  Refused: a field
    that is no integer, a negative id, a repeated id and, once ``num_rels`` is known, one outside [0, num_rels)."""
    if spec is None:
        return None if num_rels is None else list(range(num_rels))
    if os.path.isfile(spec):
        with open(spec) as f:
            fields = [line.strip() for line in f if line.strip()]
    else:
        fields = [x.strip() for x in spec.split(',') if x.strip()]
    try:
        ids = [int(x) for x in fields]
    except ValueError:
        raise ValueError(f'--relation-profile-ids takes comma-separated relation ids or a file with one id per line, got {spec!r}') from None
    if not ids:
        raise ValueError(f'--relation-profile-ids names no relation: {spec!r}')
    bad = [i for i in ids if i < 0 or (num_rels is not None and i >= num_rels)]
    if bad:
        raise ValueError(f"--relation-profile-ids: relation {bad[0]} lies outside [0, {'R' if num_rels is None else num_rels})")
    if len(set(ids)) != len(ids):
        raise ValueError(f'--relation-profile-ids: relation {[i for i in ids if ids.count(i) > 1][0]} is named twice')
    return ids


def write_relation_profiles(path, embed, w, relations, k, filter_index, flow_log_prob=None, type_constraint=None):
    """Per-relation completion as TSV, ``s  r  o  rank  logit`` (the columns of ``write_completions``: the two files join on s, r,
    o): for every relation of ``relations``, in the order given, its OWN ``k`` most confident new facts
    (ranking.complete_relations; ``filter_index``: the known ones left out, as are loops), best first with the rank counted from
    1 within the relation.  A relation with fewer than k candidates has fewer lines.  With a ``type_constraint``
    (ranking.TypeConstraint) only type-correct facts are written.  Returns the number of lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    with torch.no_grad():
        subj, obj, logits, _ = ranking.complete_relations(embed, w, k, relations=torch.as_tensor(relations, dtype=torch.long),
                                                          filter_index=filter_index, flow_log_prob=flow_log_prob, **constrained)
    n_lines = 0
    with open(path, 'w') as f:
        for r, ss, os_, xs in zip(relations, subj.tolist(), obj.tolist(), logits.tolist()):
            lines = [f"{a}\t{r}\t{b}\t{i}\t{x:.9g}\n" for i, (a, b, x) in enumerate(zip(ss, os_, xs), 1) if a >= 0]
            f.writelines(lines)
            n_lines += len(lines)
    return n_lines


def profile_lines(side, entities, rel, other, *value_columns):
    """The lines of a per-entity TSV for one side, ``entity  side  relation  other_entity  rank  value...``: one per returned fact
    of every entity of ``entities`` (``rel``, ``other`` and each value column are its (m, k) results, best first), the rank counted
    from 1, the padding slots (relation < 0) left out, every value column as ``:.9g``."""
    lines = []
    for a, rs, xs, *vs in zip(torch.as_tensor(entities).tolist(), rel.tolist(), other.tolist(), *(v.tolist() for v in value_columns)):
        lines += [f"{a}\t{side}\t{r}\t{x}\t{i}\t" + '\t'.join(f"{v:.9g}" for v in values) + '\n'
                  for i, (r, x, *values) in enumerate(zip(rs, xs, *vs), 1) if r >= 0]
    return lines


def write_profile_lines(path, entities, route, rows=PROFILE_ROWS):
    """The loop of the profile writers (this file's two and transe.py's): the 's' lines of every entity, then the 'o' lines,
    ``rows`` entities per call of ``route(part, side)`` -> ``(rel, other, *value_columns)``, as ``profile_lines`` formats them.
    Returns the number of lines written."""
    n_lines = 0
    with torch.no_grad(), open(path, 'w') as f:
        for side in ('s', 'o'):
            for at in range(0, entities.numel(), rows):
                part = entities[at:at + rows]
                lines = profile_lines(side, part, *route(part, side))
                f.writelines(lines)
                n_lines += len(lines)
    return n_lines


def write_relation_lines(path, triplets, route, rows=PROFILE_ROWS):
    """The loop of the relation-prediction writers (this file's and transe.py's): one block per triplet, in order, ``rows`` pairs per
    call of ``route(s, o)`` -> ``(ids, *value_columns)`` (each (m, k), best first), as TSV ``subject  object  position
    predicted_relation  value...`` -- the formatting of the top-k prediction files (position from 0, every value as ``:.9g``, padding
    slots written with their id -1).  Returns the number of lines written."""
    n_lines = 0
    with torch.no_grad(), open(path, 'w') as f:
        for at in range(0, triplets.shape[0], rows):
            s, o = triplets[at:at + rows, 0], triplets[at:at + rows, 2]
            ids, *values = route(s, o)
            for a, b, row_ids, *row_values in zip(s.tolist(), o.tolist(), ids.tolist(), *(v.tolist() for v in values)):
                head = f"{a}\t{b}\t"
                f.writelines(f"{head}{p}\t{e}\t" + '\t'.join(f"{x:.9g}" for x in xs) + '\n'
                             for p, (e, *xs) in enumerate(zip(row_ids, *row_values)))
                n_lines += len(row_ids)
    return n_lines


def write_relation_predictions(path, embed, w, triplets, k, pair_filter, flow_log_prob=None, type_constraint=None):
    """The ``k`` most plausible NEW relations of every triplet's pair (ranking.predict_relations; ``pair_filter``: the pair's known
    relations left out) as TSV: ``subject  object  position  predicted_relation  logit``, one block of k lines per triplet, in
    order; a pair with fewer than k relations left ends in id -1, logit -inf.  With a ``type_constraint`` (ranking.TypeConstraint)
    only type-correct relations are written, in the same columns.  Returns the number of lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    return write_relation_lines(path, triplets, lambda s, o: ranking.predict_relations(embed, w, s, o, k, pair_filter, flow_log_prob,
                                                                                       **constrained))


def write_mc_relation_predictions(path, z, w, triplets, k, pair_filter, flow_log_probs=None, type_constraint=None):
    """``write_relation_predictions`` under the posterior predictive of the samples ``z`` (S, N, h) (ranking.predict_relations_mc), as
    TSV: ``subject  object  position  predicted_relation  prob_mean  prob_std`` -- the first three columns join with the single-draw
    file; a pair with fewer than k relations left ends in id -1, mean -inf, std 0.  Returns the number of lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}
    return write_relation_lines(path, triplets, lambda s, o: ranking.predict_relations_mc(z, w, s, o, k, pair_filter, flow_log_probs,
                                                                                          **constrained))


def write_entity_profiles(path, embed, w, entities, k, filter_index, flow_log_prob=None, type_constraint=None):
    """Per-entity completion as TSV, ``entity  side  relation  other_entity  rank  logit  probability``: for every entity of
    ``entities`` its ``k`` most likely new facts over all relations (ranking.complete_entities; ``filter_index``: the known ones
    left out, as are loops), best first with the rank counted from 1 -- the 's' lines are the facts (entity, relation, other),
    then the 'o' lines the facts (other, relation, entity).  An entity with fewer than k candidates has fewer lines.  With a
    ``type_constraint`` (ranking.TypeConstraint) only type-correct facts are written, in the same columns.  Returns the number of
    lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}

    def route(part, side):
        rel, other, logits = ranking.complete_entities(embed, w, part, k, side=side, filter_index=filter_index,
                                                       flow_log_prob=flow_log_prob, **constrained)
        return rel, other, logits, torch.sigmoid(logits)

    return write_profile_lines(path, torch.as_tensor(entities, dtype=torch.long, device=embed.device).reshape(-1), route)


def write_mc_entity_profiles(path, z, w, entities, k, filter_index, flow_log_probs=None, type_constraint=None):
    """``write_entity_profiles`` under the posterior predictive of the samples ``z`` (S, N, h) (ranking.complete_entities_mc), as
    TSV: ``entity  side  relation  other_entity  rank  prob_mean  prob_std`` -- the first five columns are those of
    ``write_entity_profiles`` (the two files join on them), the last two the mean and the population standard deviation over the
    samples of the fact's probability; best mean first, the rank counted from 1.  With a ``type_constraint``
    (ranking.TypeConstraint) only type-correct facts are written.  Returns the number of lines written."""
    constrained = {} if type_constraint is None else {'type_constraint': type_constraint}

    def route(part, side):                      # (rel, other, mean, std): the value columns as they come
        return ranking.complete_entities_mc(z, w, part, k, side=side, filter_index=filter_index, flow_log_probs=flow_log_probs,
                                            **constrained)

    return write_profile_lines(path, torch.as_tensor(entities, dtype=torch.long, device=z.device).reshape(-1), route)


def write_completions(path, embed, w, filter_index, k=None, threshold=None, flow_log_prob=None, type_constraint=None):
    """Knowledge-graph completion as TSV, ``s  r  o  rank  logit``: the new triplets (``filter_index``: the known ones left out,
    s != o) that ``ranking.mine_triplets`` selects among ALL N x R x N -- the ``k`` most confident and / or those whose
    probability sigmoid(logit) reaches ``threshold`` -- best first; with a ``type_constraint`` among the type-correct ones only.
    Returns the number of lines written."""
    with torch.no_grad():
        if k:
            trip, logits, _ = ranking.mine_triplets(embed, w, k=k, filter_index=filter_index, flow_log_prob=flow_log_prob,
                                                    type_constraint=type_constraint)
            if threshold is not None:
                keep = logits >= _logit_of(threshold)
                trip, logits = trip[keep], logits[keep]
        else:
            trip, logits, _ = ranking.mine_triplets(embed, w, threshold=_logit_of(threshold), filter_index=filter_index,
                                                    flow_log_prob=flow_log_prob, type_constraint=type_constraint)
    return _write_triplets(path, trip, logits)


def write_mc_completions(path, z, w, filter_index, type_constraint, k=None, threshold=None, flow_log_probs=None):
    """``write_completions`` under the posterior predictive of the samples ``z`` (S, N, h), among the type-correct triplets
    (ranking.mine_triplets_mc), as TSV: ``s  r  o  rank  prob_mean  prob_std`` -- the first four columns are those of
    ``write_completions`` (the two files join on s, r, o; the rank here counts from 1), the last two the mean and the population
    standard deviation over the samples of the triplet's probability.  ``k`` the most probable and / or those whose mean probability reaches ``threshold``, best first.  Returns the
    number of lines written."""
    with torch.no_grad():
        sel = dict(k=k) if k else dict(threshold=float(threshold))
        trip, mean, std, _ = ranking.mine_triplets_mc(z, w, filter_index=filter_index, flow_log_probs=flow_log_probs,
                                                      type_constraint=type_constraint, **sel)
        if k and threshold is not None:
            keep = mean >= float(threshold)
            trip, mean, std = trip[keep], mean[keep], std[keep]
    with open(path, 'w') as f:
        f.writelines(f"{s}\t{r}\t{o}\t{i}\t{x:.9g}\t{y:.9g}\n"
                     for i, ((s, r, o), x, y) in enumerate(zip(trip.tolist(), mean.tolist(), std.tolist()), 1))
    return trip.shape[0]


def _logit_of(p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f'a probability lies in [0, 1], got {p}')
    return float('-inf') if p == 0.0 else float('inf') if p == 1.0 else float(np.log(p / (1.0 - p)))


def _write_triplets(path, trip, logits):
    with open(path, 'w') as f:
        f.writelines(f"{s}\t{r}\t{o}\t{i}\t{x:.9g}\n" for i, ((s, r, o), x) in enumerate(zip(trip.tolist(), logits.tolist())))
    return trip.shape[0]


def check_args(args):
    """Flag combinations that are refused before anything is loaded."""
    if not 0 <= getattr(args, 'profile_topk', 0) <= ops.TOPK_MAX:
        raise ValueError(f'--profile-topk keeps one list of at most {ops.TOPK_MAX} facts per entity (0 = off), got {args.profile_topk}')
    if getattr(args, 'profile_typed', False) and not getattr(args, 'profile_topk', 0) > 0:
        raise ValueError('--profile-typed restricts the profiles: it needs --profile-topk')
    if getattr(args, 'relation_profile_topk', 0) < 0:
        raise ValueError(f'--relation-profile-topk counts the facts kept per relation: 0 (off) or more, got {args.relation_profile_topk}')
    if getattr(args, 'relation_profile_typed', False) and not getattr(args, 'relation_profile_topk', 0) > 0:
        raise ValueError('--relation-profile-typed restricts the per-relation lists: it needs --relation-profile-topk')
    if getattr(args, 'relation_profile_ids', None) is not None:
        if not getattr(args, 'relation_profile_topk', 0) > 0:
            raise ValueError('--relation-profile-ids chooses the relations of the per-relation lists: it needs --relation-profile-topk')
        relation_profile_ids_arg(args.relation_profile_ids)
    if not 0 <= getattr(args, 'predict_relations', 0) <= ops.TOPK_MAX:
        raise ValueError(f'--predict-relations must lie in [1, {ops.TOPK_MAX}] (0 = off), got {args.predict_relations}')
    relations = getattr(args, 'relation_eval', False) or getattr(args, 'predict_relations', 0) > 0
    if getattr(args, 'relations_typed', False) and not relations:
        raise ValueError('--relations-typed restricts the relation queries: it needs --relation-eval or --predict-relations')
    if getattr(args, 'mc_relations', False):
        if not getattr(args, 'mc_samples', 0) > 0:
            raise ValueError('--mc-relations answers the relation queries on the posterior predictive: it needs --mc-samples S > 0')
        if not relations:
            raise ValueError('--mc-relations writes the posterior-predictive form of the relation queries: it needs --relation-eval '
                             'or --predict-relations')
    wants = [f for f, on in (('--relation-eval', getattr(args, 'relation_eval', False)),
                             ('--predict-relations', getattr(args, 'predict_relations', 0) > 0),
                             ('--profile-topk', getattr(args, 'profile_topk', 0) > 0),
                             ('--relation-profile-topk', getattr(args, 'relation_profile_topk', 0) > 0),
                             ('--complete-topk', getattr(args, 'complete_topk', 0) > 0),
                             ('--complete-threshold', getattr(args, 'complete_threshold', None) is not None),
                             ('--sample-graph', getattr(args, 'sample_graph', 0) > 0)) if on]
    if wants and args.test_mode is not True:
        raise ValueError(f"{' / '.join(wants)} decode a trained checkpoint: pass --test-mode True (and --model-state-file)")
    if getattr(args, 'complete_threshold', None) is not None:
        _logit_of(args.complete_threshold)
    if getattr(args, 'complete_typed', False) and not (getattr(args, 'complete_topk', 0) > 0
                                                      or getattr(args, 'complete_threshold', None) is not None):
        raise ValueError('--complete-typed restricts the completions: it needs --complete-topk or --complete-threshold')
    if getattr(args, 'type_constrain', False):
        if args.test_mode is not True:
            raise ValueError('--type-constrain reports on / predicts from a trained checkpoint: pass --test-mode True '
                             '(and --model-state-file)')
        if not getattr(args, 'filtered_eval', False):
            raise ValueError('--type-constrain needs --filtered-eval: the report is raw, filtered, raw_constrained, '
                             'filtered_constrained')
    if getattr(args, 'mc_samples', 0) < 0:
        raise ValueError(f'--mc-samples counts posterior samples: 0 (off) or more, got {args.mc_samples}')
    if getattr(args, 'mc_samples', 0) > 0:
        if args.test_mode is not True:
            raise ValueError('--mc-samples reports on / predicts from a trained checkpoint: pass --test-mode True '
                             '(and --model-state-file)')
        if args.model_class != 'KGVAE':
            raise ValueError('--mc-samples needs --model-class KGVAE: the RGCN encoder is deterministic, it has no posterior '
                             'to sample')
        if getattr(args, 'type_constrain', False):
            raise ValueError('--mc-samples with --type-constrain is not supported: --type-constrain reports on the single draw; '
                             'the type-constrained posterior-predictive report is --mc-type-constrain')
    if getattr(args, 'mc_type_constrain', False):
        if not getattr(args, 'mc_samples', 0) > 0:
            raise ValueError('--mc-type-constrain constrains the posterior-predictive report: it needs --mc-samples S > 0')
        if not getattr(args, 'filtered_eval', False):
            raise ValueError('--mc-type-constrain needs --filtered-eval: the report is raw, filtered, raw_constrained, '
                             'filtered_constrained')
    if getattr(args, 'mc_complete', False):
        if not getattr(args, 'mc_samples', 0) > 0:
            raise ValueError('--mc-complete mines on the posterior predictive: it needs --mc-samples S > 0')
        if not getattr(args, 'complete_typed', False):
            raise ValueError('--mc-complete needs --complete-typed: only the sweep over the type-correct triplets has a '
                             'Monte-Carlo form')
        # (--complete-typed without --complete-topk / --complete-threshold was refused above: a selection is given)
    if getattr(args, 'mc_profile', False):
        if not getattr(args, 'mc_samples', 0) > 0:
            raise ValueError('--mc-profile profiles the entities on the posterior predictive: it needs --mc-samples S > 0')
        if not getattr(args, 'profile_topk', 0) > 0:
            raise ValueError('--mc-profile writes the posterior-predictive form of the profiles: it needs --profile-topk K > 0')


def main(args):
    check_args(args)
    data = load_data(args.dataset)
    num_nodes, num_rels = data.num_nodes, data.num_rels
    train_data, valid_data, test_data = data.train, data.valid, data.test
    if getattr(args, 'relation_profile_topk', 0) > 0:
        relation_profile_ids_arg(getattr(args, 'relation_profile_ids', None), num_rels)      # a bad id: before the model is built

    if args.gpu < 0 or not torch.cuda.is_available():
        raise RuntimeError('gcn_vae_amd runs on a ROCm device only (pass --gpu N on an MI355X box); '
                           'there is no CPU path')
    torch.cuda.set_device(args.gpu)
    dev = torch.device('cuda', args.gpu)
    ops.set_gemm_precision('bf16' if getattr(args, 'bf16', False) else 'f32')

    model_class = KGVAE if args.model_class == "KGVAE" else RGCN
    model = LinkPredict(model_class=model_class, in_dim=num_nodes, h_dim=args.n_hidden, num_rels=num_rels,
                        num_bases=args.n_bases, num_hidden_layers=args.n_layers, dropout=args.dropout, use_cuda=True,
                        reg_param=args.regularization, kl_param=args.kl_param, mmd_param=args.mmd_param,
                        k=args.mog_k, n_flows=args.n_flows)
    model.to(dev)

    def graph_inputs(triplets):
        g, rel, norm = sampling.build_test_graph(num_nodes, num_rels, triplets)
        node_id = torch.arange(0, num_nodes, dtype=torch.long, device=dev).view(-1, 1)
        enorm = node_norm_to_edge_norm(g, torch.from_numpy(norm).view(-1, 1)).to(dev)
        return g, node_id, torch.from_numpy(rel).to(dev), enorm

    valid_t = torch.as_tensor(valid_data, dtype=torch.long, device=dev)
    val_graph, val_node_id, val_rel, val_norm = graph_inputs(valid_data)     # eval graph from VALID triplets (:141-147)
    adj_list, degrees = sampling.get_adj_and_degrees(num_nodes, train_data)
    optimizer = FlatAdam(model.parameters(), lr=args.lr, max_grad_norm=args.grad_norm)   # clip + Adam, one arena
    forward_time, backward_time, step_time = [], [], []
    # --filtered-eval: the known triplets (train + valid + test) indexed once; model selection stays on the raw MRR
    filters = ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev) \
        if getattr(args, 'filtered_eval', False) else None

    if args.test_mode is True:
        print("\nstart testing:")
        # --type-constrain: per relation and side, the entities seen there in train + valid + test
        types = ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev) \
            if getattr(args, 'type_constrain', False) else None
        checkpoint = torch.load(args.model_state_file, map_location=dev)
        test_t = torch.as_tensor(test_data, dtype=torch.long, device=dev)
        test_graph, test_node_id, test_rel, test_norm = graph_inputs(test_data)
        model.eval()
        model.load_state_dict(checkpoint['state_dict'])
        print("Using best epoch: {}".format(checkpoint['epoch']))
        with torch.no_grad():
            embed = model(test_graph, test_node_id, test_rel, test_norm)
        if getattr(args, 'predict_topk', 0) > 0:
            known = filters if filters is not None else \
                ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            n_lines = write_predictions(args.predict_out, embed, model.w_relation, test_t, args.predict_topk, known,
                                        model.encoder.get_flow_log_prob(), types)
            print(f"wrote {n_lines} predictions (top {args.predict_topk}, both directions, known triplets filtered) to "
                  f"{args.predict_out}")
        if getattr(args, 'profile_topk', 0) > 0:
            known = filters if filters is not None else \
                ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            who = profile_entities_arg(getattr(args, 'profile_entities', None), num_nodes)
            typed = None
            if getattr(args, 'profile_typed', False):      # (--type-constrain's sets are the same ones, when it is given as well)
                typed = types if types is not None else \
                    ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            n_lines = write_entity_profiles(args.profile_out, embed, model.w_relation, who, args.profile_topk, known,
                                            model.encoder.get_flow_log_prob(), typed)
            print(f"wrote {n_lines} new {'type-correct ' if typed is not None else ''}facts around {len(who)} entities (top "
                  f"{args.profile_topk} over all relations, as subject and as object, known triplets filtered) to {args.profile_out}")
        if getattr(args, 'relation_profile_topk', 0) > 0:
            known = filters if filters is not None else \
                ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            which = relation_profile_ids_arg(getattr(args, 'relation_profile_ids', None), num_rels)
            typed = None
            if getattr(args, 'relation_profile_typed', False):      # (--type-constrain's sets are the same ones, when it is given as well)
                typed = types if types is not None else \
                    ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            n_lines = write_relation_profiles(args.relation_profile_out, embed, model.w_relation, which, args.relation_profile_topk,
                                              known, model.encoder.get_flow_log_prob(), typed)
            print(f"wrote {n_lines} new {'type-correct ' if typed is not None else ''}facts of {len(which)} relations (each "
                  f"relation's own top {args.relation_profile_topk}, known triplets filtered) to {args.relation_profile_out}")
        if getattr(args, 'relation_eval', False) or getattr(args, 'predict_relations', 0) > 0:
            pairs = ranking.PairFilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            rel_types = None
            if getattr(args, 'relations_typed', False):    # (--type-constrain's sets are the same ones, when it is given as well)
                rel_types = types if types is not None else \
                    ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            if getattr(args, 'relation_eval', False):
                ranking.calc_relation_mrr(embed, model.w_relation, test_t, pairs if filters is not None else None, hits=[1, 3, 10],
                                          flow_log_prob=model.encoder.get_flow_log_prob(), type_constraint=rel_types)
            if getattr(args, 'predict_relations', 0) > 0:
                n_lines = write_relation_predictions(args.relations_out, embed, model.w_relation, test_t, args.predict_relations,
                                                     pairs, model.encoder.get_flow_log_prob(), rel_types)
                print(f"wrote {n_lines} relation predictions (top {args.predict_relations} {'type-correct ' if rel_types is not None else ''}"
                      f"per test pair, known relations filtered) to {args.relations_out}")
        if getattr(args, 'complete_topk', 0) > 0 or getattr(args, 'complete_threshold', None) is not None:
            known = filters if filters is not None else \
                ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            typed = None
            if getattr(args, 'complete_typed', False):
                typed = types if types is not None else \
                    ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
            n_lines = write_completions(args.complete_out, embed, model.w_relation, known, k=args.complete_topk or None,
                                        threshold=args.complete_threshold, flow_log_prob=model.encoder.get_flow_log_prob(),
                                        type_constraint=typed)
            scored = "the type-correct triplets" if typed is not None else f"all {num_nodes} x {num_rels} x {num_nodes}"
            print(f"wrote {n_lines} new triplets ({scored} scored, known triplets filtered) to {args.complete_out}")
        if getattr(args, 'sample_graph', 0) > 0:
            from . import generate
            _, trip, logits = generate.sample_graph(model, args.sample_graph, k=args.sample_topk)
            print(f"wrote {_write_triplets(args.sample_out, trip, logits)} triplets of a graph decoded from {args.sample_graph} "
                  f"prior samples to {args.sample_out}")
        if types is not None:
            mrr = ranking.calc_constrained_mrr(embed, model.w_relation, test_t, filters, types, hits=[1, 3, 10],
                                               eval_bz=args.eval_batch_size, all_batches=True,
                                               flow_log_prob=model.encoder.get_flow_log_prob())['mrr_raw']
        elif filters is not None:
            mrr = ranking.calc_filtered_mrr(embed, model.w_relation, test_t, filters, hits=[1, 3, 10],
                                            eval_bz=args.eval_batch_size, all_batches=True,
                                            flow_log_prob=model.encoder.get_flow_log_prob())['mrr_raw']
        else:
            mrr = ranking.calc_mrr(embed, model.w_relation, test_t, hits=[1, 3, 10], eval_bz=args.eval_batch_size,
                                   all_batches=True, flow_log_prob=model.encoder.get_flow_log_prob())
        if getattr(args, 'mc_samples', 0) > 0:
            # the posterior predictive, after everything the single draw reports: S seeded samples of the latents, one encoder pass
            z, flps = model.encoder.posterior_samples(test_graph, test_node_id, test_rel, test_norm, args.mc_samples,
                                                      seed=args.mc_seed)
            print(f"\nMonte-Carlo posterior predictive: {args.mc_samples} samples, seed {args.mc_seed}")
            # --mc-type-constrain: the sets of --type-constrain (train + valid + test), applied to the posterior predictive
            mc_types = ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev) \
                if getattr(args, 'mc_type_constrain', False) else None
            if mc_types is not None:
                ranking.calc_mc_constrained_mrr(z, model.w_relation, test_t, filters, mc_types, flps, hits=[1, 3, 10],
                                                eval_bz=args.eval_batch_size, all_batches=True)
            else:
                ranking.calc_mc_mrr(z, model.w_relation, test_t, filters, flps, hits=[1, 3, 10], eval_bz=args.eval_batch_size,
                                    all_batches=True)
            if getattr(args, 'predict_topk', 0) > 0:
                known = filters if filters is not None else \
                    ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
                n_lines = write_mc_predictions(args.mc_predict_out, z, model.w_relation, test_t, args.predict_topk, known, flps,
                                               mc_types)
                typed_note = ", type-correct entities only" if mc_types is not None else ""
                print(f"wrote {n_lines} posterior-predictive predictions (top {args.predict_topk}, both directions, known "
                      f"triplets filtered{typed_note}, mean and spread over {args.mc_samples} samples) to {args.mc_predict_out}")
            if getattr(args, 'mc_relations', False):
                if getattr(args, 'relation_eval', False):
                    ranking.calc_relation_mc_mrr(z, model.w_relation, test_t, pairs if filters is not None else None, flps,
                                                 hits=[1, 3, 10], type_constraint=rel_types)
                if getattr(args, 'predict_relations', 0) > 0:
                    n_lines = write_mc_relation_predictions(args.mc_relations_out, z, model.w_relation, test_t, args.predict_relations,
                                                            pairs, flps, rel_types)
                    print(f"wrote {n_lines} posterior-predictive relation predictions (top {args.predict_relations} "
                          f"{'type-correct ' if rel_types is not None else ''}per test pair, known relations filtered, mean and spread "
                          f"over {args.mc_samples} samples) to {args.mc_relations_out}")
            if getattr(args, 'mc_complete', False):
                known = filters if filters is not None else \
                    ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
                typed = types if types is not None else \
                    ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
                n_lines = write_mc_completions(args.mc_complete_out, z, model.w_relation, known, typed, k=args.complete_topk or None,
                                               threshold=args.complete_threshold, flow_log_probs=flps)
                print(f"wrote {n_lines} new type-correct triplets (known triplets filtered, mean and spread over "
                      f"{args.mc_samples} samples) to {args.mc_complete_out}")
            if getattr(args, 'mc_profile', False):
                known = filters if filters is not None else \
                    ranking.FilterIndex(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
                who = profile_entities_arg(getattr(args, 'profile_entities', None), num_nodes)
                typed = None
                if getattr(args, 'profile_typed', False):
                    typed = types if types is not None else \
                        ranking.TypeConstraint(num_nodes, num_rels, train_data, valid_data, test_data, device=dev)
                n_lines = write_mc_entity_profiles(args.mc_profile_out, z, model.w_relation, who, args.profile_topk, known, flps, typed)
                print(f"wrote {n_lines} new {'type-correct ' if typed is not None else ''}facts around {len(who)} entities (top "
                      f"{args.profile_topk} over all relations, as subject and as object, known triplets filtered, mean and spread "
                      f"over {args.mc_samples} samples) to {args.mc_profile_out}")
        return mrr

    print("start training...")
    epoch, best_mrr = 0, 0
    if args.load is True:
        print(f"Loading checkpoint file {args.model_state_file} for training")
        checkpoint = torch.load(args.model_state_file, map_location=dev)
        model.load_state_dict(checkpoint['state_dict'])
        epoch = checkpoint['epoch']

    dev_sampler = None
    if getattr(args, 'device_sampler', False):
        from .device_sampling import DeviceSampler
        dev_sampler = DeviceSampler(train_data, num_nodes, num_rels, dev, sampler=args.edge_sampler)

    graphed = None
    if getattr(args, 'graph_step', False):
        if dev_sampler is None:
            raise ValueError('--graph-step records the device sampler with the step: pass --device-sampler too')
        from .graph_step import GraphedMiniBatchStep
        if args.kl_param <= 0:
            raise ValueError('--graph-step needs --kl-param > 0 (the captured loss head reads the device row count there)')
        model.train()
        graphed = GraphedMiniBatchStep(model, optimizer, dev_sampler, args.graph_batch_size, args.graph_split_size,
                                       args.negative_sample)
        graph_warmup = 3                             # the first steps run eagerly (ordinary epochs: printed, evaluated), then the recording

    while True:
        model.train()
        epoch += 1
        if graphed is not None:      # the whole step -- sampling to Adam -- is one hipGraph replay
            if graphed.graph is None and graph_warmup == 0:
                graphed.capture(warmup=0)
            graph_warmup = max(0, graph_warmup - 1)
            _sync()
            t0 = time.time()
            loss, pred_loss, kl, mmd = graphed()
            _sync()
            step_time.append(time.time() - t0)
            print("Epoch {:04d} | Loss {:.4f} | Best MRR {:.4f} | pred_loss {:.4f} | kl {:.4f} | mmd {:.4f}".format(
                epoch, loss.item(), best_mrr, pred_loss.item(), kl.item(), mmd.item()))
        elif dev_sampler is not None:
            b = dev_sampler.sample(args.graph_batch_size, args.graph_split_size, args.negative_sample)
            g, node_id, edge_type, edge_norm, batch, labels = b.g, b.node_id, b.edge_type, b.edge_norm, b.samples, b.labels
        else:
            g, node_id, edge_type, node_norm, batch, labels = sampling.generate_sampled_graph_and_labels(
                train_data, args.graph_batch_size, args.graph_split_size, num_rels, adj_list, degrees,
                args.negative_sample, args.edge_sampler)
            node_id = torch.from_numpy(node_id).view(-1, 1).long().to(dev)
            edge_type = torch.from_numpy(edge_type).to(dev)
            edge_norm = node_norm_to_edge_norm(g, torch.from_numpy(node_norm).view(-1, 1)).to(dev)
            batch, labels = torch.from_numpy(batch).to(dev), torch.from_numpy(labels).to(dev)

        if graphed is None:
            _sync()
            t0 = time.time()
            embed = model(g, node_id, edge_type, edge_norm)
            loss, pred_loss, kl, mmd = model.get_loss(g, embed, batch, labels)
            _sync()
            t1 = time.time()
            loss.backward()
            optimizer.step()              # clip_grad_norm_(grad_norm) + Adam, fused
            _sync()
            t2 = time.time()
            forward_time.append(t1 - t0)
            backward_time.append(t2 - t1)
            print("Epoch {:04d} | Loss {:.4f} | Best MRR {:.4f} | pred_loss {:.4f} | kl {:.4f} | mmd {:.4f}".format(
                epoch, loss.item(), best_mrr, pred_loss.item(), kl.item(), mmd.item()))
            optimizer.zero_grad()

        if epoch % args.evaluate_every == 0:
            model.eval()
            print("start eval")
            torch.save({'state_dict': host_state_dict(model), 'epoch': epoch}, args.model_state_file)
            with torch.no_grad():
                embed = model(val_graph, val_node_id, val_rel, val_norm)
            if filters is not None:
                mrr = ranking.calc_filtered_mrr(embed, model.w_relation, valid_t, filters, hits=[1, 3, 10],
                                                eval_bz=args.eval_batch_size, all_batches=False,
                                                flow_log_prob=model.encoder.get_flow_log_prob())['mrr_raw']
            else:
                mrr = ranking.calc_mrr(embed, model.w_relation, valid_t, hits=[1, 3, 10], eval_bz=args.eval_batch_size,
                                       all_batches=False, flow_log_prob=model.encoder.get_flow_log_prob())
            if mrr < best_mrr:
                torch.save({'state_dict': host_state_dict(model), 'epoch': epoch}, args.model_state_file + "_latest")
            else:
                best_mrr = mrr
                torch.save({'state_dict': host_state_dict(model), 'epoch': epoch}, args.model_state_file)
        if epoch >= args.n_epochs:
            break

    print("training done")
    if step_time:     # the captured step has no forward / backward boundary on the host: one figure
        print("Mean step time (forward + backward + update, one hipGraph): {:4f}s".format(np.mean(step_time)))
    else:
        print("Mean forward time: {:4f}s".format(np.mean(forward_time)))
        print("Mean Backward time: {:4f}s".format(np.mean(backward_time)))
    return best_mrr


def build_parser():
    p = argparse.ArgumentParser(description='Link Prediction')
    p.add_argument("--dropout", type=float, default=0.2, help="dropout probability")
    p.add_argument("--n-hidden", type=int, default=500, help="number of hidden units")
    p.add_argument("--gpu", type=int, default=-1, help="gpu")
    p.add_argument("--lr", type=float, default=1e-3, help="learning rate")
    p.add_argument("--n-bases", type=int, default=100, help="number of weight blocks for each relation")
    p.add_argument("--n-layers", type=int, default=2, help="number of propagation rounds")
    p.add_argument("--n-epochs", type=int, default=1e5, help="number of minimum training epochs")
    p.add_argument("-d", "--dataset", type=str, required=True, help="dataset to use")
    p.add_argument("--eval-batch-size", type=int, default=400, help="batch size when evaluating")
    p.add_argument("--regularization", type=float, default=0.01, help="regularization weight")
    p.add_argument("--kl-param", type=float, default=1e-5, help="kl regularization weight")
    p.add_argument("--mmd-param", type=float, default=0, help="mmd regularization weight")
    p.add_argument("--mog-k", type=int, default=10, help="number of mixture of gaussian")
    p.add_argument("--n-flows", type=int, default=0, help="number of flow transform layers")
    p.add_argument("--grad-norm", type=float, default=1.0, help="norm to clip gradient to")
    p.add_argument("--graph-batch-size", type=int, default=20000, help="number of edges to sample in each iteration")
    p.add_argument("--graph-split-size", type=float, default=0.5, help="portion of edges used as positive sample")
    p.add_argument("--negative-sample", type=int, default=10, help="number of negative samples per positive sample")
    p.add_argument("--evaluate-every", type=int, default=200, help="perform evaluation every n epochs")
    p.add_argument("--edge-sampler", type=str, default="uniform", help="type of edge sampler: 'uniform' or 'neighbor'")
    p.add_argument("--test-mode", type=bool, default=False, help="only evaluate on test dataset")
    p.add_argument("--model-state-file", type=str, default='model_state.pth', help="model state file to load or save")
    p.add_argument("--model-class", type=str, default='KGVAE', help="model class")
    p.add_argument("--load", type=bool, default=False, help="whether to load a model state file for training")
    p.add_argument("--generate", type=bool, default=False, help="(reference demo; not supported here)")
    p.add_argument("--bf16", action="store_true",
                   help="dense products (MaskedLinear, self-loop term, evaluation scorer) with bf16 operands and fp32 "
                        "accumulation (BASELINE configs[2]); not a reference flag, default fp32")
    p.add_argument("--graph-step", action="store_true",
                   help="with --device-sampler: record sampling + forward + loss + backward + clip/Adam once and replay it "
                        "as one hipGraph per step (static shapes: node rows padded, counts kept on the device)")
    p.add_argument("--device-sampler", action="store_true",
                   help="prepare batches on the GPU (uniform sampler, torch's device RNG instead of numpy's: not the "
                        "reference's random stream, ~10x less host time per step)")
    p.add_argument("--filtered-eval", action="store_true",
                   help="also report filtered MRR and Hits@1/3/10 (the other known answers of a query -- train + valid + "
                        "test -- left out of its rank); model selection stays on the raw MRR; not a reference flag")
    p.add_argument("--type-constrain", action="store_true",
                   help="with --test-mode and --filtered-eval: the type-constrained protocol (candidates: the entities seen on "
                        "that side of the relation in train + valid + test); the report is raw, filtered, raw_constrained and "
                        "filtered_constrained, and --predict-topk writes such entities only; --complete-topk / "
                        "--complete-threshold are not touched and keep writing unconstrained completions (see --complete-typed); "
                        "not a reference flag")
    p.add_argument("--predict-topk", type=int, default=0,
                   help="with --test-mode: write the K most likely new entities of both directions of every test triplet "
                        "(train + valid + test triplets filtered out) to --predict-out; 0 = off; not a reference flag")
    p.add_argument("--predict-out", type=str, default="predictions.tsv",
                   help="TSV of --predict-topk: direction, query entity, relation, position, predicted entity, logit")
    p.add_argument("--mc-samples", type=int, default=0,
                   help="with --test-mode (KGVAE): after the usual report, rank on the Monte-Carlo posterior predictive -- the "
                        "mean over S seeded posterior samples of the triplet probability -- raw, and filtered under "
                        "--filtered-eval; with --predict-topk also write --mc-predict-out; 0 = off; not a reference flag")
    p.add_argument("--mc-seed", type=int, default=0, help="seed of the --mc-samples posterior samples")
    p.add_argument("--mc-predict-out", type=str, default="mc_predictions.tsv",
                   help="TSV of --mc-samples with --predict-topk: direction, query entity, relation, position, predicted entity, "
                        "mean and standard deviation over the samples of its probability")
    p.add_argument("--complete-topk", type=int, default=0,
                   help="with --test-mode: score ALL triplets (s, r, o) and write the K most confident NEW ones (train + valid + "
                        "test triplets and s == o left out) to --complete-out; 0 = off; not a reference flag")
    p.add_argument("--complete-threshold", type=float, default=None,
                   help="with --test-mode: write every new triplet whose probability reaches P (with --complete-topk: the K best, "
                        "cut at P) to --complete-out")
    p.add_argument("--complete-out", type=str, default="completions.tsv",
                   help="TSV of --complete-topk / --complete-threshold: subject, relation, object, rank, logit")
    p.add_argument("--complete-typed", action="store_true",
                   help="with --complete-topk / --complete-threshold: mine among type-correct triplets only (the subject seen as "
                        "subject, the object seen as object of the relation in train + valid + test); needs no --filtered-eval")
    p.add_argument("--mc-type-constrain", action="store_true",
                   help="with --mc-samples and --filtered-eval: the type-constrained protocol on the posterior predictive -- the MC "
                        "report becomes raw / filtered / raw_constrained / filtered_constrained, and --mc-predict-out proposes "
                        "only entities seen on that side of the relation in train + valid + test; reproducible for a fixed "
                        "--mc-seed (--type-constrain itself stays a single-draw report)")
    p.add_argument("--mc-complete", action="store_true",
                   help="with --mc-samples, --complete-typed and --complete-topk / --complete-threshold: also mine the type-correct "
                        "completions on the posterior predictive (the mean over the samples of the triplet probability; the "
                        "threshold is compared with that mean) and write them to --mc-complete-out; reproducible for a fixed "
                        "--mc-seed")
    p.add_argument("--mc-complete-out", type=str, default="mc_completions.tsv",
                   help="TSV of --mc-complete: subject, relation, object, rank (the columns of --complete-out), then the mean and "
                        "the standard deviation over the samples of the triplet's probability")
    p.add_argument("--relation-eval", action="store_true",
                   help="with --test-mode: also report relation prediction over the test triplets -- MRR / Hits@k of the true "
                        "relation of (s, ?, o) among all relations; with --filtered-eval also with the pair's other known relations "
                        "(train + valid + test) left out; not a reference flag")
    p.add_argument("--predict-relations", type=int, default=0,
                   help="with --test-mode: write the K (1..128) most plausible NEW relations between subject and object of every test "
                        "triplet (the pair's train + valid + test relations left out) to --relations-out; 0 = off")
    p.add_argument("--relations-typed", action="store_true",
                   help="with --relation-eval / --predict-relations: also report the ranks among the TYPE-CORRECT relations of each "
                        "pair (the subject seen as subject of the relation, the object as its object, in train + valid + test) and "
                        "propose only those")
    p.add_argument("--mc-relations", action="store_true",
                   help="with --mc-samples S and --relation-eval / --predict-relations: the relation report and proposals on the "
                        "posterior predictive as well (honours --relations-typed)")
    p.add_argument("--mc-relations-out", type=str, default="mc_relation_predictions.tsv",
                   help="TSV written by --mc-relations with --predict-relations: subject, object, position, predicted relation, "
                        "prob_mean, prob_std; joins with --relations-out on the first three columns")
    p.add_argument("--relations-out", type=str, default="relation_predictions.tsv",
                   help="TSV of --predict-relations: subject, object, position, predicted relation, logit")
    p.add_argument("--profile-topk", type=int, default=0,
                   help="with --test-mode: for every entity of --profile-entities write its K most likely NEW facts over all "
                        "relations at once, the entity as subject and as object (train + valid + test triplets and loops left "
                        "out), to --profile-out; 1..128, 0 = off; not a reference flag")
    p.add_argument("--profile-entities", type=str, default=None,
                   help="the entities of --profile-topk: comma-separated ids, or a file with one id per line; default: every "
                        "entity")
    p.add_argument("--profile-out", type=str, default="profiles.tsv",
                   help="TSV of --profile-topk: entity, side (s: the entity is the subject, o: the object), relation, other "
                        "entity, rank from 1, logit, probability")
    p.add_argument("--profile-typed", action="store_true",
                   help="with --profile-topk: write type-correct facts only (the entity seen on its side of the relation, the other "
                        "entity seen on the other side, in train + valid + test); the same columns; --type-constrain does not "
                        "constrain profiles")
    p.add_argument("--relation-profile-topk", type=int, default=0,
                   help="with --test-mode: for every relation of --relation-profile-ids write ITS OWN K most confident NEW facts "
                        "(train + valid + test triplets and loops left out) to --relation-profile-out -- every relation has its own "
                        "threshold, where --complete-topk has one for the whole graph; 0 = off; not a reference flag")
    p.add_argument("--relation-profile-ids", type=str, default=None,
                   help="the relations of --relation-profile-topk: comma-separated ids, or a file with one id per line, each at most "
                        "once; default: every relation")
    p.add_argument("--relation-profile-out", type=str, default="relation_profiles.tsv",
                   help="TSV of --relation-profile-topk: s, r, o, rank from 1 within the relation, logit; relations in the order "
                        "asked; joins with --complete-out on s, r, o")
    p.add_argument("--relation-profile-typed", action="store_true",
                   help="with --relation-profile-topk: write type-correct facts only (s seen as subject of r, o seen as its object, "
                        "in train + valid + test); the same columns; --type-constrain and --complete-typed keep their meaning")
    p.add_argument("--mc-profile", action="store_true",
                   help="with --mc-samples and --profile-topk: also write the profiles on the posterior predictive (each entity's K "
                        "new facts of highest mean probability over the samples, with the spread) to --mc-profile-out; honours "
                        "--profile-entities and --profile-typed; reproducible for a fixed --mc-seed")
    p.add_argument("--mc-profile-out", type=str, default="mc_profiles.tsv",
                   help="TSV of --mc-profile: entity, side, relation, other entity, rank from 1 (the columns of --profile-out), then "
                        "the mean and the standard deviation over the samples of the fact's probability")
    p.add_argument("--sample-graph", type=int, default=0,
                   help="with --test-mode: draw M node latents from the prior (KGVAE.sample_z) and write the --sample-topk most "
                        "confident triplets among them to --sample-out; 0 = off")
    p.add_argument("--sample-topk", type=int, default=1000, help="triplets kept by --sample-graph")
    p.add_argument("--sample-out", type=str, default="sampled_graph.tsv",
                   help="TSV of --sample-graph: subject, relation, object, rank, logit")
    return p


if __name__ == '__main__':
    cli = build_parser().parse_args()
    print(cli)
    main(cli)
