"""The generative half of the KG-VAE: decode latents drawn from the prior into a graph.

``KGVAE.sample_z`` draws node latents from the mixture prior and pushes them back through the flows (the reference's
kgvae/model.py:61-69, which nothing there consumes).  Decoding a set of such latents is the all-pairs, all-relations selection of
``ranking.mine_triplets`` without a filter: the K most confident triplets among the sampled nodes, or all above a threshold.
"""
import torch

from . import ranking


def sample_graph(model, num_nodes, *, k=None, threshold=None, seed=None, max_results=None):
    """Sample ``num_nodes`` latents ``z = model.encoder.sample_z(num_nodes)`` (under ``torch.manual_seed(seed)`` when a seed is
    given) and mine them against ``model.w_relation``: no filter, no bias, s != o.  Returns ``(z, triplets int64 (n, 3), logits
    float32 (n,))`` in the order of ``ranking.mine_from_scores``; nodes are 0 .. num_nodes - 1 and relations the ids of
    ``w_relation`` (``num_rels`` of them, not doubled)."""
    if (k is None) == (threshold is None):
        raise ValueError('give exactly one of k and threshold')
    if seed is not None:
        torch.manual_seed(int(seed))
    with torch.no_grad():
        z = model.encoder.sample_z(int(num_nodes)).detach().to(torch.float32).contiguous()
        extra = {} if max_results is None else {'max_results': max_results}
        triplets, logits, _ = ranking.mine_triplets(z, model.w_relation, k=k, threshold=threshold, **extra)
    return z, triplets, logits
