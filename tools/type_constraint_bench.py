"""Cost of the type-constrained protocol on an MI355X: the constrained rank launch pair and the constrained top-k (k = 10, 100)
of both models against the existing unconstrained entry points, on the same queries in the same process.

    python tools/type_constraint_bench.py [--repeats 7] [--out profiles/type_constraint/bench.json]

Queries: both directions of the FB15k-237-sized synthetic test split (2 x 20 466 queries, 14 541 entities), filter and type sets
from train + valid + test.  DistMult at h = 200 with a flow bias, TransE at dim = 200, L1 and L2.  The two versions of a leg
alternate inside every repeat after three untimed rounds of both; every figure is the median of --repeats synchronised runs timed
with device events, in ms (the minimum is kept too); a ratio is constrained / unconstrained.  The drivers are timed as the CLIs
call them, host-side argument checks included, alike on both sides.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


WARMUP = 3


def _ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def _stat(out):
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), runs=[round(x, 3) for x in out])


def _pair(plain, constrained, repeats):
    """Both versions alternate inside every repeat (A B, A B, ...), after WARMUP untimed rounds of both."""
    for _ in range(WARMUP):
        plain()
        constrained()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(_ms(plain))
        tb.append(_ms(constrained))
    a, b = _stat(ta), _stat(tb)
    return dict(unconstrained=a, constrained=b, constrained_over_unconstrained=b['median_ms'] / a['median_ms'])


def run(repeats):
    from gcn_vae_amd import ranking, transe
    from gcn_vae_amd.data import load_data
    data = load_data('FB15k-237-synthetic')
    fi = ranking.FilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    tc = ranking.TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
    test = torch.as_tensor(np.asarray(data.test), dtype=torch.long).cuda()
    s, r, o = test[:, 0], test[:, 1], test[:, 2]
    n = len(test)
    sizes = tc.sizes.float()
    res = dict(queries=2 * n, entities=data.num_nodes, width=200, repeats=repeats, warmup=WARMUP,
               mean_set_share=float((sizes[torch.cat([r, r + data.num_rels])] / data.num_nodes).mean()))

    gen = torch.Generator().manual_seed(0)
    emb = (torch.randn(data.num_nodes, 200, generator=gen) * 0.3).cuda()
    w = torch.randn(data.num_rels, 200, generator=gen).cuda()
    flp = torch.tensor(0.3, device='cuda')

    def dm_rank(constrained):
        for a, b, d in ((o, s, 's'), (s, o, 'o')):
            if constrained:
                ranking.perturb_and_get_rank_constrained(emb, w, a, r, b, n, fi, tc, d, flow_log_prob=flp)
            else:
                ranking.perturb_and_get_rank_filtered(emb, w, a, r, b, n, fi, d, flow_log_prob=flp)

    def dm_topk(k, constrained):
        for a, d in ((s, 'o'), (o, 's')):
            ranking.predict_topk(emb, w, a, r, k, direction=d, filter_index=fi, flow_log_prob=flp,
                                 type_constraint=tc if constrained else None)
    res['distmult_rank'] = _pair(lambda: dm_rank(False), lambda: dm_rank(True), repeats)
    for k in (10, 100):
        res[f'distmult_topk_k{k}'] = _pair(lambda: dm_topk(k, False), lambda: dm_topk(k, True), repeats)

    torch.manual_seed(0)
    model = transe.TransE(data.num_nodes, data.num_rels, dim=200, p_norm=1, norm_flag=True).cuda()
    ent, rel = model.ent_embeddings.weight.data, model.rel_embeddings.weight.data
    for p in (1, 2):
        tables = (ent, rel, p, True)

        def te_topk(k, constrained):
            for a, d in ((s, 'o'), (o, 's')):
                transe.predict_topk(tables, a, r, k, direction=d, filter_index=fi, type_constraint=tc if constrained else None)
        res[f'transe_rank_p{p}'] = _pair(lambda: transe.rank_transe(ent, rel, test, p, True, fi),
                                         lambda: transe.rank_transe_constrained(ent, rel, test, p, True, tc, fi), repeats)
        for k in (10, 100):
            res[f'transe_topk_p{p}_k{k}'] = _pair(lambda: te_topk(k, False), lambda: te_topk(k, True), repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    res = run(a.repeats)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    for name, v in res.items():
        if isinstance(v, dict):
            print('{:24s} unconstrained {:9.3f} ms  constrained {:9.3f} ms  ratio {:.3f}'.format(
                name, v['unconstrained']['median_ms'], v['constrained']['median_ms'], v['constrained_over_unconstrained']))
    print('RESULT ' + json.dumps(res))


if __name__ == '__main__':
    main()
