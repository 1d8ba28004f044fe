#!/usr/bin/env python3
"""Relation prediction (s, ?, o) at FB15k-237-synthetic and WN18RR-synthetic size: the pairs of the test split (20 466 / 3 134),
filter = the pairs' train + valid + test relations, widths 200 and 500, DistMult and TransE (L1, L2).  Per cell three tasks --
the ranks of the true relation (raw + filtered), the top 10 new relations, and both -- and three routes:

    fused     one launch of gv_pair_rel_scores / gv_transe_pair_rel (ops.pair_relation_scores / ops.transe_pair_relations);
    composed  the existing kernels with the relation table as the candidates: the gathered rows' product (ops.mul; TransE: a torch
              subtraction) as a stored (m, h) query matrix, then ops.rank_scores_filtered / ops.topk_scores (ops.transe_rank_filtered /
              ops.transe_topk) -- "both" is the two calls on the one query matrix;
    twin      the materialised cross-check: the (m, R) matrix from one GEMM (ops.transe_distances), then ranking.mid_ranks /
              topk_from_scores in torch.

The filter ranges are looked up once, outside the timed regions (every route takes the same three arrays).  The routes are
alternated; each is warmed up once, then timed over --repeats synchronised regions of --inner calls each (a single call is tens of
microseconds: one call per region would time the clock), and the median per call is reported in ms.  The three answers are asserted
equal -- ranks by value, lists bit for bit -- before anything is timed.  Random tables: the time does not depend on the values.

    python tools/relation_bench.py [--out profiles/relation/bench.json] [--widths 200,500] [--repeats 5] [--inner 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from entity_bench_common import time_routes      # noqa: E402

DATASETS = {'fb': 'FB15k-237-synthetic', 'wn18rr': 'WN18RR-synthetic'}
K = 10


def _same_ranks(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _same_lists(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _routes(model, tables, s, o, r, filt, p):
    """{task: [(route, fn)]}; every fn returns (ranks or None, list or None)."""
    from gcn_vae_amd import ops, ranking, transe
    table, rels = tables
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    want = {'ranks': (True, False), 'topk': (False, True), 'both': (True, True)}
    if model == 'distmult':
        def fused(ranks, top):
            return ops.pair_relation_scores(table, rels, s, o, target=r if ranks else None, k=K if top else 0, **names)

        def composed(ranks, top):
            q = ops.mul(table[s].contiguous(), table[o].contiguous())
            return (ops.rank_scores_filtered(q, rels, r, *filt) if ranks else None,
                    ops.topk_scores(q, rels, K, None, *filt) if top else None)

        def twin(ranks, top):
            score = ranking.pair_scores_unfused(table, rels, s, o)
            return (ranking.relation_ranks_from_scores(score, r, *filt) if ranks else None,
                    ranking.topk_from_scores(score, K, *filt) if top else None)
    else:
        def fused(ranks, top):
            return ops.transe_pair_relations(table, rels, s, o, p, target=r if ranks else None, k=K if top else 0, **names)

        def composed(ranks, top):
            q = (table[o] - table[s]).contiguous()
            return (ops.transe_rank_filtered(q, rels, r, p, *filt) if ranks else None,
                    ops.transe_topk(q, rels, K, p, *filt) if top else None)

        def twin(ranks, top):
            dist = transe.pair_distances_unfused(table, rels, s, o, p)
            return (ranking.relation_ranks_from_scores(-dist, r, *filt) if ranks else None,
                    transe.topk_from_distances(dist, K, *filt) if top else None)
    return {task: [(nm, (lambda fn=fn, a=a: fn(*a))) for nm, fn in (('fused', fused), ('composed', composed), ('twin', twin))]
            for task, a in want.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'relation', 'bench.json'))
    ap.add_argument('--widths', default='200,500')
    ap.add_argument('--datasets', default='fb,wn18rr')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'relation_bench.py measures on the GPU: there is nothing to report without one'
    from gcn_vae_amd import ranking
    from gcn_vae_amd.data import load_data
    cells = []
    for ds in args.datasets.split(','):
        data = load_data(DATASETS[ds])
        test = torch.as_tensor(np.asarray(data.test), dtype=torch.long).cuda()
        s, r, o = (test[:, i].contiguous() for i in range(3))
        pf = ranking.PairFilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
        filt = (*pf.lookup(s, o), pf.relations('cuda'))
        for h in (int(x) for x in args.widths.split(',')):
            torch.manual_seed(0)
            ent = (torch.randn(data.num_nodes, h) * 0.3).cuda()
            rel = (torch.randn(data.num_rels, h) * 0.3).cuda()
            for model, p in (('distmult', None), ('transe', 1), ('transe', 2)):
                for task, routes in _routes(model, (ent, rel), s, o, r, filt, p).items():
                    timed = [(nm, (lambda fn=fn: [fn() for _ in range(args.inner)][-1])) for nm, fn in routes]
                    outs, ms = time_routes(timed, args.repeats)
                    for nm in ('composed', 'twin'):
                        if outs['fused'][0] is not None:
                            assert _same_ranks(outs['fused'][0], outs[nm][0]), (ds, h, model, p, task, nm)
                        if outs['fused'][1] is not None:
                            assert _same_lists(outs['fused'][1], outs[nm][1]), (ds, h, model, p, task, nm)
                    per_call = {nm: round(v / args.inner, 4) for nm, v in ms.items()}
                    cell = dict(dataset=DATASETS[ds], pairs=int(s.numel()), num_rels=int(data.num_rels), width=h,
                                model=model if p is None else f'{model}-L{p}', task=task, ms=per_call,
                                fused_over_composed=round(per_call['composed'] / per_call['fused'], 3),
                                fused_over_twin=round(per_call['twin'] / per_call['fused'], 3),
                                fused_loses_to=[nm for nm in ('composed', 'twin') if per_call[nm] < per_call['fused']])
                    cells.append(cell)
                    print(json.dumps(cell), flush=True)
    result = dict(tool='tools/relation_bench.py', k=K, repeats=args.repeats, inner_calls_per_region=args.inner,
                  unit='ms per call, median of the regions', device=torch.cuda.get_device_name(0), cells=cells,
                  losses=[c for c in cells if c['fused_loses_to']])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}: {len(cells)} cells, fused loses in {len(result["losses"])}')


if __name__ == '__main__':
    main()
