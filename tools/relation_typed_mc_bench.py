#!/usr/bin/env python3
"""Relation prediction (s, ?, o) among type-correct relations and on the posterior predictive, at FB15k-237-synthetic and
WN18RR-synthetic size: the pairs of the test split (20 466 / 3 134), filter = the pairs' train + valid + test relations, type sets
from train + valid + test, widths 200 and 500.  Every cell asks for the ranks of the true relation AND the top 10 new relations.

The constraint (DistMult, TransE-L1):
    unconstrained  the fused entry without the sets (ops.pair_relation_scores / ops.transe_pair_relations): NOT the same answer,
                   it shows what the constraint costs;
    fused          one launch with cand = TypeConstraint.relation_words (gv_pair_rel_scores_constrained /
                   gv_transe_pair_rel_constrained);
    composed       the existing constrained kernels with the relation table as the candidates: the gathered rows' product (TransE: a
                   torch subtraction) as a stored query matrix and the pairs' masks rw[s] & rw[N + o] as one set per row, then
                   ops.rank_scores_constrained + ops.topk_scores_constrained (ops.transe_rank_constrained + ops.transe_topk_constrained);
    twin           the materialised cross-check: the (m, R) matrix, TypeConstraint.pair_mask, ranking.mid_ranks / topk_from_scores.

The posterior predictive (DistMult on S in {1, 4, 16} samples, with and without the sets):
    single_x_S     S calls of the single-sample entry, one per sample: S rankings, NOT the same answer;
    fused          one launch of gv_pair_rel_scores_mc{,_constrained} (ops.pair_relation_scores_mc);
    composed       the existing MC kernels on the stacks: ops.mul(z[:, s], z[:, o]) as a stored (S, m, h) query stack against w
                   repeated per sample (made once, outside the timed region), ops.rank_scores_mc{,_constrained} +
                   ops.topk_scores_mc{,_constrained};
    twin           ranking.pair_pbar_unfused (a GEMM, a sigmoid and a running sum per sample), then mid_ranks / topk_from_scores.

Filter ranges and type sets are looked up once, outside the timed regions.  The routes are alternated; each is warmed up once, then
timed over --repeats synchronised regions of --inner calls each, and the median per call is reported in ms.  The fused and composed
answers are asserted equal bit for bit before anything is timed, and so is the twin's where its arithmetic is the kernels' (the MC
twin's sigmoid is torch's, not the device's: the tests hold it to the fused route, not this tool).

    python tools/relation_typed_mc_bench.py [--out profiles/relation_typed_mc/bench.json] [--widths 200,500] [--samples 1,4,16]"""
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


def _same(a, b):
    ranks = all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a[0], b[0]))
    return ranks and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1].view(torch.int32), b[1][1].view(torch.int32))


def _constraint_routes(model, table, rels, s, o, r, filt, tc, p):
    from gcn_vae_amd import ops, ranking, transe
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    rw, n, sets = tc.relation_words('cuda'), table.shape[0], torch.arange(s.numel(), device='cuda')
    if model == 'distmult':
        def fused(cand):
            return ops.pair_relation_scores(table, rels, s, o, target=r, k=K, cand=cand, **names)

        def composed():
            q, rows = ops.mul(table[s].contiguous(), table[o].contiguous()), rw[s] & rw[n + o]
            return ops.rank_scores_constrained(q, rels, r, rows, sets, *filt), ops.topk_scores_constrained(q, rels, K, rows, sets, None, *filt)

        def twin():
            score = ranking.pair_scores_unfused(table, rels, s, o)
            mask = tc.pair_mask(s, o, 'cuda')
            return ranking.relation_ranks_from_scores(score, r, *filt, cand_mask=mask), ranking.topk_from_scores(score, K, *filt, cand=mask)
    else:
        def fused(cand):
            return ops.transe_pair_relations(table, rels, s, o, p, target=r, k=K, cand=cand, **names)

        def composed():
            q, rows = (table[o] - table[s]).contiguous(), rw[s] & rw[n + o]
            return ops.transe_rank_constrained(q, rels, r, p, rows, sets, *filt), ops.transe_topk_constrained(q, rels, K, p, rows, sets, *filt)

        def twin():
            dist = transe.pair_distances_unfused(table, rels, s, o, p)
            mask = tc.pair_mask(s, o, 'cuda')
            return ranking.relation_ranks_from_scores(-dist, r, *filt, cand_mask=mask), transe.topk_from_distances(dist, K, *filt, cand=mask)
    return [('unconstrained', lambda: fused(None)), ('fused', lambda: fused(rw)), ('composed', composed), ('twin', twin)]


def _mc_routes(z, rels, bias, s, o, r, filt, tc):
    from gcn_vae_amd import ops, ranking
    names = dict(zip(('filt_lo', 'filt_hi', 'filt_rel'), filt))
    n_samples, n = z.shape[0], z.shape[1]
    rw = None if tc is None else tc.relation_words('cuda')
    sets, ent = torch.arange(s.numel(), device='cuda'), rels.unsqueeze(0).repeat(n_samples, 1, 1)

    def single():
        return [ops.pair_relation_scores(z[i], rels, s, o, target=r, k=K, bias=bias[i], cand=rw, **names) for i in range(n_samples)][-1]

    def fused():
        return ops.pair_relation_scores_mc(z, rels, s, o, target=r, k=K, bias=bias, cand=rw, **names)[:2]

    def composed():
        q = ops.mul(z[:, s].contiguous(), z[:, o].contiguous())
        if rw is None:
            return ops.rank_scores_mc(q, ent, r, bias, *filt)[:2], ops.topk_scores_mc(q, ent, K, bias, *filt)
        rows = rw[s] & rw[n + o]
        return (ops.rank_scores_mc_constrained(q, ent, r, rows, sets, bias, *filt)[:4],
                ops.topk_scores_mc_constrained(q, ent, K, rows, sets, bias, *filt))

    def twin():
        pbar = ranking.pair_pbar_unfused(z, rels, s, o, bias)
        mask = None if tc is None else tc.pair_mask(s, o, 'cuda')
        return ranking.relation_ranks_from_scores(pbar, r, *filt, cand_mask=mask), ranking.topk_from_scores(pbar, K, *filt, cand=mask)
    return [(f'single_x_{n_samples}', single), ('fused', fused), ('composed', composed), ('twin', twin)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'relation_typed_mc', 'bench.json'))
    ap.add_argument('--widths', default='200,500')
    ap.add_argument('--datasets', default='fb,wn18rr')
    ap.add_argument('--samples', default='1,4,16')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'relation_typed_mc_bench.py measures on the GPU: there is nothing to report without one'
    from gcn_vae_amd import ranking
    from gcn_vae_amd.data import load_data
    cells = []

    def run(routes, same, rivals, **cell):      # same: routes whose answer must equal the fused one's; rivals: whom fused can lose to
        timed = [(nm, (lambda fn=fn: [fn() for _ in range(args.inner)][-1])) for nm, fn in routes]
        outs, ms = time_routes(timed, args.repeats)
        for nm in same:
            assert _same(outs['fused'], outs[nm]), (cell, nm)
        per_call = {nm: round(v / args.inner, 4) for nm, v in ms.items()}
        others = [nm for nm in per_call if nm != 'fused']
        cell.update(ms=per_call, over_fused={nm: round(per_call[nm] / per_call['fused'], 3) for nm in others},
                    fused_loses_to=[nm for nm in others if nm in rivals and per_call[nm] < per_call['fused']])
        cells.append(cell)
        print(json.dumps(cell), flush=True)

    for ds in args.datasets.split(','):
        data = load_data(DATASETS[ds])
        test = torch.as_tensor(np.asarray(data.test), dtype=torch.long).cuda()
        s, r, o = (test[:, i].contiguous() for i in range(3))
        pf = ranking.PairFilterIndex(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
        tc = ranking.TypeConstraint(data.num_nodes, data.num_rels, data.train, data.valid, data.test, device='cuda')
        filt = (*pf.lookup(s, o), pf.relations('cuda'))
        allowed = float(tc.pair_mask(s, o).float().mean())
        for h in (int(x) for x in args.widths.split(',')):
            torch.manual_seed(0)
            ent = (torch.randn(data.num_nodes, h) * 0.3).cuda()
            rel = (torch.randn(data.num_rels, h) * 0.3).cuda()
            common = dict(dataset=DATASETS[ds], pairs=int(s.numel()), num_rels=int(data.num_rels), width=h,
                          type_correct_share=round(allowed, 4))
            for model, p in (('distmult', None), ('transe', 1)):
                run(_constraint_routes(model, ent, rel, s, o, r, filt, tc, p), ('composed', 'twin'), ('composed', 'twin'), part='constraint',
                    model=model if p is None else f'{model}-L{p}', **common)
            for n_samples in (int(x) for x in args.samples.split(',')):
                z = (ent.unsqueeze(0) + 0.1 * torch.randn(n_samples, data.num_nodes, h, device='cuda')).contiguous()
                bias = (0.5 * torch.randn(n_samples)).cuda()
                for typed in (False, True):
                    run(_mc_routes(z, rel, bias, s, o, r, filt, tc if typed else None), ('composed',), (f'single_x_{n_samples}', 'composed', 'twin'),
                        part='mc', model='distmult',
                        samples=n_samples, typed=typed, **common)
                del z
    result = dict(tool='tools/relation_typed_mc_bench.py', k=K, task='ranks (raw + filtered [+ constrained]) and top-10 in one query',
                  repeats=args.repeats, inner_calls_per_region=args.inner, unit='ms per call, median of the regions',
                  device=torch.cuda.get_device_name(0), cells=cells, losses=[c for c in cells if c['fused_loses_to']])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(f'wrote {args.out}: {len(cells)} cells, fused loses somewhere in {len(result["losses"])}')


if __name__ == '__main__':
    main()
