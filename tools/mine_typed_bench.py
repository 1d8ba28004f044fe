#!/usr/bin/env python3
"""Type-constrained whole-graph mining (ranking / transe .mine_triplets(..., type_constraint=): gv_mine_scores_typed,
gv_transe_mine_typed) against the two routes it has to be judged by, alternated in one process:
  typed unfused   .mine_triplets_unfused(..., type_constraint=): per relation, index_select the members, one small GEMM (or
                  transe_queries + transe_distances), torch selection under a running K-th value -- the real competitor
  unconstrained   .mine_triplets(...): the fused sweep over ALL N x R x N triplets (a different, larger answer: the work the
                  constraint removes)
on FB15k-237- and WN18RR-synthetic, h / dim = 200, for DistMult and TransE L1 / L2: K = 100 000 and one threshold run (each
route's threshold is the K-th value of its own top-K list, so a threshold run returns about K triplets).
    python tools/mine_typed_bench.py                       # writes profiles/mine_typed/bench.json
    python tools/mine_typed_bench.py --datasets fb --reps 3
Each figure is the median of --reps synchronised timed regions after one warm-up of every route, the routes taken in turn within
a repetition; end to end, so the typed routes pay for TypeConstraint.members and the unit plan every call.  Sets and filter are
the dataset's train + valid + test triplets.  The two typed routes must agree exactly or the run fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcn_vae_amd import data, ranking, transe   # noqa: E402

DATASETS = {'fb': 'FB15k-237-synthetic', 'wn18rr': 'WN18RR-synthetic'}


def same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
            and a[2]['count'] == b[2]['count'])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def bench(routes, reps):
    """{name: fn} -> ({name: result of the warm-up call}, {name: {'median_ms', 'min_ms', 'ms'}})"""
    results = {name: fn() for name, fn in routes.items()}
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            times[name].append(timed(fn)[1] * 1e3)
    return results, {name: {'median_ms': round(statistics.median(t), 3), 'min_ms': round(min(t), 3), 'ms': [round(x, 3) for x in t]}
                     for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--datasets', type=str, default='fb,wn18rr')
    ap.add_argument('--width', type=int, default=200)
    ap.add_argument('--k', type=int, default=100000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'mine_typed', 'bench.json'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    report = {'device': torch.cuda.get_device_name(0), 'width': args.width, 'k': args.k, 'reps': args.reps,
              'timing': 'median of synchronised wall-clock regions after one warm-up of every route, routes alternated', 'runs': []}
    for key in args.datasets.split(','):
        kg = data.load_data(DATASETS[key])
        n, num_rels = kg.num_nodes, kg.num_rels
        fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
        tc = ranking.TypeConstraint(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
        sizes = tc.sizes.double()
        typed_share = float((sizes[num_rels:] * sizes[:num_rels]).sum() / (num_rels * n * n))
        gen = torch.Generator().manual_seed(0)
        emb = (torch.randn(n, args.width, generator=gen) * 0.3).to(dev)
        w = torch.randn(num_rels, args.width, generator=gen).to(dev)
        rel = (torch.randn(num_rels, args.width, generator=gen) * 0.3).to(dev)
        models = {'distmult': (ranking.mine_triplets, ranking.mine_triplets_unfused, (emb, w))}
        for p in (1, 2):
            models[f'transe-l{p}'] = (transe.mine_triplets, transe.mine_triplets_unfused, ((emb, rel, p, True),))
        for model, (fused, unfused, tables) in models.items():
            sel, plain_sel, last = {'k': args.k}, {'k': args.k}, None
            for kind in ('topk', 'threshold'):
                if kind == 'threshold':                 # each answer's own K-th value, from the top-K runs just made
                    sel = {'threshold': float(last['typed_fused'][1][-1])}
                    plain_sel = {'threshold': float(last['unconstrained_fused'][1][-1])}
                routes = {'typed_fused': lambda s=sel: fused(*tables, filter_index=fi, type_constraint=tc, **s),
                          'typed_unfused': lambda s=sel: unfused(*tables, filter_index=fi, type_constraint=tc, **s),
                          'unconstrained_fused': lambda s=plain_sel: fused(*tables, filter_index=fi, **s)}
                results, times = bench(routes, args.reps)
                if not same(results['typed_fused'], results['typed_unfused']):
                    raise SystemExit(f'{key} {model} {kind}: the typed fused and unfused routes disagree')
                last = results
                f, u, a = (times[r]['median_ms'] for r in ('typed_fused', 'typed_unfused', 'unconstrained_fused'))
                run = {'dataset': DATASETS[key], 'entities': n, 'relations': num_rels, 'type_correct_share': typed_share,
                       'model': model, 'query': kind, 'selection': dict(sel), 'unconstrained_selection': dict(plain_sel),
                       'typed_returned': int(results['typed_fused'][0].shape[0]), 'typed_count': results['typed_fused'][2]['count'],
                       'typed_passes': results['typed_fused'][2]['passes'],
                       'unconstrained_returned': int(results['unconstrained_fused'][0].shape[0]),
                       'fused_equals_unfused': True, 'times': times,
                       'unfused_over_fused': round(u / f, 3), 'unconstrained_over_fused': round(a / f, 3)}
                report['runs'].append(run)
                print(f"{DATASETS[key]:>20} {model:>10} {kind:>9}: typed fused {f:9.2f} ms | typed unfused {u:9.2f} ms "
                      f"({u / f:6.2f}x) | unconstrained fused {a:9.2f} ms ({a / f:6.2f}x)", flush=True)
                os.makedirs(os.path.dirname(args.out), exist_ok=True)
                with open(args.out, 'w') as fh:
                    json.dump(report, fh, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
