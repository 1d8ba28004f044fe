#!/usr/bin/env python3
"""Per-entity completion end to end: the fused route (ranking.complete_entities / gv_entity_topk_scores) against the two routes that
exist without it, alternated in one process:
  per-query  ranking.predict_topk over all (a, r) queries of the entities, --chunk entities at a time, then a torch merge over
             the relations of each entity's R x k answers
  unfused    ranking.complete_entities_unfused: per relation ops.mul + ops.gemm into a (rows, R, N) tensor + torch selection; on the
             all-entities set it runs on the first --unfused-entities entities only and the figure is scaled (both are recorded)
    python tools/entity_profile_bench.py                      # FB15k-237 and WN18RR sizes, h = 200, k = 10 and 100
    python tools/entity_profile_bench.py --shapes fb-h500     # FB15k-237 size with h = 500
    python tools/entity_profile_bench.py --trace-leg          # only the fused all-entities runs, for rocprofv3 --kernel-trace --stats
Query sets: every entity, and a single one.  Each figure is the median of --reps synchronised timed regions after one warm-up of
every route, in milliseconds; the routes' answers are compared (exclude_self is off in all three: predict_topk keeps the loops).
The filter is the synthetic dataset's train + valid + test triplets.  Writes --out (profiles/entity_profile/bench.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcn_vae_amd import data, ranking   # noqa: E402
from entity_bench_common import SHAPES as WIDTH_200, merge_all_queries, same, time_routes   # noqa: E402

SHAPES = {**WIDTH_200, 'fb-h500': ('FB15k-237-synthetic', 500)}


def bench_shape(shape, ks, reps, chunk, unfused_entities, trace_leg):
    name, h = SHAPES[shape]
    kg = data.load_data(name)
    dev = torch.device('cuda')
    n, num_rels = kg.num_nodes, kg.num_rels
    fi = ranking.FilterIndex(n, num_rels, kg.train, kg.valid, kg.test, device=dev)
    gen = torch.Generator().manual_seed(0)
    emb = (torch.randn(n, h, generator=gen) * 0.3).to(dev)
    w = torch.randn(num_rels, h, generator=gen).to(dev)
    kw = dict(side='s', filter_index=fi, flow_log_prob=torch.tensor(0.3, device=dev), exclude_self=False)
    rels = torch.arange(num_rels, device=dev)
    cases = []
    for query, ents in (('all', torch.arange(n, device=dev)), ('single', torch.tensor([n // 2], device=dev))):
        for k in ks:
            m = ents.numel()
            sample = ents[:min(m, unfused_entities)]

            def fused():
                return ranking.complete_entities(emb, w, ents, k, **kw)

            def per_query():
                out = []
                for at in range(0, m, chunk):
                    part = ents[at:at + chunk]
                    ids, logits = ranking.predict_topk(emb, w, part.repeat_interleave(num_rels), rels.repeat(part.numel()), k,
                                                       direction='o', filter_index=fi, flow_log_prob=kw['flow_log_prob'])
                    out.append(merge_all_queries(ids, logits, part.numel(), n, num_rels, k, False))
                return tuple(torch.cat(t) for t in zip(*out))

            def unfused():
                return ranking.complete_entities_unfused(emb, w, sample, k, **kw)

            if trace_leg:
                if query == 'all':
                    for _ in range(3):
                        fused()
                    torch.cuda.synchronize()
                continue
            outs, med = time_routes([('fused', fused), ('per_query', per_query), ('unfused', unfused)], reps)
            case = dict(query=query, entities=m, k=k, fused_ms=med['fused'], per_query_ms=med['per_query'],
                        per_query_over_fused=med['per_query'] / med['fused'], unfused_entities=sample.numel(),
                        unfused_ms_measured=med['unfused'], unfused_ms_scaled=med['unfused'] * m / sample.numel(),
                        unfused_over_fused=med['unfused'] * m / sample.numel() / med['fused'],
                        equal_per_query=same(outs['fused'], outs['per_query']),
                        equal_unfused=same(tuple(t[:sample.numel()] for t in outs['fused']), outs['unfused']))
            print(f"{shape} {query:6s} k={k:3d}: fused {case['fused_ms']:9.2f} ms | per-query + merge {case['per_query_ms']:9.2f} ms "
                  f"({case['per_query_over_fused']:.2f}x) | unfused {case['unfused_ms_scaled']:10.2f} ms ({case['unfused_over_fused']:.2f}x, "
                  f"measured on {case['unfused_entities']} entities) | equal: {case['equal_per_query']} {case['equal_unfused']}", flush=True)
            if not (case['equal_per_query'] and case['equal_unfused']):
                raise SystemExit('the fused route differs from a cross-check route')
            cases.append(case)
    return dict(dataset=name, entities=n, relations=num_rels, h=h, filter_triplets=int(fi.ent['o'].numel()), cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=str, default='fb,wn18rr', help=f'comma list of {sorted(SHAPES)}')
    ap.add_argument('--k', type=str, default='10,100')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=2048, help='entities per predict_topk + merge chunk of the per-query route')
    ap.add_argument('--unfused-entities', type=int, default=256)
    ap.add_argument('--trace-leg', action='store_true')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'entity_profile', 'bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('entity_profile_bench measures on the GPU: no device found')
    ks = [int(x) for x in args.k.split(',')]
    result = {s: bench_shape(s, ks, args.reps, args.chunk, args.unfused_entities, args.trace_leg) for s in args.shapes.split(',')}
    if args.trace_leg:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(dict(unit='ms, median of timed regions ending in a device synchronise', reps=args.reps, shapes=result), f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
